"""Hostile memory around and under a kernel's operands (DESIGN: the hostile-memory rule).

A kernel that never writes its last tile, or reads one row before frame 0, passes every value comparison as long as the
memory it leaves alone or strays into holds plausible numbers: torch's caching allocator hands the next same-sized
``torch.empty`` the block the previous run just freed, correct answer included.  So the per-op tests give a kernel

* operands that are views into a larger allocation with a band of ``POISON`` on each side (``guarded``), and
* outputs that are such views with the payload poisoned too (``guarded_out``),

and call ``check`` after every launch: every band still holds its fill bit for bit (no stray store), and no word of an
output still holds ``POISON`` (every element was written).  A stray *read* is not flagged here: it lands in owned memory
and returns poison, which the test's own value comparison then sees as a wrong result instead of a right one by luck.

``POISON`` = 0x7FC07FC0: as fp32 a quiet NaN with a payload arithmetic never produces, as two bf16 two quiet NaNs (so it is
hostile in the fp32, the split [hi x8 | lo x8] and the bf16 layouts alike), as an int32 state no class id.  The conv
epilogues are ``fmaxf(v, floor)``, which drops a NaN: a poisoned operand surfaces as 0 (ReLU) or -inf, not as NaN, so the
detector is always the value comparison, never "is the output finite".  A max-pool absorbs NaN and -inf: its input bands
are +inf (``fill=float('inf')``).

Scope.  The kernel sees these tensors directly for float32 operands and outputs.  For the bf16 formats ``tsm_conv_op`` converts
into staging buffers of its own and launches on those: they are poisoned and banded by the library itself (same word, same
band rule; a broken band fails the call with TSM_ERR_GUARD), and what the launch leaves unwritten in them reaches ``y`` as
poison through the conversion back.  The payload check compares 32-bit words: every output here has 4-byte elements (float32,
int32); for a 2-byte output a single unwritten element next to a written one would not equal the word and would go unseen.
"""
import struct

import torch

POISON = 0x7FC07FC0
ALIGN = 512            # the view keeps the alignment torch's CUDA allocator gives a tensor of its own
MIN_BAND = 4096


class GuardError(AssertionError):
    """A guard band or an output payload failed.  ``tensor`` is the name given to guarded() / guarded_out(); ``side`` is
    'before', 'after' or 'payload'; ``offset`` the first offending element relative to the payload's first element (negative
    in the band before it, >= numel in the band after it), ``byte_offset`` the same in bytes."""

    def __init__(self, msg, tensor, side, offset, byte_offset):
        super().__init__(msg)
        self.tensor, self.side, self.offset, self.byte_offset = tensor, side, offset, byte_offset


def fill_word(fill):
    """The int32 word (signed, as torch stores it) of a fill given as a bit pattern (int) or a float value."""
    u = struct.unpack('<I', struct.pack('<f', fill))[0] if isinstance(fill, float) else int(fill) & 0xFFFFFFFF
    return u - (1 << 32) if u >= 1 << 31 else u


def band_bytes(shape, itemsize):
    """One whole frame of the tensor (the reach of a wrong temporal-shift or halo index) rounded up to 512 bytes, at
    least 4 KiB."""
    frame = itemsize
    for d in tuple(shape)[1:]:
        frame *= int(d)
    return max(MIN_BAND, -(-frame // ALIGN) * ALIGN)


class _Guard:
    __slots__ = ('base', 'lead', 'nbytes', 'word', 'name', 'is_out', 'shape', 'itemsize')


def _make(shape, dtype, device, fill, name, is_out):
    shape = tuple(int(d) for d in shape)
    itemsize = torch.empty((), dtype=dtype).element_size()
    numel = 1
    for d in shape:
        numel *= d
    g = _Guard()
    g.lead = band_bytes(shape, itemsize)
    g.nbytes = numel * itemsize
    g.word, g.name, g.is_out, g.shape, g.itemsize = fill_word(fill), name, is_out, shape, itemsize
    total = g.lead + -(-g.nbytes // ALIGN) * ALIGN + g.lead       # (the slack up to 512 bytes belongs to the band after)
    words = torch.full((total // 4,), g.word, dtype=torch.int32, device=device)
    if is_out and g.word != POISON:                               # an output's payload is POISON whatever its bands hold
        words[g.lead // 4: (g.lead + g.nbytes) // 4] = POISON
    g.base = words.view(torch.uint8)
    view = g.base[g.lead: g.lead + g.nbytes].view(dtype).view(shape)
    if view.is_cuda:
        assert view.data_ptr() % ALIGN == 0, f'{name}: guarded view lost its {ALIGN}-byte alignment'
    view._guard = g
    return view


def guarded(t, fill=POISON, name='operand'):
    """A copy of `t` that is a view into a larger allocation, a band filled with `fill` on each side."""
    t = t.contiguous()
    view = _make(t.shape, t.dtype, t.device, fill, name, False)
    view.copy_(t)
    return view


def guarded_repeat(small, reps, fill=POISON, name='operand'):
    """guarded(small.repeat(reps, 1, ...)), the periods written into the guarded view itself: a multi-GiB periodic operand
    (tests/_big_cases.py) exists once, not as a tensor and its guarded copy."""
    small = small.contiguous()
    view = _make((small.shape[0] * reps,) + tuple(small.shape[1:]), small.dtype, small.device, fill, name, False)
    g = view._guard
    g.base[g.lead: g.lead + g.nbytes].view(small.dtype).view(reps, -1).copy_(small.reshape(1, -1).expand(reps, -1))
    return view


def guarded_out(shape, dtype=torch.float32, device='cuda', fill=POISON, name='out'):
    """An output between two bands, the payload poisoned too: whatever the kernel does not write stays POISON."""
    return _make(shape, dtype, device, fill, name, True)


def where(offset, shape):
    """Element offset (relative to the payload's first element; any sign) as frames / rows / channels of `shape`."""
    names = {5: ('clip', 'frame', 'row', 'col', 'channel'), 4: ('frame', 'row', 'col', 'channel'), 3: ('frame', 'row', 'channel'),
             2: ('row', 'col'), 1: ('element',)}.get(len(shape), tuple(f'dim{i}' for i in range(len(shape))))
    idx = []
    for d in reversed(shape[1:]):
        offset, r = divmod(offset, d)      # (floor division: the element before frame 0 is the last one of frame -1)
        idx.append(r)
    idx.append(offset)
    return ', '.join(f'{n} {i}' for n, i in zip(names, reversed(idx)))


def _first_bad(bad):
    return int(torch.nonzero(bad.reshape(-1))[0])


def _check_one(view):
    g = getattr(view, '_guard', None)
    assert g is not None, 'check() takes tensors made by guarded() / guarded_out()'
    end = g.lead + g.nbytes
    end4 = (end + 3) // 4 * 4
    pattern = torch.tensor([g.word], dtype=torch.int32, device=g.base.device).view(torch.uint8)
    bands = (('before', 0, g.base[:g.lead].view(torch.int32)),
             ('after', end, g.base[end:end4] if end4 > end else None),          # (the odd bytes behind a payload of bytes)
             ('after', end4, g.base[end4:].view(torch.int32)))
    for side, start, band in bands:
        if band is None:
            continue
        bad = band != (g.word if band.dtype == torch.int32 else pattern[end % 4:])
        if bool(bad.any()):
            at = start + _first_bad(bad) * band.element_size()     # byte offset in the allocation
            rel = at - g.lead                                      # ... relative to the payload's first byte
            elem = rel // g.itemsize
            got = int(g.base[at // 4 * 4: at // 4 * 4 + 4].view(torch.int32).item()) & 0xFFFFFFFF
            dist = f'{-rel} bytes before its start' if rel < 0 else f'{rel - g.nbytes} bytes past its end'
            raise GuardError(f'{g.name}: stray store into the band {side} the tensor, {dist}: element offset {elem} = '
                             f'{where(elem, g.shape)} of shape {g.shape}; the word there is {got:#010x}, the fill '
                             f'{g.word & 0xFFFFFFFF:#010x}', g.name, side, elem, rel)
    if g.is_out and g.nbytes >= 4:
        bad = g.base[g.lead: g.lead + g.nbytes // 4 * 4].view(torch.int32) == POISON
        if bool(bad.any()):
            rel = _first_bad(bad) * 4
            elem = rel // g.itemsize
            raise GuardError(f'{g.name}: {int(bad.sum())} payload word(s) still hold the poison {POISON:#010x}: never written.  '
                             f'First at element offset {elem} = {where(elem, g.shape)} of shape {g.shape}',
                             g.name, 'payload', elem, rel)


def check(*tensors):
    """(a) both bands of every tensor bit-identical to their fill, compared as int32: no stray store, into an output's
    surroundings or an operand's; (b) no payload word of an output still equals POISON: every element was written.
    Raises GuardError naming the tensor, the side and the first offending offset in frames / rows / channels."""
    for t in tensors:
        if t is not None:
            _check_one(t)


def guarded_conv(x, w, gamma, beta, mean, var, *, residual=None, x2=None, w2=None, bn2=None, stride=1, segmented=False, **kw):
    """engine.conv_bn_act_nhwc between guards: every operand (the second source, the weights and the BatchNorm vectors
    included) goes in as guarded(), the output as guarded_out(), and check() runs after the call.  Same arguments (CUDA
    tensors), same result."""
    from workoutdetector_amd.engine import conv_bn_act_nhwc
    k = w.shape[2]
    n, hi, wi, _ = x.shape
    ho, wo = (hi + 2 * (k // 2) - k) // stride + 1, (wi + 2 * (k // 2) - k) // stride + 1
    ops = {'x': x, 'w': w, 'gamma': gamma, 'beta': beta, 'mean': mean, 'var': var, 'residual': residual, 'x2': x2, 'w2': w2}
    ops = {name: None if t is None else guarded(t, name=name) for name, t in ops.items()}
    gbn2 = None if bn2 is None else [guarded(t, name=f'bn2[{i}]') for i, t in enumerate(bn2)]
    y = guarded_out((n, ho, wo, w.shape[0]), torch.float32, x.device, name='y')
    got = conv_bn_act_nhwc(ops['x'], ops['w'], ops['gamma'], ops['beta'], ops['mean'], ops['var'], stride=stride,
                           residual=ops['residual'], x2=ops['x2'], w2=ops['w2'], bn2=gbn2, out=y, segmented=segmented, **kw)
    assert got is y
    torch.cuda.synchronize()
    check(y, *ops.values(), *(gbn2 or ()))
    return y
