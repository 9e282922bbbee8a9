"""Live-balanced XCD runs of the position-major 3x3 launch (ConvParams::pos_balance, tsm_conv_rules.h::pos_balanced_runs) per
op, through tsm_conv_op in hostile memory (tests/_guard.py), and in the engine under TSM_POISON=1.

The runs only change WHICH workgroup multiplies a tile, so every case asserts the same bits from code 3 (natural order), from
the position-major code with equal-count runs (TSM_POS_BALANCE=0) and from the same code with balanced runs (the default), in
both walk directions; y starts poisoned between poisoned bands, so a tile that no workgroup took stays poison and a workgroup
on a tile past the end breaks a band.  The mapping itself (a bijection, the grid, the balance bound) is checked on the CPU by
tests/test_pos_balance_cpu.py.  That balanced runs really ran is read from the launch trace: the launcher writes the kernel's
own ConvParams::pos_whole and its whole-tile count into the line (" [balanced 1792/1280]"), no bracket with equal-count runs,
and every case compares it with the rule restated below (_balanced_mark) -- a switch that never reached conv_route, or a
wrongly parsed TSM_POS_BALANCE, fails there.  The shapes:

  whole-K   7x7 frames, cout 128 (49 positions x 2 tiles: runs of 10-14 tiles, the grid padded past the tile count), 2x5 frames
            (10 tile groups over 8 runs) and 1x1 frames (ONE tile group: seven runs of length 0, their workgroups all return)
  tail      64 frames of 14x14, cin 128, cout 512: 1 568 tiles, at 256 CUs one round of 1 280 and a tail of 288 tiles in two
            segments -- the pieces follow the PADDED whole part; and the same at stride 2 from 28x28 frames.  Where the tail
            split does not apply on the device's CU count the case is skipped with the reason.
  engine    8 clips at 96x96 with 3 | 0x80 forced, and 16 clips at 224x224 (128 frames: layer2's 3 136 and layer3's 1 568 tiles
            leave a tail at 256 CUs) with 3 | 0x80 | 0x200 forced: the pieces behind the padded whole part in an eager forward
            under TSM_POISON=1, with splitk_reduce_pos_kernel behind them."""
import re

import numpy as np
import pytest
import torch

from tests._conv_ref import conv_ref
from tests._guard import POISON, guarded_conv
from tests._util import assert_walked, make_input
from tests._walk_cases import tail_split_applies
from tests.test_conv_forms_gpu import _bn, _check, _nchw, _nhwc, _w

pytestmark = pytest.mark.gpu

POS, TAILK = 0x80, 0x200
POS_ARM = 'kPrecF32 | kPrecPosMajor, false, true>'
KNOBS = ('TSM_AUTOTUNE', 'TSM_WALK', 'TSM_CONV_TILE', 'TSM_CONV_CODE', 'TSM_TUNE_CACHE', 'TSM_POISON', 'TSM_POS_MAJOR',
         'TSM_POS_BALANCE', 'TSM_FUSE_CONV23')


def _taps(pos, wo, hi, wi, stride):
    oy, ox = divmod(pos, wo)
    return sum(0 <= oy * stride - 1 + ky < hi and 0 <= ox * stride - 1 + kx < wi for ky in range(3) for kx in range(3))


def _balanced_mark(n, hi, wi, stride, cout, tail_cus=None):
    """The trace bracket of a balanced launch, from the rule: 8 contiguous runs of tile groups (ntn tiles of one 64-frame
    group of one position), boundary k where the cumulative live taps come closest to k / 8 of the total (a tie: the later
    one); the whole part of the grid is 8 x the longest run.  tail_cus: the CU count whose tail split applies."""
    ho, wo = (hi - 1) // stride + 1, (wi - 1) // stride + 1
    ntn, per_pos = cout // 64, n // 64
    whole = ho * wo * per_pos * ntn
    if tail_cus is not None:
        whole = whole // (5 * tail_cus) * (5 * tail_cus) // ntn * ntn
    cost = [_taps(g // per_pos, wo, hi, wi, stride) for g in range(whole // ntn)]
    cum = [0]
    for c in cost:
        cum.append(cum[-1] + c)
    bounds = [0] + [min(range(len(cum)), key=lambda g: (abs(8 * cum[g] - k * cum[-1]), -g)) for k in range(1, 8)] + [len(cost)]
    longest = max(b - a for a, b in zip(bounds, bounds[1:])) * ntn
    return f' [balanced {8 * longest}/{whole}]'


def _run_all(monkeypatch, x, w, bn, stride, code, reduces, mark):
    """Code 3, then `code` with equal-count and with balanced runs, each in both directions: the first launch's output after
    asserting that all six are bitwise equal and that the position-major arm ran behind `code`."""
    from workoutdetector_amd.engine import launch_trace
    xd, wd, bnd = _nhwc(x).cuda(), w.cuda(), [b.cuda() for b in bn]
    first = None
    for c, balance in ((3, None), (code, '0'), (code, '1'), (code, None)):
        monkeypatch.delenv('TSM_POS_BALANCE', raising=False)
        if balance is not None:
            monkeypatch.setenv('TSM_POS_BALANCE', balance)
        for rev in (False, True):
            with launch_trace() as tr:
                y = guarded_conv(xd, wd, *bnd, stride=stride, dtype='f32', code=c, reverse=rev, segmented=True)
            y = _nchw(y.cpu())
            assert_walked(tr, rev, f'code {c:#x}')
            igemm = [k for k in tr.kernels if k.startswith('conv_igemm<')]
            assert len(igemm) == 1 and (POS_ARM in igemm[0]) == bool(c & POS), (hex(c), tr.kernels)
            want = mark if c & POS and balance != '0' else ''          # (unset: balanced runs are the default)
            got = igemm[0].replace(' [reverse]', '')
            assert (got.endswith(want) if want else '[balanced' not in got), (hex(c), balance, want, igemm[0])
            n_red = sum(k.startswith('splitk_reduce') for k in tr.kernels)
            assert n_red == (reduces if c & TAILK else 0), (hex(c), tr.kernels)
            if first is None:
                first = y
            else:
                assert torch.equal(y, first), f'code {c:#x}, TSM_POS_BALANCE {balance}, reverse {rev}: differs from code 3'
    return first


WHOLE = [  # id, cin, cout, n, hi, wi
    ('7x7', 128, 128, 64, 7, 7),
    ('2x5', 128, 64, 64, 2, 5),
    ('1x1', 128, 64, 64, 1, 1),
]


@pytest.mark.parametrize('name,cin,cout,n,hi,wi', WHOLE, ids=[c[0] for c in WHOLE])
def test_balanced_whole_k_equals_equal_count_runs_and_natural_order(hip_lib, monkeypatch, name, cin, cout, n, hi, wi):
    g = torch.Generator().manual_seed(4100 + hi * 16 + wi)
    x, w, bn = torch.randn(n, cin, hi, wi, generator=g), _w(cout, cin, 3, g), _bn(cout, g)
    got = _run_all(monkeypatch, x, w, bn, 1, 3 | POS, 0, _balanced_mark(n, hi, wi, 1, cout))
    assert float((got != 0).float().mean()) > 0.2, f'{name}: the output is mostly zeros'
    _check(got.numpy(), conv_ref(x, w, bn, 1, True).numpy(), 'f32', name)


@pytest.mark.parametrize('stride', [1, 2])
def test_balanced_tail_split_equals_equal_count_runs_and_natural_order(hip_lib, monkeypatch, stride):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    if not tail_split_applies(64 * 196, 512, 2, n_cu):
        pytest.skip(f'1 568 tiles leave no tail to split on {n_cu} CUs')
    g = torch.Generator().manual_seed(4200 + stride)
    hw = 14 * stride
    x, w, bn = torch.randn(64, 128, hw, hw, generator=g), _w(512, 128, 3, g), _bn(512, g)
    got = _run_all(monkeypatch, x, w, bn, stride, 3 | POS | TAILK, 1, _balanced_mark(64, hw, hw, stride, 512, n_cu))
    assert float((got != 0).float().mean()) > 0.2


def _engine_marks(frames, size, tail_cus):
    """The 13 position-major launches of a TSM-R50 forward on `frames` frames of size x size, in launch order: (expected
    trace bracket, does the tail split apply) -- conv2 of layer2.0-3, layer3.0-5 and layer4.0-2."""
    out = []
    for blocks, cout, hw in ((4, 128, size // 4), (6, 256, size // 8), (3, 512, size // 16)):
        for b in range(blocks):
            stride, hi = (2, hw) if b == 0 else (1, hw // 2)
            ho = (hi - 1) // stride + 1
            tail = tail_cus is not None and tail_split_applies(frames * ho * ho, cout, 2, tail_cus)
            out.append((_balanced_mark(frames, hi, hi, stride, cout, tail_cus if tail else None), tail))
    return out


ENGINES = [  # id, clips, size, code
    ('96-whole-k', 8, 96, 3 | POS),
    ('224-tail-split', 16, 224, 3 | POS | TAILK),
]


@pytest.mark.parametrize('name,clips,size,code', ENGINES, ids=[e[0] for e in ENGINES])
def test_engine_balanced_is_bitwise_equal_count_under_poison(hip_lib, monkeypatch, sd0, name, clips, size, code):
    """Under TSM_POISON=1 with the position-major code forced: the engine reads TSM_POS_BALANCE at creation, and both settings
    give the logits of code 3 bit for bit with clean guard bands, in both walk directions (the engine alternates them).  The
    trace of the balanced engine carries every launch's bracket as the rule gives it, the equal-count engine's none.
    96x96 x 8 clips (64 frames; layer2 12x12, layer3 6x6, layer4 3x3): whole-K.  224x224 x 16 clips (128 frames) with the
    tail bit: layer2's and layer3's launches split their tail (asserted), the pieces behind the padded whole part."""
    from workoutdetector_amd.engine import TsmEngine, launch_trace
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    marks = _engine_marks(clips * 8, size, n_cu if code & TAILK else None)
    if code & TAILK and not any(t for _, t in marks):
        pytest.skip(f'no 3x3 launch of {clips * 8} frames at {size}x{size} leaves a tail to split on {n_cu} CUs')
    x = make_input(1965, clips, 8, size, size)

    def logits(c, balance):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        env = {'TSM_AUTOTUNE': '0', 'TSM_CONV_CODE': str(c), 'TSM_TUNE_CACHE': 'off', 'TSM_FUSE_CONV23': '0', 'TSM_POISON': '1'}
        if balance is not None:
            env['TSM_POS_BALANCE'] = balance
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng = TsmEngine(height=size, width=size, max_clips=clips, state_dict=sd0)
        try:
            with launch_trace() as tr:
                out = eng.run(None, {'input': x})[0]
        finally:
            eng.close()
        assert np.isfinite(out).all() and not (np.ascontiguousarray(out).view(np.uint32) == POISON).any()
        return out, [k for k in tr.kernels if POS_ARM in k], tr.count('splitk_reduce_pos_kernel')

    natural, none, _ = logits(3, None)
    equal, arm0, red0 = logits(code, '0')
    balanced, arm1, red1 = logits(code, None)
    assert not none and len(arm0) == len(arm1) == 13
    assert not any('[balanced' in k for k in arm0)
    assert [''.join(re.findall(r' \[balanced [0-9/]+\]', k)) for k in arm1] == [m for m, _ in marks], (arm1, marks)
    assert [re.sub(r' \[balanced [0-9/]+\]', '', k) for k in arm1] == arm0          # the same launches but for the bracket
    assert red0 == red1 == sum(t for _, t in marks)
    assert any(k.endswith(' [reverse]') for k in arm1) and any(not k.endswith(' [reverse]') for k in arm1)
    assert np.array_equal(natural, equal) and np.array_equal(natural, balanced)
