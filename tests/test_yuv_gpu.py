"""I420, YV12, P010, YUYV and UYVY frames through the four frame-transform entry points, the staged-video path and StreamBatcher.

The oracle is the existing RGB launch: a launch of a new format must equal the TSM_PIXEL_U8 launch over the upload of
``transform.yuv_to_rgb(frames)`` bit for bit, compared as int32 words (the RGB launch is held to the CPU reference by the
existing preprocess tests, ``yuv_to_rgb`` to ``nv12_to_rgb`` and to the formula by tests/test_yuv_cpu.py).  Every launch runs in
hostile memory (tests/_guard.py).

Inputs are uniformly random bytes in every plane: U != V, neighbouring chroma blocks differ, values outside the nominal range
exercise the clamp, and the low bytes of P010 are random too.  The planes are drawn once per (seed, size) and family -- 4:2:0
(I420, YV12, P010) or 4:2:2 (YUYV, UYVY) -- and every format of a family arranges the SAME planes, so that one RGB launch is the
oracle of the whole family; that the formats of a family convert to the same RGB is asserted where the frames are made.
The shapes are those of tests/test_nv12_gpu.py.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _person_crop as pc
from tests._capture import captured
from tests._guard import POISON, check, guarded, guarded_out
from tests._util import assert_ran

pytestmark = pytest.mark.gpu

FORMATS = ['i420', 'yv12', 'p010', 'yuyv', 'uyvy']
TAG = {'i420': 'I420', 'yv12': 'Yv12', 'p010': 'P010', 'yuyv': 'Yuyv', 'uyvy': 'Uyvy'}       # the kernels' template arguments
LAYOUTS = ['nthwc4', 'ntchw', 'nthwc8s', 'nthwc8b']
NAMES = ['bt601', 'bt709', 'bt601-full', 'bt709-full']
SIZES = [(52, 90), (90, 52), (36, 36)]
CASES = [((52, 90), 36, 32), ((52, 90), 37, 33), ((90, 52), 37, 33), ((36, 36), 36, 32)]      # (frame size, resize, crop)
N_STAGED, TOTAL, N_CLIPS, STEP, STRIDE = 9, 17, 4, 4, 2     # source frames 0, 2, .., 16; clip c, segment k = frame 4 c + 2 k: 18 .. 26 are the tail
INDEX = [[0, 0, 1, 8, 3, -1, 7, 2], [8, 9, 2, 2, 5, 4, -2147483648, 2147483647]]       # repeats, and entries outside the buffer
KERNEL = {'frames': 'preprocess_kernel', 'clips': 'preprocess_clips_kernel', 'indexed': 'preprocess_indexed_kernel',
          'windows': 'preprocess_windows_kernel'}


def _layout(name):
    from workoutdetector_amd import _lib
    return {'nthwc4': _lib.LAYOUT_NTHWC4, 'ntchw': _lib.LAYOUT_NTCHW, 'nthwc8s': _lib.LAYOUT_NTHWC8S, 'nthwc8b': _lib.LAYOUT_NTHWC8B}[name]


def _family(fmt):
    return '422' if fmt in ('yuyv', 'uyvy') else '420'


@functools.lru_cache(maxsize=None)
def _planes(seed, n, h, w, family):
    """Uniformly random Y [n, h, w], U and V [n, ch, w/2] (ch = h/2 for 4:2:0, h for 4:2:2) and P010's low bytes."""
    rng = np.random.default_rng(seed)
    ch = h // 2 if family == '420' else h
    return (rng.integers(0, 256, size=(n, h, w), dtype=np.uint8), rng.integers(0, 256, size=(n, ch, w // 2), dtype=np.uint8),
            rng.integers(0, 256, size=(n, ch, w // 2), dtype=np.uint8), rng.integers(0, 256, size=(n, 3 * h // 2, w), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def _frames(fmt, seed, n, h, w):
    """uint8 frames of a format in its container, arranged from _planes (shared between tests: never written)."""
    y, u, v, low = _planes(seed, n, h, w, _family(fmt))
    if fmt in ('i420', 'yv12'):
        first, second = (u, v) if fmt == 'i420' else (v, u)
        out = np.concatenate([y.reshape(n, -1), first.reshape(n, -1), second.reshape(n, -1)], axis=1).reshape(n, 3 * h // 2, w)
    elif fmt in ('nv12', 'p010'):
        out = np.concatenate([y, np.stack([u, v], axis=-1).reshape(n, h // 2, w)], axis=1)
        if fmt == 'p010':
            out = np.stack([low, out], axis=-1).reshape(n, 3 * h // 2, 2 * w)           # little-endian: (low, high)
    else:
        y2 = y.reshape(n, h, w // 2, 2)
        group = [y2[..., 0], u, y2[..., 1], v] if fmt == 'yuyv' else [u, y2[..., 0], v, y2[..., 1]]
        out = np.stack(group, axis=-1).reshape(n, h, 2 * w)
    return torch.from_numpy(np.ascontiguousarray(out))


@functools.lru_cache(maxsize=None)
def _rgb(family, seed, n, h, w, name):
    """uint8 [n, h, w, 3]: yuv_to_rgb of the family's frames of (seed, n, h, w) -- the same for each of its formats."""
    from workoutdetector_amd.transform import yuv_to_rgb
    fmts = ('i420', 'yv12', 'p010') if family == '420' else ('yuyv', 'uyvy')
    rgbs = [yuv_to_rgb(_frames(f, seed, n, h, w), f, name) for f in fmts]
    assert all(np.array_equal(r, rgbs[0]) for r in rgbs)
    return torch.from_numpy(rgbs[0])


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _boxes(h, w):
    """One box per clip: leaves the frame on all four sides, interior, no person, overhangs the bottom-right corner."""
    return [(-3, -4, h + 7, w + 9), (5, 7, 20, 17), (0, 0, 0, 0), (h - 12, w - 10, 30, 27)]


def _run(entry, frames, h, w, resize, crop, layout, trace=None, **fmt):
    """One entry point on staged frames (a CPU tensor: a format's container with frame_format=, else RGB [n, h, w, 3]) in hostile
    memory -> the output on the CPU.  `trace`: a list that receives the launch's kernel names."""
    from workoutdetector_amd import engine as E
    src = guarded(frames.cuda(), name='frames')
    ops = [src]
    if entry == 'frames':
        out = guarded_out((frames.shape[0],) + E._frame_shape(layout, crop), name='out')
        call = lambda: E.preprocess_frames(src, resize=resize, crop=crop, layout=layout, out=out, **fmt)
    elif entry == 'clips':
        rows = guarded(torch.tensor(_boxes(h, w), dtype=torch.int32).cuda(), name='boxes')
        ops.append(rows)
        out = guarded_out((N_CLIPS, 8) + E._frame_shape(layout, crop), name='out')
        call = lambda: E.preprocess_clips(src, rows, 0, TOTAL, 0, N_CLIPS, size=crop, layout=layout, clip_step=STEP,
                                          clip_stride=STRIDE, out=out, **fmt)
    else:
        index = guarded(torch.tensor(INDEX, dtype=torch.int32).cuda(), name='index')
        ops.append(index)
        out = guarded_out((2, 8) + E._frame_shape(layout, crop), name='out')
        call = lambda: E.preprocess_indexed(src, index, resize=resize, crop=crop, layout=layout, out=out, **fmt)
    with E.launch_trace() as tr:
        assert call() is out
    torch.cuda.synchronize()
    check(out, *ops)
    if trace is not None:
        trace += tr.kernels
    return out.cpu()


@functools.lru_cache(maxsize=None)
def _oracle(entry, family, seed, h, w, resize, crop, layout, name):
    """The U8 launch on the converted frames of a family: computed once, shared by its formats, never written."""
    kernels = []
    want = _run(entry, _rgb(family, seed, N_STAGED, h, w, name), h, w, resize, crop, layout, kernels)
    assert kernels == [KERNEL[entry] + '<unsigned char>'], kernels
    return want


# ---- 1. the oracle is the RGB launch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout_name', LAYOUTS)
@pytest.mark.parametrize('entry', ['frames', 'clips', 'indexed'])
@pytest.mark.parametrize('fmt', FORMATS)
def test_a_launch_equals_the_u8_launch_on_the_converted_frames(hip_lib, fmt, entry, layout_name):
    """tsm_preprocess, _clips (every box kind of _boxes, a padded tail) and _indexed (repeats, entries outside the buffer), each
    colorimetry, each frame size: bit for bit the RGB launch, one launch of the format's instantiation."""
    layout = _layout(layout_name)
    first = None
    for ci, name in enumerate(NAMES):
        for (h, w), resize, crop in CASES:
            seed = 100 * ci + h
            kernels = []
            got = _run(entry, _frames(fmt, seed, N_STAGED, h, w), h, w, resize, crop, layout, kernels, frame_format=fmt, colorimetry=name)
            assert kernels == [f'{KERNEL[entry]}<{TAG[fmt]}>'], kernels
            assert _same_bits(got, _oracle(entry, _family(fmt), seed, h, w, resize, crop, layout, name)), (fmt, entry, layout_name, name, h, w, resize, crop)
        if ci == 0:
            first = got
        elif ci == 1:   # (the colorimetry reaches the kernel: another row gives other bits on the same bytes)
            h, w = SIZES[2]
            other = _run(entry, _frames(fmt, h, N_STAGED, h, w), h, w, 36, 32, layout, frame_format=fmt, colorimetry=name)
            assert not _same_bits(other, first)


def _pack(windows):
    """CPU uint8 windows (any shape) -> (arena, byte offsets), each window at the next multiple of 16 bytes; gaps hold 0xA5."""
    offsets, total = [], 0
    for w in windows:
        offsets.append(total)
        total += (w.numel() + 15) // 16 * 16
    arena = torch.full((total,), 0xA5, dtype=torch.uint8)
    for w, off in zip(windows, offsets):
        arena[off:off + w.numel()] = w.contiguous().view(-1)
    return arena, offsets


def _run_windows(arena, table, n_segment, crop, layout, trace=None, **kw):
    from workoutdetector_amd import engine as E
    src = guarded(arena.cuda(), name='arena')
    rows = guarded(torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).cuda(), name='desc')
    out = guarded_out((len(table), n_segment) + E._frame_shape(layout, crop), name='out')
    with E.launch_trace() as tr:
        assert E.preprocess_windows(src, rows, len(table), n_segment, crop=crop, layout=layout, out=out, **kw) is out
    torch.cuda.synchronize()
    check(src, rows, out)                   # (the guard bands of the arena, the table and the output are clean)
    if trace is not None:
        trace += tr.kernels
    return out.cpu()


@functools.lru_cache(maxsize=None)
def _windows_oracle(family, ci, name, person_crop, resize, crop, layout):
    from workoutdetector_amd.transform import window_descriptors
    shapes = [SIZES[i % 3] for i in range(6)]
    rgb = [_rgb(family, 300 + 10 * ci + i, 2, *s, name) for i, s in enumerate(shapes)]
    arena, offsets = _pack(rgb)
    kernels = []
    want = _run_windows(arena, window_descriptors(shapes, offsets, _window_boxes(shapes, person_crop), resize=resize, crop=crop), 2, crop,
                        layout, kernels, person_crop=person_crop, resize=resize)
    assert kernels == ['preprocess_windows_kernel<unsigned char>'], kernels
    return want


def _window_boxes(shapes, person_crop):
    if not person_crop:
        return None
    boxes = [_boxes(*s)[i % 4] for i, s in enumerate(shapes)]
    return [None if b == (0, 0, 0, 0) else b for b in boxes]


@pytest.mark.parametrize('layout_name', LAYOUTS)
@pytest.mark.parametrize('person_crop', [False, True])
@pytest.mark.parametrize('fmt', FORMATS)
def test_the_windows_launch_equals_the_u8_windows_launch(hip_lib, fmt, person_crop, layout_name):
    """One launch mixing the three frame sizes (two windows each, interleaved, 2 frames per window) with the format's invalid
    descriptors among them -- an odd w; an odd h for 4:2:0; a window that ends one frame row past the arena -- each of which
    yields zero frames and touches nothing else."""
    from workoutdetector_amd.transform import window_descriptors
    layout = _layout(layout_name)
    t = 2
    for ci, name in enumerate(NAMES):
        for resize, crop in ((36, 32), (37, 33)):
            shapes = [SIZES[i % 3] for i in range(6)]
            wins = [_frames(fmt, 300 + 10 * ci + i, t, *s) for i, s in enumerate(shapes)]
            kw = dict(person_crop=person_crop, resize=resize)
            arena, offsets = _pack(wins)
            table = window_descriptors(shapes, offsets, _window_boxes(shapes, person_crop), resize=resize, crop=crop, frame_format=fmt)
            bad = [table[1].copy(), table[5].copy()]
            bad[0][3] += 1                  # 90 x 53: an odd w (the window would still lie in the arena: it is not the last)
            bad[1][2] += 2                  # the last window, two rows taller: it ends past the arena
            if _family(fmt) == '420':
                bad.append(table[1].copy())
                bad[2][2] += 1              # 91 x 52: an odd h
            table = np.concatenate([table[:3], np.stack(bad), table[3:]])
            keep = [0, 1, 2] + [3 + len(bad) + i for i in range(3)]
            kernels = []
            got = _run_windows(arena, table, t, crop, layout, kernels, frame_format=fmt, colorimetry=name, **kw)
            assert kernels == [f'preprocess_windows_kernel<{TAG[fmt]}>'], kernels
            want = _windows_oracle(_family(fmt), ci, name, person_crop, resize, crop, layout)
            assert _same_bits(got[keep], want), (fmt, person_crop, layout_name, name, resize, crop)
            zero = _run_windows(torch.zeros(64, dtype=torch.uint8), np.array([[0, 0, 4, 3, 0, 0, 0, 0]]), t, crop, layout, frame_format=fmt, **kw)
            for i in range(len(bad)):
                assert _same_bits(got[3 + i], zero[0]), (fmt, i)
            assert not _same_bits(got[1], zero[0])
            if layout_name == 'ntchw':
                assert torch.equal(zero[0], pc.ZERO.view(1, 3, 1, 1).expand(t, 3, crop, crop))


# ---- 2. the smallest frames at which a tap source can go wrong ------------------------------------------------------------------
@pytest.mark.parametrize('fmt', FORMATS)
def test_the_smallest_frames_upscaled(hip_lib, fmt):
    """4:2:0: 2 x 2 (one chroma block), 2 x 4 and 4 x 2 (one chroma boundary each way); 4:2:2: 1 x 2 (one pair) and 3 x 4 (an odd
    h, two pairs).  Resized up to 8 so that taps straddle the chroma boundaries; all four entry points, bit for bit the RGB launch."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.transform import window_descriptors
    sizes = [(2, 2), (2, 4), (4, 2)] if _family(fmt) == '420' else [(1, 2), (3, 4)]
    for h, w in sizes:
        for name in ('bt601', 'bt709-full'):
            seed = 500 + 10 * h + w
            src, rgb = _frames(fmt, seed, N_STAGED, h, w), _rgb(_family(fmt), seed, N_STAGED, h, w, name)
            for layout in (_lib.LAYOUT_NTCHW, _lib.LAYOUT_NTHWC8S):
                for entry in ('frames', 'clips', 'indexed'):
                    got = _run(entry, src, h, w, 8, 8, layout, frame_format=fmt, colorimetry=name)
                    assert _same_bits(got, _oracle(entry, _family(fmt), seed, h, w, 8, 8, layout, name)), (fmt, h, w, entry, name, layout)
                arena, offsets = _pack([src[:2], src[2:4]])
                arena_rgb, offsets_rgb = _pack([rgb[:2], rgb[2:4]])
                got = _run_windows(arena, window_descriptors([(h, w)] * 2, offsets, resize=8, crop=8, frame_format=fmt), 2, 8, layout,
                                   resize=8, frame_format=fmt, colorimetry=name)
                want = _run_windows(arena_rgb, window_descriptors([(h, w)] * 2, offsets_rgb, resize=8, crop=8), 2, 8, layout, resize=8)
                assert _same_bits(got, want), (fmt, h, w, name, layout)


def test_a_box_that_leaves_the_frame_on_all_four_sides_is_rgb_zero_outside(hip_lib):
    """The masked taps are RGB 0, not a YUV value: on frames of zero BYTES -- green under every colorimetry -- the corner of a box
    that leaves the frame on all four sides is still (0 - mean) / std, and the centre is not."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import preprocess_clips
    from workoutdetector_amd.transform import frame_container
    h, w, size = 36, 36, 32
    for fmt in FORMATS:
        src = guarded(torch.zeros((8,) + frame_container(h, w, fmt), dtype=torch.uint8).cuda(), name='frames')
        rows = guarded(torch.tensor([[-h, -w, 3 * h, 3 * w]], dtype=torch.int32).cuda(), name='boxes')
        out = guarded_out((1, 8, 3, size, size), name='out')
        preprocess_clips(src, rows, 0, 8, 0, 1, size=size, layout=_lib.LAYOUT_NTCHW, clip_step=8, clip_stride=1, out=out,
                         frame_format=fmt, colorimetry='bt601')
        torch.cuda.synchronize()
        check(src, rows, out)
        got = out.cpu()[0]
        for y, x in ((0, 0), (0, size - 1), (size - 1, 0), (size - 1, size - 1), (3, 16), (16, 3)):
            assert torch.equal(got[:, :, y, x], pc.ZERO.expand(8, 3)), (fmt, y, x)
        centre = ((torch.tensor([0.0, 136.0, 0.0]) - pc.MEAN.view(3)) / pc.STD.view(3)).expand(8, 3)
        assert torch.equal(got[:, 0::2, 16, 16], centre[:, 0::2]), (fmt, got[0, :, 16, 16])
        torch.testing.assert_close(got[:, 1, 16, 16], centre[:, 1], rtol=1e-6, atol=0)


# ---- 3. cross checks that need no oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', ['frames', 'clips', 'indexed'])
def test_the_formats_against_each_other(hip_lib, entry):
    """I420 equals the NV12 launch on the interleaved planes; YV12 on swapped planes equals I420; I420 and YV12 on the SAME bytes
    differ; P010 with random low bytes equals P010 with zero low bytes and the NV12 launch on its high bytes."""
    from workoutdetector_amd import _lib
    (h, w), resize, crop = CASES[1]
    layout, seed, fmt = _lib.LAYOUT_NTHWC8S, 700, dict(colorimetry='bt709')
    i420, yv12, p010, nv12 = (_frames(f, seed, N_STAGED, h, w) for f in ('i420', 'yv12', 'p010', 'nv12'))
    assert not torch.equal(i420, yv12) and torch.equal(p010[:, :, 1::2], nv12)
    kernels = []
    via_nv12 = _run(entry, nv12, h, w, resize, crop, layout, kernels, frame_format='nv12', **fmt)
    assert kernels == [KERNEL[entry] + '<Nv12>'], kernels                 # (an old code still runs its old kernel)
    via_i420 = _run(entry, i420, h, w, resize, crop, layout, frame_format='i420', **fmt)
    assert _same_bits(via_i420, via_nv12)
    assert _same_bits(_run(entry, yv12, h, w, resize, crop, layout, frame_format='yv12', **fmt), via_i420)
    assert not _same_bits(_run(entry, i420, h, w, resize, crop, layout, frame_format='yv12', **fmt), via_i420)
    via_p010 = _run(entry, p010, h, w, resize, crop, layout, frame_format='p010', **fmt)
    assert _same_bits(via_p010, via_nv12)
    clean = p010.clone()
    clean[:, :, 0::2] = 0
    assert not torch.equal(clean, p010) and _same_bits(_run(entry, clean, h, w, resize, crop, layout, frame_format='p010', **fmt), via_p010)
    if entry == 'frames':                                               # a 16-bit tensor is taken as its bytes
        from workoutdetector_amd.engine import preprocess_frames
        words = p010.cuda().view(torch.int16)
        assert tuple(words.shape) == (N_STAGED, 3 * h // 2, w)
        assert _same_bits(preprocess_frames(words, resize=resize, crop=crop, layout=layout, frame_format='p010', **fmt).cpu(), via_p010)
    yuyv, uyvy = _frames('yuyv', seed, N_STAGED, h, w), _frames('uyvy', seed, N_STAGED, h, w)
    via_yuyv = _run(entry, yuyv, h, w, resize, crop, layout, frame_format='yuyv', **fmt)
    assert _same_bits(_run(entry, uyvy, h, w, resize, crop, layout, frame_format='uyvy', **fmt), via_yuyv)
    assert not _same_bits(_run(entry, yuyv, h, w, resize, crop, layout, frame_format='uyvy', **fmt), via_yuyv)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------
def test_odd_sizes_misaligned_bases_and_unknown_codes_are_refused(hip_lib):
    """Odd sizes, a misaligned base for P010 / YUYV / UYVY and the pixel codes 20, 31, 52 and 255: TSM_ERR_INVALID_ARG, the poisoned
    output untouched, nothing launched.  Every new code succeeds and names its kernel."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import _stream, launch_trace
    lib = _lib.load()
    h, w, crop = 36, 36, 32
    src = guarded(_frames('p010', 900, N_STAGED, h, w).cuda(), name='frames')          # (3 h w bytes a frame: enough for every format)
    boxes = guarded(torch.tensor(_boxes(h, w), dtype=torch.int32).cuda(), name='boxes')
    index = guarded(torch.tensor(INDEX, dtype=torch.int32).cuda(), name='index')
    desc = guarded(torch.tensor([[0, 0, h, w, 0, 0, 0, 0]], dtype=torch.int32).cuda(), name='desc')
    out = guarded_out((N_CLIPS, 8, 3, crop, crop), name='out')
    s = _stream(src)
    nchw = _lib.LAYOUT_NTCHW

    def calls(pixel, hh, ww, shift=0):
        base = src.data_ptr() + shift
        return {'preprocess': lambda: lib.tsm_preprocess(base, pixel, N_STAGED, hh, ww, out.data_ptr(), nchw, 36, crop, 0, s),
                'preprocess_clips': lambda: lib.tsm_preprocess_clips(base, pixel, N_STAGED, hh, ww, 0, TOTAL, 0, N_CLIPS, 8, STEP,
                                                                     STRIDE, boxes.data_ptr(), out.data_ptr(), nchw, crop, 0, s),
                'preprocess_indexed': lambda: lib.tsm_preprocess_indexed(base, pixel, N_STAGED, hh, ww, index.data_ptr(), 2, 8,
                                                                         out.data_ptr(), nchw, 36, crop, 0, s),
                'preprocess_windows': lambda: lib.tsm_preprocess_windows(src.data_ptr(), src.numel(), pixel, desc.data_ptr(), 1, 8, 0,
                                                                         out.data_ptr(), nchw, 36, crop, 0, s)}
    with launch_trace() as tr:
        for pixel in (20, 21, 31, 52, 255):
            for op, call in calls(pixel, h, w).items():
                assert call() == -1, (op, pixel)
                assert b'pixel' in lib.tsm_last_error(None)
        for f, fmt in enumerate(FORMATS):
            pixel = 32 + 4 * f + 1
            odd = ((h - 1, w), (h, w - 1), (h - 1, w - 1)) if _family(fmt) == '420' else ((h, w - 1), (h - 1, w - 1))
            for hh, ww in odd:
                for op, call in calls(pixel, hh, ww).items():
                    if op == 'preprocess_windows':
                        continue                            # (a window's size is in its descriptor: the kernel's rule, test 1)
                    assert call() == -1, (op, fmt, hh, ww)
                    msg = lib.tsm_last_error(None).decode()
                    assert op + ':' in msg and 'even' in msg and f'{hh} x {ww}' in msg and fmt.upper() in msg, msg
            if fmt in ('p010', 'yuyv', 'uyvy'):
                for shift in (1, 2, 3):
                    for op, call in calls(pixel, h, w, shift).items():
                        if op != 'preprocess_windows':
                            assert call() == -1, (op, fmt, shift)
                            assert 'aligned' in lib.tsm_last_error(None).decode()
    torch.cuda.synchronize()
    assert tr.kernels == [] and bool((out.view(torch.int32) == POISON).all())
    check(src, boxes, index, desc)
    for f, fmt in enumerate(FORMATS):
        for c in range(4):
            for op, call in calls(32 + 4 * f + c, h - 1 if _family(fmt) == '422' and c == 0 else h, w).items():
                with launch_trace() as tr:
                    assert call() == 0, (op, fmt, c, lib.tsm_last_error(None))
                assert tr.kernels == [f'{op}_kernel<{TAG[fmt]}>'], tr.kernels
    for shift in (1, 3):                                    # the planar formats take any base
        assert lib.tsm_preprocess(src.data_ptr() + shift, 32, 1, h, w, out.data_ptr(), nchw, 36, crop, 0, s) == 0
        assert lib.tsm_preprocess(src.data_ptr() + shift, 36, 1, h, w, out.data_ptr(), nchw, 36, crop, 0, s) == 0
    torch.cuda.synchronize()
    check(src, boxes, index, desc, out)


# ---- 5. capture and replay ----------------------------------------------------------------------------------------------------
def test_an_i420_launch_is_captured_and_replayed(hip_lib, monkeypatch):
    """tests/_capture.py on the I420 form of tsm_preprocess: captured on a side stream, replayed bit-identical to eager."""
    from workoutdetector_amd import engine as E
    monkeypatch.delenv('TSM_POISON', raising=False)
    h, w, resize, crop = 52, 90, 36, 32
    sets = [[_frames('i420', 1200 + k, N_STAGED, h, w)] for k in range(3)]
    frames = guarded(sets[0][0].cuda(), name='frames')
    out = guarded_out((N_STAGED, crop, crop, 4), name='out')
    tr = captured(lambda: E.preprocess_frames(frames, resize=resize, crop=crop, out=out, frame_format='i420', colorimetry='bt709'),
                  [frames], lambda k: sets[k], [out])
    assert_ran(tr, 'preprocess_kernel<I420>', 'preprocess')


# ---- 6. end to end on an engine -------------------------------------------------------------------------------------------------
def _make_engine(sd, dtype, poison):
    from workoutdetector_amd.engine import TsmEngine
    keep = {k: os.environ.get(k) for k in ('TSM_AUTOTUNE', 'TSM_POISON')}
    os.environ['TSM_AUTOTUNE'] = '0'
    os.environ.pop('TSM_POISON', None)
    if poison:
        os.environ['TSM_POISON'] = '1'
    try:
        return TsmEngine(num_class=12, num_segments=8, max_clips=4, state_dict=sd, dtype=dtype)       # (TSM_* are read in tsm_create)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope='module', params=[('f32', False), ('bf16x3', True)], ids=['f32', 'bf16x3-poison'])
def engine(request, hip_lib, sd0):
    """A seeded engine per dtype; the bf16x3 one runs under TSM_POISON=1."""
    eng = _make_engine(sd0, *request.param)
    yield eng
    eng.close()


@pytest.mark.parametrize('fmt', ['i420', 'yuyv'])
def test_video_clip_logits_and_one_stream_step_equal_the_rgb_run_bit_for_bit(engine, fmt):
    """64 x 64 frames, 21 of them: 3 clips, the last two with padded tails (the staged pad is black_frame); then one StreamBatcher
    step over two streams of different sizes.  One launch of the format's kernel per batch and no RGB one."""
    from workoutdetector_amd import inference_count as ic
    from workoutdetector_amd.engine import launch_trace
    from workoutdetector_amd.streaming import StreamBatcher
    from workoutdetector_amd.transform import TestTransform, yuv_to_rgb
    name = 'bt709'
    vid = _frames(fmt, 1000, 21, 64, 64)
    rgb = torch.from_numpy(yuv_to_rgb(vid, fmt, name))
    kernel = f'preprocess_kernel<{TAG[fmt]}>'
    with launch_trace() as tr:
        got = ic.video_clip_logits(engine, vid, TestTransform(), batch_clips=3, video_name='v', frame_format=fmt, colorimetry=name)
    assert tr.ran(kernel) and not tr.ran('preprocess_kernel<unsigned char>') and not tr.ran('preprocess_kernel<float>'), tr.kernels
    want = ic.video_clip_logits(engine, rgb, TestTransform(), batch_clips=3, video_name='v')
    assert tuple(got.shape) == (3, 12) and bool(torch.isfinite(got).all())
    assert _same_bits(got, want), (fmt, float((got - want).abs().max()))

    vids = {'a': _frames(fmt, 1100, 8, 64, 64), 'b': _frames(fmt, 1101, 8, 48, 80)}
    got = StreamBatcher(engine, threshold=0.0, max_batch=4, frame_format=fmt, colorimetry=name)
    want = StreamBatcher(engine, threshold=0.0, max_batch=4)
    with launch_trace() as tr:
        for t in range(8):
            for k, v in vids.items():
                got.push(k, v[t].numpy())
        ev_got = got.step()
    assert tr.count(f'preprocess_windows_kernel<{TAG[fmt]}>') == 1 and tr.count('preprocess_windows_kernel') == 1, tr.kernels
    for t in range(8):
        for k, v in vids.items():
            want.push(k, yuv_to_rgb(v[t].numpy(), fmt, name)[0])
    ev_want = want.step()
    assert ev_got == ev_want and {k: len(e) for k, e in ev_got.items()} == {'a': 1, 'b': 1}
    assert all(got.result(k) == want.result(k) for k in vids)
    for k in vids:
        got.close(k)
        want.close(k)
