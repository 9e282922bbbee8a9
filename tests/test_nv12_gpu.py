"""NV12 frames through the four frame-transform entry points, the staged-video path and StreamBatcher.

The oracle is the existing RGB launch: the NV12 launch must equal the TSM_PIXEL_U8 launch over the upload of
``transform.nv12_to_rgb(frames)`` bit for bit (the RGB launch is held to the CPU reference by the existing preprocess tests,
``nv12_to_rgb`` to the float64 matrices by tests/test_nv12_cpu.py).  Every launch runs in hostile memory (tests/_guard.py).

Inputs are uniformly random bytes in all three planes: neighbouring 2x2 blocks differ, and values outside the nominal range
exercise the clamp.  Frames are 52 x 90, 90 x 52 and 36 x 36 (which resizes exactly), 9 staged frames, 4 clips of 8 segments
with a padded tail, (resize, crop) = (36, 32) and (37, 33) -- the latter a half-filled pixel pair in the bf16 layouts: the
shapes of the existing preprocess tests.
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

LAYOUTS = ['nthwc4', 'ntchw', 'nthwc8s', 'nthwc8b']
NAMES = ['bt601', 'bt709', 'bt601-full', 'bt709-full']
SIZES = [(52, 90), (90, 52), (36, 36)]
CASES = [((52, 90), 36, 32), ((52, 90), 37, 33), ((90, 52), 37, 33), ((36, 36), 36, 32)]      # (frame size, resize, crop)
N_STAGED, TOTAL, N_CLIPS, STEP, STRIDE = 9, 17, 4, 4, 2     # source frames 0, 2, .., 16; clip c, segment k = frame 4 c + 2 k: 18 .. 26 are the tail


def _layout(name):
    from workoutdetector_amd import _lib
    return {'nthwc4': _lib.LAYOUT_NTHWC4, 'ntchw': _lib.LAYOUT_NTCHW, 'nthwc8s': _lib.LAYOUT_NTHWC8S, 'nthwc8b': _lib.LAYOUT_NTHWC8B}[name]


@functools.lru_cache(maxsize=None)
def _nv12(seed, n, h, w):
    """uint8 [n, 3h/2, w]: uniformly random bytes in all three planes (shared between tests: never written)."""
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(n, 3 * h // 2, w), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def _rgb(seed, n, h, w, name):
    """uint8 [n, h, w, 3]: nv12_to_rgb of _nv12(seed, n, h, w), once."""
    from workoutdetector_amd.transform import nv12_to_rgb
    return torch.from_numpy(nv12_to_rgb(_nv12(seed, n, h, w), name))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _boxes(h, w):
    """One box per clip: leaves the frame on all four sides, interior, no person, overhangs the bottom-right corner."""
    return [(-3, -4, h + 7, w + 9), (5, 7, 20, 17), (0, 0, 0, 0), (h - 12, w - 10, 30, 27)]


INDEX = [[0, 0, 1, 8, 3, -1, 7, 2], [8, 9, 2, 2, 5, 4, -2147483648, 2147483647]]       # repeats, and entries outside the buffer


def _run(entry, frames, h, w, resize, crop, layout, trace=None, **fmt):
    """One entry point on staged frames (CPU tensor: NV12 [n, 3h/2, w] with frame_format='nv12', else RGB [n, h, w, 3]) in
    hostile memory -> the output on the CPU.  `trace`: a list that receives the launch's kernel names."""
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


KERNEL = {'frames': 'preprocess_kernel', 'clips': 'preprocess_clips_kernel', 'indexed': 'preprocess_indexed_kernel',
          'windows': 'preprocess_windows_kernel'}


# ---- 1. the oracle is the RGB launch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout_name', LAYOUTS)
@pytest.mark.parametrize('entry', ['frames', 'clips', 'indexed'])
def test_the_nv12_launch_equals_the_u8_launch_on_the_converted_frames(hip_lib, entry, layout_name):
    """tsm_preprocess, _clips (every box kind of _boxes, a padded tail) and _indexed (repeats, entries outside the buffer), each
    colorimetry, each frame size: bit for bit the RGB launch, one launch of the <Nv12> instantiation."""
    layout = _layout(layout_name)
    for ci, name in enumerate(NAMES):
        outs = []
        for (h, w), resize, crop in CASES:
            seed = 100 * ci + h
            kernels = []
            got = _run(entry, _nv12(seed, N_STAGED, h, w), h, w, resize, crop, layout, kernels, frame_format='nv12', colorimetry=name)
            assert kernels == [KERNEL[entry] + '<Nv12>'], kernels
            kernels = []
            want = _run(entry, _rgb(seed, N_STAGED, h, w, name), h, w, resize, crop, layout, kernels)
            assert kernels == [KERNEL[entry] + '<unsigned char>'], kernels
            assert _same_bits(got, want), (entry, layout_name, name, h, w, resize, crop)
            outs.append(got)
        if ci:      # (the colorimetry reaches the kernel: another row gives other bits on the same bytes)
            h, w = SIZES[0]
            other = _run(entry, _nv12(100 * ci + h, N_STAGED, h, w), h, w, 36, 32, layout, frame_format='nv12', colorimetry=NAMES[0])
            assert not _same_bits(other, outs[0])


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
    check(src, rows, out)
    if trace is not None:
        trace += tr.kernels
    return out.cpu()


@pytest.mark.parametrize('layout_name', LAYOUTS)
@pytest.mark.parametrize('person_crop', [False, True])
def test_the_nv12_windows_launch_equals_the_u8_windows_launch(hip_lib, person_crop, layout_name):
    """One launch mixing the three frame sizes (two windows each, interleaved, 2 frames per window) with one invalid descriptor
    among them -- an odd height, of a window that still lies in the arena -- which yields zero frames and touches nothing else."""
    from workoutdetector_amd.transform import window_descriptors
    layout = _layout(layout_name)
    t = 2
    for ci, name in enumerate(NAMES):
        for resize, crop in ((36, 32), (37, 33)):
            shapes = [SIZES[i % 3] for i in range(6)]
            nv, rgb = [_nv12(300 + 10 * ci + i, t, *s) for i, s in enumerate(shapes)], [_rgb(300 + 10 * ci + i, t, *s, name) for i, s in enumerate(shapes)]
            boxes = [_boxes(*s)[i % 4] for i, s in enumerate(shapes)] if person_crop else None
            boxes = None if boxes is None else [None if b == (0, 0, 0, 0) else b for b in boxes]
            kw = dict(person_crop=person_crop, resize=resize)
            arena, offsets = _pack(nv)
            table = window_descriptors(shapes, offsets, boxes, resize=resize, crop=crop, frame_format='nv12')
            bad = table[1].copy()
            bad[2] += 1                     # 91 x 52: an odd height (the window would still lie in the arena)
            table = np.concatenate([table[:3], bad[None], table[3:]])
            kernels = []
            got = _run_windows(arena, table, t, crop, layout, kernels, frame_format='nv12', colorimetry=name, **kw)
            assert kernels == ['preprocess_windows_kernel<Nv12>'], kernels
            arena_rgb, offsets_rgb = _pack(rgb)
            kernels = []
            want = _run_windows(arena_rgb, window_descriptors(shapes, offsets_rgb, boxes, resize=resize, crop=crop), t, crop, layout, kernels, **kw)
            assert kernels == ['preprocess_windows_kernel<unsigned char>'], kernels
            assert _same_bits(got[[0, 1, 2, 4, 5, 6]], want), (person_crop, layout_name, name, resize, crop)
            zero = _run_windows(torch.zeros(64, dtype=torch.uint8), np.array([[0, 0, 3, 4, 0, 0, 0, 0]]), t, crop, layout, frame_format='nv12', **kw)
            assert _same_bits(got[3], zero[0]) and not _same_bits(got[1], zero[0])
            if layout_name == 'ntchw':
                assert torch.equal(zero[0], pc.ZERO.view(1, 3, 1, 1).expand(t, 3, crop, crop))


# ---- 2. seams the equality alone could miss -----------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', [(2, 2), (2, 40)])
def test_tiny_frames_where_every_tap_clamps_to_the_border(hip_lib, h, w):
    """A 2 x 2 frame and a 2-row frame resized up (resize 36: 36 x 36 and 36 x 720), all four entry points: bit for bit the RGB
    launch; the 2 x 2 frame is one chroma block, so its four pixels differ in luma only."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.transform import window_descriptors
    for name in ('bt601', 'bt709-full'):
        nv, rgb = _nv12(500 + w, N_STAGED, h, w), _rgb(500 + w, N_STAGED, h, w, name)
        for layout in (_lib.LAYOUT_NTCHW, _lib.LAYOUT_NTHWC8S):
            for entry in ('frames', 'clips', 'indexed'):
                got = _run(entry, nv, h, w, 36, 33, layout, frame_format='nv12', colorimetry=name)
                assert _same_bits(got, _run(entry, rgb, h, w, 36, 33, layout)), (entry, name, layout)
            arena, offsets = _pack([nv[:2], nv[2:4]])
            arena_rgb, offsets_rgb = _pack([rgb[:2], rgb[2:4]])
            got = _run_windows(arena, window_descriptors([(h, w)] * 2, offsets, resize=36, crop=33, frame_format='nv12'), 2, 33, layout,
                               resize=36, frame_format='nv12', colorimetry=name)
            want = _run_windows(arena_rgb, window_descriptors([(h, w)] * 2, offsets_rgb, resize=36, crop=33), 2, 33, layout, resize=36)
            assert _same_bits(got, want), (name, layout)


def test_a_box_that_leaves_the_frame_on_all_four_sides_is_rgb_zero_outside(hip_lib):
    """The masked taps are RGB 0, not a YUV value: on a frame of zero BYTES -- green under every colorimetry -- the corner of a
    box that leaves the frame on all four sides is still (0 - mean) / std, and the centre is the green's normalised value."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import preprocess_clips
    h, w, size = 36, 36, 32
    green = {'bt601': 136.0, 'bt709': 77.0, 'bt601-full': 135.0, 'bt709-full': 84.0}
    for name in NAMES:
        src = guarded(torch.zeros((8, 3 * h // 2, w), dtype=torch.uint8).cuda(), name='frames')
        rows = guarded(torch.tensor([[-h, -w, 3 * h, 3 * w]], dtype=torch.int32).cuda(), name='boxes')
        out = guarded_out((1, 8, 3, size, size), name='out')
        preprocess_clips(src, rows, 0, 8, 0, 1, size=size, layout=_lib.LAYOUT_NTCHW, clip_step=8, clip_stride=1, out=out,
                         frame_format='nv12', colorimetry=name)
        torch.cuda.synchronize()
        check(src, rows, out)
        got = out.cpu()[0]
        for y, x in ((0, 0), (0, size - 1), (size - 1, 0), (size - 1, size - 1), (3, 16), (16, 3)):
            assert torch.equal(got[:, :, y, x], pc.ZERO.expand(8, 3)), (name, y, x)
        # (R and B are bilinear sums of exact zeros; G sums four equal taps with weights that add up to 1 only up to rounding)
        centre = ((torch.tensor([0.0, green[name], 0.0]) - pc.MEAN.view(3)) / pc.STD.view(3)).expand(8, 3)
        assert torch.equal(got[:, 0::2, 16, 16], centre[:, 0::2]), (name, got[0, :, 16, 16])
        torch.testing.assert_close(got[:, 1, 16, 16], centre[:, 1], rtol=1e-6, atol=0)


def test_each_frame_reads_its_own_chroma_plane(hip_lib):
    """Two frames of equal luma whose chroma planes are constant 0 and constant 255: a kernel that reads frame 1's chroma from
    frame 0's offset (or strides frames by h * w) cannot pass.  All four entry points against the RGB launch, and the two frames
    of the output differ."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.transform import nv12_to_rgb, window_descriptors
    h, w = 52, 90
    luma = _nv12(700, 1, h, w)[0, :h]
    nv = torch.empty((N_STAGED, 3 * h // 2, w), dtype=torch.uint8)
    nv[:, :h] = luma
    for j in range(N_STAGED):
        nv[j, h:] = 0 if j % 2 == 0 else 255
    rgb = torch.from_numpy(nv12_to_rgb(nv, 'bt601'))
    layout = _lib.LAYOUT_NTCHW
    for entry, odd_row in (('frames', 1), ('clips', 1), ('indexed', 2)):          # (output row 0 shows frame 0, `odd_row` frame 1)
        got = _run(entry, nv, h, w, 36, 32, layout, frame_format='nv12', colorimetry='bt601')
        assert _same_bits(got, _run(entry, rgb, h, w, 36, 32, layout)), entry
        flat = got.reshape((-1,) + tuple(got.shape[-3:]))
        assert not _same_bits(flat[0], flat[odd_row]), entry
    assert _same_bits(flat[0], flat[1]) and _same_bits(flat[2], flat[6])        # (INDEX[0] = 0, 0, 1, 8, 3, -1, 7, 2: rows 2 and 6 show odd frames)
    arena, offsets = _pack([nv[:2], nv[1:3]])
    arena_rgb, offsets_rgb = _pack([rgb[:2], rgb[1:3]])
    got = _run_windows(arena, window_descriptors([(h, w)] * 2, offsets, resize=36, crop=32, frame_format='nv12'), 2, 32, layout,
                       resize=36, frame_format='nv12', colorimetry='bt601')
    want = _run_windows(arena_rgb, window_descriptors([(h, w)] * 2, offsets_rgb, resize=36, crop=32), 2, 32, layout, resize=36)
    assert _same_bits(got, want) and _same_bits(got[0, 1], got[1, 0]) and not _same_bits(got[0, 0], got[0, 1])


def test_a_clip_whose_tail_reads_the_pad(hip_lib):
    """tsm_gather_clips behind the NV12 tsm_preprocess, the staged-video path's pair: the pad frame behind the staged frames is
    nv12_black, so a tail segment is the normalised zero frame to the bit, as the RGB path's zero-byte pad frame gives it; a pad
    of zero bytes would not."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import gather_clips, preprocess_frames
    from workoutdetector_amd.transform import nv12_black
    h, w = 52, 90
    for name in ('bt601', 'bt709-full'):
        nv = torch.cat([_nv12(800, N_STAGED, h, w), torch.from_numpy(nv12_black(h, w, name))[None]])
        frames = preprocess_frames(nv.cuda(), resize=36, crop=32, layout=_lib.LAYOUT_NTCHW, frame_format='nv12', colorimetry=name)
        clips = gather_clips(frames, 0, TOTAL, 0, N_CLIPS, n_segment=8, clip_step=STEP, clip_stride=STRIDE).cpu()
        zero = pc.ZERO.view(3, 1, 1).expand(3, 32, 32)
        assert torch.equal(clips[1, 7], zero) and torch.equal(clips[3, 3], zero) and not torch.equal(clips[1, 6], zero)
        nv[-1] = 0
        frames = preprocess_frames(nv.cuda(), resize=36, crop=32, layout=_lib.LAYOUT_NTCHW, frame_format='nv12', colorimetry=name)
        assert not torch.equal(frames[-1].cpu(), zero)


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------
def test_odd_sizes_and_unknown_pixel_codes_are_refused_and_pixel_16_succeeds(hip_lib):
    """Odd h, odd w and pixel codes 2, 15 and 20: TSM_ERR_INVALID_ARG, the poisoned output untouched, nothing launched.  Pixel
    16 succeeds (the library before NV12 answered TSM_ERR_INVALID_ARG)."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import _stream, launch_trace
    lib = _lib.load()
    h, w, crop = 36, 36, 32
    src = guarded(_nv12(900, N_STAGED, h, w).cuda(), name='frames')
    boxes = guarded(torch.tensor(_boxes(h, w), dtype=torch.int32).cuda(), name='boxes')
    index = guarded(torch.tensor(INDEX, dtype=torch.int32).cuda(), name='index')
    desc = guarded(torch.tensor([[0, 0, h, w, 0, 0, 0, 0]], dtype=torch.int32).cuda(), name='desc')
    out = guarded_out((N_CLIPS, 8, 3, crop, crop), name='out')
    s = _stream(src)
    nchw = _lib.LAYOUT_NTCHW

    def calls(pixel, hh, ww):
        return {'preprocess': lambda: lib.tsm_preprocess(src.data_ptr(), pixel, N_STAGED, hh, ww, out.data_ptr(), nchw, 36, crop, 0, s),
                'preprocess_clips': lambda: lib.tsm_preprocess_clips(src.data_ptr(), pixel, N_STAGED, hh, ww, 0, TOTAL, 0, N_CLIPS, 8, STEP,
                                                                     STRIDE, boxes.data_ptr(), out.data_ptr(), nchw, crop, 0, s),
                'preprocess_indexed': lambda: lib.tsm_preprocess_indexed(src.data_ptr(), pixel, N_STAGED, hh, ww, index.data_ptr(), 2, 8,
                                                                         out.data_ptr(), nchw, 36, crop, 0, s),
                'preprocess_windows': lambda: lib.tsm_preprocess_windows(src.data_ptr(), src.numel(), pixel, desc.data_ptr(), 1, 8, 0,
                                                                         out.data_ptr(), nchw, 36, crop, 0, s)}
    with launch_trace() as tr:
        for pixel in (2, 15, 20, -1):
            for op, call in calls(pixel, h, w).items():
                assert call() == -1, (op, pixel)
                assert b'pixel' in lib.tsm_last_error(None)
        for hh, ww in ((h - 1, w), (h, w - 1), (h - 1, w - 1)):
            for op, call in calls(_lib.PIXEL_NV12_BT601, hh, ww).items():
                if op == 'preprocess_windows':
                    continue                                # (a window's size is in its descriptor: the kernel's rule, test 1)
                assert call() == -1, (op, hh, ww)
                msg = lib.tsm_last_error(None).decode()
                assert op + ':' in msg and 'even' in msg and f'{hh} x {ww}' in msg, msg
        assert lib.tsm_preprocess(src.data_ptr() + 1, 16, 1, h, w, out.data_ptr(), nchw, 36, crop, 0, s) == -1      # a chroma pair is one 2-byte load
    torch.cuda.synchronize()
    assert tr.kernels == [] and bool((out.view(torch.int32) == POISON).all())
    check(src, boxes, index, desc)
    for pixel in (16, 17, 18, 19):
        for op, call in calls(pixel, h, w).items():
            with launch_trace() as tr:
                assert call() == 0, (op, pixel, lib.tsm_last_error(None))
            assert tr.kernels == [op + '_kernel<Nv12>'], tr.kernels
    torch.cuda.synchronize()
    check(src, boxes, index, desc)


# ---- 4. end to end on an engine -------------------------------------------------------------------------------------------------
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


def _clip_box(video_name, clip):
    return [(-5, -7, 80, 90), None, (10, 12, 40, 30), (30, 2, 50, 70)][clip % 4]


def test_video_clip_logits_on_nv12_equals_the_rgb_call_bit_for_bit(engine):
    """64 x 64 frames, 29 of them: 4 clips, the last two with padded tails (the staged pad is nv12_black).  Centre crop and person
    crop; one NV12 launch of the right kind per batch and no RGB one."""
    from workoutdetector_amd import inference_count as ic
    from workoutdetector_amd.engine import launch_trace
    from workoutdetector_amd.transform import PersonCropTransform, TestTransform, nv12_to_rgb
    vid = _nv12(1000, 29, 64, 64)
    centre = {}
    for name in ('bt601', 'bt709'):
        rgb = torch.from_numpy(nv12_to_rgb(vid, name))
        for transform, kernel in ((TestTransform(), 'preprocess_kernel'), (PersonCropTransform(_clip_box), 'preprocess_clips_kernel')):
            with launch_trace() as tr:
                got = ic.video_clip_logits(engine, vid, transform, batch_clips=3, video_name='v', frame_format='nv12', colorimetry=name)
            assert tr.ran(kernel + '<Nv12>') and not tr.ran(kernel + '<unsigned char>') and not tr.ran(kernel + '<float>'), tr.kernels
            want = ic.video_clip_logits(engine, rgb, transform, batch_clips=3, video_name='v')
            assert tuple(got.shape) == (4, 12) and bool(torch.isfinite(got).all())
            assert _same_bits(got, want), (name, kernel, float((got - want).abs().max()))
            centre.setdefault(name, got)
    assert not _same_bits(centre['bt601'], centre['bt709'])


def test_stream_batcher_on_nv12_equals_the_rgb_batcher_on_the_converted_frames(engine):
    """Two streams of different sizes (64 x 64 and 48 x 80), 16 frames each, person crop off and on: one <Nv12> windows launch per
    batch, the same states and counts as the RGB batcher on nv12_to_rgb of the frames, and the pinned budget counts 3hw/2 bytes
    per frame."""
    from workoutdetector_amd.engine import launch_trace
    from workoutdetector_amd.streaming import StreamBatcher
    from workoutdetector_amd.transform import nv12_to_rgb
    vids = {'a': _nv12(1100, 16, 64, 64), 'b': _nv12(1101, 16, 48, 80)}
    for person_crop in (False, True):
        got = StreamBatcher(engine, threshold=0.0, max_batch=4, person_crop=person_crop, frame_format='nv12', colorimetry='bt709')
        want = StreamBatcher(engine, threshold=0.0, max_batch=4, person_crop=person_crop)
        ev_got, ev_want = {}, {}
        with launch_trace() as tr:
            for t in range(16):
                for k, v in vids.items():
                    kw = dict(box=(3 + t % 5, 4, 40, 43 + t % 3)) if person_crop and k == 'a' else {}
                    got.push(k, v[t].numpy(), **kw)
                    if t == 0 and k == 'b':
                        assert got.pinned_bytes == 8 * (3 * 64 * 64 // 2 + 3 * 48 * 80 // 2)
                if t % 8 == 7:
                    for k, e in got.step().items():
                        ev_got.setdefault(k, []).extend(e)
        assert tr.count('preprocess_windows_kernel<Nv12>') == 2 and tr.count('preprocess_windows_kernel') == 2, tr.kernels
        for t in range(16):
            for k, v in vids.items():
                kw = dict(box=(3 + t % 5, 4, 40, 43 + t % 3)) if person_crop and k == 'a' else {}
                want.push(k, nv12_to_rgb(v[t].numpy(), 'bt709')[0], **kw)
            if t % 8 == 7:
                for k, e in want.step().items():
                    ev_want.setdefault(k, []).extend(e)
        assert ev_got == ev_want and {k: len(e) for k, e in ev_got.items()} == {'a': 2, 'b': 2}
        assert all(got.result(k) == want.result(k) for k in vids)
        assert -1 not in {s for e in ev_got.values() for _, s, _ in e}
        for k in vids:
            got.close(k)
            want.close(k)


# ---- 5. capture and replay ----------------------------------------------------------------------------------------------------
def test_the_nv12_form_of_each_launch_is_captured_and_replayed(hip_lib, monkeypatch):
    """tests/_capture.py on the NV12 form of the four launches: captured on a side stream, replayed bit-identical to eager."""
    from workoutdetector_amd import engine as E
    from workoutdetector_amd.transform import window_descriptors
    monkeypatch.delenv('TSM_POISON', raising=False)
    h, w, resize, crop = 52, 90, 36, 32
    fmt = dict(frame_format='nv12', colorimetry='bt709')
    sets = [[_nv12(1200 + k, N_STAGED, h, w)] for k in range(3)]
    frames = guarded(sets[0][0].cuda(), name='frames')
    out = guarded_out((N_STAGED, crop, crop, 4), name='out')
    tr = captured(lambda: E.preprocess_frames(frames, resize=resize, crop=crop, out=out, **fmt), [frames], lambda k: sets[k], [out])
    assert_ran(tr, 'preprocess_kernel<Nv12>', 'preprocess')

    rows = guarded(torch.tensor(_boxes(h, w), dtype=torch.int32).cuda(), name='boxes')
    out = guarded_out((N_CLIPS, 8, crop, crop, 4), name='out')
    tr = captured(lambda: E.preprocess_clips(frames, rows, 0, TOTAL, 0, N_CLIPS, size=crop, clip_step=STEP, clip_stride=STRIDE, out=out, **fmt),
                  [frames], lambda k: sets[k], [out])
    assert_ran(tr, 'preprocess_clips_kernel<Nv12>', 'preprocess_clips')

    index = guarded(torch.tensor(INDEX, dtype=torch.int32).cuda(), name='index')
    out = guarded_out((2, 8, crop, crop, 4), name='out')
    tr = captured(lambda: E.preprocess_indexed(frames, index, resize=resize, crop=crop, out=out, **fmt), [frames], lambda k: sets[k], [out])
    assert_ran(tr, 'preprocess_indexed_kernel<Nv12>', 'preprocess_indexed')

    shapes = [(52, 90), (36, 36), (52, 90)]
    wsets, table = [], None
    for k in range(3):
        arena, offsets = _pack([_nv12(1300 + 10 * k + i, 2, *s) for i, s in enumerate(shapes)])
        table = window_descriptors(shapes, offsets, resize=resize, crop=crop, frame_format='nv12')
        wsets.append([arena])
    arena = guarded(wsets[0][0].cuda(), name='arena')
    desc = guarded(torch.from_numpy(table).cuda(), name='desc')
    out = guarded_out((3, 2, crop, crop, 4), name='out')
    tr = captured(lambda: E.preprocess_windows(arena, desc, 3, 2, resize=resize, crop=crop, out=out, **fmt), [arena], lambda k: wsets[k], [out])
    assert_ran(tr, 'preprocess_windows_kernel<Nv12>', 'preprocess_windows')
    check(rows, index, desc)
