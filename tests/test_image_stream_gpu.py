"""tsm_preprocess_windows in image mode (TSM_WINDOWS_IMAGE: the image model's transform over windows of different sizes, one
launch) against tsm_preprocess_image per window and against the NumPy ImageTransform, and ImageStreamBatcher on real engines
against image_states / count_by_image_model.

Every launch runs in hostile memory (tests/_guard.py): the arena and the descriptor table between poisoned bands, the output
poisoned before the launch, bands and payload checked after it.  Every comparison is bit for bit: the resample is integer
arithmetic, the normalisation three correctly rounded fp32 operations, and the engine sums in a fixed order.

Sizes are h x w.  torchvision's Resize(int) keeps the aspect ratio, so at resize = 24 a frame with a side of 24 keeps BOTH
sides: 24 x 41, 24 x 24, 3700 x 24 and 16800 x 24 are all copied (no tables), whatever their long side.  A vertical support
that presses on the LDS needs both sides large: 3700 x 3700 is the window whose band falls back below 8, 16800 x 16800 the
one whose support does not fit at all; they stand beside the sizes above."""
import functools
import os

import numpy as np
import pytest
import torch

from tests._capture import captured
from tests._guard import check, guarded, guarded_out

pytestmark = pytest.mark.gpu

LAYOUTS = ('nthwc4', 'ntchw', 'nthwc8s', 'nthwc8b')
FORMATS = ('rgb', 'nv12')
COLORIMETRY = 'bt709'
RESIZE, CROP = 24, 16
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
# the issue's list, in its order; NV12: the even sizes nearest to them
SIZES = {'rgb': [(90, 31), (31, 90), (24, 41), (24, 24), (10, 17), (3700, 24)],
         'nv12': [(90, 32), (32, 90), (24, 42), (24, 24), (10, 18), (3700, 24)]}


def _layout(name):
    from workoutdetector_amd import _lib
    return {'nthwc4': _lib.LAYOUT_NTHWC4, 'ntchw': _lib.LAYOUT_NTCHW, 'nthwc8s': _lib.LAYOUT_NTHWC8S,
            'nthwc8b': _lib.LAYOUT_NTHWC8B}[name]


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _window(seed, t, h, w, fmt):
    """One window of noise: uint8 [t, h, w, 3], or NV12 surfaces [t, 3h/2, w]."""
    rng = np.random.default_rng([seed, t, h, w])
    a = rng.integers(0, 256, size=(t, h, w, 3) if fmt == 'rgb' else (t, 3 * h // 2, w), dtype=np.uint8)
    a.setflags(write=False)
    return a


def _rgb(window, fmt):
    from workoutdetector_amd.transform import nv12_to_rgb
    return window if fmt == 'rgb' else nv12_to_rgb(window, COLORIMETRY)


def _hw(window, fmt):
    return (window.shape[1], window.shape[2]) if fmt == 'rgb' else (window.shape[1] * 2 // 3, window.shape[2])


def _pack(windows, fmt, resize, crop, shared=True, tables_first=False):
    """The arena of one launch (uint8 ndarray) and its descriptors: transform.image_window_arena's layout (frames, then one
    block per distinct geometry), or -- shared=False -- a block of its own behind every window; tables_first: the blocks in
    front, so that the last window ends with the arena."""
    from workoutdetector_amd.transform import image_tables, image_window_arena, image_window_descriptors
    shapes = [_hw(w, fmt) for w in windows]
    t = windows[0].shape[0]
    if shared and not tables_first:
        desc, offsets, tables, nbytes = image_window_arena(shapes, n_segment=t, resize=resize, crop=crop, frame_format=fmt)
        arena = np.zeros(nbytes, dtype=np.uint8)
        for off, block in tables:
            arena[off:off + block.nbytes] = block.view(np.uint8)
    else:
        pieces, offsets, tabs, total = [], [], [], 0

        def put(data):
            nonlocal total
            pieces.append((total, data))
            total += (data.size + 15) // 16 * 16
            return pieces[-1][0]
        blocks = [image_tables(h, w, resize, crop).view(np.uint8) for h, w in shapes]
        if tables_first:
            tabs = [put(b) for b in blocks]
        for w, b in zip(windows, blocks):
            offsets.append(put(w.reshape(-1)))
            if not tables_first:
                tabs.append(put(b))
        arena = np.zeros(max(total, 16), dtype=np.uint8)
        for off, data in pieces:
            arena[off:off + data.size] = data
        desc = image_window_descriptors(shapes, offsets, tabs, resize, crop, fmt)
    for w, off in zip(windows, offsets):
        arena[off:off + w.size] = w.reshape(-1)
    return arena, desc


def _launch(arena, desc, t, resize, crop, layout_name, fmt, arena_bytes=None):
    """engine.preprocess_image_windows in hostile memory; arena_bytes: launch on the arena's first arena_bytes only."""
    from workoutdetector_amd.engine import _frame_shape, launch_trace, preprocess_image_windows
    src = guarded(torch.from_numpy(np.array(arena)).cuda() if isinstance(arena, np.ndarray) else arena, name='arena')
    rows = guarded(torch.from_numpy(np.ascontiguousarray(desc, dtype=np.int32)).cuda(), name='desc')
    n = rows.shape[0]
    out = guarded_out((n, t) + _frame_shape(_layout(layout_name), crop), name='out')
    with launch_trace() as tr:
        got = preprocess_image_windows(src if arena_bytes is None else src[:arena_bytes], rows, n, t, resize=resize, crop=crop,
                                       out_layout=_layout(layout_name), frame_format=fmt,
                                       colorimetry=COLORIMETRY if fmt == 'nv12' else None, out=out)
    assert got is out
    kernel = 'preprocess_image_windows_kernel<' + ('Nv12' if fmt == 'nv12' else 'unsigned char') + '>'
    assert tr.kernels == [kernel], tr.kernels
    torch.cuda.synchronize()
    check(src, rows, out)
    return out.cpu()


def _alone(window, fmt, resize, crop, layout_name):
    """tsm_preprocess_image on the window's frames alone (NV12: on transform.nv12_to_rgb of them)."""
    from workoutdetector_amd.engine import preprocess_image
    return preprocess_image(torch.from_numpy(np.array(_rgb(window, fmt))).cuda(), resize, crop, out_layout=_layout(layout_name)).cpu()


@functools.lru_cache(maxsize=None)
def _numpy(seed, t, h, w, fmt, resize, crop):
    from workoutdetector_amd.transform import ImageTransform
    return ImageTransform(resize, crop)(_rgb(_window(seed, t, h, w, fmt), fmt))


def _zero_frame(t, crop, layout_name):
    """The normalised zero frame in a layout: tsm_preprocess_image of black frames that need no resample."""
    from workoutdetector_amd.engine import preprocess_image
    black = torch.zeros((t, crop, crop, 3), dtype=torch.uint8, device='cuda')
    z = preprocess_image(black, crop, crop, out_layout=_layout(layout_name)).cpu()
    if layout_name == 'ntchw':
        mean, std = np.float32([0.485, 0.456, 0.406]), np.float32([0.229, 0.224, 0.225])
        want = torch.from_numpy(((np.float32(0) - mean) / std).astype(np.float32)).view(1, 3, 1, 1).expand(t, 3, crop, crop)
        assert _same_bits(z, want.contiguous())
    return z


# ---- 1. one launch over windows of different sizes -----------------------------------------------------------------------
@pytest.mark.parametrize('t', [1, 2])
@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('layout_name', LAYOUTS)
def test_mixed_sizes_in_one_launch_equal_preprocess_image_per_window(hip_lib, layout_name, fmt, t):
    """90 x 31 and 31 x 90 (both passes, tall and wide), 24 x 41 and 24 x 24 (Resize keeps both sides: no tables, the rows are
    copied; the descriptor's tab is garbage and ignored), 10 x 17 (upscale, 3 taps), 3700 x 24 (copied too: see the module's
    note).  Row (c, k) equals tsm_preprocess_image's row for that frame bit for bit, and the fp32 layouts equal NumPy's
    ImageTransform bit for bit."""
    from workoutdetector_amd.transform import image_tables
    windows = [_window(100 + i, t, h, w, fmt) for i, (h, w) in enumerate(SIZES[fmt])]
    arena, desc = _pack(windows, fmt, RESIZE, CROP)
    for i, (h, w) in enumerate(SIZES[fmt]):
        if not image_tables(h, w, RESIZE, CROP).size:
            desc[i, 4:6] = (0x7FFFFFF7, I32_MAX) if i % 2 else (-9, I32_MIN)          # no block: tab is not looked at
    assert [bool(image_tables(h, w, RESIZE, CROP).size) for h, w in SIZES[fmt]] == [True, True, False, False, True, False]
    got = _launch(arena, desc, t, RESIZE, CROP, layout_name, fmt)
    for i, (h, w) in enumerate(SIZES[fmt]):
        assert _same_bits(got[i], _alone(windows[i], fmt, RESIZE, CROP, layout_name)), (i, h, w)
        want = _numpy(100 + i, t, h, w, fmt, RESIZE, CROP)
        if layout_name == 'ntchw':
            assert _same_bits(got[i], want), (i, h, w)
        elif layout_name == 'nthwc4':
            assert _same_bits(got[i][..., :3], want.permute(0, 2, 3, 1)) and not got[i][..., 3].any(), (i, h, w)


@pytest.mark.parametrize('fmt', FORMATS)
def test_a_band_below_eight_rows_gives_the_same_bits(hip_lib, fmt):
    """3700 x 3700 at 24 / 16: a 154x downscale on both axes, 311 taps per row; 9 * 154.2 + 2 rows of 48 bytes do not fit 64 KB,
    so the workgroup works in bands of 4 rows (tests/image_windows_host.cpp pins the 4), next to a 90 x 31 neighbour that works
    in bands of 8.  The result is integer arithmetic: it cannot depend on the band."""
    sizes = [(90, 31 if fmt == 'rgb' else 32), (3700, 3700)]
    windows = [_window(150 + i, 1, h, w, fmt) for i, (h, w) in enumerate(sizes)]
    arena, desc = _pack(windows, fmt, RESIZE, CROP)
    want = _numpy(151, 1, 3700, 3700, fmt, RESIZE, CROP)
    for layout_name in LAYOUTS:
        got = _launch(arena, desc, 1, RESIZE, CROP, layout_name, fmt)
        for i in range(2):
            assert _same_bits(got[i], _alone(windows[i], fmt, RESIZE, CROP, layout_name)), (layout_name, i)
        if layout_name == 'ntchw':
            assert _same_bits(got[1], want)


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('layout_name', LAYOUTS)
def test_an_odd_crop(hip_lib, layout_name, fmt):
    """resize 16, crop 15: the pair layouts end every row in a half pixel pair, and the crop offsets are halves that round to
    the even neighbour (40 x 56 -> 16 x 22: left = round(3.5) = 4; 16 x 16: round(0.5) = 0; 56 x 40 -> 22 x 16: top = 4)."""
    from workoutdetector_amd.transform import crop_offsets, resized_hw
    sizes = [(40, 56), (16, 16), (56, 40), (90, 32)]
    assert [crop_offsets(*resized_hw(h, w, 16), 15) for h, w in sizes[:3]] == [(0, 4), (0, 0), (4, 0)]
    windows = [_window(200 + i, 2, h, w, fmt) for i, (h, w) in enumerate(sizes)]
    arena, desc = _pack(windows, fmt, 16, 15)
    got = _launch(arena, desc, 2, 16, 15, layout_name, fmt)
    for i, (h, w) in enumerate(sizes):
        assert _same_bits(got[i], _alone(windows[i], fmt, 16, 15, layout_name)), (i, h, w)
        if layout_name == 'ntchw':
            assert _same_bits(got[i], _numpy(200 + i, 2, h, w, fmt, 16, 15)), (i, h, w)


@pytest.mark.parametrize('fmt', FORMATS)
def test_shared_and_separate_table_blocks_give_the_same_bits(hip_lib, fmt):
    sizes = [(40, 56), (90, 32), (40, 56), (40, 56), (90, 32)]
    windows = [_window(300 + i, 2, h, w, fmt) for i, (h, w) in enumerate(sizes)]
    shared, d_shared = _pack(windows, fmt, RESIZE, CROP)
    apart, d_apart = _pack(windows, fmt, RESIZE, CROP, shared=False)
    assert len(set(d_shared[:, 4].tolist())) == 2 and len(set(d_apart[:, 4].tolist())) == 5
    for layout_name in LAYOUTS:
        a = _launch(shared, d_shared, 2, RESIZE, CROP, layout_name, fmt)
        b = _launch(apart, d_apart, 2, RESIZE, CROP, layout_name, fmt)
        assert _same_bits(a, b), layout_name
        assert _same_bits(a[0], _alone(windows[0], fmt, RESIZE, CROP, layout_name))


# ---- 2. invalid windows between valid ones ---------------------------------------------------------------------------------
def _row(off, h, w, tab):
    def words(v):
        v &= (1 << 64) - 1
        lo, hi = v & 0xFFFFFFFF, v >> 32
        return [lo - (1 << 32) if lo >= 1 << 31 else lo, hi - (1 << 32) if hi >= 1 << 31 else hi]
    return words(off) + [h, w] + words(tab) + [0, 0]


@pytest.mark.parametrize('fmt', FORMATS)
def test_invalid_windows_are_zero_frames_and_leave_their_neighbours_alone(hip_lib, fmt):
    """One launch: three valid 40 x 56 windows with the invalid descriptors between them -- an unaligned off, off = -16, frames
    past the arena, h = 0, a side of 65536, INT32_MIN / INT32_MAX / 0 in every word, an unaligned tab, tab = -16, a tab past
    the arena and, for NV12, an odd side.  Then the two ends of the arena by one byte and by one word: the arena cut one byte
    short of the last window's frames, and cut one word short of the last window's table block.  An invalid window is the
    normalised zero frame, a valid one equals the launch without the invalid rows, every band is intact.  The documented
    behaviour, exercised; not an attempt to fault."""
    h, w, t = 40, 56, 2
    windows = [_window(400 + i, t, h, w, fmt) for i in range(3)]
    arena, valid = _pack(windows, fmt, RESIZE, CROP, tables_first=True)         # the last window ends with the arena
    n_bytes, nbytes = arena.size, windows[0].size
    valid = valid.tolist()
    assert valid[2][0] + nbytes == n_bytes
    tab = valid[0][4]
    bad = [_row(8, h, w, tab), _row(-16, h, w, tab), _row(n_bytes, h, w, tab), _row(n_bytes - nbytes + 1, h, w, tab),
           _row(n_bytes - nbytes + 16, h, w, tab), _row(0, 0, w, tab), _row(0, h, 0, tab), _row(0, 65536, w, tab), _row(0, h, 65536, tab),
           _row(0, -1, w, tab), [I32_MIN] * 8, [I32_MAX] * 8, [0] * 8, _row(0, h, w, tab + 8), _row(0, h, w, -16), _row(0, h, w, n_bytes),
           _row(0, h, w, n_bytes - 16), _row(0, h, w, 2 ** 63 - 16), _row(2 ** 63 - 16, h, w, tab)]
    if fmt == 'nv12':
        bad += [_row(0, h - 1, w, tab), _row(0, h, w - 1, tab)]
    cut = len(bad) // 2
    table = np.array([valid[0]] + bad[:cut] + [valid[1]] + bad[cut:] + [valid[2]], dtype=np.int64).astype(np.int32)
    where_valid = [0, cut + 1, len(bad) + 2]
    for layout_name in LAYOUTS:
        got = _launch(arena, table, t, RESIZE, CROP, layout_name, fmt)
        alone = _launch(arena, np.array(valid), t, RESIZE, CROP, layout_name, fmt)
        zero = _zero_frame(t, CROP, layout_name)
        for i in range(len(table)):
            if i in where_valid:
                j = where_valid.index(i)
                assert _same_bits(got[i], alone[j]) and _same_bits(got[i], _alone(windows[j], fmt, RESIZE, CROP, layout_name)), (layout_name, i)
                assert not _same_bits(got[i], zero)
            else:
                assert _same_bits(got[i], zero), (layout_name, i, table[i].tolist())
    # one byte: the arena ends inside the last byte of the last window's frames
    got = _launch(arena, np.array(valid), t, RESIZE, CROP, 'ntchw', fmt, arena_bytes=n_bytes - 1)
    assert _same_bits(got[:2], alone_ntchw(arena, valid, t, fmt)[:2]) and _same_bits(got[2], _zero_frame(t, CROP, 'ntchw'))
    # one word: the same windows with the last one's block at the arena's end, the arena cut 4 bytes short
    apart, d_apart = _pack(windows, fmt, RESIZE, CROP, shared=False)
    end = apart.size
    assert d_apart[2, 4] + 4 * 2 * CROP * 7 == end                              # 40 x 56 -> 24 x 33: 5 taps on both axes
    got = _launch(apart, d_apart, t, RESIZE, CROP, 'ntchw', fmt, arena_bytes=end - 4)
    assert _same_bits(got[:2], alone_ntchw(arena, valid, t, fmt)[:2]) and _same_bits(got[2], _zero_frame(t, CROP, 'ntchw'))
    assert not _same_bits(_launch(apart, d_apart, t, RESIZE, CROP, 'ntchw', fmt)[2], _zero_frame(t, CROP, 'ntchw'))


def alone_ntchw(arena, valid, t, fmt):
    return _launch(arena, np.array(valid), t, RESIZE, CROP, 'ntchw', fmt)


@pytest.mark.parametrize('fmt', FORMATS)
def test_a_vertical_support_beyond_the_lds_is_a_zero_frame(hip_lib, fmt):
    """16800 x 16800 at 24 / 16: one output row's support is 2 * 700 + 2 rows of 48 bytes, more than 64 KB -- the window is
    invalid although its frame lies in the arena (uninitialised device memory: nothing of it is read), and tsm_preprocess_image
    refuses the same frame with TSM_ERR_UNSUPPORTED.  16800 x 24 beside it keeps both sides and is copied."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import preprocess_image
    from workoutdetector_amd.transform import frame_bytes, image_tables
    big = frame_bytes(16800, 16800, fmt)
    small = _window(500, 1, 16800, 24, fmt)
    edge = _window(501, 1, 90, 32, fmt)
    block = image_tables(90, 32, RESIZE, CROP).view(np.uint8)
    off_small = (big + 15) // 16 * 16
    off_edge = off_small + (small.size + 15) // 16 * 16
    tab = off_edge + (edge.size + 15) // 16 * 16
    arena = torch.empty(tab + block.size, dtype=torch.uint8, device='cuda')
    for off, data in ((off_small, small), (off_edge, edge), (tab, block)):
        arena[off:off + data.size] = torch.from_numpy(np.array(data).reshape(-1)).cuda()
    desc = np.array([_row(off_edge, 90, 32, tab), _row(0, 16800, 16800, tab), _row(off_small, 16800, 24, 0), _row(off_edge, 90, 32, tab)])
    for layout_name in ('ntchw', 'nthwc8b'):
        got = _launch(arena, desc, 1, RESIZE, CROP, layout_name, fmt)
        assert _same_bits(got[1], _zero_frame(1, CROP, layout_name))
        assert _same_bits(got[0], _alone(edge, fmt, RESIZE, CROP, layout_name)) and _same_bits(got[3], got[0])
        assert _same_bits(got[2], _alone(small, fmt, RESIZE, CROP, layout_name))
    if fmt == 'rgb':
        with pytest.raises(_lib.TsmError) as ei:
            preprocess_image(arena[:big].view(1, 16800, 16800, 3), RESIZE, CROP)
        assert ei.value.status == -7


# ---- 3. hostile table contents ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('fill', ['min', 'max', 'random'])
def test_hostile_table_contents_stay_inside_the_frames_and_the_rows(hip_lib, fmt, fill):
    """The table CONTENTS cannot be validated: every hb / vb word INT32_MIN, INT32_MAX or random and the weights random, the
    launch succeeds, every band is intact and no output word is left poison.  The values are unspecified.  The documented
    behaviour, exercised; not an attempt to fault."""
    from workoutdetector_amd.transform import image_tables
    sizes = [(90, 32), (32, 90), (10, 18), (40, 56)]
    windows = [_window(600 + i, 2, h, w, fmt) for i, (h, w) in enumerate(sizes)]
    arena, desc = _pack(windows, fmt, RESIZE, CROP, shared=False)
    rng = np.random.default_rng(7)
    for (h, w), row in zip(sizes, desc):
        n = image_tables(h, w, RESIZE, CROP).size
        half = n // 2                                                       # [hb 2 * crop][hk ...][vb 2 * crop][vk ...], two equal halves here
        block = rng.integers(I32_MIN, I32_MAX, size=n, dtype=np.int64).astype(np.int32)
        bounds = {'min': I32_MIN, 'max': I32_MAX}.get(fill)
        if bounds is not None:
            block[:2 * CROP] = bounds
            block[half:half + 2 * CROP] = bounds
        arena[row[4]:row[4] + 4 * n] = block.view(np.uint8)
    for layout_name in LAYOUTS:
        _launch(arena, desc, 2, RESIZE, CROP, layout_name, fmt)                 # (check() inside: bands intact, no poison left)


# ---- 4. more work items than workgroups ------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', FORMATS)
def test_the_grid_stride_loop_wraps(hip_lib, fmt):
    """4100 frames of 10 x 17 at crop 16: 2 work items per frame, 8200 > the 8192-workgroup cap, so the first workgroups take a
    second item.  The same frames in two launches of 2050 give the same bits."""
    h, w = (10, 17) if fmt == 'rgb' else (10, 18)
    frames = _window(700, 4100, h, w, fmt)
    windows = [frames[i:i + 1] for i in range(4100)]
    arena, desc = _pack(windows, fmt, RESIZE, CROP)
    assert len(set(desc[:, 4].tolist())) == 1
    for layout_name in ('nthwc4', 'nthwc8b'):
        whole = _launch(arena, desc, 1, RESIZE, CROP, layout_name, fmt)
        halves = torch.cat([_launch(arena, desc[:2050], 1, RESIZE, CROP, layout_name, fmt), _launch(arena, desc[2050:], 1, RESIZE, CROP, layout_name, fmt)])
        assert _same_bits(whole, halves), layout_name
        for i in (0, 2049, 2050, 4095, 4096, 4099):
            assert _same_bits(whole[i], _alone(windows[i], fmt, RESIZE, CROP, layout_name)), (layout_name, i)


# ---- 5. enqueue-only: capture on a side stream and replay ------------------------------------------------------------------
@pytest.mark.parametrize('fmt', FORMATS)
def test_capture_and_replay(hip_lib, fmt):
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import _frame_shape, preprocess_image_windows
    sizes = [(90, 32), (24, 24), (10, 18), (32, 90)]

    def arena_of(k):
        return _pack([_window(800 + 10 * k + i, 2, h, w, fmt) for i, (h, w) in enumerate(sizes)], fmt, RESIZE, CROP)
    arena0, desc0 = arena_of(0)
    arena = guarded(torch.from_numpy(arena0).cuda(), name='arena')
    desc = guarded(torch.from_numpy(desc0).cuda(), name='desc')
    out = guarded_out((4, 2) + _frame_shape(_lib.LAYOUT_NTHWC8S, CROP), name='out')

    def run():
        preprocess_image_windows(arena, desc, 4, 2, resize=RESIZE, crop=CROP, out_layout=_lib.LAYOUT_NTHWC8S, frame_format=fmt,
                                 colorimetry=COLORIMETRY if fmt == 'nv12' else None, out=out)
    tr = captured(run, [arena, desc], lambda k: [torch.from_numpy(arena_of(k)[0]), torch.from_numpy(desc0)], [out])
    assert len(tr.kernels) == 1 and tr.ran('preprocess_image_windows_kernel<'), tr.kernels
    assert tr.kernel_nodes in (None, 1)


def test_the_binding_refuses_what_the_mode_does_not_take(hip_lib):
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import launch_trace, preprocess_image_windows
    arena0, desc0 = _pack([_window(1, 1, 40, 56, 'rgb')], 'rgb', RESIZE, CROP)
    arena, desc = torch.from_numpy(arena0).cuda(), torch.from_numpy(desc0).cuda()
    with launch_trace() as tr:
        for a, d in ((arena.cpu(), desc), (arena, desc.cpu()), (arena.float(), desc), (arena[1:], desc), (arena, desc.float()), (arena, desc[:, :4])):
            with pytest.raises(ValueError):
                preprocess_image_windows(a, d, 1, 1, resize=RESIZE, crop=CROP)
        with pytest.raises(ValueError):
            preprocess_image_windows(arena, desc, 0, 1)
        with pytest.raises(NotImplementedError):
            preprocess_image_windows(arena, desc, 1, 1, resize=RESIZE, crop=CROP, frame_format='i420')
        with pytest.raises(_lib.TsmError) as ei:
            preprocess_image_windows(arena, desc, 1, 1, resize=16, crop=17)
    assert ei.value.status == -1 and tr.kernels == []


# ---- 6. ImageStreamBatcher on engines --------------------------------------------------------------------------------------
E_RESIZE, E_CROP = 40, 32
BIAS_SHIFT = 4.75           # tests/test_image_path_gpu.py: puts the seeded R18's decision between its dark and its bright frames
STREAMS = {'a': (41, 37, 46, 60), 'b': (42, 30, 60, 46), 'c': (43, 44, 32, 32), 'd': (44, 25, 90, 52)}      # seed, frames, h, w


@functools.lru_cache(maxsize=None)
def _video(k):
    seed, n, h, w = STREAMS[k]
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    for a in range(seed % 10, n, 10):
        frames[a:a + 5] //= 6                   # dark and bright stretches of five frames
    frames.setflags(write=False)
    return frames


def _with_env(make, poison):
    keep = {k: os.environ.get(k) for k in ('TSM_AUTOTUNE', 'TSM_POISON')}
    os.environ['TSM_AUTOTUNE'] = '0'
    os.environ.pop('TSM_POISON', None)
    if poison:
        os.environ['TSM_POISON'] = '1'
    try:
        return make()                            # (TSM_* are read in tsm_create)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope='module')
def checkpoint(tmp_path_factory):
    from workoutdetector_amd.weights import make_state_dict
    tv = {}
    for k, v in make_state_dict(0, 2, 'resnet18').items():
        tv[k[len('base_model.'):].replace('.conv1.net.', '.conv1.') if k.startswith('base_model.') else k] = torch.from_numpy(v.copy())
    tv['fc.bias'][1] += BIAS_SHIFT
    path = str(tmp_path_factory.mktemp('ckpt') / 'image_r18.pth')
    torch.save(tv, path)
    return path


def _r18(checkpoint, poison=False):
    from workoutdetector_amd.engine import create_image_model
    return _with_env(lambda: create_image_model(num_class=2, base_model='resnet18', checkpoint=checkpoint, resize=E_RESIZE, crop=E_CROP,
                                                max_frames=8), poison)


def _convnext():
    from workoutdetector_amd.engine import TsmEngine
    from workoutdetector_amd.weights import make_state_dict
    depths = (1, 1, 2, 1)
    eng = _with_env(lambda: TsmEngine(num_class=2, num_segments=1, height=E_CROP, width=E_CROP, is_shift=False, max_clips=8,
                                      state_dict=make_state_dict(0, 2, 'convnext_base', depths=depths), base_model='convnext_base',
                                      convnext_depths=depths), False)
    eng.image_resize, eng.image_crop = E_RESIZE, E_CROP
    return eng


@pytest.fixture(scope='module')
def r18(hip_lib, checkpoint):
    eng = _r18(checkpoint)
    yield eng
    eng.close()


def _play(model, seed, max_batch=None, fmt='rgb', videos=None):
    """Push the four streams in a seeded random interleaving, step at random -> ({stream: states}, {stream: (count, reps)},
    [(frames, geometries) of every batch]).  videos: what is pushed in place of the RGB frames of _video."""
    from workoutdetector_amd.streaming import ImageStreamBatcher
    sb = ImageStreamBatcher(model, max_batch=max_batch, frame_format=fmt, colorimetry=COLORIMETRY if fmt == 'nv12' else None)
    videos = videos or {k: _video(k) for k in STREAMS}
    sizes = []
    inner = sb._preds_device

    def spy(ch):
        sizes.append((len(ch.sids), len(set(ch.shapes))))
        return inner(ch)
    sb._preds_device = spy
    rng = np.random.default_rng(seed)
    nxt, rows = {k: 0 for k in STREAMS}, {k: [] for k in STREAMS}
    while any(nxt[k] < STREAMS[k][1] for k in STREAMS):
        k = str(rng.choice([k for k in STREAMS if nxt[k] < STREAMS[k][1]]))
        sb.push(k, videos[k][nxt[k]])
        nxt[k] += 1
        if rng.random() < 0.06:
            for sid, r in sb.step().items():
                rows[sid] += r
    for sid, r in sb.step().items():
        rows[sid] += r
    states = {k: [s for _, s, _ in rows[k]] for k in STREAMS}
    assert all(states[k] == sb.streams[k].states and [i for i, _, _ in rows[k]] == list(range(STREAMS[k][1])) for k in STREAMS)
    counted = {k: sb.close(k) for k in STREAMS}
    assert not sb.streams and not sb._free
    return states, counted, sizes


def _offline(model):
    from workoutdetector_amd import inference_count as ic
    return ({k: ic.image_states(model, np.array(_video(k)))[0] for k in STREAMS},
            {k: ic.count_by_image_model(model, np.array(_video(k))) for k in STREAMS})


@pytest.mark.parametrize('seed', [0, 1])
def test_batcher_on_resnet18_equals_the_offline_loop_per_stream(r18, seed):
    """Four streams of four sizes, seeded interleavings of push and step, batches that split across max_batch = 8: per stream
    the states equal image_states and (count, reps) equal count_by_image_model; every batch is exactly one
    preprocess_image_windows_kernel launch whatever the number of resolutions in it, one scores_to_states launch, and no other
    transform kernel runs."""
    from workoutdetector_amd.engine import launch_trace
    want_states, want_counts = _offline(r18)
    print({k: ''.join(map(str, v)) for k, v in want_states.items()}, want_counts)
    with launch_trace() as tr:
        states, counted, sizes = _play(r18, seed)
    assert states == want_states and counted == want_counts
    assert max(n for n, _ in sizes) == 8 and max(g for _, g in sizes) >= 3 and sum(n for n, _ in sizes) == sum(v[1] for v in STREAMS.values())
    assert tr.count('preprocess_image_windows_kernel<unsigned char>') == len(sizes) == tr.count('scores_to_states_kernel'), tr.kernels
    assert not tr.ran('preprocess_image_kernel') and not tr.ran('preprocess_kernel') and not tr.ran('preprocess_windows_kernel') and \
        not tr.ran('frame_votes_kernel'), tr.kernels
    small = _play(r18, seed + 10, max_batch=3)
    assert small[:2] == (want_states, want_counts) and max(n for n, _ in small[2]) == 3


def test_nv12_batcher_equals_the_rgb_batcher_on_converted_frames(r18):
    from workoutdetector_amd.engine import launch_trace
    from workoutdetector_amd.transform import nv12_to_rgb, rgb_to_nv12
    surfaces = {k: rgb_to_nv12(_video(k), COLORIMETRY) for k in STREAMS}
    with launch_trace() as tr:
        nv12 = _play(r18, 3, fmt='nv12', videos=surfaces)
    assert tr.count('preprocess_image_windows_kernel<Nv12>') == len(nv12[2]) and not tr.ran('preprocess_image_windows_kernel<unsigned char>'), tr.kernels
    rgb = _play(r18, 3, videos={k: nv12_to_rgb(v, COLORIMETRY) for k, v in surfaces.items()})
    assert nv12 == rgb


def test_whole_engine_run_under_poison_gives_the_same_states(r18, checkpoint):
    """TSM_POISON=1: every device buffer of the engine between poisoned bands, activations poisoned before each forward."""
    clean = _play(r18, 5)
    eng = _r18(checkpoint, poison=True)
    try:
        poisoned = _play(eng, 5)
    finally:
        eng.close()
    assert poisoned == clean and clean[:2] == _offline(r18)


def test_batcher_on_a_convnext_engine_equals_the_offline_loop_per_stream(hip_lib):
    eng = _convnext()
    try:
        want = _offline(eng)
        got = _play(eng, 2)
        assert got[:2] == want
        assert _play(eng, 12, max_batch=5)[:2] == want
        # the engine's own method: its layout, its geometry
        from workoutdetector_amd.engine import preprocess_image_windows
        arena0, desc0 = _pack([_window(900, 1, 46, 60, 'rgb'), _window(901, 1, 90, 52, 'rgb')], 'rgb', E_RESIZE, E_CROP)
        arena, desc = torch.from_numpy(arena0).cuda(), torch.from_numpy(desc0).cuda()
        assert _same_bits(eng.preprocess_image_windows(arena, desc, 2).cpu(),
                          preprocess_image_windows(arena, desc, 2, 1, resize=E_RESIZE, crop=E_CROP, out_layout=eng.packed_layout).cpu())
    finally:
        eng.close()
