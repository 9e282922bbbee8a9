"""tsm_preprocess_windows (mixed-size windows from one arena through a device descriptor table, centre crop or person crop, one
launch) against the single-size entry points it must equal bit for bit, and StreamBatcher on a real engine.

Every launch runs in hostile memory (tests/_guard.py): arena and table between poisoned bands, the output poisoned before
the launch, bands and payload checked after it.  Shapes are the smallest that still take every path: 40 x 56, 56 x 40 (h > w),
52 x 90 and 36 x 36 (the resize exactly) frames, sizes 32 and 33 (33: a half-filled pixel pair ends every row of the bf16
layouts), 2 and 8 frames per window; windows start at 16-byte steps of the arena, so most are not 512-byte aligned.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _person_crop as pc
from tests._guard import POISON, check, guarded, guarded_out
from tests._stub import synthetic_video

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
I64_MAX = 2 ** 63 - 1
LAYOUTS = ['nthwc4', 'ntchw', 'nthwc8s', 'nthwc8b']


def _layout(name):
    from workoutdetector_amd import _lib
    return {'nthwc4': _lib.LAYOUT_NTHWC4, 'ntchw': _lib.LAYOUT_NTCHW, 'nthwc8s': _lib.LAYOUT_NTHWC8S, 'nthwc8b': _lib.LAYOUT_NTHWC8B}[name]


@functools.lru_cache(maxsize=None)
def _window(seed, t, h, w):
    """uint8 [t, h, w, 3] noise (shared between tests: never written)."""
    return pc.video(seed, t, h, w)


def _pack(windows, f32):
    """CPU windows [t, h, w, 3] -> (arena: one flat tensor of the pixel type, byte offsets), each window at the next multiple
    of 16 bytes; the gaps hold 0xA5 bytes."""
    elem = 4 if f32 else 1
    offsets, total = [], 0
    for w in windows:
        offsets.append(total)
        total += (w.numel() * elem + 15) // 16 * 16
    arena = torch.full((total,), 0xA5, dtype=torch.uint8)
    for w, off in zip(windows, offsets):
        src = (w.float() if f32 else w).contiguous().view(-1).view(torch.uint8)
        arena[off:off + src.numel()] = src
    return (arena.view(torch.float32) if f32 else arena), offsets


def _launch(arena, table, n_segment, size, layout, **kw):
    """engine.preprocess_windows in hostile memory; arena: CPU tensor, table: int32 ndarray [n, 8]."""
    from workoutdetector_amd.engine import _frame_shape, preprocess_windows
    src = guarded(arena.cuda(), name='arena')
    rows = guarded(torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).cuda(), name='desc')
    out = guarded_out((len(table), n_segment) + _frame_shape(layout, size), name='out')
    assert preprocess_windows(src, rows, len(table), n_segment, crop=size, layout=layout, out=out, **kw) is out
    torch.cuda.synchronize()
    check(src, rows, out)
    return out.cpu()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _frames_alone(window, f32, size, layout, resize):
    """preprocess_frames of one window staged alone, in hostile memory."""
    from workoutdetector_amd.engine import _frame_shape, preprocess_frames
    src = guarded((window.float() if f32 else window).cuda(), name='frames')
    out = guarded_out((window.shape[0],) + _frame_shape(layout, size), name='alone')
    preprocess_frames(src, resize=resize, crop=size, layout=layout, out=out)
    torch.cuda.synchronize()
    check(src, out)
    return out.cpu()


def _clips_alone(window, box, f32, size, layout):
    """preprocess_clips of one window staged alone: n_clips=1, clip_step=n_segment, clip_stride=1, total_frames=n_segment."""
    from workoutdetector_amd.engine import _frame_shape, preprocess_clips
    t = window.shape[0]
    src = guarded((window.float() if f32 else window).cuda(), name='frames')
    rows = guarded(torch.tensor([box or (0, 0, 0, 0)], dtype=torch.int32).cuda(), name='box')
    out = guarded_out((1, t) + _frame_shape(layout, size), name='alone')
    preprocess_clips(src, rows, 0, t, 0, 1, size=size, layout=layout, n_segment=t, clip_step=t, clip_stride=1, out=out)
    torch.cuda.synchronize()
    check(src, rows, out)
    return out.cpu()[0]


# ---- 1. centre crop, mixed shapes ------------------------------------------------------------------------------------------
SHAPES = [(40, 56), (56, 40), (52, 90), (36, 36)]


@pytest.mark.parametrize('layout_name', LAYOUTS)
@pytest.mark.parametrize('size', [32, 33])
def test_centre_crop_of_mixed_shapes_equals_preprocess_frames_per_window(hip_lib, size, layout_name):
    """Two windows per shape, interleaved in batch order; 2 and 8 frames per window; uint8 and float32 arenas; resize 36.
    Every window's rows equal preprocess_frames of that window alone bit for bit."""
    from workoutdetector_amd.transform import window_descriptors
    layout = _layout(layout_name)
    for n_segment in (2, 8):
        windows = [_window(100 * i + n_segment, n_segment, *SHAPES[i % 4]) for i in range(8)]
        for f32 in (False, True):
            arena, offsets = _pack(windows, f32)
            table = window_descriptors([tuple(w.shape[1:3]) for w in windows], offsets, resize=36, crop=size)
            got = _launch(arena, table, n_segment, size, layout, resize=36)
            for i, w in enumerate(windows):
                want = _frames_alone(w, f32, size, layout, 36)
                assert _same_bits(got[i], want), (i, tuple(w.shape), n_segment, f32)
            assert not _same_bits(got[0], got[4])          # (two windows of one shape hold different frames)


# ---- 2. person crop, mixed shapes ------------------------------------------------------------------------------------------
PC_SHAPES = [(40, 56), (57, 33)]


def _pc_cases(size):
    """24 windows: every box kind of boxes_for on each of the two shapes, the shapes alternating in batch order."""
    cases = []
    for kind in range(12):
        for s, (h, w) in enumerate(PC_SHAPES):
            cases.append((_window(1000 + 2 * kind + s, 8, h, w), pc.boxes_for(h, w, size)[kind]))
    return cases


@functools.lru_cache(maxsize=None)
def _pc_reference(size):
    """[24, 8, 3, size, size]: tests/_person_crop.py's torch composition on the CPU, once per size."""
    return torch.stack([pc.reference(w.permute(0, 3, 1, 2), box, size) for w, box in _pc_cases(size)])


@pytest.mark.parametrize('layout_name', LAYOUTS)
@pytest.mark.parametrize('size', [32, 33])
def test_person_crop_of_mixed_shapes_equals_preprocess_clips_and_the_torch_composition(hip_lib, size, layout_name):
    """Each window equals preprocess_clips on that window staged alone bit for bit (all layouts, uint8 and float32), and the
    fp32 layouts are within rtol 1e-5, atol 1e-4 of tests/_person_crop.py's reference."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.transform import window_descriptors
    layout = _layout(layout_name)
    cases = _pc_cases(size)
    windows, boxes = [w for w, _ in cases], [b for _, b in cases]
    for f32 in (False, True):
        arena, offsets = _pack(windows, f32)
        table = window_descriptors([tuple(w.shape[1:3]) for w in windows], offsets, boxes=boxes)
        got = _launch(arena, table, 8, size, layout, person_crop=True)
        for i, (w, box) in enumerate(cases):
            assert _same_bits(got[i], _clips_alone(w, box, f32, size, layout)), (i, tuple(w.shape), box, f32)
        if layout in (_lib.LAYOUT_NTCHW, _lib.LAYOUT_NTHWC4):
            val = got if layout == _lib.LAYOUT_NTCHW else got[..., :3].permute(0, 1, 4, 2, 3)
            want = _pc_reference(size)
            err = (val.double() - want.double()).abs()
            bound = 1e-5 * want.double().abs() + 1e-4
            print(f'{layout_name} size {size} f32={f32}: max err {float(err.max()):.3g}, max err / bound {float((err / bound).max()):.3g}')
            torch.testing.assert_close(val, want, rtol=1e-5, atol=1e-4)


# ---- 3. invalid descriptors beside valid ones ------------------------------------------------------------------------------
def _invalid_rows(arena_bytes, nbytes, h, w):
    """The invalid descriptors of tests/windows_host.cpp for a window of `nbytes` in an arena of `arena_bytes`."""
    def row(off, hh=h, ww=w, box=(5, 7, 20, 17)):
        off &= (1 << 64) - 1
        lo, hi = off & 0xFFFFFFFF, off >> 32
        return [lo - (1 << 32) if lo >= 1 << 31 else lo, hi - (1 << 32) if hi >= 1 << 31 else hi, hh, ww, *box]
    rows = [[e] * 8 for e in (I32_MIN, I32_MAX, 0)]
    for word in range(4):                                    # one edge value in one word of a valid descriptor
        for e in (I32_MIN, I32_MAX, 0):
            if word <= 1 and e == 0:
                continue                                     # (off_lo = 0 / off_hi = 0 is the valid descriptor itself)
            r = row(0)
            r[word] = e
            rows.append(r)
    rows += [row(-16), row(arena_bytes), row(arena_bytes - nbytes + 1), row(arena_bytes - nbytes + 16), row(I64_MAX), row(I64_MAX - 15),
             row(-2 ** 63), row(8), row(0, hh=65536), row(0, ww=65536), row(0, hh=-1), row(0, ww=-40)]
    return rows


@pytest.mark.parametrize('person_crop', [False, True])
def test_invalid_descriptors_give_zero_frames_and_leave_their_neighbours_alone(hip_lib, person_crop):
    """One launch: valid windows with every invalid descriptor between them.  Invalid windows are exactly the normalised zero
    frame, valid ones equal the launch without the invalid rows bit for bit, and every guard band is intact -- the frames'
    arena lies between poisoned bands, so a read the validity test should have stopped returns poison or trips nothing,
    never a plausible value.  The documented behaviour, exercised; not an attempt to fault."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.transform import window_descriptors
    h, w, size, t = 40, 56, 32, 8
    windows = [_window(2000 + i, t, h, w) for i in range(3)]
    boxes = [(5, 7, 20, 17), None, (-6, -9, 25, 30)]
    for f32 in (False, True):
        arena, offsets = _pack(windows, f32)
        arena_bytes = arena.numel() * arena.element_size()
        nbytes = windows[0].numel() * arena.element_size()
        assert offsets[2] == arena_bytes - nbytes                   # (the last valid window ends exactly at the arena's end)
        valid = window_descriptors([(h, w)] * 3, offsets, boxes=boxes if person_crop else None, resize=36, crop=size).tolist()
        bad = _invalid_rows(arena_bytes, nbytes, h, w)
        cut = len(bad) // 2
        table = np.array([valid[0]] + bad[:cut] + [valid[1]] + bad[cut:] + [valid[2]], dtype=np.int64).astype(np.int32)
        where_valid = [0, cut + 1, len(bad) + 2]
        for layout_name in LAYOUTS:
            layout = _layout(layout_name)
            kw = dict(person_crop=person_crop, resize=36)
            got = _launch(arena, table, t, size, layout, **kw)
            alone = _launch(arena, np.array(valid, dtype=np.int32), t, size, layout, **kw)
            zero = _launch(torch.zeros_like(arena), np.array(valid[:1], dtype=np.int32), t, size, layout, person_crop=True)[0]
            for i in range(len(table)):
                if i in where_valid:
                    assert _same_bits(got[i], alone[where_valid.index(i)]), (layout_name, i)
                    assert not _same_bits(got[i], zero)
                else:
                    assert _same_bits(got[i], zero), (layout_name, i, table[i].tolist())
            if layout == _lib.LAYOUT_NTCHW:                        # ... and that zero frame is (0 - mean) / std to the bit
                assert torch.equal(zero, pc.ZERO.view(1, 3, 1, 1).expand(t, 3, size, size))


def test_a_centre_crop_that_does_not_fit_is_refused_on_the_host_or_a_zero_frame(hip_lib):
    """The short side of a resized frame is `resize`, so a crop larger than the resized frame means crop > resize: the host
    refuses it before any launch (TSM_ERR_INVALID_ARG, the output untouched).  The device-side geometry test can only fail
    where the long side leaves int32 -- resize = INT32_MAX on a frame that is not square: that window is the zero frame, its
    square neighbours equal preprocess_frames with the same arguments bit for bit."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import _frame_shape, launch_trace, preprocess_windows
    size, t = 32, 2
    windows = [_window(3000, t, 36, 36), _window(3001, t, 40, 56), _window(3002, t, 36, 36)]
    arena, offsets = _pack(windows, False)
    table = np.array([[off, 0, w.shape[1], w.shape[2], 0, 0, 0, 0] for w, off in zip(windows, offsets)], dtype=np.int32)
    src = guarded(arena.cuda(), name='arena')
    rows = guarded(torch.from_numpy(table).cuda(), name='desc')
    out = guarded_out((3, t) + _frame_shape(_lib.LAYOUT_NTCHW, 36), name='out')
    with launch_trace() as tr:
        with pytest.raises(_lib.TsmError) as ei:
            preprocess_windows(src, rows, 3, t, resize=32, crop=36, layout=_lib.LAYOUT_NTCHW, out=out)
    assert ei.value.status == -1 and tr.kernels == []
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == POISON).all())
    check(src, rows)
    got = _launch(arena, table, t, size, _lib.LAYOUT_NTCHW, resize=I32_MAX)
    assert torch.equal(got[1], pc.ZERO.view(1, 3, 1, 1).expand(t, 3, size, size))
    for i in (0, 2):
        assert _same_bits(got[i], _frames_alone(windows[i], False, size, _lib.LAYOUT_NTCHW, I32_MAX)), i


def test_the_binding_refuses_malformed_tensors_and_one_launch_names_the_kernel(hip_lib):
    from workoutdetector_amd.engine import launch_trace, preprocess_windows
    arena, offsets = _pack([_window(1, 2, 40, 56)], False)
    dev = arena.cuda()
    table = torch.tensor([[0, 0, 40, 56, 0, 0, 0, 0]], dtype=torch.int32).cuda()
    for a, d in ((dev.cpu(), table), (dev, table.cpu()), (dev.to(torch.int16), table), (dev[1:], table), (dev, table.float()),
                 (dev, table.view(8)), (dev, table[:, :4])):
        with pytest.raises(ValueError):
            preprocess_windows(a, d, 1, 2, resize=36, crop=32)
    with pytest.raises(ValueError):
        preprocess_windows(dev, table, 0, 2)
    with launch_trace() as tr:
        preprocess_windows(dev, table, 1, 2, resize=36, crop=32)
    assert len(tr.kernels) == 1 and tr.ran('preprocess_windows_kernel<unsigned char>'), tr.kernels


# ---- 4. / 5. StreamBatcher on an engine -------------------------------------------------------------------------------------
def _make_engine(sd, poison=False):
    from workoutdetector_amd.engine import TsmEngine
    keep = {k: os.environ.get(k) for k in ('TSM_AUTOTUNE', 'TSM_POISON')}
    os.environ['TSM_AUTOTUNE'] = '0'
    os.environ.pop('TSM_POISON', None)
    if poison:
        os.environ['TSM_POISON'] = '1'
    try:
        return TsmEngine(num_class=12, num_segments=8, max_clips=8, state_dict=sd)       # (TSM_* are read in tsm_create)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope='module')
def engine(hip_lib, sd0):
    eng = _make_engine(sd0)
    yield eng
    eng.close()


VIDS = {'a': (31, 48, 90, 52, 24), 'b': (32, 40, 120, 68, 32), 'c': (33, 32, 90, 52, 20)}      # seed, frames, h, w, period


def _vid(k):
    seed, frames, h, w, period = VIDS[k]
    return synthetic_video(seed, frames, h, w, period=period)


def _box(k, t):
    """A made-up detector: (x1, y1, x2, y2) of frame t of stream k; stream 'c' has a window without any box (frames 8 .. 15)."""
    _, _, h, w, _ = VIDS[k]
    if k == 'c' and 8 <= t < 16:
        return None
    cx, cy = w * (0.5 + 0.25 * np.sin(t / 5.0)), h * (0.5 + 0.2 * np.cos(t / 7.0))
    return (cx - 0.35 * w, cy - 0.3 * h, cx + 0.3 * w + t % 3, cy + 0.35 * h)


def _play(model, max_batch, every, person_crop=False, spy=None):
    """Push the three streams frame by frame, step every `every` frames -> (events, results).  spy(windows, crops, logits)
    sees every batch.  threshold 0: every state is the arg-max class (the seed-0 classifier's softmax never reaches 0.5)."""
    from workoutdetector_amd.streaming import StreamBatcher
    sb = StreamBatcher(model, threshold=0.0, max_batch=max_batch, person_crop=person_crop)
    if spy is not None:
        inner = sb._logits

        def logits(windows, crops):
            out = inner(windows, crops)
            spy([torch.as_tensor(w).clone() for w in windows], list(crops), out)
            return out
        sb._logits = logits
    vids = {k: _vid(k) for k in VIDS}
    ev = {k: [] for k in vids}
    for t in range(max(len(v) for v in vids.values())):
        for k, v in vids.items():
            if t < len(v):
                sb.push(k, v[t], **(dict(box=_box(k, t)) if person_crop else {}))
        if t % every == every - 1:
            for k, e in sb.step().items():
                ev[k] += e
    for k, e in sb.step().items():
        ev[k] += e
    res = {k: sb.result(k) for k in vids}
    for k in vids:
        sb.close(k)
    assert sb.pinned_bytes == 0 and not sb._free
    return ev, res


def test_stream_batcher_runs_one_windows_launch_per_batch_and_matches_per_window_transforms(engine):
    """Three streams of two frame sizes, a step every 16 frames = up to 6 mixed-size windows.  Under launch_trace a step's
    batch shows exactly one preprocess_windows_kernel launch and no preprocess_kernel<; its logits equal per-window
    preprocess_frames + forward_device bit for bit; events and counts at max_batch=32 equal those at max_batch=1."""
    from workoutdetector_amd.engine import launch_trace, preprocess_frames
    batches = []
    with launch_trace() as tr:
        ev32, res32 = _play(engine, 32, 16, spy=lambda w, c, out: batches.append((w, out.clone())))
    mixed = [b for b in batches if len({tuple(w.shape) for w in b[0]}) > 1]
    assert len(batches) == 3 and len(mixed) >= 2 and max(len(b[0]) for b in batches) == 6
    assert tr.count('preprocess_windows_kernel') == len(batches), tr.kernels
    assert not tr.ran('preprocess_kernel<'), tr.kernels
    layout = engine.packed_layout
    for windows, got in batches:
        clips = torch.stack([preprocess_frames(w.cuda(), layout=layout) for w in windows])
        assert _same_bits(got.cpu(), engine.forward_device(clips, layout=layout).cpu())
        alone = torch.cat([engine.forward_device(c[None], layout=layout) for c in clips])
        assert _same_bits(got.cpu(), alone.cpu())
    n = []
    with launch_trace() as tr4:
        ev4, res4 = _play(engine, 4, 16, spy=lambda w, c, out: n.append(len(w)))
    assert n == [4, 2, 4, 2, 3] and tr4.count('preprocess_windows_kernel') == 5 and not tr4.ran('preprocess_kernel<'), (n, tr4.kernels)
    ev1, res1 = _play(engine, 1, 8)
    assert ev32 == ev4 == ev1 and res32 == res4 == res1
    assert all(len(ev32[k]) == VIDS[k][1] // 8 for k in VIDS)
    assert -1 not in {s for e in ev32.values() for _, s, _ in e}


class _HostRoute:
    """The engine behind the onnxruntime duck type only: StreamBatcher takes its torch path (PersonCropTransform on the CPU)."""

    def __init__(self, eng):
        self.eng = eng

    def get_inputs(self):
        return self.eng.get_inputs()

    def run(self, names, feed):
        return self.eng.run(names, feed)


def test_stream_batcher_person_crop_on_an_engine_equals_the_host_torch_route(engine, sd0):
    """person_crop=True: one preprocess_windows_kernel launch per batch; states and counts equal the host torch route on the
    same frames and boxes, the logits within the bound test_dataset_path_is_one_fused_launch_per_batch_and_matches_the_
    torch_transform holds the fused person crop to (rtol 1e-5, atol 1e-4); the same run under TSM_POISON=1 gives identical
    events."""
    from workoutdetector_amd.engine import launch_trace
    from workoutdetector_amd.transform import person_box
    dev_logits, host_logits, crops = [], [], []
    with launch_trace() as tr:
        ev, res = _play(engine, 4, 16, person_crop=True, spy=lambda w, c, out: (dev_logits.append(out.clone()), crops.extend(c)))
    assert tr.count('preprocess_windows_kernel') == 5 and not tr.ran('preprocess_kernel<') and not tr.ran('preprocess_clips'), tr.kernels
    want_c1 = None                                          # stream c's window 1 came without boxes: the whole frame
    assert crops[1] == person_box([_box('b', t) for t in range(8)]) and crops.count(want_c1) == 1
    ev_host, res_host = _play(_HostRoute(engine), 4, 16, person_crop=True,
                              spy=lambda w, c, out: host_logits.append(torch.from_numpy(np.asarray(out))))
    got, want = torch.cat(dev_logits).cpu().numpy(), torch.cat(host_logits).numpy()
    print(f'max |fused - torch| {np.abs(got - want).max():.3g}, logit scale {np.abs(want).max():.3g}')
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-4)
    assert ev == ev_host and res == res_host
    assert -1 not in {s for e in ev.values() for _, s, _ in e}
    eng = _make_engine(sd0, poison=True)
    try:
        ev_poison, res_poison = _play(eng, 4, 16, person_crop=True)
    finally:
        eng.close()
    assert ev_poison == ev and res_poison == res


def test_a_step_ends_in_one_states_launch_and_its_sync_recycles_every_window_buffer(engine):
    """Three windows in two batches: the step's last launch is its ONE scores_to_states_kernel, and the copy of those states --
    the step's only sync, behind every upload -- is followed by the recycling of all three page-locked window buffers."""
    from workoutdetector_amd.engine import launch_trace
    from workoutdetector_amd.streaming import StreamBatcher
    sb = StreamBatcher(engine, threshold=0.0, max_batch=2)
    vid = _vid('a')
    for t in range(24):
        sb.push('a', vid[t])
    assert sb.ready() == 3 and not sb._free and sb.pinned_bytes == 3 * 8 * 90 * 52 * 3
    with launch_trace() as tr:
        out = sb.step()
    assert tr.count('preprocess_windows_kernel') == 2 and tr.count('scores_to_states_kernel') == 1, tr.kernels
    assert 'scores_to_states_kernel' in tr.kernels[-1]
    assert not sb._inflight and len(sb._free[(90, 52, 3)]) == 3
    assert [w for w, _s, _c in out['a']] == [0, 1, 2]
    sb.close('a')
    assert sb.pinned_bytes == 0 and not sb._free
