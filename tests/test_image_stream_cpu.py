"""The image model on streams without a GPU: tsm_preprocess_windows' image mode (TSM_WINDOWS_IMAGE) -- the constant, the
kernel's integer geometry and descriptor verdicts under ASAN + UBSAN (tests/image_windows_host.cpp, a stand-alone program:
the functions the kernel inlines, on the CPU first), the entry point's host-side refusals, the descriptor builder and the
arena layout -- and ImageStreamBatcher on the host path of a stub model."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {(256, 224), (24, 16), (16, 15), (8, 8)}


def test_the_mode_is_a_constant_not_an_export():
    from workoutdetector_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'tsm_hip.h')).read()
    assert re.search(r'#define\s+TSM_WINDOWS_IMAGE\s+16\b', text) and _lib.WINDOWS_IMAGE == 16
    assert re.search(r'#define\s+TSM_ABI_VERSION\s+7\b', text) and _lib.ABI_VERSION == 7
    assert len(_lib.EXPORTS) == 44


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tests/image_windows_host.cpp built with ASAN + UBSAN (runtimes linked statically: the program runs as it is) and run
    once; returns (stdout, the geometry records int32 [n, 12])."""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    tmp = tmp_path_factory.mktemp('image_windows_host')
    exe, dump = str(tmp / 'image_windows_host'), str(tmp / 'geometry.bin')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-fno-omit-frame-pointer', '-Wall', '-Wextra', '-Werror',
           os.path.join(ROOT, 'tests', 'image_windows_host.cpp'), '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe, dump], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stdout + run.stderr
    return run.stdout, np.fromfile(dump, dtype=np.int32).reshape(-1, 12)


def test_integer_geometry_equals_the_python_transform(host_program):
    """Every (h, w) in 1 .. 300 squared at the four (resize, crop) pairs: nh, nw against resized_hw's rule, top and left against
    int(round((n - crop) / 2.0)), ksx and ksy against pil_ksize, the word count against image_tables(...).size; a window the
    program refused is one whose crop does not fit (no side of these is beyond the LDS)."""
    from workoutdetector_amd.transform import image_tables, pil_ksize, resized_hw
    stdout, rec = host_program
    assert 'image windows host ok' in stdout
    assert rec.shape[0] == 4 * 300 * 300
    assert {(int(r), int(c)) for r, c in np.unique(rec[:, 2:4], axis=0)} == PAIRS
    for h, w, resize, crop, ok, nh, nw, top, left, ksx, ksy, words in rec.tolist():
        want = resized_hw(h, w, resize)
        if crop > min(want):
            assert not ok, (h, w, resize, crop)
            continue
        assert ok and (nh, nw) == want, (h, w, resize, crop)
        assert (top, left) == (int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))), (h, w, resize, crop)
        assert ksx == (pil_ksize(w, nw) if nw != w else 0) and ksy == (pil_ksize(h, nh) if nh != h else 0), (h, w, resize, crop)
        assert words == image_tables.__wrapped__(h, w, resize, crop).size, (h, w, resize, crop)


def test_descriptor_verdicts_under_the_sanitizers(host_program):
    """INT32_MIN / INT32_MAX / 0 in every word, offsets -16, arena_bytes, arena_bytes - bytes + 1, an unaligned off and an
    unaligned tab, a tab whose block ends one word past the arena, sides of 65536, odd NV12 sides, the LDS cases, 200 000
    random descriptors against a 128-bit restatement of the rule: every verdict right (the program counts failures) and
    UBSAN silent (-fno-sanitize-recover: it would abort)."""
    stdout, _ = host_program
    assert 'FAIL' not in stdout and stdout.strip().endswith('image windows host ok')


def test_image_window_descriptors_layout_and_refusals():
    from workoutdetector_amd.transform import image_window_descriptors
    d = image_window_descriptors([(40, 56), (56, 40, 3), (24, 24)], [0, 6720, (1 << 32) + 16], [16384, (1 << 31) + 32, (5 << 32) + 0xFFFFFFF0],
                                 resize=24, crop=16)
    assert d.dtype == np.int32 and d.shape == (3, 8)
    assert d.tolist() == [[0, 0, 40, 56, 16384, 0, 0, 0], [6720, 0, 56, 40, -(1 << 31) + 32, 0, 0, 0], [16, 1, 24, 24, -16, 5, 0, 0]]
    assert image_window_descriptors([], [], []).shape == (0, 8)
    assert image_window_descriptors([(40, 56)], [0], [0], 24, 16, frame_format='nv12').tolist() == [[0, 0, 40, 56, 0, 0, 0, 0]]
    for kw in (dict(shapes=[(0, 8)], offsets=[0], table_offsets=[0]), dict(shapes=[(8, 65536)], offsets=[0], table_offsets=[0]),
               dict(shapes=[(8, 8, 4)], offsets=[0], table_offsets=[0]), dict(shapes=[(8.0, 8)], offsets=[0], table_offsets=[0]),
               dict(shapes=[(8, 8)], offsets=[-16], table_offsets=[0]), dict(shapes=[(8, 8)], offsets=[8], table_offsets=[0]),
               dict(shapes=[(8, 8)], offsets=[16.0], table_offsets=[0]), dict(shapes=[(8, 8)], offsets=[1 << 63], table_offsets=[0]),
               dict(shapes=[(8, 8)], offsets=[0, 16], table_offsets=[0]), dict(shapes=[(8, 8)], offsets=[0], table_offsets=[]),
               dict(shapes=[(8, 8)], offsets=[0], table_offsets=[-16]), dict(shapes=[(8, 8)], offsets=[0], table_offsets=[8]),
               dict(shapes=[(8, 8)], offsets=[0], table_offsets=[16.0]), dict(shapes=[(8, 8)], offsets=[0], table_offsets=[1 << 63]),
               dict(shapes=[(40, 56)], offsets=[0], table_offsets=[0], resize=16, crop=17),   # a crop larger than the resized frame
               dict(shapes=[(41, 56)], offsets=[0], table_offsets=[0], frame_format='nv12'),
               dict(shapes=[(40, 56, 3)], offsets=[0], table_offsets=[0], frame_format='nv12'),
               dict(shapes=[(40, 56)], offsets=[0], table_offsets=[0], frame_format='i420'),
               dict(shapes=[(40, 56)], offsets=[0], table_offsets=[0], frame_format='bgr')):
        with pytest.raises(ValueError):
            image_window_descriptors(**kw)


def test_image_window_arena_places_frames_then_one_block_per_geometry():
    from workoutdetector_amd.transform import image_tables, image_window_arena
    shapes = [(40, 56), (31, 90), (40, 56), (24, 24), (31, 90)]
    desc, offsets, tables, nbytes = image_window_arena(shapes, n_segment=2, resize=24, crop=16)
    assert offsets == [0, 13440, 13440 + 16752, 13440 + 16752 + 13440, 13440 + 16752 + 13440 + 3456]          # 2 x 31 x 90 x 3 = 16740 -> 16752
    end = offsets[-1] + 16752
    (t0, b0), (t1, b1) = tables                                     # 24 x 24 has no block
    assert t0 == end and b0 is image_tables(40, 56, 24, 16) and t1 == t0 + (b0.nbytes + 15) // 16 * 16 and b1 is image_tables(31, 90, 24, 16)
    assert nbytes == t1 + (b1.nbytes + 15) // 16 * 16 and nbytes % 16 == 0
    assert desc[:, :4].tolist() == [[o, 0, h, w] for o, (h, w) in zip(offsets, shapes)]
    assert desc[:, 4].tolist()[:3] == [t0, t1, t0] and desc[4, 4] == t1 and not desc[:, 5:].any()
    d, offs, tabs, n = image_window_arena([(40, 56)], resize=24, crop=16, frame_format='nv12')
    assert offs == [0] and tabs[0][0] == 3360 and d[0].tolist() == [0, 0, 40, 56, 3360, 0, 0, 0]
    assert image_window_arena([(24, 24)], resize=24, crop=16)[2:] == ([], 1728)


def test_invalid_arguments_are_refused_before_anything_touches_a_gpu():
    """The image mode's host-side refusals: scale_255 = 1 and crop > resize are TSM_ERR_INVALID_ARG, TSM_PIXEL_F32 and an I420
    code TSM_ERR_UNSUPPORTED, each with an empty launch trace.  Nothing is dereferenced on the host, so made-up addresses
    serve.  The values 2 and -1 of person_crop stay refused."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.build import build_library
    from workoutdetector_amd.engine import launch_trace
    build_library()
    lib = _lib.load()
    good = dict(arena=0x10000, arena_bytes=1 << 20, pixel=_lib.PIXEL_U8, desc=0x20000, n_windows=2, n_segment=1,
                person_crop=_lib.WINDOWS_IMAGE, out=0x30000, out_layout=_lib.LAYOUT_NTHWC4, resize=256, crop=224, scale_255=0, stream=None)
    bad = [(dict(scale_255=1), -1), (dict(resize=224, crop=225), -1), (dict(resize=24, crop=25), -1), (dict(pixel=_lib.PIXEL_F32), -7),
           (dict(pixel=_lib.PIXEL_I420_BT601), -7), (dict(pixel=_lib.PIXEL_UYVY_BT709_FULL), -7), (dict(pixel=2), -1),
           (dict(arena=None), -1), (dict(desc=0x20004), -1), (dict(arena_bytes=0), -1), (dict(n_windows=0), -1),
           (dict(out_layout=_lib.LAYOUT_NTHWC), -1), (dict(resize=30000, crop=21846), -7), (dict(person_crop=2), -1), (dict(person_crop=-1), -1),
           (dict(person_crop=17), -1)]
    for change, code in bad:
        args = dict(good, **change)
        with launch_trace() as tr:
            rc = lib.tsm_preprocess_windows(*args.values())
        assert rc == code, (change, rc)
        assert tr.kernels == [], (change, tr.kernels)


# ---- ImageStreamBatcher on the host path ---------------------------------------------------------------------------------------
class _Brightness(torch.nn.Module):
    """Two classes from the mean of the transformed frame: a bright frame is class 1."""
    image_resize, image_crop = 24, 16

    def forward(self, x):
        m = x.mean(dim=(1, 2, 3))
        return torch.stack([-m, m], dim=1)


def _blinking(seed, n, h, w, period=16):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    for a in range(seed % period, n, period):
        frames[a:a + period // 2] //= 5
    return frames


def _reference(model, frames):
    """(states, (count, reps)) of one stream's frames by the offline loop; frames of several sizes go frame by frame."""
    from workoutdetector_amd import inference_count as ic
    from workoutdetector_amd.counting import pred_to_count, vote_states
    if isinstance(frames, np.ndarray):
        return ic.image_states(model, frames)[0], ic.count_by_image_model(model, frames)
    preds = [int(ic.inference_image(model, f).argmax()) for f in frames]
    states = vote_states(preds)[0]
    return states, pred_to_count(states, step=7)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_three_streams_of_three_sizes_under_random_interleavings(seed):
    from workoutdetector_amd.streaming import ImageStreamBatcher
    model = _Brightness()
    vids = {'a': _blinking(3, 50, 30, 40), 'b': _blinking(8, 41, 40, 30), 'c': _blinking(13, 64, 24, 24)}
    want = {k: _reference(model, v) for k, v in vids.items()}
    assert all(w[1][0] >= 2 for w in want.values())                 # the videos do blink
    rng = np.random.default_rng(seed)
    seen = []
    sb = ImageStreamBatcher(model, max_batch=int(rng.integers(1, 9)), on_frame=lambda *a: seen.append(a))
    nxt, rows = {k: 0 for k in vids}, {k: [] for k in vids}
    while any(nxt[k] < len(vids[k]) for k in vids):
        k = str(rng.choice([k for k in vids if nxt[k] < len(vids[k])]))
        sb.push(k, vids[k][nxt[k]])
        nxt[k] += 1
        if rng.random() < 0.15:
            assert sb.ready() == sum(s.queued for s in sb.streams.values())
            for sid, r in sb.step().items():
                rows[sid] += r
            assert sb.ready() == 0
    for sid, r in sb.step().items():
        rows[sid] += r
    for k in vids:
        states, counted = want[k]
        assert [s for _, s, _ in rows[k]] == states == sb.streams[k].states
        assert [i for i, _, _ in rows[k]] == list(range(len(states)))
        assert rows[k][-1][2] == counted[0] and sb.result(k) == counted
        assert [a[1:] for a in seen if a[0] == k] == rows[k]
        assert sb.close(k) == counted
    assert not sb.streams


def test_a_stream_whose_frame_size_changes_and_close_with_queued_frames():
    from workoutdetector_amd.streaming import ImageStreamBatcher
    from workoutdetector_amd.transform import nv12_to_rgb, rgb_to_nv12
    model = _Brightness()
    parts = [_blinking(2, 20, 30, 40), _blinking(5, 17, 56, 24), _blinking(1, 12, 24, 24)]
    frames = [f for p in parts for f in p]
    states, counted = _reference(model, frames)
    assert counted[0] >= 1
    sb = ImageStreamBatcher(model, max_batch=5)
    other = _blinking(4, 30, 40, 30)
    for i, f in enumerate(frames):
        sb.push('x', f)
        if i < len(other):
            sb.push('y', other[i])
        if i == 25:
            sb.step()
    assert sb.ready() == len(frames) - 26 + len(other) - 26
    assert sb.close('x') == counted                                 # the queued frames are run, not dropped
    assert sb.ready() == 0 and list(sb.step()) == ['y']             # the rows of 'y' that close() ran come with the next step
    assert sb.streams['y'].states == _reference(model, other)[0] and sb.close('y') == _reference(model, other)[1]
    # NV12 surfaces on the host path: converted as they arrive, so the batcher equals an RGB one on the converted frames
    surfaces = [rgb_to_nv12(f)[0] for f in parts[0]]
    a, b = ImageStreamBatcher(model, frame_format='nv12', colorimetry='bt709'), ImageStreamBatcher(model)
    for s in surfaces:
        a.push(0, s)
        b.push(0, nv12_to_rgb(s, 'bt709')[0])
    assert a.step() == b.step() and a.close(0) == b.close(0)
    for bad in (np.zeros((30, 40), np.uint8), np.zeros((30, 40, 3), np.float32), np.zeros((30, 40, 4), np.uint8)):
        with pytest.raises(ValueError):
            sb.push('z', bad)
    with pytest.raises(ValueError):
        a.push(0, np.zeros((45, 41), np.uint8))                     # an odd width
    assert 'z' not in sb.streams


class _FakeEngine:
    """What the up-front checks read of an engine, and nothing that works."""
    packed_layout, num_segments, height, width, max_clips, consensus_type, tdn_depths = 2, 1, 224, 224, 8, 'avg', None

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def forward_device(self, *a, **k):
        raise AssertionError('nothing may run')


def test_every_up_front_refusal_comes_before_the_library_loads(monkeypatch):
    from workoutdetector_amd import _lib
    from workoutdetector_amd.streaming import ImageStreamBatcher

    def boom(*a, **k):
        raise AssertionError('the library must not load')
    monkeypatch.setattr(_lib, 'load', boom)
    with pytest.raises(ValueError, match='StreamBatcher'):
        ImageStreamBatcher(_FakeEngine(num_segments=8))
    with pytest.raises(NotImplementedError, match='TdnStreamBatcher'):
        ImageStreamBatcher(_FakeEngine(tdn_depths=(3, 4, 6, 3), num_segments=8))
    with pytest.raises(ValueError, match='identity'):
        ImageStreamBatcher(_FakeEngine(consensus_type='identity'))
    for fmt in ('i420', 'yv12', 'p010', 'yuyv', 'uyvy', 'bgr'):
        with pytest.raises(NotImplementedError):
            ImageStreamBatcher(_FakeEngine(), frame_format=fmt)
    with pytest.raises(ValueError):
        ImageStreamBatcher(_FakeEngine(), colorimetry='bt709')      # a colorimetry needs a YUV format
    with pytest.raises(ValueError):
        ImageStreamBatcher(_Brightness(), max_batch=0)
    sb = ImageStreamBatcher(_Brightness())
    with pytest.raises(ValueError):
        sb.push('s', np.zeros((40, 56, 3), np.uint8)[:, :, :2])
    model = _Brightness()
    model.image_resize, model.image_crop = 16, 17
    with pytest.raises(ValueError):
        ImageStreamBatcher(model).push('s', np.zeros((40, 56, 3), np.uint8))     # a crop larger than the resized frame


def test_the_three_batchers_ask_the_same_of_a_pushed_frame_in_the_same_words():
    """transform.pushed_frame behind StreamBatcher, ImageStreamBatcher and TdnStreamBatcher: one message per format, the luma
    size, conversion on arrival only when asked; a side of 0 pixels is ImageStreamBatcher's own refusal."""
    import re
    from tests._stub import StubModel
    from workoutdetector_amd.streaming import ImageStreamBatcher, StreamBatcher
    from workoutdetector_amd.tdn_pipeline import TdnStreamBatcher
    from workoutdetector_amd.transform import nv12_to_rgb, pushed_frame, rgb_to_nv12, rgb_to_yuv, yuv_to_rgb

    class Tdn:
        num_class, num_segments, height, width = 3, 8, 16, 16

    rgb_words = re.escape('frame must be uint8 [H,W,3], got ')
    for make in (lambda: StreamBatcher(StubModel()), lambda: ImageStreamBatcher(_Brightness()), lambda: TdnStreamBatcher(Tdn())):
        for bad in (np.zeros((30, 40), np.uint8), np.zeros((30, 40, 3), np.float32), np.zeros((30, 40, 4), np.uint8)):
            with pytest.raises(ValueError, match=rgb_words + re.escape(f'{bad.dtype} {bad.shape}')):
                make().push('s', bad)
    nv12_words = re.escape('an NV12 frame must be uint8 [3H/2,W], got ')
    for make in (lambda: StreamBatcher(StubModel(), frame_format='nv12'), lambda: ImageStreamBatcher(_Brightness(), frame_format='nv12')):
        for bad in (np.zeros((30, 40, 3), np.uint8), np.zeros((45, 40), np.int16)):
            with pytest.raises(ValueError, match=nv12_words + re.escape(f'{bad.dtype} {bad.shape}')):
                make().push('s', bad)
        with pytest.raises(ValueError, match=re.escape('NV12 frames are [3h/2, w] with h and w even, got 45 x 41')):
            make().push('s', np.zeros((45, 41), np.uint8))
    with pytest.raises(ValueError, match=re.escape('a yuyv frame must be its uint8 container [rows, bytes], got uint8 (30, 40, 3)')):
        StreamBatcher(StubModel(), frame_format='yuyv').push('s', np.zeros((30, 40, 3), np.uint8))
    with pytest.raises(ValueError, match=re.escape('i420 frames are [3h/2, w] with h and w even, got 45 x 41')):
        StreamBatcher(StubModel(), frame_format='i420').push('s', np.zeros((45, 41), np.uint8))
    # a side of 0: ImageStreamBatcher alone refuses it
    empty = np.zeros((0, 40, 3), np.uint8)
    with pytest.raises(ValueError, match=rgb_words):
        ImageStreamBatcher(_Brightness()).push('s', empty)
    StreamBatcher(StubModel()).push('s', empty)
    TdnStreamBatcher(Tdn()).push('s', empty)
    # what is queued: the frame as it is, or -- converted on arrival -- its RGB pixels; the luma size either way
    rgb = _blinking(1, 1, 30, 40)[0]
    nv12, p010 = rgb_to_nv12(rgb)[0], rgb_to_yuv(rgb, 'p010')[0]
    arr, hw = pushed_frame(rgb, 'rgb', None, False)
    assert arr is rgb and hw == (30, 40)
    arr, hw = pushed_frame(nv12, 'nv12', 'bt709', False)
    assert arr is nv12 and hw == (30, 40)
    arr, hw = pushed_frame(nv12, 'nv12', 'bt709', True)
    assert np.array_equal(arr, nv12_to_rgb(nv12, 'bt709')[0]) and hw == (30, 40)
    wide = p010.view('<u2')                                          # a 16-bit P010 frame is taken as its bytes
    arr, hw = pushed_frame(wide, 'p010', 'bt601', False)
    assert arr.dtype == np.uint8 and np.array_equal(arr, p010) and hw == (30, 40)
    assert np.array_equal(pushed_frame(wide, 'p010', 'bt601', True)[0], yuv_to_rgb(p010, 'p010', 'bt601')[0])
