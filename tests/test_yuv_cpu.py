"""I420, YV12, P010, YUYV and UYVY frames on the host: ``transform.yuv_to_rgb`` against ``nv12_to_rgb`` of the same samples and
against a per-pixel loop over the formula, the pad frame, the pixel codes against the header, the layout rules, the refusals that
come before the library is touched, the host-path equalities on a stub model, and tests/yuv_host.cpp under ASAN + UBSAN.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests._stub import StubModel, synthetic_video
from workoutdetector_amd import engine
from workoutdetector_amd import inference_count as ic
from workoutdetector_amd import transform as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ('i420', 'yv12', 'p010', 'yuyv', 'uyvy')
NAMES = ('bt601', 'bt709', 'bt601-full', 'bt709-full')


def _random_frames(seed, n, h, w, fmt):
    """Uniformly random bytes in the format's container (P010: random low bytes too)."""
    return np.random.default_rng(seed).integers(0, 256, size=(n,) + tf.frame_container(h, w, fmt), dtype=np.uint8)


# ---- names and codes ------------------------------------------------------------------------------------------------------------
def test_pixel_code_is_the_headers_enum():
    """_lib.pixel_code against include/tsm_hip.h, parsed from the file: 32 + 4 f + c, 20 new values, and the old ones unmoved."""
    from workoutdetector_amd import _lib
    with open(os.path.join(ROOT, 'include', 'tsm_hip.h')) as f:
        text = f.read()
    body = re.search(r'typedef enum tsm_pixel \{(.*?)\} tsm_pixel;', text, re.S).group(1)
    enum = {k: int(v) for k, v in re.findall(r'\b(TSM_PIXEL_\w+) = (\d+)', body)}
    assert len(enum) == 26 and sorted(enum.values()) == [0, 1, 16, 17, 18, 19] + list(range(32, 52))
    assert tf.YUV_FORMATS == FORMATS == _lib.YUV_FORMATS and tf.FRAME_FORMATS == ('rgb', 'nv12') + FORMATS
    for f, fmt in enumerate(FORMATS):
        for c, name in enumerate(NAMES):
            key = f'TSM_PIXEL_{fmt.upper()}_{name.upper().replace("-", "_")}'
            assert enum[key] == 32 + 4 * f + c == _lib.pixel_code(fmt, name) == getattr(_lib, key[4:]), key
        assert _lib.pixel_code(fmt) == _lib.pixel_code(fmt, None) == 32 + 4 * f          # (the default is 'bt601')
    for c, name in enumerate(NAMES):
        assert _lib.pixel_code('nv12', name) == _lib.nv12_pixel(name) == 16 + c
    assert _lib.pixel_code('rgb') == _lib.PIXEL_U8 == 0
    for fmt, name in (('yuv', 'bt601'), ('I420', 'bt601'), ('', 'bt601'), (None, 'bt601'), (32, 'bt601'), ('i420', 'bt2020'),
                      ('uyvy', 'BT601'), ('rgb', 'bt601')):
        with pytest.raises(ValueError):
            _lib.pixel_code(fmt, name)
    assert re.search(r'#define TSM_ABI_VERSION 7\b', text) and _lib.ABI_VERSION == 7
    assert 'HIGH byte' in text and 'Codes 2..15, 20..31 and 52 on are invalid' in text


def test_sizes_and_containers():
    for fmt, shape, nbytes in (('i420', (9, 8), 72), ('yv12', (9, 8), 72), ('p010', (9, 16), 144), ('yuyv', (6, 16), 96), ('uyvy', (6, 16), 96),
                               ('nv12', (9, 8), 72), ('rgb', (6, 8, 3), 144)):
        assert tf.frame_container(6, 8, fmt) == shape and tf.frame_bytes(6, 8, fmt) == nbytes == int(np.prod(shape))
        assert tf.frame_hw((5,) + shape, fmt) == (6, 8)
    assert tf.frame_container(3, 4, 'yuyv') == (3, 8) and tf.frame_hw((3, 8), 'uyvy') == (3, 4)       # an odd h is legal in 4:2:2
    for fmt in FORMATS:
        with pytest.raises(ValueError):
            tf.frame_container(4, 3, fmt)
        with pytest.raises(ValueError):
            tf.frame_container(0, 4, fmt)
    for fmt in ('i420', 'yv12', 'p010'):
        with pytest.raises(ValueError):
            tf.frame_container(3, 4, fmt)
    for fmt, bad in (('i420', (8, 8)), ('i420', (9, 7)), ('yv12', (10, 8)), ('p010', (9, 14)), ('p010', (8, 16)), ('yuyv', (6, 14)),
                     ('uyvy', (6, 15)), ('yuyv', (0, 16))):
        with pytest.raises(ValueError):
            tf.frame_hw(bad, fmt)
    with pytest.raises(ValueError):
        tf.frame_container(4, 4, 'yuv')


# ---- the conversion ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_planar_frames_convert_as_the_nv12_frame_of_the_same_planes(name):
    h, w = 6, 10
    i420 = _random_frames(1, 3, h, w, 'i420')
    u, v = i420[:, h:].reshape(3, 2, h // 2, w // 2)[:, 0], i420[:, h:].reshape(3, 2, h // 2, w // 2)[:, 1]
    nv = i420.copy()
    nv[:, h:] = np.stack([u, v], axis=-1).reshape(3, h // 2, w)
    want = tf.nv12_to_rgb(nv, name)
    assert np.array_equal(tf.yuv_to_rgb(i420, 'i420', name), want)
    yv12 = i420.copy()
    yv12[:, h:] = np.stack([v, u], axis=1).reshape(3, h // 2, w)
    assert np.array_equal(tf.yuv_to_rgb(yv12, 'yv12', name), want)
    assert not np.array_equal(tf.yuv_to_rgb(i420, 'yv12', name), want)              # (the same bytes read the other way differ)
    assert np.array_equal(tf.yuv_to_rgb(nv, 'nv12', name), want)
    assert np.array_equal(tf.yuv_to_rgb(i420[0], 'i420', name), want[:1])           # one frame


@pytest.mark.parametrize('name', NAMES)
def test_p010_converts_as_the_nv12_frame_of_its_high_bytes_whatever_the_low_bytes(name):
    h, w = 6, 10
    p = _random_frames(2, 3, h, w, 'p010')
    want = tf.nv12_to_rgb(np.ascontiguousarray(p[:, :, 1::2]), name)
    assert np.array_equal(tf.yuv_to_rgb(p, 'p010', name), want)
    for low in (0, 255):
        q = p.copy()
        q[:, :, 0::2] = low
        assert np.array_equal(tf.yuv_to_rgb(q, 'p010', name), want)
    words = p.view('<u2')                                                       # a 16-bit array is taken as its bytes
    assert words.shape == (3, 9, 10) and np.array_equal(tf.yuv_to_rgb(words, 'p010', name), want)
    assert np.array_equal(tf.yuv_to_rgb(torch.from_numpy(words.view(np.int16)), 'p010', name), want)


def _pixel_rgb(k, y, u, v):
    """tsm_host::nv12_pixel_rgb in Python integers (>> is arithmetic)."""
    y_off, cy, crv, cgu, cgv, cbu = k
    c, d, e = cy * (y - y_off) + 8192, u - 128, v - 128
    return [min(255, max(0, t >> 14)) for t in (c + crv * e, c + cgu * d + cgv * e, c + cbu * d)]


@pytest.mark.parametrize('fmt', ['yuyv', 'uyvy'])
def test_packed_frames_against_a_loop_over_the_formula(fmt):
    """Every pixel of 3 x 4 (an odd h) and 2 x 6 frames: Y its own byte, U and V those of its pair in the SAME row."""
    pos = {'yuyv': (0, 1, 2, 3), 'uyvy': (1, 0, 3, 2)}[fmt]                      # byte of (Y0, U, Y1, V) in a group
    for name in NAMES:
        k = tf.nv12_coefficients(name)
        for h, w in ((3, 4), (2, 6), (1, 2)):
            a = _random_frames(10 * h + w, 2, h, w, fmt)
            got = tf.yuv_to_rgb(a, fmt, name)
            assert got.shape == (2, h, w, 3) and got.dtype == np.uint8
            for n in range(2):
                for y in range(h):
                    for x in range(w):
                        g = a[n, y, 4 * (x // 2):4 * (x // 2) + 4]
                        want = _pixel_rgb(k, int(g[pos[2 * (x % 2)]]), int(g[pos[1]]), int(g[pos[3]]))
                        assert got[n, y, x].tolist() == want, (name, h, w, n, y, x)


def test_black_frame_is_rgb_zero_in_every_format_and_colorimetry():
    for fmt in ('nv12',) + FORMATS:
        for name in NAMES:
            for h, w in ((2, 2), (4, 6)) + (((1, 2), (3, 4)) if fmt in ('yuyv', 'uyvy') else ()):
                black = tf.black_frame(h, w, fmt, name)
                assert black.dtype == np.uint8 and black.shape == tf.frame_container(h, w, fmt)
                assert not tf.yuv_to_rgb(black, fmt, name).any(), (fmt, name)
                assert tf.yuv_to_rgb(np.zeros_like(black), fmt, name).any()     # zero bytes are green
            y, u, v = tf.yuv_planes(tf.black_frame(4, 6, fmt, name)[None], fmt)
            assert (y == tf.nv12_coefficients(name)[0]).all() and (u == 128).all() and (v == 128).all()
        if fmt == 'p010':
            assert not tf.black_frame(4, 6, fmt)[:, 0::2].any()                 # the values sit in the high byte
    assert np.array_equal(tf.black_frame(4, 6, 'nv12', 'bt709'), tf.nv12_black(4, 6, 'bt709'))
    assert not tf.black_frame(4, 6, 'rgb').any() and tf.black_frame(4, 6, 'rgb').shape == (4, 6, 3)
    for fmt, h, w in (('i420', 3, 4), ('yuyv', 4, 3), ('p010', 4, 5), ('yuv', 4, 4)):
        with pytest.raises(ValueError):
            tf.black_frame(h, w, fmt)


def test_rgb_to_yuv_round_trips_flat_pictures_and_agrees_between_formats():
    """rgb_to_yuv builds inputs: a flat picture comes back within the 8-bit quantisation, the 4:2:0 formats carry rgb_to_nv12's
    samples, and YUYV / UYVY are each other's byte swap."""
    rgb = np.random.default_rng(5).integers(0, 256, size=(2, 1, 1, 3), dtype=np.uint8).repeat(4, axis=1).repeat(6, axis=2)
    for name in ('bt601', 'bt709-full'):
        nv = tf.rgb_to_nv12(rgb, name)
        for fmt in ('nv12',) + FORMATS:
            a = tf.rgb_to_yuv(rgb, fmt, name)
            assert a.shape == (2,) + tf.frame_container(4, 6, fmt)
            back = tf.yuv_to_rgb(a, fmt, name).astype(int)
            assert np.abs(back - rgb).max() <= 3, (fmt, name)
            if fmt in ('nv12', 'i420', 'yv12', 'p010'):
                assert np.array_equal(tf.yuv_to_rgb(a, fmt, name), tf.nv12_to_rgb(nv, name))
        yuyv, uyvy = tf.rgb_to_yuv(rgb, 'yuyv', name), tf.rgb_to_yuv(rgb, 'uyvy', name)
        assert np.array_equal(yuyv.reshape(-1, 2)[:, ::-1].reshape(uyvy.shape), uyvy)
    with pytest.raises(ValueError):
        tf.rgb_to_yuv(np.zeros((3, 4, 3), dtype=np.uint8), 'i420')
    assert tf.rgb_to_yuv(np.zeros((3, 4, 3), dtype=np.uint8), 'yuyv').shape == (1, 3, 8)


def test_window_descriptors_take_each_formats_parity():
    for fmt in FORMATS:
        rows = tf.window_descriptors([(52, 90), (36, 36)], [0, 14048], resize=36, crop=32, frame_format=fmt)
        assert rows.tolist() == [[0, 0, 52, 90, 0, 0, 0, 0], [14048, 0, 36, 36, 0, 0, 0, 0]]
        for shape in ((52, 89), (52, 90, 3)):
            with pytest.raises(ValueError):
                tf.window_descriptors([shape], [0], resize=36, crop=32, frame_format=fmt)
        if fmt in ('yuyv', 'uyvy'):
            assert tf.window_descriptors([(51, 90)], [0], resize=36, crop=32, frame_format=fmt)[0, 2] == 51
        else:
            with pytest.raises(ValueError):
                tf.window_descriptors([(51, 90)], [0], resize=36, crop=32, frame_format=fmt)
    with pytest.raises(ValueError):
        tf.window_descriptors([(52, 90)], [0], frame_format='yuv')


# ---- refusals before the library is touched -------------------------------------------------------------------------------------
def test_refusals_before_the_gpu(tmp_path, monkeypatch):
    def no_gpu(*_a, **_k):
        raise AssertionError('the refusal must come before the library is touched')
    monkeypatch.setattr(engine._lib, 'load', no_gpu)
    from workoutdetector_amd.streaming import StreamBatcher
    rgb = torch.zeros((4, 40, 56, 3), dtype=torch.uint8)
    index = torch.zeros((1, 8), dtype=torch.int32)
    boxes = torch.zeros((1, 4), dtype=torch.int32)
    desc = torch.zeros((1, 8), dtype=torch.int32)
    calls = {'frames': lambda f, **kw: engine.preprocess_frames(f, **kw),
             'clips': lambda f, **kw: engine.preprocess_clips(f, boxes, 0, 8, 0, 1, **kw),
             'indexed': lambda f, **kw: engine.preprocess_indexed(f, index, **kw),
             'windows': lambda f, **kw: engine.preprocess_windows(f.view(-1), desc, 1, 4, **kw)}
    model = StubModel()
    for fmt in FORMATS:
        frames = torch.zeros((4,) + tf.frame_container(40, 56, fmt), dtype=torch.uint8)
        for what, call in calls.items():
            with pytest.raises(ValueError, match='colorimetry'):            # unknown colorimetry
                call(frames, frame_format=fmt, colorimetry='bt2020')
            with pytest.raises(ValueError, match='colorimetry'):            # a colorimetry with RGB frames
                call(rgb, frame_format='rgb', colorimetry='bt601')
            with pytest.raises(ValueError, match='frame_format'):           # unknown names ('yuv' stays refused)
                call(frames, frame_format='yuv')
            with pytest.raises(ValueError, match='frame_format'):
                call(frames, frame_format=fmt.upper())
            with pytest.raises(ValueError):                                 # a CPU tensor
                call(frames, frame_format=fmt)
            with pytest.raises(ValueError):                                 # wrong dtype
                call(frames.float(), frame_format=fmt)
            if what != 'windows':
                with pytest.raises(ValueError):                             # wrong rank
                    call(frames[0], frame_format=fmt)
                with pytest.raises(ValueError):                             # an RGB tensor given as this format
                    call(rgb, frame_format=fmt)
        # parity, as the shape of the container says it (checked before the device is: these are CPU tensors of a bad shape)
        bad_shapes = {'i420': [(61, 56), (60, 55)], 'yv12': [(61, 56), (60, 55)], 'p010': [(61, 112), (60, 110)], 'yuyv': [(40, 110)],
                      'uyvy': [(40, 109)]}[fmt]
        for shape in bad_shapes:
            with pytest.raises(ValueError):
                tf.frame_hw((4,) + shape, fmt)
            with pytest.raises(ValueError):
                ic.stage_video(model, torch.zeros((4,) + shape, dtype=torch.uint8), frame_format=fmt)
            with pytest.raises(ValueError):
                StreamBatcher(model, frame_format=fmt).push('x', np.zeros(shape, dtype=np.uint8))
        for kw in (dict(frame_format=fmt, colorimetry='bt2020'), dict(colorimetry='bt601'), dict(frame_format='yuv')):
            with pytest.raises(ValueError):
                ic.stage_video(model, frames, **kw)
            with pytest.raises(ValueError):
                ic.video_clip_logits(model, frames, tf.TestTransform(), **kw)
            with pytest.raises(ValueError):
                StreamBatcher(model, **kw)
            with pytest.raises(ValueError):
                ic.inference_dataset(model, ['test'], str(tmp_path / 'out'), 'ckpt', data_root=str(tmp_path), **kw)
        with pytest.raises(ValueError):
            ic.stage_video(model, rgb, frame_format=fmt)                    # an RGB video given as this format
        with pytest.raises(ValueError):
            ic.stage_video(model, frames.float(), frame_format=fmt)
        with pytest.raises(ValueError):
            StreamBatcher(model, frame_format=fmt).push('x', np.zeros((40, 56, 3), dtype=np.uint8))
        with pytest.raises(NotImplementedError, match='global'):
            ic.inference_dataset(model, ['test'], str(tmp_path / 'out'), 'ckpt', data_root=str(tmp_path), frame_format=fmt, shard='global')
    assert not (tmp_path / 'out').exists()


# ---- staging and the host path on a stub model ------------------------------------------------------------------------------------
def _video(seed, frames, h, w, fmt, name='bt601'):
    return torch.from_numpy(tf.rgb_to_yuv(synthetic_video(seed, frames, h, w), fmt, name))


class _DeviceModel(StubModel):
    """A stub that claims the device path (the predicate is monkeypatched): nothing of it runs in these tests."""
    packed_layout = 2


@pytest.mark.parametrize('fmt', FORMATS)
def test_the_pad_frame_of_a_staged_range_is_black_frame(monkeypatch, fmt):
    def upload(shape, fill, dev, stream=None, pool=None):
        pinned = torch.full(tuple(shape), 0x5A, dtype=torch.uint8)
        fill(pinned)
        return pinned, None
    monkeypatch.setattr(ic.staging, 'device_path', lambda model: isinstance(model, _DeviceModel))
    monkeypatch.setattr(ic.staging, 'engine_device', lambda model: torch.device('cpu') if isinstance(model, _DeviceModel) else None)
    monkeypatch.setattr(ic.staging, 'upload', upload)
    name = 'bt709'
    vid = _video(3, 21, 8, 12, fmt, name)                              # 21 frames: clips at 0, 8, 16; the last two have padded tails
    st = ic.stage_video(_DeviceModel(), vid, frame_format=fmt, colorimetry=name)
    assert st.on_device and st.frame_format == fmt and st.colorimetry == name and st.hw == (8, 12)
    assert (st.total, st.lo, st.hi, st.f_lo) == (21, 0, 3, 0) and tuple(st.frames.shape) == (12,) + tf.frame_container(8, 12, fmt)
    assert torch.equal(st.frames[:-1], vid[0::2])
    assert np.array_equal(st.frames[-1].numpy(), tf.black_frame(8, 12, fmt, name)) and st.frames[-1].any()
    assert not tf.yuv_to_rgb(st.frames[-1].numpy(), fmt, name).any()


def _boxes(video_name, clip):
    return [(2, 3, 20, 30), None, (-5, -7, 40, 66), (10, 20, 50, 40)][clip % 4]


@pytest.mark.parametrize('fmt', FORMATS)
def test_stage_video_and_video_clip_logits_equal_the_rgb_run_on_the_converted_video(fmt):
    """A model without a device path: yuv_to_rgb on the host, then exactly the RGB path.  29 frames: clips at 0, 8, 16, 24, the
    last two with padded tails."""
    model = StubModel()
    name = 'bt709'
    vid = _video(7, 29, 40, 56, fmt, name)
    rgb = torch.from_numpy(tf.yuv_to_rgb(vid, fmt, name))
    st, st_rgb = ic.stage_video(model, vid, None, None, fmt, name), ic.stage_video(model, rgb)
    assert st.frame_format == 'rgb' and st.hw == st_rgb.hw == (40, 56) and torch.equal(st.frames, st_rgb.frames)
    for transform in (tf.TestTransform(size=36, crop=32), tf.PersonCropTransform(_boxes, size=32)):
        want = ic.video_clip_logits(model, rgb, transform, batch_clips=3, video_name='v')
        got = ic.video_clip_logits(model, vid, transform, batch_clips=3, video_name='v', frame_format=fmt, colorimetry=name)
        assert tuple(got.shape) == (4, 12) and torch.equal(got, want)
    if fmt == 'p010':                                                   # a 16-bit video is taken as its bytes
        words = vid.view(torch.int16)
        assert tuple(words.shape) == (29, 60, 56)
        assert torch.equal(ic.video_clip_logits(model, words, tf.TestTransform(size=36, crop=32), frame_format=fmt, colorimetry=name),
                           ic.video_clip_logits(model, rgb, tf.TestTransform(size=36, crop=32)))


@pytest.mark.parametrize('fmt', FORMATS)
def test_stream_batcher_equals_the_rgb_batcher_on_the_converted_frames(fmt):
    from workoutdetector_amd.streaming import StreamBatcher
    vids = {'a': _video(11, 16, 40, 56, fmt), 'b': _video(12, 9, 52, 36, fmt)}
    for person_crop in (False, True):
        got = StreamBatcher(StubModel(), threshold=0.0, max_batch=2, person_crop=person_crop, frame_format=fmt, colorimetry='bt601')
        want = StreamBatcher(StubModel(), threshold=0.0, max_batch=2, person_crop=person_crop)
        ev_got, ev_want = {}, {}
        for t in range(16):
            for k, v in vids.items():
                if t < len(v):
                    kw = dict(box=(3 + t % 5, 4, 30, 33 + t % 3)) if person_crop and k == 'a' else {}
                    got.push(k, v[t].numpy(), **kw)
                    want.push(k, tf.yuv_to_rgb(v[t].numpy(), fmt)[0], **kw)
            if t % 8 == 7:
                for ev, sb in ((ev_got, got), (ev_want, want)):
                    for k, e in sb.step().items():
                        ev.setdefault(k, []).extend(e)
        assert ev_got == ev_want and {k: len(e) for k, e in ev_got.items()} == {'a': 2, 'b': 1}
        assert all(got.result(k) == want.result(k) for k in vids)
        assert [s.states for s in got.streams.values()] == [s.states for s in want.streams.values()]


# ---- the host program -------------------------------------------------------------------------------------------------------------
def test_host_arithmetic_under_sanitizers(tmp_path):
    """tests/yuv_host.cpp built with ASAN + UBSAN (runtimes linked statically: the program runs as it is) and run once."""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'yuv_host')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-fno-omit-frame-pointer', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'yuv_host.cpp'),
           '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stdout + run.stderr and 'yuv_host ok' in run.stdout
