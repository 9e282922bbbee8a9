"""NV12 frames on the host: the integer conversion (transform.nv12_to_rgb) against the float64 matrices and Pillow, the layout
rules, what the staged-video path stages, the host-path equalities on a stub model, the refusals that come before the library
is touched, the header, and tests/nv12_host.cpp under ASAN + UBSAN.  No GPU."""
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
TABLE = {'bt601': (16, 16, 19077, 26149, -6419, -13320, 33050), 'bt709': (17, 16, 19077, 29372, -3494, -8731, 34610),
         'bt601-full': (18, 0, 16384, 22970, -5638, -11700, 29032), 'bt709-full': (19, 0, 16384, 25802, -3069, -7670, 30402)}
MATRIX = {'bt601': (0.299, 0.114, True), 'bt709': (0.2126, 0.0722, True), 'bt601-full': (0.299, 0.114, False),
          'bt709-full': (0.2126, 0.0722, False)}
ZERO_GREEN = {'bt601': 136, 'bt709': 77, 'bt601-full': 135, 'bt709-full': 84}


def test_names_codes_and_coefficients_are_the_issues_table():
    from workoutdetector_amd import _lib
    assert tf.COLORIMETRIES == tuple(TABLE)
    for name, row in TABLE.items():
        assert _lib.nv12_pixel(name) == row[0] and tf.nv12_coefficients(name) == row[1:]
    assert (_lib.PIXEL_NV12_BT601, _lib.PIXEL_NV12_BT709, _lib.PIXEL_NV12_BT601_FULL, _lib.PIXEL_NV12_BT709_FULL) == (16, 17, 18, 19)
    for bad in ('bt2020', 'BT601', '', None, 16):
        with pytest.raises(ValueError):
            tf.nv12_coefficients(bad)
        with pytest.raises(ValueError):
            _lib.nv12_pixel(bad)


# ---- the formula --------------------------------------------------------------------------------------------------------------
def _triples():
    """The fixed set of (Y, U, V) the formula is checked on: every Y with U, V on the lattice 3, 7, .., 255 (1/16 of the 2^24
    triples: the full set costs several seconds and a GB of float64), plus all 2^16 (U, V) with Y in {0, 16, 235, 255}, as quads
    [Q, 4] of luma values that share one pair."""
    lat = np.arange(3, 256, 4)
    q, u, v = np.meshgrid(np.arange(64), lat, lat, indexing='ij')
    quads = [(4 * q.reshape(-1, 1) + np.arange(4)), ]
    us, vs = [u.reshape(-1)], [v.reshape(-1)]
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    quads.append(np.broadcast_to(np.array([0, 16, 235, 255]), (65536, 4)))
    us.append(u.reshape(-1))
    vs.append(v.reshape(-1))
    return np.concatenate(quads).astype(np.uint8), np.concatenate(us).astype(np.uint8), np.concatenate(vs).astype(np.uint8)


def _as_frame(quads, u, v):
    """One NV12 frame [3, 2Q] whose block b holds the four luma values quads[b] and the pair (u[b], v[b])."""
    n = len(u)
    frame = np.empty((3, 2 * n), dtype=np.uint8)
    frame[0] = quads[:, 0:2].reshape(-1)
    frame[1] = quads[:, 2:4].reshape(-1)
    frame[2, 0::2], frame[2, 1::2] = u, v
    return frame


def _float_rgb(name, y, u, v):
    """float64 [N, 3]: the matrix of the colorimetry, exact coefficients from (Kr, Kb), no rounding, no clamp."""
    kr, kb, limited = MATRIX[name]
    kg = 1.0 - kr - kb
    ys, cs, y_off = (255.0 / 219.0, 255.0 / 224.0, 16.0) if limited else (1.0, 1.0, 0.0)
    c, d, e = (y.astype(np.float64) - y_off) * ys, (u.astype(np.float64) - 128.0) * cs, (v.astype(np.float64) - 128.0) * cs
    return np.stack([c + 2.0 * (1.0 - kr) * e, c - 2.0 * kb * (1.0 - kb) / kg * d - 2.0 * kr * (1.0 - kr) / kg * e,
                     c + 2.0 * (1.0 - kb) * d], axis=-1)


@pytest.fixture(scope='module')
def triples():
    quads, u, v = _triples()
    frame = _as_frame(quads, u, v)
    frame.setflags(write=False)
    # per pixel, in the frame's raster order: (dy, block, dx)
    y = np.stack([quads[:, 0:2], quads[:, 2:4]]).reshape(2, -1)
    return frame, y, np.broadcast_to(u.repeat(2), y.shape), np.broadcast_to(v.repeat(2), y.shape)


@pytest.mark.parametrize('name', list(TABLE))
def test_the_integer_formula_is_within_one_of_the_float64_matrix(triples, name):
    frame, y, u, v = triples
    got = tf.nv12_to_rgb(frame, name)
    assert got.shape == (1, 2, frame.shape[1], 3) and got.dtype == np.uint8
    want = np.clip(np.floor(_float_rgb(name, y, u, v) + 0.5), 0, 255).astype(np.int32)
    diff = np.abs(got[0].astype(np.int32) - want)
    share = (diff != 0).reshape(-1, 3).mean(axis=0)
    print(f'{name}: {y.size} triples, max |int - float64| {diff.max()}, differing share per channel {share}')
    assert diff.max() <= 1
    assert (share <= 0.005).all(), share


@pytest.mark.parametrize('name', list(TABLE))
def test_black_and_white_are_exact_and_zero_bytes_are_not_black(name):
    y_off = TABLE[name][1]
    assert not tf.nv12_to_rgb(tf.nv12_black(4, 6, name), name).any()
    black = tf.nv12_black(4, 6, name)
    assert black.shape == (6, 6) and (black[:4] == y_off).all() and (black[4:] == 128).all()
    white = np.full((6, 6), 128, dtype=np.uint8)
    white[:4] = 235 if MATRIX[name][2] else 255
    assert (tf.nv12_to_rgb(white, name) == 255).all()
    zero = tf.nv12_to_rgb(np.zeros((6, 6), dtype=np.uint8), name)
    assert (zero == np.array([0, ZERO_GREEN[name], 0], dtype=np.uint8)).all()


def test_bt601_full_is_within_one_of_pillow_everywhere(triples):
    """Pillow's YCbCr -> RGB tables keep 6 fractional bits, so equality is not to be expected: within 1 on every triple."""
    Image = pytest.importorskip('PIL.Image')
    frame, y, u, v = triples
    got = tf.nv12_to_rgb(frame, 'bt601-full')[0].reshape(-1, 3).astype(np.int32)
    ycc = np.ascontiguousarray(np.stack([y.reshape(-1), u.reshape(-1), v.reshape(-1)], axis=-1)[None])
    want = np.asarray(Image.fromarray(ycc, 'YCbCr').convert('RGB'))[0].astype(np.int32)
    diff = np.abs(got - want)
    print(f'bt601-full vs Pillow: max {diff.max()}, differing share per channel {(diff != 0).mean(axis=0)}')
    assert diff.max() <= 1


@pytest.mark.parametrize('name', list(TABLE))
def test_rgb_to_nv12_and_back_returns_a_blockwise_constant_frame_within_two(name):
    """How the 2 comes about.  rgb_to_nv12 rounds each of Y, U, V once, by at most 0.5 code units; the chroma mean of a
    constant block is exact.  The inverse matrix carries those into a channel with its row's absolute sum: at most
    0.5 * (255/219 + 2 (1 - Kb) 255/224) = 0.5 * (1.164 + 2.112) = 1.64 (blue, limited BT.709).  nv12_to_rgb then rounds once
    more (0.5) with coefficients rounded to 2^-14 (255 * 3 * 2^-15 < 0.03): below 2.2 in all, the difference is an integer,
    and the clamp only moves a value towards the original, which lies in 0 .. 255.  So: within 2."""
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, size=(3, 8, 9, 3), dtype=np.uint8).repeat(2, axis=1).repeat(2, axis=2)
    rgb[0, :2, :2] = 0
    rgb[0, :2, 2:4] = 255
    nv12 = tf.rgb_to_nv12(rgb, name)
    assert nv12.shape == (3, 24, 18) and nv12.dtype == np.uint8
    back = tf.nv12_to_rgb(nv12, name)
    diff = np.abs(back.astype(np.int32) - rgb.astype(np.int32))
    print(f'{name}: round trip max {diff.max()}')
    assert diff.max() <= 2
    assert np.array_equal(tf.rgb_to_nv12(rgb[1], name), nv12[1:2])              # (one frame [h, w, 3] -> [1, 3h/2, w])


def test_layout_errors():
    ok = np.zeros((6, 4), dtype=np.uint8)
    assert tf.nv12_to_rgb(ok).shape == (1, 4, 4, 3) and tf.nv12_to_rgb(ok[None].repeat(2, 0)).shape == (2, 4, 4, 3)
    assert tf.nv12_luma_hw((9, 6, 4)) == (4, 4) and tf.frame_hw((9, 6, 4), 'nv12') == (4, 4) and tf.frame_hw((9, 6, 4, 3)) == (6, 4)
    assert tf.frame_bytes(4, 6, 'nv12') == 36 and tf.frame_bytes(4, 6) == 72
    for shape in ((6, 5), (7, 4), (5, 4), (8, 4), (4, 4), (0, 4), (6, 0)):      # odd w; rows no multiple of 3 (an odd h among them)
        with pytest.raises(ValueError):
            tf.nv12_to_rgb(np.zeros(shape, dtype=np.uint8))
    for bad in (np.zeros((6, 4), dtype=np.float32), np.zeros((1, 1, 6, 4), dtype=np.uint8), np.zeros((6,), dtype=np.uint8)):
        with pytest.raises(ValueError):
            tf.nv12_to_rgb(bad)
    for shape in ((5, 4, 3), (4, 5, 3), (4, 4, 4), (4, 4)):
        with pytest.raises(ValueError):
            tf.rgb_to_nv12(np.zeros(shape, dtype=np.uint8))
    for h, w in ((3, 4), (4, 3), (0, 4)):
        with pytest.raises(ValueError):
            tf.nv12_black(h, w)
    with pytest.raises(ValueError):
        tf.nv12_to_rgb(ok, 'bt2020')


def test_window_descriptors_accept_even_nv12_windows_only():
    rows = tf.window_descriptors([(52, 90), (36, 36)], [0, 7024], resize=36, crop=32, frame_format='nv12')
    assert rows.tolist() == [[0, 0, 52, 90, 0, 0, 0, 0], [7024, 0, 36, 36, 0, 0, 0, 0]]
    assert np.array_equal(rows, tf.window_descriptors([(52, 90), (36, 36)], [0, 7024], resize=36, crop=32))
    for shape in ((51, 90), (52, 89), (52, 90, 3)):
        with pytest.raises(ValueError):
            tf.window_descriptors([shape], [0], resize=36, crop=32, frame_format='nv12')
    with pytest.raises(ValueError):
        tf.window_descriptors([(52, 90)], [0], frame_format='yuv')


# ---- staging ------------------------------------------------------------------------------------------------------------------
def _nv12_video(seed, frames, h, w, name='bt601'):
    return torch.from_numpy(tf.rgb_to_nv12(synthetic_video(seed, frames, h, w), name))


class _DeviceModel(StubModel):
    """A stub that claims the device path (the predicate is monkeypatched): nothing of it runs in these tests."""
    packed_layout = 2


def _fake_device_path(monkeypatch):
    def upload(shape, fill, dev, stream=None, pool=None):
        pinned = torch.full(tuple(shape), 0x5A, dtype=torch.uint8)
        fill(pinned)
        return pinned, None
    monkeypatch.setattr(ic.staging, 'device_path', lambda model: isinstance(model, _DeviceModel))
    monkeypatch.setattr(ic.staging, 'engine_device', lambda model: torch.device('cpu') if isinstance(model, _DeviceModel) else None)
    monkeypatch.setattr(ic.staging, 'upload', upload)


@pytest.mark.parametrize('name', ['bt601', 'bt709-full'])
def test_the_pad_frame_of_a_staged_nv12_range_is_black_not_zero_bytes(monkeypatch, name):
    _fake_device_path(monkeypatch)
    vid = _nv12_video(3, 21, 8, 12, name)                              # 21 frames: clips at 0, 8, 16; the last two have padded tails
    st = ic.stage_video(_DeviceModel(), vid, frame_format='nv12', colorimetry=name)
    assert st.on_device and st.frame_format == 'nv12' and st.colorimetry == name and st.hw == (8, 12)
    assert (st.total, st.lo, st.hi, st.f_lo) == (21, 0, 3, 0) and tuple(st.frames.shape) == (12, 12, 12)
    assert torch.equal(st.frames[:-1], vid[0::2])
    assert np.array_equal(st.frames[-1].numpy(), tf.nv12_black(8, 12, name)) and st.frames[-1].any()
    assert not tf.nv12_to_rgb(st.frames[-1].numpy(), name).any()
    rgb = ic.stage_video(_DeviceModel(), torch.from_numpy(synthetic_video(3, 21, 8, 12)))
    assert rgb.frame_format == 'rgb' and rgb.colorimetry is None and not rgb.frames[-1].any()     # (RGB: the zero frame, as before)


def test_an_oversized_nv12_video_is_cut_by_its_real_bytes_per_frame(monkeypatch):
    _fake_device_path(monkeypatch)
    h, w = 8, 12
    vid = _nv12_video(4, 80, h, w)
    monkeypatch.setattr(ic, 'MAX_STAGE_BYTES', 16 * 3 * h * w // 2)      # 16 NV12 frames: clips_per_piece gives 2 clips (8 as RGB: 1)
    st = ic.stage_video(_DeviceModel(), vid, frame_format='nv12')
    assert not st.on_device and st.frame_format == 'nv12' and st.colorimetry == 'bt601' and tuple(st.frames.shape) == (40, 12, 12)
    asked, pieces = [], []
    real = ic.clips_per_piece

    def spy(per_frame_bytes):
        asked.append(per_frame_bytes)
        return real(per_frame_bytes)

    def stage(dev, total, lo, hi, f_lo, hw, even, stream=None, frame_format='rgb', colorimetry=None):
        pieces.append((lo, hi, f_lo, tuple(even.shape), frame_format, colorimetry))
        return ic.StagedVideo(total, lo, lo, f_lo, hw, even[:0], False)         # (an empty range: nothing runs behind it)
    monkeypatch.setattr(ic, 'clips_per_piece', spy)
    monkeypatch.setattr(ic, '_stage', stage)
    out = ic.staged_clip_logits(_DeviceModel(), st, tf.TestTransform(size=8, crop=8))
    assert asked == [3 * h * w // 2] and real(3 * h * w // 2) == 2 and real(3 * h * w) == 1
    assert [p[:2] for p in pieces] == [(a, min(a + 2, 10)) for a in range(0, 10, 2)]
    assert all(p[4:] == ('nv12', 'bt601') and p[3][1:] == (12, 12) for p in pieces)
    assert tuple(out.shape) == (0, 12)


# ---- host-path equality on a stub model -----------------------------------------------------------------------------------------
def _boxes(video_name, clip):
    return [(2, 3, 20, 30), None, (-5, -7, 40, 66), (10, 20, 50, 40)][clip % 4]


@pytest.mark.parametrize('name', ['bt601', 'bt709'])
def test_video_clip_logits_on_nv12_equals_the_rgb_call_on_the_converted_video(name):
    """A model without a device path: nv12_to_rgb on the host, then exactly the RGB path.  29 frames: clips at 0, 8, 16, 24, the
    last two with padded tails."""
    model = StubModel()
    vid = _nv12_video(7, 29, 40, 56, name)
    rgb = torch.from_numpy(tf.nv12_to_rgb(vid, name))
    for transform in (tf.TestTransform(size=36, crop=32), tf.PersonCropTransform(_boxes, size=32)):
        want = ic.video_clip_logits(model, rgb, transform, batch_clips=3, video_name='v')
        got = ic.video_clip_logits(model, vid, transform, batch_clips=3, video_name='v', frame_format='nv12', colorimetry=name)
        assert tuple(got.shape) == (4, 12) and torch.equal(got, want)
        part = ic.video_clip_logits(model, vid, transform, (1, 3), video_name='v', frame_format='nv12', colorimetry=name)
        assert torch.equal(part, want[1:3])
    other = ic.video_clip_logits(model, vid, tf.TestTransform(size=36, crop=32), frame_format='nv12',
                                 colorimetry='bt601-full')
    assert not torch.equal(other, ic.video_clip_logits(model, rgb, tf.TestTransform(size=36, crop=32)))


def test_stream_batcher_on_nv12_equals_the_rgb_batcher_on_the_converted_frames():
    from workoutdetector_amd.streaming import StreamBatcher
    vids = {'a': _nv12_video(11, 24, 40, 56), 'b': _nv12_video(12, 17, 52, 36)}
    for person_crop in (False, True):
        got = StreamBatcher(StubModel(), threshold=0.0, max_batch=2, person_crop=person_crop, frame_format='nv12', colorimetry='bt601')
        want = StreamBatcher(StubModel(), threshold=0.0, max_batch=2, person_crop=person_crop)
        ev_got, ev_want = {}, {}
        for t in range(24):
            for k, v in vids.items():
                if t < len(v):
                    kw = dict(box=(3 + t % 5, 4, 30, 33 + t % 3)) if person_crop and k == 'a' else {}
                    got.push(k, v[t].numpy(), **kw)
                    want.push(k, tf.nv12_to_rgb(v[t].numpy())[0], **kw)
            if t % 8 == 7:
                for ev, sb in ((ev_got, got), (ev_want, want)):
                    for k, e in sb.step().items():
                        ev.setdefault(k, []).extend(e)
        assert ev_got == ev_want and {k: len(e) for k, e in ev_got.items()} == {'a': 3, 'b': 2}
        assert all(got.result(k) == want.result(k) for k in vids)
        assert [s.states for s in got.streams.values()] == [s.states for s in want.streams.values()]
    sb = StreamBatcher(StubModel(), frame_format='nv12')
    for bad in (np.zeros((40, 56, 3), dtype=np.uint8), np.zeros((60, 55), dtype=np.uint8), np.zeros((61, 56), dtype=np.uint8),
                np.zeros((60, 56), dtype=np.float32)):
        with pytest.raises(ValueError):
            sb.push('x', bad)
    with pytest.raises(ValueError):
        StreamBatcher(StubModel()).push('x', np.zeros((60, 56), dtype=np.uint8))


def test_inference_dataset_on_nv12_writes_the_score_files_of_the_converted_videos(tmp_path, golden_dir):
    """Two RepCount test videos as NV12 .npy frames and as nv12_to_rgb of them: shard='clips' (the default for NV12) and
    'videos' write the same score files as the RGB job."""
    import json
    import pandas as pd
    anno = pd.read_csv(f'{golden_dir}/repcount_annotation.csv', index_col=0)
    rows = anno[anno['name'].isin(['stu1_40.mp4', 'stu3_53.mp4'])].copy()
    assert len(rows) == 2
    rows['name'] = [n.replace('.mp4', '.npy') for n in rows['name']]
    roots = {}
    for fmt in ('nv12', 'rgb'):
        roots[fmt] = tmp_path / fmt
        (roots[fmt] / 'videos' / 'test').mkdir(parents=True)
        rows.to_csv(roots[fmt] / 'annotation.csv')
    for i, (name, frames) in enumerate(zip(rows['name'], (37, 20))):
        nv = tf.rgb_to_nv12(synthetic_video(i, frames, 44, 26, period=20), 'bt709')
        np.save(roots['nv12'] / 'videos' / 'test' / name, nv)
        np.save(roots['rgb'] / 'videos' / 'test' / name, tf.nv12_to_rgb(nv, 'bt709'))
    reader = lambda path: torch.from_numpy(np.load(path))
    ic.inference_dataset(StubModel(), ['test'], str(tmp_path / 'want'), 'stub', data_root=str(roots['rgb']), video_reader=reader,
                         shard='clips')
    for shard in (None, 'videos'):
        out = tmp_path / f'got_{shard}'
        ic.inference_dataset(StubModel(), ['test'], str(out), 'stub', data_root=str(roots['nv12']), video_reader=reader, shard=shard,
                             frame_format='nv12', colorimetry='bt709')
        assert sorted(os.listdir(out)) == sorted(os.listdir(tmp_path / 'want')) and len(os.listdir(out)) == 2
        for name in os.listdir(out):
            got, want = json.load(open(out / name)), json.load(open(tmp_path / 'want' / name))
            assert got == want and len(got['scores']) == len(range(0, got['total_frames'], 8))


# ---- refusals before the library is touched -------------------------------------------------------------------------------------
def test_refusals_before_the_gpu(tmp_path, monkeypatch):
    def no_gpu(*_a, **_k):
        raise AssertionError('the refusal must come before the library is touched')
    monkeypatch.setattr(engine._lib, 'load', no_gpu)
    from workoutdetector_amd.streaming import StreamBatcher
    nv12 = torch.zeros((4, 60, 56), dtype=torch.uint8)
    rgb = torch.zeros((4, 40, 56, 3), dtype=torch.uint8)
    index = torch.zeros((1, 8), dtype=torch.int32)
    boxes = torch.zeros((1, 4), dtype=torch.int32)
    desc = torch.zeros((1, 8), dtype=torch.int32)
    calls = {'frames': lambda f, **kw: engine.preprocess_frames(f, **kw),
             'clips': lambda f, **kw: engine.preprocess_clips(f, boxes, 0, 8, 0, 1, **kw),
             'indexed': lambda f, **kw: engine.preprocess_indexed(f, index, **kw),
             'windows': lambda f, **kw: engine.preprocess_windows(f.view(-1), desc, 1, 4, **kw)}
    for what, call in calls.items():
        with pytest.raises(ValueError, match='colorimetry'):            # unknown colorimetry
            call(nv12, frame_format='nv12', colorimetry='bt2020')
        with pytest.raises(ValueError, match='colorimetry'):            # a colorimetry with RGB frames
            call(rgb, frame_format='rgb', colorimetry='bt601')
        with pytest.raises(ValueError, match='frame_format'):
            call(nv12, frame_format='yuv')
        with pytest.raises(ValueError):                                 # NV12 frames are a contiguous CUDA uint8 tensor [n, 3h/2, w]
            call(nv12, frame_format='nv12')
        with pytest.raises(ValueError):
            call(nv12.float(), frame_format='nv12')
    model = StubModel()
    for kw in (dict(frame_format='nv12', colorimetry='bt2020'), dict(colorimetry='bt601'), dict(frame_format='yuv')):
        with pytest.raises(ValueError):
            ic.stage_video(model, nv12, **kw)
        with pytest.raises(ValueError):
            ic.video_clip_logits(model, nv12, tf.TestTransform(), **kw)
        with pytest.raises(ValueError):
            StreamBatcher(model, **kw)
        with pytest.raises(ValueError):
            ic.inference_dataset(model, ['test'], str(tmp_path / 'out'), 'ckpt', data_root=str(tmp_path), **kw)
    with pytest.raises(ValueError):
        ic.stage_video(model, rgb, frame_format='nv12')                 # an RGB video given as NV12
    with pytest.raises(NotImplementedError, match='global'):
        ic.inference_dataset(model, ['test'], str(tmp_path / 'out'), 'ckpt', data_root=str(tmp_path), frame_format='nv12',
                             shard='global')
    assert not (tmp_path / 'out').exists()


# ---- the header and the host program --------------------------------------------------------------------------------------------
def test_the_header_holds_the_four_codes_and_abi_7():
    with open(os.path.join(ROOT, 'include', 'tsm_hip.h')) as f:
        text = f.read()
    for name, value in (('TSM_PIXEL_U8', 0), ('TSM_PIXEL_F32', 1), ('TSM_PIXEL_NV12_BT601', 16), ('TSM_PIXEL_NV12_BT709', 17),
                        ('TSM_PIXEL_NV12_BT601_FULL', 18), ('TSM_PIXEL_NV12_BT709_FULL', 19)):
        assert re.search(rf'\b{name} = {value}\b', text), name
    assert re.search(r'#define TSM_ABI_VERSION 7\b', text)
    for row in TABLE.values():                                          # ... and the comment's table is the table
        assert re.search(r'\s+'.join(str(v) for v in row[1:]), text), row


def test_host_arithmetic_under_sanitizers(tmp_path):
    """tests/nv12_host.cpp built with ASAN + UBSAN (runtimes linked statically: the program runs as it is) and run once."""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'nv12_host')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-fno-omit-frame-pointer', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'nv12_host.cpp'),
           '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stdout + run.stderr and 'nv12_host ok' in run.stdout
