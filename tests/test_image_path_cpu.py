"""The image-model path on the CPU: Pillow's 8-bit bilinear resample in NumPy (transform.pil_resize_u8) against recorded and
live Pillow, the coefficient tables, the host vote against the reference's loop, the torchvision key remap, the counting
driver on a stub model, and the ABI declarations of the two new entry points."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import _image_path as ip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', ip.CASES)
def test_pil_resize_u8_plus_crop_equals_the_fixture_exactly(name):
    from workoutdetector_amd.transform import ImageTransform
    frames, want, resize, crop = ip.fixture(name)
    tf = ImageTransform(resize, crop)
    for f, w in zip(frames, want):
        assert np.array_equal(tf.crop_u8(f), w), name
    # ... and the float form is NumPy's normalisation of those bytes, NCHW
    got = tf(frames).numpy()
    assert got.dtype == np.float32 and got.shape == (3, 3, crop, crop)
    assert np.array_equal(got, ip.normalised(want).transpose(0, 3, 1, 2))


def test_pil_resize_u8_equals_live_pillow_on_random_sizes():
    Image = pytest.importorskip('PIL.Image')
    from workoutdetector_amd.transform import pil_resize_u8, resized_hw
    rng = np.random.default_rng(2024)
    done = 0
    for t in range(50):
        h, w, r = int(rng.integers(1, 100)), int(rng.integers(1, 100)), int(rng.integers(1, 64))
        if t % 5 == 0:
            r = min(h, w)                       # the shorter side keeps its size: nothing is resampled
        if t % 5 == 1:
            w = h                               # square: both sides become r
        if t % 5 == 2:
            h, r = (r, r) if h <= w else (h, w)  # one axis unchanged, the other resampled or not
        nh, nw = resized_hw(h, w, r)
        if nh <= 0 or nw <= 0:
            continue
        f = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        img = Image.fromarray(f)
        want = np.asarray(img.resize((nw, nh), Image.BILINEAR) if (nh, nw) != (h, w) else img)
        assert np.array_equal(pil_resize_u8(f, r), want), (h, w, r)
        done += 1
    assert done >= 45


def test_tables_stay_inside_the_input_and_rows_sum_to_one():
    from workoutdetector_amd.transform import PRECISION_BITS, image_tables, pil_ksize, pil_resample_tables
    assert PRECISION_BITS == 22
    for in_size, out_size in [(53, 34), (37, 24), (20, 32), (90, 46), (31, 16), (720, 256), (1280, 455), (2160, 256), (7, 7), (1, 5)]:
        bounds, kk = pil_resample_tables(in_size, out_size)
        assert bounds.shape == (out_size, 2) and kk.shape == (out_size, pil_ksize(in_size, out_size))
        assert bounds.dtype == np.int32 and kk.dtype == np.int32
        lo, n = bounds[:, 0].astype(int), bounds[:, 1].astype(int)
        assert (lo >= 0).all() and (n >= 1).all() and (lo + n <= in_size).all() and (n <= kk.shape[1]).all()
        assert (np.diff(lo) >= 0).all()
        for i in range(out_size):
            assert abs(int(kk[i].astype(np.int64).sum()) - (1 << 22)) <= n[i], (in_size, out_size, i)
            assert not kk[i, n[i]:].any()
    # the packed block of the launch: crop * (2 + taps) words per resampled axis, none for an axis that keeps its size
    assert image_tables(37, 53, 24, 16).size == 16 * (2 + pil_ksize(53, 34)) + 16 * (2 + pil_ksize(37, 24))
    assert image_tables(24, 41, 24, 16).size == 0       # the shorter side is 24 already: Resize(24) resamples nothing
    assert image_tables(24, 24, 24, 16).size == 0
    assert image_tables(90, 31, 16, 15).size == 15 * (2 + pil_ksize(31, 16)) + 15 * (2 + pil_ksize(90, 46))
    with pytest.raises(ValueError):
        image_tables(37, 53, 24, 25)


def test_host_vote_is_the_reference_loop_whole_and_split_at_every_boundary():
    from workoutdetector_amd.counting import vote_states
    rng = np.random.default_rng(5)
    for c in (2, 5):
        for n in (1, 6, 7, 8, 23, 40):
            preds = rng.integers(0, c, size=n).tolist()
            want = ip.reference_vote(preds)
            got, hist = vote_states(preds)
            assert got == want and hist == preds[-6:]
            for batch in range(1, 9):
                got, hist = [], []
                for a in range(0, n, batch):
                    s, hist = vote_states(preds[a:a + batch], hist)
                    got += s
                assert got == want, (c, n, batch)


def test_torchvision_keys_are_mapped_onto_the_engine_names():
    from workoutdetector_amd.weights import make_state_dict, remap_torchvision_keys, required_keys
    sd = make_state_dict(0, 2, 'resnet18')
    tv = {}
    for k, v in sd.items():                     # the engine's names -> torchvision's own
        tv[k[len('base_model.'):].replace('.conv1.net.', '.conv1.') if k.startswith('base_model.') else k] = v
    tv['bn1.num_batches_tracked'] = np.int64(0)
    assert 'conv1.weight' in tv and 'layer1.0.conv1.weight' in tv and 'layer2.0.downsample.0.weight' in tv and 'fc.weight' in tv
    got = remap_torchvision_keys(tv)
    want = {k.replace('.conv1.net.', '.conv1.'): v for k, v in sd.items()}
    assert {k for k in got if not k.endswith('num_batches_tracked')} == set(want)
    assert all(got[k] is want[k] for k in want)
    assert {k.replace('.conv1.net.', '.conv1.') for k in required_keys(base_model='resnet18')} <= set(got)
    # a Lightning state dict: one leading component on every key
    lightning = {'model.' + k: v for k, v in tv.items()}
    assert list(remap_torchvision_keys(lightning)) == list(got)
    with pytest.raises(ValueError):
        remap_torchvision_keys({'backbone.conv1.conv.weight': 0, 'cls_head.fc_cls.weight': 0})
    with pytest.raises(ValueError):
        remap_torchvision_keys(dict(tv, avgpool=0))


def test_create_image_model_refuses_unknown_keywords_and_bad_geometry():
    from workoutdetector_amd.engine import create_image_model
    for kw in (dict(max_frame=8), dict(shift_place='block'), dict(num_segments=8)):
        with pytest.raises(TypeError):
            create_image_model(**kw)
    with pytest.raises(ValueError):
        create_image_model(resize=32, crop=40)
    with pytest.raises(NotImplementedError):
        create_image_model(base_model='resnet101')


class _Brightness(torch.nn.Module):
    """Two classes from the mean of the transformed frame: a bright frame is class 1."""

    def forward(self, x):
        m = x.mean(dim=(1, 2, 3))
        return torch.stack([-m, m], dim=1)


def _blinking_video():
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, size=(45, 30, 40, 3), dtype=np.uint8)
    for a in range(0, 45, 16):
        frames[a:a + 8] //= 5               # 8 dark frames, 8 bright ones, ...
    return frames


def test_count_by_image_model_with_a_stub_model(tmp_path):
    from workoutdetector_amd import inference_count as ic
    from workoutdetector_amd.counting import pred_to_count
    from workoutdetector_amd.transform import ImageTransform
    model = _Brightness()
    model.image_resize, model.image_crop = 24, 16
    frames = _blinking_video()
    scores = model(ImageTransform(24, 16)(frames)).numpy()
    states = ip.reference_vote(scores.argmax(axis=1))
    want = pred_to_count(states, step=7)
    assert want[0] >= 2                                             # the video does blink
    path = str(tmp_path / 'scores')
    assert ic.count_by_image_model(model, frames, ground_truth=[0, 1] * want[0], pred_out_path=path, threshold=0.9) == want
    saved = json.load(open(path + '.json'))
    assert list(saved['scores']) == [str(i) for i in range(45)]
    np.testing.assert_array_equal(np.float32([[r['0'], r['1']] for r in saved['scores'].values()]), scores)
    for batch in (1, 5, 8):
        assert ic.count_by_image_model(model, list(frames), batch_frames=batch) == want
        assert ic.image_states(model, torch.from_numpy(frames), batch_frames=batch)[0] == states
    one = ic.inference_image(model, frames[3])
    assert one.dtype == np.float32 and one.shape == (2,) and np.array_equal(one, scores[3])
    assert np.array_equal(ic.inference_images(model, frames[:4]), scores[:4])


def test_header_library_and_binding_carry_the_two_entry_points():
    from workoutdetector_amd import _lib
    from workoutdetector_amd.build import LIB_PATH, build_library
    build_library()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tsm_hip.h')).read(), flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ('tsm_preprocess_image', 'tsm_frame_votes'):
        assert re.search(r'\bint\s+' + sym + r'\s*\(', text)
        assert re.search(r' T ' + sym + r'\b', out)
        assert sym in _lib.EXPORTS
    lib = _lib.load()
    assert len(lib.tsm_preprocess_image.argtypes) == 11 and len(lib.tsm_frame_votes.argtypes) == 9
    # refusals that need no GPU: NULL pointers, a history count outside 0..6
    assert lib.tsm_preprocess_image(None, 1, 8, 8, None, 0, None, 2, 8, 8, None) == -1
    assert lib.tsm_frame_votes(None, 1, 2, None, 0, None, None, None, None) == -1
    # (non-NULL stand-ins: the count is refused before anything is launched or read)
    import ctypes
    buf = (ctypes.c_int32 * 16)()
    at = ctypes.addressof(buf)
    for n_hist in (7, -1):
        assert lib.tsm_frame_votes(at, 1, 2, at, n_hist, at, at, None, None) == -1
        assert b'n_hist' in lib.tsm_last_error(None)
    assert lib.tsm_frame_votes(at, 1, 2, None, 1, at, at, None, None) == -1          # a count without a history
    assert lib.tsm_frame_votes(at, 1, 2, at, 3, at, at, at, None) == -1 and b'alias' in lib.tsm_last_error(None)
