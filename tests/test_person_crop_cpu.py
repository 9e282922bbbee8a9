"""person_crop=True without a GPU: the reference's box arithmetic, the torch PersonCropTransform against an independent
composition (tests/_person_crop.py), the factory, the ABI declaration of tsm_preprocess_clips, and the dataset driver's
up-front refusals and its torch fallback for a model that is not an engine."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import _person_crop as pc
from tests._stub import StubModel, synthetic_video

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_person_box_is_the_reference_arithmetic():
    from workoutdetector_amd.transform import person_box
    # union x 8 .. 110.5, y 20.25 .. 230: w 102.5, h 209.75 -> left int(8 - 5.125) = 2, top int(20.25 - 10.4875) = 9,
    # w int(112.75) = 112, h int(230.725) = 230
    assert person_box([[10.5, 20.25, 110.5, 220.25], [8, 25, 100, 230]]) == (9, 2, 230, 112)
    assert person_box(torch.tensor([[10.5, 20.25, 110.5, 220.25], [8, 25, 100, 230]])) == (9, 2, 230, 112)
    # int() truncates toward zero: x1 = 2.5, w = 100 -> int(2.5 - 5) = int(-2.5) = -2 (floor would give -3)
    top, left, h, w = person_box([[2.5, 10.0, 102.5, 50.0]])
    assert (top, left, h, w) == (8, -2, 44, 110)
    # a zero-area union is "no person"
    assert person_box([[4, 4, 4, 90]]) is None and person_box([[0, 0, 0, 0], [0, 0, 0, 0]]) is None
    # one detection per frame, the union is over the clip
    assert person_box([[50, 60, 70, 80]] * 8) == person_box([[50, 60, 70, 80]])
    # a side that the enlargement leaves at 0 pixels cannot be resized
    with pytest.raises(ValueError):
        person_box([[10, 10, 10.5, 40]])


@pytest.mark.parametrize('h,w', [(40, 56), (57, 33)])
@pytest.mark.parametrize('scale_255', [False, True])
def test_person_crop_transform_equals_pad_slice_interpolate(h, w, scale_255):
    from workoutdetector_amd.transform import PersonCropTransform
    size = 32
    tf = PersonCropTransform({}, size=size, scale_255=scale_255)
    frames = pc.video(h * w, 3, h, w).permute(0, 3, 1, 2)
    for box in pc.boxes_for(h, w, size):
        got = tf(frames, box)
        want = pc.reference(frames, box, size, scale_255)
        assert tuple(got.shape) == (3, 3, size, size) and got.dtype == torch.float32
        assert torch.equal(got, want), box
    # entirely outside: every pixel is what a zero becomes
    for box in [(h + 5, 2, 9, 9), (-3, -w - 4, 11, w), (-40, -40, 12, 12), (3, w, 4, 4)]:
        got = tf(frames, box)
        assert torch.equal(got, pc.ZERO.view(1, 3, 1, 1).expand(3, 3, size, size)), box
    # None and a non-positive side are the whole frame
    whole = pc.reference(frames, (0, 0, h, w), size, scale_255)
    for box in [None, (4, 4, 0, 13), (4, 4, 13, -2)]:
        assert torch.equal(tf(frames, box), whole), box
    # uint8 frames are promoted, not scaled, unless scale_255 says so
    assert torch.equal(tf(frames.to(torch.uint8), (5, 7, 20, 17)), pc.reference(frames, (5, 7, 20, 17), size, scale_255))


def test_factory_returns_the_transform_and_keeps_refusing_without_boxes():
    from workoutdetector_amd.transform import PersonCropTransform, TestTransform, build_test_transform
    boxes = {'a.npy': [(1, 2, 3, 4), None]}
    tf = build_test_transform(person_crop=True, boxes=boxes, scale_255=True)
    assert isinstance(tf, PersonCropTransform) and tf.size == 224 and tf.scale_255 is True
    assert tf.box('a.npy', 0) == (1, 2, 3, 4) and tf.box('a.npy', 1) is None
    assert tf.box_rows('a.npy', 0, 2).tolist() == [[1, 2, 3, 4], [0, 0, 0, 0]] and tf.box_rows('a.npy', 0, 2).dtype == torch.int32
    fn = build_test_transform(person_crop=True, boxes=lambda name, c: (c, 0, 5, 5))
    assert fn.box('x', 3) == (3, 0, 5, 5)
    with pytest.raises(NotImplementedError) as ei:
        build_test_transform(person_crop=True)
    assert 'detector' in str(ei.value) and 'boxes' in str(ei.value)
    assert isinstance(build_test_transform(False), TestTransform)
    with pytest.raises(TypeError):
        PersonCropTransform([(1, 2, 3, 4)])


def test_header_library_and_binding_carry_tsm_preprocess_clips():
    from workoutdetector_amd import _lib
    from workoutdetector_amd.build import LIB_PATH, build_library
    build_library()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tsm_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+tsm_preprocess_clips\s*\(', text)
    assert re.search(r'#define\s+TSM_ABI_VERSION\s+7\b', text)
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r' T tsm_preprocess_clips\b', out)
    assert 'tsm_preprocess_clips' in _lib.EXPORTS
    lib = _lib.load()
    assert lib.tsm_abi_version() == _lib.ABI_VERSION == 7
    assert len(lib.tsm_preprocess_clips.argtypes) == 18
    # the refusals of NULL pointers come before anything touches a GPU
    assert lib.tsm_preprocess_clips(None, 0, 1, 8, 8, 0, 8, 0, 1, 8, 8, 2, None, None, 2, 8, 0, None) == -1
    assert b'preprocess_clips' in lib.tsm_last_error(None)


def test_person_crop_refuses_the_global_shard_before_touching_any_file(tmp_path):
    from workoutdetector_amd import inference_count as ic
    out = tmp_path / 'out'
    with pytest.raises(ValueError) as ei:
        ic.inference_dataset(StubModel(), ['test'], str(out), checkpoint='stub', person_crop=True, shard='global',
                             boxes=lambda name, c: None, data_root=str(tmp_path / 'no_such_dataset'))
    assert 'global' in str(ei.value) and not out.exists()
    with pytest.raises(NotImplementedError):            # no boxes: the detector is still out of scope, whatever the shard
        ic.inference_dataset(StubModel(), ['test'], str(out), checkpoint='stub', person_crop=True,
                             data_root=str(tmp_path / 'no_such_dataset'))
    assert not out.exists()


def test_dataset_driver_runs_the_torch_transform_for_a_model_that_is_not_an_engine(tmp_path, golden_dir, monkeypatch):
    """A session / stub has no device path: every clip goes through PersonCropTransform.__call__ with ITS box, the tail
    padded before the transform; shard None resolves to 'clips' and 'videos' writes the same files."""
    import pandas as pd
    from workoutdetector_amd import inference_count as ic, staging
    monkeypatch.setattr(staging, 'engine_device', lambda model: None)       # (the stub has no device path on a GPU box either)
    anno = pd.read_csv(f'{golden_dir}/repcount_annotation.csv', index_col=0)
    rows = anno[anno['name'].isin(['stu1_40.mp4', 'stu5_32.mp4'])].copy()
    rows['name'] = [n.replace('.mp4', '.npy') for n in rows['name']]
    root = tmp_path / 'RepCount'
    (root / 'videos' / 'test').mkdir(parents=True)
    rows.to_csv(root / 'annotation.csv')
    vids = {'stu1_40.npy': synthetic_video(1, 27, 45, 26), 'stu5_32.npy': synthetic_video(2, 41, 45, 26)}
    boxes = {'stu1_40.npy': [(3, 2, 20, 15), (-5, -5, 30, 30), None, (30, 10, 40, 40)],
             'stu5_32.npy': [(1, 1, 9, 9), None, (0, 0, 45, 26), (50, 0, 5, 5), (10, -3, 8, 40), (2, 2, 1, 1)]}
    reader = lambda path: torch.from_numpy(vids[os.path.basename(path)])
    outs = {}
    for shard in (None, 'videos'):
        outs[shard] = str(tmp_path / f'out_{shard}')
        ic.inference_dataset(StubModel(), ['test'], outs[shard], checkpoint='stub', data_root=str(root), person_crop=True,
                             boxes=boxes, video_reader=reader, batch_clips=4, shard=shard)
    model = StubModel()
    for name, vid in vids.items():
        d = json.load(open(os.path.join(outs[None], f'{name}.score.json')))
        assert d == json.load(open(os.path.join(outs['videos'], f'{name}.score.json')))
        assert list(d) == ['video_name', 'model', 'input_shape', 'checkpoint', 'total_frames', 'ground_truth', 'action', 'scores']
        assert list(d['scores']) == [str(s) for s in range(0, len(vid), 8)]
        for c, box in enumerate(boxes[name]):
            x = pc.reference(pc.window(torch.from_numpy(vid), c), box, 224)[None].numpy()
            want = model.run(None, {'input': x})[0][0]
            got = np.float32([d['scores'][str(8 * c)][str(k)] for k in range(12)])
            np.testing.assert_array_equal(got, want)
