"""workoutdetector_amd/classification.py without a GPU: the deterministic frame sampling against the reference's recorded
vectors and hand-derived edges, the annotation reader, the host pipeline on a stub model whose logits are a known function
of the clip (tests/_stub.py), and the ABI declaration of tsm_preprocess_indexed / tsm_top1_tally."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import _segments as sg
from tests._stub import StubModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- sample_frames ---------------------------------------------------------------------------------------------------------
def test_sample_frames_equals_the_references_doctest_vectors(golden_dir):
    from workoutdetector_amd.classification import sample_frames
    cases = json.load(open(os.path.join(golden_dir, 'ref_sample_frames.json')))
    assert len(cases) == 4
    for c in cases:
        assert sample_frames(c['total'], c['num'], c['offset']) == c['want'], c
        assert sg.sample(c['total'], c['num'], c['offset']) == c['want'], c        # (the tests' own write-out agrees too)


@pytest.mark.parametrize('total,want', [
    (1, [0] * 8),
    (3, [0, 0, 0, 1, 1, 1, 2, 2]),               # each frame three times = 9 entries, interval 1, the first 8
    (5, [0, 0, 1, 1, 2, 2, 3, 3]),               # each frame twice = 10 entries, interval 1: frame 4 is never sampled
    (16, [0, 2, 4, 6, 8, 10, 12, 14]),
    (17, [0, 2, 4, 6, 8, 10, 12, 14]),           # interval 17 // 8 = 2, nine starts, the first 8
])
def test_sample_frames_edges(total, want):
    from workoutdetector_amd.classification import sample_frames
    assert sample_frames(total, 8) == want
    assert sample_frames(total, 8, 7) == [v + 7 for v in want]
    assert sg.sample(total, 8) == want


def test_sample_frames_refuses_an_empty_segment():
    from workoutdetector_amd.classification import sample_frames
    for total in (0, -3):
        with pytest.raises(ValueError):
            sample_frames(total, 8)


def test_sample_frames_is_the_write_out_for_every_short_and_long_total():
    from workoutdetector_amd.classification import sample_frames
    for total in range(1, 70):
        got = sample_frames(total, 8, 1)
        assert got == sg.sample(total, 8, 1), total
        assert len(got) == 8 and got == sorted(got) and 1 <= got[0] and got[-1] <= total


# ---- load_annotation -------------------------------------------------------------------------------------------------------
def test_load_annotation_reads_three_and_four_columns(tmp_path):
    from workoutdetector_amd.classification import load_annotation
    four = tmp_path / 'val.txt'
    four.write_text('train/vid_a 1 30 4\nval/vid_b 17 5 11\nval/empty 1 0 2\n')
    pre = os.path.join('/data', 'rawframes')
    assert load_annotation(str(four), pre) == [
        dict(frame_dir=os.path.join(pre, 'train/vid_a'), start_index=1, total_frames=30, label=4),
        dict(frame_dir=os.path.join(pre, 'val/vid_b'), start_index=17, total_frames=5, label=11),
        dict(frame_dir='val/empty', start_index=1, total_frames=0, label=2)]      # (no frames: the prefix is not joined)
    assert [s['frame_dir'] for s in load_annotation(str(four))] == ['train/vid_a', 'val/vid_b', 'val/empty']
    three = tmp_path / 'three.txt'
    three.write_text('vid_c 12 0\nvid_d 40 1\n')
    assert load_annotation(str(three), 'p', anno_col=3) == [
        dict(frame_dir=os.path.join('p', 'vid_c'), start_index=1, total_frames=12, label=0),
        dict(frame_dir=os.path.join('p', 'vid_d'), start_index=1, total_frames=40, label=1)]
    with pytest.raises(ValueError):
        load_annotation(str(three), anno_col=4)
    with pytest.raises(ValueError):
        load_annotation(str(three), anno_col=5)


# ---- eval_classification on a stub ------------------------------------------------------------------------------------------
DIRS = {'a': (11, 60, 40, 56), 'b': (12, 45, 57, 33)}            # seed, frames, h, w; frame number n is video[n - 1]
SEGMENTS = [('a', 1, 30), ('b', 3, 8), ('a', 21, 3), ('a', 25, 17), ('b', 10, 30), ('a', 1, 5), ('b', 40, 1)]
RESIZE, CROP = 36, 32


class Reader:
    def __init__(self):
        self.calls = []

    def __call__(self, frame_dir, numbers):
        self.calls.append((frame_dir, list(numbers)))
        seed, total, h, w = DIRS[frame_dir]
        return sg.video(seed, total, h, w)[[n - 1 for n in numbers]].numpy()


@pytest.fixture(scope='module')
def expected():
    """Logits of the stub on the clips the tests' own sampling and the oracle transform build, sample by sample."""
    model = StubModel(seed=3)
    rows = []
    for d, start, total in SEGMENTS:
        seed, frames, h, w = DIRS[d]
        numbers = tuple(n - 1 for n in sg.sample(total, 8, start))
        clip = sg.reference(seed, frames, h, w, (numbers,), RESIZE, CROP, True)
        rows.append(model.run(None, {'input': clip.numpy()})[0][0])
    return np.stack(rows)


def _samples(labels):
    return [dict(frame_dir=d, start_index=s, total_frames=t, label=l) for (d, s, t), l in zip(SEGMENTS, labels)]


def test_eval_classification_on_a_stub_counts_the_intent(expected):
    from workoutdetector_amd.classification import eval_classification
    from workoutdetector_amd.transform import TestTransform
    preds = expected.argmax(axis=1).tolist()
    # right, wrong, right, a label outside the classes, right, wrong, a negative label
    labels = [preds[0], (preds[1] + 1) % 12, preds[2], 12, preds[4], (preds[5] + 5) % 12, -1]
    reader = Reader()
    model = StubModel(seed=3)
    res = eval_classification(model, _samples(labels), frame_reader=reader, batch_clips=2, return_logits=True,
                              transform=TestTransform(RESIZE, CROP, scale_255=True))
    assert list(res) == ['correct', 'total', 'acc', 'overall', 'preds', 'logits']
    assert res['preds'] == preds                                      # sample order, across the interleaved directories
    np.testing.assert_allclose(res['logits'], expected, rtol=1e-5, atol=1e-5)
    correct, total = sg.tally(preds, labels, 12)
    assert res['correct'] == correct and res['total'] == total
    assert sum(total) == 5 and sum(correct) == 3
    assert res['overall'] == 3 / 5
    assert res['acc'] == [c / n if n else None for c, n in zip(correct, total)] and None in res['acc']
    # the reader was asked once per directory, in first-appearance order, for exactly the union of the sampled frames
    union = {d: sorted({n for (dd, s, t) in SEGMENTS if dd == d for n in sg.sample(t, 8, s)}) for d in DIRS}
    assert reader.calls == [('a', union['a']), ('b', union['b'])]
    assert 5 not in union['a'] and 4 in union['a']                     # ('a', 1, 5): frame 5 of a 5-frame segment is never sampled
    assert model.calls == 2 + 2                                        # batches of two inside a directory: 4 and 3 samples
    json.dumps({k: v for k, v in res.items() if k != 'logits'})        # the result is JSON as it stands


def test_a_torch_module_and_a_plain_callable_take_the_host_path_like_a_session(expected):
    """The host path calls its model through staging.call_host: a torch module and a plain callable on [B, T, 3, H, W] give
    what the session gives (they used to fail with AttributeError on get_inputs)."""
    from workoutdetector_amd.classification import eval_classification
    from workoutdetector_amd.transform import TestTransform

    class Module(torch.nn.Module):
        num_class = 12

        def __init__(self):
            super().__init__()
            self.stub = StubModel(seed=3)

        def forward(self, x):
            assert isinstance(x, torch.Tensor) and not torch.is_grad_enabled()
            return torch.from_numpy(self.stub.run(None, {'input': x.numpy()})[0])

    labels = expected.argmax(axis=1).tolist()
    kw = dict(batch_clips=2, return_logits=True, transform=TestTransform(RESIZE, CROP, scale_255=True))
    want = eval_classification(StubModel(seed=3), _samples(labels), frame_reader=Reader(), **kw)
    module, stub = Module(), StubModel(seed=3)
    for model, calls in ((module, lambda: module.stub.calls), (lambda x: stub.run(None, {'input': x.numpy()})[0], lambda: stub.calls)):
        reader = Reader()
        got = eval_classification(model, _samples(labels), frame_reader=reader, **kw)
        assert np.array_equal(got.pop('logits'), want['logits']) and got == {k: v for k, v in want.items() if k != 'logits'}
        assert [d for d, _n in reader.calls] == ['a', 'b'] and calls() == 2 + 2
    assert want['overall'] == 1.0 and want['logits'].dtype == np.float32


def test_eval_classification_without_samples_and_bad_arguments():
    from workoutdetector_amd.classification import eval_classification
    res = eval_classification(StubModel(), [], frame_reader=Reader())
    assert res == {'correct': [0] * 12, 'total': [0] * 12, 'acc': [None] * 12, 'overall': None, 'preds': []}
    with pytest.raises(ValueError):
        eval_classification(StubModel(), _samples([0] * 7), frame_reader=Reader(), batch_clips=-1)
    with pytest.raises(ValueError):                                    # an empty segment: the reference divides by zero
        eval_classification(StubModel(), [dict(frame_dir='a', start_index=1, total_frames=0, label=0)], frame_reader=Reader())
    with pytest.raises(ValueError):                                    # a reader that returns something else
        eval_classification(StubModel(), _samples([0] * 7), frame_reader=lambda d, n: np.zeros((len(n), 4, 4, 3), np.float32))


def test_an_identity_shaped_model_is_refused_up_front():
    from workoutdetector_amd.classification import eval_classification
    model = StubModel()
    model.consensus_type = 'identity'
    reader = Reader()
    with pytest.raises(ValueError, match='identity'):
        eval_classification(model, _samples([0] * 7), frame_reader=reader)
    assert reader.calls == [] and model.calls == 0


def test_main_writes_one_entry_per_split_and_refuses_person_crop(tmp_path, expected):
    from workoutdetector_amd import classification as cl
    preds = expected.argmax(axis=1).tolist()
    anno = tmp_path / 'val.txt'
    anno.write_text(''.join(f'{d} {s} {t} {l}\n' for (d, s, t), l in zip(SEGMENTS, preds)))
    out = tmp_path / 'acc.json'
    seen = []

    def reader(frame_dir, numbers):
        seen.append(frame_dir)
        return Reader()(os.path.basename(frame_dir), numbers)

    model = StubModel(seed=3)
    model.height = CROP                                                # (the default transform takes the crop from the model)
    res = cl.main({'val': str(anno), 'test': str(anno)}, str(tmp_path / 'root'), str(out), model=model, data_prefix='rawframes',
                  frame_reader=reader)
    assert json.load(open(out)) == res and list(res) == ['val', 'test']
    assert seen[:2] == [str(tmp_path / 'root' / 'rawframes' / 'a'), str(tmp_path / 'root' / 'rawframes' / 'b')]
    # (Resize(256) here, not the 36 of `expected`: only that the pipeline runs end to end and tallies its own preds)
    for split in res.values():
        assert split['total'] == sg.tally(split['preds'], preds, 12)[1] and sum(split['total']) == 7
        assert split['correct'] == sg.tally(split['preds'], preds, 12)[0]
    with pytest.raises(NotImplementedError):
        cl.main({'val': str(anno)}, str(tmp_path), str(out), model=model, person_crop=True)


def test_default_reader_decodes_the_references_file_names(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    from workoutdetector_amd.classification import read_frames
    frames = sg.video(5, 3, 8, 10).numpy()
    for n, f in zip((1, 2, 12), frames):
        Image.fromarray(f).save(tmp_path / f'img_{n:05}.png')
    got = read_frames(str(tmp_path), [12, 1, 1], filename_tmpl='img_{:05}.png')
    assert got.dtype == np.uint8 and np.array_equal(got, frames[[2, 0, 0]])


# ---- the two entry points --------------------------------------------------------------------------------------------------
def test_header_library_and_binding_carry_the_two_entry_points():
    from workoutdetector_amd import _lib
    from workoutdetector_amd.build import LIB_PATH, build_library
    build_library()
    raw = open(os.path.join(ROOT, 'include', 'tsm_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ('tsm_preprocess_indexed', 'tsm_top1_tally'):
        assert re.search(r'\bint\s+' + sym + r'\s*\(', text)
        assert re.search(r' T ' + sym + r'\b', out)
        assert sym in _lib.EXPORTS
        assert re.search(r'^ \*   ' + sym + r'\b', raw, flags=re.M), f'{sym} is missing from the entry-point list of the header'
    assert '#define TSM_ABI_VERSION 7' in raw
    lib = _lib.load()
    assert len(lib.tsm_preprocess_indexed.argtypes) == 14 and len(lib.tsm_top1_tally.argtypes) == 8
    # refusals that need no GPU: NULL pointers, non-positive sizes, a bad pixel type / layout, a crop beyond the resized frame,
    # more than 1024 classes (non-NULL stand-ins: each is refused before anything is launched or read)
    import ctypes
    buf = (ctypes.c_int32 * 16)()
    at = ctypes.addressof(buf)
    good = dict(frames=at, pixel=0, n_frames=1, h=8, w=8, index=at, n_clips=1, n_segment=8, out=at, layout=2, resize=8, crop=8,
                scale=1, stream=None)
    for bad in (dict(frames=None), dict(index=None), dict(out=None), dict(n_frames=0), dict(h=0), dict(w=-1), dict(n_clips=0),
                dict(n_segment=0), dict(resize=0), dict(crop=0), dict(pixel=2), dict(layout=1), dict(layout=5), dict(crop=9),
                dict(h=16, resize=8, crop=9)):
        assert lib.tsm_preprocess_indexed(*{**good, **bad}.values()) == -1, bad
        assert lib.tsm_last_error(None)
    assert lib.tsm_top1_tally(None, at, 1, 2, at, at, at + 8, None) == -1
    assert lib.tsm_top1_tally(at, None, 1, 2, at, at, at + 8, None) == -1
    assert lib.tsm_top1_tally(at, at, 0, 2, at, at, at + 8, None) == -1
    assert lib.tsm_top1_tally(at, at, 1, 0, at, at, at + 8, None) == -1
    assert lib.tsm_top1_tally(at, at, 1, 2, at, at, at, None) == -1 and b'alias' in lib.tsm_last_error(None)
    assert lib.tsm_top1_tally(at, at, 1, 1025, None, at, at + 8, None) == -7 and b'1024' in lib.tsm_last_error(None)


def test_bindings_refuse_wrong_tensors_before_the_c_abi():
    from workoutdetector_amd.engine import preprocess_indexed, top1_tally
    frames = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    index = torch.zeros((1, 8), dtype=torch.int32)
    with pytest.raises(ValueError):
        preprocess_indexed(frames, index)                              # host tensors
    with pytest.raises(ValueError):
        preprocess_indexed(frames.to(torch.int16), index)
    logits = torch.zeros((3, 12))
    counters = torch.zeros((2, 12), dtype=torch.int32)
    with pytest.raises(ValueError):
        top1_tally(logits, torch.zeros(3, dtype=torch.int32), counters[0], counters[1])
