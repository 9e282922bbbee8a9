"""tsm_preprocess_indexed (the centre-crop test transform through a device index table, one launch) against the CPU
composition of tests/_segments.py, tsm_top1_tally against a NumPy tally, and eval_classification on a real engine.

Every launch runs in hostile memory (tests/_guard.py): frames, table, logits, labels and counters between poisoned bands,
outputs poisoned before the launch, bands and payload checked after it.  Tolerance: the project's preprocess bound,
|err| <= 1e-5 |want| + 5e-4 (tests/test_preprocess_gpu.py::_check).  Shapes: 40 x 56 and 57 x 33 frames (an odd width,
h > w), 9 staged frames, 4 clips of 8 segments; (resize, crop) = (36, 32), (37, 33) -- a pixel-pair tail column in the bf16
layouts -- and (64, 48), which scales up.
"""
import os

import numpy as np
import pytest
import torch

from oracle import transform_oracle
from tests import _image_path as ip
from tests import _segments as sg
from tests._guard import POISON, check, guarded, guarded_out
from tests._stub import synthetic_video

pytestmark = pytest.mark.gpu

N_FRAMES = 9
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
# One launch meets every kind of list: ascending; the pattern of a segment shorter than 8 frames (the same frame twice in a
# clip); descending, from buffer frame 8 -- the guard band lies right behind it; a 3-frame segment's pattern that shares its
# frames with the clips before it (the same frame in two clips).
TABLE = ((0, 1, 2, 3, 4, 5, 6, 7), (2, 2, 3, 3, 4, 4, 5, 5), (8, 7, 6, 5, 4, 3, 2, 1), (6, 6, 6, 7, 7, 7, 8, 8))
GEOMETRIES = [(36, 32), (37, 33), (64, 48)]


def _check(got, want, what):
    got, want = got.double(), want.double()
    err = (got - want).abs()
    bound = 1e-5 * want.abs() + 5e-4
    print(f'{what}: max err {float(err.max()):.3g}, max err / bound {float((err / bound).max()):.3g}')
    assert bool((err <= bound).all()), f'{what}: max err {float(err.max()):.3g}'


def _layouts():
    from workoutdetector_amd import _lib
    return {'nthwc4': _lib.LAYOUT_NTHWC4, 'ntchw': _lib.LAYOUT_NTCHW, 'nthwc8s': _lib.LAYOUT_NTHWC8S, 'nthwc8b': _lib.LAYOUT_NTHWC8B}


def _shape(layout, n, t, crop):
    from workoutdetector_amd.engine import _frame_shape
    return (n, t) + _frame_shape(layout, crop)


def _launch(frames, table, resize, crop, layout, **kw):
    """engine.preprocess_indexed in hostile memory; `frames`: the staged frames (CPU tensor), `table`: rows of int32 entries."""
    from workoutdetector_amd.engine import preprocess_indexed
    src = guarded(frames.cuda(), name='frames')
    idx = guarded(torch.tensor(table, dtype=torch.int32).cuda(), name='index')
    out = guarded_out(_shape(layout, len(table), len(table[0]), crop), name='out')
    assert preprocess_indexed(src, idx, resize=resize, crop=crop, layout=layout, out=out, **kw) is out
    torch.cuda.synchronize()
    check(src, idx, out)
    return out.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('layout_name', ['nthwc4', 'ntchw', 'nthwc8s', 'nthwc8b'])
@pytest.mark.parametrize('resize,crop', GEOMETRIES)
@pytest.mark.parametrize('h,w', [(40, 56), (57, 33)])
def test_preprocess_indexed_matches_the_cpu_composition(hip_lib, h, w, resize, crop, layout_name):
    """Every kind of list in one launch, uint8 and float sources, scale_255 on and off.  fp32 layouts against the CPU reference
    under the preprocess bound, pad channel exactly 0; the pixel-pair layouts against the fp32 output of the same kernel:
    bf16 = RNE of it, split hi = the same and hi + lo within 2^-16, pad channel and the odd pixel of an odd size exactly 0."""
    from workoutdetector_amd import _lib
    layout = _layouts()[layout_name]
    seed = h * w
    frames = sg.video(seed, N_FRAMES, h, w)
    n, pairs = len(TABLE), (crop + 1) // 2
    for f32_src, scale_255 in [(False, True), (True, False), (False, False), (True, True)]:
        what = f'{h}x{w} -> {resize}/{crop} {layout_name} {"f32" if f32_src else "u8"} scale_255={scale_255}'
        src = frames.float() if f32_src else frames
        want = sg.reference(seed, N_FRAMES, h, w, TABLE, resize, crop, scale_255)          # [4,8,3,crop,crop]
        got = _launch(src, TABLE, resize, crop, layout, scale_255=scale_255)
        if layout == _lib.LAYOUT_NTCHW:
            _check(got, want, what)
            continue
        if layout == _lib.LAYOUT_NTHWC4:
            assert float(got[..., 3].abs().max()) == 0.0, what
            _check(got[..., :3].permute(0, 1, 4, 2, 3), want, what)
            continue
        nchw = _launch(src, TABLE, resize, crop, _lib.LAYOUT_NTCHW, scale_255=scale_255)
        _check(nchw, want, what + ' (its fp32 form)')
        f32 = nchw.permute(0, 1, 3, 4, 2)                                                  # [4,8,crop,crop,3]
        if layout == _lib.LAYOUT_NTHWC8B:
            px = got.view(torch.bfloat16).reshape(n, 8, crop, pairs * 2, 4).float()
            val = hi = px
        else:
            g = got.view(torch.bfloat16).reshape(n, 8, crop, pairs, 2, 8).float()           # [hi x8 | lo x8] per pair
            hi = g[..., 0, :].reshape(n, 8, crop, pairs * 2, 4)
            val = (g[..., 0, :] + g[..., 1, :]).reshape(n, 8, crop, pairs * 2, 4)
        assert torch.equal(hi[..., :crop, :3], f32.to(torch.bfloat16).float()), what
        if layout == _lib.LAYOUT_NTHWC8S:
            assert bool(((val[..., :crop, :3] - f32).abs() <= f32.abs() * 2.0 ** -16 + 1e-30).all()), what
        assert float(val[..., 3].abs().max()) == 0.0, what
        if crop % 2:
            assert float(val[..., crop:, :].abs().max()) == 0.0, what


@pytest.mark.parametrize('layout_name', ['nthwc4', 'nthwc8s'])
@pytest.mark.parametrize('resize,crop', GEOMETRIES)
def test_a_row_equals_the_row_of_preprocess_frames_bit_for_bit(hip_lib, resize, crop, layout_name):
    """The indexed launch reuses preprocess_pixel: row (c, k) is tsm_preprocess' row for frame TABLE[c][k], to the bit."""
    from workoutdetector_amd.engine import preprocess_frames
    layout = _layouts()[layout_name]
    for h, w in [(40, 56), (57, 33)]:
        frames = sg.video(h + w, N_FRAMES, h, w)
        for f32_src, scale_255 in [(False, True), (True, False)]:
            src = frames.float() if f32_src else frames
            per_frame = preprocess_frames(src.cuda(), resize=resize, crop=crop, scale_255=scale_255, layout=layout).cpu()
            got = _launch(src, TABLE, resize, crop, layout, scale_255=scale_255)
            want = per_frame[torch.tensor(TABLE).reshape(-1)].reshape(got.shape)
            assert torch.equal(_bits(got), _bits(want)), (h, w, f32_src, scale_255)


def test_entries_outside_the_buffer_give_the_zero_frame_and_read_nothing(hip_lib):
    """The kernel is total in the table (device memory, no host check sees it): -1, 9 = n_frames, INT32_MIN and INT32_MAX mixed
    with good entries.  Each such row is (0 - mean) / std to the bit, each neighbour is the row of the clean launch, and the
    bands around frames, table and output stay intact.  The documented behaviour, exercised; not an attempt to fault."""
    from workoutdetector_amd import _lib
    h, w, resize, crop = 40, 56, 37, 33
    frames = sg.video(17, N_FRAMES, h, w)
    hostile = ((0, -1, 2, 9, 4, I32_MIN, 6, I32_MAX), (-1, -1, 3, 3, 9, 9, 5, 5), (8, I32_MAX, 6, I32_MIN, 4, 3, 2, 1),
               (I32_MIN, 6, I32_MAX, 7, -1, 7, 9, 8))
    bad = torch.tensor([[not 0 <= v < N_FRAMES for v in row] for row in hostile])
    assert int(bad.sum()) == 14
    clean = tuple(tuple(v if 0 <= v < N_FRAMES else 0 for v in row) for row in hostile)
    zero = sg.ZERO.view(3, 1, 1).expand(3, crop, crop)
    for scale_255 in (True, False):
        got = _launch(frames, hostile, resize, crop, _lib.LAYOUT_NTCHW, scale_255=scale_255)
        ref = _launch(frames, clean, resize, crop, _lib.LAYOUT_NTCHW, scale_255=scale_255)
        assert torch.equal(_bits(got[bad]), _bits(zero.expand(14, 3, crop, crop)))
        assert torch.equal(_bits(got[~bad]), _bits(ref[~bad]))
        assert not torch.equal(ref[0, 1], zero)
        packed = _launch(frames, hostile, resize, crop, _lib.LAYOUT_NTHWC4, scale_255=scale_255)
        assert torch.equal(_bits(packed[..., :3].permute(0, 1, 4, 2, 3)), _bits(got))
        assert float(packed[..., 3].abs().max()) == 0.0
        # the pixel-pair form of the zero frame: bf16(zero) in both pixels, 0 in the pad channel and in the odd tail pixel
        pairs = (crop + 1) // 2
        b = _launch(frames, hostile, resize, crop, _lib.LAYOUT_NTHWC8B, scale_255=scale_255)
        px = b.view(torch.bfloat16).reshape(4, 8, crop, pairs * 2, 4).float()[bad]
        assert torch.equal(px[..., :crop, :3], sg.ZERO.to(torch.bfloat16).float().expand(14, crop, crop, 3))
        assert float(px[..., 3].abs().max()) == 0.0 and float(px[..., crop:, :].abs().max()) == 0.0
    # a float source, and a table that holds nothing but hostile entries
    only = ((I32_MIN, I32_MAX, -1, 9, 2 ** 30, -2 ** 30, 10, 1 << 16),)
    got = _launch(frames.float(), only, resize, crop, _lib.LAYOUT_NTCHW)
    assert torch.equal(_bits(got), _bits(zero.expand(1, 8, 3, crop, crop)))


def test_host_validation_refuses_before_any_launch(hip_lib):
    """NULL pointers, zero sizes, a bad pixel type or layout, a crop larger than the resized side: TSM_ERR_INVALID_ARG, the
    output still all poison and the launch trace empty.  The good call launches exactly one kernel."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import launch_trace, preprocess_indexed
    h, w, resize, crop = 40, 56, 36, 32
    frames = guarded(sg.video(3, N_FRAMES, h, w).cuda(), name='frames')
    index = guarded(torch.tensor(TABLE, dtype=torch.int32).cuda(), name='index')
    out = guarded_out(_shape(_lib.LAYOUT_NTHWC4, 4, 8, crop), name='out')
    good = dict(frames=frames.data_ptr(), pixel=_lib.PIXEL_U8, n_frames=N_FRAMES, h=h, w=w, index=index.data_ptr(), n_clips=4,
                n_segment=8, out=out.data_ptr(), layout=_lib.LAYOUT_NTHWC4, resize=resize, crop=crop, scale=1, stream=None)
    cases = [dict(frames=None), dict(index=None), dict(out=None), dict(n_frames=0), dict(h=0), dict(w=0), dict(n_clips=0),
             dict(n_segment=0), dict(resize=0), dict(crop=0), dict(pixel=2), dict(layout=_lib.LAYOUT_NTHWC), dict(layout=5),
             dict(crop=37),                                   # the resized frame is 36 x 50
             dict(resize=32, crop=33)]
    for bad in cases:
        with launch_trace() as tr:
            status = hip_lib.tsm_preprocess_indexed(*{**good, **bad}.values())
        assert status == -1, bad
        assert tr.kernels == [], (bad, tr.kernels)
        torch.cuda.synchronize()
        assert bool((out.view(torch.int32) == POISON).all()), bad
        check(frames, index)
    # through the binding: the crop check raises the library's error, a wrong table never reaches the C ABI
    with launch_trace() as tr:
        with pytest.raises(_lib.TsmError) as ei:
            preprocess_indexed(frames, index, resize=32, crop=33)
    assert ei.value.status == -1 and tr.kernels == []
    for wrong in (index.float(), index.reshape(-1), index.cpu(), index.long()):
        with pytest.raises(ValueError):
            preprocess_indexed(frames, wrong, resize=resize, crop=crop)
    with pytest.raises(ValueError):
        preprocess_indexed(frames, index, resize=resize, crop=crop, layout=_lib.LAYOUT_NTHWC)
    with pytest.raises(ValueError):
        preprocess_indexed(frames, index, resize=resize, crop=crop, out=out[:3])
    # ... and the same call with good arguments launches exactly one kernel
    with launch_trace() as tr:
        preprocess_indexed(frames, index, resize=resize, crop=crop, out=out)
    assert tr.kernels == ['preprocess_indexed_kernel<unsigned char>'], tr.kernels
    torch.cuda.synchronize()
    check(frames, index, out)


# ---- the tally ---------------------------------------------------------------------------------------------------------------
def _labels(seed, preds, num_class, hostile):
    """Half the rows labelled with their own arg-max, the rest at random; `hostile` values planted at fixed rows."""
    rng = np.random.default_rng(seed)
    labels = np.where(rng.random(len(preds)) < 0.5, preds, rng.integers(0, num_class, len(preds))).astype(np.int64)
    for at, v in zip((1, len(preds) // 2, len(preds) - 1), hostile):
        labels[at] = v
    return labels


def _tally(logits, labels, correct, total):
    from workoutdetector_amd.engine import launch_trace, top1_tally
    x = guarded(torch.from_numpy(logits).cuda(), name='logits')
    lab = guarded(torch.from_numpy(labels.astype(np.int32)).cuda(), name='labels')
    pred = guarded_out((len(logits),), torch.int32, name='pred')
    with launch_trace() as tr:
        assert top1_tally(x, lab, correct, total, out=pred) is pred
    assert tr.kernels == ['top1_tally_kernel'], tr.kernels
    torch.cuda.synchronize()
    check(x, lab, pred, correct, total)
    return pred.cpu().tolist()


def test_top1_tally_equals_numpy_and_accumulates(hip_lib):
    """n = 37, 12 classes, planted exact ties (the FIRST maximum wins), labels -1, 12 and INT32_MIN among them: two calls into
    the same counters give preds and counters equal to the NumPy tally exactly; then 1024 classes; 1025 are refused."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import launch_trace, top1_tally
    n, c = 37, 12
    correct = guarded(torch.zeros(c, dtype=torch.int32).cuda(), name='correct')
    total = guarded(torch.zeros(c, dtype=torch.int32).cuda(), name='total')
    want_c, want_t = [0] * c, [0] * c
    for call, hostile in enumerate([(-1, c, I32_MIN), (I32_MAX, -2, c + 1000)]):
        x = ip.logits_with_ties(100 + call, n, c)
        preds = x.argmax(axis=1)                                   # numpy: the first maximum
        labels = _labels(call, preds, c, hostile)
        assert _tally(x, labels, correct, total) == preds.tolist()
        cc, tt = sg.tally(preds.tolist(), labels.tolist(), c)
        want_c = [a + b for a, b in zip(want_c, cc)]
        want_t = [a + b for a, b in zip(want_t, tt)]
        assert sum(tt) == n - 3 and 0 < sum(cc) < sum(tt)
        assert correct.cpu().tolist() == want_c and total.cpu().tolist() == want_t, call
    # the largest class count, every thread a class of its own: labels at both ends of the range and one outside
    c = 1024
    x = ip.logits_with_ties(7, 3, c)
    x[1, :] = -1.0
    x[1, c - 1] = 5.0                                               # row 1: the last class
    preds = x.argmax(axis=1)
    assert preds[0] == 0 and preds[1] == c - 1                      # (row 0 of logits_with_ties is constant: the first class)
    labels = np.array([0, c - 1, c], dtype=np.int64)
    correct = guarded(torch.zeros(c, dtype=torch.int32).cuda(), name='correct')
    total = guarded(torch.full((c,), 5, dtype=torch.int32).cuda(), name='total')      # counters accumulate onto what they hold
    assert _tally(x, labels, correct, total) == preds.tolist()
    cc, tt = sg.tally(preds.tolist(), labels.tolist(), c)
    assert correct.cpu().tolist() == cc and total.cpu().tolist() == [5 + v for v in tt] and sum(cc) == 2
    # 1025 classes: refused, nothing launched
    x = torch.zeros((2, 1025), dtype=torch.float32, device='cuda')
    counters = torch.zeros((2, 1025), dtype=torch.int32, device='cuda')
    with launch_trace() as tr:
        with pytest.raises(_lib.TsmError) as ei:
            top1_tally(x, torch.zeros(2, dtype=torch.int32, device='cuda'), counters[0], counters[1])
    assert ei.value.status == -7 and tr.kernels == []
    torch.cuda.synchronize()
    assert int(counters.abs().sum()) == 0
    # the binding's own refusals
    lab = torch.zeros(3, dtype=torch.int32, device='cuda')
    x = torch.zeros((3, 12), dtype=torch.float32, device='cuda')
    cnt = torch.zeros((2, 12), dtype=torch.int32, device='cuda')
    for args in ((x, lab.long(), cnt[0], cnt[1]), (x, lab[:2], cnt[0], cnt[1]), (x, lab, cnt[0].cpu(), cnt[1]),
                 (x, lab, cnt[0], cnt[0]), (x, lab, cnt[0, :11], cnt[1]), (x.double(), lab, cnt[0], cnt[1])):
        with pytest.raises(ValueError):
            top1_tally(*args)


# ---- eval_classification on a real engine ------------------------------------------------------------------------------------
DIRS = {'stu1': (31, 64, 48, 36), 'stu5': (52, 50, 36, 52)}            # seed, frames, h, w; frame number n is video[n - 1]
# (frame_dir, start_index, total_frames): 6 samples of one directory and 3 of the other, interleaved; segments shorter than 8
# frames (3, 5, 1), exactly 8, and longer with and without a remainder (17, 30, 16, 40)
SEGMENTS = [('stu1', 1, 3), ('stu5', 2, 8), ('stu1', 4, 8), ('stu1', 12, 17), ('stu5', 10, 30), ('stu1', 30, 30), ('stu1', 60, 5),
            ('stu5', 49, 1), ('stu1', 20, 40)]


def _video(name):
    seed, frames, h, w = DIRS[name]
    return torch.from_numpy(synthetic_video(seed, frames, h, w, period=12))


def _reader(frame_dir, numbers):
    return _video(frame_dir)[[n - 1 for n in numbers]].numpy()


def _make_engine(sd0, poison):
    from workoutdetector_amd.engine import TsmEngine
    keep = {k: os.environ.get(k) for k in ('TSM_AUTOTUNE', 'TSM_POISON')}
    os.environ['TSM_AUTOTUNE'] = '0'
    os.environ.pop('TSM_POISON', None)
    if poison:
        os.environ['TSM_POISON'] = '1'
    try:
        return TsmEngine(num_class=12, num_segments=8, max_clips=4, state_dict=sd0)       # (TSM_* are read in tsm_create)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope='module')
def engine(hip_lib, sd0):
    eng = _make_engine(sd0, poison=False)
    yield eng
    eng.close()


def _samples(labels):
    return [dict(frame_dir=d, start_index=s, total_frames=t, label=int(l)) for (d, s, t), l in zip(SEGMENTS, labels)]


@pytest.fixture(scope='module')
def labels(engine):
    """A first pass tells which class the engine calls each sample; the labels of the tests keep five of those, replace three
    and put one outside the classes -- so both counters have something to count."""
    from workoutdetector_amd.classification import eval_classification
    preds = eval_classification(engine, _samples([0] * len(SEGMENTS)), frame_reader=_reader)['preds']
    out = list(preds)
    for i in (1, 4, 6):
        out[i] = (preds[i] + 1 + i) % 12
    out[8] = -1
    return out


def _consistent(res, labels, logits):
    """A run with other batches: its logits within the pipeline bar of `logits`, preds and counters exact against ITS logits."""
    np.testing.assert_allclose(res['logits'], logits, rtol=1e-5, atol=1e-4)
    assert res['preds'] == res['logits'].argmax(axis=1).tolist()
    correct, total = sg.tally(res['preds'], labels, 12)
    assert res['correct'] == correct and res['total'] == total


def test_engine_path_is_one_indexed_launch_and_one_tally_per_batch(engine, labels):
    """eval_classification on a TsmEngine: per batch of <= max_clips samples one preprocess_indexed_kernel launch, the forward
    and one top1_tally_kernel launch -- neither preprocess_kernel nor gather_clips_kernel runs; the logits equal forward_device
    on the host-transformed clips of the same engine within the bound the pipeline test holds the HIP transform to against the
    torch one (tests/test_pipeline_gpu.py: rtol 1e-5, atol 1e-4); preds are the first arg-max of the path's own logits and the
    counters the NumPy tally of those preds, exactly."""
    from workoutdetector_amd.classification import eval_classification
    from workoutdetector_amd.engine import launch_trace
    with launch_trace() as tr:
        res = eval_classification(engine, _samples(labels), frame_reader=_reader, return_logits=True)
    assert tr.count('preprocess_indexed_kernel') == 2 + 1, tr.kernels          # 6 samples = two batches, 3 samples = one
    assert tr.count('top1_tally_kernel') == 3, tr.kernels
    assert not tr.ran('preprocess_kernel') and not tr.ran('gather_clips') and not tr.ran('preprocess_clips'), tr.kernels
    clips = []
    for d, start, total in SEGMENTS:
        idx = [n - 1 for n in sg.sample(total, 8, start)]
        clips.append(transform_oracle.test_transform(_video(d)[idx].permute(0, 3, 1, 2).float(), 256, 224, True))
    x = torch.stack(clips)
    want = torch.cat([engine.forward_device(x[a:a + 4].cuda()) for a in range(0, x.shape[0], 4)]).cpu().numpy()
    got = res['logits']
    assert got.dtype == np.float32 and got.shape == (len(SEGMENTS), 12)
    print(f'max |indexed - host transform| {np.abs(got - want).max():.3g}, logit scale {np.abs(want).max():.3g}')
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-4)
    assert res['preds'] == got.argmax(axis=1).tolist()
    correct, total = sg.tally(res['preds'], labels, 12)
    assert res['correct'] == correct and res['total'] == total
    assert sum(total) == 8 and sum(correct) == 5
    assert res['acc'] == [c / n if n else None for c, n in zip(correct, total)] and res['overall'] == 5 / 8
    # a smaller batch: more launches, the same result
    with launch_trace() as tr:
        small = eval_classification(engine, _samples(labels), frame_reader=_reader, batch_clips=2, return_logits=True)
    assert tr.count('preprocess_indexed_kernel') == 3 + 2 and tr.count('top1_tally_kernel') == 5, tr.kernels
    _consistent(small, labels, got)


def test_a_directory_beyond_the_staging_budget_is_staged_in_pieces_of_whole_samples(engine, labels, monkeypatch):
    """The budget shrunk to 12 frames of the larger directory: its 6 samples go in several pieces, each staging only its own
    union.  (Other batches may take other conv kernels: the logits are held to the pipeline bar against the whole-directory run,
    preds and counters to the run's own logits.)"""
    from workoutdetector_amd import inference_count as ic
    from workoutdetector_amd.classification import eval_classification
    from workoutdetector_amd.engine import launch_trace
    whole = eval_classification(engine, _samples(labels), frame_reader=_reader, return_logits=True)
    monkeypatch.setattr(ic, 'MAX_STAGE_BYTES', 12 * 48 * 36 * 3)
    asked = []

    def reader(frame_dir, numbers):
        asked.append((frame_dir, len(numbers)))
        return _reader(frame_dir, numbers)

    with launch_trace() as tr:
        pieces = eval_classification(engine, _samples(labels), frame_reader=reader, return_logits=True)
    assert tr.count('preprocess_indexed_kernel') > 3 and tr.count('top1_tally_kernel') == tr.count('preprocess_indexed_kernel')
    assert all(n <= 12 for _d, n in asked), asked
    _consistent(pieces, labels, whole['logits'])


def test_whole_path_under_poison_gives_the_same_result(engine, sd0, labels):
    """TSM_POISON=1: every device buffer of the engine between poisoned bands, activations poisoned before each forward."""
    from workoutdetector_amd.classification import eval_classification
    clean = eval_classification(engine, _samples(labels), frame_reader=_reader, return_logits=True)
    eng = _make_engine(sd0, poison=True)
    try:
        poisoned = eval_classification(eng, _samples(labels), frame_reader=_reader, return_logits=True)
    finally:
        eng.close()
    assert np.array_equal(poisoned.pop('logits'), clean.pop('logits'))
    assert poisoned == clean


def test_an_identity_engine_is_refused_up_front(engine):
    from workoutdetector_amd.classification import eval_classification

    class Identity:
        consensus_type = 'identity'
        num_class, num_segments, max_clips, packed_layout = 12, 8, 4, engine.packed_layout
        forward_device = None

    asked = []
    with pytest.raises(ValueError, match='identity'):
        eval_classification(Identity(), _samples([0] * len(SEGMENTS)), frame_reader=lambda d, n: asked.append(d))
    assert asked == []


def test_the_reader_is_asked_for_one_probe_frame_then_every_pieces_union_without_it(engine, labels, monkeypatch):
    """What the engine path asks of the frame reader and of the GPU, to the call: per directory ONE read of its smallest sampled
    frame, then per staged piece one read of the piece's union without that frame; no read and no launch for an empty list; the
    same launches in the same order whether or not the logits are asked for; frames of another size than the probe's refused."""
    from workoutdetector_amd import inference_count as ic
    from workoutdetector_amd.classification import eval_classification
    from workoutdetector_amd.engine import launch_trace
    asked = []

    def reader(frame_dir, numbers):
        asked.append((frame_dir, list(numbers)))
        return _reader(frame_dir, numbers)

    rows = {d: [sg.sample(t, 8, s) for dd, s, t in SEGMENTS if dd == d] for d in DIRS}
    union = {d: sorted(set().union(*rows[d])) for d in DIRS}
    with launch_trace() as with_logits:
        res = eval_classification(engine, _samples(labels), frame_reader=reader, return_logits=True)
    assert asked == [('stu1', union['stu1'][:1]), ('stu1', union['stu1'][1:]), ('stu5', union['stu5'][:1]), ('stu5', union['stu5'][1:])]
    with launch_trace() as without:
        plain = eval_classification(engine, _samples(labels), frame_reader=_reader)
    assert without.kernels == with_logits.kernels and plain == {k: v for k, v in res.items() if k != 'logits'}
    starts = [i for i, k in enumerate(without.kernels) if 'preprocess_indexed_kernel' in k]
    assert len(starts) == 3 and starts[0] == 0 and 'top1_tally_kernel' in without.kernels[-1]      # per batch: transform, forward, tally
    assert all('top1_tally_kernel' in without.kernels[i - 1] for i in starts[1:])
    # pieces: the budget of 12 frames of the larger directory (11 of the other); a piece's read leaves the probed frame out
    budget = 12 * 48 * 36 * 3
    monkeypatch.setattr(ic, 'MAX_STAGE_BYTES', budget)
    del asked[:]
    eval_classification(engine, _samples(labels), frame_reader=reader)
    want = []
    for d, (_seed, _frames, h, w) in DIRS.items():
        pieces, cur = [], set()
        for r in rows[d]:
            if cur and len(cur | set(r)) * h * w * 3 > budget:
                pieces.append(cur)
                cur = set()
            cur |= set(r)
        want += [(d, union[d][:1])] + [(d, sorted(p - {union[d][0]})) for p in pieces + [cur]]
    assert asked == want and len(want) > 4 + 1, asked
    monkeypatch.undo()
    del asked[:]
    with launch_trace() as tr:
        empty = eval_classification(engine, [], frame_reader=reader, return_logits=True)
    assert asked == [] and tr.kernels == [] and empty['preds'] == [] and empty['overall'] is None and empty['logits'].shape == (0, 12)

    def mixed(frame_dir, numbers):                                     # every frame but the probed one is a row short
        got = _reader(frame_dir, numbers)
        return got if len(numbers) == 1 else got[:, :-1]
    with launch_trace() as tr:
        with pytest.raises(ValueError, match=r'stu1: frames of \(47, 36\) and \(48, 36\) pixels'):
            eval_classification(engine, _samples(labels), frame_reader=mixed)
    assert tr.kernels == []
