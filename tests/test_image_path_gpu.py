"""tsm_preprocess_image (Pillow's antialiased 8-bit resample + crop + normalise + pack in one launch) against Pillow's own
recorded output, tsm_frame_votes against the reference's loop, and the image-model path end to end on a real engine.

Every launch runs in hostile memory (tests/_guard.py): frames, tables and logits between poisoned bands, outputs poisoned
before the launch, bands and payload checked after it.

Bound of the fp32 layouts: the resample is integer arithmetic, so the kernel's uint8 must be Pillow's to the bit, and the
normalisation is three correctly rounded fp32 operations: |got - want| <= 2 ulps of want = ((u8 / 255) - mean) / std in NumPy
fp32 (the kernel may contract to an fma).  Adjacent grey levels are ~0.017 apart after normalisation: one uint8 off by one
misses the bound by four orders of magnitude.
"""
import os

import numpy as np
import pytest
import torch

from tests import _image_path as ip
from tests._guard import check, guarded, guarded_out
from tests._util import assert_close

pytestmark = pytest.mark.gpu

LAYOUTS = ('nthwc4', 'ntchw', 'nthwc8s', 'nthwc8b')


def _layout(name):
    from workoutdetector_amd import _lib
    return {'nthwc4': _lib.LAYOUT_NTHWC4, 'ntchw': _lib.LAYOUT_NTCHW, 'nthwc8s': _lib.LAYOUT_NTHWC8S,
            'nthwc8b': _lib.LAYOUT_NTHWC8B}[name]


def _shape(name, n, crop):
    pairs = (crop + 1) // 2
    return (n,) + {'nthwc4': (crop, crop, 4), 'ntchw': (3, crop, crop), 'nthwc8s': (crop, pairs, 8), 'nthwc8b': (crop, pairs, 4)}[name]


def _launch(frames, resize, crop, layout_name):
    """engine.preprocess_image in hostile memory: frames (uint8 ndarray [n,H,W,3]) and the table block as guarded views,
    the output poisoned."""
    from workoutdetector_amd.engine import preprocess_image
    from workoutdetector_amd.transform import image_tables
    n, h, w, _ = frames.shape
    src = guarded(torch.from_numpy(np.array(frames)).cuda(), name='frames')
    block = image_tables(h, w, resize, crop)
    tables = guarded(torch.from_numpy(block.copy()).cuda(), name='tables') if block.size else torch.zeros(0, dtype=torch.int32, device='cuda')
    out = guarded_out(_shape(layout_name, n, crop), name='out')
    assert preprocess_image(src, resize, crop, out_layout=_layout(layout_name), out=out, tables=tables) is out
    torch.cuda.synchronize()
    check(src, out, *([tables] if block.size else []))
    return out.cpu()


def _check_f32(got_nhwc3, want_u8, what):
    want = ip.normalised(want_u8)
    u = ip.ulps(got_nhwc3.numpy(), want)
    print(f'{what}: max {float(u.max()):.3g} ulp, max |err| {float(np.abs(got_nhwc3.numpy() - want).max()):.3g}')
    assert float(u.max()) <= 2.0, f'{what}: {float(u.max()):.3g} ulps'


@pytest.mark.parametrize('layout_name', LAYOUTS)
@pytest.mark.parametrize('name', ip.CASES)
def test_preprocess_image_is_pillow_to_the_bit(hip_lib, name, layout_name):
    """Every fixture x every layout x n in {1, 3}.  fp32 layouts: within 2 ulps of NumPy's normalisation of Pillow's bytes,
    pad channel exactly 0.  Pixel-pair layouts, by the rule the person-crop tests hold the same packing code to: bf16 = RNE of
    the kernel's own fp32 output (itself held to the 2 ulps), split hi the same and hi + lo within 2^-16 relative, pad channel and the odd pixel of an odd crop 0."""
    frames, want, resize, crop = ip.fixture(name)
    pairs = (crop + 1) // 2
    for n in (1, 3):
        what = f'{name} {layout_name} n={n}'
        got = _launch(frames[:n], resize, crop, layout_name)
        if layout_name == 'ntchw':
            _check_f32(got.permute(0, 2, 3, 1), want[:n], what)
            continue
        if layout_name == 'nthwc4':
            assert float(got[..., 3].abs().max()) == 0.0, what
            _check_f32(got[..., :3], want[:n], what)
            continue
        nchw = _launch(frames[:n], resize, crop, 'ntchw')
        _check_f32(nchw.permute(0, 2, 3, 1), want[:n], what + ' (its fp32 form)')
        f32 = nchw.permute(0, 2, 3, 1)                                                # [n,crop,crop,3]
        if layout_name == 'nthwc8b':
            val = hi = got.view(torch.bfloat16).reshape(n, crop, pairs * 2, 4).float()
        else:
            g = got.view(torch.bfloat16).reshape(n, crop, pairs, 2, 8).float()        # [hi x8 | lo x8] per pair
            hi = g[..., 0, :].reshape(n, crop, pairs * 2, 4)
            val = (g[..., 0, :] + g[..., 1, :]).reshape(n, crop, pairs * 2, 4)
        assert torch.equal(hi[..., :crop, :3], f32.to(torch.bfloat16).float()), what
        if layout_name == 'nthwc8s':
            assert bool(((val[..., :crop, :3] - f32).abs() <= f32.abs() * 2.0 ** -16 + 1e-30).all()), what
        halves = (hi,) if layout_name == 'nthwc8b' else (hi, g[..., 1, :].reshape(n, crop, pairs * 2, 4))
        for half in halves:                      # (each half on its own: a hi with lo = -hi is not a zero pad)
            assert float(half[..., 3].abs().max()) == 0.0, what
            if crop % 2:
                assert float(half[..., crop:, :].abs().max()) == 0.0, what


def test_support_reads_stop_at_the_row_and_the_frame_edge(hip_lib):
    """The frames are the MIDDLE of a larger staged buffer whose neighbours are hostile: the frame before and the frame
    behind are 0 / 255 checkerboards (a tap past the first or last row of a frame lands there; a tap past a row's end lands
    in the next row, which is noise).  The launch takes the [n,H,W,3] view; the result is still Pillow's."""
    from workoutdetector_amd.engine import preprocess_image
    frames, want, resize, crop = ip.fixture('tall')                  # 90 x 31: the window's support touches both side edges
    n, h, w, _ = frames.shape
    hostile = np.indices((h, w)).sum(axis=0) % 2 * 255
    buf = np.empty((n + 2, h, w, 3), dtype=np.uint8)
    buf[0] = buf[-1] = hostile[..., None]
    buf[1:-1] = frames
    dev = guarded(torch.from_numpy(buf).cuda(), name='staged')
    out = guarded_out((n, crop, crop, 4), name='out')
    preprocess_image(dev[1:-1], resize, crop, out=out)
    torch.cuda.synchronize()
    check(dev, out)
    _check_f32(out.cpu()[..., :3], want, 'view into a staged buffer')
    # a window that reaches the frame's corners: resize == crop, every edge tap of both passes is used
    f2, w2, r2, c2 = ip.fixture('upscale')
    assert r2 == c2
    got = _launch(f2, r2, c2, 'nthwc4')
    _check_f32(got[..., :3], w2, 'window = whole resized frame')


def test_the_launch_is_the_new_kernel_and_refusals_come_before_it(hip_lib):
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import launch_trace, preprocess_image
    frames, _want, resize, crop = ip.fixture('landscape')
    src = torch.from_numpy(np.array(frames)).cuda()
    with launch_trace() as tr:
        preprocess_image(src, resize, crop)
    assert tr.kernels == ['preprocess_image_kernel'] and not tr.ran('preprocess_kernel'), tr.kernels
    # a table block of another geometry, a crop larger than the resized frame: refused, nothing launched
    other = torch.zeros(7, dtype=torch.int32, device='cuda')
    for kw in (dict(resize=resize, crop=crop, tables=other), dict(resize=resize, crop=resize + 1)):
        with launch_trace() as tr:
            with pytest.raises((_lib.TsmError, ValueError)):
                preprocess_image(src, **kw)
        assert tr.kernels == [], tr.kernels
    # one output row's vertical support beyond 64 KB of LDS: TSM_ERR_UNSUPPORTED, nothing launched.  The smallest frame that
    # gets there: the support is ~2 * short / resize rows of ~3 * crop bytes with crop <= resize, i.e. ~6 * short bytes whatever
    # resize and crop are (8 * short at crop 1, whose 3-byte row is padded to 4), so short > 8190 and the frame >= 8200^2 x 3.
    huge = torch.zeros((1, 8200, 8200, 3), dtype=torch.uint8, device='cuda')
    with launch_trace() as tr:
        with pytest.raises(_lib.TsmError) as ei:
            preprocess_image(huge, 1, 1)
    assert ei.value.status == -7 and tr.kernels == [], (ei.value, tr.kernels)
    del huge


def test_the_old_transform_is_not_pillow_and_the_new_kernel_is(hip_lib):
    """Why the feature needed a kernel: tsm_preprocess (ATen's bilinear on floats, no antialias) on the 5.6x downscale does
    NOT meet the 2-ulp condition against Pillow -- it is grey levels away -- while tsm_preprocess_image does."""
    from workoutdetector_amd.engine import preprocess_frames
    frames, want, resize, crop = ip.fixture('tall')
    src = torch.from_numpy(np.array(frames)).cuda()
    old = preprocess_frames(src, resize=resize, crop=crop, scale_255=True).cpu()[..., :3].numpy()
    u = ip.ulps(old, ip.normalised(want))
    levels = np.abs(old - ip.normalised(want)) * 255.0 * ip.STD
    print(f'tsm_preprocess vs Pillow: max {float(u.max()):.3g} ulp, mean |diff| {float(levels.mean()):.3g} grey levels')
    assert float(u.max()) > 2.0 and float(levels.mean()) > 1.0
    _check_f32(_launch(frames, resize, crop, 'nthwc4')[..., :3], want, 'tsm_preprocess_image')


# ---- votes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [2, 5])
@pytest.mark.parametrize('n', [1, 6, 7, 8, 65, 130])
def test_frame_votes_equal_the_reference_loop_whole_and_in_batches(hip_lib, n, c):
    from workoutdetector_amd.engine import frame_votes, launch_trace
    x = ip.logits_with_ties(n * 10 + c, n, c)
    preds = x.argmax(axis=1)                                   # numpy: the first maximum
    want = ip.reference_vote(preds)

    def run(rows, history):
        logits = guarded(torch.from_numpy(rows).cuda(), name='logits')
        hist = None if history is None else guarded(history.clone(), name='history')
        out = (guarded_out((len(rows),), torch.int32, name='pred'), guarded_out((len(rows),), torch.int32, name='state'),
               guarded_out((6,), torch.int32, name='history_out'))
        with launch_trace() as tr:
            pred, state, new = frame_votes(logits, hist, out=out)
        assert tr.kernels == ['frame_votes_kernel'], tr.kernels
        torch.cuda.synchronize()
        check(logits, hist, *out)
        return pred.cpu().tolist(), state.cpu().tolist(), new

    pred, state, hist = run(x, None)
    assert pred == preds.tolist() and state == want
    assert hist.cpu().tolist() == preds.tolist()[-6:]
    for batch in (1, 3, 7, 64):
        if batch >= n and batch != 1:
            continue
        got_p, got_s, hist = [], [], None
        for a in range(0, n, batch):
            p, s, hist = run(x[a:a + batch], hist)
            got_p += p
            got_s += s
        assert got_p == preds.tolist() and got_s == want, (n, c, batch)


# ---- end to end ----------------------------------------------------------------------------------------------------------
RESIZE, CROP, FRAMES = 40, 32, 30
# The seeded R18 calls every frame of the video below class 0: on the CPU oracle its margin logit[1] - logit[0] lies between
# -5.9 and -1.5, the dark frames at the low end, with its widest gap between -5.11 and -4.38.  The checkpoint the engine loads
# has fc.bias[1] raised by BIAS_SHIFT, which puts the decision into that gap (no frame within 0.3 of it: the engine's fp32
# error, ~1e-3 relative, cannot flip one): the dark stretches become class 0 and the bright ones, but for one frame, class 1.
BIAS_SHIFT = 4.75


@pytest.fixture(scope='module')
def checkpoint(tmp_path_factory):
    """A torch.save'd state dict with plain torchvision keys (conv1.weight, layer1.0.conv1.weight, ..., fc.*)."""
    from workoutdetector_amd.weights import make_state_dict
    tv = {}
    for k, v in make_state_dict(0, 2, 'resnet18').items():
        tv[k[len('base_model.'):].replace('.conv1.net.', '.conv1.') if k.startswith('base_model.') else k] = torch.from_numpy(v.copy())
    tv['fc.bias'][1] += BIAS_SHIFT
    tv['bn1.num_batches_tracked'] = torch.tensor(0)
    path = str(tmp_path_factory.mktemp('ckpt') / 'image_r18.pth')
    torch.save(tv, path)
    return path


def _make_engine(checkpoint, poison):
    from workoutdetector_amd.engine import create_image_model
    keep = {k: os.environ.get(k) for k in ('TSM_AUTOTUNE', 'TSM_POISON')}
    os.environ['TSM_AUTOTUNE'] = '0'
    os.environ.pop('TSM_POISON', None)
    if poison:
        os.environ['TSM_POISON'] = '1'
    try:
        return create_image_model(num_class=2, checkpoint=checkpoint, resize=RESIZE, crop=CROP, max_frames=8)   # (TSM_* are read in tsm_create)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope='module')
def engine(hip_lib, checkpoint):
    eng = _make_engine(checkpoint, poison=False)
    yield eng
    eng.close()


@pytest.fixture(scope='module')
def video():
    rng = np.random.default_rng(77)
    frames = rng.integers(0, 256, size=(FRAMES, 45, 60, 3), dtype=np.uint8)
    for a in range(0, FRAMES, 10):
        frames[a:a + 5] //= 6                   # dark and bright stretches of five frames
    return frames


@pytest.fixture(scope='module')
def host_path(engine, video):
    """The same engine fed by the CPU ImageTransform, voted on the host: (scores, states, (count, reps))."""
    from workoutdetector_amd.counting import pred_to_count
    from workoutdetector_amd.transform import ImageTransform
    x = ImageTransform(RESIZE, CROP)(video).numpy()
    scores = engine.forward_host(x.reshape(FRAMES, 1, 3, CROP, CROP))
    states = ip.reference_vote(scores.argmax(axis=1))
    return scores, states, pred_to_count(states, step=7)


def test_the_video_exercises_the_vote(host_path):
    """What makes the comparisons below mean something: both classes occur, no frame is near the decision, the voted state
    changes several times, repetitions are counted, and for every batch size of the tests a frame's 7-frame window reaches
    into the previous batch with class-1 frames in it that decide its state -- dropping the history would change the states."""
    from workoutdetector_amd.counting import vote_states
    scores, states, (count, reps) = host_path
    preds = scores.argmax(axis=1).tolist()
    margin = np.abs(scores[:, 1] - scores[:, 0])
    print(f'preds {preds}\nstates {states}\ncount {count} reps {reps}; min |margin| {float(margin.min()):.3g}')
    assert preds == [0] * 5 + [1] * 5 + [0] * 5 + [1] * 5 + [0] * 6 + [1] * 4           # (frame 25, bright, stays below the gap)
    assert float(margin.min()) > 0.1
    assert 0 < sum(states) < len(states) and count >= 2 and len(reps) == 2 * count
    for batch in (1, 5, 8):
        forgetful = []
        for a in range(0, FRAMES, batch):
            forgetful += vote_states(preds[a:a + batch], [])[0]
        assert forgetful != states, batch


def test_image_engine_is_a_one_segment_unshifted_r18(engine):
    assert (engine.base_model, engine.num_segments, engine.height, engine.width, engine.max_clips) == ('resnet18', 1, CROP, CROP, 8)
    assert (engine.image_resize, engine.image_crop, engine.consensus_type, engine.num_class) == (RESIZE, CROP, 'avg', 2)


def test_inference_images_equals_the_engine_on_the_cpu_transform(engine, video, host_path):
    from workoutdetector_amd import inference_count as ic
    from workoutdetector_amd.engine import launch_trace
    scores = host_path[0]
    with launch_trace() as tr:
        got = ic.inference_images(engine, video)
    assert tr.count('preprocess_image_kernel') == 1 and not tr.ran('preprocess_kernel'), tr.kernels
    assert got.dtype == np.float32 and got.shape == (FRAMES, 2)
    assert_close(got, scores, rtol=1e-3, atol_scale=1e-5, what='inference_images vs forward_host(ImageTransform)')
    one = ic.inference_image(engine, video[4])
    assert one.shape == (2,) and one.dtype == np.float32
    assert_close(one[None], scores[4:5], rtol=1e-3, atol_scale=1e-5, what='inference_image')


@pytest.mark.parametrize('batch', [1, 5, 8, None])
def test_count_by_image_model_equals_the_host_path(engine, video, host_path, batch, tmp_path):
    from workoutdetector_amd import inference_count as ic
    from workoutdetector_amd.engine import launch_trace
    _scores, states, counted = host_path
    with launch_trace() as tr:
        got_states, rows = ic.image_states(engine, video, batch_frames=batch, return_scores=True)
    nb = -(-FRAMES // (batch or 8))
    assert tr.count('preprocess_image_kernel') == nb and tr.count('frame_votes_kernel') == nb, tr.kernels
    assert not tr.ran('preprocess_kernel') and not tr.ran('scores_to_states'), tr.kernels
    assert got_states == states
    assert_close(rows, host_path[0], rtol=1e-3, atol_scale=1e-5, what=f'scores, batch {batch}')
    path = str(tmp_path / 'pred')
    assert ic.count_by_image_model(engine, list(video), pred_out_path=path, batch_frames=batch) == counted
    assert os.path.exists(path + '.json')
    assert ic.count_by_image_model(engine, torch.from_numpy(np.array(video)), batch_frames=batch) == counted


def test_whole_image_path_under_poison_gives_the_same_states(engine, checkpoint, video, host_path):
    """TSM_POISON=1: every device buffer of the engine between poisoned bands, activations poisoned before each forward."""
    from workoutdetector_amd import inference_count as ic
    clean = ic.image_states(engine, video, batch_frames=5, return_scores=True)
    eng = _make_engine(checkpoint, poison=True)
    try:
        poisoned = ic.image_states(eng, video, batch_frames=5, return_scores=True)
    finally:
        eng.close()
    assert poisoned[0] == clean[0] == host_path[1]
    assert np.array_equal(poisoned[1], clean[1])
