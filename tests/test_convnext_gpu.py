"""ConvNeXt-Base image engines (``TsmEngine(base_model='convnext_base')``, include/tsm_hip.h: tsm_set_convnext) on the GPU.

Shallow engines, depths (1, 1, 2, 1), unless a test says otherwise: every kernel and every width runs, an engine is built in
well under a second.  Frame sizes: 64 x 64 (maps 16, 8, 4, 2: at 4 x 4 and 2 x 2 every 7 x 7 window is mostly padding),
80 x 80 (20, 10, 5, 2: a floor drops a row and a column, and 10, 5 and 2 are no whole number of 4 x 4 tiles), 36 x 36 (9, 4, 2, 1:
only the centre tap exists on the 1 x 1 map) and 64 x 96 (not square).

Bars.  Per operator, through taps: from the engine's own tap in front of an operator the float64 result of exactly that
operator (tests/_convnext.py), at the project's per-op bar, rtol 1e-4 + 1e-4 of the tensor's scale.  Whole network, full depth
(3, 3, 27, 3): logits at rtol 1e-3 + 1e-5 of the scale, taps at rtol 1e-3 + 3e-5 of the scale -- the engine bars of the other
backbones' tests.  Everything that compares two runs of the engine is bit for bit."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _convnext as cn
from tests import _convnext_cases as cc
from tests import _image_path as ip
from tests._guard import guarded, guarded_out
from tests._util import assert_close

pytestmark = pytest.mark.gpu

SHALLOW = (1, 1, 2, 1)
FULL = (3, 3, 27, 3)
SIZES = ((64, 64), (80, 80), (36, 36), (64, 96))
OP_BAR = dict(rtol=1e-4, atol_scale=1e-4)
LOGITS_BAR = dict(rtol=1e-3, atol_scale=1e-5)
TAP_BAR = dict(rtol=1e-3, atol_scale=3e-5)
NUM_CLASS = 5
KNOBS = ('TSM_AUTOTUNE', 'TSM_POISON')


@functools.lru_cache(maxsize=None)
def _sd(depths, seed=0, num_class=NUM_CLASS):
    from workoutdetector_amd.weights import make_state_dict
    sd = make_state_dict(seed, num_class, 'convnext_base', depths=depths)
    for v in sd.values():
        v.setflags(write=False)
    return sd


@functools.lru_cache(maxsize=None)
def _frames(h, w, n=3, seed=11):
    """[n, 1, 3, h, w] float32 noise; the LAST frame is all zero (its stem output is the stem's bias in every pixel)."""
    x = np.random.default_rng([seed, h, w]).standard_normal((n, 1, 3, h, w)).astype(np.float32)
    x[-1] = 0.0
    x.setflags(write=False)
    return x


def _engine(h, w, depths=SHALLOW, max_clips=3, sd=None, autotune=False, poison=False, num_class=NUM_CLASS):
    """TSM_AUTOTUNE / TSM_POISON are read in tsm_create: set for the constructor only, then restored."""
    from workoutdetector_amd.engine import TsmEngine
    keep = {k: os.environ.get(k) for k in KNOBS}
    os.environ['TSM_AUTOTUNE'] = '1' if autotune else '0'
    os.environ.pop('TSM_POISON', None)
    if poison:
        os.environ['TSM_POISON'] = '1'
    try:
        return TsmEngine(num_class=num_class, num_segments=1, height=h, width=w, is_shift=False, max_clips=max_clips,
                         state_dict=sd if sd is not None else _sd(depths, num_class=num_class), base_model='convnext_base', convnext_depths=depths)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- per kernel, through taps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_every_operator_against_float64_from_the_tap_in_front_of_it(hip_lib, size, capsys):
    """dwconv7 + LayerNorm in all four widths, fc1 + GELU, fc2 + layer scale + residual, the three downsamples (LayerNorm + 2x2
    conv), the stem, the pool and the head LayerNorm: each from the engine's tap in front of it.  The last frame is all zero."""
    h, w = size
    sd, x = _sd(SHALLOW), _frames(h, w)
    eng = _engine(h, w)
    try:
        taps = {}

        def tap(name):
            if name not in taps:
                taps[name] = eng.forward_tap(x, name)
            return taps[name]

        worst = {}

        def close(name, want, what):
            worst[what] = max(worst.get(what, 0.0), assert_close(tap(name), want, what=f'{name} ({what}) at {h}x{w}', **OP_BAR))

        for name, what, want in cc.operator_cases(sd, SHALLOW, x, tap):
            close(name, want, what)
        # the all-zero frame: the stem's bias through its LayerNorm in every pixel, the same bits everywhere
        stem = tap('stem')
        bias_row = cn.layer_norm(sd['stem.0.bias'], sd['stem.1.weight'], sd['stem.1.bias'])
        assert (_bits(stem[2]) == _bits(stem[2])[0, 0]).all(), 'the zero frame\'s stem output is not constant over the pixels'
        assert_close(stem[2, 0, 0], bias_row, what='stem of the zero frame', **OP_BAR)
    finally:
        eng.close()
    with capsys.disabled():
        print(f'\n[convnext per-op {h}x{w}] max|err|/scale: ' + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()))


# ---- determinism ----------------------------------------------------------------------------------------------------------
def test_a_frame_does_not_depend_on_its_batch(hip_lib):
    """Three frames through max_clips = 2 (a forward of two, then of one) equal their single-frame forwards bit for bit; the
    same for the .dwln tap of every width, a pair of frames against each alone.  80 x 80: most maps are no whole number of tiles and
    the lane groups of one workgroup hold tiles of different frames."""
    h, w = 80, 80
    x = _frames(h, w)
    eng = _engine(h, w, max_clips=2)
    try:
        together = eng.forward_host(x)
        alone = np.concatenate([eng.forward_host(x[i:i + 1]) for i in range(3)])
        assert together.shape == (3, NUM_CLASS) and np.array_equal(_bits(together), _bits(alone))
        assert not np.array_equal(together[0], together[1])
        for s in range(4):
            name = f'stages.{s}.blocks.0.dwln'
            pair = eng.forward_tap(x[:2], name)
            for i in range(2):
                assert np.array_equal(_bits(pair[i:i + 1]), _bits(eng.forward_tap(x[i:i + 1], name))), (name, i)
    finally:
        eng.close()


# ---- residual path --------------------------------------------------------------------------------------------------------
def test_gamma_zero_leaves_the_block_input_bit_for_bit(hip_lib):
    """With gamma = 0 in one block its output is its input, to the bit: the residual path adds x and nothing else."""
    sd = dict(_sd(SHALLOW))
    sd['stages.1.blocks.0.gamma'] = np.zeros(256, dtype=np.float32)
    x = _frames(64, 64)
    eng = _engine(64, 64, sd=sd)
    try:
        xin, out = eng.forward_tap(x, 'stages.1.downsample'), eng.forward_tap(x, 'stages.1.blocks.0')
        other_in, other_out = eng.forward_tap(x, 'stages.2.downsample'), eng.forward_tap(x, 'stages.2.blocks.0')
    finally:
        eng.close()
    assert np.array_equal(_bits(xin), _bits(out))
    assert not np.array_equal(other_in, other_out)


# ---- whole network --------------------------------------------------------------------------------------------------------
FULL_TAPS = ('stem', 'stages.1.blocks.2', 'stages.2.blocks.26', 'stages.3.blocks.2')


@functools.lru_cache(maxsize=None)
def _full_reference():
    x = _frames(64, 64, n=2, seed=23)
    x = np.array(x)
    x[-1] = np.random.default_rng(5).standard_normal(x[-1].shape).astype(np.float32)       # (no zero frame here)
    return x, cn.forward(_sd(FULL), x[:, 0], FULL, keep=FULL_TAPS)


@pytest.fixture(scope='module')
def full_engine(hip_lib):
    eng = _engine(64, 64, depths=FULL, max_clips=2)
    yield eng
    eng.close()


def test_full_depth_logits_taps_and_features_against_float64(full_engine, capsys):
    x, ref = _full_reference()
    assert all(0.5 < r < 100.0 for r in ref['rms']), ref['rms']
    got = full_engine.forward_host(x)
    e_logits = assert_close(got, ref['logits'], what='logits', **LOGITS_BAR)
    errs = {name: assert_close(full_engine.forward_tap(x, name), ref[name], what=name, **TAP_BAR) for name in FULL_TAPS}
    feats = full_engine.forward_features(x)
    e_feat = assert_close(feats, ref['head.norm'], what='forward_features vs LN(pool)', **LOGITS_BAR)
    unit = full_engine.forward_features(x, normalize=True)
    assert_close(unit, ref['head.norm'] / np.linalg.norm(ref['head.norm'], axis=1, keepdims=True), what='unit rows', **LOGITS_BAR)
    with capsys.disabled():
        print(f'\n[convnext_base full depth 2x64x64] max|err|/scale: logits {e_logits:.3g}, features {e_feat:.3g}, '
              + ', '.join(f'{k} {v:.3g}' for k, v in errs.items()))


def test_full_depth_tuned_and_poisoned_equal_plain_bit_for_bit(full_engine):
    """The tile choices of the autotuner change no bit, and neither does TSM_POISON=1 (every buffer between poisoned bands,
    the workspace poisoned before the forward, the bands verified after it: a guard error would raise)."""
    x, _ = _full_reference()
    plain = full_engine.forward_host(x)
    for kw in (dict(autotune=True), dict(poison=True)):
        eng = _engine(64, 64, depths=FULL, max_clips=2, **kw)
        try:
            got = eng.forward_host(x)
            tap = eng.forward_tap(x, 'stages.2.blocks.13.dwln') if kw.get('poison') else None
            if kw.get('autotune'):
                tiles = eng.conv_tiles(2)
                assert len(tiles) == 76 and all(v != 'heuristic' for v in tiles.values()), tiles
        finally:
            eng.close()
        assert np.array_equal(_bits(got), _bits(plain)), kw
        if tap is not None:
            assert np.array_equal(_bits(tap), _bits(full_engine.forward_tap(x, 'stages.2.blocks.13.dwln')))


# ---- launch trace ---------------------------------------------------------------------------------------------------------
def test_launch_trace_of_the_full_depth_forward(full_engine):
    from workoutdetector_amd.engine import launch_trace
    x, _ = _full_reference()
    with launch_trace() as tr:
        full_engine.forward_host(x)
    want = {'pack_input_kernel<': 1, 'stem_pack4_kernel': 1, 'conv_igemm<': 76, 'ln_kernel<128, S2D> [S2D = false]': 1,
            'ln_kernel<1024, S2D> [S2D = false]': 1, 'ln_kernel<128, S2D> [S2D = true]': 1, 'ln_kernel<256, S2D> [S2D = true]': 1,
            'ln_kernel<512, S2D> [S2D = true]': 1, 'dwconv7_ln_kernel<128>': 3, 'dwconv7_ln_kernel<256>': 3, 'dwconv7_ln_kernel<512>': 27,
            'dwconv7_ln_kernel<1024>': 3, 'gelu_kernel': 36, 'pool_feat_kernel<kPrecF32>': 1, 'head_pool_kernel<kPrecF32>': 1, 'head_fc_kernel': 1}
    got = {k: tr.count(k) for k in want}
    assert got == want and len(tr.kernels) == sum(want.values()), (got, sorted(set(tr.kernels)))
    assert tr.count('dwconv7_ln_kernel') == 36
    names = full_engine.launch_names()
    assert len(names) == len(tr.kernels) - 1 and names[-1] == 'head'          # (the head slot is launch_head's two kernels)
    full_engine.set_layer_timing(1)
    full_engine.forward_host(x)
    times = full_engine.layer_times_ms(0)
    assert list(times) == names and all(v >= 0 for v in times.values())


def test_a_resnet_image_engine_launches_none_of_the_new_kernels(hip_lib):
    from workoutdetector_amd.engine import create_image_model, launch_trace
    eng = create_image_model(num_class=2, base_model='resnet18', max_frames=2, resize=64, crop=64)
    try:
        with launch_trace() as tr:
            eng.forward_host(np.array(_frames(64, 64, n=2)))
    finally:
        eng.close()
    assert tr.kernels and not any(k.startswith(('dwconv7_ln_kernel', 'ln_kernel', 'stem_pack4_kernel', 'gelu_kernel')) for k in tr.kernels), tr.kernels


# ---- the setter's contract ------------------------------------------------------------------------------------------------
def test_set_convnext_contract(hip_lib):
    """tsm_set_convnext: TSM_ERR_UNSUPPORTED (-7) with its reason on an engine with num_segments != 1, with is_shift, of another
    dtype, for a depth outside 1 .. 64 and after tsm_set_backbone / tsm_set_non_local / tsm_set_temporal_pool; the ResNet setters
    are refused in turn on a ConvNeXt engine; TSM_ERR_INVALID_ARG (-1) after the first tensor and for depths == NULL; the keys
    of the topology are timm's, and no other engine knows them."""
    import ctypes as C
    from workoutdetector_amd import _lib
    lib = hip_lib
    base = (C.c_int32 * 4)(*FULL)

    def engine(t=1, shift=0, dtype=_lib.DTYPE_F32):
        cfg = _lib.TsmConfig(C.sizeof(_lib.TsmConfig), 3, t, 64, 64, 8, shift, 1, 0, dtype)
        h = C.c_void_p()
        _lib.check(lib.tsm_create(C.byref(cfg), C.byref(h)))
        return h

    def refused(h, code, text, depths=base):
        assert lib.tsm_set_convnext(h, depths) == code
        assert text in lib.tsm_last_error(h).decode(), lib.tsm_last_error(h)

    for kw, text in ((dict(t=8), 'num_segments must be 1'), (dict(shift=1), 'is_shift must be 0'), (dict(dtype=_lib.DTYPE_BF16X3), 'TSM_DTYPE_F32 only'),
                     (dict(dtype=_lib.DTYPE_BF16), 'TSM_DTYPE_F32 only')):
        h = engine(**kw)
        refused(h, -7, text)
        lib.tsm_destroy(h)
    h = engine()
    refused(h, -7, '1 .. 64', (C.c_int32 * 4)(3, 0, 27, 3))
    refused(h, -7, '1 .. 64', (C.c_int32 * 4)(3, 3, 65, 3))
    refused(h, -1, 'depths is NULL', None)
    assert lib.tsm_set_convnext(h, base) == 0 and lib.tsm_set_convnext(h, (C.c_int32 * 4)(*SHALLOW)) == 0      # (the last call holds)
    for call in (lambda: lib.tsm_set_backbone(h, 18), lambda: lib.tsm_set_bottleneck_width(h, 128), lambda: lib.tsm_set_shift_place(h, 1),
                 lambda: lib.tsm_set_non_local(h, 1), lambda: lib.tsm_set_temporal_pool(h, 1)):
        assert call() == -7 and 'ConvNeXt engine' in lib.tsm_last_error(h).decode()
    one = np.ones(1024, np.float32)
    shape = (C.c_int64 * 1)(256)
    assert lib.tsm_set_tensor(h, b'stages.2.blocks.1.gamma', one.ctypes.data, (C.c_int64 * 1)(512), 1) == 0
    assert lib.tsm_set_tensor(h, b'stages.2.blocks.2.gamma', one.ctypes.data, (C.c_int64 * 1)(512), 1) == -1        # SHALLOW has two blocks there
    assert lib.tsm_set_tensor(h, b'stages.1.downsample.1.bias', one.ctypes.data, shape, 1) == 0
    assert lib.tsm_set_tensor(h, b'stages.0.downsample.1.bias', one.ctypes.data, shape, 1) == -1
    assert lib.tsm_set_tensor(h, b'base_model.conv1.weight', one.ctypes.data, shape, 1) == -1
    refused(h, -1, 'must come before the first tsm_set_tensor')
    assert lib.tsm_finalize(h) == -4 and 'missing' in lib.tsm_last_error(h).decode()
    lib.tsm_destroy(h)
    for setter, arg in ((lib.tsm_set_backbone, 50), (lib.tsm_set_non_local, 1)):
        h = engine(dtype=_lib.DTYPE_F32)
        assert setter(h, arg) == 0
        refused(h, -7, 'excludes')
        lib.tsm_destroy(h)
    h = engine(t=8, shift=1)
    assert lib.tsm_set_temporal_pool(h, 1) == 0
    refused(h, -7, 'num_segments must be 1')
    assert lib.tsm_set_tensor(h, b'stem.0.weight', one.ctypes.data, shape, 1) == -1          # a ResNet engine does not know timm's keys
    lib.tsm_destroy(h)


# ---- stream capture -------------------------------------------------------------------------------------------------------
def test_forward_captured_on_a_side_stream_replays_the_eager_logits(hip_lib):
    from tests._capture import captured
    h, w, b = 64, 64, 2
    sets = [torch.from_numpy(np.random.default_rng([41, k]).standard_normal((b, 1, 3, h, w)).astype(np.float32)) for k in range(3)]
    eng = _engine(h, w, max_clips=b)
    try:
        x = guarded(torch.zeros(b, 1, 3, h, w).cuda(), name='clips')
        out = guarded_out(eng._out_shape(b), name='logits')
        eng.warmup([b])
        tr = captured(lambda: eng.forward_device(x, out=out), [x], lambda k: [sets[k]], [out], engine=eng)
        want = cn.forward(_sd(SHALLOW), sets[0][:, 0].numpy(), SHALLOW)['logits']
    finally:
        eng.close()
    assert tr.count('dwconv7_ln_kernel') == sum(SHALLOW) and tr.count('conv_igemm<') == 1 + 3 + 2 * sum(SHALLOW)
    assert_close(tr.refs['A'][0].cpu().numpy(), want, what='captured forward, set A', **LOGITS_BAR)


# ---- image path -----------------------------------------------------------------------------------------------------------
RESIZE, CROP, N_VIDEO = 72, 64, 22


@functools.lru_cache(maxsize=None)
def _video():
    rng = np.random.default_rng(77)
    frames = rng.integers(0, 256, size=(N_VIDEO, 45, 60, 3), dtype=np.uint8)
    for a in range(0, N_VIDEO, 10):
        frames[a:a + 5] //= 6                   # dark and bright stretches of five frames
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def _image_reference():
    """(state dict with the classifier's bias moved into the widest central gap of the margins, float64 logits of it)."""
    from workoutdetector_amd.transform import ImageTransform
    sd = dict(_sd(FULL, num_class=2))
    x = ImageTransform(RESIZE, CROP)(np.array(_video())).numpy()
    logits = cn.forward(sd, x, FULL)['logits']
    margin = np.sort(logits[:, 0] - logits[:, 1])
    lo, hi = N_VIDEO // 4, N_VIDEO - N_VIDEO // 4
    k = lo + int(np.argmax(np.diff(margin[lo:hi])))
    shift = 0.5 * (margin[k] + margin[k + 1])
    bias = sd['head.fc.bias'].copy()
    bias[1] += np.float32(shift)
    sd['head.fc.bias'] = bias
    logits = logits + np.array([0.0, float(np.float32(shift))])
    return sd, logits, float(margin[k + 1] - margin[k])


def test_image_path_from_a_lightning_checkpoint_with_timm_keys(hip_lib, tmp_path, capsys):
    """create_image_model(base_model='convnext_base', checkpoint=<timm keys under 'classifier.'>) -> inference_images and
    count_by_image_model: logits against the float64 model on transform.ImageTransform's output, states and count equal the
    host vote; one preprocess launch, one forward and one vote launch per batch."""
    from workoutdetector_amd import inference_count as ic
    from workoutdetector_amd.counting import pred_to_count
    from workoutdetector_amd.engine import create_image_model, launch_trace
    sd, want, gap = _image_reference()
    video = np.array(_video())
    preds = want.argmax(axis=1)
    scale = float(np.abs(want).max())
    assert 0 < preds.sum() < N_VIDEO and gap > 1e-2 * scale, (preds, gap, scale)      # both classes; no frame near the decision
    states = ip.reference_vote(preds)
    path = str(tmp_path / 'lit_convnext.ckpt')
    torch.save({'state_dict': {'classifier.' + k: torch.from_numpy(np.array(v)) for k, v in sd.items()}}, path)
    keep = os.environ.get('TSM_AUTOTUNE')
    os.environ['TSM_AUTOTUNE'] = '0'
    try:
        eng = create_image_model(num_class=2, base_model='convnext_base', checkpoint=path, resize=RESIZE, crop=CROP, max_frames=8)
    finally:
        os.environ.pop('TSM_AUTOTUNE', None)
        if keep is not None:
            os.environ['TSM_AUTOTUNE'] = keep
    try:
        assert (eng.base_model, eng.convnext_depths, eng.num_segments, eng.feature_dim, eng.max_clips) == ('convnext_base', FULL, 1, 1024, 8)
        got = ic.inference_images(eng, video)
        with launch_trace() as tr:
            got_states, rows = ic.image_states(eng, video, batch_frames=8, return_scores=True)
        counted = ic.count_by_image_model(eng, list(video), batch_frames=5)
    finally:
        eng.close()
    err = assert_close(got, want, what='inference_images vs float64 on ImageTransform', **LOGITS_BAR)
    assert_close(rows, want, what='image_states scores', **LOGITS_BAR)
    nb = -(-N_VIDEO // 8)
    assert tr.count('preprocess_image_kernel') == nb and tr.count('frame_votes_kernel') == nb and tr.count('head_fc_kernel') == nb, tr.kernels
    assert tr.count('dwconv7_ln_kernel') == 36 * nb and not tr.ran('preprocess_kernel')
    assert got_states == states and counted == pred_to_count(states, step=7)
    with capsys.disabled():
        print(f'\n[convnext image path] logits max|err|/scale {err:.3g}; preds {preds.tolist()} states {states} count {counted[0]}')


def test_video_features_of_a_convnext_engine(hip_lib):
    """similarity.video_features drives forward_features of a ConvNeXt engine unchanged: rows = LayerNorm(pool), against the
    float64 model on the normalised frames (64 x 64 frames at resize = crop = 64: the transform only normalises)."""
    from workoutdetector_amd import similarity
    frames = np.random.default_rng(3).integers(0, 256, size=(5, 64, 64, 3), dtype=np.uint8)
    eng = _engine(64, 64, max_clips=4)
    eng.image_resize, eng.image_crop = 64, 64
    try:
        feats = similarity.video_features(eng, frames).cpu().numpy()
        unit = similarity.video_features(eng, frames, normalize=True, batch_frames=2).cpu().numpy()
        dist = similarity.self_similarity(eng, frames).cpu().numpy()
    finally:
        eng.close()
    want = cn.forward(_sd(SHALLOW), ip.normalised(frames).transpose(0, 3, 1, 2), SHALLOW)['head.norm']
    assert_close(feats, want, what='video_features', **LOGITS_BAR)
    assert_close(unit, want / np.linalg.norm(want, axis=1, keepdims=True), what='unit rows', **LOGITS_BAR)
    assert dist.shape == (5, 5) and (np.diag(dist) == 0).all() and dist[0, 1] > 1e-4
