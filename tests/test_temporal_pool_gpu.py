"""create_model(temporal_pool=True) on the MI355X: the pool launch bit for bit against torch.max_pool3d on the engine's own taps,
and the engine against the float64 torch model with the wrapper's module tree (tests/_temporal_pool.py).

Inputs are 64 x 64 (layer1 16 x 16, layer4 2 x 2; one case 80 x 80: 20 x 20 down to 3 x 3), seeded normal clips, two clips or more
wherever the shift matters: with one clip a stage that still shifted over T instead of T / 2 would read the same frames.  The non-square frames come from
tests/_geometry_cases.py (48 x 80, 80 x 48 and 90 x 70 with T = 6: layer1 23 x 18, three segments behind the pool); their tap shapes
are asserted from that table.

Bars.  The pool: ``torch.equal``.  Engine: the existing engine bars for f32 and bf16x3 alike (tests/test_bf16x3_gpu.py), logits
``rtol=1e-3, atol_scale=1e-5`` and taps ``rtol=1e-3, atol_scale=3e-5``."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _geometry_cases as G
from tests._temporal_pool import clip_input, last_block, run_with_taps, taps_of, torch_tsm_tp, wrapper_keys
from tests._util import assert_close

pytestmark = pytest.mark.gpu

R50, WRN, R18 = 'resnet50', 'wide_resnet50_2', 'resnet18'
POOL_KERNEL = 'temporal_maxpool_kernel'


@functools.lru_cache(maxsize=None)
def _sd(base_model=R50, place='blockres'):
    from workoutdetector_amd.weights import make_state_dict
    return make_state_dict(0, 12, base_model, place)


def _hw(size):
    return (size, size) if isinstance(size, int) else tuple(size)


def _frame_id(v):
    return '%dx%d' % v if isinstance(v, tuple) else None


def _engine(base_model=R50, place='blockres', T=8, size=64, consensus='avg', max_clips=2, dtype='f32', sd=None, temporal_pool=True):
    from workoutdetector_amd.engine import TsmEngine
    h, w = _hw(size)
    return TsmEngine(num_class=12, num_segments=T, height=h, width=w, max_clips=max_clips,
                     state_dict=sd if sd is not None else _sd(base_model, place), base_model=base_model, shift_place=place,
                     consensus_type=consensus, dtype=dtype, temporal_pool=temporal_pool)


def _pool_ref(x, T):
    """torch.max_pool3d over the frames of each clip of an NHWC tap [B * T, H, W, C] -> [B * T / 2, H, W, C]."""
    n, h, w, c = x.shape
    v = torch.from_numpy(x).view(n // T, T, h, w, c).permute(0, 4, 1, 2, 3)          # [B, C, T, H, W]
    v = F.max_pool3d(v, kernel_size=(3, 1, 1), stride=(2, 1, 1), padding=(1, 0, 0))
    return v.permute(0, 2, 3, 4, 1).reshape(n // 2, h, w, c).contiguous()


# ---- the pool launch, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'bf16x3'])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('T', [8, 4, 2])
def test_pool_equals_max_pool3d_bit_for_bit(hip_lib, T, B, dtype):
    x = clip_input(10 * T + B, B, T, 64, 64)
    eng = _engine(T=T, max_clips=B, dtype=dtype)
    before = eng.forward_tap(x, f'layer1.{last_block(R50, 1)}')
    after = eng.forward_tap(x, 'layer2.tpool')
    eng.close()
    assert before.shape == (B * T, 16, 16, 256) and after.shape == (B * T // 2, 16, 16, 256)
    want = _pool_ref(before, T)
    assert torch.equal(torch.from_numpy(after), want), f'T {T} B {B} {dtype}: {int((torch.from_numpy(after) != want).sum())} elements differ'
    if T == 2:
        assert np.array_equal(after, np.maximum(before[0::2], before[1::2]))
    # the pool is no copy: it must pick from the odd neighbours too
    assert not np.array_equal(after, before[0::2])


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3'])
@pytest.mark.parametrize('T', [8, 6, 2])
@pytest.mark.parametrize('hw', G.frames_of('temporal_pool'), ids=_frame_id)
def test_pool_equals_max_pool3d_bit_for_bit_on_non_square_frames(hip_lib, hw, T, dtype):
    """The frames of tests/_geometry_cases.py (layer1 12 x 20, 20 x 12 and the odd 23 x 18), three clips; T = 6 leaves three
    segments.  The tap shapes are the table's."""
    B, (h1, w1) = 3, G.maps_of('temporal_pool', *hw)['layer1']
    x = clip_input(10 * T + hw[0], B, T, *hw)
    eng = _engine(T=T, size=hw, max_clips=B, dtype=dtype)
    before = eng.forward_tap(x, f'layer1.{last_block(R50, 1)}')
    after = eng.forward_tap(x, 'layer2.tpool')
    eng.close()
    assert before.shape == (B * T, h1, w1, 256) and after.shape == (B * T // 2, h1, w1, 256)
    want = _pool_ref(before, T)
    assert torch.equal(torch.from_numpy(after), want), f'{hw} T {T} {dtype}: {int((torch.from_numpy(after) != want).sum())} elements differ'
    assert not np.array_equal(after, before[0::2])


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3'])
def test_three_clips_through_two_slots_equal_the_single_runs(hip_lib, dtype):
    x = clip_input(31, 3, 8, 64, 64)
    eng = _engine(dtype=dtype)
    all3 = eng.run(None, {'input': x})[0]
    assert all3.shape == (3, 12)
    pair = eng.forward_tap(x[:2], 'layer2.tpool')
    for c in range(3):
        assert np.array_equal(eng.run(None, {'input': x[c:c + 1]})[0][0], all3[c]), c
    for c in range(2):
        assert np.array_equal(eng.forward_tap(x[c:c + 1], 'layer2.tpool'), pair[4 * c:4 * c + 4]), c
    eng.close()


def test_three_clips_through_two_slots_on_a_non_square_frame(hip_lib):
    """90 x 70, T = 6: three segments a clip behind the pool, so clip c's pooled frames are rows 3 c .. 3 c + 2."""
    x = clip_input(31, 3, 6, 90, 70)
    eng = _engine(T=6, size=(90, 70))
    all3 = eng.run(None, {'input': x})[0]
    assert all3.shape == (3, 12)
    pair = eng.forward_tap(x[:2], 'layer2.tpool')
    assert pair.shape == (6, *G.maps_of('temporal_pool', 90, 70)['layer1'], 256)
    for c in range(3):
        assert np.array_equal(eng.run(None, {'input': x[c:c + 1]})[0][0], all3[c]), c
    for c in range(2):
        assert np.array_equal(eng.forward_tap(x[c:c + 1], 'layer2.tpool'), pair[3 * c:3 * c + 3]), c
    eng.close()


# ---- the engine against the float64 torch model --------------------------------------------------------------------------
# (base_model, shift_place, T, size, mode, dtype)
CASES = [(R50, 'blockres', 8, 64, 'avg', 'f32'), (R50, 'blockres', 4, 64, 'avg', 'f32'), (R50, 'blockres', 2, 64, 'avg', 'f32'),
         (R50, 'block', 8, 64, 'avg', 'f32'), (WRN, 'blockres', 8, 64, 'avg', 'f32'), (R18, 'blockres', 8, 64, 'avg', 'f32'),
         (R50, 'blockres', 8, 64, 'identity', 'f32'), (R50, 'blockres', 8, 64, 'features', 'f32'),
         (R50, 'blockres', 8, 64, 'avg', 'bf16x3'), (R50, 'blockres', 8, 80, 'avg', 'f32')]
# the non-square frames of tests/_geometry_cases.py (size = (h, w)); 90 x 70 with T = 6: an odd segment count behind the pool
CASES += [(R50, 'blockres', c['T'], (c['h'], c['w']), 'avg', c['dtype']) for c in G.TEMPORAL_POOL]
CASES += [(R50, 'blockres', 6, (90, 70), 'identity', 'f32')]
STAGE_MAPS = {'layer2.0': ('layer2', 512), 'layer3.1': ('layer3', 1024), 'layer4.2': ('layer4', 2048)}


@functools.lru_cache(maxsize=None)
def _reference(base_model, place, T, size):
    """The float64 torch model's outputs for the seeded weights and this configuration's two clips: computed once."""
    h, w = _hw(size)
    x = clip_input(100 + size + T if isinstance(size, int) else 100 + h + w + T, 2, T, h, w)
    net = torch_tsm_tp(base_model, place, 12, T, sd=_sd(base_model, place))
    logits, seg, pooled, taps = run_with_taps(net, x, taps_of(base_model))
    return x, logits, seg, pooled, taps


@pytest.mark.parametrize('base_model,place,T,size,mode,dtype', CASES, ids=_frame_id)
def test_engine_against_float64_torch(hip_lib, base_model, place, T, size, mode, dtype):
    x, logits, seg, pooled, taps = _reference(base_model, place, T, size)
    eng = _engine(base_model, place, T, size, 'identity' if mode == 'identity' else 'avg', dtype=dtype)
    what = f'{base_model} {place} T{T} {"%dx%d" % _hw(size)} {mode} {dtype}'
    maps = G.maps_of('temporal_pool', *size) if isinstance(size, tuple) else None
    assert eng.out_segments == T // 2
    if mode == 'features':
        got = eng.forward_features(x)
        assert got.shape == (2 * (T // 2), eng.feature_dim)
        assert_close(got, pooled, rtol=1e-3, atol_scale=1e-5, what=what + ' features')
    else:
        got = eng.run(None, {'input': x})[0]
        assert got.shape == ((2, T // 2, 12) if mode == 'identity' else (2, 12))
        assert eng.get_outputs()[0].shape == [None] + list(got.shape[1:])
        assert_close(got, seg if mode == 'identity' else logits, rtol=1e-3, atol_scale=1e-5, what=what + ' logits')
    for stage in ('layer2.0', 'layer3.1', f'layer4.{last_block(base_model, 4)}'):
        tap = eng.forward_tap(x, stage)
        assert tap.shape[0] == 2 * (T // 2)
        if maps is not None:                                    # a frame of the table: the whole shape, from the table
            assert tap.shape == (2 * (T // 2), *maps[STAGE_MAPS[stage][0]], STAGE_MAPS[stage][1]), (stage, tap.shape)
        assert_close(tap, taps[stage], rtol=1e-3, atol_scale=3e-5, what=f'{what} {stage}')
    eng.close()


def test_device_forward_and_the_wrapper_spelling(hip_lib):
    """forward_device gives the host path's bits in the pooled shapes, and a state dict in the wrapper's spelling
    (``layer2.net.<b>.*``) loads the same network through tsm_set_tensor."""
    x = clip_input(36, 2, 8, 64, 64)
    eng = _engine(consensus='identity')
    want = eng.run(None, {'input': x})[0]
    got = eng.forward_device(torch.from_numpy(x).cuda())
    assert tuple(got.shape) == (2, 4, 12) and np.array_equal(got.cpu().numpy(), want)
    feats = eng.forward_features(torch.from_numpy(x).cuda())
    assert tuple(feats.shape) == (8, 2048) and np.array_equal(feats.cpu().numpy(), eng.forward_features(x))
    eng.close()
    eng = _engine(consensus='identity', sd=wrapper_keys(_sd()))
    assert np.array_equal(eng.run(None, {'input': x})[0], want)
    eng.close()


# ---- neutrality ----------------------------------------------------------------------------------------------------------------
def test_tuned_and_untuned_forwards_are_bitwise_equal(hip_lib, monkeypatch, tmp_path):
    monkeypatch.setenv('TSM_TUNE_CACHE', str(tmp_path / 'tune.txt'))
    x = clip_input(32, 2, 8, 80, 80)
    eng = _engine(size=80)
    eng.warmup([2])
    tuned = eng.run(None, {'input': x})[0]
    tiles = eng.conv_tiles(2)
    assert len(tiles) == 53 and 'layer2.tpool' not in tiles
    eng.close()
    line = (tmp_path / 'tune.txt').read_text().splitlines()
    assert len(line) == 1 and line[0].split('|')[0].endswith(' tp'), line
    monkeypatch.setenv('TSM_AUTOTUNE', '0')
    eng = _engine(size=80)
    plain = eng.run(None, {'input': x})[0]
    eng.close()
    assert np.array_equal(tuned, plain)


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3'])
def test_poisoned_engine_gives_the_same_bits(hip_lib, monkeypatch, dtype):
    """TSM_POISON=1: every buffer between poisoned bands, the workspace poisoned before every forward -- the pool relies on
    nothing it did not read from layer1's output and stores nothing outside the pooled tensor."""
    x = clip_input(33, 2, 8, 80, 80)
    eng = _engine(size=80, dtype=dtype)
    want = eng.run(None, {'input': x})[0]
    want_pool = eng.forward_tap(x, 'layer2.tpool')
    eng.close()
    monkeypatch.setenv('TSM_POISON', '1')
    eng = _engine(size=80, dtype=dtype)
    assert np.array_equal(eng.run(None, {'input': x})[0], want)
    assert np.array_equal(eng.run(None, {'input': x[:1]})[0], want[:1])
    assert np.array_equal(eng.forward_tap(x, 'layer2.tpool'), want_pool)
    eng.close()


@pytest.mark.parametrize('hw, T', [((80, 48), 4), ((90, 70), 6)], ids=_frame_id)
def test_poisoned_engine_gives_the_same_bits_on_a_non_square_frame(hip_lib, monkeypatch, hw, T):
    """A per-frame buffer sized with the wrong side, or for T frames where T / 2 are left, breaks a band or reads poison."""
    x = clip_input(33 + hw[0], 2, T, *hw)
    eng = _engine(T=T, size=hw)
    want = eng.run(None, {'input': x})[0]
    want_pool = eng.forward_tap(x, 'layer2.tpool')
    eng.close()
    assert want_pool.shape == (T, *G.maps_of('temporal_pool', *hw)['layer1'], 256)
    monkeypatch.setenv('TSM_POISON', '1')
    eng = _engine(T=T, size=hw)
    assert np.array_equal(eng.run(None, {'input': x})[0], want)
    assert np.array_equal(eng.run(None, {'input': x[:1]})[0], want[:1])
    assert np.array_equal(eng.forward_tap(x, 'layer2.tpool'), want_pool)
    eng.close()


# ---- launches ------------------------------------------------------------------------------------------------------------------
def test_launch_trace_and_timing_slot(hip_lib):
    from workoutdetector_amd.engine import launch_trace
    x = clip_input(34, 2, 8, 64, 64)
    eng = _engine()
    eng.run(None, {'input': x})
    with launch_trace() as tr:
        eng.run(None, {'input': x})
    assert tr.count(POOL_KERNEL) == 1, tr.kernels
    assert tr.count(POOL_KERNEL + '<kPrecF32>') == 1, tr.kernels
    names = eng.launch_names()
    assert names.count('layer2.tpool') == 1 and names.index('layer2.tpool') == names.index('layer1.2.conv3') + 1
    eng.set_layer_timing(1)
    eng.run(None, {'input': x})
    times = eng.layer_times_ms(0)
    assert times['layer2.tpool'] > 0 and times['head'] > 0, times
    eng.close()
    plain = _engine(temporal_pool=False)
    plain.run(None, {'input': x})
    with launch_trace() as tr0:
        plain.run(None, {'input': x})
    assert tr0.count(POOL_KERNEL) == 0, tr0.kernels
    assert 'layer2.tpool' not in plain.launch_names() and plain.out_segments == 8
    with pytest.raises(Exception, match='unknown stage'):
        plain.forward_tap(x, 'layer2.tpool')
    plain.close()


def test_set_temporal_pool_contract(hip_lib):
    """The C ABI's setter: refused after the first tensor, with a value other than 0 / 1, on a bf16 engine, without the shift, with
    an odd segment count, and together with tsm_set_non_local in either order -- each with its message and nothing launched."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import launch_trace
    lib = hip_lib

    def engine(dtype=_lib.DTYPE_F32, T=8, is_shift=1):
        cfg = _lib.TsmConfig(C.sizeof(_lib.TsmConfig), 12, T, 64, 64, 8, is_shift, 1, 0, dtype)
        h = C.c_void_p()
        _lib.check(lib.tsm_create(C.byref(cfg), C.byref(h)))
        return h

    def refused(h, code, word, on=1):
        assert lib.tsm_set_temporal_pool(h, on) == code
        msg = (lib.tsm_last_error(h) or b'').decode()
        assert word in msg, msg

    with launch_trace() as tr:
        h = engine(_lib.DTYPE_BF16)
        refused(h, -7, 'TSM_DTYPE_F32 and TSM_DTYPE_BF16X3 only')
        assert lib.tsm_set_temporal_pool(h, 0) == 0
        lib.tsm_destroy(h)
        h = engine(_lib.DTYPE_BF16X3)
        assert lib.tsm_set_temporal_pool(h, 1) == 0 and lib.tsm_set_temporal_pool(h, 0) == 0
        lib.tsm_destroy(h)
        h = engine(is_shift=0)
        refused(h, -7, 'is_shift')
        lib.tsm_destroy(h)
        for T in (1, 3, 7):
            h = engine(T=T)
            refused(h, -7, 'even num_segments')
            lib.tsm_destroy(h)
        h = engine()
        refused(h, -7, 'must be 0 or 1', on=2)
        refused(h, -7, 'must be 0 or 1', on=-1)
        assert lib.tsm_set_non_local(h, 1) == 0                 # non-local first
        refused(h, -7, 'exclude each other')
        assert lib.tsm_set_non_local(h, 0) == 0 and lib.tsm_set_temporal_pool(h, 1) == 0
        assert lib.tsm_set_non_local(h, 1) == -7                # the pool first
        assert 'exclude each other' in lib.tsm_last_error(h).decode()
        assert lib.tsm_set_backbone(h, 18) == 0 and lib.tsm_set_shift_place(h, 1) == 0 and lib.tsm_set_consensus(h, 1) == 0
        lib.tsm_destroy(h)
        h = engine()
        assert lib.tsm_set_temporal_pool(h, 1) == 0
        arr = np.ones(128 * 256, np.float32)
        shape = (C.c_int64 * 4)(128, 256, 1, 1)
        assert lib.tsm_set_tensor(h, b'base_model.layer2.net.0.conv1.net.weight', arr.ctypes.data, shape, 4) == 0
        assert lib.tsm_set_tensor(h, b'base_model.layer3.net.0.conv1.net.weight', arr.ctypes.data, shape, 4) == -1      # layer2 only
        refused(h, -1, 'tsm_set_temporal_pool must come before the first tsm_set_tensor', on=0)
        refused(h, -1, 'tsm_set_temporal_pool must come before the first tsm_set_tensor')
        lib.tsm_destroy(h)
        h = engine()                                             # a plain engine does not know the wrapper's spelling
        assert lib.tsm_set_tensor(h, b'base_model.layer2.net.0.conv1.net.weight', arr.ctypes.data, shape, 4) == -1
        lib.tsm_destroy(h)
    assert not tr.kernels, tr.kernels


# ---- one pipeline check -----------------------------------------------------------------------------------------------------------
def test_inference_video_returns_the_float64_classes(hip_lib):
    """inference_video over a temporal-pool engine: an 'avg' engine's output shape is what it was, so the reference-style clip
    path needs no change; four clips, the float64 model's class for each."""
    from workoutdetector_amd import inference_count as ic
    rng = np.random.default_rng(41)
    frames = torch.from_numpy(rng.integers(0, 256, (4, 8, 64, 64, 3), dtype=np.uint8)).float()

    def transform(v):                                         # [8, 3, H, W] in 0 .. 255 -> roughly unit normal
        return (v / 255.0 - 0.5) / 0.29
    eng = _engine(max_clips=1)
    net = torch_tsm_tp(sd=_sd())
    for c in range(4):
        scores = ic.inference_video(eng, frames[c], transform=transform)
        assert [i for i, _ in scores] == list(range(12))
        x = transform(frames[c].permute(0, 3, 1, 2)).unsqueeze(0)
        want = run_with_taps(net, x.numpy(), ())[0][0]
        assert_close(np.float32([v for _, v in scores]), want, rtol=1e-3, atol_scale=1e-5, what=f'clip {c}')
        assert int(np.argmax([v for _, v in scores])) == int(np.argmax(want)), c
    eng.close()
