"""Every enqueue-only entry point of include/tsm_hip.h held to its stream: captured on a side stream and replayed
(tests/_capture.py; the table of entry points: tests/_stream_cases.py).

On the null stream -- where every other test runs -- a launch handed the wrong stream, a lazy allocation or a
synchronisation behind ``tsm_tune`` all pass.  Inside a capture they are an error or a launch missing from the replay, and
the replay's bits then differ from the eager run's: every comparison of a replay is bitwise against an eager run of the same
build on the same inputs.  Each engine's eager result is also anchored to the float64 torch module of tests/_torch_tsm.py
(the bf16 engines: to the bf16-storage oracle, as every bf16 engine test is) at the bar of the existing engine tests:
rtol 1e-3 + 1e-5 of the scale for f32 / bf16x3, ``bf16_logits_report`` for bf16.

Geometries are the smallest at which the forced-switch tests of the other files run the kernels named here; the trace of
the CAPTURE is what each case asserts its kernels from, so a forced form that fell back fails its case.
"""
import functools

import numpy as np
import pytest
import torch

from tests import _features as ft
from tests import _image_path as ip
from tests import _person_crop as pc
from tests._capture import captured
from tests._guard import POISON, check, guarded, guarded_out
from tests._util import assert_close, assert_ran, assert_ran_tile, bf16_logits_report, make_input

pytestmark = pytest.mark.gpu

KNOBS = ('TSM_AUTOTUNE', 'TSM_WALK', 'TSM_CONV_TILE', 'TSM_CONV_CODE', 'TSM_POISON', 'TSM_POS_MAJOR', 'TSM_FUSE_CONV23',
         'TSM_FUSE_BLOCK', 'TSM_FUSE_C3C1', 'TSM_FUSE_FRONT', 'TSM_STEM_DIRECT')
F32_BAR = dict(rtol=1e-3, atol_scale=1e-5)        # tests/test_engine_gpu.py, tests/test_bf16x3_gpu.py
POS_ARM = 'kPrecF32 | kPrecPosMajor, false, true>'      # tests/test_conv_pos_major_gpu.py


@pytest.fixture
def env(hip_lib, monkeypatch):
    """No tuning knob inherited, no tune cache file; a case sets what it forces.  TSM_POISON stays unset and layer timing
    off: the header excludes both from a capture."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('TSM_TUNE_CACHE', 'off')

    def set_env(**kw):
        for k, v in kw.items():
            monkeypatch.setenv(k, str(v))
    return set_env


# ---- shared weights, inputs and anchors (computed once, never written) -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sd(seed=0, base_model='resnet50', place='blockres', non_local=False):
    from workoutdetector_amd.weights import make_state_dict
    return make_state_dict(seed, 12, base_model, place, non_local)


@functools.lru_cache(maxsize=None)
def _inputs(seed, b, t, h, w):
    """Input sets A, B, C of one geometry: CPU float32 [b, t, 3, h, w]."""
    return tuple(torch.from_numpy(make_input(seed + k, b, t, h, w)) for k in range(3))


@functools.lru_cache(maxsize=None)
def _module(base_model, place, non_local, sd_seed, t, dtype):
    from tests._nonlocal import torch_tsm_nl
    from tests._torch_tsm import TorchTSM
    sd = _sd(sd_seed, base_model, place, non_local)
    if non_local:
        return torch_tsm_nl(base_model, place, 12, t, True, sd=sd, dtype=dtype)
    return TorchTSM(base_model, 64, place, 12, t).load_engine_state_dict(sd).to(dtype).eval()


@functools.lru_cache(maxsize=None)
def _anchor(kind, base_model, place, non_local, sd_seed, in_seed, b, t, h, w, dtype=torch.float64):
    """The CPU torch module's result for input set A: 'avg' logits [b, 12], 'identity' [b, t, 12], 'pooled' [b * t, feat]."""
    net = _module(base_model, place, non_local, sd_seed, t, dtype)
    x = _inputs(in_seed, b, t, h, w)[0].to(dtype)
    with torch.no_grad():
        if kind == 'avg':
            return net(x).numpy()
        pooled = net.base_model(x.view(-1, 3, h, w))
        return pooled.numpy() if kind == 'pooled' else net.new_fc(pooled).view(b, t, -1).numpy()


@functools.lru_cache(maxsize=None)
def _anchor_bf16(base_model, sd_seed, in_seed, b, t, h, w):
    """The bf16-storage oracle's logits for input set A (what every bf16 engine test asserts against)."""
    from oracle import tsm_oracle
    from workoutdetector_amd.weights import to_torch
    x = _inputs(in_seed, b, t, h, w)[0]
    return tsm_oracle.forward(to_torch(_sd(sd_seed, base_model)), x, base_model, bf16=True, n_segment=t).numpy()


def _engine(b, t, h, w, dtype='f32', base_model='resnet50', place='blockres', consensus='avg', non_local=False, sd_seed=0):
    from workoutdetector_amd.engine import TsmEngine
    return TsmEngine(num_class=12, num_segments=t, height=h, width=w, max_clips=b, state_dict=_sd(sd_seed, base_model, place, non_local),
                     dtype=dtype, base_model=base_model, shift_place=place, consensus_type=consensus, non_local=non_local)


def _capture_forward(eng, b, in_seed, refs_after=False, warm=True):
    """warmup (the documented recipe), then ``forward_device(x, out=...)`` through tests/_capture.py -> (trace, ref_A)."""
    t, h, w = eng.num_segments, eng.height, eng.width
    sets = _inputs(in_seed, b, t, h, w)
    x = guarded(torch.zeros(b, t, 3, h, w).cuda(), name='clips')
    out = guarded_out(eng._out_shape(b), name='logits')
    if warm:
        eng.warmup([b])
    tr = captured(lambda: eng.forward_device(x, out=out), [x], lambda k: [sets[k]], [out], engine=eng, refs_after=refs_after)
    return tr, tr.refs['A'][0].cpu().numpy()


def _anchored(got, eng, b, in_seed, capsys=None, sd_seed=0, module_dtype=torch.float64):
    t, h, w = eng.num_segments, eng.height, eng.width
    kind = 'identity' if eng.consensus_type == 'identity' else 'avg'
    want = _anchor(kind, eng.base_model, eng.shift_place, eng.non_local, sd_seed, in_seed, b, t, h, w, module_dtype)
    what = f'{eng.base_model} {eng.dtype} {eng.shift_place} {kind} {b}x{t}x{h}x{w}'
    if eng.dtype == 'bf16':
        bf16_logits_report(got, _anchor_bf16(eng.base_model, sd_seed, in_seed, b, t, h, w), want, what, capsys)
    else:
        assert_close(got, want, what=what, **F32_BAR)


# ---- engines --------------------------------------------------------------------------------------------------------------
F32_SMALL = (2, 8, 96, 96)       # 2 clips of 8 x 96 x 96: tests/test_engine_gpu.py's forced split-K / tuner geometry
F32_SEED = 4100


def test_f32_engine_tuned_in_the_process(env):
    """The documented recipe: autotune on, no cache file, ``warmup([2])``, then the capture."""
    b, t, h, w = F32_SMALL
    eng = _engine(b, t, h, w)
    try:
        tr, ref_a = _capture_forward(eng, b, F32_SEED)
        assert_ran(tr, 'conv_igemm<', 'tuned f32 engine')
        assert_ran(tr, 'head_fc_kernel', 'tuned f32 engine')
        _anchored(ref_a, eng, b, F32_SEED)
    finally:
        eng.close()


def test_f32_engine_tuned_from_a_file(env, tmp_path):
    """Engine 1 writes the tune cache, engine 2 reads it: its ``warmup`` times nothing and runs one forward only to load the
    code objects, and its FIRST device forward is the captured one (the eager references are taken after the replays)."""
    b, t, h, w = F32_SMALL
    path = tmp_path / 'tune.txt'
    env(TSM_TUNE_CACHE=path)
    first = _engine(b, t, h, w)
    try:
        first.warmup([b])
        tiles = first.conv_tiles(b)
    finally:
        first.close()
    assert len(path.read_text().splitlines()) == 1
    eng = _engine(b, t, h, w)
    try:
        eng.warmup([b])
        assert len(path.read_text().splitlines()) == 1 and eng.conv_tiles(b) == tiles      # (read, not timed again)
        tr, ref_a = _capture_forward(eng, b, F32_SEED, refs_after=True, warm=False)
        assert_ran(tr, 'conv_igemm<', 'file-tuned f32 engine')
        _anchored(ref_a, eng, b, F32_SEED)
    finally:
        eng.close()


def _tail_split_clips(n_cu, t=8, rows_per_frame=9, limit=64):
    """The fewest clips of t x 96 x 96 (layer4: 3 x 3 rows per frame) at which the tail split applies to layer4.0's conv3 +
    downsample GEMM (cout 2048, K = 512 + 1024 in three or more segments): one whole round of 5 n_cu workgroups and a tail."""
    from tests._walk_cases import tail_split_applies
    for b in range(1, limit + 1):
        if tail_split_applies(b * t * rows_per_frame, 2048, 3, n_cu):
            return b
    return None


@pytest.mark.parametrize('form', ['split_k', 'position_major', 'fused_conv23', 'tail_split'])
def test_f32_engine_forced_forms(env, form):
    """Four forms forced with TSM_AUTOTUNE=0: split-K (d_partial written and reduced inside the graph), the position-major
    3x3 at 8 clips x 8 segments (whole 64-frame batches), the fused conv2 + conv3, and the tail split with its ordered
    reduction at the fewest 96 x 96 clips that fill one round of workgroups on this chip (36 on 256 CUs)."""
    b, t, h, w = (8, 8, 96, 96) if form == 'position_major' else F32_SMALL
    seed = {'position_major': 4200, 'tail_split': 4250}.get(form, F32_SEED)
    env(TSM_AUTOTUNE=0)
    if form == 'split_k':
        env(TSM_CONV_CODE=0x103)
    elif form == 'position_major':
        env(TSM_CONV_CODE=0x83, TSM_FUSE_CONV23=0)
    elif form == 'tail_split':
        b = _tail_split_clips(torch.cuda.get_device_properties(0).multi_processor_count)
        assert b is not None, 'no clip count up to 64 takes the tail split on this chip'
        env(TSM_CONV_CODE=0x203, TSM_FUSE_CONV23=0)
    else:
        env(TSM_FUSE_CONV23=1)
    eng = _engine(b, t, h, w)
    try:
        tr, ref_a = _capture_forward(eng, b, seed)
        if form == 'split_k':
            assert_ran(tr, 'splitk_reduce_kernel', form)
            assert any(k.startswith('conv_igemm<') and 'true>' in k.split('[')[0] and '[BM = 64, BN = 64,' in k for k in tr.kernels), tr.kernels
        elif form == 'position_major':
            assert any(k.startswith('conv_igemm<') and POS_ARM in k for k in tr.kernels), sorted(set(tr.kernels))
        elif form == 'tail_split':       # (the code carries no split-K bit: a reduction here is the tail's)
            assert_ran(tr, 'splitk_reduce_kernel', form)
        else:
            assert tr.ran('conv23_fused_kernel<64,') and tr.ran('conv23_fused_kernel<128,'), sorted(set(tr.kernels))
        # (64 frames and more: the anchor module runs in float32 there, as the oracle of the existing engine tests does)
        _anchored(ref_a, eng, b, seed, module_dtype=torch.float32 if b > 2 else torch.float64)
    finally:
        eng.close()


BF16_FUSED = (5, 4, 64, 96)      # 5 clips of 4 x 64 x 96: the geometry all three forced bf16 switches of test_bf16_gpu.py share
BF16_SEED = 4300


def test_bf16_engine_fused_forms(env, capsys):
    """TSM_FUSE_BLOCK, TSM_FUSE_C3C1 and TSM_FUSE_FRONT forced on one engine: the whole-block kernel, the cross-block conv3 +
    conv1 kernels and layer2.0's front all inside one graph."""
    b, t, h, w = BF16_FUSED
    env(TSM_FUSE_BLOCK=1, TSM_FUSE_C3C1=1, TSM_FUSE_FRONT=1)
    eng = _engine(b, t, h, w, 'bf16')
    try:
        tr, ref_a = _capture_forward(eng, b, BF16_SEED)
        assert_ran(tr, 'bneck_ws_kernel<', 'bf16 fused')
        assert tr.ran('conv31_fused_kernel<') or tr.ran('conv31_pc_kernel<'), sorted(set(tr.kernels))
        assert_ran(tr, 'front_s2_kernel<', 'bf16 fused')
        _anchored(ref_a, eng, b, BF16_SEED, capsys)
    finally:
        eng.close()


# Input seeds of the bf16 cases are chosen ON THE CPU, with the references alone, so that the bf16-storage oracle's top-2 margin
# of every clip of set A exceeds twice BF16_E2E_BAR of the logit scale (bf16_logits_report asserts the arg-max): 6 % of the
# scale at 4300 for the first two geometries and at 4310 for the third (4300 gives 0.4 % there), 41 % for resnet18 at 4500.
@pytest.mark.parametrize('tile,b,t,h,w,seed', [('ws', 3, 8, 90, 70, BF16_SEED), ('256x256p', 3, 2, 64, 64, 4310)])
def test_bf16_engine_forced_tiles(env, capsys, tile, b, t, h, w, seed):
    """The weight-stationary families (smallest geometry of the forced-everywhere test) and the persistent 256x256 kernel."""
    env(TSM_AUTOTUNE=0, TSM_CONV_TILE=tile, TSM_FUSE_CONV23=0)
    eng = _engine(b, t, h, w, 'bf16')
    try:
        tr, ref_a = _capture_forward(eng, b, seed)
        if tile == 'ws':
            assert_ran(tr, 'conv3x3_ws', 'bf16 ws')
            assert_ran(tr, 'conv1x1_ws', 'bf16 ws')
        else:
            assert_ran_tile(tr, tile, 'bf16 256x256p')
        _anchored(ref_a, eng, b, seed, capsys)
    finally:
        eng.close()


def test_bf16x3_engine(env):
    """The default schedule (tuned) at the smallest golden shape of test_bf16x3_gpu.py: 5 clips of 4 x 32 x 32."""
    b, t, h, w = 5, 4, 32, 32
    eng = _engine(b, t, h, w, 'bf16x3')
    try:
        tr, ref_a = _capture_forward(eng, b, 4400)
        assert any('kPrecBf16x3' in k for k in tr.kernels), sorted(set(tr.kernels))
        _anchored(ref_a, eng, b, 4400)
    finally:
        eng.close()


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_resnet18_engine(env, capsys, dtype):
    """The BasicBlock path: the temporal shift inside the 3x3 loader."""
    b, t, h, w = 2, 8, 64, 64
    eng = _engine(b, t, h, w, dtype, base_model='resnet18')
    try:
        tr, ref_a = _capture_forward(eng, b, 4500)
        assert any(k.startswith('conv_igemm<') and 'KS = 3, SHIFT = true' in k for k in tr.kernels), sorted(set(tr.kernels))
        _anchored(ref_a, eng, b, 4500, capsys)
    finally:
        eng.close()


def test_block_placement_engine(env):
    b, t, h, w = 2, 8, 64, 64
    eng = _engine(b, t, h, w, place='block')
    try:
        tr, ref_a = _capture_forward(eng, b, 4600)
        assert any('kPrecBlockShift' in k for k in tr.kernels), sorted(set(tr.kernels))      # (tests/test_block_place_gpu.py)
        _anchored(ref_a, eng, b, 4600)
    finally:
        eng.close()


def test_identity_consensus_engine(env):
    b, t, h, w = 2, 8, 64, 64
    eng = _engine(b, t, h, w, consensus='identity')
    try:
        tr, ref_a = _capture_forward(eng, b, 4700)
        assert_ran(tr, 'head_seg_kernel', 'identity consensus')
        assert ref_a.shape == (b, t, 12)
        _anchored(ref_a, eng, b, 4700)
    finally:
        eng.close()


def test_forward_features(env):
    """``forward_features`` with ``normalize`` False and True as ONE graph of two forwards: the pooled rows against the module
    at the engine bar, the unit rows against the pooled rows over their norm at test_features_gpu.py's 1e-5."""
    b, t, h, w = 2, 8, 64, 64
    eng = _engine(b, t, h, w)
    try:
        sets = _inputs(4800, b, t, h, w)
        x = guarded(torch.zeros(b, t, 3, h, w).cuda(), name='clips')
        pooled = guarded_out((b * t, eng.feature_dim), name='pooled')
        unit = guarded_out((b * t, eng.feature_dim), name='unit')
        eng.warmup([b])

        def run():
            eng.forward_features(x, normalize=False, out=pooled)
            eng.forward_features(x, normalize=True, out=unit)
        tr = captured(run, [x], lambda k: [sets[k]], [pooled, unit], engine=eng)
        assert tr.count('pool_feat_kernel') == 2, tr.kernels
        assert not tr.ran('head_'), tr.kernels
        got, got_unit = (r.cpu().numpy() for r in tr.refs['A'])
        assert_close(got, _anchor('pooled', 'resnet50', 'blockres', False, 0, 4800, b, t, h, w), what='pooled features', **F32_BAR)
        g64 = got.astype(np.float64)
        norms = np.sqrt((g64 * g64).sum(1, keepdims=True))
        assert np.allclose(got_unit, g64 / np.where(norms == 0, 1.0, norms), rtol=1e-5, atol=0.0)
    finally:
        eng.close()


def test_non_local_engine(env):
    """``non_local=True`` at the smallest case of test_nonlocal_gpu.py (48 x 48: layer3's keys are 1 x 1 per frame): the three
    launches per wrapped block inside the graph."""
    b, t, h, w = 2, 8, 48, 48
    eng = _engine(b, t, h, w, non_local=True)
    try:
        tr, ref_a = _capture_forward(eng, b, 4900)
        assert tr.count('maxpool2x2_kernel') == 5 and tr.count('nonlocal_attn_kernel') == 5, tr.kernels
        _anchored(ref_a, eng, b, 4900)
    finally:
        eng.close()


# ---- per-op entry points --------------------------------------------------------------------------------------------------
def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _op(run, statics, sets, outputs, kernel, **kw):
    tr = captured(run, statics, lambda k: sets[k], outputs, **kw)
    assert_ran(tr, kernel, kernel)
    return tr


def test_op_temporal_shift(env):
    from workoutdetector_amd.engine import temporal_shift_nhwc
    nb, t, c, h, w = 3, 4, 32, 2, 5
    sets = [[_randn(10 + k, nb * t, h, w, c)] for k in range(3)]
    x, y = guarded(sets[0][0].cuda(), name='x'), guarded_out((nb * t, h, w, c), name='y')
    _op(lambda: temporal_shift_nhwc(x, t, 8, out=y), [x], sets, [y], 'temporal_shift_kernel')


def test_op_maxpool3x3s2(env):
    from workoutdetector_amd.engine import maxpool3x3s2_nhwc
    n, h, w, c = 3, 15, 13, 64
    sets = [[_randn(20 + k, n, h, w, c)] for k in range(3)]
    x = guarded(sets[0][0].cuda(), fill=float('inf'), name='x')
    y = guarded_out((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), name='y')
    _op(lambda: maxpool3x3s2_nhwc(x, out=y), [x], sets, [y], 'maxpool3x3s2_kernel')


def test_op_maxpool2x2(env):
    from workoutdetector_amd.engine import maxpool2x2_nhwc
    n, h, w, cw, c0, c = 3, 5, 5, 24, 8, 12
    sets = []
    for k in range(3):
        v = torch.full((n, h, w, cw), float('inf'))
        v[..., c0:c0 + c] = _randn(30 + k, n, h, w, c)
        sets.append([v])
    x = guarded(sets[0][0].cuda(), fill=float('inf'), name='x')
    y = guarded_out((n, h // 2, w // 2, c), name='y')
    _op(lambda: maxpool2x2_nhwc(x, c0, c, out=y), [x], sets, [y], 'maxpool2x2_kernel')


def test_op_nonlocal_attention(env):
    """d = 256 with 65 queries and 65 keys: more than one tile each way."""
    from tests.test_nonlocal_gpu import _qkv
    from workoutdetector_amd.engine import nonlocal_attention
    sets = [list(_qkv(40 + k, 2, 65, 65, 256)) for k in range(3)]
    q, k_, v = (guarded(t.cuda(), name=n) for t, n in zip(sets[0], 'qkv'))
    y = guarded_out((2, 65, 256), name='y')
    _op(lambda: nonlocal_attention(q, k_, v, out=y), [q, k_, v], sets, [y], 'nonlocal_attn_kernel<256>')


def _video_sets(seed, n, h, w):
    return [[pc.video(seed + k, n, h, w)] for k in range(3)]


def test_op_preprocess(env):
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import preprocess_frames
    n, h, w, resize, crop = 3, 40, 56, 36, 32
    sets = _video_sets(50, n, h, w)
    frames = guarded(sets[0][0].cuda(), name='frames')
    out = guarded_out((n, crop, crop, 4), name='out')
    _op(lambda: preprocess_frames(frames, resize=resize, crop=crop, layout=_lib.LAYOUT_NTHWC4, out=out), [frames], sets, [out], 'preprocess_kernel')


def test_op_gather_clips(env):
    """43 source frames, every second one transformed: 6 clips, the last ones padded with the buffer's last frame."""
    from workoutdetector_amd.engine import gather_clips
    total, n_clips = 43, 6
    sets = [[_randn(60 + k, 23, 8, 8, 4)] for k in range(3)]
    frames = guarded(sets[0][0].cuda(), name='frames')
    out = guarded_out((n_clips, 8, 8, 8, 4), name='clips')
    _op(lambda: gather_clips(frames, 0, total, 0, n_clips, out=out), [frames], sets, [out], 'gather_clips_kernel')


def test_op_preprocess_clips(env):
    from workoutdetector_amd.engine import preprocess_clips
    total, n_clips, h, w, size = 43, 6, 40, 56, 32
    boxes = [(0, 0, 0, 0) if b is None else b for b in pc.boxes_for(h, w, size)]
    sets = [[pc.video(70 + k, 22, h, w), torch.tensor(boxes[2 * k:2 * k + n_clips], dtype=torch.int32)] for k in range(3)]
    frames, bx = guarded(sets[0][0].cuda(), name='frames'), guarded(sets[0][1].cuda(), name='boxes')
    out = guarded_out((n_clips, 8, size, size, 4), name='out')
    _op(lambda: preprocess_clips(frames, bx, 0, total, 0, n_clips, size=size, out=out), [frames, bx], sets, [out], 'preprocess_clips_kernel')


def test_op_preprocess_indexed(env):
    """A table with repeated frames and entries outside the buffer (the zero frame)."""
    from workoutdetector_amd.engine import preprocess_indexed
    n, h, w, resize, crop = 5, 40, 56, 36, 32
    tables = ([[0, 0, 1, 4], [3, -1, 7, 2]], [[4, 3, 2, 1], [0, 5, 2, 2]], [[1, 1, 1, 1], [-2147483648, 2147483647, 0, 4]])
    sets = [[pc.video(80 + k, n, h, w), torch.tensor(tables[k], dtype=torch.int32)] for k in range(3)]
    frames, index = guarded(sets[0][0].cuda(), name='frames'), guarded(sets[0][1].cuda(), name='index')
    out = guarded_out((2, 4, crop, crop, 4), name='out')
    _op(lambda: preprocess_indexed(frames, index, resize=resize, crop=crop, out=out), [frames, index], sets, [out], 'preprocess_indexed_kernel')


def test_op_preprocess_windows(env):
    """Two frame sizes in one arena, interleaved in batch order."""
    from tests.test_windows_gpu import _pack
    from workoutdetector_amd.engine import preprocess_windows
    from workoutdetector_amd.transform import window_descriptors
    t, size = 2, 32
    shapes = [(40, 56), (33, 47), (40, 56)]
    sets, table = [], None
    for k in range(3):
        windows = [pc.video(90 + 10 * k + i, t, h, w) for i, (h, w) in enumerate(shapes)]
        arena, offsets = _pack(windows, False)
        table = window_descriptors(shapes, offsets, resize=36, crop=size)
        sets.append([arena, torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32))])
    arena, desc = guarded(sets[0][0].cuda(), name='arena'), guarded(sets[0][1].cuda(), name='desc')
    out = guarded_out((len(shapes), t, size, size, 4), name='out')
    _op(lambda: preprocess_windows(arena, desc, len(shapes), t, resize=36, crop=size, out=out), [arena, desc], sets, [out],
        'preprocess_windows_kernel')


def test_op_preprocess_image(env):
    from workoutdetector_amd.engine import preprocess_image
    from workoutdetector_amd.transform import image_tables
    frames_a, _want, resize, crop = ip.fixture('landscape')
    a = torch.from_numpy(frames_a.copy())
    sets = [[a], [a.flip(1).contiguous()], [a.flip(2).contiguous()]]
    n, h, w, _ = a.shape
    frames = guarded(a.cuda(), name='frames')
    tables = guarded(torch.from_numpy(image_tables(h, w, resize, crop).copy()).cuda(), name='tables')
    out = guarded_out((n, crop, crop, 4), name='out')
    tr = _op(lambda: preprocess_image(frames, resize=resize, crop=crop, out=out, tables=tables), [frames], sets, [out], 'preprocess_image_kernel')
    check(tables)
    got = tr.refs['A'][0].cpu().numpy()[..., :3]        # anchored to Pillow's own pixels (tests/golden/ref_image_transform.npz)
    assert float(ip.ulps(got, ip.normalised(_want)).max()) <= 2.0


def _head_sets(seed, n, h, w, c, cls):
    return [[_randn(seed + 3 * k, n, h, w, c), _randn(seed + 3 * k + 1, cls, c) * 0.05, _randn(seed + 3 * k + 2, cls)] for k in range(3)]


def test_op_head(env):
    """``tsm_head``: two launches and the pooled rows between them, a stream-ordered allocation of the call's own."""
    from workoutdetector_amd.engine import head_nhwc
    b, t, h, w, c, cls = 3, 4, 2, 2, 512, 5
    sets = _head_sets(100, b * t, h, w, c, cls)
    feat, fw, fb = (guarded(v.cuda(), name=n) for v, n in zip(sets[0], ('feat', 'fc_w', 'fc_b')))
    out = guarded_out((b, cls), name='logits')
    tr = _op(lambda: head_nhwc(feat, fw, fb, t, out=out), [feat, fw, fb], sets, [out], 'head_pool_kernel')
    assert_ran(tr, 'head_fc_kernel', 'head')
    from oracle import tsm_oracle
    want = tsm_oracle.head(sets[0][0].permute(0, 3, 1, 2).double(), {'fc.weight': sets[0][1].double(), 'fc.bias': sets[0][2].double()}, t)
    assert_close(tr.refs['A'][0].cpu().numpy(), want.numpy(), rtol=1e-4, atol_scale=1e-5, what='head')      # (tests/test_ops_gpu.py)


def test_op_head_segments(env):
    from workoutdetector_amd.engine import head_segments_nhwc
    n, h, w, c, cls = 12, 2, 2, 512, 5
    sets = _head_sets(110, n, h, w, c, cls)
    feat, fw, fb = (guarded(v.cuda(), name=nm) for v, nm in zip(sets[0], ('feat', 'fc_w', 'fc_b')))
    out = guarded_out((n, cls), name='logits')
    _op(lambda: head_segments_nhwc(feat, fw, fb, out=out), [feat, fw, fb], sets, [out], 'head_seg_kernel')


def test_op_pool_features(env):
    from workoutdetector_amd.engine import pool_features_nhwc
    n, h, w, c = 3, 7, 1, 512
    sets = [[_randn(120 + k, n, h, w, c)] for k in range(3)]
    feat = guarded(sets[0][0].cuda(), name='feat')
    pooled, unit = guarded_out((n, c), name='pooled'), guarded_out((n, c), name='unit')
    _op(lambda: pool_features_nhwc(feat, out=pooled, out_unit=unit), [feat], sets, [pooled, unit], 'pool_feat_kernel')


def test_op_cosine_distances(env):
    """Two bands of one matrix as two launches of one graph: rows [0, 32), then [32, 40) with its mirror."""
    from workoutdetector_amd.engine import cosine_distances
    n, c = 40, 72
    sets = [[torch.from_numpy(ft.unit_rows_host(ft.feature_rows(n, c, 'relu', seed=k)))] for k in range(3)]
    unit = guarded(sets[0][0].cuda(), name='unit')
    dist = guarded_out((n, n), name='dist')

    def run():
        cosine_distances(unit, out=dist, rows=(0, 32))
        cosine_distances(unit, out=dist, rows=(32, n))
    tr = _op(run, [unit], sets, [dist], 'cosine_dist_kernel')
    assert len(tr.kernels) == 2, tr.kernels
    got = tr.refs['A'][0].cpu().numpy()
    u = sets[0][0].numpy().astype(np.float64)
    want = np.clip(1.0 - u @ u.T, 0.0, 2.0)
    np.fill_diagonal(want, 0.0)
    assert float(np.abs(got - want).max()) <= ft.DIST_BAR and np.array_equal(got, got.T)


def test_op_scores_to_states(env):
    from workoutdetector_amd.engine import scores_to_states
    n, c = 64, 12
    sets = [[torch.from_numpy(ip.logits_with_ties(130 + k, n, c) * np.float32(3.0))] for k in range(3)]
    logits = guarded(sets[0][0].cuda(), name='logits')
    states, top = guarded_out((n,), torch.int32, name='states'), guarded_out((n,), name='top')
    _op(lambda: scores_to_states(logits, threshold=0.3, return_top=True, out=states, out_top=top), [logits], sets, [states, top],
        'scores_to_states_kernel')


def test_op_frame_votes_carries_its_history_across_replays(env):
    """``hist_out`` of one replay is the next replay's ``hist_in`` (a device copy between replays): three replays over three
    batches equal the reference's deque over the concatenated frames."""
    from workoutdetector_amd.engine import frame_votes
    n, c = 9, 2
    first = [1, 0, 1, 1, 0, 1]                                   # the six frames before the first batch
    sets = [[torch.from_numpy(ip.logits_with_ties(140 + k, n, c)), torch.tensor(first[k:] + first[:k], dtype=torch.int32)]
            for k in range(3)]
    logits, hist_in = guarded(sets[0][0].cuda(), name='logits'), guarded(sets[0][1].cuda(), name='history')
    pred, state = guarded_out((n,), torch.int32, name='pred'), guarded_out((n,), torch.int32, name='state')
    hist_out = guarded_out((6,), torch.int32, name='history_out')
    tr = _op(lambda: frame_votes(logits, history=hist_in, out=(pred, state, hist_out)), [logits, hist_in], sets, [pred, state, hist_out],
             'frame_votes_kernel')
    hist_in.copy_(torch.tensor(first, dtype=torch.int32))
    preds, states = [], []
    for k in range(3):
        logits.copy_(sets[k][0])
        for o in (pred, state, hist_out):
            o.view(torch.int32).fill_(POISON)
        tr.graph.replay()
        torch.cuda.synchronize()
        check(pred, state, hist_out, logits, hist_in)
        preds += pred.cpu().tolist()
        states += state.cpu().tolist()
        hist_in.copy_(hist_out)                                   # the device copy between replays
    want_pred = np.concatenate([s[0].numpy().argmax(1) for s in sets]).tolist()
    assert preds == want_pred
    assert states == ip.reference_vote(first + want_pred)[6:]
    assert hist_in.cpu().tolist() == want_pred[-6:]


def test_op_top1_tally_accumulates_across_replays(env):
    """The counters accumulate: after k replays they equal those of k eager calls (and NumPy's count)."""
    from workoutdetector_amd.engine import top1_tally
    n, c = 37, 5
    rng = np.random.default_rng(150)
    sets = [[torch.from_numpy(ip.logits_with_ties(150 + k, n, c)), torch.from_numpy(rng.integers(-1, c + 1, n).astype(np.int32)),
             torch.from_numpy(rng.integers(0, 50, c).astype(np.int32)), torch.from_numpy(rng.integers(50, 99, c).astype(np.int32))]
            for k in range(3)]
    logits, labels, correct, total = (guarded(v.cuda(), name=nm) for v, nm in zip(sets[0], ('logits', 'labels', 'correct', 'total')))
    pred = guarded_out((n,), torch.int32, name='pred')
    tr = _op(lambda: top1_tally(logits, labels, correct, total, out=pred), [logits, labels, correct, total], sets, [pred], 'top1_tally_kernel',
             inout=[correct, total])

    def counters(step):
        logits.copy_(sets[1][0])
        labels.copy_(sets[1][1])
        correct.zero_()
        total.zero_()
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        check(pred, logits, labels, correct, total)
        return correct.cpu().numpy().copy(), total.cpu().numpy().copy()
    replayed = counters(tr.graph.replay)
    eager = counters(lambda: top1_tally(logits, labels, correct, total, out=pred))
    lab, arg = sets[1][1].numpy(), sets[1][0].numpy().argmax(1)
    valid = (lab >= 0) & (lab < c)
    want_total = 3 * np.bincount(lab[valid], minlength=c)
    want_correct = 3 * np.bincount(lab[valid & (arg == lab)], minlength=c)
    for got in (replayed, eager):
        assert np.array_equal(got[0], want_correct) and np.array_equal(got[1], want_total), (got, want_correct, want_total)


# ---- one serving step as one graph -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'bf16x3'])
def test_one_serving_step_as_one_graph(env, dtype):
    """uint8 frames -> tsm_preprocess -> tsm_gather_clips -> forward_device -> tsm_scores_to_states, the pipeline
    tests/abi_c_smoke.c drives (43 frames of 70 x 90, six clips, the last ones zero-padded), captured once and replayed with
    new frames: packed frames, clips, logits, states and top scores equal the eager pipeline's, in each engine's own packed
    layout."""
    from workoutdetector_amd import engine
    from workoutdetector_amd.weights import make_state_dict
    frames_n, h, w, resize, crop, n_clips = 43, 70, 90, 72, 64, 6
    sd = dict(make_state_dict(3, 12))
    sd['fc.weight'] = sd['fc.weight'] * np.float32(40.0)          # spread the softmax so that states are not all -1
    eng = engine.TsmEngine(num_class=12, num_segments=8, height=crop, width=crop, max_clips=n_clips, state_dict=sd, dtype=dtype)
    try:
        layout = eng.packed_layout
        sets = [[torch.cat([pc.video(160 + k, frames_n, h, w)[0::2], torch.zeros((1, h, w, 3), dtype=torch.uint8)])] for k in range(3)]
        even = guarded(sets[0][0].cuda(), name='frames')
        shape = engine._frame_shape(layout, crop)
        packed = guarded_out((even.shape[0],) + shape, name='packed')
        clips = guarded_out((n_clips, 8) + shape, name='clips')
        logits = guarded_out((n_clips, 12), name='logits')
        states, top = guarded_out((n_clips,), torch.int32, name='states'), guarded_out((n_clips,), name='top')
        eng.warmup([n_clips])

        def run():
            engine.preprocess_frames(even, resize=resize, crop=crop, layout=layout, out=packed)
            engine.gather_clips(packed, 0, frames_n, 0, n_clips, out=clips)
            eng.forward_device(clips, out=logits, layout=layout)
            engine.scores_to_states(logits, threshold=0.1, return_top=True, out=states, out_top=top)
        tr = captured(run, [even], lambda k: sets[k], [packed, clips, logits, states, top], engine=eng)
        for kernel in ('preprocess_kernel', 'gather_clips_kernel', 'scores_to_states_kernel'):
            assert_ran(tr, kernel, 'serving step')
        got = tr.refs['A'][3].cpu().numpy()
        assert (got >= 0).any() and ((got >= -1) & (got < 12)).all(), got
    finally:
        eng.close()
