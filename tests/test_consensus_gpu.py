"""consensus_type='identity' on the GPU: head_seg_kernel in hostile memory, whole engines of every backbone, placement and
dtype against the per-segment reference (tests/_consensus.py), identity against avg from one state dict, what ran, the
engine under TSM_POISON=1, and the way the output is used (scores_to_states over B*T rows).

Arg-max rule: equality is asserted only on (clip, segment) rows whose REFERENCE top-2 margin exceeds twice the bar times the
logit scale; at most one row in eight may be undecided, asserted per case (the seeds are picked on the CPU so that the
reference alone meets that: tests/test_consensus_cpu.py::test_argmax_cap_holds_for_the_reference_alone)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _consensus as cs
from tests._guard import POISON, check, guarded, guarded_out
from tests._util import BF16_E2E_BAR, assert_close, assert_not_ran, assert_ran, make_input

pytestmark = pytest.mark.gpu

KNOBS = ('TSM_AUTOTUNE', 'TSM_WALK', 'TSM_CONV_TILE', 'TSM_CONV_CODE', 'TSM_POISON')


# ---- per-op, hostile memory ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_frames', [1, 8, 24])
@pytest.mark.parametrize('num_class', [1, 2, 12, 13])
@pytest.mark.parametrize('hw', [1, 4, 49, 64])
@pytest.mark.parametrize('c', [512, 2048])
def test_head_segments_in_hostile_memory(hip_lib, c, hw, num_class, n_frames):
    """Operands between poison bands, the output pre-poisoned: every output written, nothing else; values at the bar
    test_ops_gpu.py::_head_case holds tsm_head to (same weight scale); and the segment mean of the result against tsm_head."""
    from workoutdetector_amd.engine import head_nhwc, head_segments_nhwc, launch_trace
    g = torch.Generator().manual_seed(c + 100 * hw + 10 * num_class + n_frames)
    feat = torch.randn(n_frames, hw, 1, c, generator=g)              # NHWC [n, h = hw, w = 1, c]
    w, b = torch.randn(num_class, c, generator=g) * 0.05, torch.randn(num_class, generator=g)
    want = F.linear(feat.reshape(n_frames, hw, c).mean(1), w, b)
    ops = [guarded(feat.cuda(), name='feat'), guarded(w.cuda(), name='fc_w'), guarded(b.cuda(), name='fc_b')]
    out = guarded_out((n_frames, num_class), name='logits')
    with launch_trace() as tr:
        assert head_segments_nhwc(*ops, out=out) is out
    torch.cuda.synchronize()
    check(out, *ops)
    assert tr.kernels == ['head_seg_kernel<kPrecF32>'], tr.kernels
    what = f'head_seg c{c} hw{hw} cls{num_class} n{n_frames}'
    assert_close(out.cpu().numpy(), want.numpy(), rtol=1e-4, atol_scale=1e-5, what=what)
    t = 8 if n_frames % 8 == 0 else 1
    avg = head_nhwc(*ops, t)
    assert_close(out.view(n_frames // t, t, num_class).mean(1).cpu().numpy(), avg.cpu().numpy(), rtol=1e-4, atol_scale=1e-5,
                 what=what + ' segment mean vs tsm_head')


@pytest.mark.parametrize('hw', [1, 7, 49, 64])
@pytest.mark.parametrize('c', [512, 2048])
def test_pooled_value_is_the_avg_heads_to_the_bit(hip_lib, c, hw):
    """The contract: a frame's pooled value is computed exactly as head_pool_kernel computes it.  With num_class = c, an
    identity classifier and a zero bias both heads return their pooled vector unchanged (every other product is an exact
    zero; tsm_head at T = 1 takes the mean of one frame), so the two outputs must be equal bit for bit."""
    from workoutdetector_amd.engine import head_nhwc, head_segments_nhwc
    g = torch.Generator().manual_seed(7 * c + hw)
    feat = (torch.randn(8, hw, 1, c, generator=g) * 3.0).cuda()
    eye, zero = torch.eye(c).cuda(), torch.zeros(c).cuda()
    seg = head_segments_nhwc(feat, eye, zero)
    avg = head_nhwc(feat, eye, zero, 1)
    assert tuple(seg.shape) == tuple(avg.shape) == (8, c)
    assert torch.equal(seg, avg), f'c{c} hw{hw}: {int((seg != avg).sum())} pooled values differ from head_pool_kernel\'s'
    assert_close(seg.cpu().numpy(), feat.reshape(8, hw, c).mean(1).cpu().numpy(), rtol=1e-5, atol_scale=1e-6, what='pooled')


def test_head_segments_refuses_what_it_cannot_run(hip_lib):
    from workoutdetector_amd._lib import TsmError
    from workoutdetector_amd.engine import head_segments_nhwc
    feat = torch.zeros(2, 1, 1, 4096).cuda()
    with pytest.raises(TsmError, match='TSM_ERR_UNSUPPORTED'):      # wider than the kernel's LDS row
        head_segments_nhwc(feat, torch.zeros(3, 4096).cuda(), torch.zeros(3).cuda())
    with pytest.raises(ValueError):
        head_segments_nhwc(feat, torch.zeros(3, 2048).cuda(), torch.zeros(3).cuda())
    with pytest.raises(ValueError):
        head_segments_nhwc(feat.cpu(), torch.zeros(3, 4096).cuda(), torch.zeros(3).cuda())
    with pytest.raises(ValueError):
        head_segments_nhwc(feat, torch.zeros(3, 4096).cuda(), torch.zeros(3).cuda(), out=torch.zeros(2, 4).cuda())


# ---- whole engines ----------------------------------------------------------------------------------------------------------
_REF = {}


def _reference(base_model, place, bf16):
    key = (base_model, place, bf16)
    if key not in _REF:
        _, sdt = cs.state_dict(base_model, place)
        _REF[key] = cs.per_segment_reference(sdt, cs.case_input(base_model, place), base_model, place, bf16).numpy()
    return _REF[key]


def _engine(base_model, place, dtype, consensus='identity', max_clips=2, sd=None):
    from workoutdetector_amd.engine import TsmEngine
    sd = sd if sd is not None else cs.state_dict(base_model, place)[0]
    return TsmEngine(num_class=cs.NUM_CLASS, num_segments=cs.T, height=cs.H, width=cs.W, max_clips=max_clips, state_dict=sd,
                     dtype=dtype, base_model=base_model, shift_place=place, consensus_type=consensus)


def _against_reference(got, base_model, place, dtype, what, capsys=None):
    want = _reference(base_model, place, False)
    assert got.shape == (cs.B, cs.T, cs.NUM_CLASS) == want.shape
    if dtype == 'bf16':
        want16 = _reference(base_model, place, True)
        scale = float(np.abs(want).max())
        e16, e32 = float(np.abs(got - want16).max()) / scale, float(np.abs(got - want).max()) / scale
        msg = (f'[{what}] per-segment logits max|err|/scale: {e16:.3g} vs the bf16-storage reference (bar {BF16_E2E_BAR:g}), '
               f'{e32:.3g} vs the fp32 reference')
        if capsys is not None:
            with capsys.disabled():
                print('\n' + msg)
        assert np.isfinite(got).all() and e16 <= BF16_E2E_BAR, msg
        cs.assert_argmax(got, want16, BF16_E2E_BAR, what)
    else:
        assert_close(got, want, rtol=1e-3, atol_scale=1e-5, what=what)
        cs.assert_argmax(got, want, cs.F32_BAR, what)


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('place', cs.PLACES)
@pytest.mark.parametrize('base_model', cs.BASE_MODELS)
def test_identity_engine_against_the_per_segment_reference(hip_lib, capsys, base_model, place, dtype):
    """B = 3 through max_clips = 2 (the chunk loop), host and device forward: [B, T, C], the project's logits bar, and the
    two forwards bit for bit."""
    x = cs.case_input(base_model, place)
    eng = _engine(base_model, place, dtype)
    try:
        assert eng.consensus_type == 'identity' and eng.get_outputs()[0].shape == [None, cs.T, cs.NUM_CLASS]
        host = eng.run(None, {'input': x})[0]
        dev = eng.forward_device(torch.from_numpy(x).cuda())
        assert tuple(dev.shape) == (cs.B, cs.T, cs.NUM_CLASS) and dev.is_contiguous()
        # (an engine takes ONE in-flight call: the device forward only enqueues on torch's stream, the host forward below runs on
        #  the engine's own non-blocking stream over the same workspace, so it must not start before that one has finished)
        torch.cuda.synchronize()
        called = eng(torch.from_numpy(x).reshape(cs.B * cs.T, 3, cs.H, cs.W))        # nn.Module duck type, CPU tensor
        assert tuple(called.shape) == (cs.B, cs.T, cs.NUM_CLASS)
        with pytest.raises(ValueError, match=rf'\[{cs.B}, {cs.T}, {cs.NUM_CLASS}\]'):
            eng.forward_device(torch.from_numpy(x).cuda(), out=torch.empty(cs.B, cs.NUM_CLASS, device='cuda'))
        into = torch.full((cs.B, cs.T, cs.NUM_CLASS), float('nan'), device='cuda')
        assert eng.forward_device(torch.from_numpy(x).cuda(), out=into) is into
        torch.cuda.synchronize()
    finally:
        eng.close()
    assert np.array_equal(host, dev.cpu().numpy()), 'forward_host and forward_device differ'
    assert np.array_equal(host, called.numpy()), 'the nn.Module call differs from run()'
    assert np.array_equal(host, into.cpu().numpy()), 'forward_device(out=...) differs from forward_host'
    _against_reference(host, base_model, place, dtype, f'{base_model} {place} {dtype} identity', capsys)


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('base_model', ['resnet18', 'resnet50'])
def test_identity_mean_is_the_avg_engine(hip_lib, base_model, dtype):
    """Two engines from ONE state dict on one input.  NOT bit-equal: avg sums the segments' pooled features and then takes
    one dot product, identity takes a dot product per segment and the test takes the mean -- a different summation order, held
    to the head's per-op bar."""
    sd = cs.state_dict(base_model, 'blockres')[0]
    x = cs.case_input(base_model, 'blockres')
    out = {}
    for consensus in ('avg', 'identity'):
        eng = _engine(base_model, 'blockres', dtype, consensus, sd=sd)
        try:
            out[consensus] = eng.run(None, {'input': x})[0]
        finally:
            eng.close()
    assert out['avg'].shape == (cs.B, cs.NUM_CLASS) and out['identity'].shape == (cs.B, cs.T, cs.NUM_CLASS)
    assert_close(out['identity'].astype(np.float64).mean(1), out['avg'], rtol=1e-4, atol_scale=1e-5,
                 what=f'{base_model} {dtype} identity.mean(1) vs avg')


@pytest.mark.parametrize('dtype,fmt', [('f32', 'kPrecF32'), ('bf16x3', 'kPrecBf16x3'), ('bf16', 'kPrecBf16')])
def test_what_runs_and_what_is_timed(hip_lib, dtype, fmt):
    """An identity forward runs head_seg_kernel of the engine's storage format and neither kernel of the avg head; an avg
    forward the reverse.  The launch names and the per-launch times keep the avg engine's keys, 'head' recorded."""
    from workoutdetector_amd.engine import launch_trace
    x = cs.case_input('resnet50', 'blockres')[:2]
    seen = {}
    for consensus in ('avg', 'identity'):
        eng = _engine('resnet50', 'blockres', dtype, consensus)
        try:
            eng.run(None, {'input': x})          # (tunes)
            eng.set_layer_timing(1)
            with launch_trace() as tr:
                eng.run(None, {'input': x})
            seen[consensus] = (tr, eng.launch_names(), eng.layer_times_ms(0), eng.conv_tiles(2))
        finally:
            eng.close()
    tr, names, times, tiles = seen['identity']
    assert tr.count('head_seg_kernel<') == 1 and tr.ran(f'head_seg_kernel<{fmt}>'), tr.kernels
    assert_not_ran(tr, 'head_pool_kernel<', 'identity')
    assert_not_ran(tr, 'head_fc_kernel', 'identity')
    tr_avg, names_avg, times_avg, tiles_avg = seen['avg']
    assert_ran(tr_avg, 'head_pool_kernel<', 'avg')
    assert_ran(tr_avg, 'head_fc_kernel', 'avg')
    assert_not_ran(tr_avg, 'head_seg_kernel<', 'avg')
    assert names == names_avg and list(times) == list(times_avg) == names and list(tiles) == list(tiles_avg)
    assert times['head'] > 0 and times_avg['head'] > 0


def test_set_consensus_contract(hip_lib):
    """tsm_set_consensus: legal until the first tsm_set_tensor, other values unsupported -- tsm_set_shift_place's contract."""
    from workoutdetector_amd.engine import TsmEngine
    eng = TsmEngine(num_class=3, height=64, width=64, max_clips=1)
    try:
        assert hip_lib.tsm_set_consensus(eng._h, 2) == -7 and b'consensus' in hip_lib.tsm_last_error(eng._h)
        assert hip_lib.tsm_set_consensus(eng._h, -1) == -7
        assert hip_lib.tsm_set_consensus(eng._h, 1) == 0 and hip_lib.tsm_set_consensus(eng._h, 0) == 0
        w = np.zeros((3, 2048), np.float32)
        shape = (ctypes.c_int64 * 2)(3, 2048)
        assert hip_lib.tsm_set_tensor(eng._h, b'fc.weight', w.ctypes.data, shape, 2) == 0
        assert hip_lib.tsm_set_consensus(eng._h, 1) == -1 and b'tsm_set_consensus' in hip_lib.tsm_last_error(eng._h)
    finally:
        eng.close()


def test_a_tune_cache_written_by_an_avg_engine_serves_an_identity_engine(hip_lib, monkeypatch, tmp_path):
    cache = tmp_path / 'tune.txt'
    monkeypatch.setenv('TSM_TUNE_CACHE', str(cache))
    monkeypatch.delenv('TSM_AUTOTUNE', raising=False)
    sd = cs.state_dict('resnet18', 'blockres')[0]
    eng = _engine('resnet18', 'blockres', 'bf16', 'avg', sd=sd)
    try:
        eng.warmup([2])
        tiles = eng.conv_tiles(2)
    finally:
        eng.close()
    written = cache.read_text()
    assert written.strip(), 'the avg engine wrote no cache line'
    eng = _engine('resnet18', 'blockres', 'bf16', 'identity', sd=sd)
    try:
        eng.warmup([2])
        assert eng.conv_tiles(2) == tiles
        assert eng.run(None, {'input': cs.case_input('resnet18', 'blockres')[:2]})[0].shape == (2, cs.T, cs.NUM_CLASS)
    finally:
        eng.close()
    assert cache.read_text() == written, 'the identity engine tuned again instead of reading the avg engine\'s line'


# ---- TSM_POISON=1 --------------------------------------------------------------------------------------------------------------
def _env(monkeypatch, poison):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if poison:
        monkeypatch.setenv('TSM_POISON', '1')


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('base_model', ['resnet18', 'resnet50'])
def test_identity_engine_under_poison(hip_lib, monkeypatch, capsys, base_model, dtype):
    """Every device buffer between poisoned bands, the workspace (the T-times larger d_logits included) poisoned before each
    forward, the bands verified after it: the tuning pass, tsm_tune, a tap, host and device forwards all succeed, no poison
    word reaches the [B, T, C] output, and the result is the clean engine's bit for bit.  (The environment is read in
    tsm_create, so each engine of the pair is built under its own setting, as in tests/test_poison_gpu.py.)"""
    x = cs.case_input(base_model, 'blockres')
    out = {}
    for poison in (False, True):
        _env(monkeypatch, poison)
        eng = _engine(base_model, 'blockres', dtype)
        try:
            first = eng.run(None, {'input': x})[0]                   # tunes buckets 2 and 1 into d_logits, then the forwards
            eng.warmup([1, 2])
            tap = eng.forward_tap(x[:2], 'layer4.1')                  # (runs the forward into d_logits up to the stage)
            host = eng.run(None, {'input': x})[0]
            dev = eng.forward_device(torch.from_numpy(x).cuda()).cpu().numpy()
        finally:
            eng.close()
        out[poison] = dict(first=first, tap=tap, host=host, dev=dev)
    for name, a in out[True].items():
        a = np.ascontiguousarray(a)
        assert not (a.view(np.uint32) == POISON).any(), f'{name}: holds the poison word'
        assert np.isfinite(a).all(), f'{name}: non-finite values'
        assert np.array_equal(a, out[False][name]), f'{name}: TSM_POISON=1 moved bits'
    assert np.array_equal(out[True]['host'], out[True]['dev']) and np.array_equal(out[True]['host'], out[True]['first'])
    _against_reference(out[True]['host'], base_model, 'blockres', dtype, f'{base_model} {dtype} identity poisoned', capsys)


# ---- use ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('threshold', [0.5, 0.2])
def test_per_segment_states_equal_the_host_counting_path(hip_lib, threshold):
    """[B, T, C] -> B*T rows with .view: scores_to_states on the GPU equals counting.scores_to_preds on the same rows."""
    from workoutdetector_amd.counting import scores_to_preds
    from workoutdetector_amd.engine import scores_to_states
    x = cs.case_input('resnet18', 'blockres')
    eng = _engine('resnet18', 'blockres', 'f32', max_clips=cs.B)
    try:
        logits = eng.forward_device(torch.from_numpy(x).cuda())
    finally:
        eng.close()
    rows = logits.view(cs.B * cs.T, cs.NUM_CLASS)
    for softmax in (True, False):
        states = scores_to_states(rows, threshold=threshold, softmax=softmax).cpu().tolist()
        assert states == scores_to_preds(rows.cpu().numpy().tolist(), threshold=threshold, softmax=softmax)
    assert len(states) == cs.B * cs.T
