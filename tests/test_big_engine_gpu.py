"""The engine at the next sizes up from config 5 (B = 64, T = 16, 256^2, whose largest activation is exactly 2^32 bytes in fp32 and
2^31 in bf16): T = 8 at 256^2 with

  f32   B = 136   stem and layer1 outputs of 4.56e9 bytes, past 2^32
  bf16  B = 264   the largest activation 4.43e9 bytes, past 2^32; the weight-stationary kernels still inside their rules
  bf16  B = 480   layer1 has M = 15.7 M rows, past M * 128 < 2.0e9: layer1's conv1x1_ws / conv3x3_ws forms must give way

by the periodic method of tests/test_big_conv_gpu.py: the input is two distinct clips repeated B / 2 times on the device, so the
feature rows and the logits must repeat with that period bit for bit (batch invariance: an element's bits do not depend on its
batch, tile or launch), the first two logit rows must equal a forward of those two clips alone on the same engine bit for bit,
and they meet the CPU oracle at the bars of tests/test_full_size_gpu.py.  A forced and an unforced engine of one size agree bit
for bit: the forced engines run with TSM_AUTOTUNE=0, so that the trace holds the forced forms' launches only, and between them
show every tile-walking family (tests._util.WALKING) at one of these sizes; the unforced engine of each dtype has NO switch set
(the tuner picks tiles and fused forms on the real launches) and must give the same bits.  Every engine runs under TSM_POISON=1
(a stray store lands in a band and fails the forward).  A temporal_pool engine at B = 136 (f32 and bf16x3) runs
temporal_maxpool_kernel on layer1's 4.56e9-byte output, against the float64 torch model at the bars of
tests/test_temporal_pool_gpu.py.  No tap is pulled to the host."""
import pytest
import torch

from oracle import tsm_oracle
from tests._big_cases import rule_accepts
from tests._guard import POISON
from tests._util import WALKING, assert_close, assert_periodic, bf16_logits_report, make_input

pytestmark = pytest.mark.gpu

T, S, P = 8, 256, 2
FUSE = ('TSM_FUSE_BLOCK', 'TSM_FUSE_FRONT', 'TSM_FUSE_C3C1', 'TSM_FUSE_CONV23')
KNOBS = FUSE + ('TSM_AUTOTUNE', 'TSM_WALK', 'TSM_CONV_TILE', 'TSM_CONV_CODE', 'TSM_TUNE_CACHE', 'TSM_POISON', 'TSM_POS_MAJOR')
# engine -> (dtype, clips, switches, the tile-walking families its trace must show)
ENGINES = {
    'f32-136-conv23': ('f32', 136, {'TSM_FUSE_CONV23': '1', 'TSM_POS_MAJOR': '1'}, ('conv_igemm<', 'conv23_fused_kernel<')),
    'f32-136-plain': ('f32', 136, {'TSM_FUSE_CONV23': '0', 'TSM_POS_MAJOR': '0'}, ('conv_igemm<',)),
    'bf16-264-fused-ws': ('bf16', 264, dict({k: '1' for k in FUSE}, TSM_CONV_TILE='ws'),
                          ('bneck_ws_kernel<', 'front_s2_kernel<', 'conv31_', 'conv3x3_ws', 'conv1x1_ws')),
    'bf16-264-256p': ('bf16', 264, dict({k: '0' for k in FUSE}, TSM_CONV_TILE='256x256p'), ('conv_bf16_256',)),
    # (the same switches as the B = 480 engine below: here, inside their rules, layer1's weight-stationary forms run)
    'bf16-264-ws': ('bf16', 264, dict({k: '0' for k in FUSE}, TSM_CONV_TILE='ws'),
                    ('conv1x1_ws_kernel<', 'conv3x3_ws_kernel<false>', 'conv3x3_ws128_kernel<', 'conv1x1_wsn_kernel<')),
    # no switch set: the tuning pass chooses (a None in place of the switches)
    'f32-136-default': ('f32', 136, None, ()),
    'bf16-264-default': ('bf16', 264, None, ()),
    'bf16-480-ws': ('bf16', 480, dict({k: '0' for k in FUSE}, TSM_CONV_TILE='ws'),
                    ('conv3x3_ws', 'conv1x1_ws', 'conv_igemm<')),
}
assert set(WALKING) <= {f for e in ENGINES.values() for f in e[3]}


@pytest.fixture(scope='module')
def clips():
    """The two distinct clips every batch here repeats."""
    return torch.from_numpy(make_input(2048, P, T, S, S))


@pytest.fixture(scope='module')
def oracle(clips, sd0):
    """Their oracle logits, fp32 and bf16 storage, computed once."""
    return {'f32': tsm_oracle.tsm_forward(sd0, clips, n_segment=T).numpy(),
            'bf16': tsm_oracle.tsm_forward_bf16(sd0, clips, n_segment=T).numpy()}


def _run(monkeypatch, sd0, clips, name, engine=None, **engine_kw):
    """One engine on its periodic batch: (logits, features) as device tensors, after the periodicity, first-period and trace checks."""
    from workoutdetector_amd.engine import TsmEngine, launch_trace
    dtype, b, env, families = engine or ENGINES[name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    switches = {} if env is None else dict(env, TSM_AUTOTUNE='0')
    for k, v in dict(switches, TSM_TUNE_CACHE='off', TSM_POISON='1').items():
        monkeypatch.setenv(k, v)
    x = clips.cuda().repeat(b // P, 1, 1, 1, 1)
    eng = TsmEngine(num_segments=T, height=S, width=S, max_clips=b, state_dict=sd0, dtype=dtype, **engine_kw)
    rows = b * eng.out_segments
    try:
        with launch_trace() as tr:
            feats = eng.forward_features(x)
            torch.cuda.synchronize()
            logits = eng.forward_device(x)
            torch.cuda.synchronize()
        for fam in families:
            assert tr.ran(fam), (name, fam, sorted(set(tr.kernels)))
        assert tuple(feats.shape) == (rows, 2048) and tuple(logits.shape) == (b, 12)
        assert bool(torch.isfinite(logits).all()) and not bool((logits.view(torch.int32) == POISON).any()), name
        assert_periodic(feats, b // P, f'{name}: feature rows')
        assert_periodic(logits, b // P, f'{name}: logits')
        alone = eng.forward_device(x[:P].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(logits[:P], alone), f'{name}: the first {P} clips of the batch differ from a forward of them alone'
        print(f'\n[{name}] torch peak {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB, '
              f'device memory in use {(torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0]) / 2 ** 30:.1f} GiB')
        return logits.clone(), feats.clone(), tr
    finally:
        eng.close()
        del x
        torch.cuda.empty_cache()


def _meets_oracle(name, logits, oracle, capsys):
    got = logits[:P].cpu().numpy()
    if ENGINES[name][0] == 'f32':
        assert_close(got, oracle['f32'], rtol=1e-3, atol_scale=1e-5, what=name)
    else:
        bf16_logits_report(got, oracle['bf16'], oracle['f32'], name, capsys)


@pytest.mark.parametrize('forced,others', [('f32-136-conv23', ('f32-136-plain', 'f32-136-default')),
                                           ('bf16-264-fused-ws', ('bf16-264-256p', 'bf16-264-ws', 'bf16-264-default'))])
def test_engine_past_2_32(hip_lib, monkeypatch, sd0, clips, oracle, capsys, forced, others):
    la, fa, _ = _run(monkeypatch, sd0, clips, forced)
    _meets_oracle(forced, la, oracle, capsys)
    for other in others:
        lb, fb, _ = _run(monkeypatch, sd0, clips, other)
        assert torch.equal(la, lb), f'{forced} and {other}: logits differ'
        assert torch.equal(fa, fb), f'{forced} and {other}: feature rows differ'


def test_engine_past_the_ws_rules(hip_lib, monkeypatch, sd0, clips, oracle, capsys):
    """B = 480: layer1 (64 x 64 pixels) has 15 728 640 rows.  The restated rules refuse conv1x1_ws and conv3x3_ws<false> there
    (M * 128 >= 2.0e9) and still accept the 128-channel 3x3 forms of layer2 (M * 256 < 2.0e9 at 32 x 32 pixels): none of the
    former is in the trace, the latter are."""
    name = 'bf16-480-ws'
    b = ENGINES[name][1]
    layer1 = dict(hi=64, wi=64, k=1, stride=1, cin=64, cout=64)
    assert not rule_accepts(dict(layer1, family='ws1x1'), b * T) and rule_accepts(dict(layer1, family='ws1x1'), 264 * T)
    assert not rule_accepts(dict(layer1, family='ws3x3', k=3), b * T)
    assert rule_accepts(dict(hi=32, wi=32, k=3, stride=1, cin=128, cout=128, family='ws128'), b * T)
    logits, _, tr = _run(monkeypatch, sd0, clips, name)
    for refused in ('conv1x1_ws_kernel<', 'conv3x3_ws_kernel<false>'):
        assert not tr.ran(refused), f'{name}: {refused} ran at a size its rule refuses: {sorted(set(tr.kernels))}'
    assert tr.ran('conv3x3_ws128_kernel<false>'), sorted(set(tr.kernels))
    _meets_oracle(name, logits, oracle, capsys)


@pytest.fixture(scope='module')
def pool_reference(clips):
    """The float64 torch model with the temporal pool on the two clips: (state dict, logits, pooled features), computed once."""
    from tests._temporal_pool import run_with_taps, torch_tsm_tp
    from workoutdetector_amd.weights import make_state_dict
    sd = make_state_dict(0, 12)
    logits, _, pooled, _ = run_with_taps(torch_tsm_tp('resnet50', 'blockres', 12, T, sd=sd), clips.numpy(), ())
    return sd, logits, pooled


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3'])
def test_temporal_pool_past_2_32(hip_lib, monkeypatch, clips, pool_reference, dtype):
    """B = 136: the pool reads layer1's output, 1 088 frames of 64 x 64 x 256 (4.56e9 bytes in either format: src = x + clip * T *
    frame passes 2^32 from clip 129 on) and writes half of it; layers 2-4 run on 4 segments a clip."""
    sd, want_logits, want_pooled = pool_reference
    name = f'{dtype}-136-tpool'
    kernel = 'temporal_maxpool_kernel<%s>' % {'f32': 'kPrecF32', 'bf16x3': 'kPrecBf16x3'}[dtype]
    logits, feats, tr = _run(monkeypatch, sd, clips, name, engine=(dtype, 136, {}, (kernel, 'conv_igemm<')), temporal_pool=True)
    assert tr.count(kernel) == 2, tr.kernels                       # (one per forward inside the trace)
    assert 136 * T * 64 * 64 * 256 * 4 > 1 << 32 and tuple(feats.shape) == (136 * T // 2, 2048)
    assert_close(logits[:P].cpu().numpy(), want_logits, rtol=1e-3, atol_scale=1e-5, what=name + ' logits')
    assert_close(feats[:P * T // 2].cpu().numpy(), want_pooled, rtol=1e-3, atol_scale=1e-5, what=name + ' features')
