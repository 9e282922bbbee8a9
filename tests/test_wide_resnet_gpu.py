"""TSM-Wide-ResNet-50-2 on the MI355X: logits and stage taps against the CPU oracle (which reads every width from the state
dict: oracle/tsm_oracle.py) under both shift placements, the two-chunk fused conv2 + conv3 kernel of layer1.1-2 (bitwise
against the separate launches), every other fused / specialised form either bit-identical or refused, tuned vs untuned,
the tsm_set_bottleneck_width contract and the tune cache.

Bars as for the R50 engine: fp32 and split-bf16 rtol 1e-3 against the fp32 oracle; bf16 BF16_E2E_BAR of the logit scale
against the bf16-storage oracle (bf16_logits_report), BF16_TAP_BAR on taps."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import tsm_oracle
from tests._util import BF16_TAP_BAR, assert_close, assert_fused_slots, bf16_logits_report, make_input

pytestmark = pytest.mark.gpu

WRN = 'wide_resnet50_2'
TAPS = ['layer1.0', 'layer1.1', 'layer1.2', 'layer4.2']


def _sd(seed=0, place='blockres'):
    from workoutdetector_amd.weights import make_state_dict
    return make_state_dict(seed, 12, base_model=WRN, shift_place=place)


def _torch_sd(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


# (dtype, shift_place, T, is_shift, size, taps): the three precisions at 224^2 with taps; both placements, T = 8 / 16 and
# the shift off at 112 x 128 (odd tile counts per frame)
CASES = [('f32', 'blockres', 8, True, (224, 224), True),
         ('bf16x3', 'blockres', 8, True, (224, 224), True),
         ('bf16', 'blockres', 8, True, (224, 224), True),
         ('f32', 'block', 8, True, (112, 128), True),
         ('bf16x3', 'block', 16, True, (112, 128), False),
         ('bf16', 'block', 16, True, (112, 128), False),
         ('f32', 'blockres', 16, False, (112, 128), False),
         ('bf16x3', 'blockres', 16, True, (112, 128), False),
         ('bf16', 'blockres', 8, False, (112, 128), False)]


@pytest.mark.parametrize('dtype,place,T,is_shift,size,taps', CASES)
def test_wide_engine_against_oracle(hip_lib, capsys, dtype, place, T, is_shift, size, taps):
    from workoutdetector_amd.engine import create_model
    h, w = size
    sd = _sd(0, place)
    eng = create_model(num_class=12, num_segments=T, base_model=WRN, shift_place=place, is_shift=is_shift, height=h,
                       width=w, max_clips=2, dtype=dtype)
    x = make_input(41 + T, 2, T, h, w)
    got = eng.run(None, {'input': x})[0]
    t32, t16 = {}, {}
    want = tsm_oracle.forward(_torch_sd(sd), torch.from_numpy(x), WRN, place, n_segment=T, is_shift=is_shift, taps=t32).numpy()
    what = f'WRN-50-2 {dtype} {place} T{T} shift {is_shift} {h}x{w}'
    if dtype == 'bf16':
        want16 = tsm_oracle.forward(_torch_sd(sd), torch.from_numpy(x), WRN, place, True, n_segment=T, is_shift=is_shift,
                                    taps=t16).numpy()
        bf16_logits_report(got, want16, want, what, capsys)
    else:
        assert_close(got, want, rtol=1e-3, atol_scale=1e-5, what=what + ' logits')
    if taps:
        for stage in TAPS:
            g = eng.forward_tap(x, stage)
            if dtype == 'bf16':
                t = t16[stage].permute(0, 2, 3, 1).numpy()
                assert g.shape == t.shape, stage
                e = float(np.abs(g - t).max()) / float(np.abs(t).max())
                assert e <= BF16_TAP_BAR, (what, stage, e)
            else:
                assert_close(g, t32[stage].permute(0, 2, 3, 1).numpy(), rtol=1e-3, atol_scale=3e-5, what=f'{what} {stage}')
    eng.close()


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3'])
def test_wide_fused_conv23_is_the_two_chunk_kernel_and_bitwise(hip_lib, monkeypatch, dtype):
    """TSM_FUSE_CONV23=1: layer1.1 and layer1.2 (128 mid channels, 256 outputs) run conv23_fused2_kernel, never the
    four-chunk conv23_fused_kernel; layer2-4 (mid 256+) keep their separate launches.  Logits and taps bitwise equal to
    TSM_FUSE_CONV23=0."""
    from workoutdetector_amd.engine import create_model, launch_trace
    monkeypatch.setenv('TSM_AUTOTUNE', '0')
    x = make_input(7, 2, 8, 224, 224)
    out = {}
    for fuse in ('0', '1'):
        monkeypatch.setenv('TSM_FUSE_CONV23', fuse)
        eng = create_model(num_class=12, base_model=WRN, max_clips=2, dtype=dtype)
        with launch_trace() as tr:
            logits = eng.run(None, {'input': x})[0]
        if fuse == '1':
            assert tr.count('conv23_fused2_kernel<128, ') == 2, tr.kernels
            assert not tr.ran('conv23_fused_kernel<'), tr.kernels
            assert_fused_slots(eng, x, {'layer1.1.conv3', 'layer1.2.conv3'}, what=dtype)
        else:
            assert not tr.ran('conv23_fused'), tr.kernels
        out[fuse] = [logits] + [eng.forward_tap(x, s) for s in ('layer1.1', 'layer1.2', 'layer2.1')]
        eng.close()
    for a, b, what in zip(out['0'], out['1'], ['logits', 'layer1.1', 'layer1.2', 'layer2.1']):
        assert np.array_equal(a, b), (dtype, what)


def test_wide_fused_conv23_tap_of_conv2_keeps_the_separate_launches(hip_lib, monkeypatch):
    """A tap of layer1.1.conv2 needs the mid tensor in memory: the fused form stands down for that block only."""
    from workoutdetector_amd.engine import create_model, launch_trace
    monkeypatch.setenv('TSM_AUTOTUNE', '0')
    monkeypatch.setenv('TSM_FUSE_CONV23', '1')
    eng = create_model(num_class=12, base_model=WRN, height=112, width=112, max_clips=1)
    x = make_input(8, 1, 8, 112, 112)
    with launch_trace() as tr:
        eng.forward_tap(x, 'layer1.1.conv2')
    assert tr.count('conv23_fused2_kernel<') == 0, tr.kernels      # (the forward stops at the tapped layer)
    with launch_trace() as tr:
        eng.forward_tap(x, 'layer1.2')
    assert tr.count('conv23_fused2_kernel<') == 2, tr.kernels
    eng.close()


@pytest.mark.parametrize('var,family', [('TSM_FUSE_BLOCK', 'bneck_ws'), ('TSM_FUSE_FRONT', 'front_s2'),
                                        ('TSM_FUSE_C3C1', 'conv31_'), ('TSM_FUSE_CONV23', 'conv3x3_ws_kernel<')])
def test_wide_bf16_fused_forms_are_refused(hip_lib, monkeypatch, var, family):
    """The bf16 whole-block, front-of-layer2.0, conv3 + next conv1 and conv2 + conv3 forms are built for R50's widths only;
    forcing each on a WRN engine runs none of them and changes no bit."""
    from workoutdetector_amd.engine import create_model, launch_trace
    monkeypatch.setenv('TSM_AUTOTUNE', '0')
    x = make_input(9, 2, 8, 224, 224)
    res = {}
    for v in ('0', '1'):
        monkeypatch.setenv(var, v)
        eng = create_model(num_class=12, base_model=WRN, max_clips=2, dtype='bf16')
        with launch_trace() as tr:
            res[v] = eng.run(None, {'input': x})[0]
        assert not tr.ran(family), (var, v, sorted(set(tr.kernels)))
        assert not tr.ran('conv23_fused'), (var, v)
        eng.close()
    assert np.array_equal(res['0'], res['1']), var


@pytest.mark.parametrize('tile,family', [('ws', 'conv1x1_wsn_kernel<'), ('256x256', 'conv_bf16_256_kernel'),
                                         ('256x256p', 'conv_bf16_256p_kernel<')])
def test_wide_bf16_specialised_tiles_are_bit_identical(hip_lib, monkeypatch, tile, family):
    """Forced wherever their predicates accept a WRN layer (the weight-stationary 256 -> 128 shifted conv1 of layer1.1-2
    and 512 -> 256 of layer2.1-3; the 256^2 tiles), the specialised bf16 kernels give the generic 64x64 tile's bits."""
    from workoutdetector_amd.engine import create_model, launch_trace
    monkeypatch.setenv('TSM_AUTOTUNE', '0')
    x = make_input(10, 2, 8, 224, 224)
    monkeypatch.setenv('TSM_CONV_TILE', '64x64')
    eng = create_model(num_class=12, base_model=WRN, max_clips=2, dtype='bf16')
    base = eng.run(None, {'input': x})[0]
    eng.close()
    monkeypatch.setenv('TSM_CONV_TILE', tile)
    eng = create_model(num_class=12, base_model=WRN, max_clips=2, dtype='bf16')
    with launch_trace() as tr:
        got = eng.run(None, {'input': x})[0]
    assert tr.ran(family), (tile, sorted(set(tr.kernels)))
    eng.close()
    assert np.array_equal(got, base), tile


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3', 'bf16'])
def test_wide_tuned_and_untuned_forwards_are_bitwise_equal(hip_lib, monkeypatch, tmp_path, dtype):
    from workoutdetector_amd.engine import create_model
    monkeypatch.setenv('TSM_TUNE_CACHE', str(tmp_path / 'tune.txt'))
    x = make_input(11, 2, 8, 160, 160)
    eng = create_model(num_class=12, base_model=WRN, height=160, width=160, max_clips=2, dtype=dtype)
    eng.warmup([2])
    tuned = eng.run(None, {'input': x})[0]
    eng.close()
    monkeypatch.setenv('TSM_AUTOTUNE', '0')
    eng = create_model(num_class=12, base_model=WRN, height=160, width=160, max_clips=2, dtype=dtype)
    plain = eng.run(None, {'input': x})[0]
    eng.close()
    assert np.array_equal(tuned, plain), dtype


def test_set_bottleneck_width_contract(hip_lib):
    from workoutdetector_amd import _lib
    lib = _lib.load()
    cfg = _lib.TsmConfig(C.sizeof(_lib.TsmConfig), 12, 8, 64, 64, 8, 1, 1, 0, _lib.DTYPE_F32)

    def engine():
        h = C.c_void_p()
        _lib.check(lib.tsm_create(C.byref(cfg), C.byref(h)))
        return h
    h = engine()
    try:
        for bad in (0, 32, 96, 256, -64):
            assert lib.tsm_set_bottleneck_width(h, bad) == -7, bad
        assert lib.tsm_set_bottleneck_width(h, 64) == 0 and lib.tsm_set_bottleneck_width(h, 128) == 0
        for depth in (18, 34):                               # width first, BasicBlock depth second
            assert lib.tsm_set_backbone(h, depth) == -7
        assert lib.tsm_set_backbone(h, 50) == 0
        arr = np.ones(128 * 64, np.float32)
        shape = (C.c_int64 * 4)(128, 64, 1, 1)
        assert lib.tsm_set_tensor(h, b'base_model.layer1.0.conv1.net.weight', arr.ctypes.data, shape, 4) == 0
        assert lib.tsm_set_bottleneck_width(h, 64) == -1     # after the first tsm_set_tensor
        assert lib.tsm_set_bottleneck_width(h, 128) == -1
    finally:
        lib.tsm_destroy(h)
    for depth in (18, 34):                                   # BasicBlock depth first, width second
        h = engine()
        try:
            assert lib.tsm_set_backbone(h, depth) == 0
            assert lib.tsm_set_bottleneck_width(h, 128) == -7
            assert lib.tsm_set_bottleneck_width(h, 64) == 0
        finally:
            lib.tsm_destroy(h)


def test_r50_and_wrn_checkpoints_do_not_cross(hip_lib):
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import TsmEngine
    from workoutdetector_amd.weights import make_state_dict
    with pytest.raises(_lib.TsmError, match=r'TSM_ERR_SHAPE: shape mismatch for base_model\.layer1\.0\.conv1\.net\.weight'):
        TsmEngine(num_class=12, height=64, width=64, max_clips=1, base_model=WRN, state_dict=make_state_dict(0, 12))
    with pytest.raises(_lib.TsmError, match=r'TSM_ERR_SHAPE: shape mismatch for base_model\.layer1\.0\.conv1\.net\.weight'):
        TsmEngine(num_class=12, height=64, width=64, max_clips=1, state_dict=_sd())


def test_tune_cache_keeps_wrn_and_r50_apart(hip_lib, monkeypatch, tmp_path):
    import re
    from workoutdetector_amd.engine import create_model
    cache = tmp_path / 'tune.txt'
    monkeypatch.setenv('TSM_TUNE_CACHE', str(cache))
    create_model(num_class=12, base_model=WRN, height=64, width=64, max_clips=1).warmup([1]).close()
    lines = cache.read_text().splitlines()
    assert len(lines) == 1 and lines[0].split('|')[0].endswith(' w128'), lines
    create_model(num_class=12, height=64, width=64, max_clips=1).warmup([1]).close()
    lines = cache.read_text().splitlines()
    assert len(lines) == 2 and not re.search(r' (w\d+|r\d+|block)\|', lines[1]), lines
    create_model(num_class=12, base_model=WRN, shift_place='block', height=64, width=64, max_clips=1).warmup([1]).close()
    lines = cache.read_text().splitlines()
    assert len(lines) == 3 and lines[2].split('|')[0].endswith(' w128 block'), lines
    # a second WRN engine reads its line back: no new one
    create_model(num_class=12, base_model=WRN, height=64, width=64, max_clips=1).warmup([1]).close()
    assert len(cache.read_text().splitlines()) == 3


def test_wrn_onnx_export_runs_on_the_engine(hip_lib, tmp_path):
    from tests._torch_tsm import LitWrapper, TorchTSM, export_onnx
    from workoutdetector_amd.engine import create_model
    sd = _sd(6)
    net = TorchTSM(WRN, 128).load_engine_state_dict(sd)
    path = str(tmp_path / 'tsm_wrn.onnx')
    export_onnx(LitWrapper(net), path, sample_shape=(1, 8, 3, 64, 64))
    eng = create_model(num_class=12, checkpoint=path, base_model=WRN, height=112, width=112, max_clips=2)
    x = make_input(3, 2, 8, 112, 112)
    want = tsm_oracle.forward(_torch_sd(sd), torch.from_numpy(x), WRN).numpy()
    assert_close(eng.run(None, {'input': x})[0], want, rtol=1e-3, atol_scale=1e-5, what='onnx wrn')
    eng.close()
