"""TSM-ResNet18 / 34 on the MI355X: the shifted 3x3 loader and the 3x3 + residual epilogue per op, the BasicBlock
forward end to end against the CPU reference (oracle/tsm_oracle.py), and what runs (launch trace).

Bars: fp32 and split-bf16 as for the R50 engine (rtol 1e-3 on logits and taps); bf16 against the bf16-storage
restatement (BF16_E2E_BAR on logits, BF16_TAP_BAR on taps); per op as in test_ops_gpu / test_bf16x3_gpu / test_bf16_gpu."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from oracle import tsm_oracle
from tests._util import BF16_TAP_BAR, assert_bf16_op, assert_close, bf16_logits_report, make_input

pytestmark = pytest.mark.gpu


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _bn(c, g):
    return (torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1,
            torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5)


def _check_op(got, x, w, bn, stride, relu, res, dtype, shiftT=0, div=8):
    xin = tsm_oracle.temporal_shift(x, shiftT, div) if shiftT else x
    if dtype == 'bf16':
        assert_bf16_op(_nchw(got.cpu()).numpy(), tsm_oracle.conv_bn_act_bf16(xin, w, bn, stride, 1, relu, res).numpy(),
                       what='3x3 bf16')
    else:
        want = tsm_oracle.conv_bn_act(xin, w, bn, stride, 1, relu, res).numpy()
        tol = 1e-4 if dtype == 'f32' else 3e-4
        assert_close(_nchw(got.cpu()).numpy(), want, rtol=tol, atol_scale=tol, what=f'3x3 {dtype}')


# (n frames, hi, wi, cin, cout, stride, T, shift_div): frames of 7x7 .. 15x13 outputs put every 64-row tile across a frame
# boundary, clip boundaries every T frames, and the 3x3 padding on every tile's edge rows
SHIFT3_CASES = [
    (16, 14, 14, 64, 64, 1, 8, 8),
    (16, 15, 13, 128, 128, 2, 8, 8),      # odd sizes, stride 2
    (32, 9, 11, 64, 128, 1, 16, 8),       # T = 16, ragged M
    (16, 7, 7, 256, 256, 2, 8, 16),       # layer4-like, fold 16
    (16, 14, 14, 512, 512, 1, 8, 8),      # layer4 class, fold 64
    (64, 28, 28, 64, 128, 2, 8, 8),       # stride 2 from 28x28
    (64, 28, 28, 64, 128, 1, 8, 8),       # >= 256 tiles of 128 rows: the 128x128 path
    (16, 14, 14, 64, 64, 1, 8, 16),       # fold 4: fp32 only (the bf16 formats need fold % 8 == 0)
]
SHIFT3_PARAMS = [(d,) + c for d in ('f32', 'bf16x3', 'bf16') for c in SHIFT3_CASES if d == 'f32' or (c[3] // c[7]) % 8 == 0]


@pytest.mark.parametrize('dtype,n,hi,wi,cin,cout,stride,T,div', SHIFT3_PARAMS)
def test_shifted_3x3(hip_lib, dtype, n, hi, wi, cin, cout, stride, T, div):
    from workoutdetector_amd.engine import conv_bn_act_nhwc, launch_trace
    g = torch.Generator().manual_seed(77 + cin + cout + hi + stride + T + div)
    x = torch.randn(n, cin, hi, wi, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    bn = _bn(cout, g)
    with launch_trace() as tr:
        got = conv_bn_act_nhwc(_nhwc(x).cuda(), w.cuda(), *[b.cuda() for b in bn], stride=stride, relu=True,
                               shift_segments=T, fold_div=div, dtype=dtype)
    assert any('KS = 3, SHIFT = true' in k for k in tr.kernels), tr.kernels
    assert not tr.ran('temporal_shift_kernel'), tr.kernels
    _check_op(got, x, w, bn, stride, True, None, dtype, T, div)


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('n,hi,wi,cin,cout,stride', [(16, 14, 14, 64, 64, 1), (16, 15, 13, 128, 256, 2),
                                                     (8, 7, 7, 512, 512, 1), (64, 28, 28, 128, 128, 1)])
def test_3x3_with_residual(hip_lib, dtype, n, hi, wi, cin, cout, stride):
    from workoutdetector_amd.engine import conv_bn_act_nhwc, launch_trace
    g = torch.Generator().manual_seed(500 + cin + cout + hi + stride)
    x = torch.randn(n, cin, hi, wi, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    bn = _bn(cout, g)
    ho, wo = (hi - 1) // stride + 1, (wi - 1) // stride + 1
    res = torch.randn(n, cout, ho, wo, generator=g)
    with launch_trace() as tr:
        got = conv_bn_act_nhwc(_nhwc(x).cuda(), w.cuda(), *[b.cuda() for b in bn], stride=stride, relu=True,
                               residual=_nhwc(res).cuda(), dtype=dtype)
    assert any('KS = 3, SHIFT = false, RES = true' in k for k in tr.kernels), tr.kernels
    _check_op(got, x, w, bn, stride, True, res, dtype)


def test_shifted_3x3_is_bit_identical_across_tiles(hip_lib, monkeypatch):
    """Every generic tile shape runs the shifted loader and accumulates each output in the same k order."""
    from workoutdetector_amd.engine import conv_bn_act_nhwc, launch_trace
    from tests._util import assert_ran_tile
    g = torch.Generator().manual_seed(9)
    x = torch.randn(32, 128, 15, 13, generator=g)
    w = torch.randn(128, 128, 3, 3, generator=g) * (2.0 / (128 * 9)) ** 0.5
    bn = _bn(128, g)
    outs = {}
    for tile in ('128x128', '128x64', '64x64', '32x32', '128x128w8'):
        monkeypatch.setenv('TSM_CONV_TILE', tile)
        with launch_trace() as tr:
            outs[tile] = conv_bn_act_nhwc(_nhwc(x).cuda(), w.cuda(), *[b.cuda() for b in bn], stride=2, relu=True,
                                          shift_segments=8, fold_div=8).cpu()
        assert_ran_tile(tr, tile, what=tile)
    first = outs['64x64']
    for tile, o in outs.items():
        assert torch.equal(o, first), tile
    _check_op(first.cuda(), x, w, bn, 2, True, None, 'f32', 8, 8)


def test_shifted_3x3_refuses_what_it_does_not_implement(hip_lib):
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import conv_bn_act_nhwc
    x = torch.randn(16, 14, 14, 64).cuda()
    w = torch.randn(64, 64, 3, 3).cuda()
    bn = [torch.ones(64).cuda() for _ in range(4)]
    with pytest.raises(_lib.TsmError):          # shift + residual: no such launch
        conv_bn_act_nhwc(x, w, *bn, residual=torch.zeros(16, 14, 14, 64).cuda(), shift_segments=8)
    with pytest.raises(_lib.TsmError):          # frames not a whole number of clips
        conv_bn_act_nhwc(x[:12], w, *bn, shift_segments=8)


# ---- engine -----------------------------------------------------------------------------------------------------------
def _sd(base_model, seed=0):
    from workoutdetector_amd.weights import make_state_dict
    return make_state_dict(seed, 12, base_model=base_model)


def _torch_sd(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


TAPS = {'resnet18': ['layer1.0.conv1', 'layer1.1', 'layer2.0.conv1', 'layer2.0', 'layer3.1.conv1', 'layer4.0', 'layer4.1'],
        'resnet34': ['layer1.2.conv1', 'layer2.0.conv1', 'layer2.3', 'layer3.0', 'layer3.5.conv1', 'layer4.2']}


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('h,w', [(224, 224), (97, 131)])
@pytest.mark.parametrize('base_model', ['resnet18', 'resnet34'])
def test_basic_engine_against_cpu_reference(hip_lib, capsys, base_model, h, w, dtype):
    from workoutdetector_amd.engine import create_model
    sd = _sd(base_model)
    eng = create_model(num_class=12, base_model=base_model, height=h, width=w, max_clips=2, dtype=dtype)
    x = make_input(31, 2, 8, h, w)
    taps, taps16 = {}, {}
    want = tsm_oracle.forward(_torch_sd(sd), torch.from_numpy(x), base_model, taps=taps).numpy()
    got = eng.run(None, {'input': x})[0]
    what = f'{base_model} {dtype} {h}x{w}'
    if dtype == 'bf16':
        want16 = tsm_oracle.forward(_torch_sd(sd), torch.from_numpy(x), base_model, bf16=True, taps=taps16).numpy()
        bf16_logits_report(got, want16, want, what, capsys)
    else:
        assert_close(got, want, rtol=1e-3, atol_scale=1e-5, what=what + ' logits')
    for stage in TAPS[base_model]:
        g = eng.forward_tap(x, stage)
        if dtype == 'bf16':
            t = taps16[stage].permute(0, 2, 3, 1).numpy()
            assert g.shape == t.shape, stage
            e = float(np.abs(g - t).max()) / float(np.abs(t).max())
            assert e <= BF16_TAP_BAR, (what, stage, e)
        else:
            assert_close(g, taps[stage].permute(0, 2, 3, 1).numpy(), rtol=1e-3, atol_scale=3e-5, what=f'{what} {stage}')
    eng.close()


def _igemm_dims(k):
    i = k.find('[BM = ')
    return k[i:].split(', KS')[0] if i >= 0 else ''


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_basic_forward_runs_the_shifted_3x3_and_no_bottleneck_kernel(hip_lib, dtype):
    from workoutdetector_amd.engine import create_model, launch_trace
    eng = create_model(num_class=12, base_model='resnet18', max_clips=2, dtype=dtype)
    x = make_input(4, 2, 8, 224, 224)
    eng.warmup([2])
    with launch_trace() as tr:
        eng.run(None, {'input': x})
    shifted = [k for k in tr.kernels if k.startswith('conv_igemm<') and 'KS = 3, SHIFT = true' in k]
    residual = [k for k in tr.kernels if k.startswith('conv_igemm<') and 'KS = 3, SHIFT = false, RES = true' in k]
    assert len(shifted) == 8 and len(residual) == 8, tr.kernels          # conv1 and conv2 of each of the 8 blocks
    for fam in ('temporal_shift_kernel', 'bneck_ws', 'conv23_fused', 'conv31', 'front_s2'):
        assert not tr.ran(fam), (fam, tr.kernels)
    assert len(eng.launch_names()) == 3 + 8 * 2 + 3 + 1
    tiles = eng.conv_tiles(2)
    assert list(tiles) == [n for n in eng.launch_names() if n not in ('pack_input', 'maxpool', 'head')]
    eng.set_layer_timing(1)
    eng.run(None, {'input': x})
    times = eng.layer_times_ms(0)
    assert all(times[f'layer{li}.{b}.conv{c}'] > 0 for li in range(1, 5) for b in range(2) for c in (1, 2))
    eng.close()


def test_basic_engine_without_shift(hip_lib):
    from workoutdetector_amd.engine import create_model, launch_trace
    sd = _sd('resnet18', 2)
    eng = create_model(num_class=12, base_model='resnet18', is_shift=False, height=128, width=160, max_clips=2, seed=2)
    x = make_input(8, 2, 8, 128, 160)
    with launch_trace() as tr:
        got = eng.run(None, {'input': x})[0]
    assert not any('SHIFT = true' in k for k in tr.kernels)
    want = tsm_oracle.forward(_torch_sd(sd), torch.from_numpy(x), 'resnet18', is_shift=False).numpy()
    assert_close(got, want, rtol=1e-3, atol_scale=1e-5, what='resnet18 no shift')
    shifted = tsm_oracle.forward(_torch_sd(sd), torch.from_numpy(x), 'resnet18').numpy()
    assert np.abs(shifted - want).max() > 1e-3 * np.abs(want).max()      # the shift matters at this size


@pytest.mark.parametrize('dtype,codes', [('f32', (1, 2, 3, 4, 5)), ('bf16', (1, 2, 3, 5))])
def test_basic_engine_bit_identical_across_tile_codes(hip_lib, monkeypatch, dtype, codes):
    from tests._util import IGEMM_TILE_DIMS
    from workoutdetector_amd.engine import TsmEngine, create_model, launch_trace
    monkeypatch.setenv('TSM_AUTOTUNE', '0')
    x = make_input(12, 2, 8, 112, 144)
    stages = ['layer1.0.conv1', 'layer2.0', 'layer3.1.conv1', 'layer4.1']
    results = {}
    for code in codes:
        monkeypatch.setenv('TSM_CONV_CODE', str(code))
        eng = create_model(num_class=12, base_model='resnet18', height=112, width=144, max_clips=2, dtype=dtype)
        with launch_trace() as tr:
            logits = eng.run(None, {'input': x})[0]
        dims = '[BM = %d, BN = %d, WGM = %d, WGN = %d' % IGEMM_TILE_DIMS[TsmEngine.TILE_NAMES[code]]
        basic = [k for k in tr.kernels if k.startswith('conv_igemm<') and 'KS = 3' in k]
        assert any(_igemm_dims(k) == dims for k in basic if 'SHIFT = true' in k), (code, basic)
        assert any(_igemm_dims(k) == dims for k in basic if 'RES = true' in k), (code, basic)
        results[code] = [logits] + [eng.forward_tap(x, s) for s in stages]
        eng.close()
    first = results[codes[0]]
    for code, r in results.items():
        for a, b, what in zip(r, first, ['logits'] + stages):
            assert np.array_equal(a, b), (dtype, code, what)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_basic_engine_batch_split_is_identical(hip_lib, dtype):
    from workoutdetector_amd.engine import create_model
    eng = create_model(num_class=12, base_model='resnet18', max_clips=32, dtype=dtype)
    x = make_input(21, 32, 8, 224, 224)
    whole = eng.run(None, {'input': x})[0]
    parts = np.concatenate([eng.run(None, {'input': x[:7]})[0], eng.run(None, {'input': x[7:]})[0]])
    assert np.array_equal(whole, parts)
    eng.close()


def test_basic_onnx_export_runs_on_the_engine(hip_lib, tmp_path):
    from tests._torch_tsm import LitWrapper, TorchTSM, export_onnx
    from workoutdetector_amd.engine import create_model
    sd = _sd('resnet18', 6)
    net = TorchTSM('resnet18').load_engine_state_dict(sd)
    path = str(tmp_path / 'tsm_r18.onnx')
    export_onnx(LitWrapper(net), path, sample_shape=(1, 8, 3, 64, 64))
    eng = create_model(num_class=12, checkpoint=path, base_model='resnet18', height=112, width=112, max_clips=2)
    x = make_input(3, 2, 8, 112, 112)
    want = tsm_oracle.forward(_torch_sd(sd), torch.from_numpy(x), 'resnet18').numpy()
    assert_close(eng.run(None, {'input': x})[0], want, rtol=1e-3, atol_scale=1e-5, what='onnx r18')
    eng.close()


def test_set_backbone_contract(hip_lib, tmp_path, monkeypatch):
    """tsm_set_backbone: 18 / 34 / 50 between tsm_create and the first tsm_set_tensor, nothing else; R50 by default;
    tune-cache lines of one backbone are never read by another."""
    from workoutdetector_amd import _lib
    lib = _lib.load()
    cfg = _lib.TsmConfig(C.sizeof(_lib.TsmConfig), 12, 8, 64, 64, 8, 1, 1, 0, _lib.DTYPE_F32)
    h = C.c_void_p()
    _lib.check(lib.tsm_create(C.byref(cfg), C.byref(h)))
    try:
        assert lib.tsm_set_backbone(h, 101) == -7 and lib.tsm_set_backbone(h, 0) == -7
        one = np.ones(64, np.float32)
        shape = (C.c_int64 * 1)(64)
        # an R50 engine knows conv3; after tsm_set_backbone(18) the name is unknown
        assert lib.tsm_set_backbone(h, 50) == 0
        assert lib.tsm_set_backbone(h, 18) == 0
        assert lib.tsm_set_tensor(h, b'base_model.layer1.0.bn3.weight', one.ctypes.data, shape, 1) == -1
        assert lib.tsm_set_backbone(h, 34) == -1                 # after the first tsm_set_tensor
    finally:
        lib.tsm_destroy(h)
    from workoutdetector_amd.engine import create_model
    cache = tmp_path / 'tune.txt'
    monkeypatch.setenv('TSM_TUNE_CACHE', str(cache))
    create_model(num_class=12, base_model='resnet18', height=64, width=64, max_clips=1).warmup([1]).close()
    lines = cache.read_text().splitlines()
    assert len(lines) == 1 and ' r18|' in lines[0]
    create_model(num_class=12, height=64, width=64, max_clips=1).warmup([1]).close()
    lines = cache.read_text().splitlines()
    assert len(lines) == 2 and not re.search(r' r\d+\|', lines[1])
