"""TSM_DTYPE_BF16 (BASELINE.json config 5: bf16 weights + activations, fp32 accumulate).

This mode is NOT claimed to meet fp32 rtol 1e-3: every activation is rounded to 8 significand bits once per
layer.  Its parity oracle is therefore the bf16-STORAGE restatement (oracle/tsm_oracle.py::tsm_forward_bf16,
conv_bn_act_bf16: weights after the BN fold and every stored activation rounded exactly where the engine rounds, fp32
accumulate): per conv op the stored value must be a correct bf16 rounding of the oracle's fp32 result (rtol 2^-8 =
3.9e-3, tests/_util.py::assert_bf16_op), logits within 1e-2 of the logit scale with the same arg-max.  The distance
to the fp32 oracle is printed (-s) as the mode's accuracy figure, not asserted as parity."""
import numpy as np
import pytest
import torch

from oracle import tsm_oracle
from tests._guard import guarded_conv
from tests._util import (BF16_TAP_BAR, assert_bf16_op, assert_close, assert_fused_slots, assert_not_ran, assert_ran, assert_ran_tile, bf16_logits_report,
                         make_input, ran_tile)
from tests.test_ops_gpu import CONV_CASES, _bn, _nchw, _nhwc

pytestmark = pytest.mark.gpu

BF16_CASES = [c for c in CONV_CASES if c[3] % 64 == 0 or c[5] == 7]


@pytest.mark.parametrize('n,hi,wi,cin,cout,k,stride,relu,use_res,shiftT', BF16_CASES)
def test_conv_bn_act_bf16(hip_lib, n, hi, wi, cin, cout, k, stride, relu, use_res, shiftT):
    g = torch.Generator().manual_seed(1000 + cin + cout + k + hi)
    x = torch.randn(n, cin, hi, wi, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    bn = _bn(cout, g)
    pad = k // 2
    ho, wo = (hi + 2 * pad - k) // stride + 1, (wi + 2 * pad - k) // stride + 1
    res = torch.randn(n, cout, ho, wo, generator=g) if use_res else None
    xin = tsm_oracle.temporal_shift(x, shiftT, 8) if shiftT else x
    want = tsm_oracle.conv_bn_act_bf16(xin, w, bn, stride, pad, relu, res)
    got = guarded_conv(_nhwc(x).cuda(), w.cuda(), *[b.cuda() for b in bn], stride=stride, relu=relu,
                       residual=None if res is None else _nhwc(res).cuda(), shift_segments=shiftT, fold_div=8,
                       dtype='bf16')
    assert_bf16_op(_nchw(got.cpu()).numpy(), want.numpy(), what='conv bf16')


def test_config5_shape_t16_256(hip_lib, sd0, capsys):
    """T=16, 256x256, bf16: the stress configuration's shape (batch 2 here; batch 64 x 8 GPUs in BASELINE)."""
    from workoutdetector_amd.engine import TsmEngine
    x = make_input(55, 2, 16, 256, 256)
    want = tsm_oracle.tsm_forward(sd0, torch.from_numpy(x), n_segment=16).numpy()
    want_bf16 = tsm_oracle.tsm_forward_bf16(sd0, torch.from_numpy(x), n_segment=16).numpy()
    eng = TsmEngine(num_segments=16, height=256, width=256, max_clips=2, state_dict=sd0, dtype='bf16')
    got = eng.run(None, {'input': x})[0]
    eng.close()
    bf16_logits_report(got, want_bf16, want, 'bf16 T=16 256^2', capsys)
    # the same shape in the exact-fp32 engine meets the fp32 bar
    f32 = TsmEngine(num_segments=16, height=256, width=256, max_clips=2, state_dict=sd0)
    assert_close(f32.run(None, {'input': x})[0], want, rtol=1e-3, atol_scale=1e-5, what='f32 T=16 256^2')
    f32.close()


def test_bf16_engine_224_taps_and_packed_input(hip_lib, sd0, capsys):
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import TsmEngine, preprocess_frames
    from tests._stub import synthetic_video
    from oracle import transform_oracle
    eng = TsmEngine(max_clips=2, state_dict=sd0, dtype='bf16')
    x = make_input(100, 2, 8, 224, 224)
    taps = {}
    want = tsm_oracle.tsm_forward(sd0, torch.from_numpy(x)).numpy()
    want_bf16 = tsm_oracle.tsm_forward_bf16(sd0, torch.from_numpy(x), taps=taps).numpy()
    got = eng.run(None, {'input': x})[0]
    bf16_logits_report(got, want_bf16, want, 'bf16 224', capsys)
    # Stage taps against the bf16-storage oracle.  The stem is one conv deep: every element must be the oracle's value
    # or its bf16 neighbour (a boundary flip).  Deeper taps: a flipped input moves each of its ~600 consumers by a tenth
    # of an ulp, so flips breed flips and the two roundings of the SAME network drift apart like a random walk in
    # units of ulps -- the bar there is the worst element's distance in units of the tap's scale, and it is reported.
    t = taps['stem'].permute(0, 2, 3, 1).numpy()
    g = eng.forward_tap(x, 'stem')
    assert not (np.abs(g - t) > 2.0 ** -7 * np.abs(t) + 1e-5 * float(np.abs(t).max())).any(), 'stem'
    for stage in ['layer1.0', 'layer2.0', 'layer3.0', 'layer4.2']:
        t = taps[stage].permute(0, 2, 3, 1).numpy()
        e = float(np.abs(eng.forward_tap(x, stage) - t).max()) / float(np.abs(t).max())
        with capsys.disabled():
            print(f'[bf16 224] {stage}: max|err|/scale = {e:.3g} vs the bf16-storage oracle')
        assert e <= BF16_TAP_BAR, stage
    vid = torch.from_numpy(synthetic_video(3, 16, 120, 90))
    packed = preprocess_frames(vid.cuda(), layout=eng.packed_layout, scale_255=True)
    assert eng.packed_layout == _lib.LAYOUT_NTHWC8B and tuple(packed.shape) == (16, 224, 112, 4)
    a = eng.forward_device(packed.reshape(2, 8, 224, 112, 4), layout=_lib.LAYOUT_NTHWC8B).cpu().numpy()
    ref_in = transform_oracle.test_transform(vid.permute(0, 3, 1, 2).float(), scale_255=True).reshape(2, 8, 3, 224, 224)
    b = eng.run(None, {'input': ref_in.numpy()})[0]
    assert float(np.abs(a - b).max()) <= 2e-2 * float(np.abs(b).max())
    eng.close()


@pytest.mark.parametrize('dtype', ['bf16', 'bf16x3'])
def test_tile_choice_is_bitwise_neutral_in_bf16_modes(hip_lib, sd0, monkeypatch, dtype):
    """bf16 / split-bf16 engines: tuned, heuristic and forced tilings give bit-identical logits -- the k order of every output is tile-independent."""
    from workoutdetector_amd.engine import TsmEngine, launch_trace
    x = make_input(22, 3, 8, 96, 96)
    outs = {}
    for name, env in [('tuned', {}), ('heuristic', {'TSM_AUTOTUNE': '0'}),
                      ('64x64', {'TSM_AUTOTUNE': '0', 'TSM_CONV_TILE': '64x64'}),
                      ('128x128', {'TSM_AUTOTUNE': '0', 'TSM_CONV_TILE': '128x128'}),
                      ('128x128w8', {'TSM_AUTOTUNE': '0', 'TSM_CONV_TILE': '128x128w8'}),
                      # the 8-wave LDS-DMA kernel wherever it applies (bf16, Cout % 256 == 0): every conv3 (residual
                      # arm; K-concatenated downsample arm in the first block of a stage), conv2 / conv1 of layer3-4
                      ('256x256', {'TSM_AUTOTUNE': '0', 'TSM_CONV_TILE': '256x256'}),
                      # ... and its persistent form (same arms incl. the K-concatenated downsample one; K >= 128, Cout <= 2048)
                      ('256x256p', {'TSM_AUTOTUNE': '0', 'TSM_CONV_TILE': '256x256p'}),
                      # the weight-stationary 3x3 kernel where it applies (bf16, 64 -> 64 channels: conv2 of layer1)
                      ('ws', {'TSM_AUTOTUNE': '0', 'TSM_CONV_TILE': 'ws'})]:
        for k in ('TSM_AUTOTUNE', 'TSM_CONV_TILE'):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng = TsmEngine(height=96, width=96, max_clips=3, state_dict=sd0, dtype=dtype)
        with launch_trace() as tr:
            outs[name] = eng.run(None, {'input': x})[0]
        eng.close()
        if name in ('64x64', '128x128', '128x128w8'):
            assert_ran_tile(tr, name, f'{dtype} engine forced onto {name}')
        elif name in ('256x256', '256x256p', 'ws'):      # bf16-only kernels: split-bf16 must fall back to the heuristic tiles
            assert ran_tile(tr, name) == (dtype == 'bf16'), (name, dtype, sorted(set(tr.kernels)))
    for name in outs:
        assert np.array_equal(outs['tuned'], outs[name]), name


@pytest.mark.parametrize('dtype', ['bf16', 'bf16x3'])
@pytest.mark.parametrize('n,hi,wi', [(2, 32, 32), (3, 45, 37), (4, 96, 96), (2, 224, 224), (1, 70, 250), (17, 40, 34)])
def test_direct_stem_equals_the_generic_kernel_bitwise(hip_lib, monkeypatch, dtype, n, hi, wi):
    """The dedicated stem of the bf16 formats (direct conv from an LDS-resident pixel-pair patch, persistent workgroups)
    against the generic implicit-GEMM kernel on the same packed weights: same K order per output -> same bits,
    including ragged tiles (sizes that are not multiples of the 8x16 tile), odd widths and more tiles than workgroups."""
    from workoutdetector_amd.engine import launch_trace
    g = torch.Generator().manual_seed(500 + hi + wi)
    x = _nhwc(torch.randn(n, 3, hi, wi, generator=g)).cuda()
    w = (torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5).cuda()
    bn = [b.cuda() for b in _bn(64, g)]
    outs = {}
    for flag in ('1', '0'):
        monkeypatch.setenv('TSM_STEM_DIRECT', flag)
        for relu in (True, False):
            with launch_trace() as tr:
                outs[flag, relu] = guarded_conv(x, w, *bn, stride=2, relu=relu, dtype=dtype).cpu()
            assert tr.ran('stem_direct_kernel<') == (flag == '1') and tr.ran('conv_igemm<') == (flag == '0'), tr.kernels
    for relu in (True, False):
        assert torch.equal(outs['1', relu], outs['0', relu]), relu


@pytest.mark.parametrize('dtype', ['bf16', 'bf16x3', 'f32'])
@pytest.mark.parametrize('h,w', [(224, 224), (96, 96), (64, 96), (90, 70), (256, 256)])
def test_fused_stem_maxpool_equals_separate_kernels_bitwise(hip_lib, sd0, monkeypatch, dtype, h, w):
    """Stem + max-pool in one kernel (7x8 pooled tiles over 15x17 conv tiles, -inf outside the image, the maximum taken
    over the values the format would have stored) against the two separate kernels, through the engine: the pooled
    'stem' tap and the logits must agree bit for bit, on sizes with ragged pooled tiles too."""
    from workoutdetector_amd.engine import TsmEngine, launch_trace
    x = make_input(70 + h, 2, 8, h, w)
    got = {}
    for flag in ('1', '0'):
        monkeypatch.setenv('TSM_STEM_POOL', flag)
        eng = TsmEngine(height=h, width=w, max_clips=2, state_dict=sd0, dtype=dtype)
        with launch_trace() as tr:
            stem_tap, logits = eng.forward_tap(x, 'stem'), eng.run(None, {'input': x})[0]
        fused_ran = tr.count('stem_pool_kernel<') + tr.count('stem_pool_f32_kernel<')
        # (fused: the tap, the tuning pass of the first forward and the forward itself)
        assert (fused_ran >= 2 if flag == '1' else fused_ran == 0) and tr.ran('maxpool3x3s2_kernel') == (flag == '0'), tr.kernels
        with launch_trace() as tr:
            got[flag] = (stem_tap, logits, eng.forward_tap(x, 'conv1'))
        assert not tr.ran('stem_pool'), tr.kernels       # the un-pooled tap comes from the un-fused kernel either way
        eng.close()
    assert np.array_equal(got['1'][0], got['0'][0]) and np.array_equal(got['1'][1], got['0'][1])
    assert np.array_equal(got['1'][2], got['0'][2])        # the un-pooled tap still comes from the un-fused kernel
    assert got['1'][0].shape == (16, (h // 2 + 1) // 2, (w // 2 + 1) // 2, 64)


@pytest.mark.parametrize('dtype', ['bf16', 'bf16x3', 'f32'])
@pytest.mark.parametrize('h,w,b', [(224, 224, 2), (256, 256, 3), (90, 70, 2), (91, 75, 2), (33, 47, 5), (64, 97, 2)])
def test_stem_reading_the_reference_layout_equals_the_packed_input_bitwise(hip_lib, sd0, monkeypatch, dtype, h, w, b):
    """The pool-fused stem fed with the reference layout itself ([N, T, 3, H, W] fp32: it rounds / splits while staging its
    patch, no pack launch) against the same stem behind pack_input_kernel (TSM_STEM_PLANAR=0): the pooled 'stem' tap and
    the logits agree bit for bit -- even and odd widths (an odd width ends a row in half a pixel pair), ragged tiles."""
    from workoutdetector_amd.engine import TsmEngine, launch_trace
    x = make_input(170 + h + w, b, 8, h, w)
    got = {}
    for flag in ('1', '0'):
        monkeypatch.setenv('TSM_STEM_PLANAR', flag)
        eng = TsmEngine(height=h, width=w, max_clips=b, state_dict=sd0, dtype=dtype)
        with launch_trace() as tr:
            got[flag] = (eng.forward_tap(x, 'stem'), eng.run(None, {'input': x})[0])
        eng.close()
        # '1': the stem's PLANAR instantiation reads [N, T, 3, H, W] itself, no pack launch; '0': pack launch + packed stem
        planar = [k for k in tr.kernels if k in ('stem_pool_f32_kernel<true>', 'stem_pool_kernel<false, true>', 'stem_pool_kernel<true, true>')]
        stems = tr.count('stem_pool')       # the tap, the tuning pass of the first forward, the forward itself
        assert stems >= 2 and len(planar) == (stems if flag == '1' else 0), (flag, tr.kernels)
        assert tr.ran('pack_input_kernel') == (flag == '0'), (flag, tr.kernels)
    assert np.array_equal(got['1'][0], got['0'][0]) and np.array_equal(got['1'][1], got['0'][1])
    assert np.isfinite(got['1'][1]).all() and np.abs(got['1'][0]).max() > 0


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
def test_a_reference_layout_tensor_that_is_only_4_byte_aligned_gives_the_same_logits(hip_lib, sd0, dtype):
    """The fp32-reading stem loads pixel pairs with 8-byte loads: a device pointer that is not 16-byte aligned (a view one
    float into a larger buffer) takes the pack launch instead -- same bits either way."""
    from workoutdetector_amd.engine import TsmEngine
    x = torch.from_numpy(make_input(77, 2, 8, 64, 64)).cuda()
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device='cuda')
    xm = buf[1:].view_as(x)
    xm.copy_(x)
    assert xm.data_ptr() % 16 == 4 and xm.is_contiguous()
    eng = TsmEngine(height=64, width=64, max_clips=2, state_dict=sd0, dtype=dtype)
    a, b = eng.forward_device(x).cpu(), eng.forward_device(xm).cpu()
    eng.close()
    assert torch.equal(a, b) and torch.isfinite(a).all()


@pytest.mark.parametrize('n,hi,wi,cin,cout,k,stride,relu,shiftT,use_res', [
    (8, 16, 16, 256, 256, 3, 1, True, 0, False),   # layer3 conv2 at the config-5 size: 2048 rows = 8 full tiles
    (4, 16, 16, 256, 256, 3, 2, True, 0, False),   # stride 2 (layer3.0 / layer4.0 conv2): 256 rows
    (3, 7, 9, 512, 512, 3, 1, False, 0, False),    # ragged: 189 rows in one tile, two n-tiles, K = 4608 (72 K-tiles)
    (8, 14, 14, 1024, 256, 1, 1, True, 8, False),  # layer3 conv1 with the fused temporal shift, 1568 rows (ragged last tile)
    (4, 8, 8, 2048, 512, 1, 1, True, 4, False),    # layer4 conv1, T = 4
    (2, 20, 20, 64, 256, 1, 1, True, 0, False),    # a single K-tile (K = 64): prologue + dead stages only
    (2, 12, 12, 64, 256, 3, 1, True, 0, False),    # K = 576 = 9 K-tiles (odd count)
    (4, 16, 16, 256, 1024, 1, 1, True, 0, True),   # layer3 conv3 + residual: four n-tiles
    (3, 9, 7, 128, 512, 1, 1, True, 0, True),      # layer2 conv3 + residual, ragged (189 rows), K = 128
    (2, 8, 8, 512, 2048, 1, 1, False, 0, True),    # layer4 conv3 + residual, no ReLU
    (96, 16, 16, 256, 1024, 1, 1, True, 0, True),  # 384 tiles on 256 workgroups: the persistent form's second tile, ragged tail of the grid
    (40, 14, 14, 256, 256, 3, 1, True, 0, False),  # 3x3, 31 m-tiles (ragged last one) x 1: fewer tiles than workgroups
    (208, 16, 16, 128, 512, 1, 1, True, 0, True),  # K = 128 (two K-tiles: every refill of a tile's last K-tile is the NEXT tile's), 416 tiles
    (72, 16, 16, 1024, 256, 1, 1, True, 8, False), # shifted conv1, 72 tiles; clips of 8 frames cross tile boundaries
    (200, 12, 12, 128, 256, 3, 1, False, 0, False),# 3x3, K = 1152, 113 m-tiles, no ReLU
    (300, 16, 16, 64, 256, 3, 1, True, 0, False),  # 300 tiles (K = 576: odd K-tile count -> the buffer parity flips from tile to tile)
])
def test_lds_dma_256_tile_equals_the_128_tiles_bitwise(hip_lib, monkeypatch, n, hi, wi, cin, cout, k, stride, relu, shiftT,
                                                       use_res):
    """conv_bf16_256_kernel (256 x 256 tile, 8 waves, LDS-DMA staging, counted vmcnt) and its persistent form
    conv_bf16_256p_kernel (flat K pipeline across a workgroup's tiles, transposed product, register epilogue) against
    conv_igemm's bf16 tiles through the per-op entry point: same k order per output -> same bits; and against the
    bf16-storage oracle at the bf16 mode's per-op bar."""
    from workoutdetector_amd.engine import launch_trace
    g = torch.Generator().manual_seed(7000 + cin + cout + k + hi)
    x = torch.randn(n, cin, hi, wi, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    bn = _bn(cout, g)
    pad = k // 2
    ho, wo = (hi + 2 * pad - k) // stride + 1, (wi + 2 * pad - k) // stride + 1
    res = torch.randn(n, cout, ho, wo, generator=g) if use_res else None
    outs = {}
    persistent = cin * k * k >= 128        # conv_bf16_256p_kernel needs two K-tiles per tile
    for tile in ('256x256', '128x128', '64x64') + (('256x256p',) if persistent else ()):
        monkeypatch.setenv('TSM_CONV_TILE', tile)
        with launch_trace() as tr:
            outs[tile] = guarded_conv(_nhwc(x).cuda(), w.cuda(), *[b.cuda() for b in bn], stride=stride, relu=relu,
                                      residual=None if res is None else _nhwc(res).cuda(),
                                      shift_segments=shiftT, fold_div=8, dtype='bf16').cpu()
        assert_ran_tile(tr, tile, f'per-op conv forced onto {tile}')
    assert torch.equal(outs['256x256'], outs['128x128']) and torch.equal(outs['256x256'], outs['64x64'])
    if persistent:      # the same pipeline run persistently over a workgroup's tiles, register epilogue
        assert torch.equal(outs['256x256p'], outs['256x256'])
    xin = tsm_oracle.temporal_shift(x, shiftT, 8) if shiftT else x
    want = tsm_oracle.conv_bn_act_bf16(xin, w, bn, stride, k // 2, relu, res)
    assert_bf16_op(_nchw(outs['256x256']).numpy(), want.numpy(), what='256x256 bf16')


@pytest.mark.parametrize('ch,n,hi,wi,relu', [
    (64, 16, 64, 64, True),     # layer1 at the config-5 size: 16 x 16 tiles, 256 tiles = one per workgroup
    (64, 40, 64, 64, True),     # 640 tiles: 2.5 per workgroup (double-buffered patches, ragged persistent tail)
    (64, 8, 56, 56, True),      # layer1 at 224^2: 4 x 56 tiles (224 of 256 lanes used), 112 tiles
    (64, 3, 23, 18, False),     # ragged in both directions, no ReLU
    (64, 5, 7, 5, True),        # a frame smaller than one tile
    (64, 2, 130, 9, True),      # narrow and tall
    (64, 1, 3, 200, True),      # wider than any tile: several tiles per row, frame shorter than a tile
    (64, 300, 8, 8, True),      # more frames than workgroups, one tile each
    (128, 16, 32, 32, True),    # layer2 at the config-5 size: 8 x 16 tiles, 8 per frame
    (128, 80, 32, 32, True),    # 640 tiles: 2.5 per workgroup
    (128, 8, 28, 28, True),     # layer2 at 224^2: 4 x 28 tiles
    (128, 3, 23, 18, False),    # ragged, no ReLU
    (128, 5, 7, 5, True),       # a frame smaller than one tile
    (128, 1, 3, 200, True),     # several tiles per row
    (128, 300, 8, 8, True),     # more frames than workgroups
])
def test_weight_stationary_3x3_equals_the_igemm_tiles_bitwise(hip_lib, monkeypatch, ch, n, hi, wi, relu):
    """conv3x3_ws_kernel / conv3x3_ws128_kernel (weights resident in registers -- all of W2 per wave for 64 channels, a
    32-output-channel slice per wave for 128 --, input patch by LDS-DMA, transposed MFMA, register epilogue through
    v_permlane32_swap) against conv_igemm's bf16 tiles through the per-op entry point: same k order per output -> same
    bits; and against the fp32 oracle at the bf16 mode's tolerance."""
    from workoutdetector_amd.engine import launch_trace
    g = torch.Generator().manual_seed(9100 + ch + n + hi + wi)
    x = torch.randn(n, ch, hi, wi, generator=g)
    w = torch.randn(ch, ch, 3, 3, generator=g) * (2.0 / (9 * ch)) ** 0.5
    bn = _bn(ch, g)
    outs = {}
    for tile in ('ws', '128x64', '64x64'):
        monkeypatch.setenv('TSM_CONV_TILE', tile)
        with launch_trace() as tr:
            outs[tile] = guarded_conv(_nhwc(x).cuda(), w.cuda(), *[b.cuda() for b in bn], stride=1, relu=relu, dtype='bf16').cpu()
        if tile == 'ws':
            assert_ran(tr, 'conv3x3_ws_kernel<false>' if ch == 64 else 'conv3x3_ws128_kernel<false>', 'weight-stationary 3x3')
        else:
            assert_ran_tile(tr, tile)
    assert torch.equal(outs['64x64'], outs['128x64'])
    assert torch.equal(outs['ws'], outs['64x64'])
    if n * hi * wi <= 70000:
        want = tsm_oracle.conv_bn_act_bf16(x, w, bn, 1, 1, relu, None)
        assert_bf16_op(_nchw(outs['ws']).numpy(), want.numpy(), what='ws bf16')


@pytest.mark.parametrize('n,hi,wi,relu', [
    (16, 64, 64, True),      # layer2.0.conv2 at the config-5 size: 32 x 32 outputs, 8 x 8 tiles (17 x 17 patch: the one-pixel tenth DMA round), 256 tiles
    (80, 64, 64, True),      # 1280 tiles: five per workgroup, both accumulator sets end a workgroup's run
    (48, 64, 64, True),      # 768 tiles: three per workgroup (odd count: the other set ends the run)
    (8, 56, 56, True),       # at 224^2: 28 x 28 outputs, 4 x 14 tiles on 16 lanes per row
    (3, 23, 18, False),      # odd input sizes (the last output column's right tap is padding), ragged tiles, no ReLU
    (5, 7, 5, True),         # a frame smaller than one tile
    (2, 33, 31, True),       # 17 x 16 outputs
    (1, 3, 200, True),       # one tile row, 100 outputs across
    (2, 130, 9, True),       # narrow and tall: tiles of 5 columns on 8 lanes per row
    (300, 8, 8, True),       # more frames than workgroups: 4 x 4 outputs
    (4, 16, 96, True),       # tiles wider than 32 outputs cannot hold two rows: geometry search over all lane layouts
])
def test_weight_stationary_3x3_stride2_equals_the_igemm_tiles_bitwise(hip_lib, monkeypatch, n, hi, wi, relu):
    """conv3x3_ws128_kernel<true> (layer2.0's conv2: stride 2, 128 -> 128 channels; the patch stored with de-interleaved
    columns, one M-tile pair per tile, the accumulator sets alternating between tiles) against conv_igemm's bf16 tiles
    through the per-op entry point: same bits; and against the oracle at the bf16 mode's tolerance."""
    from workoutdetector_amd.engine import launch_trace
    g = torch.Generator().manual_seed(9300 + n + hi + wi)
    x = torch.randn(n, 128, hi, wi, generator=g)
    w = torch.randn(128, 128, 3, 3, generator=g) * (2.0 / (9 * 128)) ** 0.5
    bn = _bn(128, g)
    outs = {}
    for tile in ('ws', '128x128', '64x64'):
        monkeypatch.setenv('TSM_CONV_TILE', tile)
        with launch_trace() as tr:
            outs[tile] = guarded_conv(_nhwc(x).cuda(), w.cuda(), *[b.cuda() for b in bn], stride=2, relu=relu, dtype='bf16').cpu()
        if tile == 'ws':
            assert_ran(tr, 'conv3x3_ws128_kernel<true>', 'stride-2 weight-stationary 3x3')
        else:
            assert_ran_tile(tr, tile)
    assert outs['ws'].shape == (n, (hi - 1) // 2 + 1, (wi - 1) // 2 + 1, 128)
    assert torch.equal(outs['64x64'], outs['128x128'])
    assert torch.equal(outs['ws'], outs['64x64'])
    if n * hi * wi <= 70000:
        want = tsm_oracle.conv_bn_act_bf16(x, w, bn, 2, 1, relu, None)
        assert_bf16_op(_nchw(outs['ws']).numpy(), want.numpy(), what='ws stride 2 bf16')


@pytest.mark.parametrize('cin,n,hi,wi,shiftT,relu', [
    (256, 16, 64, 64, 16, True),   # layer1.1 / 1.2 conv1 at the config-5 size (one clip): 512 tiles, shift over 16 frames
    (256, 32, 56, 56, 8, True),    # at 224^2, four clips: 784 tiles (3 per workgroup), tiles straddle frames (3136 rows per frame)
    (64, 16, 64, 64, 16, True),    # layer1.0 conv1 (stem output, 64 channels): fold = 8
    (64, 24, 23, 18, 8, False),    # ragged last tile, no ReLU
    (256, 9, 7, 5, 3, True),       # frames smaller than a tile: a tile spans several frames of several clips
    (256, 5, 20, 20, 0, True),     # no shift at all
    (64, 700, 8, 8, 7, True),      # more tiles than workgroups, odd segment count
])
def test_weight_stationary_1x1_equals_the_igemm_tiles_bitwise(hip_lib, monkeypatch, cin, n, hi, wi, shiftT, relu):
    """conv1x1_ws_kernel (layer1's conv1: W1 resident in registers, a whole 128-pixel tile by LDS-DMA one tile ahead, the
    temporal shift as an address choice per 16-byte chunk, zeros at the clip's ends) against conv_igemm's bf16 tiles
    through the per-op entry point -- same bits -- and against the fp32 oracle at the bf16 mode's tolerance."""
    from workoutdetector_amd.engine import launch_trace
    g = torch.Generator().manual_seed(9300 + cin + n + hi)
    x = torch.randn(n, cin, hi, wi, generator=g)
    w = torch.randn(64, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5
    bn = _bn(64, g)
    outs = {}
    for tile in ('ws', '128x64', '64x64'):
        monkeypatch.setenv('TSM_CONV_TILE', tile)
        with launch_trace() as tr:
            outs[tile] = guarded_conv(_nhwc(x).cuda(), w.cuda(), *[b.cuda() for b in bn], stride=1, relu=relu,
                                      shift_segments=shiftT, fold_div=8, dtype='bf16').cpu()
        if tile == 'ws':
            assert_ran(tr, 'conv1x1_ws_kernel<%d>' % cin, 'weight-stationary 1x1')
        else:
            assert_ran_tile(tr, tile)
    assert torch.equal(outs['64x64'], outs['128x64'])
    assert torch.equal(outs['ws'], outs['64x64'])
    xin = tsm_oracle.temporal_shift(x, shiftT, 8) if shiftT else x
    want = tsm_oracle.conv_bn_act_bf16(xin, w, bn, 1, 0, relu, None)
    assert_bf16_op(_nchw(outs['ws']).numpy(), want.numpy(), what='ws 1x1 bf16')


@pytest.mark.parametrize('cin,cout,n,hi,wi,shiftT,relu', [
    (256, 128, 16, 64, 64, 16, True),   # layer2.0 conv1 at the config-5 size (one clip)
    (512, 128, 16, 32, 32, 16, True),   # layer2.x conv1: 64-pixel tiles
    (512, 256, 16, 32, 32, 16, True),   # layer3.0 conv1: 64 weight fragments per wave (accumulation registers)
    (256, 128, 24, 23, 18, 8, False),   # ragged last tile, no ReLU
    (512, 128, 9, 7, 5, 3, True),       # frames smaller than a tile
    (512, 256, 5, 20, 20, 0, True),     # no shift
    (256, 128, 700, 4, 4, 7, True),     # more tiles than workgroups, odd segment count
])
def test_weight_stationary_1x1_wide_equals_the_igemm_tiles_bitwise(hip_lib, monkeypatch, cin, cout, n, hi, wi, shiftT, relu):
    """conv1x1_wsn_kernel (output channels split over the waves, whole pixel tiles by LDS-DMA one tile ahead, fused temporal
    shift) against conv_igemm's bf16 tiles through the per-op entry point -- same bits -- and against the fp32 oracle."""
    from workoutdetector_amd.engine import launch_trace
    g = torch.Generator().manual_seed(9500 + cin + cout + n + hi)
    x = torch.randn(n, cin, hi, wi, generator=g)
    w = torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5
    bn = _bn(cout, g)
    outs = {}
    for tile in ('ws', '128x128', '64x64'):
        monkeypatch.setenv('TSM_CONV_TILE', tile)
        with launch_trace() as tr:
            outs[tile] = guarded_conv(_nhwc(x).cuda(), w.cuda(), *[b.cuda() for b in bn], stride=1, relu=relu,
                                      shift_segments=shiftT, fold_div=8, dtype='bf16').cpu()
        if tile == 'ws':
            assert_ran(tr, 'conv1x1_wsn_kernel<%d, %d, false>' % (cin, cout), 'wide weight-stationary 1x1')
        else:
            assert_ran_tile(tr, tile)
    assert torch.equal(outs['64x64'], outs['128x128'])
    assert torch.equal(outs['ws'], outs['64x64'])
    xin = tsm_oracle.temporal_shift(x, shiftT, 8) if shiftT else x
    want = tsm_oracle.conv_bn_act_bf16(xin, w, bn, 1, 0, relu, None)
    assert_bf16_op(_nchw(outs['ws']).numpy(), want.numpy(), what='wsn 1x1 bf16')


@pytest.mark.parametrize('h,w,b', [(256, 256, 2), (224, 224, 2), (90, 70, 3)])
def test_weight_stationary_kernels_forced_everywhere_equal_the_igemm_engine_bitwise(hip_lib, sd0, monkeypatch, h, w, b):
    """An engine with TSM_CONV_TILE=ws (every layer that has a weight-stationary form runs it: conv1 / conv2 of layer1,
    conv3 + downsample of layer1.0 and of layer2.0 as the K-concatenated GEMM, conv1 / conv2 of layer2, conv1 of layer3.0) against one
    forced onto the 64x64 tile: block outputs and logits bit for bit."""
    from workoutdetector_amd.engine import TsmEngine, launch_trace
    x = make_input(300 + h, b, 8, h, w)
    got = {}
    for tile in ('ws', '64x64'):
        monkeypatch.setenv('TSM_AUTOTUNE', '0')
        monkeypatch.setenv('TSM_CONV_TILE', tile)
        monkeypatch.setenv('TSM_FUSE_CONV23', '0')
        eng = TsmEngine(height=h, width=w, max_clips=b, state_dict=sd0, dtype='bf16')
        with launch_trace() as tr:
            got[tile] = [eng.forward_tap(x, s) for s in ('layer1.0', 'layer1.2', 'layer2.0', 'layer2.3', 'layer3.0')] + \
                        [eng.run(None, {'input': x})[0]]
        eng.close()
        ws_families = ('conv3x3_ws_kernel<false>', 'conv3x3_ws128_kernel<false>', 'conv3x3_ws128_kernel<true>', 'conv1x1_ws_kernel<64>',
                       'conv1x1_ws_kernel<256>', 'conv1x1_wsn_kernel<128, 256, true>', 'conv1x1_wsn_kernel<256, 128, false>',
                       'conv1x1_wsn_kernel<512, 128, false>', 'conv1x1_wsn_kernel<512, 256, false>',
                       'conv1x1_wsn_kernel<384, 256, true, 2>')     # (conv3 + downsample of layer2.0: two output-channel halves on workgroup pairs)
        for fam in ws_families:      # every weight-stationary form has a layer of ResNet-50 it applies to
            assert tr.ran(fam) == (tile == 'ws'), (tile, fam, sorted(set(tr.kernels)))
    for a, c in zip(got['ws'], got['64x64']):
        assert np.array_equal(a, c)


def _random_ws_cases():
    """Seeded random shapes for the weight-stationary kernels: (kind, cin, cout, n, h, w, T)."""
    rng = np.random.default_rng(20260)
    cases = []
    for _ in range(6):
        cases.append(('3x3', 64, 64, int(rng.integers(1, 40)), int(rng.integers(3, 70)), int(rng.integers(3, 70)), 0))
        cases.append(('3x3', 128, 128, int(rng.integers(1, 40)), int(rng.integers(3, 40)), int(rng.integers(3, 40)), 0))
        t = int(rng.choice([0, 2, 3, 4, 8]))
        cin, cout = [(64, 64), (256, 64), (256, 128), (512, 128), (512, 256)][int(rng.integers(0, 5))]
        cases.append(('1x1', cin, cout, max(t, 1) * int(rng.integers(1, 6)), int(rng.integers(2, 40)), int(rng.integers(2, 40)), t))
    return cases


@pytest.mark.parametrize('kind,cin,cout,n,hi,wi,shiftT', _random_ws_cases())
def test_weight_stationary_kernels_on_random_shapes_bitwise(hip_lib, monkeypatch, kind, cin, cout, n, hi, wi, shiftT):
    """Seeded random frame counts / sizes / segment counts (ragged tiles, tiles straddling frames and clips, frames
    smaller than a tile) through every weight-stationary kernel family, bit-compared with the 64x64 igemm tile."""
    from workoutdetector_amd.engine import launch_trace
    k = 3 if kind == '3x3' else 1
    g = torch.Generator().manual_seed(n * 1000 + hi * 10 + wi + cin)
    x = torch.randn(n, cin, hi, wi, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    bn = _bn(cout, g)
    outs = {}
    for tile in ('ws', '64x64'):
        monkeypatch.setenv('TSM_CONV_TILE', tile)
        with launch_trace() as tr:
            outs[tile] = guarded_conv(_nhwc(x).cuda(), w.cuda(), *[b.cuda() for b in bn], stride=1, relu=True,
                                      shift_segments=shiftT, fold_div=8, dtype='bf16').cpu()
        assert_ran_tile(tr, tile, f'{kind} {cin}->{cout} n={n} {hi}x{wi} T={shiftT}')
    assert torch.equal(outs['ws'], outs['64x64'])


@pytest.mark.parametrize('h,w,b,t,div,shift', [
    (256, 256, 2, 16, 8, True),    # the config-5 geometry: 64 x 64 frames at layer1, 33 steps per frame, T = 16
    (224, 224, 2, 8, 8, True),     # the headline geometry: 56 x 56 (a step is 112 pixels: the fourth M-tile is half empty)
    (90, 70, 3, 8, 8, True),       # 23 x 18: odd height (last step has one live row), M-tiles straddle the two rows
    (64, 96, 4, 4, 8, True),       # 16 x 24 frames, T = 4: 16 frames over 16 workgroups
    (72, 40, 3, 3, 8, True),       # 18 x 10 frames, odd segment count: more frames than some workgroups' share
    (224, 224, 1, 8, 8, False),    # no temporal shift at all (FOLDG = 0)
    (40, 250, 2, 8, 8, True),      # 10 x 63: the widest row the line buffer takes but one
    (270, 480, 1, 8, 8, True),     # 68 x 120: too wide for the line buffer -- the forced switch must fall back, same bits
    (32, 32, 5, 1, 8, True),       # the smallest engine: 8 x 8 frames, single-frame clips (both shifted groups read zeros)
    (250, 256, 1, 4, 8, True),     # 63 x 64: the widest row with an odd height; 4 frames on 4 workgroups
    (256, 256, 1, 8, 8, False),    # 64-wide rows without the shift: all four waves take their identity from the LDS input slots
    (256, 256, 5, 1, 8, True),     # ... single-frame clips (the shifted channels are zeros, the wave that owns them still loads its identity)
    (130, 256, 3, 4, 8, True),     # ... 33 x 64 frames: odd height, 12 frames
    (32, 256, 2, 8, 8, True),      # ... 8 x 64 frames: five steps per frame, the row held across a step changes frame every fifth
])
def test_whole_bottleneck_kernel_equals_the_separate_launches_bitwise(hip_lib, monkeypatch, h, w, b, t, div, shift):
    """bneck_ws_kernel (every layer1 block in bf16 as ONE launch: shift + conv1 into an LDS line buffer, conv2 from it,
    conv3 + residual -- layer1.0: conv3 + the K-concatenated downsample branch -- from an LDS mid tile; the block input
    streamed once) against the separate launches: block outputs
    and logits bit for bit, on the BASELINE geometries, ragged sizes, with and without the shift."""
    from workoutdetector_amd.engine import TsmEngine, launch_trace
    from workoutdetector_amd.weights import make_state_dict
    sd = make_state_dict(11, 12)
    x = make_input(500 + h + t, b, t, h, w)
    got = {}
    for flag in ('1', '0'):
        monkeypatch.setenv('TSM_FUSE_BLOCK', flag)
        eng = TsmEngine(num_segments=t, height=h, width=w, shift_div=div, is_shift=shift, max_clips=b, state_dict=sd, dtype='bf16')
        with launch_trace() as tr:
            got[flag] = [eng.forward_tap(x, s) for s in ('layer1.0', 'layer1.1', 'layer1.2', 'layer2.0')] + [eng.run(None, {'input': x})[0]]
        tiles = eng.conv_tiles(b)
        wp = (((w - 1) // 2 + 1) - 1) // 2 + 1          # layer1's row length: stem (stride 2) then max-pool (stride 2)
        fits = flag == '1' and wp <= 64
        assert_fused_slots(eng, x, {f'layer1.{k}.conv{c}' for k in range(3) for c in (2, 3)} if fits else set(), flag)
        eng.close()
        assert not any(v.endswith('+block') for v in tiles.values())    # (a forced form is not a tuner choice: no code carries the bit)
        # What RAN.  Forced on, all three layer1 blocks take the whole-block kernel where the line buffer fits (frames of <= 64
        # columns: W <= 256) -- layer1.0 on the 64-channel form, layer1.1 / 1.2 on the 256-channel one (LDS identity at 64
        # columns) -- and a too-wide frame falls back; forced off, it never runs.
        sh = 'true' if shift else 'false'
        wide = f'bneck_ws_kernel<256, {sh}, true>' if wp == 64 else f'bneck_ws_kernel<256, {sh}>'
        # (taps 'layer1.0' .. 'layer2.0' run 1 + 2 + 3 + 3 blocks, the forward 3, its tuning pass none: the forced form is not timed)
        assert tr.count(f'bneck_ws_kernel<64, {sh}>') == (5 if fits else 0), sorted(set(tr.kernels))
        assert tr.count(wide) == (7 if fits else 0), sorted(set(tr.kernels))
        assert tr.ran('bneck_ws_kernel<') == fits, sorted(set(tr.kernels))
    for name, a, c in zip(('layer1.0', 'layer1.1', 'layer1.2', 'layer2.0', 'logits'), got['1'], got['0']):
        assert np.array_equal(a, c), name
    assert np.isfinite(got['1'][-1]).all()


@pytest.mark.parametrize('h,w,b,t,div,shift', [
    (256, 256, 2, 16, 8, True),    # the config-5 geometry: 32 x 32 frames at layer2, tiles of 16 frames x 16 pixels
    (224, 224, 3, 8, 8, True),     # the headline geometry: 28 x 28 = 784 pixels, tiles of 8 x 32 (the 25th tile of a clip is half empty)
    (96, 64, 5, 4, 8, True),       # 12 x 8 = 96 pixels, T = 4: tiles of 4 x 64, the second one half empty; more tiles than some workgroups' share
    (90, 70, 3, 8, 8, True),       # 12 x 9 = 108 pixels: ragged in the last tile, odd row length
    (64, 64, 3, 2, 8, True),       # T = 2: tiles of 2 x 128 pixels over 8 x 8 frames (one tile holds a whole clip)
    (224, 224, 2, 8, 8, False),    # no temporal shift: every chunk reads its own rows
    (128, 128, 2, 32, 8, True),    # T = 32: tiles of 32 frames x 8 pixels (a wave's rows are four frames of one pixel run)
    (72, 40, 3, 3, 8, True),       # odd segment count: no clip-major tile exists -- the forced switch must fall back, same bits
    (64, 96, 2, 64, 8, True),      # T = 64 > 32: not enough pixels per tile -- falls back as well
])
def test_conv3_conv1_cross_block_kernel_equals_the_separate_launches_bitwise(hip_lib, monkeypatch, h, w, b, t, div, shift):
    """conv31_fused_kernel (conv3 + residual + ReLU of layer2.k and temporal shift + conv1 of layer2.k+1 as ONE
    launch on clip-major tiles -- all T frames of a clip x 256 / T pixels, so the frames t +- 1 the shifted channels come
    from are rows of the same tile; models/tsm.py:35-50,125-137 across the Bottleneck boundary) against the two launches it
    replaces: every layer2 block output (= the kernel's y), the next block's conv1 tap (= its t1) and the logits, bit for
    bit -- BASELINE geometries, ragged tiles, T from 2 to 32, no shift, and geometries without a clip-major tile."""
    from workoutdetector_amd.engine import TsmEngine, launch_trace
    from workoutdetector_amd.weights import make_state_dict
    sd = make_state_dict(13, 12)
    x = make_input(700 + h + t, b, t, h, w)
    # (layer2.k -> k+1 on the 8-wave form; layer2.3 -> layer3.0.conv1 and layer3.k -> k+1 on the 4-wave forms, 128-row tiles)
    stages = ('layer2.0', 'layer2.1', 'layer2.2.conv1', 'layer2.2', 'layer2.3.conv1', 'layer2.3', 'layer3.0.conv1', 'layer3.0',
              'layer3.1', 'layer3.2.conv1', 'layer3.2', 'layer3.4', 'layer3.5.conv1', 'layer3.5', 'layer4.0')
    got = {}
    for flag in ('1', '0'):
        monkeypatch.setenv('TSM_FUSE_C3C1', flag)
        eng = TsmEngine(num_segments=t, height=h, width=w, shift_div=div, is_shift=shift, max_clips=b, state_dict=sd, dtype='bf16')
        with launch_trace() as tr:
            got[flag] = [eng.run(None, {'input': x})[0]] + [eng.forward_tap(x, s) for s in stages] + [eng.run(None, {'input': x})[0]]
        # (the next block's conv1 launches the forced form takes over, per instantiation below)
        taken = {256: ('layer2.2.conv1', 'layer2.3.conv1'), 128: ('layer3.0.conv1', 'layer3.2.conv1', 'layer3.3.conv1', 'layer3.4.conv1',
                                                                'layer3.5.conv1')}
        assert_fused_slots(eng, x, {n for rows, ns in taken.items() if flag == '1' and rows % t == 0 and rows // t >= 8 for n in ns}, flag)
        eng.close()
        # What RAN: forced on, every geometry with a clip-major tile runs its instantiation -- layer2.k -> k+1 (<128, 512, 128>),
        # layer2.3 -> layer3.0 (<128, 512, 256>), layer3.k -> k+1 (<256, 1024, 256>) -- and the geometries without one (odd T,
        # T = 64; T = 32 on the 128-row forms) fall back; forced off, none runs.
        # (a tile is `rows` = T frames x rows / T >= 8 pixels: 256 rows on conv31_fused_kernel, 128 on conv31_pc_kernel)
        for rows, inst in ((256, 'conv31_fused_kernel<K3, C, N1> [K3 = 128, C = 512, N1 = 128]'),
                           (128, 'conv31_pc_kernel<K3, C, N1> [K3 = 128, C = 512, N1 = 256]'),       # (producer / consumer waves)
                           (128, 'conv31_pc_kernel<K3, C, N1> [K3 = 256, C = 1024, N1 = 256]')):
            has_tile = flag == '1' and rows % t == 0 and rows // t >= 8
            assert tr.ran(inst) == has_tile, (flag, inst, sorted(set(tr.kernels)))
    for name, a, c in zip(('logits',) + stages + ('logits again',), got['1'], got['0']):
        assert np.array_equal(a, c), name
    assert np.isfinite(got['1'][0]).all() and np.array_equal(got['1'][0], got['1'][-1])


def test_tuner_may_choose_the_cross_block_kernel_and_reports_it(hip_lib, sd0):
    """At the config-5 geometry the tuner times conv3 + the next conv1 as one launch against the tuned pair (bit 4096 of
    conv3's tile code, '+conv1' in conv_tiles); whatever it picks, the logits are those of an engine that may not fuse."""
    import os
    from workoutdetector_amd.engine import TsmEngine, launch_trace
    x = make_input(77, 4, 16, 256, 256)
    eng = TsmEngine(num_segments=16, height=256, width=256, max_clips=4, state_dict=sd0, dtype='bf16')
    ya = eng.run(None, {'input': x})[0]
    with launch_trace() as tr:
        assert np.array_equal(eng.run(None, {'input': x})[0], ya)
    n31 = tr.count('conv31_fused_kernel') + tr.count('conv31_pc_kernel')
    tiles = eng.conv_tiles(4)
    eng.close()
    fused = [k for k, v in tiles.items() if v.endswith('+conv1')]
    assert all(k in ('layer2.1.conv3', 'layer2.2.conv3', 'layer2.3.conv3', 'layer3.1.conv3', 'layer3.2.conv3', 'layer3.3.conv3',
                     'layer3.4.conv3') for k in fused), fused
    # the choice is timing-based; what is asserted is that the REPORT is the truth: a forward of the tuned engine launches the
    # cross-block kernel exactly once per '+conv1' code (none when the tuner kept the pairs: the bitwise comparison below is
    # then the test of the engine's plain path, and says so)
    assert n31 == len(fused), (n31, fused)
    if not fused:
        print('\n[tuner kept the separate conv3 / conv1 launches at 4 clips of 16 x 256 x 256: the cross-block kernel is covered by the forced test only]')
    os.environ['TSM_FUSE_C3C1'] = '0'
    try:
        ref = TsmEngine(num_segments=16, height=256, width=256, max_clips=4, state_dict=sd0, dtype='bf16')
        yb = ref.run(None, {'input': x})[0]
        assert not any(v.endswith('+conv1') for v in ref.conv_tiles(4).values())
        ref.close()
    finally:
        del os.environ['TSM_FUSE_C3C1']
    assert np.array_equal(ya, yb)


@pytest.mark.parametrize('h,w,b,t,shift', [
    (256, 256, 2, 16, True),     # the config-5 geometry: 64 x 64 frames at layer2.0's input, 32 output rows of 32 pixels
    (224, 224, 2, 8, True),      # the headline geometry: 56 x 56 (a row is 56 of the slot's 64 pixels, 28 output pixels per row)
    (64, 96, 5, 4, True),        # 16 x 24 frames, T = 4: 20 frames over 20 workgroups
    (32, 256, 3, 1, True),       # 8 x 64 frames, single-frame clips (the shifted channels read zeros)
    (224, 224, 1, 8, False),     # no temporal shift
    (128, 40, 3, 3, True),       # 32 x 10 frames: narrow rows, odd segment count
    (256, 256, 9, 16, True),     # 144 frames: more than one frame per workgroup on a big chip (the row pipeline runs across frames)
    (90, 70, 2, 8, True),        # 23 x 18: odd height -- the forced switch must fall back, same bits
    (270, 480, 1, 8, True),      # 68 x 120: rows too wide for a slot -- falls back as well
])
def test_front_of_layer2_0_as_one_launch_equals_the_separate_launches_bitwise(hip_lib, monkeypatch, h, w, b, t, shift):
    """front_s2_kernel (round 5: temporal shift + conv1 + bn1 + ReLU + the stride-2 conv2 + bn2 + ReLU of layer2.0 as ONE
    launch -- conv1 row by row into a three-row line buffer in LDS, conv2 from it; the 128-channel tensor between them never
    exists in memory; models/tsm.py:35-50,125-137 + torchvision Bottleneck.conv1 / conv2) against the two launches it replaces:
    conv2's tap (= the kernel's output), the block output and the logits bit for bit, and the trace shows which of them ran."""
    from workoutdetector_amd.engine import TsmEngine, launch_trace
    from workoutdetector_amd.weights import make_state_dict
    sd = make_state_dict(17, 12)
    x = make_input(900 + h + t, b, t, h, w)
    stages = ('layer1.2', 'layer2.0.conv2', 'layer2.0', 'layer2.1')
    got = {}
    for flag in ('1', '0'):
        monkeypatch.setenv('TSM_FUSE_FRONT', flag)
        eng = TsmEngine(num_segments=t, height=h, width=w, is_shift=shift, max_clips=b, state_dict=sd, dtype='bf16')
        got[flag] = [eng.run(None, {'input': x})[0]]
        with launch_trace() as tr:
            got[flag] += [eng.forward_tap(x, s) for s in stages] + [eng.run(None, {'input': x})[0]]
        hp, wp = (((h - 1) // 2 + 1) - 1) // 2 + 1, (((w - 1) // 2 + 1) - 1) // 2 + 1      # layer1's frame = layer2.0's input
        fits = flag == '1' and hp % 2 == 0 and wp <= 64
        assert_fused_slots(eng, x, {'layer2.0.conv2'} if fits else set(), flag)
        eng.close()
        kern = 'front_s2_kernel<true>' if shift else 'front_s2_kernel<false>'
        # (the taps 'layer2.0.conv2', 'layer2.0', 'layer2.1' and the forward run layer2.0's front once each)
        assert tr.count(kern) == (4 if fits else 0) and tr.ran('front_s2_kernel') == fits, (flag, sorted(set(tr.kernels)))
        # ... and the launches it replaces ran exactly when it did not: layer2.0's conv1 is the only 256 -> 128 1x1, its conv2 the only stride-2 128 -> 128 3x3
        assert tr.ran('conv3x3_ws128_kernel<true>') == (not fits) or not tr.ran('conv3x3_ws128_kernel'), sorted(set(tr.kernels))
    for name, a, c in zip(('logits',) + stages + ('logits again',), got['1'], got['0']):
        assert np.array_equal(a, c), name
    assert np.isfinite(got['1'][0]).all() and np.array_equal(got['1'][0], got['1'][-1])
