"""Per-op tests of block placement's conv forms and the K-concatenated conv3 + downsample GEMM (tsm_conv_op, through
engine.conv_bn_act_nhwc's keyword arguments) against the float64 reference of tests/_conv_ref.py:

  a. the shifted identity: 1x1 + residual (Bottleneck conv3) and 3x3 + residual (BasicBlock conv2),
  b. conv3 + downsample as one GEMM, unshifted and with the second source shifted (segmented fp32 forms, split-K, tail split),
  c. the shifted 1x1 at stride 2 (BasicBlock downsample),
  d. exact data-movement checks that need no tolerance,
  e. the refusals, which launch nothing.

Every case asserts from the launch trace that the intended kernel family ran and that the shift was never materialised
(temporal_shift_kernel); every tile code of a case is bit-identical to the others, in both tile walk directions.
Bars: f32 rtol 1e-4 + 1e-4 of the scale (test_ops_gpu.py), split-bf16 3e-4 (test_basicblock_gpu.py), bf16 assert_bf16_op."""
import numpy as np
import pytest
import torch

from oracle.tsm_oracle import bf16_round, temporal_shift
from tests._conv_ref import conv_ref
from tests._guard import guarded_conv
from tests._k_cases import conv_num_segments, segment_len
from tests._util import IGEMM_TILE_DIMS, assert_bf16_op, assert_close, ran_tile, sweep as _sweep
from tests._walk_cases import tail_split_applies

pytestmark = pytest.mark.gpu

DTYPES = ['f32', 'bf16x3', 'bf16']
NAMES = {1: '128x128', 2: '128x64', 3: '64x64', 4: '32x32', 5: '128x128w8', 6: '256x256', 7: 'ws', 8: '256x256p'}
SPLITK, TAILK = 0x100, 0x200
ARM = 'kPrecBlockShift'


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _bn(c, g):
    return (torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1,
            torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5)


def _w(cout, cin, k, g):
    return torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5


def _igemm_codes(dtype, cout):
    return [c for c in (1, 2, 3, 4, 5) if (cout % 128 == 0 or c in (2, 3, 4)) and (c != 4 or dtype == 'f32')]


def _check(got, want, dtype, what):
    if dtype == 'bf16':
        assert_bf16_op(got, want, what=what)
    else:
        tol = 1e-4 if dtype == 'f32' else 3e-4
        assert_close(got, want, rtol=tol, atol_scale=tol, what=what)


def _run(x, w, bn, dtype, code, reverse, **kw):
    from workoutdetector_amd.engine import launch_trace
    bn2 = kw.pop('bn2', None)
    with launch_trace() as tr:
        y = guarded_conv(_nhwc(x).cuda(), w.cuda(), *[b.cuda() for b in bn], dtype=dtype, code=code, reverse=reverse,
                         bn2=None if bn2 is None else [b.cuda() for b in bn2], **kw)     # (hostile memory: tests/_guard.py)
    assert not tr.ran('temporal_shift_kernel'), ('the shifted tensor must never be materialised', tr.kernels)
    return _nchw(y.cpu()), tr


def _igemm(tr):
    return [k for k in tr.kernels if k.startswith('conv_igemm<')]


# ---- a. the shifted identity ------------------------------------------------------------------------------------------
# (k, clips, T, ho, wo, cin, cout, fold_div): frames of 1x1 .. 14x14 (tiles spanning many frames and clips), T = 1 .. 16,
# folds of 8 .. 256 channels, Cout 192 with div 8 (fold 24: the t+1 / t-1 / t boundaries inside a 64-wide tile), ragged M
IDENTITY_CASES = [
    (1, 2, 8, 7, 7, 128, 512, 8),
    (1, 1, 16, 1, 1, 512, 2048, 8),
    (1, 3, 1, 3, 5, 64, 256, 4),
    (1, 2, 2, 14, 14, 64, 256, 16),
    (1, 1, 3, 2, 2, 64, 192, 8),
    (1, 5, 3, 3, 5, 256, 1024, 16),
    (3, 2, 8, 7, 7, 64, 64, 8),
    (3, 1, 3, 14, 14, 128, 128, 16),
    (3, 2, 2, 3, 5, 256, 256, 4),
    (3, 3, 1, 1, 1, 512, 512, 8),
    (3, 1, 16, 2, 2, 64, 64, 8),
]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k,clips,T,ho,wo,cin,cout,div', IDENTITY_CASES)
def test_shifted_identity(hip_lib, dtype, k, clips, T, ho, wo, cin, cout, div):
    g = torch.Generator().manual_seed(k * 1000 + cout + T)
    n = clips * T
    x, w, bn = torch.randn(n, cin, ho, wo, generator=g), _w(cout, cin, k, g), _bn(cout, g)
    res = torch.randn(n, cout, ho, wo, generator=g)
    codes = _igemm_codes(dtype, cout)
    if dtype == 'bf16' and k == 1 and cout % 256 == 0 and cin >= 128:
        codes.append(8)

    def expect(code, tr):
        if code == 8:
            assert tr.ran('conv_bf16_256p_kernel<1, true, true, false>'), tr.kernels
        else:
            assert ran_tile(tr, NAMES[code]), (code, tr.kernels)
            assert any(k_.endswith(']') and f'{ARM}>' in k_ and 'RES = true' in k_ for k_ in _igemm(tr)), tr.kernels

    got = _sweep(codes, lambda code, rev: _run(x, w, bn, dtype, code, rev, residual=_nhwc(res).cuda(), shift_segments=T,
                                               fold_div=div, shift_identity=True), expect)
    want = conv_ref(x, w, bn, 1, True, residual=res, T=T, fold_div=div, shift_target=1, bf16=dtype == 'bf16')
    _check(got.numpy(), want.numpy(), dtype, f'{k}x{k} + shifted residual {dtype}')


# ---- b. conv3 + downsample as one GEMM ---------------------------------------------------------------------------------
# (K1, C2, Cout, ho, wo, stride2, hi2, wi2, clips, T, fold_div): the R50 stage shapes and small / odd frames
DUAL_CASES = [
    (64, 64, 256, 14, 14, 1, 14, 14, 2, 8, 8),
    (128, 256, 512, 7, 7, 2, 13, 13, 1, 8, 8),
    (256, 512, 1024, 3, 5, 2, 5, 9, 2, 3, 16),
    (512, 1024, 2048, 2, 2, 2, 3, 3, 2, 2, 8),
    (64, 64, 256, 2, 3, 2, 3, 5, 3, 1, 4),
    (128, 256, 512, 7, 7, 1, 7, 7, 1, 16, 8),
    (512, 1024, 2048, 7, 7, 2, 14, 14, 8, 8, 8),   # 3136 rows x 32 tiles of 64: the tail split on a 256-CU part
]
TAIL_CASE = DUAL_CASES[-1]
DUAL_PARAMS = [(d,) + c for c in DUAL_CASES for d in DTYPES if c != TAIL_CASE or d == 'f32']   # (segmented in fp32 only)


@pytest.mark.parametrize('shift', [False, True])
@pytest.mark.parametrize('dtype,k1,c2,cout,ho,wo,s2,hi2,wi2,clips,T,div', DUAL_PARAMS)
def test_conv3_downsample_gemm(hip_lib, dtype, shift, k1, c2, cout, ho, wo, s2, hi2, wi2, clips, T, div):
    g = torch.Generator().manual_seed(k1 + c2 + cout + ho)
    n = clips * T
    x, w, bn = torch.randn(n, k1, ho, wo, generator=g), _w(cout, k1, 1, g), _bn(cout, g)
    x2, w2, bn2 = torch.randn(n, c2, hi2, wi2, generator=g), _w(cout, c2, 1, g), _bn(cout, g)
    seg = segment_len(k1 + c2, dtype) > 0
    if seg:   # segmented: whole-K 64x64 / 32x32, split-K and the tail split, all the same bits
        codes = [3, 4, 3 | SPLITK, 4 | SPLITK, 3 | TAILK]
    else:
        codes = _igemm_codes(dtype, cout)
        if dtype == 'bf16' and cout % 256 == 0:
            codes += [8] if shift else [6, 8]
        if dtype == 'bf16' and not shift and (k1, c2, cout) in ((64, 64, 256), (128, 256, 512)):
            codes.append(7)   # (conv1x1_wsn_valid: the layer1.0 / layer2.0 shapes, unshifted)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    tail = seg and tail_split_applies(n * ho * wo, cout, conv_num_segments(k1 + c2, segment_len(k1 + c2, dtype)), n_cu)
    if (k1, c2, cout, ho, wo, s2, hi2, wi2, clips, T, div) == TAIL_CASE and n_cu == 256:
        assert tail, 'the tail-split shape must split on a 256-CU part'

    def expect(code, tr):
        ig = _igemm(tr)
        if code == 6:
            assert tr.ran('conv_bf16_256_kernel<1, false, false, true>'), tr.kernels
        elif code == 8:
            assert tr.ran('conv_bf16_256p_kernel<1, true, false, true>' if shift else 'conv_bf16_256p_kernel<1, false, false, true>'), tr.kernels
        elif code == 7:
            assert tr.ran('conv1x1_wsn_kernel<'), tr.kernels
            assert any(', true' in k_ for k_ in tr.kernels if k_.startswith('conv1x1_wsn_kernel<')), tr.kernels
        else:
            tile = NAMES[code & 0xF]
            assert ran_tile(tr, tile), (code, tr.kernels)
            arms = [k_ for k_ in ig if (f'{ARM}, true' in k_ if shift else (', true>' in k_ or ', true, true>' in k_) and ARM not in k_)]
            assert arms, (code, tr.kernels)
            if seg:
                assert all(', true, true>' in k_ for k_ in arms), ('the segmented (SEG) form must run', arms)
            split = code & SPLITK or (code & TAILK and tail)
            assert tr.ran('splitk_reduce_kernel') == bool(split), (code, tail, tr.kernels)

    got = _sweep(codes, lambda code, rev: _run(x, w, bn, dtype, code, rev, x2=_nhwc(x2).cuda(), w2=w2.cuda(), bn2=bn2,
                                               stride2=s2, shift_segments=T if shift else 0, fold_div=div,
                                               shift_identity=shift), expect)
    want = conv_ref(x, w, bn, 1, True, T=T if shift else 0, fold_div=div, shift_target=1, x2=x2, w2=w2, bn2=bn2, stride2=s2,
                    bf16=dtype == 'bf16')
    _check(got.numpy(), want.numpy(), dtype, f'conv3 + downsample {k1}+{c2}->{cout} s2={s2} shift={shift} {dtype}')


# ---- c. the shifted 1x1 at stride 2 -------------------------------------------------------------------------------------
# (cin, cout, hi, wi, clips, T, fold_div): odd input sizes
STRIDED_CASES = [(64, 128, 13, 9, 2, 8, 8), (128, 256, 7, 7, 1, 3, 16), (256, 512, 5, 3, 3, 1, 8)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cin,cout,hi,wi,clips,T,div', STRIDED_CASES)
def test_shifted_strided_1x1(hip_lib, dtype, cin, cout, hi, wi, clips, T, div):
    g = torch.Generator().manual_seed(cin + hi)
    n = clips * T
    x, w, bn = torch.randn(n, cin, hi, wi, generator=g), _w(cout, cin, 1, g), _bn(cout, g)
    codes = _igemm_codes(dtype, cout) + [6, 7, 8]   # (256x256, ws and 256x256p have no such arm: conv_igemm runs)

    def expect(code, tr):
        ig = [k_ for k_ in _igemm(tr) if 'KS = 1, SHIFT = true, RES = false' in k_]
        assert ig, (code, tr.kernels)
        if code in NAMES and NAMES[code] in IGEMM_TILE_DIMS:
            assert ran_tile(tr, NAMES[code]), (code, tr.kernels)
        for fam in ('conv_bf16_256_kernel<', 'conv_bf16_256p_kernel<', 'conv1x1_ws', 'conv3x3_ws'):
            assert not tr.ran(fam), (code, tr.kernels)

    got = _sweep(codes, lambda code, rev: _run(x, w, bn, dtype, code, rev, stride=2, shift_segments=T, fold_div=div,
                                               shift_identity=True), expect)
    want = conv_ref(x, w, bn, 2, True, T=T, fold_div=div, shift_target=1, bf16=dtype == 'bf16')
    _check(got.numpy(), want.numpy(), dtype, f'shifted 1x1 s2 {dtype}')


# ---- d. exact data movement ---------------------------------------------------------------------------------------------
def _exact(t, dtype):
    return bf16_round(t) if dtype != 'f32' else t   # (values the storage format holds exactly: hi = value, lo = 0)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k,clips,T,ho,wo,cin,cout,div', [(1, 2, 8, 7, 7, 128, 512, 8), (1, 1, 3, 2, 2, 64, 192, 8),
                                                          (1, 1, 16, 1, 1, 512, 2048, 8), (3, 2, 2, 3, 5, 256, 256, 4),
                                                          (3, 3, 1, 2, 3, 64, 64, 8)])
def test_shifted_residual_moves_exactly(hip_lib, dtype, k, clips, T, ho, wo, cin, cout, div):
    """Main weights folded to exactly zero (gamma 0, beta 0), ReLU off: the output IS the shifted residual, bit for bit."""
    g = torch.Generator().manual_seed(cout + ho)
    n = clips * T
    x, w = torch.randn(n, cin, ho, wo, generator=g), _w(cout, cin, k, g)
    bn = (torch.zeros(cout), torch.zeros(cout), torch.randn(cout, generator=g), torch.rand(cout, generator=g) + 0.5)
    res = _exact(torch.randn(n, cout, ho, wo, generator=g), dtype)
    codes = _igemm_codes(dtype, cout) + ([8] if dtype == 'bf16' and k == 1 and cout % 256 == 0 and cin >= 128 else [])
    got = _sweep(codes, lambda code, rev: _run(x, w, bn, dtype, code, rev, relu=False, residual=_nhwc(res).cuda(),
                                               shift_segments=T, fold_div=div, shift_identity=True),
                 lambda code, tr: None)
    want = temporal_shift(res, T, div)
    bad = (got != want)
    assert not bad.any(), f'{int(bad.sum())} elements differ; first at {tuple(bad.nonzero()[0].tolist())}'


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k1,c2,ho,wo,s2,hi2,wi2,clips,T,div', [(64, 256, 7, 7, 2, 13, 13, 1, 8, 8),
                                                                (128, 512, 3, 5, 2, 5, 9, 2, 3, 16),
                                                                (512, 1024, 1, 1, 1, 1, 1, 3, 2, 8)])
def test_shifted_second_source_moves_exactly(hip_lib, dtype, k1, c2, ho, wo, s2, hi2, wi2, clips, T, div):
    """conv3 folded to zero and the downsample a channel permutation (ReLU off): the output is the stride-2 subsample of
    shift(x2), permuted, times the BatchNorm scale."""
    g = torch.Generator().manual_seed(k1 + c2)
    n, cout = clips * T, c2
    x, w = torch.randn(n, k1, ho, wo, generator=g), _w(cout, k1, 1, g)
    bn = (torch.zeros(cout), torch.zeros(cout), torch.randn(cout, generator=g), torch.rand(cout, generator=g) + 0.5)
    x2 = _exact(torch.randn(n, c2, hi2, wi2, generator=g), dtype)
    perm = torch.randperm(c2, generator=g)
    w2 = torch.zeros(cout, c2, 1, 1)
    w2[torch.arange(cout), perm, 0, 0] = 1.0
    bn2 = (torch.ones(cout), torch.zeros(cout), torch.zeros(cout), torch.ones(cout))
    scale = np.float32(1.0) / np.sqrt(np.float32(1.0) + np.float32(1e-5))
    if dtype == 'bf16':
        scale = float(bf16_round(torch.tensor([scale])).item())
    codes = ([3, 4, 3 | SPLITK] if segment_len(k1 + c2, dtype) > 0 else _igemm_codes(dtype, cout) +
             ([8] if dtype == 'bf16' and cout % 256 == 0 else []))
    got = _sweep(codes, lambda code, rev: _run(x, w, bn, dtype, code, rev, relu=False, x2=_nhwc(x2).cuda(), w2=w2.cuda(), bn2=bn2,
                                               stride2=s2, shift_segments=T, fold_div=div, shift_identity=True),
                 lambda code, tr: None)
    want = temporal_shift(x2, T, div)[:, perm][:, :, ::s2, ::s2].to(torch.float64) * float(scale)
    assert_close(got.numpy(), want.numpy(), rtol=1e-6, atol_scale=0.0, what=f'permuted shifted x2 {dtype}')


# ---- e. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(hip_lib):
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import conv_bn_act_nhwc, launch_trace
    g = torch.Generator().manual_seed(3)
    bn = [t.cuda() for t in _bn(64, g)]
    x = torch.randn(16, 4, 4, 64, generator=g).cuda()
    w1, w3 = _w(64, 64, 1, g).cuda(), _w(64, 64, 3, g).cuda()
    res = torch.randn(16, 4, 4, 64, generator=g).cuda()
    second = dict(x2=x, w2=w1, bn2=bn)
    cases = [
        ('shift_target 1 with nothing to shift', -1, dict(w=w3, shift_segments=8, shift_identity=True)),
        ('a second source with k = 3', -7, dict(w=w3, **second)),
        ('a second source with a residual', -1, dict(w=w1, residual=res, **second)),
        ('bf16 with fold % 8', -7, dict(w=w1, residual=res, shift_segments=8, fold_div=16, shift_identity=True, dtype='bf16')),
        ('split-bf16 with fold % 8', -7, dict(w=w1, residual=res, shift_segments=8, fold_div=16, shift_identity=True,
                                             dtype='bf16x3')),
        ('2 * fold above the channels', -1, dict(w=w1, residual=res, shift_segments=8, fold_div=1, shift_identity=True)),
        ('2 * fold above the second source channels', -1, dict(w=w1, shift_segments=8, fold_div=1, shift_identity=True,
                                                                **second)),
        ('N % T', -1, dict(w=w1, residual=res, shift_segments=3, shift_identity=True)),
        ('N % T (second source)', -1, dict(w=w1, shift_segments=5, shift_identity=True, **second)),
        ('a shifted first source with a second source', -1, dict(w=w1, shift_segments=8, **second)),
    ]
    for what, status, kw in cases:
        kw = dict(kw)
        wt = kw.pop('w')
        with launch_trace() as tr:
            with pytest.raises(_lib.TsmError) as ei:
                conv_bn_act_nhwc(x, wt, *bn, **kw)
        assert ei.value.status == status, (what, ei.value)
        assert tr.kernels == [], (what, tr.kernels)
