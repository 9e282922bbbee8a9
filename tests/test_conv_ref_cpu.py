"""The float64 per-op reference of tests/_conv_ref.py against the oracle it restates (CPU only): where the two overlap they agree,
the K-concatenated conv3 + downsample form is the sum of its two branches, and shifting the identity is the unshifted form on
the shifted tensor."""
import pytest
import torch

from oracle import tsm_oracle
from tests._conv_ref import conv_ref
from tests._util import assert_close


def _bn(c, g):
    return (torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1,
            torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5)


def _operands(seed, n, cin, cout, k, hi, wi):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, hi, wi, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    return g, x, w, _bn(cout, g)


@pytest.mark.parametrize('k,stride,relu,use_res', [(1, 1, True, True), (3, 1, False, True), (3, 2, True, False),
                                                   (1, 2, False, False)])
def test_matches_the_oracle_where_they_overlap(k, stride, relu, use_res):
    g, x, w, bn = _operands(k + stride, 4, 32, 64, k, 6, 5)
    ho, wo = (6 + 2 * (k // 2) - k) // stride + 1, (5 + 2 * (k // 2) - k) // stride + 1
    res = torch.randn(4, 64, ho, wo, generator=g) if use_res else None
    want = tsm_oracle.conv_bn_act(x, w, bn, stride, k // 2, relu, res)
    assert_close(conv_ref(x, w, bn, stride, relu, res).numpy(), want.numpy(), rtol=1e-5, atol_scale=1e-6, what='f32')
    want16 = tsm_oracle.conv_bn_act_bf16(x, w, bn, stride, k // 2, relu, res)
    assert_close(conv_ref(x, w, bn, stride, relu, res, bf16=True).numpy(), want16.numpy(), rtol=1e-5, atol_scale=1e-6,
                 what='bf16')


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('stride2,hi2,wi2,shift', [(1, 3, 5, 0), (2, 5, 9, 0), (2, 5, 9, 1)])
def test_dual_is_the_sum_of_its_branches(bf16, stride2, hi2, wi2, shift):
    g, x, w, bn = _operands(7, 4, 32, 64, 1, 3, 5)
    x2 = torch.randn(4, 64, hi2, wi2, generator=g)
    w2 = torch.randn(64, 64, 1, 1, generator=g) * 0.2
    bn2 = _bn(64, g)
    T = 2 if shift else 0
    got = conv_ref(x, w, bn, 1, True, T=T, fold_div=8, shift_target=1, x2=x2, w2=w2, bn2=bn2, stride2=stride2, bf16=bf16)
    x2s = tsm_oracle.temporal_shift(x2, 2, 8) if shift else x2
    a = conv_ref(x, w, bn, 1, False, bf16=bf16)
    b = conv_ref(x2s, w2, bn2, stride2, False, bf16=bf16)
    # (bf16: the two biases are summed in fp32 once, the branches carry one each)
    assert_close(got.numpy(), torch.relu(a + b).numpy(), rtol=1e-6 if bf16 else 1e-12, atol_scale=1e-7 if bf16 else 1e-12,
                 what='dual')
    if not bf16:   # and it is the oracle's conv3 + downsample sum
        want = torch.relu(tsm_oracle.conv_bn_act(x, w, bn, 1, 0, False) + tsm_oracle.conv_bn_act(x2s, w2, bn2, stride2, 0, False))
        assert_close(got.numpy(), want.numpy(), rtol=1e-5, atol_scale=1e-6, what='dual vs oracle')


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('form', ['residual1x1', 'residual3x3', 'dual', 'strided1x1'])
def test_shifting_the_identity_is_the_unshifted_form_on_the_shifted_tensor(bf16, form):
    T, div = 3, 4
    k = 3 if form == 'residual3x3' else 1
    stride = 2 if form == 'strided1x1' else 1
    g, x, w, bn = _operands(11, 6, 32, 64, k, 5, 4)
    kw = dict(bf16=bf16)
    if form.startswith('residual'):
        r = torch.randn(6, 64, 5, 4, generator=g)
        got = conv_ref(x, w, bn, stride, True, residual=r, T=T, fold_div=div, shift_target=1, **kw)
        want = conv_ref(x, w, bn, stride, True, residual=tsm_oracle.temporal_shift(r, T, div), **kw)
    elif form == 'dual':
        x2 = torch.randn(6, 64, 9, 7, generator=g)
        w2, bn2 = torch.randn(64, 64, 1, 1, generator=g) * 0.2, _bn(64, g)
        got = conv_ref(x, w, bn, 1, True, T=T, fold_div=div, shift_target=1, x2=x2, w2=w2, bn2=bn2, stride2=2, **kw)
        want = conv_ref(x, w, bn, 1, True, x2=tsm_oracle.temporal_shift(x2, T, div), w2=w2, bn2=bn2, stride2=2, **kw)
    else:
        got = conv_ref(x, w, bn, 2, True, T=T, fold_div=div, shift_target=1, **kw)
        want = conv_ref(tsm_oracle.temporal_shift(x, T, div), w, bn, 2, True, **kw)
    assert torch.equal(got, want), form
    # and the shift did something: the unshifted form differs
    plain = {'residual1x1': lambda: conv_ref(x, w, bn, 1, True, residual=r, **kw),
             'residual3x3': lambda: conv_ref(x, w, bn, 1, True, residual=r, **kw),
             'dual': lambda: conv_ref(x, w, bn, 1, True, x2=x2, w2=w2, bn2=bn2, stride2=2, **kw),
             'strided1x1': lambda: conv_ref(x, w, bn, 2, True, **kw)}[form]()
    assert not torch.equal(got, plain), form
