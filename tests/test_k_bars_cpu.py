"""The per-op bars at the K lengths of tests/_k_cases.py, restated on the CPU: do they still separate a right kernel from a wrong
one at K = 32 (one step), 4608 (the 3x3 at cin 512) and 8192 (the longest chain)?  N(0,1) inputs and He-scaled weights, as the
GPU tests draw them; each model's worst |error| / bound over a 64 x 64 tile:

  float32 ascending-k chain against float64, at the fp32 bar (rtol 1e-4 + 1e-4 of the scale);
  the split model hi*hi + hi*lo + lo*hi in float32, at the split-bf16 bar (3e-4 + 3e-4);
  a float32 chain over bf16-rounded operands against float64 of the same operands, at assert_bf16_op's bar.

A correct kernel's arithmetic must stay below ONE TENTH of its bar (the chain order inside an MFMA differs from a scalar chain,
so the kernels are not held to these numbers, only the bars are); the split model with its lo*hi term dropped -- the kind of
subtly wrong kernel the bar is there to catch -- must miss it."""
import numpy as np
import pytest
import torch

from oracle.tsm_oracle import bf16_round
from tests import _k_cases as kc
from tests._util import BF16_OP_RTOL

M = N = 64


def _operands(k):
    g = torch.Generator().manual_seed(k)
    return torch.randn(M, k, generator=g), torch.randn(k, N, generator=g) * (2.0 / k) ** 0.5


def _chain(terms):
    """Ascending-k float32 accumulation of per-k [M, N] float32 products: each product and each sum rounded to float32."""
    acc = np.zeros((M, N), np.float32)
    for t in terms:
        acc = acc + t
    return acc


def _products(a, b):
    a, b = a.numpy(), b.numpy()
    return (a[:, i:i + 1] * b[i:i + 1, :] for i in range(a.shape[1]))


def _over_bound(got, want, rtol, atol_scale):
    want = want.numpy()
    bound = rtol * np.abs(want) + atol_scale * np.abs(want).max()
    return float((np.abs(got.astype(np.float64) - want) / bound).max())


def _split(t):
    hi = bf16_round(t)
    return hi, bf16_round(t - hi)


def test_the_k_values_are_the_tables_extremes():
    ks = {kc.kp_total(c) for c in kc.cases(256) if c['k'] != 7}
    assert min(ks) == 32 and max(ks) == 8192 and 4608 in ks


@pytest.mark.parametrize('k', [32, 4608, 8192])
def test_bars_have_room_and_still_separate(k):
    a, b = _operands(k)
    want = a.double() @ b.double()
    f32 = _over_bound(_chain(_products(a, b)), want, 1e-4, 1e-4)
    (ah, al), (bh, bl) = _split(a), _split(b)
    split = _over_bound(_chain(t for three in zip(_products(ah, bh), _products(ah, bl), _products(al, bh)) for t in three), want, 3e-4, 3e-4)
    dropped = _over_bound(_chain(t for two in zip(_products(ah, bh), _products(ah, bl)) for t in two), want, 3e-4, 3e-4)
    bf = _over_bound(_chain(_products(ah, bh)), ah.double() @ bh.double(), BF16_OP_RTOL, 2e-5)
    print(f'K = {k}: worst error / bound: fp32 chain {f32:.3g}, split {split:.3g}, bf16 {bf:.3g}; split without lo*hi {dropped:.3g}')
    assert f32 < 0.1 and split < 0.1 and bf < 0.1, (k, f32, split, bf)
    assert dropped > 1.0, (k, dropped)
