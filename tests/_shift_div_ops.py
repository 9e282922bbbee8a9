"""Operands, references and bars of the tests/_shift_div_cases.py cases, shared by the CPU preconditions
(tests/test_shift_div_cases_cpu.py) and the GPU run (tests/test_shift_div_gpu.py) so that both are about the same numbers."""
import numpy as np
import torch

from oracle import tsm_oracle
from oracle.tsm_oracle import temporal_shift
from tests._conv_ref import conv_ref
from tests._shift_div_cases import GEOMETRIES, shifted_channels
from tests._util import BF16_E2E_BAR, BF16_OP_RTOL, BF16_TAP_BAR, make_input
from workoutdetector_amd.weights import make_state_dict, to_torch

# the per-op bars: (rtol, atol as a fraction of the scale) -- fp32 1e-4 + 1e-4, split-bf16 3e-4 + 3e-4, bf16 assert_bf16_op's
BARS = {'f32': (1e-4, 1e-4), 'bf16x3': (3e-4, 3e-4), 'bf16': (BF16_OP_RTOL, 2e-5)}


def _bn(c, g):
    return (torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1,
            torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5)


def _w(cout, cin, k, g):
    return torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5


def operands(c):
    """The case's operands on the CPU (NCHW, seeded by its id): (x, w, bn) and the reference's keyword operands."""
    g = torch.Generator().manual_seed(sum(map(ord, c['id'])))
    x, w, bn = torch.randn(c['n'], c['cin'], c['hi'], c['wi'], generator=g), _w(c['cout'], c['cin'], c['k'], g), _bn(c['cout'], g)
    pad = c['k'] // 2
    ho, wo = (c['hi'] + 2 * pad - c['k']) // c['stride'] + 1, (c['wi'] + 2 * pad - c['k']) // c['stride'] + 1
    ref = {}
    if c['form'] == 'shift_res':
        ref['residual'] = torch.randn(c['n'], c['cout'], ho, wo, generator=g)
    if 'cin2' in c:
        ref.update(x2=torch.randn(c['n'], c['cin2'], c['hi2'], c['wi2'], generator=g), w2=_w(c['cout'], c['cin2'], 1, g),
                   bn2=_bn(c['cout'], g), stride2=c['stride2'])
    return (x, w, bn), ref


def reference(c, ops, ref, fold_div=None, swap=False):
    """conv_ref of the case (NCHW float64).  `fold_div`: another one than the case's (a wrong fold).  `swap`: frames t + 1 and
    t - 1 exchanged -- the two channel groups of the shifted operand are swapped before the shift and swapped back behind it,
    so that group 0 reads t - 1 and group 1 reads t + 1."""
    x, w, bn = ops
    div = c['fold_div'] if fold_div is None else fold_div
    target = int(c['form'] != 'shift')
    if not swap:
        return conv_ref(x, w, bn, c['stride'], True, bf16=c['dtype'] == 'bf16', T=c['T'], fold_div=div, shift_target=target, **ref)
    fold = shifted_channels(c) // div
    assert 2 * fold <= shifted_channels(c)

    def sw(t):
        return torch.cat([t[:, fold:2 * fold], t[:, :fold], t[:, 2 * fold:]], dim=1)

    def shifted(t):
        return sw(temporal_shift(sw(t), c['T'], div))
    ref = dict(ref)
    if c['form'] == 'shift_res':
        ref['residual'] = shifted(ref['residual'])
    elif c['form'] == 'dual_shift':
        ref['x2'] = shifted(ref['x2'])
    else:
        x = shifted(x)
    return conv_ref(x, w, bn, c['stride'], True, bf16=c['dtype'] == 'bf16', **ref)


def misses(got, want, dtype):
    """By how many times the worst element of `got` misses the dtype's per-op bar against `want` (<= 1: it passes)."""
    rtol, atol = BARS[dtype]
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = rtol * np.abs(want) + atol * float(np.abs(want).max())
    return float((np.abs(got - want) / bound).max())


# ---- the engine cases ---------------------------------------------------------------------------------------------------------
KEEP_TAPS = ('layer1.0.conv1', 'layer2.0.conv1', 'layer3.0.conv1', 'layer4.0.conv1', 'layer4.2', 'layer4.1')
_ORACLE = {}


def engine_input(geo):
    """(state-dict seed, x [B, T, 3, H, W]) of a GEOMETRIES key."""
    t, h, w, sd_seed, x_seed = GEOMETRIES[geo]
    return sd_seed, make_input(x_seed, 2, t, h, w)


def engine_state_dict(base_model, place, geo):
    return make_state_dict(GEOMETRIES[geo][3], 12, base_model, shift_place=place)


def engine_oracle(base_model, place, bf16, div, geo):
    """(logits, {tap: NHWC array}) of oracle/tsm_oracle.py's forward at `div` (the bf16-storage restatement when `bf16`), computed
    once per configuration and left unchanged."""
    key = (base_model, place, bool(bf16), div, geo)
    if key not in _ORACLE:
        _, x = engine_input(geo)
        taps = {}
        logits = tsm_oracle.forward(to_torch(engine_state_dict(base_model, place, geo)), torch.from_numpy(x), base_model, place, bf16=bool(bf16),
                                    n_segment=GEOMETRIES[geo][0], shift_div=div, taps=taps).numpy()
        _ORACLE[key] = (logits, {k: v.permute(0, 2, 3, 1).contiguous().numpy() for k, v in taps.items() if k in KEEP_TAPS})
    return _ORACLE[key]


def logits_misses(got, want, dtype):
    """By how many times `got` misses the dtype's logits bar against `want`: f32 and split-bf16 rtol 1e-3 + 1e-5 of the scale;
    bf16 BF16_E2E_BAR of the scale (against the bf16-storage oracle)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = float(np.abs(want).max())
    if dtype == 'bf16':
        return float(np.abs(got - want).max()) / scale / BF16_E2E_BAR
    return float((np.abs(got - want) / (1e-3 * np.abs(want) + 1e-5 * scale)).max())


def tap_misses(got, want, dtype):
    """The same for a stage tap: rtol 1e-3 + 3e-5 of the scale; bf16 BF16_TAP_BAR of the scale."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = float(np.abs(want).max())
    if dtype == 'bf16':
        return float(np.abs(got - want).max()) / scale / BF16_TAP_BAR
    return float((np.abs(got - want) / (1e-3 * np.abs(want) + 3e-5 * scale)).max())
