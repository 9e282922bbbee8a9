"""Crafted cases that pin the BatchNorm eps of the TSM ResNet family (kBnEps in csrc/tsm_host_util.h: fold_and_pack for every conv,
fold_and_pack_stem_pairs for the stems of the bf16 formats, fold_and_pack_bias for the non-local W; concat_k_pair sums two folded
biases), shared by tests/test_bn_cases_cpu.py (the preconditions: a float32 copy fits the bars, a tenth more eps at any one fold site
does not) and tests/test_bn_eps_gpu.py (the same cases through the engine and through tsm_conv_op).  No GPU code here.

    recipe      tests/_tdn.py's small_variance on a make_state_dict dict: running_var log-uniform in 1e-6 .. 1e-4, gamma scaled so
                that the folded scale keeps its size.  Under the seeded draws (running_var in 0.6 .. 1.4) eps is 1e-5 of what stands
                under the root and no test of the family sees it.
    weights / network / clips / reference / emulated    cached, shared, read-only: the float32 arrays the engine loads, the float64
                torch module computed from them, its input, its logits and taps, a float32 copy
    mutant      a copy of the float64 network with another eps at one fold site or at all of them
    op_case     the per-op cases: tensors for guarded_conv and the float64 result of tests/_conv_ref.py
    bars        tests/_tdn_cases.py's bar_ratio: the worst element's error over tests._util.assert_close's bound
"""
import copy
import functools

import numpy as np
import torch
import torch.nn as nn

from tests import _conv_ref
from tests._nonlocal import torch_tsm_nl
from tests._tdn import small_variance
from tests._tdn_cases import bar_ratio
from tests._torch_tsm import TorchTSM
from tests._util import make_input
from workoutdetector_amd.weights import BACKBONES, WIDTHS, make_state_dict

LOGITS_BAR = dict(rtol=1e-3, atol_scale=1e-5)
TAP_BAR = dict(rtol=1e-3, atol_scale=3e-5)
OP_BARS = {'f32': dict(rtol=1e-4, atol_scale=1e-4), 'bf16x3': dict(rtol=3e-4, atol_scale=3e-4)}
NUM_CLASS, WEIGHT_SEED, INPUT_SEED = 12, 3, 17
CLIPS, T = 2, 2
R18, R34, R50, WRN = 'resnet18', 'resnet34', 'resnet50', 'wide_resnet50_2'
MUTANT_EPS = 1.1e-5
KNOBS = ('TSM_AUTOTUNE', 'TSM_POISON', 'TSM_CONV_CODE', 'TSM_CONV_TILE', 'TSM_TUNE_CACHE')

# The variance seed: of 0 .. 9 the draw on which the eps = 1.1e-5 mutant of the weakest single site (over every engine case below,
# the better of the logits and the site's tap) misses its bar by the most.  Measured (tests/test_bn_cases_cpu.py prints them):
#     seed      0     1     2     3     4     5     6     7     8     9
#     weakest   27.5  22.0  21.1  26.8  29.2  21.9  22.1  21.4  24.8  25.9      (times the bar; the test asserts 10)
# Every one of them is resnet18's 'last' site, layer4.1.bn2: one BatchNorm in front of a 512-wide average.  At seed 4 it is the
# block-placement case, 29.2 at the tap layer4.1 and 6.5 on the logits -- a site the logits alone would not hold to the factor.
VARIANCE_SEED = 4


# ---- engine cases -------------------------------------------------------------------------------------------------------------
class Case:
    """One engine configuration at the smallest geometry: 2 clips of T = 2 frames of 32 x 32 (the non-local case: 32 x 64, the
    smallest frame of tests/test_nonlocal_gpu.py).  ``taps``: the engine's tap names, one directly behind each fold site; ``sites``:
    {single fold site: the tap that must see its mutant}."""

    def __init__(self, base_model, dtype, place, non_local=False, h=32, w=32):
        self.base_model, self.dtype, self.place, self.non_local, self.h, self.w = base_model, dtype, place, non_local, h, w
        last = f'layer4.{BACKBONES[base_model][0][3] - 1}'
        down = 'layer1.0' if BACKBONES[base_model][1] == 'bottleneck' else 'layer2.0'
        # stem: bn1 through the max-pool; layer1.0: the first block (a Bottleneck's K-concatenated conv3 + downsample GEMM);
        # layer2.0: a block with a downsample in every backbone; last: layer4's last block, behind its last BatchNorm
        self.taps = ('stem', 'layer1.0', 'layer2.0', last)
        self.sites = {'stem': 'stem', 'downsample': down, 'last': last}
        if non_local:
            self.taps += ('layer2.0.block', 'layer3.4')       # layer2.0 is the wrapper's output: block -> attention -> W -> + x
            self.sites['nl.W'] = 'layer2.0'
        self.id = f'{base_model}-{dtype}-{place}' + ('-nl' if non_local else '')
        self.key = (base_model, place, non_local, h, w)        # what the float64 reference depends on

    def __repr__(self):
        return self.id


# every backbone once in f32 and once in bf16x3, the placements alternating; R50 with non-local blocks (f32 only).
# One bf16 R50 case against the bf16-storage oracle: the all-sites mutant moves that oracle's logits by 0.20 of their scale, 20
# times BF16_E2E_BAR (tests/test_bn_cases_cpu.py asserts 10), so the case is in.  It adds no fold site that bf16x3 does not run.
#
# Measured on the CPU at VARIANCE_SEED (tests/test_bn_cases_cpu.py prints and asserts them): how many times the eps = 1.1e-5 mutant
# misses the logits bar / the bar of the site's tap, and the largest share of any bar the float32 copy uses.
#     case                      all sites   stem         downsample    last         nl.W        float32 copy
#     resnet18 blockres         899         131 / 39.4   622 / 146     44.5 / 20.4              0.011
#     resnet18 block            483         175 / 39.4   410 / 156     6.46 / 29.2              0.012
#     resnet34 block            3040        505 / 39.4   2130 / 284    107 / 31.8               0.015
#     resnet34 blockres         1230        53.8 / 39.4  604 / 186     26.4 / 30.3              0.0099
#     resnet50 blockres         516         77.3 / 39.4  233 / 289     38.1 / 76.8              0.012
#     resnet50 block            2840        591 / 39.4   1520 / 220    134 / 72                 0.012
#     wide_resnet50_2 block     551         124 / 39.4   230 / 249     57.8 / 62.7              0.011
#     wide_resnet50_2 blockres  429         39.6 / 39.4  138 / 240     13.3 / 90.8              0.0095
#     resnet50 blockres nl      843         73.9 / 39.3  213 / 269     26.4 / 139   60.9 / 174  0.022
# Under the plain make_state_dict weights the same networks WITHOUT eps (1e-12) stay at 0.08 .. 0.72 of the logits bar.
# Per op the mutant misses its bar 173 (shifted 1x1), 157 (3x3 stride 2), 187 (stem), 62.5 (stem bf16x3) and 175 (conv3 +
# downsample) times; torch's own float32 uses under 0.003 of it.
ENGINE_CASES = [Case(R18, 'f32', 'blockres'), Case(R18, 'bf16x3', 'block'), Case(R34, 'f32', 'block'), Case(R34, 'bf16x3', 'blockres'),
                Case(R50, 'f32', 'blockres'), Case(R50, 'bf16x3', 'block'), Case(WRN, 'f32', 'block'), Case(WRN, 'bf16x3', 'blockres'),
                Case(R50, 'f32', 'blockres', non_local=True, h=32, w=64), Case(R50, 'bf16', 'blockres')]
TUNED_CASE = ENGINE_CASES[4]          # the R50 f32 case that runs twice, tuned and with TSM_AUTOTUNE=0


@functools.lru_cache(maxsize=None)
def weights(base_model, place, non_local=False, recipe='small_variance', variance_seed=None):
    """The float32 arrays the engine loads, read-only: make_state_dict's seeded draw, under ``recipe`` small_variance with the
    variance redrawn (``variance_seed``: VARIANCE_SEED unless given)."""
    sd = make_state_dict(WEIGHT_SEED, NUM_CLASS, base_model, place, non_local=non_local)
    if recipe == 'small_variance':
        sd = small_variance(sd, VARIANCE_SEED if variance_seed is None else variance_seed)
    else:
        assert recipe == 'plain', recipe
    for v in sd.values():
        v.setflags(write=False)
    return sd


@functools.lru_cache(maxsize=None)
def network(base_model, place, non_local=False, recipe='small_variance', dtype=torch.float64, variance_seed=None):
    """The torch module of the case's weights in ``dtype``, eval mode (tests/_torch_tsm.py; tests/_nonlocal.py wraps the five blocks)."""
    sd = {k: np.array(v) for k, v in weights(base_model, place, non_local, recipe, variance_seed).items()}
    if non_local:
        return torch_tsm_nl(base_model, place, NUM_CLASS, T, sd=sd, dtype=dtype)
    return TorchTSM(base_model, WIDTHS.get(base_model, 64), place, NUM_CLASS, T).load_engine_state_dict(sd).to(dtype).eval()


@functools.lru_cache(maxsize=None)
def clips(h, w):
    x = make_input(INPUT_SEED, CLIPS, T, h, w)
    x.setflags(write=False)
    return x


def _tap_module(net, name):
    if name == 'stem':
        return net.base_model.maxpool
    if name.endswith('.block'):
        return net.base_model.get_submodule(name[:-len('.block')]).block
    return net.base_model.get_submodule(name)


@torch.no_grad()
def run(net, x, taps):
    """(logits [clips, classes], {tap: NHWC ndarray}) of ``net`` on clips x [clips, T, 3, h, w], in the module's own dtype."""
    got, handles = {}, []
    for name in taps:
        handles.append(_tap_module(net, name).register_forward_hook(
            lambda _m, _i, out, name=name: got.__setitem__(name, out.detach().permute(0, 2, 3, 1).contiguous().numpy())))
    try:
        logits = net(torch.from_numpy(np.array(x)).to(next(net.parameters()).dtype)).numpy()
    finally:
        for h in handles:
            h.remove()
    return logits, got


def _frozen(logits, taps):
    logits.setflags(write=False)
    for v in taps.values():
        v.setflags(write=False)
    return logits, taps


@functools.lru_cache(maxsize=None)
def _reference(key, taps, recipe, variance_seed):
    base_model, place, non_local, h, w = key
    return _frozen(*run(network(base_model, place, non_local, recipe, torch.float64, variance_seed), clips(h, w), taps))


def reference(case, recipe='small_variance', variance_seed=None):
    """The float64 module's (logits, taps) for the case: computed once, read-only."""
    return _reference(case.key, case.taps, recipe, variance_seed)


@functools.lru_cache(maxsize=None)
def _emulated(key, taps):
    base_model, place, non_local, h, w = key
    return _frozen(*run(network(base_model, place, non_local, dtype=torch.float32), clips(h, w), taps))


def emulated(case):
    """The same network computed in float32 by torch on the CPU: what a correct float32 implementation loses."""
    return _emulated(case.key, case.taps)


def bf16_reference(case, eps=None):
    """(logits, {tap: NHWC}) of the bf16-storage oracle (oracle/tsm_oracle.py) and the fp32 oracle's logits for a bf16 case;
    ``eps``: with that constant in place of the oracle's BN_EPS."""
    from oracle import tsm_oracle
    sd = {k: torch.from_numpy(np.array(v)) for k, v in weights(case.base_model, case.place).items()}
    x = torch.from_numpy(np.array(clips(case.h, case.w)))
    keep = tsm_oracle.BN_EPS
    try:
        if eps is not None:
            tsm_oracle.BN_EPS = eps
        taps = {}
        logits16 = tsm_oracle.forward(sd, x, case.base_model, case.place, True, n_segment=T, taps=taps).numpy()
        logits32 = tsm_oracle.forward(sd, x, case.base_model, case.place, False, n_segment=T).numpy()
    finally:
        tsm_oracle.BN_EPS = keep
    return logits16, {name: taps[name].permute(0, 2, 3, 1).contiguous().numpy() for name in case.taps}, logits32


# ---- mutants ------------------------------------------------------------------------------------------------------------------
def site_modules(net, site):
    """The BatchNorm modules of a fold site: 'all'; 'stem' (bn1); 'downsample' (every downsample.1); 'nl.W' (every non-local
    W.1); 'last' (the last BatchNorm of layer4's last block)."""
    named = [(n, m) for n, m in net.named_modules() if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d))]
    if site == 'all':
        return [m for _n, m in named]
    if site == 'stem':
        return [net.base_model.bn1]
    if site == 'downsample':
        return [m for n, m in named if n.endswith('.downsample.1')]
    if site == 'nl.W':
        return [m for n, m in named if n.endswith('.nl.W.1')]
    assert site == 'last', site
    return [[m for n, m in named if n.startswith('base_model.layer4.') and '.downsample.' not in n][-1]]


def mutant(case, site, eps=MUTANT_EPS, recipe='small_variance', variance_seed=None):
    """(logits, taps) of a copy of the case's float64 network with ``eps`` in the BatchNorms of ``site``."""
    base_model, place, non_local, h, w = case.key
    net = copy.deepcopy(network(base_model, place, non_local, recipe, torch.float64, variance_seed))
    mods = site_modules(net, site)
    assert mods, site
    for m in mods:
        assert m.eps == 1e-5
        m.eps = eps
    return run(net, clips(h, w), case.taps)


def misses(case, got, want):
    """{'logits' and every tap of the case: bar_ratio at its bar} of a (logits, taps) pair against the reference pair."""
    out = {'logits': bar_ratio(got[0], want[0], **LOGITS_BAR)}
    out.update({name: bar_ratio(got[1][name], want[1][name], **TAP_BAR) for name in case.taps})
    return out


# ---- per-op cases -------------------------------------------------------------------------------------------------------------
# the smallest shape of its kind in tests/test_ops_gpu.py's CONV_CASES / tests/test_conv_forms_gpu.py's DUAL_CASES:
# name -> (dtype, n, hi, wi, cin, cout, k, stride, shift T, second source (cin2, hi2, wi2, stride2) or None)
OP_CASES = {
    'shifted 1x1': ('f32', 8, 14, 14, 64, 64, 1, 1, 8, None),
    '3x3 stride 2': ('f32', 4, 14, 14, 128, 128, 3, 2, 0, None),
    'stem': ('f32', 2, 32, 32, 3, 64, 7, 2, 0, None),
    'stem bf16x3': ('bf16x3', 2, 32, 32, 3, 64, 7, 2, 0, None),          # fold_and_pack_stem_pairs
    'conv3 + downsample': ('f32', 3, 2, 3, 64, 256, 1, 1, 0, (64, 3, 5, 2)),      # concat_k_pair: two folds, their biases summed
}


def _op_bn(c, g, tag, variance_seed):
    """(gamma, beta, mean, var) as the per-op tests draw them, the variance and gamma by the recipe."""
    plain = {tag + '.weight': (torch.rand(c, generator=g) + 0.5).numpy(), tag + '.running_var': (torch.rand(c, generator=g) + 0.5).numpy()}
    beta, mean = torch.randn(c, generator=g) * 0.1, torch.randn(c, generator=g) * 0.1
    sv = small_variance(plain, variance_seed)
    return (torch.from_numpy(sv[tag + '.weight']), beta, mean, torch.from_numpy(sv[tag + '.running_var']))


@functools.lru_cache(maxsize=None)
def op_case(name):
    """The operands of a per-op case (CPU float32, NCHW) and conv_ref's keyword arguments; shared, not to be written to."""
    dtype, n, hi, wi, cin, cout, k, stride, shift_t, second = OP_CASES[name]
    g = torch.Generator().manual_seed(4000 + cin + cout + k + hi)
    x = torch.randn(n, cin, hi, wi, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    op = dict(dtype=dtype, x=x, w=w, bn=_op_bn(cout, g, 'bn', VARIANCE_SEED), stride=stride, T=shift_t, x2=None, w2=None, bn2=None, stride2=1)
    if second is not None:
        cin2, hi2, wi2, stride2 = second
        op.update(x2=torch.randn(n, cin2, hi2, wi2, generator=g), w2=torch.randn(cout, cin2, 1, 1, generator=g) * (2.0 / cin2) ** 0.5,
                  bn2=_op_bn(cout, g, 'bn2', VARIANCE_SEED + 1), stride2=stride2)
    return op


def op_reference(name, eps=None):
    """tests/_conv_ref.py's float64 result of a per-op case (NCHW); ``eps``: with that constant in place of its BN_EPS."""
    op = op_case(name)
    keep = _conv_ref.BN_EPS
    try:
        if eps is not None:
            _conv_ref.BN_EPS = eps
        return _conv_ref.conv_ref(op['x'], op['w'], op['bn'], op['stride'], True, T=op['T'], fold_div=8, x2=op['x2'], w2=op['w2'],
                                  bn2=op['bn2'], stride2=op['stride2']).numpy()
    finally:
        _conv_ref.BN_EPS = keep


# ---- engines ------------------------------------------------------------------------------------------------------------------
def engine(case, env=None, dtype=None, max_clips=CLIPS):
    """A TsmEngine of the case's weights.  The TSM_* variables are read in tsm_create: ``env`` is set for the constructor only
    (every other knob unset, the tune cache off), then the environment is restored."""
    import os

    from workoutdetector_amd.engine import TsmEngine
    keep = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ['TSM_TUNE_CACHE'] = '0'
    os.environ.update(env or {})
    try:
        return TsmEngine(num_class=NUM_CLASS, num_segments=T, height=case.h, width=case.w, max_clips=max_clips,
                         state_dict=dict(weights(case.base_model, case.place, case.non_local)), base_model=case.base_model,
                         shift_place=case.place, dtype=dtype or case.dtype, non_local=case.non_local)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
