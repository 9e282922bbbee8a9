"""Crafted cases for the TDN engine (csrc/tsm_tdn.hip, run_tdn / run_mse / finalize_tdn in csrc/tsm_engine.hip), shared by
tests/test_tdn_cases_cpu.py (the preconditions: what a case reaches, and that it tells the documented arithmetic from its near
misses) and tests/test_tdn_edges_gpu.py (the same cases through the engine's taps), and the engine helpers of tests/test_tdn_gpu.py.

    recipes     'plain' (tests/_tdn.py's draw), 'damped' (residual_gain 0.25: full depth stays a usable test network),
                'small_variance' (running_var 1e-6 .. 1e-4: pins kBnEps), 'saturated' (gate_gain 64: e beyond expf's range)
    network / clips / reference / emulated    cached, shared, read-only: the float64 model, its input, its taps, a float32 copy
    gates       the long-term module per operator: the float64 gate of a conv1 tap
    wraps       which frames hold a multiple of one pass of a grid-stride launch (grid_for's cap x the workgroup)
    bars        ``bar_ratio``: the worst element's error over tests._util.assert_close's bound (> 1: assert_close fails)
"""
import copy
import functools
import os
import re

import numpy as np
import torch

from tests import _tdn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP_BAR = dict(rtol=1e-4, atol_scale=1e-4)
LOGITS_BAR = dict(rtol=1e-3, atol_scale=1e-5)
TAP_BAR = dict(rtol=1e-3, atol_scale=3e-5)
NUM_CLASS = 7
SEED = 5
KNOBS = ('TSM_AUTOTUNE', 'TSM_POISON', 'TSM_CONV_CODE', 'TSM_TUNE_CACHE')
D96, FULL, EVEN, FOUR = (1, 2, 1, 2), (3, 4, 6, 3), (2, 1, 1, 1), (4, 1, 1, 2)

# (the variance seed: of 0 .. 9 the draw on which the eps = 1.1e-5 mutant misses the tap bar by the most at its weakest family,
#  141 times at diff.conv1_5 -- tests/test_tdn_cases_cpu.py asserts 100)
RESIDUAL_GAIN, GATE_GAIN, VARIANCE_SEED = 0.25, 64.0, 9
RECIPES = {'plain': None, 'damped': lambda w: _tdn.residual_gain(w, RESIDUAL_GAIN),
           'small_variance': lambda w: _tdn.small_variance(w, VARIANCE_SEED), 'saturated': lambda w: _tdn.gate_gain(w, GATE_GAIN)}

# (depths, recipe, h, w, T, clips, consensus): the model that ships, twice; the even arm of run_tdn's buffer choice; a fourth block
DEPTH_CASES = [(FULL, 'damped', 64, 96, 3, 2, 'identity'), (FULL, 'damped', 64, 64, 2, 1, 'avg'), (EVEN, 'plain', 64, 64, 3, 2, 'avg'),
               (FOUR, 'plain', 64, 64, 3, 2, 'identity')]
# frames whose layer4 maps are 2 x 3, 3 x 2 and 5 x 3 (an even side with an odd one, both ways, and H > W)
PARITY_FRAMES = {(64, 96): ((2, 3), (1, 1)), (96, 64): ((3, 2), (1, 1)), (160, 96): ((5, 3), (2, 1))}
EPS_MUTANTS = (1.1e-5, 2e-5, 1e-3, 1e-12)          # (1e-12 stands for 0, which torch's batch_norm refuses)
EPS_FAMILIES = {'diff.conv1_5': r'^diff\.conv1_5$', 'stem': r'^stem$', 'a plain Bottleneck': r'^(resnext_layer1|layer1)\.\d+$',
                "a BottleneckShift's conv1": r'^layer[234]\.\d+\.conv1$', '.mse.fwd': r'\.mse\.fwd$'}
EXPF_RANGE = 89.0                                  # expf(x) overflows above 88.72 and expf(-x) is below FLT_MIN: e beyond +-89


# ---- networks, inputs, references: computed once, shared, left unchanged ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def network(depths, T, recipe='plain', dtype=torch.float64):
    """(the seeded model of ``recipe`` in ``dtype`` with per-segment logits, its weights as read-only float32 arrays)"""
    model, w = _tdn.build(NUM_CLASS, T, depths, SEED, consensus='identity', dtype=dtype, recipe=RECIPES[recipe])
    for v in w.values():
        v.setflags(write=False)
    return model, w


@functools.lru_cache(maxsize=None)
def clips(h, w, T, n, seed=31):
    x = np.random.default_rng([seed, h, w, T]).standard_normal((n, T, 15, h, w)).astype(np.float32)
    x.setflags(write=False)
    return x


def run(model, x):
    """(per-segment logits [n, T, cls], taps) of ``model`` on clips x [n, T, 15, h, w], in the model's own dtype."""
    n, T, _c, h, w = x.shape
    dtype = next(model.parameters()).dtype
    with torch.no_grad():
        logits, taps = model(torch.from_numpy(np.array(x).reshape(n * T, 15, h, w)).to(dtype), taps=True)
    return logits.numpy(), taps


# The saturated network's input.  Its gates pass on what the blocks in front of them lose 64 times over, so the worst of a tap's
# 700 000 elements is heavy-tailed: over the input seeds 31 .. 46 a float32 copy on the CPU uses 0.15 to 0.94 of the tap bar, and
# the figure moves with the summation order (torch's thread count).  Seed 46 is the one of them that stays under a quarter with 1,
# 3 and 16 threads (0.24, 0.17, 0.17), which tests/test_tdn_cases_cpu.py asserts; every other case uses the suite's seed.
CLIP_SEEDS = {'saturated': 46}


def clips_of(recipe, h, w, T, n):
    return clips(h, w, T, n, CLIP_SEEDS.get(recipe, 31))


@functools.lru_cache(maxsize=None)
def reference(h, w, depths, T, n, recipe='plain'):
    return run(network(depths, T, recipe)[0], clips_of(recipe, h, w, T, n))


@functools.lru_cache(maxsize=None)
def emulated(h, w, depths, T, n, recipe='plain'):
    """The same network computed in float32 by torch on the CPU: what a correct float32 implementation loses."""
    return run(network(depths, T, recipe, torch.float32)[0], clips_of(recipe, h, w, T, n))


def mutant(depths, T, recipe, **eps):
    """A copy of the float64 network with another BatchNorm eps (tests/_tdn.py: set_eps)."""
    return _tdn.set_eps(copy.deepcopy(network(depths, T, recipe)[0]), **eps)


# ---- names ----------------------------------------------------------------------------------------------------------------------
def tap_names(depths):
    names = ['diff.conv1_5', 'diff.stem', 'stem', 'fuse1', 'fuse2']
    names += [f'resnext_layer1.{b}' for b in range(depths[0])] + [f'layer1.{b}' for b in range(depths[0])]
    for li, b in shift_blocks(depths):
        p = f'layer{li}.{b}'
        names += [p, p + '.conv1', p + '.mse.fwd', p + '.mse.bwd', p + '.shift', p + '.conv2']
    return names


def shift_blocks(depths):
    return [(li, b) for li in (2, 3, 4) for b in range(depths[li - 1])]


def n_conv_names(depths):
    """The stem, conv1_5, three convs per block of both paths, a downsample in resnext_layer1 and in each trunk stage."""
    return 2 + 3 * (depths[0] + sum(depths)) + 5


# ---- bars -----------------------------------------------------------------------------------------------------------------------
def bar_ratio(got, want, rtol, atol_scale):
    """max over the elements of |got - want| / (rtol |want| + atol_scale max|want|); a non-finite element counts as infinite."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    err[~np.isfinite(got)] = np.inf
    return float((err / (rtol * np.abs(want) + atol_scale * np.abs(want).max())).max())


def moved(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


def worst_taps(taps, ref_taps, names):
    """{tap name: bar_ratio at TAP_BAR} over ``names``."""
    return {name: bar_ratio(taps[name], ref_taps[name], **TAP_BAR) for name in names}


# ---- the long-term module per operator --------------------------------------------------------------------------------------------
def gate64(model, li, b, conv1_tap):
    """(g, m+, m-) NHWC of block layer<li>.<b>'s long-term module in the model's dtype, from a conv1 tap [N, H, W, C] (float32)."""
    mse = getattr(model.base_model, f'layer{li}_bak')[b].mse
    dtype = next(mse.parameters()).dtype
    with torch.no_grad():
        t = torch.from_numpy(np.asarray(conv1_tap)).to(dtype).permute(0, 3, 1, 2)
        ms, _es = mse.directions(t)
        return _tdn.nhwc(mse(t)), _tdn.nhwc(ms[0]), _tdn.nhwc(ms[1])


def with_temporal(w, shift_block=None):
    """The weights with every shift.conv.weight replaced by (0, 1, 0) -- but for block ``shift_block`` ('layerL_bak.B'), which gets
    ShiftModule's initial pattern, fold = C / 8."""
    sd = dict(w)
    for k, v in w.items():
        if k.endswith('.shift.conv.weight'):
            t = np.zeros_like(v)
            fold = v.shape[0] // 8
            if shift_block is None or f'.{shift_block}.' not in k:
                t[:, 0, 1] = 1
            else:
                t[:fold, 0, 2] = 1
                t[fold:2 * fold, 0, 0] = 1
                t[2 * fold:, 0, 1] = 1
            sd[k] = t
    return sd


def sigmoid_near_miss32(e):
    """exp(e) / (1 + exp(e)) in float32: the rewrite of 1 / (1 + exp(-e)) that is inf / inf once expf overflows."""
    e = np.asarray(e, dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        p = np.exp(e)
        y = p / (np.float32(1) + p)
    assert y.dtype == np.float32
    return y


# ---- grid-stride launches: one pass and the frames at its multiples -------------------------------------------------------------
def launch_pass(kernel, count):
    """Threads in one pass of ``kernel``'s grid-stride launch, read from the code: the launch line in csrc/tsm_tdn.hip must be
    ``TSM_KLAUNCH(<kernel>, dim3(grid_for(<count>, CAP)), dim3(THREADS), ...`` and grid_for (csrc/tsm_device.h) must cap the blocks at
    CAP with THREADS per block.  Returns CAP * THREADS; an AssertionError if the code no longer says so."""
    csrc = os.path.join(ROOT, 'workoutdetector_amd', 'csrc')
    tdn = open(os.path.join(csrc, 'tsm_tdn.hip')).read()
    dev = open(os.path.join(csrc, 'tsm_device.h')).read()
    m = re.search(r'TSM_KLAUNCH\(' + re.escape(kernel) + r'(?:<\w+>)?, dim3\(grid_for\(' + count + r', (\d+)\)\), dim3\((\d+)\)', tdn)
    assert m, f'{kernel}: the launch is no longer a capped grid_for launch'
    cap, threads = int(m.group(1)), int(m.group(2))
    body = dev[dev.index('inline unsigned grid_for(int64_t total, int cap)'):]
    body = body[:body.index('\n}\n')]
    assert f'(total + {threads - 1}) / {threads}' in body and 'blocks < cap' in body and ': cap)' in body, body
    return cap * threads


def wrap_frames(n_frames, per_frame, one_pass):
    """The frames that hold element k * one_pass, k = 1, 2, ... (a pass of the launch ends and the next begins inside them)."""
    total = n_frames * per_frame
    return [k * one_pass // per_frame for k in range(1, (total - 1) // one_pass + 1)]


def blend64(a, d, alpha, beta):
    """(alpha a + beta up(d), |alpha a| + |beta up(d)|) in float64; a [n, h, w, c], d [n, hd, wd, c] float32 taps."""
    n, h, w, _c = a.shape
    iy = [_tdn.nearest_index(i, d.shape[1], h) for i in range(h)]
    ix = [_tdn.nearest_index(i, d.shape[2], w) for i in range(w)]
    pa, pb = alpha * a.astype(np.float64), beta * d.astype(np.float64)[:, iy][:, :, ix]
    return pa + pb, np.abs(pa) + np.abs(pb)


# ---- engines ----------------------------------------------------------------------------------------------------------------------
def engine(h, w, T, depths, sd, max_clips=3, consensus='avg', autotune=False, poison=False, code=None):
    """A TDN engine of the float32 weights ``sd``.  The TSM_* variables are read in tsm_create: set for the constructor only, then
    restored."""
    from workoutdetector_amd.engine import TsmEngine
    keep = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ['TSM_AUTOTUNE'] = '1' if autotune else '0'
    os.environ['TSM_TUNE_CACHE'] = '0'
    if poison:
        os.environ['TSM_POISON'] = '1'
    if code is not None:
        os.environ['TSM_CONV_CODE'] = str(code)
    try:
        return TsmEngine(num_class=NUM_CLASS, num_segments=T, height=h, width=w, is_shift=False, max_clips=max_clips, state_dict=sd,
                         base_model='tdn_resnet50', tdn_depths=depths, consensus_type=consensus)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
