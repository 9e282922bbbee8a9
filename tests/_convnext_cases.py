"""Crafted cases for the ConvNeXt kernels (csrc/tsm_convnext.hip), shared by tests/test_convnext_cases_cpu.py (the preconditions:
what a case reaches, and that it tells the documented arithmetic from its near misses) and tests/test_convnext_edges_gpu.py (the
same cases through the engine's taps).

    coverage    which (accumulator, tap) pairs of dwconv7_ln_kernel's TS x TS tile ever multiply an in-frame input
    float32     the kernels' documented orders in numpy float32: the fmaf chain of the depthwise conv (from the bias, ky-major,
                kx inside), the LayerNorm's two passes with the lane / butterfly / wave reduction, and a one-pass variance
                (E[x^2] - mean^2) in the same reduction order, which the kernels must NOT be
    state dicts small signal (pins eps), common offset (pins the two-pass order), dead rows, chosen GELU inputs
    bars        ``bar_ratio``: the worst element's error over tests._util.assert_close's bound (> 1: assert_close fails)
"""
import collections
import functools
import math

import numpy as np

from tests import _convnext as cn

f32 = np.float32
DW_TILE = {128: 4, 256: 4, 512: 4, 1024: 2}            # cnx_dw_tile, as tests/convnext_host.cpp asserts it
THREADS = 256                                          # a workgroup of dwconv7_ln_kernel: 1024 / C lane groups of C / 4 lanes


@functools.lru_cache(maxsize=None)
def noise(h, w, seed=31):
    """[2, 1, 3, h, w] float32 noise, both frames (no all-zero frame: its rows would leave every variance window)."""
    x = np.random.default_rng([seed, h, w]).standard_normal((2, 1, 3, h, w)).astype(f32)
    x.setflags(write=False)
    return x


# ---- maps, tiles, coverage --------------------------------------------------------------------------------------------------
def maps(h, w):
    """The four stages' map sizes of an h x w frame (floors: stem / 4, every downsample / 2)."""
    return [(h // 4 >> s, w // 4 >> s) for s in range(4)]


def tap_coverage(h, w, ts):
    """(the set of (y % ts, x % ts, ky, kx) over the h x w map whose input (y + ky - 3, x + kx - 3) is in the frame,
    whether a tile exists whose whole (ts + 6)^2 input window is in the frame)."""
    def along(n):
        return {(p % ts, k) for p in range(n) for k in range(7) if 0 <= p + k - 3 < n}

    def interior(n):
        return any(t * ts - 3 >= 0 and t * ts + ts + 2 < n for t in range(-(-n // ts)))
    ys, xs = along(h), along(w)
    return {(oy, ox, ky, kx) for oy, ky in ys for ox, kx in xs}, interior(h) and interior(w)


def tiles_per_frame(h, w, ts):
    return -(-h // ts) * -(-w // ts)


def groups_per_workgroup(c):
    return THREADS // (c // 4)


# ---- bars -------------------------------------------------------------------------------------------------------------------
def bar_ratio(got, want, rtol, atol_scale):
    """max over the elements of |got - want| / (rtol |want| + atol_scale max|want|); a non-finite element counts as infinite."""
    got, want = cn.f64(got), cn.f64(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    err[~np.isfinite(got)] = np.inf
    return float((err / (rtol * np.abs(want) + atol_scale * np.abs(want).max())).max())


# ---- float64 with a chosen eps; float32 in the kernels' orders ----------------------------------------------------------------
def layer_norm64(x, w, b, eps=cn.LN_EPS):
    x = cn.f64(x)
    mean = x.mean(axis=-1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
    with np.errstate(divide='ignore', invalid='ignore'):
        return (x - mean) / np.sqrt(var + eps) * cn.f64(w) + cn.f64(b)


def _group_sum32(q):
    """q [..., C / 4] float32, one value per lane of a pixel -> [..., 1]: the xor butterfly inside a wave (adjacent pairs, then
    pairs of pairs, ...), then the waves' sums in ascending order."""
    lanes = q.shape[-1]
    s = q.reshape(q.shape[:-1] + (max(lanes // 64, 1), min(lanes, 64)))
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    s = s[..., 0]
    total = s[..., 0]
    for k in range(1, s.shape[-1]):
        total = total + s[..., k]
    assert total.dtype == f32
    return total[..., None]


def layer_norm32(x, w, b, eps=cn.LN_EPS, one_pass=False):
    """The kernels' LayerNorm in float32: a lane's ((v0 + v1) + v2) + v3, _group_sum32, mean = sum / C, the same over the squared
    deviations.  one_pass: the variance as E[x^2] - mean^2 from the same reductions instead -- the mutation."""
    x, w, b = (np.asarray(a, dtype=f32) for a in (x, w, b))
    c = x.shape[-1]
    q = x.reshape(x.shape[:-1] + (c // 4, 4))

    def total(v):
        return _group_sum32(((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3])[..., None]
    mean = total(q) / f32(c)
    d = q - mean
    var = total(q * q) / f32(c) - mean * mean if one_pass else total(d * d) / f32(c)
    with np.errstate(divide='ignore', invalid='ignore'):
        y = d * (f32(1.0) / np.sqrt(var + f32(eps))) * w.reshape(c // 4, 4) + b.reshape(c // 4, 4)
    assert y.dtype == f32
    return y.reshape(x.shape)


def dwconv7_chain32(x, w, b):
    """The depthwise conv as the kernel sums it: per output one fmaf chain from the bias, ky-major, kx inside.  (fmaf as a float64
    product and sum rounded once more to float32: the product is exact, the double rounding differs from fmaf in rare ties.)"""
    x = np.asarray(x, dtype=f32)
    n, h, wd, c = x.shape
    xp = np.zeros((n, h + 6, wd + 6, c))
    xp[:, 3:3 + h, 3:3 + wd] = x
    wt = cn.f64(np.asarray(w, dtype=f32))
    acc = np.broadcast_to(np.asarray(b, dtype=f32), x.shape).copy()
    for ky in range(7):
        for kx in range(7):
            acc = (xp[:, ky:ky + h, kx:kx + wd] * wt[:, 0, ky, kx] + acc).astype(f32)
    return acc


def stem_conv32(x_nchw, w, b):
    """The stem's conv as a float32 GEMM with the bias added behind it: the 48 products summed (here in float64, rounded once: a
    GEMM's own order loses far less than the bias add under a common offset) and the float32 bias added to the float32 sum."""
    x = cn.f64(np.asarray(x_nchw, dtype=f32)).transpose(0, 2, 3, 1)
    return cn.patch_conv(x, np.asarray(w, dtype=f32), np.zeros(len(b)), 4).astype(f32) + np.asarray(b, dtype=f32)


# ---- the LayerNorm sites of a model --------------------------------------------------------------------------------------------
class Site(collections.namedtuple('Site', 'tap key pre64 pre32 finish w b')):
    """One LayerNorm of the network, seen from the engine's tap in front of it.  tap: the engine tap that holds its output (for a
    downsample: behind the 2x2 conv); key: its state dict prefix; pre64() / pre32(): what it reads, in float64 and as the kernel
    forms it in float32, both from the float32 tensor in front; finish: from its output to the tap."""

    def variance(self):
        z = self.pre64()
        return ((z - z.mean(axis=-1, keepdims=True)) ** 2).mean(axis=-1)

    def want(self, eps=cn.LN_EPS):
        return self.finish(layer_norm64(self.pre64(), self.w, self.b, eps))

    def emulated(self, one_pass=False):
        return self.finish(layer_norm32(self.pre32(), self.w, self.b, one_pass=one_pass))


def block_inputs(depths):
    """{block name: the tap that is its input}."""
    out, prev = {}, 'stem'
    for s, nb in enumerate(depths):
        if s > 0:
            prev = f'stages.{s}.downsample'
        for b in range(nb):
            out[f'stages.{s}.blocks.{b}'] = prev
            prev = f'stages.{s}.blocks.{b}'
    return out


def ln_sites(sd, x_nchw, depths):
    """{tap: Site} of every LayerNorm of the model on x [n, 3, H, W]: 'stem', every '<block>.dwln', the three
    'stages.S.downsample' and 'head.norm'.  The tensors in front come from the float64 model, rounded to float32 as a tap is."""
    inputs = block_inputs(depths)
    ref = cn.forward(sd, x_nchw, depths, keep=tuple(inputs) + tuple(f'stages.{s}.downsample' for s in (1, 2, 3)))
    sites = {}

    def add(tap, key, pre64, pre32, finish=lambda y: cn.f64(y)):
        sites[tap] = Site(tap, key, pre64, pre32, finish, sd[key + '.weight'], sd[key + '.bias'])
    add('stem', 'stem.1', lambda: cn.patch_conv(cn.f64(x_nchw).transpose(0, 2, 3, 1), sd['stem.0.weight'], sd['stem.0.bias'], 4),
        lambda: stem_conv32(x_nchw, sd['stem.0.weight'], sd['stem.0.bias']))
    for blk, src in inputs.items():
        xin = ref[src].astype(f32)
        add(blk + '.dwln', blk + '.norm', lambda xin=xin, blk=blk: cn.dwconv7(xin, sd[blk + '.conv_dw.weight'], sd[blk + '.conv_dw.bias']),
            lambda xin=xin, blk=blk: dwconv7_chain32(xin, sd[blk + '.conv_dw.weight'], sd[blk + '.conv_dw.bias']))
    for s in (1, 2, 3):
        xin = ref[f'stages.{s - 1}.blocks.{depths[s - 1] - 1}'].astype(f32)
        p = f'stages.{s}.downsample'
        add(p, p + '.0', lambda xin=xin: cn.f64(xin), lambda xin=xin: xin,
            lambda y, p=p: cn.patch_conv(y, sd[p + '.1.weight'], sd[p + '.1.bias'], 2))
    pool = ref['head.pool'].astype(f32)
    add('head.norm', 'head.norm', lambda: cn.f64(pool), lambda: pool)
    return sites


def operator_cases(sd, depths, x, tap):
    """(tap name, operator, float64 result) of every operator of the model on x [n, 1, 3, H, W], each computed from the engine's own
    tap in front of it (``tap(name)``): the stem, per block dwconv7 + LayerNorm, fc1 + GELU and fc2 + layer scale + residual, the
    three downsamples (LayerNorm + 2x2 conv), the pool and the head LayerNorm.  The taps' shapes are asserted on the way."""
    n, sizes = x.shape[0], maps(x.shape[-2], x.shape[-1])
    assert tap('stem').shape == (n,) + sizes[0] + (128,)
    yield 'stem', 'stem', cn.stem(sd, x[:, 0])
    for blk, src in block_inputs(depths).items():
        s = int(blk.split('.')[1])
        c = cn.WIDTHS[s]
        xin = tap(src)
        assert xin.shape == (n,) + sizes[s] + (c,), (blk, xin.shape)
        yield blk + '.dwln', f'dwln{c}', cn.layer_norm(cn.dwconv7(xin, sd[blk + '.conv_dw.weight'], sd[blk + '.conv_dw.bias']),
                                                      sd[blk + '.norm.weight'], sd[blk + '.norm.bias'])
        assert tap(blk + '.fc1').shape == (n,) + sizes[s] + (4 * c,)
        yield blk + '.fc1', 'fc1+gelu', cn.gelu(cn.linear(tap(blk + '.dwln'), sd[blk + '.mlp.fc1.weight'], sd[blk + '.mlp.fc1.bias']))
        yield blk, 'fc2+residual', cn.f64(xin) + cn.f64(sd[blk + '.gamma']) * cn.linear(tap(blk + '.fc1'), sd[blk + '.mlp.fc2.weight'],
                                                                                       sd[blk + '.mlp.fc2.bias'])
    for s in (1, 2, 3):
        yield f'stages.{s}.downsample', 'downsample', cn.downsample(sd, s, tap(f'stages.{s - 1}.blocks.{depths[s - 1] - 1}'))
        assert tap(f'stages.{s}.downsample').shape == (n,) + sizes[s] + (cn.WIDTHS[s],)
    pool, _ = cn.head_norm(sd, tap(f'stages.3.blocks.{depths[3] - 1}'))
    yield 'head.pool', 'pool', pool.reshape(n, 1, 1, 1024)
    _, norm = cn.head_norm(sd, tap('head.pool').reshape(n, 1, 1, 1024))
    yield 'head.norm', 'head.norm', norm.reshape(n, 1, 1, 1024)


LN_OPERATORS = ('stem', 'dwln128', 'dwln256', 'dwln512', 'dwln1024', 'downsample', 'head.norm')      # those of operator_cases that hold a LayerNorm


# ---- crafted state dicts ----------------------------------------------------------------------------------------------------
SMALL_SHIFT = -9           # the small-signal dict: 2^-9, a standard deviation of 1e-3 .. 3e-3 in front of every LayerNorm (eps = 1e-6)
EPS_MUTATIONS = (1e-5, 0.0, 2e-6)


def small_signal_sd(sd, depths, shift=SMALL_SHIFT):
    """The tensors that set the size of what a LayerNorm reads, times 2^shift (exact): the stem conv, the stem LayerNorm's affine,
    every conv_dw.bias, every gamma and every downsample conv.  The residual stream and every conv in front of a LayerNorm then
    carry 2^shift of their seeded size; the LayerNorms inside the blocks keep their affine, so the MLPs see ordinary numbers."""
    out, k = dict(sd), f32(2.0 ** shift)
    names = ['stem.0.weight', 'stem.0.bias', 'stem.1.weight', 'stem.1.bias']
    names += [f'stages.{s}.downsample.1.{t}' for s in (1, 2, 3) for t in ('weight', 'bias')]
    for blk in block_inputs(depths):
        names += [blk + '.conv_dw.bias', blk + '.gamma']
    for name in names:
        out[name] = sd[name] * k
    return out


def offset_sd(sd, adds):
    """sd with K added to every element of the named tensors: adds = {name: K}."""
    out = dict(sd)
    for name, k in adds.items():
        out[name] = (sd[name] + f32(k)).astype(f32)
    return out


# Common offsets, a power of two per site: the float32 two-pass emulation stays under a quarter of the per-op bar while the
# one-pass emulation exceeds it three times -- scanning each offset alone, the largest power of two that meets both with every
# smaller one down to where one pass stops failing (tests/test_convnext_cases_cpu.py asserts both and holds the table).
# Three dicts, since an offset must reach its LayerNorm without sitting in the tap that is compared: 'front' carries the stem's
# and the fused kernel's (the LayerNorm removes it at once), 'even' and 'odd' put it into the residual stream of alternate
# stages so that every downsample's and the head's LayerNorm read it while the conv behind them has its seeded bias.
OFFSET_DICTS = {
    'front': {'stem': ('stem.0.bias', 256), 'stages.0.blocks.0.dwln': ('stages.0.blocks.0.conv_dw.bias', 128),
              'stages.1.blocks.0.dwln': ('stages.1.blocks.0.conv_dw.bias', 128), 'stages.2.blocks.0.dwln': ('stages.2.blocks.0.conv_dw.bias', 128),
              'stages.2.blocks.1.dwln': ('stages.2.blocks.1.conv_dw.bias', 128), 'stages.3.blocks.0.dwln': ('stages.3.blocks.0.conv_dw.bias', 128)},
    'even': {'stages.1.downsample': ('stem.1.bias', 256), 'stages.3.downsample': ('stages.2.downsample.1.bias', 256)},
    'odd': {'stages.2.downsample': ('stages.1.downsample.1.bias', 256), 'head.norm': ('stages.3.downsample.1.bias', 512)},
}
TWO_PASS_SHARE, ONE_PASS_TIMES = 0.25, 3.0


def offset_dict(sd, which, scale=1):
    """The state dict of OFFSET_DICTS[which] (every offset times ``scale``: the CPU test looks at 2 K as well)."""
    return offset_sd(sd, {name: k * scale for name, k in OFFSET_DICTS[which].values()})


def dead_rows_sd(sd):
    """conv_dw.weight = 0 and conv_dw.bias = 0.75 in the first block of every stage: the conv's output is 0.75 in every channel,
    every partial sum of the LayerNorm is exact (0.75 * 2^k), every deviation exactly 0, and .dwln is norm.bias to the bit."""
    out = dict(sd)
    for s in range(4):
        p = f'stages.{s}.blocks.0.conv_dw.'
        out[p + 'weight'] = np.zeros_like(sd[p + 'weight'])
        out[p + 'bias'] = np.full_like(sd[p + 'bias'], 0.75)
    return out


# ---- GELU on chosen inputs ----------------------------------------------------------------------------------------------------
GELU_SHIFTS = (1, 0, -1, -2)
GELU_SPECIALS = np.array([0.0, -0.0, 1e-30, -1e-30, 8.0, -8.0, 12.0, -12.0, 40.0, -40.0, 1e4, -1e4], dtype=f32)
# |got - want| <= GELU_RTOL |want| + GELU_ATOL: four times what gelu_formula32 loses on these inputs (gelu_yardstick: 4.30e-7
# absolute over all of them, 9.06e-8 relative over x >= 4), the factor for the difference between erf implementations
GELU_RTOL, GELU_ATOL = 3.62e-7, 1.72e-6


def gelu_rows(stage):
    """norm.bias of the crafted block of ``stage``: the special values, then one uniform draw from each of C - 12 equal cells of
    [-3, 3]; the four power-of-two rows of fc1 spread them over [-6, 6], densest where the approximations of GELU are worst."""
    m = cn.WIDTHS[stage] - GELU_SPECIALS.size
    rng = np.random.default_rng([97, stage])
    return np.concatenate([GELU_SPECIALS, (-3.0 + 6.0 * (np.arange(m) + rng.uniform(0.0, 1.0, m)) / m).astype(f32)])


def gelu_inputs(stage):
    """The 4 C pre-activations of the crafted block, exact: x[o] = b[o % C] * 2^GELU_SHIFTS[o // C]."""
    b = gelu_rows(stage)
    return np.concatenate([b * f32(2.0 ** k) for k in GELU_SHIFTS])


def gelu_sd(sd):
    """The first block of every stage turned into a table of GELU inputs: norm.weight = 0 and norm.bias = b make .dwln b in every
    pixel, fc1 is a selection (row o: 2^k at column o % C, bias 0), so fc1's output o is b[o % C] * 2^k without rounding -- every
    other product is an exact zero.  gamma = 0: the block hands its input on, whatever the GELU of 1e4 would do to the stream."""
    out = dict(sd)
    for s, c in enumerate(cn.WIDTHS):
        p = f'stages.{s}.blocks.0.'
        w = np.zeros((4 * c, c), dtype=f32)
        o = np.arange(4 * c)
        w[o, o % c] = np.repeat(f32(2.0) ** np.array(GELU_SHIFTS, dtype=f32), c)
        out.update({p + 'norm.weight': np.zeros(c, dtype=f32), p + 'norm.bias': gelu_rows(s), p + 'mlp.fc1.weight': w,
                    p + 'mlp.fc1.bias': np.zeros(4 * c, dtype=f32), p + 'gamma': np.zeros(c, dtype=f32)})
    return out


def gelu_formula32(x):
    """The kernel's formula in float32 on the CPU (torch): 0.5 x (1 + erf(x * 0.70710678f)) -- the yardstick of the bar."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=f32))
    y = (0.5 * t) * (1.0 + torch.erf(t * f32(0.70710678118654752440)))
    assert y.dtype == torch.float32
    return y.numpy()


def gelu_tanh(x):
    x = cn.f64(x)
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_sigmoid(x):
    x = cn.f64(x)
    with np.errstate(over='ignore'):
        return x / (1.0 + np.exp(-1.702 * x))


def gelu_yardstick(x):
    """(worst absolute error of gelu_formula32 over x, its worst relative error over x >= 4) against the float64 exact GELU."""
    want = cn.gelu(x)
    err = np.abs(cn.f64(gelu_formula32(x)) - want)
    tail = np.asarray(x) >= 4.0
    return float(err.max()), float((err[tail] / want[tail]).max())


def gelu_ratio(got, want):
    """max |got - want| / (GELU_RTOL |want| + GELU_ATOL)."""
    got, want = cn.f64(got), cn.f64(want)
    err = np.abs(got - want)
    err[~np.isfinite(got)] = np.inf
    return float((err / (GELU_RTOL * np.abs(want) + GELU_ATOL)).max())
