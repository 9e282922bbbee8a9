"""The preconditions of tests/test_convnext_edges_gpu.py, without a GPU: what its frames reach inside dwconv7_ln_kernel's tile,
and that every crafted case (tests/_convnext_cases.py) separates the kernels' documented arithmetic -- emulated in float32 -- from
its near misses: eps = 1e-5, 0 and 2e-6, a one-pass variance, the tanh and the sigmoid form of GELU.  Each near miss must fail
the very bar the GPU test applies, and the emulation must use a small stated share of it."""
import functools

import numpy as np
import pytest

from tests import _convnext as cn
from tests import _convnext_cases as cc
from tests._util import assert_close
from workoutdetector_amd import weights

SHALLOW = (1, 1, 2, 1)
SUITE_SIZES = ((64, 64), (80, 80), (36, 36), (64, 96))          # tests/test_convnext_gpu.py: SIZES
OP_BAR = dict(rtol=1e-4, atol_scale=1e-4)                       # tests/test_convnext_gpu.py: OP_BAR


@functools.lru_cache(maxsize=None)
def _sd():
    sd = weights.make_state_dict(0, 5, 'convnext_base', depths=SHALLOW)
    for v in sd.values():
        v.setflags(write=False)
    return sd


def _sites(sd):
    return cc.ln_sites(sd, cc.noise(64, 64)[:, 0], SHALLOW)


ALL_SITES = ('stem', 'stages.0.blocks.0.dwln', 'stages.1.blocks.0.dwln', 'stages.2.blocks.0.dwln', 'stages.2.blocks.1.dwln',
             'stages.3.blocks.0.dwln', 'stages.1.downsample', 'stages.2.downsample', 'stages.3.downsample', 'head.norm')


# ---- A. coverage ----------------------------------------------------------------------------------------------------------------
def test_the_tile_is_fully_walked_at_176x224_and_not_by_the_small_frames():
    """(accumulator, tap) pairs of the TS x TS tile that ever multiply an in-frame input.  The small frames of test_convnext_gpu.py:
    784, 784, 548 of 784 and 32 of 196; 176 x 224: all of them in every width, with an interior tile (its whole (TS + 6)^2 window
    in the frame) at C = 128, 256 and 512 -- the 5 x 7 map of C = 1024 cannot hold one."""
    assert [cc.DW_TILE[c] for c in cn.WIDTHS] == [4, 4, 4, 2]
    assert cc.maps(176, 224) == [(44, 56), (22, 28), (11, 14), (5, 7)] and cc.maps(224, 224) == [(56, 56), (28, 28), (14, 14), (7, 7)]
    before, after, interior_before, interior_after = [], [], [], []
    for s, c in enumerate(cn.WIDTHS):
        ts = cc.DW_TILE[c]
        small = [cc.tap_coverage(*cc.maps(h, w)[s], ts) for h, w in SUITE_SIZES]
        before.append(len(set().union(*(pairs for pairs, _ in small))))
        interior_before.append(any(inner for _, inner in small))
        pairs, inner = cc.tap_coverage(*cc.maps(176, 224)[s], ts)
        assert all(0 <= oy < ts and 0 <= ox < ts and 0 <= ky < 7 and 0 <= kx < 7 for oy, ox, ky, kx in pairs)
        after.append(len(pairs))
        interior_after.append(inner)
    assert before == [784, 784, 548, 32] and interior_before == [True, False, False, False]
    assert after == [784, 784, 784, 196] and interior_after == [True, True, True, False]
    # the counting itself, on maps small enough to do by hand: one pixel sees its centre tap only; a 4 x 4 map under one 4 x 4 tile
    # pairs accumulator p with the taps 3 - p .. 6 - p along each side, 4 x 4 of them per side in all
    assert cc.tap_coverage(1, 1, 2) == ({(0, 0, 3, 3)}, False)
    assert len(cc.tap_coverage(4, 4, 4)[0]) == 16 * 16 and cc.tap_coverage(11, 11, 4)[1] and not cc.tap_coverage(10, 11, 4)[1]


def test_workgroups_hold_tiles_of_two_frames_at_176x176():
    """Tiles are numbered frame-major over the launch and a workgroup takes 1024 / C of them in a row: it holds tiles of two frames
    when the tiles of a frame are no multiple of that.  176 x 176: 121 tiles against 8 groups at C = 128, 9 against 2 at C = 512;
    the 80 x 80 frame of the existing batch test has 4 tiles at C = 512."""
    counts = [cc.tiles_per_frame(*cc.maps(176, 176)[s], cc.DW_TILE[c]) for s, c in enumerate(cn.WIDTHS)]
    groups = [cc.groups_per_workgroup(c) for c in cn.WIDTHS]
    assert counts == [121, 36, 9, 9] and groups == [8, 4, 2, 1]
    assert counts[0] % groups[0] and counts[2] % groups[2]
    assert cc.tiles_per_frame(*cc.maps(80, 80)[2], 4) % groups[2] == 0


# ---- the emulations -------------------------------------------------------------------------------------------------------------
def test_the_float32_emulations_follow_the_documented_orders():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 512)).astype(np.float32)
    w, b = rng.uniform(0.8, 1.2, 512).astype(np.float32), rng.standard_normal(512).astype(np.float32)
    assert np.array_equal(cc.layer_norm64(x, w, b), cn.layer_norm(x, w, b))
    # the reduction against a lane-by-lane replay of group_sum<512>: xor shuffles inside each wave of 64, then the two waves' sums
    lane = ((x[:, 0::4] + x[:, 1::4]) + x[:, 2::4]) + x[:, 3::4]
    v = lane.copy()
    for off in (1, 2, 4, 8, 16, 32):
        v = v + v[:, np.arange(128) ^ off]
    assert (v[:, :64] == v[:, :1]).all() and (v[:, 64:] == v[:, 64:65]).all()
    assert np.array_equal(cc._group_sum32(lane)[:, 0], v[:, 0] + v[:, 64])
    for c in cn.WIDTHS:
        xc = rng.standard_normal((5, c)).astype(np.float32)
        wc, bc = np.ones(c, np.float32), np.zeros(c, np.float32)
        assert_close(cc.layer_norm32(xc, wc, bc), cn.layer_norm(xc, wc, bc), rtol=1e-5, atol_scale=1e-6, what=f'two passes, C = {c}')
        assert_close(cc.layer_norm32(xc, wc, bc, one_pass=True), cn.layer_norm(xc, wc, bc), rtol=1e-5, atol_scale=1e-6, what=f'one pass, C = {c}')
    xi = rng.standard_normal((1, 6, 5, 8)).astype(np.float32)
    wi, bi = rng.standard_normal((8, 1, 7, 7)).astype(np.float32), rng.standard_normal(8).astype(np.float32)
    assert_close(cc.dwconv7_chain32(xi, wi, bi), cn.dwconv7(xi, wi, bi), rtol=1e-5, atol_scale=1e-6, what='fmaf chain')
    assert_close(cc.stem_conv32(cc.noise(64, 64)[:, 0], _sd()['stem.0.weight'], _sd()['stem.0.bias']),
                 cn.patch_conv(cc.noise(64, 64)[:, 0].transpose(0, 2, 3, 1), _sd()['stem.0.weight'], _sd()['stem.0.bias'], 4), rtol=1e-6, atol_scale=1e-6)
    assert cc.bar_ratio([1.0, 2.0 + 3e-4], [1.0, 2.0], **OP_BAR) == pytest.approx(3e-4 / 4e-4) and cc.bar_ratio([np.nan], [1.0], **OP_BAR) == np.inf


# ---- B. LayerNorm ---------------------------------------------------------------------------------------------------------------
def test_small_signal_puts_every_variance_at_eps_and_fails_every_other_eps(capsys):
    """cc.small_signal_sd (2^-9) on the float64 model: the channel variance of every row in front of every LayerNorm lies in
    0.1 eps .. 10 eps (measured 0.25 .. 6.9 eps).  At the per-op bar the float32 two-pass emulation then uses under a tenth
    (measured 0.0016 at the most) while eps = 1e-5, 0 and 2e-6 in float64 miss it at every site (measured 500 to 6 000 times).  The seeded
    dict itself has no variance under 0.08 (80 000 eps) and lets all three pass: the contrast."""
    sites = _sites(cc.small_signal_sd(_sd(), SHALLOW))
    assert tuple(sorted(sites)) == tuple(sorted(ALL_SITES))
    lines = []
    for tap in ALL_SITES:
        s = sites[tap]
        var, want = s.variance(), s.want()
        emu = cc.bar_ratio(s.emulated(), want, **OP_BAR)
        miss = [cc.bar_ratio(s.want(eps), want, **OP_BAR) for eps in cc.EPS_MUTATIONS]
        lines.append(f'{tap}: variance {var.min() / cn.LN_EPS:.3g} .. {var.max() / cn.LN_EPS:.3g} eps, two-pass {emu:.2g}, '
                     + ', '.join(f'eps {e:g}: {m:.3g}' for e, m in zip(cc.EPS_MUTATIONS, miss)))
        assert 0.1 * cn.LN_EPS <= var.min() and var.max() <= 10 * cn.LN_EPS, lines[-1]
        assert emu < 0.1 and min(miss) > 1.0, lines[-1]
    with capsys.disabled():
        print('\n[convnext small signal, shares of the per-op bar]\n  ' + '\n  '.join(lines))
    plain = _sites(_sd())
    for tap in ALL_SITES:
        s = plain[tap]
        assert s.variance().min() > 0.08 and max(cc.bar_ratio(s.want(eps), s.want(), **OP_BAR) for eps in cc.EPS_MUTATIONS) < 1.0, tap


@pytest.mark.parametrize('which', sorted(cc.OFFSET_DICTS))
def test_offsets_pass_two_passes_and_fail_one(which, capsys):
    """Per site of cc.OFFSET_DICTS the common offset K, at the per-op bar: the float32 emulation in the documented order (for the
    fused kernel the fmaf chain from the bias, ky-major with kx inside, then two passes) stays under a quarter and the one-pass
    emulation misses it at least three times.  K came from a scan of each offset alone over the powers of two: the largest that
    meets both conditions with every smaller one down to where one pass stops failing; the next power of two is printed beside
    it.  (The sites with few rows -- head.norm has two, stages.3.downsample eight -- jump with the rounding of a row's mean: alone,
    1024 in front of head.norm and 512 in front of stages.3.downsample use 0.44 and 0.35 of the bar, in these dicts 0.11 and 0.21.)

        site                      K    two-pass  one-pass    two-pass at 2 K
        stem                      256  0.11      51          0.27
        stages.0.blocks.0.dwln    128  0.21      19          0.40
        stages.1.blocks.0.dwln    128  0.20      16          0.40
        stages.2.blocks.0.dwln    128  0.17      22          0.40
        stages.2.blocks.1.dwln    128  0.23      16          0.48
        stages.3.blocks.0.dwln    128  0.19      69          0.34
        stages.1.downsample       256  0.17      45          0.35
        stages.2.downsample       256  0.17      41          0.46
        stages.3.downsample       256  0.11      33          0.21
        head.norm                 512  0.079     137         0.11
    """
    entries = cc.OFFSET_DICTS[which]
    at_k, at_2k = _sites(cc.offset_dict(_sd(), which)), _sites(cc.offset_dict(_sd(), which, scale=2))
    lines = []
    for tap, (name, k) in entries.items():
        assert k & (k - 1) == 0 and np.array_equal(cc.offset_dict(_sd(), which)[name], _sd()[name] + np.float32(k))
        want = at_k[tap].want()
        two, one = cc.bar_ratio(at_k[tap].emulated(), want, **OP_BAR), cc.bar_ratio(at_k[tap].emulated(one_pass=True), want, **OP_BAR)
        two_2k = cc.bar_ratio(at_2k[tap].emulated(), at_2k[tap].want(), **OP_BAR)
        lines.append(f'{tap}: K = {k}, two-pass {two:.2g}, one-pass {one:.3g}; at 2 K two-pass {two_2k:.2g}')
        assert two < cc.TWO_PASS_SHARE and one >= cc.ONE_PASS_TIMES, lines[-1]
    with capsys.disabled():
        print(f'\n[convnext offsets {which}, shares of the per-op bar]\n  ' + '\n  '.join(lines))


def test_dead_rows_are_the_norm_bias_in_the_emulation_and_nan_without_eps():
    sd = cc.dead_rows_sd(_sd())
    sites = _sites(sd)
    for s in range(4):
        site = sites[f'stages.{s}.blocks.0.dwln']
        conv = site.pre32()
        assert (conv == np.float32(0.75)).all() and (site.variance() == 0).all()
        assert np.array_equal(site.emulated().astype(np.float32).view(np.uint32), np.broadcast_to(sd[f'stages.{s}.blocks.0.norm.bias'], conv.shape).view(np.uint32))
        assert np.isnan(site.want(eps=0.0)).all()


# ---- C. GELU ----------------------------------------------------------------------------------------------------------------------
def test_gelu_inputs_bar_and_mutations(capsys):
    """The 7 680 inputs of the crafted blocks (7 500 distinct): no gap over 0.03 inside [-6, 6], the specials and their multiples,
    nothing non-finite.  The bar |err| <= GELU_RTOL |want| + GELU_ATOL is four times the yardstick, the kernel's own formula in
    float32 on the CPU against the float64 exact GELU: worst absolute error 4.30e-7 over all inputs (ATOL 1.72e-6), worst
    relative error 9.06e-8 over x >= 4 (RTOL 3.62e-7; in the negative tail 1 + erf cancels and the relative error is percents, in
    torch's own float32 GELU too: only ATOL bounds it).  The tanh form misses this bar 275 times, x sigmoid(1.702 x) 11 800 times."""
    xs = np.concatenate([cc.gelu_inputs(s) for s in range(4)])
    assert xs.dtype == np.float32 and xs.size == 4 * sum(cn.WIDTHS) == 7680 and np.isfinite(xs).all() and np.unique(xs).size > 7000
    inner = np.sort(xs[np.abs(xs) <= 6.0])
    assert inner[0] < -5.97 and inner[-1] > 5.97 and np.diff(inner).max() < 0.03
    for v in cc.GELU_SPECIALS:
        assert (xs.view(np.uint32) == np.float32(v).view(np.uint32)).sum() >= 4, v          # (bit patterns: -0.0 is not +0.0)
    for s in range(4):                                                                        # exact: a float64 product says the same
        assert np.array_equal(cn.f64(cc.gelu_inputs(s)), np.concatenate([cn.f64(cc.gelu_rows(s)) * 2.0 ** k for k in cc.GELU_SHIFTS]))
        w = cc.gelu_sd(_sd())[f'stages.{s}.blocks.0.mlp.fc1.weight']
        assert ((w != 0).sum(axis=1) == 1).all() and np.array_equal(cn.f64(w) @ cn.f64(cc.gelu_rows(s)), cn.f64(cc.gelu_inputs(s)))
    worst_abs, worst_rel = cc.gelu_yardstick(xs)
    assert 4.0 * worst_abs == pytest.approx(cc.GELU_ATOL, rel=0.02) and 4.0 * worst_rel == pytest.approx(cc.GELU_RTOL, rel=0.02), (worst_abs, worst_rel)
    want = cn.gelu(xs)
    own, tanh, sigmoid = (cc.gelu_ratio(f(xs), want) for f in (cc.gelu_formula32, cc.gelu_tanh, cc.gelu_sigmoid))
    with capsys.disabled():
        print(f'\n[convnext gelu bar] yardstick abs {worst_abs:.3g} rel {worst_rel:.3g}; shares of the bar: own formula {own:.3g}, tanh {tanh:.4g}, sigmoid {sigmoid:.4g}')
    assert own <= 0.25 + 1e-9 and tanh >= 100.0 and sigmoid >= 100.0
    assert np.array_equal(cc.gelu_formula32(xs)[xs >= 1e4], xs[xs >= 1e4]) and (want[xs <= -40] == 0).all() and (want[xs == 0] == 0).all()
