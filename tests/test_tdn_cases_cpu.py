"""The preconditions of tests/test_tdn_edges_gpu.py, without a GPU: that each crafted case of tests/_tdn_cases.py reaches what it is
meant to reach, that a float32 implementation fits the bars on it, and that the near misses it is there to catch do not.  All of it
is the float64 tests/_tdn.py (pinned to the reference by tests/test_tdn_cpu.py) and float32 copies of the same networks."""
import re

import numpy as np
import pytest
import torch

from tests import _tdn
from tests import _tdn_cases as tc

QUARTER = 0.25          # the share of a bar a float32 copy of the network may use
MISS = 100.0            # a near miss must exceed its bar this many times


def _gate_figures(taps):
    return {k[:-len('.mse.e')]: (float(v.numpy().std()), float((np.abs(v.numpy()) > 4).mean())) for k, v in taps.items() if k.endswith('.mse.e')}


def _emulation_shares(h, w, depths, T, n, recipe):
    """(logits, worst tap): the float32 copy's error over the bars."""
    logits, taps = tc.reference(h, w, depths, T, n, recipe)
    logits32, taps32 = tc.emulated(h, w, depths, T, n, recipe)
    worst = tc.worst_taps(taps32, taps, tc.tap_names(depths))
    return tc.bar_ratio(logits32, logits, **tc.LOGITS_BAR), max(worst.values())


def _gate_shares(h, w, depths, T, n, recipe):
    """{block: the float32 module's error over OP_BAR}: g, m+ and m- from the float64 network's conv1 tap rounded to float32."""
    _logits, taps = tc.reference(h, w, depths, T, n, recipe)
    m64, m32 = tc.network(depths, T, recipe)[0], tc.network(depths, T, recipe, torch.float32)[0]
    out = {}
    for li, b in tc.shift_blocks(depths):
        c1 = taps[f'layer{li}.{b}.conv1'].astype(np.float32)
        out[f'layer{li}.{b}'] = max(tc.bar_ratio(g, wnt, **tc.OP_BAR) for g, wnt in zip(tc.gate64(m32, li, b, c1), tc.gate64(m64, li, b, c1)))
    return out


# ---- 0. the recipes -------------------------------------------------------------------------------------------------------------
def test_recipes_change_what_they_name_and_nothing_else():
    plain = tc.network(tc.D96, 3)[1]
    golden_model, golden_w = _tdn.build(tc.NUM_CLASS, 3, tc.D96, tc.SEED)
    assert all(np.array_equal(plain[k], golden_w[k]) for k in golden_w) and set(plain) == set(golden_w)      # build's defaults stand
    blocks = tc.D96[0] + sum(tc.D96)          # resnext_layer1 and the trunk
    for recipe, changed, factor in (('damped', r'.bn3.weight', tc.RESIDUAL_GAIN), ('saturated', '.mse.bn3.', tc.GATE_GAIN)):
        w = tc.network(tc.D96, 3, recipe)[1]
        diff = [k for k in plain if not np.array_equal(plain[k], w[k])]
        assert all(changed in k and ('.mse.' in k) == (recipe == 'saturated') for k in diff), diff
        assert len(diff) == (blocks if recipe == 'damped' else 2 * sum(tc.D96[1:]))
        assert all(np.array_equal(w[k], plain[k] * np.float32(factor)) and w[k].dtype == np.float32 for k in diff)
    w = tc.network(tc.D96, 3, 'small_variance')[1]
    diff = [k for k in plain if not np.array_equal(plain[k], w[k])]
    n_bn = sum(k.endswith('running_var') for k in plain)
    assert len(diff) == 2 * n_bn and all(k.endswith(('running_var', '.weight')) for k in diff)
    for k in diff:
        if k.endswith('running_var'):
            assert w[k].dtype == np.float32 and 1e-6 <= w[k].min() and w[k].max() <= 1e-4 * (1 + 1e-6), k
            gamma = k[:-len('running_var')] + 'weight'
            # the folded scale is the seeded weight again, to float32 rounding: the network keeps its size
            scale = w[gamma].astype(np.float64) / np.sqrt(w[k].astype(np.float64) + 1e-5)
            assert np.abs(scale / plain[gamma] - 1).max() < 1e-6, k
    assert np.log10(np.concatenate([w[k] for k in diff if k.endswith('running_var')])).std() > 0.5      # spread over the two decades
    # the float64 model computes from the float32 arrays the engine loads
    model = tc.network(tc.D96, 3, 'small_variance')[0]
    sd = model.state_dict()
    assert all(sd[k].dtype == torch.float64 and np.array_equal(sd[k].numpy(), w[k].astype(np.float64)) for k in w)


# ---- 1. the real depths ---------------------------------------------------------------------------------------------------------
def test_full_depth_needs_the_damped_residual():
    """Depths (3, 4, 6, 3) at 64 x 96, T = 3, 2 clips.  Damped (bn3.weight x 0.25): every block's gate is neither saturated nor flat
    -- the condition of tests/test_tdn_cpu.py.  Undamped: the activations grow block by block and the condition fails, so the gain
    is not decoration."""
    h, w, depths, T, n = 64, 96, tc.FULL, 3, 2
    logits, taps = tc.reference(h, w, depths, T, n, 'damped')
    figures = _gate_figures(taps)
    assert len(figures) == 13
    for name, (std, share) in figures.items():
        print(f'damped {name}: e std {std:.2f}, |e| > 4 in {share:.3f}')
        assert std >= 0.3 and share <= 0.10, name
    scales = {name: float(np.abs(taps[name]).max()) for name in tc.tap_names(depths)}
    print('damped: largest tap scale %.3g, logit scale %.3g' % (max(scales.values()), np.abs(logits).max()))
    l32, t32 = _emulation_shares(h, w, depths, T, n, 'damped')
    print(f'damped float32 copy: {l32:.3g} of the logits bar, {t32:.3g} of the tap bar')
    assert l32 <= QUARTER and t32 <= QUARTER
    _logits, plain_taps = tc.run(tc.network(depths, T, 'plain')[0], tc.clips(h, w, T, n))
    plain = _gate_figures(plain_taps)
    print('undamped: worst |e| > 4 share %.2f, largest e std %.0f' % (max(s for _d, s in plain.values()), max(d for d, _s in plain.values())))
    assert any(share > 0.10 for _std, share in plain.values())


@pytest.mark.parametrize('depths', [tc.EVEN, tc.FOUR], ids=str)
def test_the_small_depth_cases_fit_the_bars_in_float32(depths):
    """The even arm (2, 1, 1, 1) and a fourth block (4, 1, 1, 2) with the plain recipe: the cases are about run_tdn's buffers, and a
    float32 copy fits the bars with room.  (Four undamped blocks in front saturate layer2.0's gate of (4, 1, 1, 2) -- |e| up to 72,
    inside expf's range; the gate's own cases are the other recipes'.)"""
    logits, taps = tc.reference(64, 64, depths, 3, 2)
    for name, (std, share) in _gate_figures(taps).items():
        print(f'{depths} {name}: e std {std:.2f}, |e| > 4 in {share:.3f}')
    assert max(np.abs(v.numpy()).max() for k, v in taps.items() if k.endswith('.mse.e')) < tc.EXPF_RANGE
    l32, t32 = _emulation_shares(64, 64, depths, 3, 2, 'plain')
    print(f'{depths} float32 copy: {l32:.3g} of the logits bar, {t32:.3g} of the tap bar')
    assert l32 <= QUARTER and t32 <= QUARTER


def test_the_conv_name_count_is_the_engines():
    from workoutdetector_amd import weights
    for depths in (tc.FULL, tc.D96, tc.EVEN):
        convs = [k for k, shape, _kind in weights.tdn_specs(depths) if len(shape) == 4 and '.mse.' not in k]
        assert len(convs) == tc.n_conv_names(depths), depths
    assert tc.n_conv_names(tc.FULL) == 64


# ---- 2. launch-cap wraps ----------------------------------------------------------------------------------------------------------
def test_the_wrap_batch_is_the_smallest_that_wraps_all_three():
    """21 clips of 8 frames at 224 x 224: fuse1, fuse2 and layer2.0's mse_mix_kernel<8> all go round their grid-stride loop again; 20
    clips leave the mix launch inside one pass."""
    one = tc.launch_pass('tdn_fuse_kernel', 'quads')
    assert one == tc.launch_pass('mse_mix_kernel', 'outs') == 16384 * 256 == 4194304
    frames, per = 21 * 8, {'fuse1': 56 * 56 * 16, 'fuse2': 56 * 56 * 64, 'mix': 56 * 56 * 8}
    assert {k: frames * v for k, v in per.items()} == {'fuse1': 8429568, 'fuse2': 33718272, 'mix': 4214784}
    assert tc.wrap_frames(frames, per['fuse1'], one) == [83, 167]
    assert tc.wrap_frames(frames, per['fuse2'], one) == [20, 41, 62, 83, 104, 125, 146, 167]
    assert tc.wrap_frames(frames, per['mix'], one) == [167]
    assert tc.wrap_frames(20 * 8, per['mix'], one) == []
    # the largest launch of tests/test_tdn_gpu.py stays inside one pass: nothing there reaches the second
    assert tc.wrap_frames(24, 24 * 40 * 64, one) == [] and tc.wrap_frames(2, 56 * 56 * 64, one) == []


def test_blend64_is_the_models_blend():
    _logits, taps = tc.reference(96, 160, tc.D96, 3, 2)
    for got, a, d in (('fuse1', 'stem', 'diff.stem'), ('fuse2', 'layer1.0', 'resnext_layer1.0')):
        want, mag = tc.blend64(taps[a].astype(np.float32), taps[d].astype(np.float32), 0.75, 0.25)
        assert np.abs(want - taps[got]).max() <= 2.0 ** -23 * mag.max() and taps[d].shape[1] * 2 == taps[a].shape[1]
        swapped, _mag = tc.blend64(taps[a].astype(np.float32), taps[d].astype(np.float32), 0.25, 0.75)
        assert (np.abs(swapped - taps[got]) > 2.0 ** -23 * mag).mean() > 0.5


# ---- 3. BatchNorm eps -------------------------------------------------------------------------------------------------------------
SV = (96, 160, tc.D96, 3, 2, 'small_variance')


def test_small_variances_keep_the_network_usable():
    h, w, depths, T, n, recipe = SV
    logits, taps = tc.reference(*SV)
    for name, (std, share) in _gate_figures(taps).items():
        print(f'small variance {name}: e std {std:.2f}, |e| > 4 in {share:.3f}')
        assert std >= 0.3 and share <= 0.10, name
    l32, t32 = _emulation_shares(*SV)
    g32 = _gate_shares(*SV)
    print(f'small variance float32 copy: {l32:.3g} of the logits bar, {t32:.3g} of the tap bar, {max(g32.values()):.3g} of the per-operator bar')
    assert l32 <= QUARTER and t32 <= QUARTER and max(g32.values()) <= QUARTER


@pytest.mark.parametrize('eps', tc.EPS_MUTANTS)
def test_another_eps_misses_the_bars(eps):
    """Every BatchNorm with another eps: each family of folds misses the tap bar 100 times over at one tap or more.  Only the four
    BatchNorms of the long-term modules with another eps: the gate computed from the conv1 tap misses the per-operator bar, 100
    times over as well -- but for eps = 1.1e-5, a tenth off, which moves a gate by 1.4 to 1.7 % of its scale: 96 to 103 times the bar, asserted at 50."""
    h, w, depths, T, n, recipe = SV
    logits, taps = tc.reference(*SV)
    x = tc.clips(h, w, T, n)
    got_logits, got = tc.run(tc.mutant(depths, T, recipe, eps=eps), x)
    ratios = tc.worst_taps(got, taps, tc.tap_names(depths))
    print(f'eps {eps:g}: logits move by {tc.moved(got_logits, logits):.3g} of the scale')
    for family, pattern in tc.EPS_FAMILIES.items():
        hit = {k: v for k, v in ratios.items() if re.search(pattern, k)}
        print(f'eps {eps:g}, {family}: {max(hit.values()):.3g} times the tap bar')
        assert hit and max(hit.values()) >= MISS, (family, hit)
    model, only = tc.network(depths, T, recipe)[0], tc.mutant(depths, T, recipe, eps=eps, only_mse=True)
    for li, b in ((2, 0), (3, 0), (4, 1)):
        c1 = taps[f'layer{li}.{b}.conv1'].astype(np.float32)
        g, want = tc.gate64(only, li, b, c1)[0], tc.gate64(model, li, b, c1)[0]
        ratio = tc.bar_ratio(g, want, **tc.OP_BAR)
        print(f'eps {eps:g} in the mSE only, layer{li}.{b}: the gate moves by {tc.moved(g, want):.3g} of its scale, {ratio:.3g} times the bar')
        assert ratio >= (MISS if eps != 1.1e-5 else MISS / 2)


# ---- 4. mixed parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('frame', list(tc.PARITY_FRAMES), ids=str)
def test_layer4_maps_have_mixed_parity(frame):
    (mh, mw), pool = tc.PARITY_FRAMES[frame]
    _logits, taps = tc.reference(*frame, tc.D96, 3, 2)
    assert taps['layer4.1.mse.fwd'].shape == (6, mh, mw, 32) and taps['layer4.1.conv1'].shape == (6, mh, mw, 512)
    assert (mh // 2, mw // 2) == pool and (mh % 2, mw % 2) != (0, 0) and ((mh % 2, mw % 2) != (1, 1) or mh > mw)
    for name, (std, share) in _gate_figures(taps).items():
        assert std >= 0.3 and share <= 0.10, name


# ---- 5. saturated gates -----------------------------------------------------------------------------------------------------------
SAT = (96, 160, tc.D96, 3, 2, 'saturated')


def test_the_saturated_gates_leave_expfs_range_both_ways():
    h, w, depths, T, n, recipe = SAT
    logits, taps = tc.reference(*SAT)
    es = {k: v.numpy() for k, v in taps.items() if k.endswith('.mse.e')}
    assert len(es) == 5 and np.isfinite(logits).all()
    for name, e in es.items():
        over, under, mid = (e > tc.EXPF_RANGE).mean(), (e < -tc.EXPF_RANGE).mean(), (np.abs(e) < 4).mean()
        print(f'saturated {name}: e > 89 in {over:.3f}, e < -89 in {under:.3f}, |e| < 4 in {mid:.3f}, max |e| {np.abs(e).max():.0f}')
        assert over >= 0.01 and under >= 0.01 and mid >= 0.05, name
        # the near miss: exp(e) / (1 + exp(e)) in float32 is inf / inf on these inputs, the documented form is not
        assert not np.isfinite(tc.sigmoid_near_miss32(e)).all()
        with np.errstate(over='ignore'):
            assert np.isfinite(np.float32(1) / (np.float32(1) + np.exp(-e.astype(np.float32)))).all()
    l32, t32 = _emulation_shares(*SAT)
    g32 = _gate_shares(*SAT)
    print(f'saturated float32 copy: {l32:.3g} of the logits bar (scale {np.abs(logits).max():.3g}), {t32:.3g} of the tap bar, '
          + ', '.join(f'{k} {v:.3g}' for k, v in g32.items()) + ' of the per-operator bar')
    assert l32 <= QUARTER and t32 <= QUARTER and max(g32.values()) <= QUARTER
