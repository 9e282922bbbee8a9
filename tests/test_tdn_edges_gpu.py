"""TDN engines on the GPU where tests/test_tdn_gpu.py does not reach: the depths that ship and the even arm of run_tdn's buffer
choice, launches that go round their grid-stride loop again, BatchNorm variances that make eps visible, mSE maps with one even and
one odd side, and gates beyond expf's range.  The cases and their preconditions are tests/_tdn_cases.py and
tests/test_tdn_cases_cpu.py; the reference is the float64 tests/_tdn.py computing from the engine's own fp32 weights.

Bars, those of tests/test_tdn_gpu.py: per operator, from the engine's own tap in front of it, rtol 1e-4 + 1e-4 of the scale; network
taps rtol 1e-3 + 3e-5 of the scale; logits rtol 1e-3 + 1e-5 of the scale; the blends 2^-23 (|alpha a| + |beta b|) per element;
everything that compares two runs of the engine bit for bit.  Each test prints its worst error over the scale.

Measured on the MI355X (max |err| / scale): DESIGN.md 4.25."""
import copy
import time

import numpy as np
import pytest

from tests import _tdn
from tests import _tdn_cases as tc
from tests._tdn_cases import LOGITS_BAR, OP_BAR, TAP_BAR
from tests._util import assert_close

pytestmark = pytest.mark.gpu


def _say(capsys, text):
    with capsys.disabled():
        print('\n' + text)


def _network(eng, x, logits, taps, depths, consensus):
    """Every tap, the logits and forward_features of ``eng`` against the float64 (per-segment logits, taps): (the logits' error, the
    worst tap's error and its share of the bar as text)."""
    want = logits if consensus == 'identity' else logits.mean(1)
    worst = share = 0.0
    for name in tc.tap_names(depths):
        got = eng.forward_tap(x, name)
        share = max(share, tc.bar_ratio(got, taps[name], **TAP_BAR))
        worst = max(worst, assert_close(got, taps[name], what=f'tap {name} ({share:.2g} of the bar)', **TAP_BAR))
    got = eng.forward_host(x)
    assert got.shape == want.shape
    err = assert_close(got, want, what='logits', **LOGITS_BAR)
    assert_close(eng.forward_features(x), taps['features'], what='forward_features', **LOGITS_BAR)
    return err, f'{worst:.2g} ({share:.2g} of its bar)'


def _gates(centre, model, x, blocks, bounded=False):
    """The long-term module per operator on an engine whose temporal weights are (0, 1, 0) (its '.shift' tap is g): g, m+ and m-
    against the float64 module of the engine's OWN conv1 tap.  bounded: also 0.5 |x| <= |g| <= 1.5 |x| and the sign of x, up to the
    bar (y lies in [-0.5, 0.5] whatever e is)."""
    worst = {}
    for li, b in blocks:
        p = f'layer{li}.{b}'
        c1 = centre.forward_tap(x, p + '.conv1')
        g = centre.forward_tap(x, p + '.shift')
        want_g, want_f, want_b = tc.gate64(model, li, b, c1)
        worst[p] = assert_close(g, want_g, what=p + ' gate', **OP_BAR)
        assert_close(centre.forward_tap(x, p + '.mse.fwd'), want_f, what=p + '.mse.fwd', **OP_BAR)
        assert_close(centre.forward_tap(x, p + '.mse.bwd'), want_b, what=p + '.mse.bwd', **OP_BAR)
        assert np.abs(g - c1).max() > 1e-2 * np.abs(c1).max()          # the gate does something
        if bounded:
            tol = OP_BAR['rtol'] * np.abs(want_g) + OP_BAR['atol_scale'] * np.abs(want_g).max()
            ax, ag = np.abs(c1.astype(np.float64)), np.abs(g.astype(np.float64))
            assert (ag >= 0.5 * ax - tol).all() and (ag <= 1.5 * ax + tol).all(), p
            sure = 0.5 * ax > tol          # (where a g inside the bar cannot have crossed zero)
            assert sure.any() and (np.sign(g[sure]) == np.sign(c1[sure])).all(), p
    return worst


# ---- 1. the real depths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('depths, recipe, h, w, T, n, consensus', tc.DEPTH_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_depths_against_float64(hip_lib, depths, recipe, h, w, T, n, consensus, capsys):
    """(3, 4, 6, 3), the model create_tdn_model builds; (2, 1, 1, 1): an even depths[0] puts xd1 into run_tdn's other buffer;
    (4, 1, 1, 2): a third and a fourth block in a stage."""
    x = tc.clips(h, w, T, n)
    logits, taps = tc.reference(h, w, depths, T, n, recipe)
    eng = tc.engine(h, w, T, depths, tc.network(depths, T, recipe)[1], max_clips=n, consensus=consensus)
    try:
        err, worst = _network(eng, x, logits, taps, depths, consensus)
    finally:
        eng.close()
    _say(capsys, f'[tdn depths {depths} {recipe} {h}x{w} T={T} n={n} {consensus}] max|err|/scale: logits {err:.2g}, worst tap {worst}')


def test_full_depth_gates_poison_and_conv_names(hip_lib, capsys):
    """The full-depth engine at 64 x 96: the last block of layers 2, 3 and 4 per operator; TSM_POISON=1 keeps the logits' bits; one
    tile name per conv."""
    depths, recipe, h, w, T, n, _consensus = tc.DEPTH_CASES[0]
    x = tc.clips(h, w, T, n)
    model, weights = tc.network(depths, T, recipe)
    centre = tc.engine(h, w, T, depths, tc.with_temporal(weights), max_clips=n)
    try:
        worst = _gates(centre, model, x, [(li, depths[li - 1] - 1) for li in (2, 3, 4)])
    finally:
        centre.close()
    plain, hostile = tc.engine(h, w, T, depths, weights, max_clips=n), tc.engine(h, w, T, depths, weights, max_clips=n, poison=True)
    try:
        names = plain.conv_tiles(n)
        assert len(names) == tc.n_conv_names(depths) == 64 and list(names)[:2] == ['conv1', 'diff.conv1_5']
        assert np.array_equal(tc.bits(plain.forward_host(x)), tc.bits(hostile.forward_host(x)))
    finally:
        plain.close()
        hostile.close()
    _say(capsys, '[tdn full depth, gate per-op] max|err|/scale: ' + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()))


# ---- 2. launch-cap wraps ----------------------------------------------------------------------------------------------------------
def _blend_check(got, a, d, alpha, beta, frames, what):
    """|got - (alpha a + beta up(d))| <= 2^-23 (|alpha a| + |beta up(d)|) on ``frames``: alpha a rounds once, beta b is exact (beta a
    power of two), the sum rounds once; contracting to an FMA only removes a rounding.  Returns the worst error over that bound."""
    want, mag = tc.blend64(a[frames], d[frames], alpha, beta)
    err = np.abs(got[frames].astype(np.float64) - want)
    assert np.isfinite(got[frames]).all() and (err <= 2.0 ** -23 * mag).all(), (what, float((err / (2.0 ** -23 * mag + 1e-300)).max()))
    swapped, _mag = tc.blend64(a[frames], d[frames], beta, alpha)
    assert alpha == beta or (np.abs(got[frames] - swapped) > 2.0 ** -23 * mag).mean() > 0.5          # (the check tells alpha from beta)
    return float((err / (2.0 ** -23 * mag + 1e-300)).max())


def test_launches_that_wrap_their_grid(hip_lib, capsys):
    """21 clips of 8 frames at 224 x 224, depths (1, 1, 1, 1): fuse1 (2.01 passes of 16384 x 256 threads), fuse2 (8.04) and layer2.0's
    mse_mix_kernel<8> (1.005: the tail of frame 167) go round their grid-stride loops again, as the benchmark's launches do.  The
    blends exactly, in the frames where a pass ends; the long-term module of the last clip per operator (temporal weights (0, 1, 0)
    throughout: '.shift' is g); the logits of the first and the last clip against float64; clips either side of the front end's
    chunks (8 + 8 + 5) equal their single-clip forwards bit for bit."""
    t0 = time.perf_counter()
    h = w = 224
    T, n, depths = 8, 21, (1, 1, 1, 1)
    one_pass = tc.launch_pass('tdn_fuse_kernel', 'quads')
    assert one_pass == tc.launch_pass('mse_mix_kernel', 'outs')
    frames, per = n * T, {'fuse1': 56 * 56 * 16, 'fuse2': 56 * 56 * 64, 'mix': 56 * 56 * 8}
    edges = {k: tc.wrap_frames(frames, v, one_pass) for k, v in per.items()}
    assert len(edges['fuse1']) == 2 and len(edges['fuse2']) == 8 and edges['mix'] == [frames - 1], edges          # the premises
    assert tc.wrap_frames((n - 1) * T, per['mix'], one_pass) == []                                                 # no smaller batch would do
    x = np.random.default_rng([31, h, w, T, n]).standard_normal((n, T, 15, h, w), dtype=np.float32)
    model, plain = tc.network(depths, T)
    weights = {k: np.array(v) for k, v in tc.with_temporal(plain).items()}
    centre = _tdn.load(copy.deepcopy(model), weights)
    eng = tc.engine(h, w, T, depths, weights, max_clips=n, consensus='identity')
    try:
        assert eng.tdn_chunk_clips == 8
        worst = {}
        for name, a, d in (('fuse1', 'stem', 'diff.stem'), ('fuse2', 'layer1.0', 'resnext_layer1.0')):
            got, ta, td = (eng.forward_tap(x, k) for k in (name, a, d))
            assert got.shape == ta.shape == (frames, 56, 56, 4 * per[name] // (56 * 56)) and td.shape[1:3] == (28, 28)
            worst[name] = _blend_check(got, ta, td, 0.5, 0.5, sorted({0, frames - 1, *edges[name]}), name)
            del got, ta, td
        p = 'layer2.0'
        c1 = eng.forward_tap(x, p + '.conv1')
        assert c1.shape == (frames, 56, 56, 128) and frames * per['mix'] > one_pass
        got = {k: eng.forward_tap(x, p + k) for k in ('.mse.fwd', '.mse.bwd', '.shift')}
        for clip in (n - 1, 0):
            sl = slice(clip * T, (clip + 1) * T)
            for k, want in zip(('.shift', '.mse.fwd', '.mse.bwd'), tc.gate64(centre, 2, 0, c1[sl])):
                worst[f'clip {clip} {k}'] = assert_close(got[k][sl], want, what=f'{p}{k} of clip {clip}', **OP_BAR)
        del c1, got
        batch = eng.forward_host(x)
        for i in (0, 7, 8, 15, 16, 20):
            assert np.array_equal(tc.bits(batch[i:i + 1]), tc.bits(eng.forward_host(x[i:i + 1]))), i
    finally:
        eng.close()
    ends = np.ascontiguousarray(x[[0, n - 1]])
    want, _taps = tc.run(centre, ends)
    worst['logits'] = assert_close(batch[[0, n - 1]], want, what='logits of clips 0 and 20', **LOGITS_BAR)
    assert not np.array_equal(batch[0], batch[n - 1])
    _say(capsys, '[tdn wraps 224x224 T=8 n=21] blends err/bound: fuse1 %.2g, fuse2 %.2g; max|err|/scale: ' % (worst.pop('fuse1'), worst.pop('fuse2'))
         + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()) + '; wall time %.1f s' % (time.perf_counter() - t0))


def test_the_blends_take_alpha_for_the_trunk(hip_lib, capsys):
    """T = 3: alpha = 0.75 on the trunk's map, beta = 0.25 on the difference path's, through a 2 : 1 upsample of a map that is not
    square (24 x 40 from 12 x 20)."""
    h, w, T, n, depths = 96, 160, 3, 2, tc.D96
    x = tc.clips(h, w, T, n)
    eng = tc.engine(h, w, T, depths, tc.network(depths, T)[1], max_clips=n)
    try:
        worst = {}
        for name, a, d in (('fuse1', 'stem', 'diff.stem'), ('fuse2', 'layer1.0', 'resnext_layer1.0')):
            got, ta, td = (eng.forward_tap(x, k) for k in (name, a, d))
            assert ta.shape[1:3] == (24, 40) and td.shape[1:3] == (12, 20)
            worst[name] = _blend_check(got, ta, td, 0.75, 0.25, list(range(n * T)), name)
    finally:
        eng.close()
    _say(capsys, '[tdn blends 96x160 T=3] err/bound: ' + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()))


# ---- 3, 4, 5: crafted weights and frames through the network and per operator --------------------------------------------------
def _network_and_gates(h, w, depths, T, n, recipe, blocks, bounded=False):
    x = tc.clips_of(recipe, h, w, T, n)
    logits, taps = tc.reference(h, w, depths, T, n, recipe)
    model, weights = tc.network(depths, T, recipe)
    eng = tc.engine(h, w, T, depths, weights, max_clips=n)
    try:
        err, worst = _network(eng, x, logits, taps, depths, 'avg')
    finally:
        eng.close()
    centre = tc.engine(h, w, T, depths, tc.with_temporal(weights), max_clips=n)
    try:
        gates = _gates(centre, model, x, blocks, bounded)
    finally:
        centre.close()
    return f'max|err|/scale: logits {err:.2g}, worst tap {worst}; gate per-op ' + ', '.join(f'{k} {v:.2g}' for k, v in gates.items())


def test_small_variances_pin_the_batchnorm_eps(hip_lib, capsys):
    """running_var 1e-6 .. 1e-4: kBnEps = 1e-5 is a tenth to ten times the variance under every root.  Any of 1.1e-5, 2e-5, 1e-3 or 0
    misses these bars 100 times over (tests/test_tdn_cases_cpu.py)."""
    text = _network_and_gates(96, 160, tc.D96, 3, 2, 'small_variance', [(2, 0), (3, 0), (4, 1)])
    _say(capsys, '[tdn small variances 96x160 T=3] ' + text)


@pytest.mark.parametrize('frame', list(tc.PARITY_FRAMES), ids=lambda v: '%dx%d' % v)
def test_mixed_parity_and_tall_maps(hip_lib, frame, capsys):
    """layer4.1's maps 2 x 3, 3 x 2 and 5 x 3 (pools 1 x 1, 1 x 1, 2 x 1): a cell row or column that is not pooled on one side only,
    and a frame taller than wide."""
    h, w = frame
    text = _network_and_gates(h, w, tc.D96, 3, 2, 'plain', [(4, 1)])
    _say(capsys, f'[tdn mixed parity {h}x{w} T=3] ' + text)


def test_saturated_gates_stay_finite_and_bounded(hip_lib, capsys):
    """mse.bn3 x 64: e beyond +-89 in 2 to 15 % of a block's elements each way, max |e| 340 to 880.  1 / (1 + expf(-e)) is 0 or 1
    there; expf(e) / (1 + expf(e)) would be inf / inf (tests/test_tdn_cases_cpu.py).  These gates pass on 64 times what the blocks
    in front lose: the worst tap uses 0.51 of its bar on the MI355X (0.17 in a float32 copy on the CPU; the input is chosen for
    that, tests/_tdn_cases.py: CLIP_SEEDS), where every other case of this file stays under 0.06."""
    text = _network_and_gates(96, 160, tc.D96, 3, 2, 'saturated', tc.shift_blocks(tc.D96), bounded=True)
    _say(capsys, '[tdn saturated gates 96x160 T=3] ' + text)
