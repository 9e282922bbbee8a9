"""The preconditions of tests/test_bn_eps_gpu.py, without a GPU: that the small-variance cases of tests/_bn_cases.py tell the
documented BatchNorm eps (1e-5, torch's default, what the reference's torchvision backbones keep) from a tenth more at every fold
site, that a float32 implementation fits the bars on them with room, and that the references the GPU tests compare against carry
torch's constant themselves.  All of it is the float64 torch modules the GPU tests use as their reference and float32 copies."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import tsm_oracle
from tests import _bn_cases as bc
from tests import _conv_ref
from tests._tdn_cases import bar_ratio
from tests._util import BF16_E2E_BAR

TENTH = 0.1             # the share of a bar a float32 copy of the network may use
MISS = 10.0             # the eps = 1.1e-5 mutant must exceed its bar this many times
F32_CASES = [c for c in bc.ENGINE_CASES if c.dtype != 'bf16']


def test_the_recipe_is_tdns_and_changes_the_batchnorms_only():
    from tests import _tdn
    assert bc.small_variance is _tdn.small_variance            # one definition for both families
    plain = bc.weights(bc.R50, 'blockres', True, 'plain')
    w = bc.weights(bc.R50, 'blockres', True)
    diff = [k for k in plain if not np.array_equal(plain[k], w[k])]
    bns = [k[:-len('running_var')] for k in plain if k.endswith('running_var')]
    assert len(bns) == 53 + 5 and sum(p.endswith('.nl.W.1.') for p in bns) == 5
    assert sorted(diff) == sorted(p + s for p in bns for s in ('running_var', 'weight'))
    for p in bns:
        var = w[p + 'running_var']
        assert var.dtype == np.float32 and 1e-6 <= var.min() and var.max() <= 1e-4 * (1 + 1e-6), p
        scale = w[p + 'weight'].astype(np.float64) / np.sqrt(var.astype(np.float64) + 1e-5)
        assert np.abs(scale / plain[p + 'weight'] - 1).max() < 1e-6, p          # the folded scale is the seeded gamma again
    assert np.log10(np.concatenate([w[p + 'running_var'] for p in bns])).std() > 0.5
    net = bc.network(bc.R50, 'blockres', True)
    sd = net.engine_state_dict()
    assert all(sd[k].dtype == torch.float64 and np.array_equal(sd[k].numpy(), w[k].astype(np.float64)) for k in w)


def test_the_case_table_covers_what_it_is_there_for():
    ids = [c.id for c in bc.ENGINE_CASES]
    assert len(set(ids)) == len(ids)
    for model in (bc.R18, bc.R34, bc.R50, bc.WRN):
        mine = [c for c in bc.ENGINE_CASES if c.base_model == model and not c.non_local and c.dtype != 'bf16']
        assert sorted((c.dtype, c.place) for c in mine) in ([('bf16x3', 'block'), ('f32', 'blockres')], [('bf16x3', 'blockres'), ('f32', 'block')])
    assert [c.id for c in bc.ENGINE_CASES if c.non_local] == ['resnet50-f32-blockres-nl']
    assert all((c.h, c.w) == ((32, 64) if c.non_local else (32, 32)) for c in bc.ENGINE_CASES)
    assert (bc.TUNED_CASE.base_model, bc.TUNED_CASE.dtype, bc.TUNED_CASE.non_local) == (bc.R50, 'f32', False)
    for c in bc.ENGINE_CASES:
        assert set(c.sites.values()) <= set(c.taps) and set(c.sites) == {'stem', 'downsample', 'last'} | ({'nl.W'} if c.non_local else set())
        net = bc.network(*c.key[:3])
        n_down = 4 if c.base_model in (bc.R50, bc.WRN) else 3
        assert [len(bc.site_modules(net, s)) for s in ('stem', 'downsample', 'last')] == [1, n_down, 1]
        last = bc.site_modules(net, 'last')[0]
        names = [n for n, m in net.named_modules() if m is last]
        assert names[0].split('.')[-1] == ('bn3' if c.base_model in (bc.R50, bc.WRN) else 'bn2') and c.sites['last'] in names[0], names
        if c.non_local:
            assert len(bc.site_modules(net, 'nl.W')) == 5
    assert set(bc.OP_CASES) == {'shifted 1x1', '3x3 stride 2', 'stem', 'stem bf16x3', 'conv3 + downsample'}


@pytest.mark.parametrize('case', F32_CASES, ids=repr)
def test_a_float32_copy_fits_and_another_eps_does_not(case):
    """The float32 copy stays under a tenth of every bar; eps = 1.1e-5 in every BatchNorm misses the logits bar 10 times over; at
    one fold site alone it misses 10 times over on the logits or on the tap behind that site."""
    want = bc.reference(case)
    share = bc.misses(case, bc.emulated(case), want)
    print(f'{case}: float32 copy ' + ', '.join(f'{k} {v:.3g}' for k, v in share.items()) + ' of the bar')
    assert max(share.values()) <= TENTH, share
    every = bc.misses(case, bc.mutant(case, 'all'), want)
    print(f'{case}: eps {bc.MUTANT_EPS:g} everywhere misses ' + ', '.join(f'{k} {v:.3g}' for k, v in every.items()) + ' times')
    assert every['logits'] >= MISS, every
    for site, tap in case.sites.items():
        one = bc.misses(case, bc.mutant(case, site), want)
        print(f'{case}: eps {bc.MUTANT_EPS:g} in {site} only misses the logits bar {one["logits"]:.3g} times, the tap bar at {tap} {one[tap]:.3g} times')
        assert max(one['logits'], one[tap]) >= MISS, (site, one)      # (where the logits do not reach it, the GPU test's tap does)
        if site == 'nl.W':                                     # the tap in front of the site does not move: the site is what is seen
            assert one['layer2.0.block'] == 0


@pytest.mark.parametrize('case', F32_CASES, ids=repr)
def test_the_plain_weights_cannot_see_eps_and_the_recipe_keeps_the_network_usable(case):
    """The gap this closes: under make_state_dict's own variances a network without eps (1e-12 stands for 0, which torch's
    batch_norm refuses) stays inside the logits bar.  And the recipe's logit scale is within a factor of 2 of the plain weights'."""
    plain = bc.reference(case, 'plain')
    ratio = bar_ratio(bc.mutant(case, 'all', eps=1e-12, recipe='plain')[0], plain[0], **bc.LOGITS_BAR)
    scale, plain_scale = float(np.abs(bc.reference(case)[0]).max()), float(np.abs(plain[0]).max())
    print(f'{case}: plain weights, eps left out: {ratio:.3g} of the logits bar; logit scale {scale:.3g} under the recipe, {plain_scale:.3g} plain')
    assert ratio < 1.0
    assert 0.5 <= scale / plain_scale <= 2.0


def test_the_bf16_case_is_in_because_its_oracle_sees_eps():
    """The bf16-storage oracle with eps = 1.1e-5 in its fold misses BF16_E2E_BAR of the logit scale 10 times over: the condition
    under which the table may hold a bf16 case."""
    cases = [c for c in bc.ENGINE_CASES if c.dtype == 'bf16']
    assert [c.id for c in cases] == ['resnet50-bf16-blockres']
    want16, _taps, want32 = bc.bf16_reference(cases[0])
    got16, _taps, _w = bc.bf16_reference(cases[0], eps=bc.MUTANT_EPS)
    assert tsm_oracle.BN_EPS == 1e-5
    scale = float(np.abs(want32).max())
    moved, own = float(np.abs(got16 - want16).max()) / scale, float(np.abs(want16 - want32).max()) / scale
    print(f'{cases[0]}: eps {bc.MUTANT_EPS:g} moves the bf16 oracle\'s logits by {moved:.3g} of the scale, {moved / BF16_E2E_BAR:.3g} times the bar; '
          f'the format itself by {own:.3g}')
    assert moved >= MISS * BF16_E2E_BAR


# ---- per op -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(bc.OP_CASES))
def test_per_op_cases_see_eps(name):
    """The float64 reference with eps = 1.1e-5 misses the per-op bar 10 times over; torch's own float32 conv + batch_norm fits it."""
    op = bc.op_case(name)
    for bn in (op['bn'], op['bn2']):
        if bn is not None:
            assert 1e-6 <= float(bn[3].min()) and float(bn[3].max()) <= 1e-4 * (1 + 1e-6)
    want = bc.op_reference(name)
    bar = bc.OP_BARS[op['dtype']]
    miss = bar_ratio(bc.op_reference(name, eps=bc.MUTANT_EPS), want, **bar)
    assert _conv_ref.BN_EPS == 1e-5
    x = tsm_oracle.temporal_shift(op['x'], op['T'], 8) if op['T'] else op['x']
    h = F.batch_norm(F.conv2d(x, op['w'], stride=op['stride'], padding=op['w'].shape[-1] // 2), op['bn'][2], op['bn'][3], op['bn'][0], op['bn'][1])
    if op['x2'] is not None:
        h = h + F.batch_norm(F.conv2d(op['x2'], op['w2'], stride=op['stride2']), op['bn2'][2], op['bn2'][3], op['bn2'][0], op['bn2'][1])
    share = bar_ratio(torch.relu(h).numpy(), want, **bar)
    print(f'{name}: eps {bc.MUTANT_EPS:g} misses the per-op bar {miss:.3g} times; torch in float32 uses {share:.3g} of it')
    assert miss >= MISS and share <= TENTH


def _torch_default_batchnorm(x, w, bn, eps=None):
    """conv -> nn.BatchNorm2d() as torch constructs it (its default eps unless given), eval mode, float64 -> ReLU."""
    mod = nn.BatchNorm2d(w.shape[0]) if eps is None else nn.BatchNorm2d(w.shape[0], eps=eps)
    with torch.no_grad():
        for p, v in zip((mod.weight, mod.bias, mod.running_mean, mod.running_var), bn):
            p.copy_(v)
    mod = mod.double().eval()
    with torch.no_grad():
        return torch.relu(mod(F.conv2d(x.double(), w.double(), stride=2, padding=1))).numpy()


def test_the_references_carry_torchs_default_eps():
    """oracle.tsm_oracle.conv_bn_act, the oracle's bf16 fold (fold_bn) and tests/_conv_ref.py against nn.BatchNorm2d() at its
    default eps on small-variance channels, at the per-op bar; the same module with eps = 1.1e-5 misses it."""
    op = bc.op_case('3x3 stride 2')
    x, w, bn = op['x'], op['w'], op['bn']
    assert nn.BatchNorm2d(4).eps == 1e-5 == tsm_oracle.BN_EPS == _conv_ref.BN_EPS
    want = _torch_default_batchnorm(x, w, bn)
    wf, bias = tsm_oracle.fold_bn(w, bn)
    got = {'conv_bn_act': tsm_oracle.conv_bn_act(x, w, bn, 2, 1, True).numpy(),
           'fold_bn': torch.relu(F.conv2d(x.double(), wf.double(), stride=2, padding=1) + bias.double()[None, :, None, None]).numpy(),
           '_conv_ref': _conv_ref.conv_ref(x, w, bn, 2, True).numpy()}
    bar = bc.OP_BARS['f32']
    for name, g in got.items():
        share = bar_ratio(g, want, **bar)
        print(f'{name}: {share:.3g} of the per-op bar against nn.BatchNorm2d()')
        assert share <= TENTH, name
    miss = bar_ratio(_torch_default_batchnorm(x, w, bn, eps=bc.MUTANT_EPS), want, **bar)
    print(f'nn.BatchNorm2d(eps={bc.MUTANT_EPS:g}) misses the per-op bar {miss:.3g} times')
    assert miss >= MISS
