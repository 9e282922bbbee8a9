"""CPU preconditions of tests/test_shift_div_gpu.py: the table of tests/_shift_div_cases.py claims what the host rules say, and its
inputs tell a right fold from a wrong one by at least ten times the bar the GPU test holds the kernels to.  The 10x figure is a
condition on the INPUTS (a reference with the wrong fold against the reference with the right one), never a measurement of a
kernel; a case that missed it would get another seed or size, not another factor.  Every figure is printed (pytest -s)."""
import numpy as np
import pytest
import torch

from oracle import tsm_oracle
from tests import _shift_div_cases as sc
from tests._shift_div_ops import engine_oracle, logits_misses, misses, operands, reference, tap_misses

N_CU = 256        # an MI355X; the table is also built for smaller parts below
CASES = sc.cases(N_CU)
RUN = [c for c in CASES if c['expect'] == 'run']
FACTOR = 10.0


def test_table_holds_every_family_at_every_div():
    for n_cu in (8, 64, 256, 304):
        sc.cases(n_cu)
    assert sc.DIVS == {'f32': (1, 2, 4, 16), 'bf16x3': (1, 2, 4), 'bf16': (1, 2, 4)}
    have = {(c['family'], c['dtype'], c['fold_div']) for c in CASES}
    for dtype, divs in sc.DIVS.items():
        for div in divs:
            assert ('igemm', dtype, div) in have
            forms = {(c['form'], c['k'], c['stride'], c['cin']) for c in CASES if (c['family'], c['dtype'], c['fold_div']) == ('igemm', dtype, div)}
            assert forms >= {('shift', 1, 1, 64), ('shift', 1, 1, 256), ('shift', 3, 1, 64), ('shift', 3, 2, 64), ('s2shift', 1, 2, 64),
                             ('shift_res', 1, 1, 64), ('dual_shift', 1, 1, 64)}, (dtype, div, forms)
    for div in sc.DIVS['f32']:
        assert ('igemm_seg', 'f32', div) in have
    for div in sc.DIVS['bf16']:
        for fam in ('ws1x1', 'wsn', '256', '256p', '256p_block'):
            assert (fam, 'bf16', div) in have, (fam, div)
    insts = {c['inst'][0] for c in CASES if c['family'] not in ('igemm', 'igemm_seg')}
    assert insts == {'conv1x1_ws_kernel<64>', 'conv1x1_ws_kernel<256>', 'conv1x1_wsn_kernel<256, 128, false>',
                     'conv1x1_wsn_kernel<512, 128, false>', 'conv1x1_wsn_kernel<512, 256, false>', 'conv_bf16_256_kernel<1, true>',
                     'conv_bf16_256p_kernel<1, true>', 'conv_bf16_256p_kernel<1, true, true, false>',
                     'conv_bf16_256p_kernel<1, true, false, true>'}
    # fp32 div 16 at cin 64: fold 4, one 16-byte chunk each way
    assert any(c['fold'] == 4 for c in CASES if c['dtype'] == 'f32' and c['fold_div'] == 16)


@pytest.mark.parametrize('case', CASES, ids=[c['id'] for c in CASES])
def test_fold_rule(case):
    c = case
    ch = sc.shifted_channels(c)
    assert c['fold'] == ch // c['fold_div'] == sc.fold_of(c) and ch % c['fold_div'] == 0
    assert c['T'] == 3 and c['n'] % c['T'] == 0 and c['n'] // c['T'] >= 2            # first, middle, last frame; two clips
    block = c['form'] in ('shift_res', 'dual_shift')
    admits = sc.conv_op_admits(c)
    assert (c['expect'] == 'run') == admits, c['id']
    if c['expect'] == 'refuse':     # only 2 * fold > C refuses here (div 1): the groups are whole at every div of the table
        assert c['fold_div'] == 1 and c['fold'] == ch and c['status'] == sc.INVALID_ARG and c['fold'] % sc.group_of(c['dtype']) == 0
        # what an engine, which conv_op_check does not stand in front of, does at this fold
        runs = sc.FOLD_RULES[c['rule']](c['fold'], ch, c['dtype'], block)
        want = 'refused' if block or c['form'] == 's2shift' else ('runs' if runs else 'fallback')
        assert c['engine_div1'] == want, (c['id'], c['engine_div1'], want)
    else:
        assert sc.FOLD_RULES[c['rule']](c['fold'], ch, c['dtype'], block), c['id']
        assert c['codes'][0] == 3 and len(c['codes']) >= 2
    # a 64-row tile (or the family's larger one) holds frames of both clips; the persistent families' big cases have more tiles
    # than a workgroup per CU
    ho, wo = sc.out_hw(c)
    if not c['big']:
        assert c['T'] * ho * wo % 64 != 0 and c['T'] * ho * wo < 128 and (c['hi'], c['wi']) in (sc.FRAME, sc.FRAME_S2, (5, 4))
    else:
        assert c['persistent'] and sc.tiles_of(c) == N_CU + 1
    if 'cin2' in c:
        assert ((c['hi2'] - 1) // c['stride2'] + 1, (c['wi2'] - 1) // c['stride2'] + 1) == (ho, wo)


def test_fused_forms_fold_rules():
    """The fused forms of a bf16 ResNet-50 at the folds of div 1, 2, 4 and 8: the whole-block and the front kernel at 8 only;
    conv31 at every fold that is a whole number of 64-channel chunks and leaves both groups inside the tensor."""
    for div in (1, 2, 4, 8):
        assert sc.bneck_ws_fold_ok(256, 256 // div) == sc.bneck_ws_fold_ok(64, 64 // div) == (div == 8)
        assert sc.front_s2_fold_ok(256 // div) == (div == 8)
        for c in (512, 1024):
            assert sc.conv31_fold_ok(c, c // div) == (div != 1)


@pytest.mark.parametrize('case', RUN, ids=[c['id'] for c in RUN])
def test_inputs_tell_a_wrong_fold(case, capsys):
    c = case
    ops, ref = operands(c)
    want = reference(c, ops, ref)
    assert float((want != 0).double().mean()) > 0.2
    wrong = misses(reference(c, ops, ref, fold_div=8), want, c['dtype'])
    swapped = misses(reference(c, ops, ref, swap=True), want, c['dtype'])
    with capsys.disabled():
        print(f'\n[{c["id"]}] fold {c["fold"]}: fold_div = 8 misses the bar {wrong:.0f}x, t+1 / t-1 exchanged {swapped:.0f}x')
    assert wrong >= FACTOR and swapped >= FACTOR, (c['id'], wrong, swapped)


@pytest.mark.parametrize('case', sc.ENGINE_CASES, ids=[sc.engine_id(e) for e in sc.ENGINE_CASES])
def test_engine_inputs_tell_a_wrong_shift_div(case, capsys):
    """The oracle at shift_div = 8 against the oracle at the case's div: the logits and the conv1 tap of each stage's first block."""
    base_model, place, dtype, div, geo = case
    bf16 = dtype == 'bf16'
    want, taps = engine_oracle(base_model, place, bf16, div, geo)
    wrong, wtaps = engine_oracle(base_model, place, bf16, 8, geo)
    m = logits_misses(wrong, want, dtype)
    tm = {s: tap_misses(wtaps[s], taps[s], dtype) for s in sc.CONV1_TAPS}
    with capsys.disabled():
        print(f'\n[{sc.engine_id(case)}] shift_div = 8 misses the logits bar {m:.1f}x, the conv1 taps ' +
              ', '.join(f'{s} {v:.0f}x' for s, v in tm.items()))
    assert m >= FACTOR, (case, m)
    assert all(v >= FACTOR for v in tm.values()), (case, tm)


def test_oracle_shift_at_div_1_and_2(golden_dir):
    """oracle/tsm_oracle.py::temporal_shift at div 1 and 2.  tests/golden/ref_temporal_shift.npz, the reference's recorded vectors,
    holds divs 8 and 3 only -- none at 1 or 2 -- so there is no recorded vector to compare with at these divs (the fixture is
    not regenerated); instead the oracle is held to the reference's slicing written out frame by frame: channels [0, fold) of
    frame t are frame t + 1's (zeros at the clip's last frame), [fold, 2 fold) frame t - 1's (zeros at its first), the rest
    frame t's.  At div 1 that is every channel from t + 1 and an empty second group; at div 2 no channel from its own frame."""
    z = np.load(f'{golden_dir}/ref_temporal_shift.npz')
    assert sorted({int(m[5]) for m in z['meta']}) == [3, 8]
    g = torch.Generator().manual_seed(5)
    for div in (1, 2, 4, 8, 16):
        for clips, t, c in ((2, 3, 64), (1, 1, 64), (3, 2, 256), (1, 4, 16)):
            x = torch.randn(clips * t, c, 3, 2, generator=g)
            got = tsm_oracle.temporal_shift(x, t, div)
            fold = c // div
            want = torch.zeros_like(x)
            for n in range(clips):
                for f in range(t):
                    i = n * t + f
                    if f + 1 < t:
                        want[i, :fold] = x[i + 1, :fold]
                    if f > 0:
                        want[i, fold:2 * fold] = x[i - 1, fold:2 * fold]
                    want[i, 2 * fold:] = x[i, 2 * fold:]
            assert torch.equal(got, want), (div, clips, t, c)
            if div == 1:
                assert torch.equal(got.reshape(clips, t, -1)[:, :-1], x.reshape(clips, t, -1)[:, 1:]) and not got.reshape(clips, t, -1)[:, -1].any()
