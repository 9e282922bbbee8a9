"""tests/_k_cases.py, checked on the CPU: every case has the K-step count, the segments and the source-switch step it claims,
by the host rules the table restates, for several CU counts; the table as a whole holds the K lengths it exists for; and the
restated rules give the values csrc/tsm_host_util.h documents for the engine's layers."""
import pytest

from tests import _k_cases as kc

N_CUS = (256, 304, 64)


def test_restated_rules_give_the_engines_values():
    # (tests/host_sanitize.cpp holds layer_geometry and conv_op_check to the same numbers)
    assert kc.layer_geometry(512, 3, 1, 'f32') == (512, 4608, 16)
    assert kc.layer_geometry(128, 3, 2, 'f32')[2] == 18 and kc.layer_geometry(1024, 1, 1, 'f32')[2] == 16
    assert kc.layer_geometry(512, 1, 1, 'f32')[2] == 0 and kc.layer_geometry(2048, 1, 1, 'bf16x3')[2] == 0
    assert kc.layer_geometry(3, 7, 2, 'f32')[:2] == (4, 224) and kc.layer_geometry(3, 7, 2, 'bf16')[:2] == (4, 256)
    assert kc.layer_geometry(3, 7, 1, 'f32')[:2] == (4, 224)
    assert [kc.segment_len(32 * nk, 'f32') for nk in (31, 32, 33, 34, 36, 64, 65, 72, 144)] == [0, 16, 17, 17, 18, 16, 17, 18, 16]
    assert [kc.conv_num_segments(32 * nk, kc.segment_len(32 * nk, 'f32')) for nk in (16, 32, 33, 65, 144)] == [1, 2, 2, 4, 9]


@pytest.mark.parametrize('n_cu', N_CUS)
def test_every_case_has_what_it_claims(n_cu):
    for c in kc.cases(n_cu):
        assert kc.steps(c) == c['steps'], c['id']
        assert kc.segments(c) == c['segs'], (c['id'], kc.segments(c))
        if c['segs'] is not None:
            assert sum(c['segs']) == c['steps'] and len(c['segs']) == kc.conv_num_segments(kc.kp_total(c), kc.kseg_of(c)), c['id']
            assert c['dtype'] == 'f32' and all(s == c['segs'][0] for s in c['segs'][:-1]) and c['segs'][-1] <= c['segs'][0], c['id']
        assert kc.switch_step(c) == c['switch'] and kc.switch_where(c) == c['where'], (c['id'], kc.switch_step(c), kc.switch_where(c))
        if c['where'] == 'inside':
            kseg = kc.kseg_of(c)
            assert 0 < c['switch'] % kseg and c['switch'] // kseg >= 1, c['id']     # strictly inside a later segment
        assert c['steps'] * kc.KC[c['dtype']] <= 8192 + 64 and c['codes'], c['id']
        # what tsm_conv_op accepts (conv_op_check): powers of two >= 32 (bf16: a multiple of 64), folds of whole channel groups
        for cin in (c['cin'],) + ((c['cin2'],) if 'cin2' in c else ()):
            assert c['k'] == 7 or (cin >= 32 and cin & (cin - 1) == 0 and (c['dtype'] != 'bf16' or cin % 64 == 0)), c['id']
        assert c['cout'] % 64 == 0
        if c['T'] > 0:
            shifted = {'shift': c['cin'], 's2shift': c['cin'], 'shift_res': c['cout'], 'dual_shift': c.get('cin2')}[c['form']]
            fold = shifted // c['fold_div']
            assert c['n'] % c['T'] == 0 and fold % (4 if c['dtype'] == 'f32' else 8) == 0 and 0 < 2 * fold <= shifted, c['id']
        if 'cin2' in c:
            ho, wo = kc.out_hw(c)
            assert ((c['hi2'] - 1) // c['stride2'] + 1, (c['wi2'] - 1) // c['stride2'] + 1) == (ho, wo), c['id']
        if c['segmented']:      # where a segmented kernel exists, and only there
            assert c['dtype'] == 'f32' and c['k'] in (1, 3) and c['form'] in ('plain', 'shift') and 'cin2' not in c, c['id']
            assert not (c['k'] == 3 and c['T'] > 0) and c['steps'] >= 32, c['id']
        # the tile every code ends on is one the trace can name, and the fallbacks the table exists for really fall back
        for code in c['codes']:
            assert kc.tile_that_runs(c, code) in kc.TILE_NAMES, (c['id'], code)
        if c['cout'] == 320:
            assert {kc.tile_that_runs(c, 1), kc.tile_that_runs(c, 5)} == {3}, c['id']
        if c.get('tail'):
            assert kc.tail_split_applies(kc.rows(c), c['cout'], len(c['segs']), n_cu), c['id']


@pytest.mark.parametrize('n_cu', N_CUS)
def test_the_table_holds_the_lengths_it_is_for(n_cu):
    cs = kc.cases(n_cu)
    by = lambda **kw: [c for c in cs if all(c.get(k) == v for k, v in kw.items())]
    # K-step counts 1, 2, 3 and 9, in fp32 and split-bf16; one step on the 256 x 256 bf16 kernel, and its persistent twin refused
    for dtype in ('f32', 'bf16x3'):
        assert {1, 2, 3, 9} <= {c['steps'] for c in by(dtype=dtype, group='a')}, dtype
    one = [c for c in by(dtype='bf16', steps=1) if 6 in c['codes'] and 8 in c['codes']]
    assert {c['form'] for c in one} >= {'plain', 'res', 'shift'}
    assert all(kc.tile_that_runs(c, 6) == 6 and kc.tile_that_runs(c, 8) == 3 for c in one)
    big_cout = [c for c in by(dtype='bf16', cout=4096)]
    assert {c['steps'] for c in big_cout} == {1, 2} and all(kc.tile_that_runs(c, 8) == 3 and kc.tile_that_runs(c, 6) == 6 for c in big_cout)
    # the source switch at step 1, at step 2 of 3, and inside a later segment
    assert by(switch=1, steps=2) and by(switch=1, steps=3) and by(switch=2, steps=3, where='inject')
    assert by(switch=1, where='preload', segs=[17, 16])
    assert by(where='inside', switch=32, segs=[17, 16]) and by(where='inside', switch=64) and by(where='inside', switch=32, segs=[17, 17])
    # a ragged last segment under 2 and under 4 segments
    ragged = [c['segs'] for c in cs if c['segs'] and c['segs'][-1] < c['segs'][0]]
    assert {len(s) for s in ragged} >= {2, 4}
    # both stride-2 parities and both shift states of every mixed dual
    for c1, c2 in ((1024, 32), (32, 1024), (2048, 32), (1024, 64)):
        got = {(c['stride2'], c['T'] > 0, c['dtype']) for c in by(group='c', cin=c1, cin2=c2)}
        assert got >= {(s2, sh, d) for s2 in (1, 2) for sh in (False, True) for d in ('f32', 'bf16x3')}, (c1, c2)
        assert {c['T'] for c in by(group='c', cin=c1, cin2=c2) if c['T']} == {3, 8}
    assert by(group='c', dtype='bf16', cin=1024, cin2=64)
    # every segmented single-source form the engine launches (build_topology): Bottleneck conv1 = a shifted 1x1 at cin 1024 / 2048,
    # conv2 = a 3x3 at cin 128 (both strides) / 256 / 512; the unshifted 3x3 of a no-shift BasicBlock
    seg = {(c['k'], c['cin'], c['stride'], c['T'] > 0): c for c in cs if c['segmented']}
    assert {(1, 1024, 1, True), (1, 2048, 1, True), (3, 128, 1, False), (3, 128, 2, False), (3, 256, 1, False), (3, 512, 1, False)} <= set(seg)
    assert seg[(1, 1024, 1, True)]['segs'] == [16, 16] and seg[(1, 2048, 1, True)]['segs'] == [16] * 4
    assert seg[(3, 128, 1, False)]['segs'] == [18, 18] and seg[(3, 256, 1, False)]['segs'] == [18] * 4 and seg[(3, 512, 1, False)]['segs'] == [16] * 9
    assert all(c['codes'] == kc.SEG_CODES for c in cs if c['segs'])
    assert sum(bool(c.get('tail')) for c in cs) == 1
    # the longest whole-K chains, in every format and on both 256-wide kernels
    assert {(c['dtype'], c['steps']) for c in by(group='d')} >= {('f32', 128), ('f32', 256), ('bf16x3', 128), ('bf16x3', 256), ('bf16', 64), ('bf16', 128)}
    assert all({6, 8} <= set(c['codes']) for c in by(group='d', dtype='bf16'))
    # one case per group with n_cu + 1 tiles of 64 rows (d: over 4 columns), the last ragged
    for g in 'abcd':
        bigs = [c for c in by(group=g) if -(-kc.rows(c) // 64) * (c['cout'] // 64) >= n_cu + 1 and kc.rows(c) % 64]
        assert bigs, g
    # the stem: fp32 at stride 1; every format on frames smaller than the window, the bf16 formats on both stem kernels
    assert {(c['hi'], c['wi']) for c in by(group='e', stride=1, dtype='f32')} == {(9, 11), (7, 7)}
    for dtype in ('f32', 'bf16x3', 'bf16'):
        small = by(group='e', stride=2, dtype=dtype)
        assert {(c['hi'], c['wi']) for c in small} == {(1, 1), (2, 3), (6, 6)}
        assert {c['env'] for c in small} == ({None} if dtype == 'f32' else {None, '0'})
    # no case costs the float64 reference more than ~20 GFLOP
    assert max(2 * kc.rows(c) * kc.kp_total(c) * c['cout'] for c in cs) < 40e9 * n_cu / 256
