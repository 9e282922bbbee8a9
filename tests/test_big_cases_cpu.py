"""The case table of tests/test_big_conv_gpu.py (tests/_big_cases.py) holds what it claims: which tensors pass 2^31 / 2^32 bytes,
which side of its capacity rule a case is on, that conv_op_check accepts it, and the two conditions that keep the periodic
method honest -- recomputed here from the restated host rules, on several CU counts."""
import pytest

from tests import _walk_cases
from tests._big_cases import EB, cap_step, cases, edges, elements, kernel_bytes, need_gib, rule_accepts, unit_rows
from tests._walk_cases import out_hw, tail_split_applies

CAP_FAMILIES = ('ws1x1', 'ws3x3', 'ws128', 'ws128s2', 'pos')


def _odd_part(v):
    while v % 2 == 0:
        v //= 2
    return v


def check_case(c):
    """Every claim of one case, recomputed."""
    cid = c['id']
    ho, wo = out_hw(c)
    assert c['n'] == c['P'] * c['R'] and c['P'] % max(c['T'], 1) == 0 and c['P'] // max(c['T'], 1) == 3, cid
    # conv_op_check accepts it: rows and every tensor below 2^31 elements
    assert c['n'] * ho * wo < 1 << 31, cid
    assert all(v < 1 << 31 for v in elements(c).values()), (cid, elements(c))
    # the crossings, exactly as claimed; a bf16 tensor cannot reach 2^32 under the element rule
    assert edges(c) == c['big'], (cid, edges(c), c['big'], kernel_bytes(c))
    if c['dtype'] == 'bf16':
        assert all(v < 1 << 32 for k, v in kernel_bytes(c).items() if k != 'd_part'), cid
        assert (1 << 31) * EB['bf16'] == 1 << 32       # ... for any tensor the rule accepts
    assert c['big'] or c['cap'], f'{cid}: neither a crossing nor a capacity case'
    assert c['need'] == need_gib(c) and c['need'] <= 48, (cid, c['need'])
    # the capacity claim: the last periodic size the rule accepts, the first it refuses
    if c['cap'] is not None:
        assert c['family'] in CAP_FAMILIES, cid
        step = cap_step(c)
        if c['cap'] == 'inside':
            assert rule_accepts(c) and not rule_accepts(c, c['n'] + step), cid
        else:
            assert c['cap'] == 'outside' and not rule_accepts(c) and rule_accepts(c, c['n'] - step), cid
    elif c['family'] in CAP_FAMILIES:
        assert rule_accepts(c), f'{cid}: a crossing case of a ruled family must be inside its rule'
    # honesty 1: no aliasing -- the period of every tensor, in bytes of the kernel's format, has an odd factor > 1
    for name, b in kernel_bytes(c, frames=c['P']).items():
        assert _odd_part(b) > 1, (cid, name, b)
    # honesty 2: the period is not tile-aligned, and the last tile is ragged (position-major: 64 FRAMES a tile, N % 64 == 0)
    unit = unit_rows(c)
    if c['family'] == 'pos':
        assert c['P'] % 64 != 0 and (c['n'] % 64 == 0 or c['cap'] == 'outside'), cid
    elif unit:
        assert (c['P'] * ho * wo) % unit != 0, (cid, c['P'] * ho * wo, unit)
        assert (c['n'] * ho * wo) % unit != 0, (cid, c['n'] * ho * wo, unit)
        # (the igemm cases sweep every tile: ragged on each of them; 32-row tiles are fp32's)
        if c['family'].startswith('igemm'):
            units = (32, 64, 128) if c['dtype'] == 'f32' else (64, 128)
            assert all((c['n'] * ho * wo) % u and (c['P'] * ho * wo) % u for u in units), cid
        if c['family'] in ('256', '256p'):
            assert (c['n'] * ho * wo) % 128 and (c['n'] * ho * wo) % 64, cid


@pytest.mark.parametrize('n_cu', [256, 304, 80, 32])
def test_every_case_holds_its_claims(n_cu):
    table = cases(n_cu)
    assert len({c['id'] for c in table}) == len(table), 'case ids must be unique'
    for c in table:
        check_case(c)
    tail = next(c for c in table if c['id'].startswith('seg-tail'))
    ho, wo = out_hw(tail)
    assert tail_split_applies(tail['n'] * ho * wo, tail['cout'], 2, n_cu), tail['id']
    # the table holds what it is there for: every family of the walk table at a crossing or capacity size; every ruled family
    # on both sides of its rule; every tensor past its top edge somewhere, in the 4-byte formats and in bf16
    fams = {c['family'] for c in table}
    assert {c['family'] for c in _walk_cases.cases(n_cu)} <= fams, fams
    for fam in CAP_FAMILIES:
        assert {'inside', 'outside'} <= {c['cap'] for c in table if c['family'] == fam}, fam
    for t in ('x', 'y', 'residual', 'x2'):
        assert any(c['big'].get(t) == 32 for c in table), f'{t} never passes 2^32'
        assert any(c['big'].get(t) == 31 and c['dtype'] == 'bf16' for c in table), f'{t} never passes 2^31 in bf16'
    assert any(c['big'].get('d_part') == 32 and 'y' not in c['big'] for c in table)
    assert {c['T'] for c in table} >= {0, 1, 3, 8, 16} and {c['dtype'] for c in table} == {'f32', 'bf16x3', 'bf16'}


def test_the_worked_example():
    c = next(c for c in cases(256) if c['id'] == 'igemm-shift1x1-x-f32-T8')
    assert (c['P'], c['R'], c['n']) == (24, 2775, 66600)
    assert c['n'] * 63 == 4195800 and 4195800 % 128 == 88
    assert elements(c)['x'] == 1074124800 > 1 << 30
    assert kernel_bytes(c, frames=c['P'])['x'] == 1548288 == 2 ** 13 * 189


def _doctored(cid, **changes):
    c = dict(next(c for c in cases(256) if c['id'] == cid))
    c.update(changes)
    c['n'] = c['P'] * c['R']
    return c


@pytest.mark.parametrize('cid,changes', [
    ('igemm-shift1x1-x-f32-T8', dict(R=2700)),                       # an M at which x does not cross 2^32
    ('igemm-shift1x1-x-f32-T8', dict(hi=8, wi=8, R=2732)),           # a period of 2^k bytes per clip ... times three clips:
    ('igemm-shift1x1-x-f32-T8', dict(hi=8, wi=8, P=16, R=4097)),     # ... and one of 2^20 bytes exactly (P no longer 3 clips)
    ('igemm-shift1x1-x-f32-T8', dict(big={'x': 31})),                # the wrong edge
    ('igemm-shift1x1-x-f32-T8', dict(need=5)),                       # a memory claim below what the shapes need
    ('igemm-1x1-xy-f32-T0', dict(R=44416)),                          # M a multiple of the 128-row tile: no ragged last tile
    ('ws1x1-64-inside-bf16-T1', dict(cap='outside')),                # the wrong side of the rule
    ('ws1x1-64-inside-bf16-T1', dict(R=82670)),                      # inside, but not the LAST size inside
    ('ws128-outside-bf16-T0', dict(R=41337)),                        # outside, but not the FIRST size outside
    ('pos-inside-f32-T0', dict(R=20609)),                            # N % 64 != 0: not a position-major launch at all
    ('256-1x1-xy-bf16-T0', dict(big={'x': 32, 'y': 32})),            # bf16 cannot pass 2^32
])
def test_a_wrong_claim_is_caught(cid, changes):
    """check_case bites: each doctored case is refused (and the case as it stands in the table passes)."""
    check_case(_doctored(cid))
    with pytest.raises(AssertionError):
        check_case(_doctored(cid, **changes))
