"""The case table of tests/test_walk_gpu.py hits the tile counts it claims (tests/_walk_cases.py), on several CU counts."""
import pytest

from tests._walk_cases import TARGETS, cases, count_tiles, ragged, target_tiles, ws_tile_geometry


@pytest.mark.parametrize('n_cu', [256, 304, 80, 32])
def test_every_case_hits_its_tile_count(n_cu):
    table = cases(n_cu)
    assert len({c['id'] for c in table}) == len(table), 'case ids must be unique'
    for c in table:
        got = count_tiles(c)
        assert got == c['tiles'], (c['id'], got, c['tiles'])
        if c['target'] in TARGETS and c['target'] != 'ragged':
            assert got == target_tiles(c['target'], n_cu), c['id']
        if c['target'] == 'ragged':
            assert ragged(c) and got >= n_cu + 1, c['id']
        if c['target'] == 'n' and c['family'] in ('igemm64', 'igemm128', '256', '256p', 'ws1x1', 'wsn'):
            assert not ragged(c), c['id']
    # every family sees every edge
    for fam in {c['family'] for c in table}:
        labels = {c['target'] for c in table if c['family'] == fam}
        assert {'1', 'n+1'} <= labels, (fam, labels)


def test_ws_tile_geometry_restated():
    # config 5's 64 x 64 frames: 16 x 16 tiles; the headline's 56 x 56: 14 tiles either as 4 x 56 or as 8 x 29, the smaller patch wins
    assert ws_tile_geometry(64, 64) == (16, 16)
    assert ws_tile_geometry(56, 56) == (8, 29)
    assert ws_tile_geometry(19, 19) == (19, 10)
