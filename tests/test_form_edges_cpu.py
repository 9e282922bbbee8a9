"""The case table of the fused-form edge tests (tests/_form_edges.py) is AT the clauses, shown without a GPU: the geometry rules
of csrc/tsm_conv_rules.h themselves, under ASAN + UBSAN (tests/form_edges_host.cpp, a stand-alone program built from that header
alone), give the table's verdict for every (case, form); moving one clause's constant by one step (w <= 64 -> 65 / 63,
rows / T >= 8 -> 4 / 16, an even height -> any) flips exactly the verdicts the table attributes to that clause and no other; and
ws_tile_geometry cuts layer1's rows into the tile columns the table says: at least two at w = 520."""
import os
import shutil
import subprocess

import pytest

from tests import _form_edges as fe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRINTED = ('block', 'front', 'conv31_l2', 'conv31_l2l3', 'conv31_l3', 'conv23')


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tests/form_edges_host.cpp built with ASAN + UBSAN (runtimes linked statically); returns run(wmax, pxmin, anyh) ->
    [(real verdicts, (tr, tc), moved verdicts)] per case of the table."""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path_factory.mktemp('form_edges_host') / 'form_edges_host')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-fno-omit-frame-pointer', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'form_edges_host.cpp'),
           '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    lines = ''.join('%d %d %d %d %d %d %d %d\n' % ((c['clips'] * c['T'], c['T']) + c['maps']['layer1'] + c['maps']['layer2'] + c['maps']['layer3'])
                    for c in fe.CASES)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')

    def run(*moved):
        r = subprocess.run([exe] + [str(v) for v in moved], input=lines, capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert 'runtime error' not in r.stdout + r.stderr and 'FAIL' not in r.stdout, r.stdout + r.stderr
        out = r.stdout.split('\n')
        assert out[2 * len(fe.CASES)] == 'form edges host ok %d' % len(fe.CASES), r.stdout
        got = []
        for i in range(len(fe.CASES)):
            real, moved_line = out[2 * i].split(), out[2 * i + 1].split()
            assert real[0] == 'real' and real[7] == 'tile' and moved_line[0] == 'moved', (real, moved_line)
            got.append((dict(zip(PRINTED, (v == '1' for v in real[1:7]))), (int(real[8]), int(real[9])),
                        dict(zip(PRINTED[:5], (v == '1' for v in moved_line[1:6])))))
        return got
    return run


def test_the_recorded_maps_are_conv_out_of_the_frame():
    """The hand-written maps against the restated conv_out_size, and the table's own shape: ids are unique, every form has an
    entry, every move named is one of MOVES."""
    assert len({c['id'] for c in fe.CASES}) == len(fe.CASES)
    for c in fe.CASES:
        assert c['maps'] == fe.tsm_maps(c['h'], c['w']), c['id']
        assert min(c['h'], c['w']) >= 32 and c['clips'] * c['T'] <= 64 and max(c['h'], c['w']) <= 520, c['id']
        assert set(c['forms']) == set(fe.FORMS), c['id']
        for form, (verdict, clause, move) in c['forms'].items():
            assert isinstance(verdict, bool) and clause in (fe.W, fe.HE, fe.RT, fe.RD, fe.TG) and (move is None or move in fe.MOVES), (c['id'], form)


def test_every_verdict_is_the_headers(host_program):
    got = host_program()
    for c, (real, _, moved) in zip(fe.CASES, got):
        for form in fe.FORMS:
            assert real[form] == c['forms'][form][0], (c['id'], form, c['forms'][form])
        # (with the constants unmoved the program's restated clauses give the header's verdicts: the decomposition is the header's)
        assert moved == {f: real[f] for f in moved}, (c['id'], moved, real)


@pytest.mark.parametrize('move', sorted(fe.MOVES))
def test_a_clause_moved_by_one_flips_exactly_the_cases_attributed_to_it(host_program, move):
    got = host_program(*fe.MOVES[move])
    flipped = {(c['id'], f) for c, (real, _, moved) in zip(fe.CASES, got) for f in moved if moved[f] != real[f]}
    want = {(c['id'], f) for c in fe.CASES for f in fe.FORMS if c['forms'][f][2] == move}
    assert want, move
    assert flipped == want, (move, sorted(flipped - want), sorted(want - flipped))


def test_every_clause_has_a_case_on_each_side_that_it_alone_decides():
    """Per clause named in the table's docstring: a valid and an invalid (case, form) whose verdict flips when that clause's
    constant moves by one step -- for the height clause, whose only move is `even -> any`, the valid side is the neighbour map
    one row taller."""
    by_move = {m: [(c, f) for c in fe.CASES for f in fe.FORMS if c['forms'][f][2] == m] for m in fe.MOVES}
    for form in ('block', 'front'):      # w <= 64: layer1 64 columns valid, 65 invalid
        assert [c['maps']['layer1'][1] for c, f in by_move['w63'] if f == form] == [64] and all(c['forms'][f][0] for c, f in by_move['w63'])
        assert [c['maps']['layer1'][1] for c, f in by_move['w65'] if f == form] == [65] and not any(c['forms'][f][0] for c, f in by_move['w65'])
    rows = {'conv31_l2': 256, 'conv31_l2l3': 128, 'conv31_l3': 128}
    assert {(f, rows[f] // c['T']) for c, f in by_move['px16']} == {('conv31_l2', 8)} and all(c['forms'][f][0] for c, f in by_move['px16'])
    assert {(f, rows[f] // c['T']) for c, f in by_move['px4']} == {(f, 4) for f in rows} and not any(c['forms'][f][0] for c, f in by_move['px4'])
    odd = [c for c, f in by_move['anyh']]
    assert odd and all(f == 'front' and c['maps']['layer1'][0] % 2 == 1 and not c['forms'][f][0] for c, f in by_move['anyh'])
    assert any(c['forms']['front'][0] and c['forms']['front'][1] == fe.HE and c['maps']['layer1'] == (o['maps']['layer1'][0] + 1, o['maps']['layer1'][1])
               for c in fe.CASES for o in odd)
    # rows % T == 0: every T of the issue that divides neither tile size, and the T that divide both, at 32 x 32
    assert {c['T'] for c in fe.CASES if c['forms']['conv31_l2'][1] == fe.RD} == {3, 5, 6, 12}
    assert {c['T'] for c in fe.CASES if all(c['forms'][f][0] for f in rows)} == {1, 2, 4}
    # the transposed frames: the width clause must not fire
    for c in fe.CASES:
        if c['h'] > c['w'] and c['w'] == 32:
            assert c['forms']['block'][0] and c['forms']['front'][1] == fe.HE, c['id']


def test_tile_columns_of_layer1_rows(host_program):
    """ws_tile_geometry on layer1's map: the table's (rows, columns) at every case; 130 columns are cut at least in two, and no
    tile is wider than 128 columns or larger than 256 pixels and a 352-pixel patch."""
    for c, (_, tile, _) in zip(fe.CASES, host_program()):
        assert tile == c['tile'], (c['id'], tile)
        tr, tc = tile
        h1, w1 = c['maps']['layer1']
        assert 1 <= tr <= h1 and 4 <= tc <= 128 and tr * tc <= 256 and (tr + 2) * (tc + 2) <= 352, (c['id'], tile)
        cols = -(-w1 // tc)
        assert (cols >= 2) if w1 > 128 else True, (c['id'], tile)
    wide = fe.case('32x520')
    assert wide['maps']['layer1'][1] == 130 and -(-130 // wide['tile'][1]) == 5
