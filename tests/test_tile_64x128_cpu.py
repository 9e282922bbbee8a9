"""The 64x128 tile of the fp32 unsegmented 1x1 convs without a GPU: its launch rules under ASAN + UBSAN (tests/tile_64x128_host.cpp,
a stand-alone program), the built code object's budget for its four instantiations, and the name of its tile code."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (SHIFT, RES, PREC, DUAL, SEG) of the four arms: plain, shifted, residual, second source
ARMS = ['conv_igemm<64, 128, 2, 2, 1, false, false, 0, false, false>', 'conv_igemm<64, 128, 2, 2, 1, true, false, 0, false, false>',
        'conv_igemm<64, 128, 2, 2, 1, false, true, 0, false, false>', 'conv_igemm<64, 128, 2, 2, 1, false, false, 0, true, false>']


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tests/tile_64x128_host.cpp built with ASAN + UBSAN (runtimes linked statically) and run once; returns its stdout."""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path_factory.mktemp('tile_64x128_host') / 'tile_64x128_host')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-fno-omit-frame-pointer', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'tile_64x128_host.cpp'),
           '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stdout + run.stderr
    return run.stdout


def test_routes_refusals_and_names_under_the_sanitizers(host_program):
    """In the program: one route per arm; Cout 192, a segmented layer, a 3x3, the bf16 formats and the three block-placement
    forms refused (and run on the heuristic shape); the name round trip; conv_tile_valid => the route accepts the tile, for
    1, 8 and 256 CUs over 20000 random 1x1 parameter blocks."""
    assert 'FAIL' not in host_program and host_program.strip().endswith('tile 64x128 host ok'), host_program
    offered, routed = map(int, re.search(r'offered for (\d+) of 20000 .* (\d+) routed', host_program).groups())
    assert offered >= routed > 1000


def test_code_object_has_the_four_arms_within_budget():
    """27 648 bytes of LDS (one buffer of 64 + 128 rows; the epilogue stages 64-column halves inside it), at most 128 registers
    and no scratch: four workgroups of four waves per CU.  No other 64x128 instantiation is built."""
    from workoutdetector_amd import codeobj
    from workoutdetector_amd.build import build_library
    md = codeobj.kernel_metadata(build_library())
    assert sorted(k for k in md if k.startswith('conv_igemm<64, 128,')) == sorted(ARMS)
    for name in ARMS:
        r = md[name]
        assert r['.private_segment_fixed_size'] == 0 and r['.vgpr_spill_count'] == 0 and r.get('.sgpr_spill_count', 0) == 0, (name, r)
        assert r['.group_segment_fixed_size'] == 27648 and r['.max_flat_workgroup_size'] == 256, (name, r)
        assert r['.vgpr_count'] <= 128 and r['waves_per_simd'] >= 4 and r['workgroups_per_cu'] >= 4, (name, r['.vgpr_count'])


def test_tile_name_of_the_code():
    from workoutdetector_amd.engine import TsmEngine
    assert TsmEngine.TILE_NAMES[9] == '64x128' and TsmEngine.tile_name(9) == '64x128'
    assert sorted(TsmEngine.TILE_NAMES) == list(range(10))
