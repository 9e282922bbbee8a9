"""Live-balanced XCD runs of the position-major 3x3 launch without a GPU: pos_balanced_runs and conv_route against the kernel's
workgroup map under ASAN + UBSAN (tests/pos_balance_host.cpp, a stand-alone program), the per-XCD live work of the headline
launches, and the built code object's budget for the arm that changed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POS_KERNEL = 'conv_igemm<64, 64, 2, 2, 3, false, false, 8, false, true>'       # kPrecF32 | kPrecPosMajor
NATURAL = 'conv_igemm<64, 64, 2, 2, 3, false, false, 0, false, true>'


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tests/pos_balance_host.cpp built with ASAN + UBSAN (runtimes linked statically) and run once; returns its stdout."""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path_factory.mktemp('pos_balance_host') / 'pos_balance_host')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-fno-omit-frame-pointer', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'pos_balance_host.cpp'),
           '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stdout + run.stderr
    return run.stdout


def test_mapping_grid_and_balance_bound_under_the_sanitizers(host_program):
    """In the program, over frames 1x1 .. 9x9, 14x14, 2x5 and 6x3, both strides, ntn in {2, 4, 8}, N in {64, 128, 256}, whole-K and
    every tail point of 8 .. 304 CUs, both walk directions: the workgroups that do not return map one-to-one onto the whole
    tiles and the pieces onto (tail tile, segment), the grid is conv_route's, empty runs hold nothing, and every run's live
    work lies within one tile group of total / 8."""
    assert 'FAIL' not in host_program and host_program.strip().endswith('pos balance host ok'), host_program
    assert int(re.search(r'launches checked: (\d+)', host_program).group(1)) > 1000


def test_per_xcd_live_work_of_the_headline_launches(host_program):
    """N = 256 frames, 256 CUs: lightest and heaviest XCD over the mean.  The equal-count figures are the ones the change set
    out from; the balanced ones stay within the construction's bound -- one tile group (ntn tiles x 9 taps) over the mean, 0.3 %
    in layer2 to 5.8 % for layer4.1-2 with the tail split -- and that bound is below the equal-count excess at every launch."""
    got = {(m.group(1), m.group(2)): tuple(float(m.group(k)) for k in (3, 4, 5, 6, 7))
           for m in re.finditer(r'xcd work (\S+) (whole|tail) equal ([0-9.]+) ([0-9.]+) balanced ([0-9.]+) ([0-9.]+) bound ([0-9.]+)', host_program)}
    equal = {k: v[:2] for k, v in got.items()}
    assert equal == {('layer2.1-3.conv2', 'whole'): (0.927, 1.024), ('layer3.0.conv2', 'whole'): (0.826, 1.035),
                     ('layer3.1-5.conv2', 'whole'): (0.858, 1.058), ('layer4.0.conv2', 'whole'): (0.695, 1.095),
                     ('layer4.1-2.conv2', 'whole'): (0.765, 1.089), ('layer3.0.conv2', 'tail'): (0.781, 1.039),
                     ('layer3.1-5.conv2', 'tail'): (0.787, 1.046), ('layer4.0.conv2', 'tail'): (0.696, 1.118),
                     ('layer4.1-2.conv2', 'tail'): (0.727, 1.169)}
    for k, (_, _, lo, hi, bound) in got.items():
        assert 1 - bound - 5e-4 <= lo <= 1.0 <= hi <= 1 + bound + 5e-4 and 1 + bound < equal[k][1], (k, lo, hi, bound)   # (5e-4: the printed digits)


def test_position_major_arm_keeps_its_budget():
    """The run lookup and the early return are scalar: no more vector registers than before (at most the natural arm's), no
    scratch, 18 432 B of LDS, five workgroups per CU, and the arm is still the flag's only instantiation."""
    from workoutdetector_amd import codeobj
    from workoutdetector_amd.build import build_library
    md = codeobj.kernel_metadata(build_library())
    r = md[POS_KERNEL]
    assert r['.private_segment_fixed_size'] == 0 and r['.vgpr_spill_count'] == 0 and r.get('.sgpr_spill_count', 0) == 0, r
    assert r['.group_segment_fixed_size'] == 18432 and r['.max_flat_workgroup_size'] == 256
    assert r['waves_per_simd'] >= 5 and r['workgroups_per_cu'] >= 5, r['.vgpr_count']
    assert r['.vgpr_count'] <= md[NATURAL]['.vgpr_count']
    assert [k for k in md if re.match(r'conv_igemm<.*, (8|9|10|12), (false|true), (false|true)>$', k)] == [POS_KERNEL]
