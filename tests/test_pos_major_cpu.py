"""The position-major form of the segmented fp32 3x3 launch without a GPU: the pure functions the kernel inlines (row map,
live-tap mask, live K-step walk), pos_major_valid and conv_route under ASAN + UBSAN (tests/pos_major_host.cpp, a stand-alone
program), the built code object's budget for the new instantiation, and the tile name of its code bit."""
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
    """tests/pos_major_host.cpp built with ASAN + UBSAN (runtimes linked statically) and run once; returns its stdout."""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path_factory.mktemp('pos_major_host') / 'pos_major_host')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-fno-omit-frame-pointer', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'pos_major_host.cpp'),
           '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stdout + run.stderr
    return run.stdout


def test_row_map_refusals_and_live_walk_under_the_sanitizers(host_program):
    """In the program, over frames 1x1 .. 9x9, 14x14, 2x5 and 6x3, both strides, C in {128, 256, 512}: the row map is a bijection
    of [0, M) and a tile holds one position; pos_major_valid refuses each excluded form and conv_route then keeps the natural
    order; the live walk visits exactly the K-steps whose tap is in bounds, in increasing order, from any segment start, and
    the kernel's loop cuts them into the natural arm's segments."""
    assert 'FAIL' not in host_program and host_program.strip().endswith('pos major host ok'), host_program


def test_live_shares_of_the_headline_layers(host_program):
    """Live (tile, K-step) pairs at N = 256 frames: the share of the MFMAs that are still issued, per layer."""
    got = {m.group(1): float(m.group(2)) for m in re.finditer(r'live share (\S+) ([0-9.]+)', host_program)}
    assert got == {'layer2.0.conv2': 0.9763, 'layer3.0.conv2': 0.9529, 'layer3.1-5.conv2': 0.9070, 'layer4.0.conv2': 0.9070,
                   'layer4.1-2.conv2': 0.8186}


def test_code_object_has_the_position_major_instantiation_within_budget():
    """No scratch, no spills, 18 KB of LDS and at most 96 registers: five workgroups per CU like the natural arm, whose own
    figures are pinned by tests/test_code_objects.py."""
    from workoutdetector_amd import codeobj
    from workoutdetector_amd.build import build_library
    md = codeobj.kernel_metadata(build_library())
    assert POS_KERNEL in md, sorted(k for k in md if k.startswith('conv_igemm<64, 64, 2, 2, 3'))
    r = md[POS_KERNEL]
    assert r['.private_segment_fixed_size'] == 0 and r['.vgpr_spill_count'] == 0 and r.get('.sgpr_spill_count', 0) == 0, r
    assert r['.group_segment_fixed_size'] == 18432 and r['.max_flat_workgroup_size'] == 256
    assert r['waves_per_simd'] >= 5 and r['workgroups_per_cu'] >= 5, r['.vgpr_count']
    assert r['.vgpr_count'] <= md[NATURAL]['.vgpr_count']          # (the per-row masks are gone)
    assert 'splitk_reduce_pos_kernel' in md
    # the flag has this one instantiation
    assert [k for k in md if re.match(r'conv_igemm<.*, (8|9|10|12), (false|true), (false|true)>$', k)] == [POS_KERNEL]


def test_tile_name_of_the_code_bit():
    from workoutdetector_amd.engine import TsmEngine
    assert TsmEngine.tile_name(3 | 0x80) == '64x64/pos'
    assert TsmEngine.tile_name(3 | 0x80 | 0x200) == '64x64/pos/tailK'
    assert TsmEngine.tile_name(3 | 0x80 | 0x400) == '64x64/pos+conv3' and TsmEngine.tile_name(3 | 0x80 | 0x400).endswith('+conv3')
    assert TsmEngine.tile_name(3 | 0x80).split('/')[0] == '64x64'
    assert TsmEngine.tile_name(3 | 0x200) == '64x64/tailK'
