"""ASAN + UBSAN build of the engine's pure-host translation-unit pieces (host-side sanitizer build).

csrc/tsm_host_util.h holds everything of tsm_engine.hip that needs no HIP type -- BatchNorm folding and weight
packing, the bf16 / split-bf16 converters, the segment rule, a conv layer's packed geometry (layer_geometry,
conv_out_size), tsm_conv_op's argument rules (conv_op_check) and the TSM_TUNE_CACHE line parser; tests/host_sanitize.cpp
fuzzes the parser with malformed lines, checks the packers' invariants, holds conv_op_check to one row per refusal (status
and message), to the plans of the accepted forms the GPU tests use and to a loop over random and extreme int32 arguments,
and layer_geometry to the per-layer values of every backbone.

csrc/tsm_conv_rules.h holds the conv launch rules, HIP-free: the parameter blocks, the weight-stationary kernels' LDS budgets
and tile geometries (ws_tile_geometry, ws_s2_tile_geometry, ws128_tile_geometry with its bank-conflict model), every kernel
family's validity and grid rule, conv_tile_valid, the fused forms' rules and conv_route.  host_sanitize.cpp holds the
geometries and the tail split to the values tests/_walk_cases.py restates, conv_route to one hand-written row per kernel
family and template arm and one row per refusal of launch_conv's argument rules, and runs 200 000 random and extreme
tsm_conv_args that conv_op_check accepts, turned into a launch the way tsm_conv_op does, through conv_route for 1, 8 and 256
CUs: every accepted route covers M and Cout with its tiles, keeps a persistent grid within its tiles and ran a tile that
conv_tile_valid offers; and holds the fold rules (bneck_ws, front_s2, conv31, conv1x1_ws / wsn, the 256 tiles) and the engine's two
shift_div rules (shift_div_refusal, shift_place_refusal) to the folds of shift_div 1, 2, 4 and 8 at ResNet-50's channel counts.
CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not available')
def test_host_pieces_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'host_sanitize')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-fno-omit-frame-pointer', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'host_sanitize.cpp'),
           '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    env.pop('LD_PRELOAD', None)
    run = subprocess.run([exe, '20000'], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'host sanitize ok' in run.stdout
