"""bench.py without --full: the headline alone (which legs a command line runs on CPU, a real plain run on the GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests._util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA_LEGS = ('no_alt', 'no_config5', 'no_cpu_baseline', 'no_parity')


def test_plain_command_runs_no_leg_beyond_the_headline():
    import bench
    plain = bench.parse_args(['--gpus', '1', '--steps', '20', '--warmup', '5'])
    assert not plain.full and all(getattr(plain, k) for k in EXTRA_LEGS)
    assert (plain.gpus, plain.steps, plain.warmup, plain.dtype, plain.batch) == (1, 20, 5, 'f32', 32)
    full = bench.parse_args(['--gpus', '1', '--steps', '20', '--warmup', '5', '--full'])
    assert full.full and not any(getattr(full, k) for k in EXTRA_LEGS)


def test_plain_dump_still_runs_every_timed_mode_it_writes():
    """--dump-outputs writes the same files with or without --full: a plain run keeps the other timed modes for them,
    but not the CPU baseline or the oracle check."""
    import bench
    dump = bench.parse_args(['--gpus', '1', '--steps', '20', '--warmup', '5', '--dump-outputs', 'out'])
    assert not dump.no_alt and not dump.no_config5 and dump.no_cpu_baseline and dump.no_parity
    small = bench.parse_args(['--batch', '2', '--dump-outputs', 'out'])
    assert not small.no_alt and small.no_config5                            # the same files as --full at this shape
    assert bench.parse_args(['--dump-outputs', 'out', '--no-alt']).no_alt


def test_full_command_keeps_the_single_leg_switches():
    import bench
    args = bench.parse_args(['--full', '--no-cpu-baseline', '--no-alt'])
    assert args.no_cpu_baseline and args.no_alt and not args.no_config5 and not args.no_parity
    assert bench.parse_args(['--full', '--batch', '2']).no_config5          # config5 rides behind the default shape only
    c5 = bench.parse_args(['--full', '--config', '5'])
    assert (c5.dtype, c5.batch, c5.segments, c5.size) == ('bf16', 64, 16, 256)
    assert c5.no_alt and c5.no_config5 and c5.no_cpu_baseline and not c5.no_parity


@pytest.mark.gpu
def test_plain_run_times_the_headline_alone(hip_lib, tmp_path):
    """A plain run prints the headline fields and the roofline of its own timed steps and leaves every other object off
    the line, even when it times the other mode for --dump-outputs; the dump holds the files a --full run writes, and the
    headline's logits are the forward of bench.py's seeded clips, at the parity tests' bar."""
    import torch
    from oracle import tsm_oracle
    from workoutdetector_amd.weights import make_state_dict, to_torch
    env = {k: v for k, v in os.environ.items()
           if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT', 'TSM_BENCH_REHEARSAL', 'TSM_BENCH_FORCE_COLLECTIVE')}
    out_dir = tmp_path / 'out'
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                          '--batch', '2', '--dump-outputs', str(out_dir)],
                         capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout[-3000:]
    line = json.loads(lines[0])
    assert line['metric'] == 'clips/sec (8x3x224x224 TSM-R50)' and line['unit'] == 'clips/s'
    assert line['higher_is_better'] is True and line['dtype'] == 'f32' and line['steps'] == 3
    assert line['value'] > 0 and abs(line['value'] - 2 * 1e3 / line['ms_per_step']) <= 1e-3 * line['value']
    assert not {'alt_precision', 'config5', 'cpu_baseline', 'parity', 'exchange'} & set(line)
    roof = line['roofline']
    assert roof['achieved'] > 0 and roof['launches_timed'] > 0 and 'forward_kernel_ms' not in roof
    assert sorted(os.listdir(out_dir)) == ['alt_precision_logits.npy', 'logits.npy']
    got = np.load(out_dir / 'logits.npy')
    assert got.dtype == np.float32 and got.shape == (2, 12)
    clips = torch.randn(2, 8, 3, 224, 224, device='cuda', generator=torch.Generator(device='cuda').manual_seed(0))
    want = tsm_oracle.tsm_forward(to_torch(make_state_dict(0, 12)), clips.cpu(), n_segment=8).numpy()
    assert_close(got, want, rtol=1e-3, atol_scale=1e-5, what='logits')
