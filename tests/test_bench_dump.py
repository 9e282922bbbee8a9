"""bench.py --dump-outputs: the logits of the last timed step as .npy files (the size rule on CPU, a real run on the GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests._util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_writes_float32_whole_below_the_limit(tmp_path):
    import bench
    a = np.random.default_rng(1).standard_normal((7, 12))
    bench.dump_outputs(str(tmp_path / 'out'), {'logits': a})
    got = np.load(tmp_path / 'out' / 'logits.npy')
    assert got.dtype == np.float32 and np.array_equal(got, a.astype(np.float32))


def test_dump_keeps_the_same_seeded_rows_past_the_limit(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 30 * 12 * 4)          # room for 30 rows of 12 float32 in all
    big = np.arange(100 * 12, dtype=np.float64).reshape(100, 12)
    small = np.arange(20 * 12, dtype=np.float64).reshape(20, 12)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), {'big': big, 'small': small})
    written = 0
    for name, src in (('big', big), ('small', small)):
        a, b = np.load(tmp_path / 'a' / f'{name}.npy'), np.load(tmp_path / 'b' / f'{name}.npy')
        assert a.dtype == np.float32 and np.array_equal(a, b)           # the same sample on every run
        rows = (a[:, 0] // 12).astype(int)
        assert 0 < len(rows) < len(src) and (np.diff(rows) > 0).all()   # a subset of the rows, in order
        assert np.array_equal(a, src[rows].astype(np.float32))
        written += a.nbytes
    assert written <= bench.DUMP_LIMIT_BYTES


@pytest.mark.gpu
def test_bench_dumps_what_the_timed_steps_returned(hip_lib, tmp_path):
    """The dumped logits of both timed modes are the forward of bench.py's seeded clips: re-created here from the same seed,
    they agree with the CPU oracle at the parity tests' bar; a non-default shape has no config5 leg and so no config5 file."""
    import torch
    from oracle import tsm_oracle
    from workoutdetector_amd.weights import make_state_dict, to_torch
    env = {k: v for k, v in os.environ.items()
           if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT', 'TSM_BENCH_REHEARSAL', 'TSM_BENCH_FORCE_COLLECTIVE')}
    out_dir = tmp_path / 'out'
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                          '--batch', '2', '--no-cpu-baseline', '--dump-outputs', str(out_dir)],
                         capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{')][-1])
    assert line['steps'] == 3 and line['ms_per_step'] > 0
    assert sorted(os.listdir(out_dir)) == ['alt_precision_logits.npy', 'logits.npy']
    clips = torch.randn(2, 8, 3, 224, 224, device='cuda', generator=torch.Generator(device='cuda').manual_seed(0))
    want = tsm_oracle.tsm_forward(to_torch(make_state_dict(0, 12)), clips.cpu(), n_segment=8).numpy()
    for name in ('logits', 'alt_precision_logits'):
        got = np.load(out_dir / f'{name}.npy')
        assert got.dtype == np.float32 and got.shape == (2, 12)
        assert_close(got, want, rtol=1e-3, atol_scale=1e-5, what=name)
