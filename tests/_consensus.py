"""Shared pieces of the consensus_type='identity' tests (tests/test_consensus_cpu.py, tests/test_consensus_gpu.py).

The per-segment reference is written from the oracle's public pieces: ``tsm_oracle.trunk`` (fp32, or the bf16-storage
restatement), then ``adaptive_avg_pool2d`` + ``F.linear`` per frame and NO mean over the segments -- what the reference's
``TSM.forward`` returns with ``SegmentConsensus('identity')`` (tsm.py:409-419, 165-174: the consensus output is its input)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import tsm_oracle
from tests._util import BF16_E2E_BAR, make_input

BASE_MODELS = ('resnet18', 'resnet34', 'resnet50', 'wide_resnet50_2')
PLACES = ('blockres', 'block')
NUM_CLASS = 12
# whole-engine geometry: B = 3 clips through max_clips = 2 (two chunks), 24 (clip, segment) rows per case
B, T, H, W = 3, 8, 64, 64
F32_BAR = 1e-3            # rtol of the project's fp32 / split-bf16 logits bar (tests/test_engine_gpu.py)
MAX_EXEMPT_FRACTION = 8   # at most one (clip, segment) row in eight may be too close to a tie for an arg-max assertion
# Input seed per (base_model, shift_place): chosen ON THE CPU, with the oracle alone, so that the REFERENCE's near ties
# stay under the cap at both bars (tests/test_consensus_cpu.py asserts it for every case; weights are seed 0 throughout).
# Undecided rows of the reference, fp32 bar / bf16 bar, of 24: seed 1 gives resnet50 blockres 0 / 4 (over the cap of 3) and
# resnet50 block 1 / 3; seed 2 gives resnet50 blockres 0 / 2, seed 3 resnet50 block 0 / 1.  Every other case: at most 0 / 1.
INPUT_SEED = {('resnet50', 'blockres'): 2, ('resnet50', 'block'): 3}
DEFAULT_INPUT_SEED = 1


def state_dict(base_model, place, seed=0):
    from workoutdetector_amd.weights import make_state_dict
    sd = make_state_dict(seed=seed, num_class=NUM_CLASS, base_model=base_model, shift_place=place)
    return sd, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def case_input(base_model, place, b=B, t=T, h=H, w=W):
    return make_input(INPUT_SEED.get((base_model, place), DEFAULT_INPUT_SEED), b, t, h, w)


def rows_to_segments(rows, n_segment):
    """Per-frame fc rows [B*T, C], frames of a clip consecutive -> [B, T, C]: TSM.forward's ``o.view((-1, T) + o.size()[1:])``
    followed by the identity consensus and ``squeeze(1)`` (tsm.py:417-419; a no-op for T > 1)."""
    return rows.reshape(-1, n_segment, rows.shape[-1])


@torch.no_grad()
def per_segment_reference(sdt, x, base_model='resnet50', place='blockres', bf16=False, n_segment=8):
    """x [B,T,3,H,W] (ndarray or tensor) -> per-segment logits [B,T,num_class] (torch, fp32)."""
    x = torch.as_tensor(x)
    b = x.shape[0]
    feat = tsm_oracle.trunk(x.reshape((-1,) + tuple(x.shape[2:])).to(torch.float32), sdt, n_segment, base_model=base_model,
                            shift_place=place, bf16=bf16)
    o = F.linear(F.adaptive_avg_pool2d(feat, 1).flatten(1), sdt['fc.weight'], sdt['fc.bias'])
    out = rows_to_segments(o, n_segment)
    assert out.shape[0] == b
    return out


def decided_rows(ref, bar):
    """Boolean [B,T]: the rows of the reference whose top-2 margin exceeds twice `bar` times the logit scale -- only there
    is an arg-max a property of the model and not of the last bits of the arithmetic."""
    ref = np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max())
    top2 = np.sort(ref, axis=-1)[..., -2:]
    return (top2[..., 1] - top2[..., 0]) > 2.0 * bar * scale


def assert_argmax(got, ref, bar, what=''):
    """The arg-max rule: equality on the decided rows, and at most one row in eight undecided."""
    got, ref = np.asarray(got), np.asarray(ref)
    ok = decided_rows(ref, bar)
    exempt = int((~ok).sum())
    assert exempt * MAX_EXEMPT_FRACTION <= ok.size, f'{what}: {exempt} of {ok.size} rows are near ties at bar {bar:g}'
    same = got.argmax(-1) == ref.argmax(-1)
    assert same[ok].all(), f'{what}: arg-max differs on decided rows {np.argwhere(ok & ~same).tolist()}'
    return exempt


def bar_of(dtype):
    return BF16_E2E_BAR if dtype == 'bf16' else F32_BAR
