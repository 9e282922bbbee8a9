"""Launch time of ``tsm_cosine_distances`` (one shot, the whole matrix) beside the expression a user of engine-external
features would otherwise write -- ``torch.mm(u, u.T)``, ``rsub``, ``clamp``, ``fill_diagonal_`` (a hipBLAS GEMM plus three
elementwise launches) -- for N = 1024 / 4096 rows of c = 512 / 2048 channels; then ``similarity.self_similarity`` end to end on
a synthetic 1024-frame 720 x 1280 video (R18 f32 feature engine, 32 frames per batch).  DESIGN 4.17.

    python tools/similarity_times.py <out.json> [video_frames]

Per shape: 5 warm-up rounds, then 30 rounds in which the two forms alternate, each between its own pair of device events; the
median (and min / max) of the 30 is reported, and ``tflops`` counts the N^2 c multiply-adds the torch expression performs (the
hand kernel computes the lower triangle only and mirrors it).  End to end: one warm-up pass (it tunes), then 3 timed passes
from host frames, wall clock around a final synchronise; ``band_launch_ms_total`` is the sum of the distance launches alone,
timed in a separate pass over the finished unit rows."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch            # noqa: E402

from workoutdetector_amd import _lib, similarity                                       # noqa: E402
from workoutdetector_amd.engine import cosine_distances, create_feature_model          # noqa: E402

out_path = sys.argv[1]
FRAMES = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
H, W, WARM, ROUNDS, BATCH = 720, 1280, 5, 30, 32


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(t):
    return {'ms_median': statistics.median(t), 'ms_min': min(t), 'ms_max': max(t)}


res = {'rounds': ROUNDS, 'device': torch.cuda.get_device_name(0), 'build': _lib.load().tsm_build_id().decode(), 'one_shot': {}}
g = torch.Generator().manual_seed(0)
for n in (1024, 4096):
    for c in (512, 2048):
        u = torch.relu(torch.randn(n, c, generator=g))
        u = (u / u.norm(dim=1, keepdim=True)).cuda()
        ours, kept = torch.empty(n, n, device='cuda'), {}

        def hand():
            cosine_distances(u, out=ours)

        def expr():
            kept['d'] = torch.rsub(torch.mm(u, u.t()), 1.0).clamp_(0.0, 2.0).fill_diagonal_(0.0)

        for _ in range(WARM):
            hand()
            expr()
        torch.cuda.synchronize()
        t_h, t_e = [], []
        for _ in range(ROUNDS):
            t_h.append(timed(hand))
            t_e.append(timed(expr))
        flops, theirs = 2.0 * n * n * c, kept['d']
        h, e = stats(t_h), stats(t_e)
        res['one_shot'][f'n{n}_c{c}'] = {
            'cosine_dist_kernel': dict(h, tflops=flops / (h['ms_median'] * 1e-3) / 1e12),
            'torch_mm_rsub_clamp_fill': dict(e, tflops=flops / (e['ms_median'] * 1e-3) / 1e12),
            'ratio_hand_to_torch': h['ms_median'] / e['ms_median'],
            'max_abs_difference': float((ours - theirs).abs().max()),
            'symmetric_hand': bool(torch.equal(ours, ours.t())), 'symmetric_torch': bool(torch.equal(theirs, theirs.t()))}

# ---- end to end: R18 f32 feature engine, 720p frames ----
block = torch.randint(0, 256, (64, H, W, 3), dtype=torch.uint8, generator=g)
video = block.repeat(max(1, FRAMES // 64), 1, 1, 1)[:FRAMES]
eng = create_feature_model('resnet18', max_frames=BATCH)
similarity.self_similarity(eng, video, batch_frames=BATCH)
torch.cuda.synchronize()
walls = []
for _ in range(3):
    t0 = time.perf_counter()
    d = similarity.self_similarity(eng, video, batch_frames=BATCH)
    torch.cuda.synchronize()
    walls.append(time.perf_counter() - t0)
unit = similarity.video_features(eng, video, normalize=True, batch_frames=BATCH)
n = int(unit.shape[0])
mat = torch.empty(n, n, device='cuda')


def bands():
    for lo in range(0, n, BATCH):
        cosine_distances(unit, out=mat, rows=(lo, min(n, lo + BATCH)))


bands()
torch.cuda.synchronize()
t_b = [timed(bands) for _ in range(5)]
t_f = [timed(lambda: similarity.video_features(eng, video[:BATCH].cuda(), normalize=True, batch_frames=BATCH)) for _ in range(5)]


def expr_e2e():
    return torch.rsub(torch.mm(unit, unit.t()), 1.0).clamp_(0.0, 2.0).fill_diagonal_(0.0)


expr_e2e()
t_x = [timed(expr_e2e) for _ in range(5)]
res['end_to_end'] = {'model': 'resnet18 f32', 'video_frames': n, 'frame_hw': [H, W], 'batch_frames': BATCH,
                     'wall_s_median': statistics.median(walls), 'wall_s_min': min(walls), 'wall_s_max': max(walls),
                     'frames_per_s': n / statistics.median(walls),
                     'band_launches': (n + BATCH - 1) // BATCH, 'band_launch_ms_total': statistics.median(t_b),
                     'one_batch_preprocess_forward_pool_ms': statistics.median(t_f),
                     'torch_expression_on_all_rows_ms': statistics.median(t_x),
                     'bands_equal_one_shot': bool(torch.equal(mat, cosine_distances(unit))), 'bands_equal_pipeline': bool(torch.equal(mat, d))}
eng.close()
print(json.dumps(res))
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
