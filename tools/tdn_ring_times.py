"""Times of the TDN forward in two phases (``TsmEngine.tdn_segments`` + ``forward_ring``) against the whole forward,
and of ``TdnStreamBatcher``, at full depth (3, 4, 6, 3), 224 x 224, 32 consecutive clips of one video, on one GPU.

    python tools/tdn_ring_times.py <out.json> [clips]

CLIPS consecutive clips of the counting geometry from the middle of a 640 x 360 uint8 video staged on the device; the frames are
transformed once (``preprocess_frames(packed=False)``), outside every timed region.  In one process, 3 warm-up rounds, then 10
rounds in which these alternate, each between two device events:
  (a) ``forward_pool`` in window mode: the whole forward;
  (b) ``tdn_segments`` over the clips' unique segments and the pad segment (132 + 1 for 32 clips) + ``forward_ring``;
  each phase of (b) alone;
  a forward of each route with per-launch timing (an event pair around every launch): fuse2 as tdn_fuse_kernel and as
  tdn_fuse_ring_kernel, beside the bytes both must move over ``hbm_rate_bytes_per_s`` (the rate of profiles/tdn_times.json), and
  layer1's own launches, which profiles/tdn_times.json folds into "trunk convs".
Then ``TdnStreamBatcher`` with 1 and with 32 streams of 640 x 360 frames: per round every stream gets 8 frames and ``step()`` -- one
due clip per stream, upload, transform, 4 new segments and the trunk -- is timed on the host clock (it ends in its own sync), beside
``forward_pool`` of as many clips (frames already on the device and transformed: what the batcher's step adds is in the difference).
No figure here is a pass condition."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                # noqa: E402
import torch                      # noqa: E402

from workoutdetector_amd.engine import create_tdn_model, preprocess_frames      # noqa: E402
from workoutdetector_amd.tdn_pipeline import TdnSegmentRing, TdnStreamBatcher, tdn_frame_range      # noqa: E402
from workoutdetector_amd.transform import TestTransform                         # noqa: E402

out_path = sys.argv[1]
CLIPS = int(sys.argv[2]) if len(sys.argv) > 2 else 32
T, SIZE, WARM, ROUNDS, CLASSES = 8, 224, 3, 10, 12
HBM_RATE = 5.74e12
VH, VW, TOTAL, LO = 360, 640, 1000, 4


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {'ms_median': statistics.median(v), 'ms_min': min(v), 'ms_max': max(v)}


a0, b0 = tdn_frame_range(TOTAL, LO, LO + CLIPS)
nf = b0 - a0
rng = np.random.default_rng(0)
staged = torch.from_numpy(rng.integers(0, 256, (nf + 1, VH, VW, 3), dtype=np.uint8)).cuda()
staged[-1].zero_()
eng = create_tdn_model(CLASSES, num_segments=T, height=SIZE, width=SIZE, max_clips=CLIPS)
eng.warmup([CLIPS, 1])
pool = preprocess_frames(staged, resize=256, crop=SIZE, scale_255=False, packed=False)
window = dict(first_source_frame=a0, total_frames=TOTAL, first_clip=LO, clip_step=8, clip_stride=2, pad_frame=nf)

probe = TdnSegmentRing([], 0, T, 8, 2)
keys = probe.segments(LO, LO + CLIPS, TOTAL)
n_seg = len(keys) + 1
ring = TdnSegmentRing(list(range(n_seg - 2, -1, -1)), n_seg - 1, T, 8, 2)
ring.assign(keys)
table = torch.from_numpy(ring.table(LO, LO + CLIPS, TOTAL)).cuda()
seg_window = dict(first_source_frame=a0, total_frames=TOTAL, first_clip=probe.per * LO, clip_stride=2, pad_frame=nf)
sa, sd = eng.ring_shapes(n_seg)
ring_a, ring_d = torch.empty(sa, device='cuda'), torch.empty(sd, device='cuda')
out_a, out_b = torch.empty(CLIPS, CLASSES, device='cuda'), torch.empty(CLIPS, CLASSES, device='cuda')


def whole():
    eng.forward_pool(pool, window=window, n_clips=CLIPS, out=out_a)


def segments():
    eng.tdn_segments(pool, window=seg_window, n_segments=n_seg, out=(ring_a, ring_d))


def trunk():
    eng.forward_ring(ring_a, ring_d, table, n_clips=CLIPS, out=out_b)


def launches(fns):
    eng.set_layer_timing(len(fns))
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    return [{k: v for k, v in eng.layer_times_ms(i).items() if v >= 0} for i in range(len(fns))]


keys_t = ('whole', 'split', 'segments', 'trunk')
runs = {k: [] for k in keys_t}
per = {'whole': {}, 'segments': {}, 'trunk': {}}
for rnd in range(WARM + ROUNDS):
    got = {'whole': timed(whole), 'split': timed(lambda: (segments(), trunk())), 'segments': timed(segments), 'trunk': timed(trunk)}
    lw, ls, lt = launches([whole, segments, trunk])
    if rnd >= WARM:
        for k in keys_t:
            runs[k].append(got[k])
        for name, lm in (('whole', lw), ('segments', ls), ('trunk', lt)):
            for k, v in lm.items():
                per[name].setdefault(k, []).append(v)
torch.cuda.synchronize()
same = bool(torch.equal(out_a.view(torch.int32), out_b.view(torch.int32)))
res = {k: stats(v) for k, v in runs.items()}
med = {name: {k: statistics.median(v) for k, v in lm.items()} for name, lm in per.items()}


def share(lm, prefix):
    return sum(v for k, v in lm.items() if k.startswith(prefix))


N = CLIPS * T
hp, hd = SIZE // 4, SIZE // 8
fuse_bytes = N * (2 * hp * hp + hd * hd) * 256 * 4
per_segment = {k: share(med['whole'], k) for k in ('diff.front', 'diff.conv1_5', 'diff.maxpool', 'conv1', 'fuse1', 'resnext_layer1.', 'layer1.')}

# ---- streams ----------------------------------------------------------------------------------------------------------------
tf = TestTransform(256, SIZE, scale_255=False)
stream_stats = {}
for n_streams in (1, CLIPS):
    sb = TdnStreamBatcher(eng, transform=tf, max_batch=CLIPS)
    frames = [rng.integers(0, 256, (VH, VW, 3), dtype=np.uint8) for _ in range(16)]
    for s in range(n_streams):
        for i in range(17):
            sb.push(s, frames[i % 16])
    sb.step()                                   # clip 0 of every stream: 7 segments each
    steps, wholes = [], []
    for rnd in range(WARM + ROUNDS):
        for s in range(n_streams):
            for i in range(8):
                sb.push(s, frames[(i + rnd) % 16])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = sb.step()
        ms = (time.perf_counter() - t0) * 1e3
        assert sum(len(v) for v in done.values()) == n_streams
        w = timed(lambda: eng.forward_pool(pool, window=window, n_clips=n_streams, out=out_a[:n_streams]))
        if rnd >= WARM:
            steps.append(ms)
            wholes.append(w)
    stream_stats[str(n_streams)] = {'step': stats(steps), 'forward_pool_same_clips': stats(wholes), 'slots_in_use': sb.slots_in_use(),
                                    'ring_slots': int(sb._ring_a.shape[0])}
    for s in range(n_streams):
        sb.close(s)

spread_a = res['whole']['ms_max'] - res['whole']['ms_min']
saved = res['whole']['ms_median'] - res['split']['ms_median']
result = {
    'clips': CLIPS, 'segments': T, 'size': SIZE, 'depths': list(eng.tdn_depths), 'video': [VH, VW], 'rounds': ROUNDS,
    'device': torch.cuda.get_device_name(0), 'build': eng._lib.tsm_build_id().decode(), 'hbm_rate_bytes_per_s': HBM_RATE,
    'unique_segments': len(keys), 'segments_run': n_seg, 'segment_positions': N, 'logits_bit_identical': same,
    'a_whole_forward_pool': res['whole'], 'b_segments_plus_ring': res['split'], 'b_segments_alone': res['segments'], 'b_ring_alone': res['trunk'],
    'a_minus_b_ms': saved, 'a_spread_ms': spread_a, 'b_faster_than_a_by_more_than_a_spread': bool(saved > spread_a),
    'fuse2': {'tdn_fuse_kernel_ms': stats(per['whole']['fuse2']), 'tdn_fuse_ring_kernel_ms': stats(per['trunk']['fuse2']), 'bytes': fuse_bytes,
              'byte_bound_ms': fuse_bytes / HBM_RATE * 1e3},
    'per_segment_launches_of_the_whole_forward_ms': per_segment, 'per_segment_sum_ms': sum(per_segment.values()),
    'layer1_share_ms': per_segment['layer1.'], 'whole_forward_sum_of_launches_ms': sum(med['whole'].values()),
    'segment_phase_sum_of_launches_ms': sum(med['segments'].values()), 'trunk_phase_sum_of_launches_ms': sum(med['trunk'].values()),
    'ring_bytes': (ring_a.numel() + ring_d.numel()) * 4, 'slot_bytes': (ring_a[0].numel() + ring_d[0].numel()) * 4,
    'streams': stream_stats,
}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    json.dump(result, f, indent=1)
print(json.dumps({k: result[k] for k in ('logits_bit_identical', 'a_whole_forward_pool', 'b_segments_plus_ring', 'b_segments_alone', 'b_ring_alone',
                                         'a_minus_b_ms', 'a_spread_ms', 'fuse2', 'layer1_share_ms', 'per_segment_sum_ms', 'streams')}))
if not same:
    sys.exit('the two routes disagree')
