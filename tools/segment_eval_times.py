"""Launch time of the two device steps of ``eval_classification`` beside the unfused routes they replace.  DESIGN 4.16.

    python tools/segment_eval_times.py <out.json> [clips]

* ``tsm_preprocess_indexed`` (frames picked through a device table + resize + crop + normalise + pack in one launch) against
  torch ``index_select`` of the raw frames followed by ``tsm_preprocess`` on the picked copy, for 32 clips of 8 frames out of
  720 x 1280 uint8 frames, into NTHWC4 and NTHWC8B.  The table is what ``sample_frames`` gives for segments of 3 to 40 frames
  laid end to end: repeated frames, no shared windows.
* ``tsm_top1_tally`` (arg-max, compare, count per class, on the device) against a D2H copy of the logits plus a NumPy tally.

Per arm: 5 warm-up rounds, then 30 rounds in which the fused and the unfused arm alternate -- device events around the device
arms, a host clock around the arm that ends on the host; the median (and min / max) of the 30 is reported.  Bytes of the fused
launch: the packed output it stores, plus the source it reads, bracketed -- from below by its taps (4 per output pixel, 3 bytes
each: neighbouring pixels share taps, and a 2.8x downscale skips source pixels), from above by every source pixel under the crop
window once per row that samples the frame (rows that repeat a frame hit the cache).  GB/s is given for both brackets over the
median.  No ratio is asserted anywhere: the file records what was measured, on which device and build."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from workoutdetector_amd import _lib                                                   # noqa: E402
from workoutdetector_amd.classification import sample_frames                          # noqa: E402
from workoutdetector_amd.engine import preprocess_frames, preprocess_indexed, top1_tally   # noqa: E402

out_path = sys.argv[1]
B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
H, W, RESIZE, CROP, WARM, ROUNDS, T, CLASSES = 720, 1280, 256, 224, 5, 30, 8, 12

# segments of 3 .. 40 frames end to end; the staged buffer is the union of their sampled frames
rows, start = [], 0
for c in range(B):
    total = (3, 8, 17, 30, 5, 40, 12, 1)[c % 8]
    rows.append(sample_frames(total, T, start))
    start += total
union = sorted(set().union(*rows))
table = torch.from_numpy(np.searchsorted(union, np.asarray(rows)).astype(np.int32)).cuda()
g = torch.Generator().manual_seed(0)
frames = torch.randint(0, 256, (len(union), H, W, 3), dtype=torch.uint8, generator=g).cuda()
flat = table.reshape(-1).long()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed_host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(prefix, ts):
    return {f'{prefix}_ms_median': statistics.median(ts), f'{prefix}_ms_min': min(ts), f'{prefix}_ms_max': max(ts)}


res = {'clips': B, 'frames': [H, W], 'staged_frames': len(union), 'resize': RESIZE, 'crop': CROP, 'rounds': ROUNDS,
       'device': torch.cuda.get_device_name(0), 'build': _lib.load().tsm_build_id().decode()}
for name, layout, group_bytes in (('NTHWC4', _lib.LAYOUT_NTHWC4, 16 * CROP * CROP), ('NTHWC8B', _lib.LAYOUT_NTHWC8B, 8 * CROP * CROP)):
    fused_out = preprocess_indexed(frames, table, RESIZE, CROP, layout=layout)
    picked = torch.index_select(frames, 0, flat)
    unfused_out = preprocess_frames(picked, RESIZE, CROP, scale_255=True, layout=layout)
    assert torch.equal(fused_out.view(torch.int32).reshape(-1), unfused_out.view(torch.int32).reshape(-1))

    def fused():
        preprocess_indexed(frames, table, RESIZE, CROP, layout=layout, out=fused_out)

    def unfused():
        torch.index_select(frames, 0, flat, out=picked)
        preprocess_frames(picked, RESIZE, CROP, scale_255=True, layout=layout, out=unfused_out)

    for _ in range(WARM):
        fused()
        unfused()
    torch.cuda.synchronize()
    t_f, t_u = [], []
    for _ in range(ROUNDS):
        t_f.append(timed(fused))
        t_u.append(timed(unfused))
    stores, taps = B * T * group_bytes, B * T * CROP * CROP * 4 * 3
    nh, nw = (RESIZE, int(RESIZE * W / H)) if H <= W else (int(RESIZE * H / W), RESIZE)
    window = B * T * (-(-CROP * H // nh)) * (-(-CROP * W // nw)) * 3          # source pixels under the crop window, per row
    m = statistics.median(t_f)
    res[name] = {**stats('fused', t_f), **stats('unfused_pair', t_u), 'fused_store_bytes': stores,
                 'fused_tap_bytes': taps, 'fused_window_source_bytes': window, 'unfused_picked_copy_bytes': 2 * B * T * H * W * 3,
                 'fused_gb_per_s_taps': (stores + taps) / (m * 1e-3) / 1e9,
                 'fused_gb_per_s_window': (stores + window) / (m * 1e-3) / 1e9}

# the tally: a batch of B rows of logits
logits = torch.randn((B, CLASSES), generator=g).cuda()
labels_host = np.arange(B) % CLASSES
labels = torch.from_numpy(labels_host.astype(np.int32)).cuda()
counters = torch.zeros((2, CLASSES), dtype=torch.int32).cuda()
pred = torch.empty((B,), dtype=torch.int32, device='cuda')
host_counts = np.zeros((2, CLASSES), dtype=np.int64)
pinned = torch.empty((B, CLASSES), dtype=torch.float32).pin_memory()


def device_tally():
    top1_tally(logits, labels, counters[0], counters[1], out=pred)


def host_tally():
    pinned.copy_(logits, non_blocking=True)
    torch.cuda.synchronize()
    p = pinned.numpy().argmax(axis=1)
    np.add.at(host_counts[1], labels_host, 1)
    np.add.at(host_counts[0], labels_host[p == labels_host], 1)


for _ in range(WARM):
    device_tally()
    host_tally()
torch.cuda.synchronize()
t_d, t_dh, t_h = [], [], []
for _ in range(ROUNDS):
    t_d.append(timed(device_tally))
    t_dh.append(timed_host(device_tally))
    t_h.append(timed_host(host_tally))
res['top1_tally'] = {'rows': B, 'num_class': CLASSES, **stats('device_kernel', t_d), **stats('device_launch_to_done_host_clock', t_dh),
                     **stats('d2h_plus_numpy_host_clock', t_h), 'logits_bytes': B * CLASSES * 4}
print(json.dumps(res))
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
