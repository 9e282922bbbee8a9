"""Times of the TDN-ResNet50 engine (``create_tdn_model``) at 32 clips of 8 segments of 224 x 224, full depth, on one GPU.
DESIGN 4.25.

    python tools/tdn_times.py <out.json> [clips]
    python tools/tdn_times.py --pool <out.json> [clips]      the dense input route against the pool route (``pool_mode``)

In one process, 3 warm-up rounds, then 10 rounds in which these alternate, each between two device events:
  * a plain TDN forward (``forward_device``): clips/s of the whole forward;
  * a TDN forward with per-launch timing (``set_layer_timing``: an event pair around every launch, so each figure carries the
    pair's own cost, a few microseconds): per-launch medians, summed per launch kind;
  * the plain R50 engine with ``is_shift=False`` on the centre frames: what TDN costs over its trunk;
  * torch's fp32 eager run of tests/_tdn.py on the GPU with the same weights.
Every new launch stands beside its byte bound: the bytes it must touch (each operand once) over 5.74 TB/s, the rate
``temporal_maxpool_kernel`` reaches in profiles/temporal_pool_times.json.  The share of the forward spent on the patch rows
(diff.front + diff.conv1_5) decides whether a direct conv1_5 kernel is worth building.  No figure here is a pass condition."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                # noqa: E402
import torch                      # noqa: E402

from tests import _tdn                                                          # noqa: E402
from workoutdetector_amd import flops                                           # noqa: E402
from workoutdetector_amd.engine import create_model, create_tdn_model           # noqa: E402
from workoutdetector_amd.weights import TDN_DEPTHS, make_tdn_state_dict         # noqa: E402

POOL = '--pool' in sys.argv
if POOL:
    sys.argv.remove('--pool')
out_path = sys.argv[1]
CLIPS = int(sys.argv[2]) if len(sys.argv) > 2 else 32
T, SIZE, WARM, ROUNDS, CLASSES = 8, 224, 3, 10, 12
HBM_RATE = 5.74e12


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {'ms_median': statistics.median(v), 'ms_min': min(v), 'ms_max': max(v)}


def pool_mode():
    """``--pool``: CLIPS consecutive clips of the counting geometry (a clip every 8 frames, every 2nd frame, five
    frames per segment) from the middle of a 640 x 360 uint8 video staged on the device, two routes to the same logits:
      (a) the dense route: ``preprocess_indexed`` over all CLIPS * 40 table rows into [CLIPS, 8, 15, 224, 224], the NTCHW forward;
      (b) the pool route: ``preprocess_frames`` over the unique staged frames, ``forward_pool`` in window mode.
    3 warm-up rounds, then 10 rounds in which (a) and (b) alternate; per round also the transform launch of each route alone and
    a forward of each route with per-launch timing (diff.front per chunk: tdn_front_kernel against tdn_front_pool_kernel)."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import preprocess_frames, preprocess_indexed
    from workoutdetector_amd.tdn_pipeline import tdn_clip_indices, tdn_frame_range
    vh, vw, total, lo = 360, 640, 1000, 4
    a, b = tdn_frame_range(total, lo, lo + CLIPS)
    nf = b - a
    rng = np.random.default_rng(0)
    staged = torch.from_numpy(rng.integers(0, 256, (nf + 1, vh, vw, 3), dtype=np.uint8)).cuda()
    staged[-1].zero_()
    table = torch.from_numpy(tdn_clip_indices(total, lo, lo + CLIPS, T, 8, 2, a, nf, nf + 1).reshape(CLIPS, T * 5)).cuda()
    window = dict(first_source_frame=a, total_frames=total, first_clip=lo, clip_step=8, clip_stride=2, pad_frame=nf)
    eng = create_tdn_model(CLASSES, num_segments=T, height=SIZE, width=SIZE, max_clips=CLIPS)
    eng.warmup([CLIPS])
    dense = torch.empty(CLIPS, T * 5, 3, SIZE, SIZE, device='cuda')
    pool = torch.empty(nf + 1, 3, SIZE, SIZE, device='cuda')
    out_a, out_b = torch.empty(CLIPS, CLASSES, device='cuda'), torch.empty(CLIPS, CLASSES, device='cuda')
    kw = dict(resize=256, crop=SIZE, scale_255=False)

    def transform_a():
        preprocess_indexed(staged, table, layout=_lib.LAYOUT_NTCHW, out=dense, **kw)

    def transform_b():
        preprocess_frames(staged, packed=False, out=pool, **kw)

    def forward_a():
        eng.forward_device(dense.view(CLIPS, T, 15, SIZE, SIZE), out=out_a)

    def forward_b():
        eng.forward_pool(pool, window=window, n_clips=CLIPS, out=out_b)

    def fronts(forward):
        eng.set_layer_timing(1)
        forward()
        torch.cuda.synchronize()
        return {k: v for k, v in eng.layer_times_ms(0).items() if k.startswith('diff.front') and v >= 0}
    keys = ('route_a', 'route_b', 'transform_a', 'transform_b', 'forward_a', 'forward_b')
    runs = {k: [] for k in keys}
    front = {'tdn_front_kernel': {}, 'tdn_front_pool_kernel': {}}
    for rnd in range(WARM + ROUNDS):
        got = {'route_a': timed(lambda: (transform_a(), forward_a())), 'route_b': timed(lambda: (transform_b(), forward_b())),
               'transform_a': timed(transform_a), 'transform_b': timed(transform_b),
               'forward_a': timed(forward_a), 'forward_b': timed(forward_b)}
        fa, fb = fronts(forward_a), fronts(forward_b)
        if rnd >= WARM:
            for k in keys:
                runs[k].append(got[k])
            for name, f in (('tdn_front_kernel', fa), ('tdn_front_pool_kernel', fb)):
                for k, v in f.items():
                    front[name].setdefault(k, []).append(v)
    torch.cuda.synchronize()
    same = bool(torch.equal(out_a.view(torch.int32), out_b.view(torch.int32)))
    res = {k: stats(v) for k, v in runs.items()}
    spread_a = res['route_a']['ms_max'] - res['route_a']['ms_min']
    front_stats = {name: {k: stats(v) for k, v in f.items()} for name, f in front.items()}
    front_sum = {name: sum(v['ms_median'] for v in f.values()) for name, f in front_stats.items()}
    chunk_segments = eng.tdn_chunk_clips * T
    result = {
        'clips': CLIPS, 'segments': T, 'size': SIZE, 'video': [vh, vw], 'rounds': ROUNDS, 'device': torch.cuda.get_device_name(0),
        'build': eng._lib.tsm_build_id().decode(), 'staged_frames': nf + 1, 'table_rows': CLIPS * T * 5,
        'logits_bit_identical': same, **res,
        'route_b_minus_a_ms': res['route_b']['ms_median'] - res['route_a']['ms_median'], 'route_a_spread_ms': spread_a,
        'transform_b_over_a': res['transform_b']['ms_median'] / res['transform_a']['ms_median'],
        'diff_front_per_chunk': front_stats, 'diff_front_sum_ms': front_sum,
        'diff_front_bytes_per_chunk': chunk_segments * (15 * SIZE * SIZE + 4 * SIZE * SIZE + (SIZE // 4) ** 2 * 1024) * 4,
        'input_device_bytes': {'route_a_dense': dense.numel() * 4, 'route_b_pool': pool.numel() * 4,
                               'saved': (dense.numel() - pool.numel()) * 4},
    }
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: result[k] for k in ('logits_bit_identical', 'route_a', 'route_b', 'transform_a', 'transform_b', 'forward_a', 'forward_b',
                                             'diff_front_sum_ms', 'input_device_bytes')}))
    if not same:
        sys.exit('the two routes disagree')


if POOL:
    pool_mode()
    sys.exit(0)

eng = create_tdn_model(CLASSES, num_segments=T, height=SIZE, width=SIZE, max_clips=CLIPS)
plain = create_model(num_class=CLASSES, num_segments=T, is_shift=False, height=SIZE, width=SIZE, max_clips=CLIPS)
x = torch.from_numpy(np.random.default_rng(0).standard_normal((CLIPS, T, 15, SIZE, SIZE)).astype(np.float32)).cuda()
centre = x[:, :, 6:9].contiguous()
out, out_plain = torch.empty(CLIPS, CLASSES, device='cuda'), torch.empty(CLIPS, CLASSES, device='cuda')
eng.warmup([CLIPS])
plain.warmup([CLIPS])
model = _tdn.load(_tdn.TDN(CLASSES, T, TDN_DEPTHS), make_tdn_state_dict(0, CLASSES)).cuda()
flat = x.view(CLIPS * T, 15, SIZE, SIZE)


def eager():
    with torch.no_grad():
        return model(flat)


# bytes every new launch must touch, per frame of a clip (fp32)
N = CLIPS * T
bounds = {}
rows = (SIZE // 4) ** 2
chunk_frames = eng.tdn_chunk_clips * T
bounds['diff.front'] = chunk_frames * (15 * SIZE * SIZE + 4 * SIZE * SIZE + rows * 1024) * 4
bounds['diff.conv1_5'] = chunk_frames * rows * (1024 + 64) * 4
hp, hd = SIZE // 4, SIZE // 8
bounds['fuse1'] = N * (2 * hp * hp + hd * hd) * 64 * 4
bounds['fuse2'] = N * (2 * hp * hp + hd * hd) * 256 * 4
mse = {}
for li, c in ((2, 128), (3, 256), (4, 512)):
    for b in range(TDN_DEPTHS[li - 1]):
        side = SIZE // 2 ** (li if b == 0 else li + 1)      # the module works at the block's input size
        px, r, pq = side * side, c // 16, (side // 2) ** 2
        p = f'layer{li}.{b}'
        mse[p + '.mse_squeeze'] = N * px * (c + r) * 4
        mse[p + '.mse_diff'] = N * (px * 3 * r + pq * 2 * r) * 4
        mse[p + '.mse_s2'] = N * pq * 4 * r * 4
        mse[p + '.mse_mix'] = N * (px * 4 * r + pq * 2 * r) * 4
        mse[p + '.mse_excite_shift'] = N * px * (2 * c + 2 * r) * 4
bounds.update(mse)

whole, whole_plain, whole_torch, per_launch = [], [], [], {}
for rnd in range(WARM + ROUNDS):
    a = timed(lambda: eng.forward_device(x, out=out))
    eng.set_layer_timing(1)
    eng.forward_device(x, out=out)
    torch.cuda.synchronize()
    times = eng.layer_times_ms(0)
    b = timed(lambda: plain.forward_device(centre, out=out_plain))
    c = timed(eager)
    if rnd >= WARM:
        whole.append(a)
        whole_plain.append(b)
        whole_torch.append(c)
        for k, v in times.items():
            if v >= 0:
                per_launch.setdefault(k, []).append(v)

want = eager().float().cpu().numpy()
err = float(np.abs(out.cpu().numpy() - want).max() / np.abs(want).max())
med = {k: statistics.median(v) for k, v in per_launch.items()}


def kind(name):
    if name.startswith('diff.front') or name.startswith('diff.conv1_5'):
        return name.rsplit('.', 1)[0]
    if '.mse_' in name:
        return name.rsplit('.', 1)[1]
    if name.startswith('resnext_layer1'):
        return 'resnext_layer1 convs'
    return name if name in ('diff.maxpool', 'conv1', 'fuse1', 'fuse2', 'head') else 'trunk convs'


by_kind = {}
for k, v in med.items():
    by_kind[kind(k)] = by_kind.get(kind(k), 0.0) + v
launches = {}
for k, v in med.items():
    key = k.rsplit('.', 1)[0] if k.startswith(('diff.front', 'diff.conv1_5')) else k
    if key in bounds:
        bound_ms = bounds[key] / HBM_RATE * 1e3
        launches[k] = {'ms_median': v, 'bytes': bounds[key], 'byte_bound_ms': bound_ms, 'bound_over_measured': bound_ms / v}
total = sum(med.values())
w = statistics.median(whole)
result = {
    'clips': CLIPS, 'segments': T, 'size': SIZE, 'depths': list(TDN_DEPTHS), 'rounds': ROUNDS, 'device': torch.cuda.get_device_name(0),
    'build': eng._lib.tsm_build_id().decode(), 'hbm_rate_bytes_per_s': HBM_RATE,
    'tdn_forward': dict(stats(whole), clips_per_s=CLIPS / w * 1e3, tflops=flops.tdn_flops_per_clip(T, SIZE, SIZE, CLASSES) * CLIPS / w / 1e9),
    'plain_r50_no_shift_forward': dict(stats(whole_plain), clips_per_s=CLIPS / statistics.median(whole_plain) * 1e3),
    'torch_eager_fp32_forward': dict(stats(whole_torch), clips_per_s=CLIPS / statistics.median(whole_torch) * 1e3),
    'tdn_over_plain_r50': w / statistics.median(whole_plain), 'torch_over_tdn': statistics.median(whole_torch) / w,
    'logits_err_vs_torch_fp32': err,
    'per_kind_ms': by_kind, 'per_kind_share': {k: v / total for k, v in by_kind.items()},
    'patch_rows_share_of_forward': (by_kind.get('diff.front', 0.0) + by_kind.get('diff.conv1_5', 0.0)) / total,
    'long_term_share_of_forward': sum(v for k, v in by_kind.items() if k.startswith('mse_')) / total,
    'new_launches': launches,
    'conv_tiles': eng.conv_tiles(CLIPS),
}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    json.dump(result, f, indent=1)
print(json.dumps({k: result[k] for k in ('tdn_forward', 'plain_r50_no_shift_forward', 'torch_eager_fp32_forward', 'tdn_over_plain_r50',
                                         'patch_rows_share_of_forward', 'long_term_share_of_forward', 'logits_err_vs_torch_fp32', 'per_kind_ms')}))
