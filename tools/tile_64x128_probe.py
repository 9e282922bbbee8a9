"""The 64x128 tile of the fp32 unsegmented 1x1 convs (tile code 9) against 64x64, per launch, in ONE process.

    python tools/tile_64x128_probe.py [--clips 32] [--rounds 7] [--size 224] [--out profiles/tile_64x128_ab.txt]

Two comparisons on the fp32 engine, the engines of each alternating forward by forward so that clock and cache state drift
hits both alike; a layer's time is the median over the rounds of the engine's own per-launch event timing:

  forced   TSM_CONV_CODE = 3 / 9 without tuning and without the conv2 + conv3 fusion: every launch the tile applies to on the
           64x64 and on the 64x128 instantiation (code 9 falls back to the heuristic shape everywhere else: those rows are
           not printed).
  tuned    TSM_TILE_64X128 = 0 / 1 with the autotuner: which layers picked the tile, their times, the forward's.

Logits of all engines must be bit-identical."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HOOKS = ('TSM_AUTOTUNE', 'TSM_CONV_CODE', 'TSM_POS_MAJOR', 'TSM_TILE_64X128', 'TSM_CONV_TILE', 'TSM_WALK', 'TSM_FUSE_CONV23')


def make_engine(sd, clips, size, env):
    from workoutdetector_amd.engine import TsmEngine
    for k in HOOKS:
        os.environ.pop(k, None)
    os.environ.update(env)          # (the hooks are read once, in tsm_create)
    os.environ['TSM_TUNE_CACHE'] = 'off'
    eng = TsmEngine(height=size, width=size, max_clips=clips, state_dict=sd)
    for k in env:
        os.environ.pop(k, None)
    return eng


def alternate(engines, x, rounds):
    """{name: ({layer: median ms}, median forward ms, logits)}"""
    times = {k: [] for k in engines}
    total = {k: [] for k in engines}
    logits = {}
    for k, e in engines.items():     # tuning pass / first touch outside the timed rounds
        logits[k] = e.run(None, {'input': x})[0]
    for _ in range(rounds):
        for k, e in engines.items():
            e.set_layer_timing(1)
            out = e.run(None, {'input': x})[0]
            assert np.array_equal(out, logits[k]), f'{k}: logits changed between forwards'
            t = e.layer_times_ms(0)
            times[k].append(t)
            total[k].append(sum(v for v in t.values() if v > 0))
    med = {k: {n: statistics.median(t[n] for t in times[k]) for n in times[k][0]} for k in engines}
    return {k: (med[k], statistics.median(total[k]), logits[k]) for k in engines}


def eligible(sd, names):
    """The launches the tile applies to: a 1x1 conv to a multiple of 128 channels whose K is not segmented (K < 1024 fp32
    channels, a conv3's downsample operand included)."""
    out = []
    for n in names:
        key = f'base_model.{n}.weight' if f'base_model.{n}.weight' in sd else f'base_model.{n}.net.weight'   # (.net: behind the shift)
        if key not in sd or sd[key].shape[-1] != 1 or sd[key].shape[0] % 128:
            continue
        k = sd[key].shape[1]
        down = f'base_model.{n.rsplit(".", 1)[0]}.downsample.0.weight'
        if n.endswith('.conv3') and down in sd:
            k += sd[down].shape[1]
        if k < 1024:
            out.append(n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from workoutdetector_amd.weights import make_state_dict, to_torch
    sd = to_torch(make_state_dict(0, 12))
    x = np.random.default_rng(7).standard_normal((a.clips, 8, 3, a.size, a.size)).astype(np.float32)
    lines = [f'# tools/tile_64x128_probe.py --clips {a.clips} --rounds {a.rounds} --size {a.size}: fp32, {a.clips * 8} frames; '
             f'median of {a.rounds} alternating forwards, per-launch event times in us']

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    # ---- forced ----
    forced = {'64x64': 3, '64x128': 9}
    engines = {k: make_engine(sd, a.clips, a.size, {'TSM_AUTOTUNE': '0', 'TSM_CONV_CODE': str(v), 'TSM_FUSE_CONV23': '0'}) for k, v in forced.items()}
    res = alternate(engines, x, a.rounds)
    for e in engines.values():
        e.close()
    ref = res['64x64'][2]
    rows = eligible(sd, res['64x64'][0])
    emit('\n## forced codes (no tuning, no conv2+conv3 fusion): the launches the tile applies to')
    emit(f'{"layer":18s} ' + ' '.join(f'{k:>10s}' for k in forced) + '   64x128/64x64')
    for n in rows:
        t = {k: res[k][0][n] * 1e3 for k in forced}
        emit(f'{n:18s} ' + ' '.join(f'{t[k]:10.1f}' for k in forced) + f'   {t["64x128"] / t["64x64"]:7.4f}')
    for k in forced:
        emit(f'sum of the rows, {k:7s}: {sum(res[k][0][n] for n in rows) * 1e3:9.1f} us; logits bit-identical to 64x64: {np.array_equal(res[k][2], ref)}')
        assert np.array_equal(res[k][2], ref), k

    # ---- tuned ----
    engines = {'TSM_TILE_64X128=0': make_engine(sd, a.clips, a.size, {'TSM_TILE_64X128': '0'}),
               'TSM_TILE_64X128=1': make_engine(sd, a.clips, a.size, {'TSM_TILE_64X128': '1'})}
    res = alternate(engines, x, a.rounds)
    tiles = {k: e.conv_tiles(a.clips) for k, e in engines.items()}
    for e in engines.values():
        e.close()
    k0, k1 = list(engines)
    emit('\n## tuned engines')
    emit(f'{"layer":18s} {"tile, " + k0:>28s} {"us":>8s} {"tile, " + k1:>28s} {"us":>8s}   ratio')
    for n in rows:
        t0, t1 = res[k0][0][n] * 1e3, res[k1][0][n] * 1e3
        if t0 <= 0 or t1 <= 0:       # (inside a fused launch)
            continue
        emit(f'{n:18s} {tiles[k0][n]:>28s} {t0:8.1f} {tiles[k1][n]:>28s} {t1:8.1f}   {t1 / t0:6.4f}')
    picked = [n for n in tiles[k1] if tiles[k1][n].startswith('64x128')]
    emit(f'layers on the 64x128 tile: {len(picked)}: {", ".join(picked)}')
    emit(f'sum of all launches: {res[k0][1] * 1e3:.1f} us ({k0}), {res[k1][1] * 1e3:.1f} us ({k1})')
    same = np.array_equal(res[k0][2], res[k1][2]) and np.array_equal(res[k0][2], ref)
    emit(f'logits bit-identical across all engines: {same}')
    assert same
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
