"""Position-major 3x3 launches (tile code bit 0x80) against the natural order, per launch, in ONE process.

    python tools/pos_major_probe.py [--clips 32] [--rounds 7] [--size 224] [--out profiles/pos_major_ab.txt]

Two comparisons on the fp32 engine, the engines of each alternating forward by forward so that clock and cache state drift
hits both alike; a layer's time is the median over the rounds of the engine's own per-launch event timing:

  forced   TSM_CONV_CODE = 3 / 3|0x80 and 3|0x200 / 3|0x80|0x200 without tuning: every segmented 3x3 launch on the natural
           and on the position-major instantiation, whole-K and with the tail split.  The stop-point figure: the stride-1
           launches of layer3 / layer4 must be faster position-major, or the memory side has eaten the MFMAs saved.
  tuned    TSM_POS_MAJOR = 0 / 1 with the autotuner: which layers picked the form, their times, the forward's.

Logits of all engines must be bit-identical."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HOOKS = ('TSM_AUTOTUNE', 'TSM_CONV_CODE', 'TSM_POS_MAJOR', 'TSM_CONV_TILE', 'TSM_WALK')


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
    lines = [f'# tools/pos_major_probe.py --clips {a.clips} --rounds {a.rounds} --size {a.size}: fp32, {a.clips * 8} frames; '
             f'median of {a.rounds} alternating forwards, per-launch event times in us']

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    # ---- forced ----
    forced = {'3': 3, '3|pos': 3 | 0x80, '3|tailK': 3 | 0x200, '3|pos|tailK': 3 | 0x80 | 0x200}
    engines = {k: make_engine(sd, a.clips, a.size, {'TSM_AUTOTUNE': '0', 'TSM_CONV_CODE': str(v), 'TSM_FUSE_CONV23': '0'}) for k, v in forced.items()}
    res = alternate(engines, x, a.rounds)
    for e in engines.values():
        e.close()
    ref = res['3'][2]
    conv2 = [n for n in res['3'][0] if n.endswith('.conv2') and not n.startswith('layer1.')]
    emit('\n## forced codes (no tuning, no conv2+conv3 fusion): segmented 3x3 launches')
    emit(f'{"layer":18s} ' + ' '.join(f'{k:>12s}' for k in forced) + '   pos/nat  pos|tailK/tailK')
    for n in conv2:
        t = {k: res[k][0][n] * 1e3 for k in forced}
        emit(f'{n:18s} ' + ' '.join(f'{t[k]:12.1f}' for k in forced) + f'   {t["3|pos"] / t["3"]:7.4f}  {t["3|pos|tailK"] / t["3|tailK"]:7.4f}')
    for k in forced:
        emit(f'sum of the rows, {k:12s}: {sum(res[k][0][n] for n in conv2) * 1e3:9.1f} us; logits bit-identical to code 3: {np.array_equal(res[k][2], ref)}')
        assert np.array_equal(res[k][2], ref), k

    # ---- tuned ----
    engines = {'TSM_POS_MAJOR=0': make_engine(sd, a.clips, a.size, {'TSM_POS_MAJOR': '0'}),
               'TSM_POS_MAJOR=1': make_engine(sd, a.clips, a.size, {'TSM_POS_MAJOR': '1'})}
    res = alternate(engines, x, a.rounds)
    tiles = {k: e.conv_tiles(a.clips) for k, e in engines.items()}
    for e in engines.values():
        e.close()
    k0, k1 = list(engines)
    emit('\n## tuned engines')
    emit(f'{"layer":18s} {"tile, " + k0:>28s} {"us":>8s} {"tile, " + k1:>28s} {"us":>8s}   ratio')
    for n in conv2:
        t0, t1 = res[k0][0][n] * 1e3, res[k1][0][n] * 1e3
        if t0 <= 0 or t1 <= 0:       # (inside a fused launch)
            continue
        emit(f'{n:18s} {tiles[k0][n]:>28s} {t0:8.1f} {tiles[k1][n]:>28s} {t1:8.1f}   {t1 / t0:6.4f}')
    picked = [n for n in tiles[k1] if '/pos' in tiles[k1][n]]
    emit(f'layers on the position-major form: {len(picked)}: {", ".join(picked)}')
    emit(f'sum of all launches: {res[k0][1] * 1e3:.1f} us ({k0}), {res[k1][1] * 1e3:.1f} us ({k1})')
    same = np.array_equal(res[k0][2], res[k1][2]) and np.array_equal(res[k0][2], ref)
    emit(f'logits bit-identical across all engines: {same}')
    assert same
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
