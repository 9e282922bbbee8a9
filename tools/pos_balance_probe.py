"""Live-balanced XCD runs of the position-major 3x3 launches (TSM_POS_BALANCE) against equal-count runs, per launch, in ONE
process.

    python tools/pos_balance_probe.py [--clips 32] [--rounds 9] [--size 224] [--out profiles/pos_balance_ab.txt]

Two comparisons on the fp32 engine, the engines of each alternating forward by forward so that clock and cache state drift
hits both alike; a layer's time is the median over the rounds of the engine's own per-launch event timing:

  forced   TSM_CONV_CODE = 3|0x80 and 3|0x80|0x200 without tuning, each with TSM_POS_BALANCE = 0 and 1: every segmented 3x3
           launch on the position-major instantiation, whole-K and with the tail split.  The stop-point figure: a launch ends
           with its heaviest XCD, so the balanced launches of layer3 / layer4 must be faster by about the equal-count excess
           (tests/pos_balance_host.cpp prints it), or the XCDs do not finish apart as the live-work count says.
  tuned    TSM_POS_BALANCE = 0 / 1 with the autotuner: the codes picked, their times, the forward's.

Logits of all engines must be bit-identical."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pos_major_probe import alternate, make_engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from workoutdetector_amd.weights import make_state_dict, to_torch
    os.environ.pop('TSM_POS_BALANCE', None)
    sd = to_torch(make_state_dict(0, 12))
    x = np.random.default_rng(7).standard_normal((a.clips, 8, 3, a.size, a.size)).astype(np.float32)
    lines = [f'# tools/pos_balance_probe.py --clips {a.clips} --rounds {a.rounds} --size {a.size}: fp32, {a.clips * 8} frames; '
             f'median of {a.rounds} alternating forwards, per-launch event times in us']

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    # ---- forced ----
    forced = {'pos equal': (3 | 0x80, '0'), 'pos balanced': (3 | 0x80, '1'), 'pos|tailK equal': (3 | 0x80 | 0x200, '0'),
              'pos|tailK balanced': (3 | 0x80 | 0x200, '1')}
    engines = {k: make_engine(sd, a.clips, a.size, {'TSM_AUTOTUNE': '0', 'TSM_CONV_CODE': str(code), 'TSM_FUSE_CONV23': '0',
                                                    'TSM_POS_BALANCE': bal}) for k, (code, bal) in forced.items()}
    res = alternate(engines, x, a.rounds)
    for e in engines.values():
        e.close()
    ref = res['pos equal'][2]
    conv2 = [n for n in res['pos equal'][0] if n.endswith('.conv2') and not n.startswith('layer1.')]
    emit('\n## forced codes (no tuning, no conv2+conv3 fusion): segmented 3x3 launches')
    emit(f'{"layer":18s} ' + ' '.join(f'{k:>18s}' for k in forced) + '   bal/eq  bal/eq (tailK)')
    for n in conv2:
        t = {k: res[k][0][n] * 1e3 for k in forced}
        emit(f'{n:18s} ' + ' '.join(f'{t[k]:18.1f}' for k in forced) +
             f'   {t["pos balanced"] / t["pos equal"]:6.4f}  {t["pos|tailK balanced"] / t["pos|tailK equal"]:6.4f}')
    for k in forced:
        emit(f'sum of the rows, {k:18s}: {sum(res[k][0][n] for n in conv2) * 1e3:9.1f} us; logits bit-identical: {np.array_equal(res[k][2], ref)}')
        assert np.array_equal(res[k][2], ref), k

    # ---- tuned ----
    engines = {'TSM_POS_BALANCE=0': make_engine(sd, a.clips, a.size, {'TSM_POS_BALANCE': '0'}),
               'TSM_POS_BALANCE=1': make_engine(sd, a.clips, a.size, {'TSM_POS_BALANCE': '1'})}
    res = alternate(engines, x, a.rounds)
    tiles = {k: e.conv_tiles(a.clips) for k, e in engines.items()}
    for e in engines.values():
        e.close()
    k0, k1 = list(engines)
    emit('\n## tuned engines')
    emit(f'{"layer":18s} {"tile, " + k0:>30s} {"us":>8s} {"tile, " + k1:>30s} {"us":>8s}   ratio')
    for n in conv2:
        t0, t1 = res[k0][0][n] * 1e3, res[k1][0][n] * 1e3
        if t0 <= 0 or t1 <= 0:       # (inside a fused launch)
            continue
        emit(f'{n:18s} {tiles[k0][n]:>30s} {t0:8.1f} {tiles[k1][n]:>30s} {t1:8.1f}   {t1 / t0:6.4f}')
    emit(f'sum of all launches: {res[k0][1] * 1e3:.1f} us ({k0}), {res[k1][1] * 1e3:.1f} us ({k1}); ratio {res[k1][1] / res[k0][1]:.4f}')
    same = np.array_equal(res[k0][2], res[k1][2]) and np.array_equal(res[k0][2], ref)
    emit(f'logits bit-identical across all engines: {same}')
    assert same
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
