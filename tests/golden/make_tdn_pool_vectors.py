"""Generate tests/golden/ref_tdn_sample_indices.json by EXECUTING the reference's own ``TDNDataset.sample_indices`` (build
container only), by make_tdn_vectors.py's method: datasets/tdn_dataset.py is read as text at run time, the one method is pulled
out of the class with ``ast`` and executed with NumPy alone under ``np.random.seed``.  The fixture holds the recorded INTEGERS
only (data, no reference text):

  cases   [{"total", "num_segments", "seed", "offsets": [T]}] for totals 3, 5, 8, 9, 11, 12, 13, 40, 300, T = 8 and 3, seeds 0 .. 2;
          num_frames = 5.  ``randint`` of the module is numpy.random's: the global stream seeded with ``seed`` is the stream of
          ``np.random.RandomState(seed)``.

Run:  python tests/golden/make_tdn_pool_vectors.py [path of the reference's workoutdetector package]
"""
import ast
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

TOTALS = (3, 5, 8, 9, 11, 12, 13, 40, 300)
SEGMENTS = (8, 3)
SEEDS = (0, 1, 2)


def reference_method(ref_root):
    tree = ast.parse(open(os.path.join(ref_root, 'datasets', 'tdn_dataset.py')).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'TDNDataset']
    assert len(cls) == 1
    fn = [n for n in cls[0].body if isinstance(n, ast.FunctionDef) and n.name == 'sample_indices']
    assert len(fn) == 1
    fn[0].returns = None
    for a in fn[0].args.args:
        a.annotation = None
    ns = dict(np=np, randint=np.random.randint)
    exec(compile(ast.Module(body=fn, type_ignores=[]), 'tdn_dataset.py', 'exec'), ns)
    return ns['sample_indices']


def main():
    if len(sys.argv) > 1:
        ref_root = sys.argv[1]
    else:
        from make_reference_vectors import REF as ref_root
    sample_indices = reference_method(ref_root)
    cases = []
    for T in SEGMENTS:
        me = types.SimpleNamespace(num_segments=T, num_frames=5)
        for total in TOTALS:
            for seed in SEEDS:
                np.random.seed(seed)
                got = sample_indices(me, list(range(total)))
                cases.append(dict(total=total, num_segments=T, seed=seed, offsets=[int(v) for v in got]))
    path = os.path.join(HERE, 'ref_tdn_sample_indices.json')
    with open(path, 'w') as f:
        json.dump(dict(num_frames=5, cases=cases), f, indent=0)
        f.write('\n')
    print(f'wrote {path}: {len(cases)} cases')


if __name__ == '__main__':
    main()
