"""Golden vectors for consensus_type='identity', made by EXECUTING the reference's own SegmentConsensus (build container only).

Like make_reference_vectors.py: the reference's source file is read as text at run time, the class definition is pulled out
with ``ast`` and executed in a scratch namespace, and only INPUTS and OUTPUTS are stored (no reference source text):

  ref_consensus_identity.npz   SegmentConsensus('identity', 1)(x).squeeze(1)   models/tsm.py:157-174, 418-419
                               x{i} [B, T, C] per-segment fc outputs -> y{i} (what TSM.forward returns), for T > 1

Run:  python tests/golden/make_consensus_identity_vectors.py <root of the reference checkout>
Tests only read the committed fixture.
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _extract_class(path, name):
    tree = ast.parse(open(path).read())
    (node,) = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name]
    ns = dict(torch=torch, nn=torch.nn)
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, 'exec'), ns)
    return ns[name]


def main(ref_root):
    rng = np.random.default_rng(20261016)
    Consensus = _extract_class(os.path.join(ref_root, 'workoutdetector', 'models', 'tsm.py'), 'SegmentConsensus')
    out = {}
    for i, (b, t, c) in enumerate([(1, 8, 12), (4, 8, 12), (3, 16, 5), (2, 4, 7), (5, 2, 1)]):
        x = torch.from_numpy(rng.standard_normal((b, t, c)).astype(np.float32))
        y = Consensus('identity', 1)(x).squeeze(1)      # TSM.forward: output = self.consensus(o); return output.squeeze(1)
        out[f'x{i}'] = x.numpy()
        out[f'y{i}'] = y.numpy()
    np.savez_compressed(os.path.join(HERE, 'ref_consensus_identity.npz'), **out)
    print('consensus identity cases:', len(out) // 2)


if __name__ == '__main__':
    main(sys.argv[1])
