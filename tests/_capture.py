"""Stream capture and replay of enqueue-only library calls (DESIGN: the capture rule).

include/tsm_hip.h promises of most entry points that they only enqueue on the caller's stream.  On the null stream that
promise cannot fail: everything is ordered by luck.  A stream capture checks it without a race to win --

* work sent to any other stream, the null stream included, runs at capture time: it is missing from the graph (fewer kernel
  nodes than traced launches) and from the replay (a runtime may also refuse a null-stream launch while another stream
  captures: torch captures in ``global`` mode);
* a synchronisation or an allocation inside the capture is an error.

``captured`` runs one set of library calls (``run``) eagerly on three different inputs, captures it on a side stream,
shows that nothing ran at capture time, fills every intermediate buffer with another input's values, and then requires the
replays to reproduce the eager results bit for bit.  All comparisons are bitwise: each compares two runs of the same build,
and the library sums in a fixed order.  The graph is linear (one stream, no fork or join), and nothing here touches the
environment.
"""
import ctypes
import os

import torch

from tests._guard import POISON, check

SETS = ('A', 'B', 'C')
KERNEL_NODE = 0          # hipGraphNodeTypeKernel


def _poison(outputs):
    for o in outputs:
        o.view(torch.int32).fill_(POISON)          # (every output here has 4-byte elements: tests/_guard.py)


def _load(statics, values):
    assert len(statics) == len(values)
    for s, v in zip(statics, values):
        assert tuple(s.shape) == tuple(v.shape) and s.dtype == v.dtype, (tuple(s.shape), tuple(v.shape), s.dtype, v.dtype)
        s.copy_(v)


def _same(a, b):
    """Bit for bit: compared as 32-bit words, so -0.0 is not 0.0 and a NaN equals itself."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _still_poison(outputs):
    return all(bool((o.view(torch.int32) == POISON).all()) for o in outputs)


_hip = None


def _hip_runtime():
    """The HIP runtime this process already has loaded (torch's), never a second copy: its path from the process' own map,
    opened with RTLD_NOLOAD, which fails instead of loading anything."""
    global _hip
    if _hip is None:
        paths = set()
        with open('/proc/self/maps') as f:
            for line in f:
                path = line.split(None, 5)[-1].strip()
                if os.path.basename(path).startswith('libamdhip64.so'):
                    paths.add(path)
        assert len(paths) == 1, f'expected one loaded HIP runtime, found {sorted(paths)}'
        _hip = ctypes.CDLL(paths.pop(), mode=os.RTLD_NOLOAD | os.RTLD_NOW)
        _hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        _hip.hipGraphGetNodes.restype = ctypes.c_int
        _hip.hipGraphNodeGetType.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        _hip.hipGraphNodeGetType.restype = ctypes.c_int
    return _hip


def kernel_nodes(graph):
    """Number of kernel nodes of a kept ``torch.cuda.CUDAGraph`` (hipGraphGetNodes / hipGraphNodeGetType)."""
    hip = _hip_runtime()
    raw = ctypes.c_void_p(graph.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    st = hip.hipGraphGetNodes(raw, None, ctypes.byref(n))
    assert st == 0, f'hipGraphGetNodes: error {st}'
    nodes = (ctypes.c_void_p * max(n.value, 1))()
    st = hip.hipGraphGetNodes(raw, nodes, ctypes.byref(n))
    assert st == 0, f'hipGraphGetNodes: error {st}'
    count = 0
    for i in range(n.value):
        kind = ctypes.c_int(-1)
        st = hip.hipGraphNodeGetType(nodes[i], ctypes.byref(kind))
        assert st == 0, f'hipGraphNodeGetType: error {st}'
        count += kind.value == KERNEL_NODE
    return count


def captured(run, statics, fresh_inputs, outputs, *, inout=(), engine=None, refs_after=False):
    """Capture ``run()`` on a side stream and hold its replays to the eager results, bit for bit.

    ``run()`` makes the library calls on torch's current stream with every ``out=`` supplied; ``statics`` are its input
    tensors and ``outputs`` its output tensors, all from tests/_guard.py (``guarded`` / ``guarded_out``), allocated before
    the capture and reused.  ``fresh_inputs(k)`` for k = 0, 1, 2 returns the values of input sets A, B, C for ``statics``
    (seeded, pairwise different).  ``inout``: those of ``statics`` that ``run()`` also writes (accumulators): they are
    compared like outputs but never poisoned, and each run starts from the set's values.  ``engine``: the TsmEngine whose
    forward ``run()`` makes; step 6 then asks ``last_forward_ms`` first.  ``refs_after``: take the eager references after
    the replays instead of before the capture, for an engine whose first forward must be the captured one.

    Returns the launch trace of the capture (host-side: what was launched INTO the graph), with ``graph`` (the
    ``torch.cuda.CUDAGraph``), ``refs`` ({'A' | 'B' | 'C': clones of outputs + inout}) and ``kernel_nodes`` (or None where
    torch does not hand out the raw graph) as attributes."""
    from workoutdetector_amd.engine import launch_trace
    statics, outputs, inout = list(statics), list(outputs), list(inout)
    compared = outputs + inout
    sets = {name: [torch.as_tensor(v) for v in fresh_inputs(k)] for k, name in enumerate(SETS)}
    for a, b in (('A', 'B'), ('A', 'C'), ('B', 'C')):
        assert any(not torch.equal(u.cpu(), v.cpu()) for u, v in zip(sets[a], sets[b])), f'input sets {a} and {b} are equal'

    def eager(name):
        _load(statics, sets[name])
        _poison(outputs)
        run()
        torch.cuda.synchronize()
        check(*outputs, *statics)
        return [t.clone() for t in compared]

    def assert_equals(got_name, ref, what):
        for i, (t, r) in enumerate(zip(compared, ref)):
            assert _same(t, r), f'{what}: output {i} differs from the eager run of input set {got_name}'

    # 1. eager references (this also loads every code object)
    refs = {} if refs_after else {name: eager(name) for name in SETS}
    if not refs_after:
        assert any(not _same(a, b) for a, b in zip(refs['A'], refs['B'])), 'sets A and B give the same outputs'
        assert any(not _same(a, c) for a, c in zip(refs['A'], refs['C'])), 'sets A and C give the same outputs'

    # 2. capture on a fresh side stream, one stream, no fork or join
    _load(statics, sets['A'])
    _poison(outputs)
    torch.cuda.synchronize()
    keep = hasattr(torch.cuda.CUDAGraph, 'raw_cuda_graph')
    g = torch.cuda.CUDAGraph(keep_graph=True) if keep else torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with launch_trace() as tr:
        with torch.cuda.graph(g, stream=side):
            run()

    # 3. nothing ran at capture time
    torch.cuda.synchronize()
    assert _still_poison(outputs), 'an output was written while the stream was capturing: a launch escaped the capture'
    check(*statics)
    for t in inout:
        v = sets['A'][next(i for i, s in enumerate(statics) if s is t)]
        assert torch.equal(t.cpu(), v.cpu()), 'an accumulator changed while the stream was capturing'
    assert tr.kernels, 'the capture launched nothing'
    tr.kernel_nodes = None
    if keep:
        tr.kernel_nodes = kernel_nodes(g)
        assert tr.kernel_nodes == len(tr.kernels), (f'{tr.kernel_nodes} kernel nodes in the graph, {len(tr.kernels)} launches '
                                                    f'in the trace: {tr.kernels}')

    # 4. stale workspace: every intermediate buffer now holds C's values
    _load(statics, sets['C'])
    _poison(outputs)
    run()
    torch.cuda.synchronize()

    # 5. replay on B, then on A
    replayed = {}
    for name in ('B', 'A'):
        _load(statics, sets[name])
        _poison(outputs)
        g.replay()
        torch.cuda.synchronize()
        check(*outputs, *statics)
        if refs_after:
            replayed[name] = [t.clone() for t in compared]
        else:
            assert_equals(name, refs[name], f'replay of {name}')

    # 6. error hygiene: the next library call succeeds and reproduces C
    if engine is not None:
        ms = engine.last_forward_ms
        assert isinstance(ms, float) and ms == ms, ms
    after = eager('C')
    if refs_after:
        refs = {'C': after, 'A': eager('A'), 'B': eager('B')}
        for name in ('B', 'A'):
            for i, (t, r) in enumerate(zip(replayed[name], refs[name])):
                assert _same(t, r), f'replay of {name}: output {i} differs from the eager run of input set {name}'
        assert any(not _same(a, b) for a, b in zip(refs['A'], refs['B'])), 'sets A and B give the same outputs'
    else:
        for i, (t, r) in enumerate(zip(after, refs['C'])):
            assert _same(t, r), f'the eager call after the replays: output {i} differs from the first eager run of C'
    tr.graph, tr.refs = g, refs
    return tr
