"""Every prototype of include/tsm_hip.h that takes ``void *stream``, classified (tests/test_stream_cases_cpu.py holds the
table to the header, tests/test_stream_capture_gpu.py holds the ``capture`` entries to their promise).

* ``('capture', <test function>)``: the entry point only enqueues on ``stream``; the named test of
  tests/test_stream_capture_gpu.py captures it on a side stream and replays it (tests/_capture.py).
* ``('not_capture_safe', <reason>)``: the header itself says why the call is not enqueue-only.

A new entry point with a stream argument fails the CPU test until it has a line here: nobody adds one without deciding what
it owes its stream.
"""
import re

CAPTURE, NOT_CAPTURE_SAFE = 'capture', 'not_capture_safe'

STREAM_CASES = {
    'tsm_forward': (CAPTURE, 'test_f32_engine_tuned_in_the_process'),
    'tsm_forward_features': (CAPTURE, 'test_forward_features'),
    'tsm_tune': (NOT_CAPTURE_SAFE, 'synchronous: a few hundred ms of timed launches, or one forward to load the code objects'),
    'tsm_forward_tap': (NOT_CAPTURE_SAFE, 'copies the activation out and synchronises before returning (parity tests)'),
    'tsm_temporal_shift': (CAPTURE, 'test_op_temporal_shift'),
    'tsm_conv_bn_act': (NOT_CAPTURE_SAFE, 'packs the weights on every call: a test/debug entry point, not the fast path'),
    'tsm_conv_op': (NOT_CAPTURE_SAFE, 'packs the weights and allocates on every call, the split forms\' segment scratch too'),
    'tsm_maxpool3x3s2': (CAPTURE, 'test_op_maxpool3x3s2'),
    'tsm_preprocess': (CAPTURE, 'test_op_preprocess'),
    'tsm_gather_clips': (CAPTURE, 'test_op_gather_clips'),
    'tsm_preprocess_clips': (CAPTURE, 'test_op_preprocess_clips'),
    'tsm_preprocess_indexed': (CAPTURE, 'test_op_preprocess_indexed'),
    'tsm_preprocess_windows': (CAPTURE, 'test_op_preprocess_windows'),
    'tsm_preprocess_image': (CAPTURE, 'test_op_preprocess_image'),
    'tsm_head': (CAPTURE, 'test_op_head'),
    'tsm_head_segments': (CAPTURE, 'test_op_head_segments'),
    'tsm_pool_features': (CAPTURE, 'test_op_pool_features'),
    'tsm_cosine_distances': (CAPTURE, 'test_op_cosine_distances'),
    'tsm_maxpool2x2': (CAPTURE, 'test_op_maxpool2x2'),
    'tsm_nonlocal_attention': (CAPTURE, 'test_op_nonlocal_attention'),
    'tsm_scores_to_states': (CAPTURE, 'test_op_scores_to_states'),
    'tsm_frame_votes': (CAPTURE, 'test_op_frame_votes_carries_its_history_across_replays'),
    'tsm_top1_tally': (CAPTURE, 'test_op_top1_tally_accumulates_across_replays'),
}

_COMMENT = re.compile(r'/\*.*?\*/', re.S)
_PROTOTYPE = re.compile(r'\b(\w+)\s*\(([^;{}()]*)\)\s*;')
_STREAM_ARG = re.compile(r'\bvoid\s*\*\s*stream\b')


def stream_prototypes(header_text):
    """Names of the functions declared in ``header_text`` that take ``void *stream``, in declaration order."""
    text = _COMMENT.sub(' ', header_text)
    text = '\n'.join(ln for ln in text.splitlines() if not ln.lstrip().startswith('#'))
    return [m.group(1) for m in _PROTOTYPE.finditer(text) if _STREAM_ARG.search(m.group(2))]


def check_table(header_text, table=None):
    """Problems of ``table`` against the header, as a list of strings (empty: every stream prototype is classified and
    every entry names a declared function and a known class)."""
    table = STREAM_CASES if table is None else table
    declared = stream_prototypes(header_text)
    problems = [f'{name}: takes a stream and is not classified in tests/_stream_cases.py' for name in declared if name not in table]
    problems += [f'{name}: classified, but the header declares no such function with a stream' for name in table
                 if name not in declared]
    for name, entry in table.items():
        if (not isinstance(entry, tuple) or len(entry) != 2 or entry[0] not in (CAPTURE, NOT_CAPTURE_SAFE)
                or not isinstance(entry[1], str) or not entry[1]):
            problems.append(f'{name}: an entry is (\'capture\', <test function>) or (\'not_capture_safe\', <reason>), got {entry!r}')
    return problems
