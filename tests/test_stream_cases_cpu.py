"""include/tsm_hip.h against tests/_stream_cases.py: every entry point that takes a stream is either captured and replayed by
a GPU test or listed with the header's own reason why it is not enqueue-only."""
import ast
import os

from tests._stream_cases import CAPTURE, NOT_CAPTURE_SAFE, STREAM_CASES, check_table, stream_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, 'include', 'tsm_hip.h')) as f:
        return f.read()


def test_every_stream_prototype_of_the_header_is_classified():
    declared = stream_prototypes(_header())
    assert len(declared) >= 23 and len(set(declared)) == len(declared), declared
    for name in ('tsm_forward', 'tsm_forward_tap', 'tsm_conv_op', 'tsm_preprocess_windows', 'tsm_nonlocal_attention', 'tsm_top1_tally'):
        assert name in declared, (name, declared)         # (the parser sees multi-line prototypes and array parameters)
    assert 'tsm_last_forward_ms' not in declared and 'tsm_set_tensor' not in declared
    assert check_table(_header()) == []


def test_the_second_class_is_what_the_header_excludes():
    assert sorted(k for k, v in STREAM_CASES.items() if v[0] == NOT_CAPTURE_SAFE) == ['tsm_conv_bn_act', 'tsm_conv_op', 'tsm_forward_tap',
                                                                                    'tsm_tune']


def test_every_capture_entry_names_a_gpu_test_that_exists():
    with open(os.path.join(ROOT, 'tests', 'test_stream_capture_gpu.py')) as f:
        tree = ast.parse(f.read())
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith('test_')}
    missing = {k: v[1] for k, v in STREAM_CASES.items() if v[0] == CAPTURE and v[1] not in tests}
    assert not missing, f'no such test in tests/test_stream_capture_gpu.py: {missing}'


STAND_IN = '''
/* int tsm_commented_out(const float *x, void *stream); */
int tsm_known(const float *x, int32_t n, void *stream);
int tsm_new_entry_point(const float *x, float *y,
                        int64_t shape[4], void * stream);
float tsm_no_stream(tsm_engine *e);
#define TSM_MACRO(x, stream) ((x) + 1);
'''


def test_the_parser_rejects_an_unclassified_prototype_and_a_stale_entry():
    assert stream_prototypes(STAND_IN) == ['tsm_known', 'tsm_new_entry_point']
    table = {'tsm_known': (CAPTURE, 'test_x')}
    problems = check_table(STAND_IN, table)
    assert len(problems) == 1 and problems[0].startswith('tsm_new_entry_point: takes a stream and is not classified'), problems
    table['tsm_new_entry_point'] = (NOT_CAPTURE_SAFE, 'synchronous')
    assert check_table(STAND_IN, table) == []
    table['tsm_gone'] = (CAPTURE, 'test_y')
    problems = check_table(STAND_IN, table)
    assert len(problems) == 1 and problems[0].startswith('tsm_gone: classified, but the header declares no such function'), problems
    del table['tsm_gone']
    table['tsm_known'] = ('maybe', 'test_x')
    assert len(check_table(STAND_IN, table)) == 1
    table['tsm_known'] = (CAPTURE, '')
    assert len(check_table(STAND_IN, table)) == 1
