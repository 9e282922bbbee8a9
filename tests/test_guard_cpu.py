"""tests/_guard.py on CPU tensors against stand-in "kernels" in plain torch: the proof that the guards bite.  Each faulty
stand-in must be reported with the right tensor, side and offset; a correct one must pass.  (No GPU mutation build exists or
is wanted: the bands are there so that a stray access lands in owned memory.)"""
import pytest
import torch

from tests._guard import (ALIGN, MIN_BAND, POISON, GuardError, band_bytes, check, fill_word, guarded, guarded_out, guarded_repeat,
                          where)

SHAPE = (3, 5, 7, 8)     # frames, rows, cols, channels


def _operands():
    x = torch.arange(3 * 5 * 7 * 8, dtype=torch.float32).reshape(SHAPE)
    return guarded(x, name='x'), guarded_out(SHAPE, torch.float32, 'cpu', name='y')


def _flat_with_bands(t):
    """The whole allocation of a guarded tensor as float32 words, and the payload's first word in it."""
    g = t._guard
    return g.base.view(torch.float32), g.lead // 4


def _double(x, y):                       # the correct stand-in
    y.copy_(x * 2)


def test_band_rule_and_poison_word():
    assert POISON == 0x7FC07FC0 and fill_word(POISON) == POISON
    assert fill_word(float('inf')) == 0x7F800000 and fill_word(float('-inf')) == 0xFF800000 - (1 << 32)
    as_f32 = torch.tensor([POISON], dtype=torch.int32).view(torch.float32)
    assert bool(torch.isnan(as_f32).all()) and bool(torch.isnan(as_f32.view(torch.bfloat16).float()).all())
    assert band_bytes((4, 2, 2, 4), 4) == MIN_BAND                       # a 64-byte frame: the 4 KiB minimum
    assert band_bytes((4, 33, 9, 4), 4) == 4752 // ALIGN * ALIGN + ALIGN  # one frame (4752 bytes) rounded up to 512
    assert band_bytes((4, 32, 32, 64), 4) == 32 * 32 * 64 * 4
    assert band_bytes((7,), 4) == MIN_BAND


def test_layout_of_a_guarded_tensor():
    x, y = _operands()
    g = x._guard
    assert x.shape == SHAPE and x.is_contiguous() and g.lead == MIN_BAND and g.lead % ALIGN == 0
    assert g.base.numel() == g.lead + -(-g.nbytes // ALIGN) * ALIGN + g.lead
    assert torch.equal(x, torch.arange(x.numel(), dtype=torch.float32).reshape(SHAPE))
    assert bool((y.view(torch.int32) == POISON).all())
    words, at = _flat_with_bands(x)
    assert bool((words.view(torch.int32)[:at] == POISON).all()) and bool((words.view(torch.int32)[at + x.numel():] == POISON).all())
    inf = guarded(torch.zeros(2, 3, 3, 4), fill=float('inf'), name='xinf')
    words, at = _flat_with_bands(inf)
    assert bool(torch.isposinf(words[:at]).all()) and bool(torch.isposinf(words[at + inf.numel():]).all())
    check(inf)


def test_a_periodic_operand_equals_the_guarded_repeat():
    """guarded_repeat(small, R) is guarded(small.repeat(R, ...)): same payload, same bands, written in place."""
    small = torch.arange(2 * 3 * 5 * 4, dtype=torch.float32).reshape(2, 3, 5, 4)
    a, b = guarded_repeat(small, 7, name='x'), guarded(small.repeat(7, 1, 1, 1), name='x')
    assert a.shape == b.shape == (14, 3, 5, 4) and torch.equal(a, b) and torch.equal(a._guard.base, b._guard.base)
    check(a)
    inf = guarded_repeat(small, 3, fill=float('inf'))
    words, at = _flat_with_bands(inf)
    assert bool(torch.isposinf(words[:at]).all()) and bool(torch.isposinf(words[at + inf.numel():]).all())
    a._guard.base.view(torch.float32)[a._guard.lead // 4 - 1] = 1.0
    with pytest.raises(GuardError):
        check(a)


def test_a_correct_kernel_passes():
    x, y = _operands()
    _double(x, y)
    check(x, y)
    check(x, None, y)                    # (absent operands are skipped)


def test_an_unwritten_output_is_reported():
    x, y = _operands()
    with pytest.raises(GuardError) as e:
        check(x, y)
    assert (e.value.tensor, e.value.side, e.value.offset) == ('y', 'payload', 0)


def test_a_kernel_that_skips_the_last_row():
    x, y = _operands()
    _double(x, y)
    y[2, 4] = torch.tensor(POISON, dtype=torch.int32).view(torch.float32)      # as if never written
    with pytest.raises(GuardError) as e:
        check(x, y)
    first = ((2 * 5 + 4) * 7) * 8
    assert (e.value.tensor, e.value.side, e.value.offset) == ('y', 'payload', first)
    assert 'frame 2, row 4, col 0, channel 0' in str(e.value) and '56 payload word(s)' in str(e.value)


def test_a_kernel_that_skips_one_interior_element():
    x, y = _operands()
    _double(x, y)
    y.view(torch.int32)[1, 2, 3, 5] = POISON
    with pytest.raises(GuardError) as e:
        check(x, y)
    assert (e.value.tensor, e.value.side, e.value.offset) == ('y', 'payload', ((1 * 5 + 2) * 7 + 3) * 8 + 5)
    assert 'frame 1, row 2, col 3, channel 5' in str(e.value) and '1 payload word(s)' in str(e.value)


def test_a_store_one_element_past_the_end():
    x, y = _operands()
    _double(x, y)
    words, at = _flat_with_bands(y)
    words[at + y.numel()] = 1.0
    with pytest.raises(GuardError) as e:
        check(x, y)
    assert (e.value.tensor, e.value.side, e.value.offset, e.value.byte_offset) == ('y', 'after', y.numel(), y.numel() * 4)
    assert 'frame 3, row 0, col 0, channel 0' in str(e.value) and '0 bytes past its end' in str(e.value)
    assert '0x3f800000' in str(e.value)


def test_a_store_one_element_before_the_start():
    x, y = _operands()
    _double(x, y)
    words, at = _flat_with_bands(y)
    words[at - 1] = 0.0
    with pytest.raises(GuardError) as e:
        check(x, y)
    assert (e.value.tensor, e.value.side, e.value.offset, e.value.byte_offset) == ('y', 'before', -1, -4)
    assert 'frame -1, row 4, col 6, channel 7' in str(e.value) and '4 bytes before its start' in str(e.value)


def test_a_store_into_an_inputs_band():
    x, y = _operands()
    _double(x, y)
    words, at = _flat_with_bands(x)
    words[at + x.numel() + 8 * 7] = 3.0            # one row past the input's last frame
    with pytest.raises(GuardError) as e:
        check(y, x)
    assert (e.value.tensor, e.value.side, e.value.offset) == ('x', 'after', x.numel() + 56)
    assert 'frame 3, row 1, col 0, channel 0' in str(e.value)
    words[at + x.numel() + 8 * 7] = torch.tensor(POISON, dtype=torch.int32).view(torch.float32)
    words[0] = 3.0                                  # the far end of the band before it: a whole band away
    with pytest.raises(GuardError) as e:
        check(y, x)
    assert (e.value.tensor, e.value.side, e.value.offset) == ('x', 'before', -(MIN_BAND // 4))


def test_byte_and_int_tensors():
    """uint8 frames (a payload that does not end on a word) and int32 states."""
    u = guarded(torch.arange(2 * 3 * 5 * 3, dtype=torch.uint8).reshape(2, 3, 5, 3), name='frames')
    check(u)
    g = u._guard
    g.base[g.lead + g.nbytes + 1] = 0              # the second byte behind the payload (inside its last word)
    with pytest.raises(GuardError) as e:
        check(u)
    assert (e.value.tensor, e.value.side, e.value.offset) == ('frames', 'after', u.numel() + 1)
    st = guarded_out((6,), torch.int32, 'cpu', name='states')
    st.copy_(torch.tensor([0, -1, 3, 11, -1, 2], dtype=torch.int32))
    check(st)
    st[4] = POISON
    with pytest.raises(GuardError) as e:
        check(st)
    assert (e.value.tensor, e.value.side, e.value.offset) == ('states', 'payload', 4) and 'element 4' in str(e.value)


def test_where_names_offsets_on_either_side():
    assert where(0, SHAPE) == 'frame 0, row 0, col 0, channel 0'
    assert where(-1, SHAPE) == 'frame -1, row 4, col 6, channel 7'
    assert where(3 * 5 * 7 * 8 + 9, SHAPE) == 'frame 3, row 0, col 1, channel 1'
    assert where(5, (4, 12)) == 'row 0, col 5' and where(13, (4, 12)) == 'row 1, col 1'


def test_check_refuses_a_plain_tensor():
    with pytest.raises(AssertionError):
        check(torch.zeros(3))
