"""The frame helper of the memory-contract tests (tests/abi_frames.py), exercised on CPU tensors: a write one element outside the
payload rectangle is seen in each of the four directions and reported with its position; writes inside the payload are not."""
import pytest
import torch

import abi_frames as F

DTYPES = [torch.float32, torch.bfloat16, torch.int64]


def _frame(dtype, fill="sentinel"):
    payload = torch.arange(5 * 72).reshape(5, 72).to(dtype)
    return F.framed(5, 72, dtype=dtype, payload=payload, fill=fill), payload


@pytest.mark.parametrize("dtype", DTYPES)
def test_geometry_and_payload(dtype):
    f, payload = _frame(dtype)
    assert f.ld == 256 + 8 == F.default_ld(72) and F.default_ld(256) == 264 and F.default_ld(257) == 520
    assert f.guard_before >= 8 and f.guard_after >= 256
    assert f.buf.shape == (f.guard_before + 5 + f.guard_after, f.ld) and f.buf.is_contiguous()
    assert f.ptr == f.buf.data_ptr() + f.guard_before * f.ld * f.buf.element_size() == f.window().data_ptr()
    got = f.payload()
    assert got.is_contiguous() and torch.equal(got, payload)
    f.assert_frame_untouched()
    # every element outside the payload holds the sentinel's bits, which is no NaN
    outside = f.buf[f._outside]
    assert bool((F.bits(outside) == F._BITS[dtype][1]).all())
    if dtype.is_floating_point:
        assert bool(torch.isfinite(outside.float()).all())


def test_flat_frames_are_contiguous_and_still_guarded():
    f = F.framed(300, 1, ld=1, dtype=torch.int64)
    assert f.window().is_contiguous() and f.guard_before >= F.FLAT_GUARD_ELEMS and f.guard_after >= F.FLAT_GUARD_ELEMS
    f.buf[f.guard_before + 300, 0] = 7                       # the element after the last one
    assert f.first_touched() == (300, 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_payload_only_writes_pass(dtype):
    f, _ = _frame(dtype)
    f.window().fill_(3)
    f.window()[4, 71] = 0
    f.window()[0, 0] = 1
    f.assert_frame_untouched()
    assert f.first_touched() is None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where,pos", [("above", (-1, 10)), ("below", (5, 10)), ("right", (2, 72)), ("left", (1, 263))])
def test_a_write_one_element_outside_is_reported_with_its_position(dtype, where, pos):
    """above / below: the rows next to the payload; right: the first gap column; left: one element in front of row 2's first, which
    in memory is the last gap column of row 1"""
    f, _ = _frame(dtype)
    r, c = pos
    f.buf[f.guard_before + r, c] = 0                          # zero: a kernel that 'only' writes zeros there is seen too
    assert f.first_touched() == (r, c)
    with pytest.raises(AssertionError) as e:
        f.assert_frame_untouched("out")
    assert f"row {r}, col {c}" in str(e.value) and "out" in str(e.value)


def test_nan_written_over_the_sentinel_and_sentinel_valued_float_writes():
    f, _ = _frame(torch.float32)
    f.buf[f.guard_before + 5, 0] = float("nan")
    assert f.first_touched() == (5, 0)
    g, _ = _frame(torch.float32)
    g.buf[0, 0] = g.buf[0, 1]                                # the same bits again: nothing changed, nothing to see
    g.assert_frame_untouched()


def test_input_frames_are_nan_outside_the_payload():
    f, payload = _frame(torch.bfloat16, fill="nan")
    assert bool(torch.isnan(f.buf[f._outside].float()).all()) and torch.equal(f.payload(), payload)
    f.assert_frame_untouched()                                # NaN compares equal to itself through the integer view
    f.buf[0, 0] = 1.0
    assert f.first_touched() == (-f.guard_before, 0)
    with pytest.raises(ValueError):
        F.framed(4, 4, dtype=torch.int64, fill="nan")


def test_bad_geometry_is_refused():
    with pytest.raises(ValueError):
        F.framed(4, 72, ld=64)
    with pytest.raises(ValueError):
        F.framed(4, 72, payload=torch.zeros(4, 71))
    with pytest.raises(ValueError):
        F.Frame(4, 72, 264, torch.float32, None, "sentinel", None, 0, 256)


def test_call_refuses_a_number_where_a_pointer_belongs():
    """ctypes would pass an int as a void*: the direct caller checks the kinds against the bound prototype first"""
    import ctypes as C
    protos = [C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_int), C.c_uint64]
    good = (torch.zeros(2), 3, 0.5, (C.c_int * 1)(0), 7)
    F.check_kinds("f", good, protos)
    F.check_kinds("f", (None, 3, 1, None, 7), protos)                  # NULL pointers, an int for a float
    f, _ = _frame(torch.float32)
    F.check_kinds("f", (f,) + good[1:], protos)
    for i, bad in ((0, 64), (1, 0.5), (1, None), (2, None), (3, 5), (4, 1.0)):
        args = list(good)
        args[i] = bad
        with pytest.raises(TypeError):
            F.check_kinds("f", tuple(args), protos)
    with pytest.raises(TypeError):
        F.check_kinds("f", good[:-1], protos)
