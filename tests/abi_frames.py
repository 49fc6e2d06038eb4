"""Framed buffers for the C ABI's memory contract (include/pmhip.h: leading dimensions, in place, exact output extents).

A frame is ONE allocation of [guard_before + rows + guard_after, ld] elements with the payload rectangle [rows, cols] inside it:

    +---------------------------- ld ----------------------------+
    |  guard_before rows                                         |
    |  payload [rows, cols]            | gap: ld - cols columns  |
    |  guard_after rows                                          |
    +------------------------------------------------------------+

Inputs are filled with NaN (an out-of-bounds read that is used poisons the result), outputs with a fixed non-NaN bit pattern that
is compared through an integer view (a stray store of any value, zero or NaN included, is seen).  guard_after is a whole tile of
the largest kernel (256 rows) and ld = cols rounded up to 256, plus 8: a ragged-tile store that forgets its row or column guard
lands inside the allocation and is reported with its position.  Nothing here relies on, or aims at, a fault.

`call` reaches an entry point of libpaintmind_hip.so directly, with explicit pointers and leading dimensions (paintmind_amd.ops
only passes contiguous tensors).  Works on CPU tensors too (tests/test_abi_frames_cpu.py); not a conftest, not collected.
"""
import ctypes as C

import torch

GUARD_BEFORE = 8
GUARD_AFTER = 256            # one full tile of the largest kernel (gemm256.hip: 256 x 256)
FLAT_GUARD_ELEMS = 4096      # frames of narrow contiguous arrays ([M], [M][2]) get at least this many guard elements on each side

# dtype -> (integer view, sentinel bit pattern: 0x5A... is a finite float in every format and an unlikely integer)
_BITS = {
    torch.float32: (torch.int32, 0x5A5A5A5A),
    torch.bfloat16: (torch.int16, 0x5A5A),
    torch.int64: (torch.int64, 0x5A5A5A5A5A5A5A5A),
    torch.int32: (torch.int32, 0x5A5A5A5A),
    torch.uint8: (torch.uint8, 0x5A),
}


def default_ld(cols):
    """the payload width rounded up to 256, plus 8: keeps the 8- and 4-element alignment rules, never equals the width"""
    return (cols + 255) // 256 * 256 + 8


def bits(t):
    """the tensor's elements as integers of the same width (bit-for-bit comparisons; NaN == NaN, -0.0 != 0.0)"""
    return t.contiguous().view(_BITS[t.dtype][0])


class Frame:
    def __init__(self, rows, cols, ld, dtype, payload, fill, device, guard_before, guard_after):
        if ld < cols:
            raise ValueError(f"ld={ld} is smaller than the payload width {cols}")
        if guard_before < GUARD_BEFORE or guard_after < GUARD_AFTER:
            raise ValueError(f"guards must be at least {GUARD_BEFORE} rows before and {GUARD_AFTER} rows after the payload")
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        self.guard_before, self.guard_after = guard_before, guard_after
        self.buf = torch.empty(guard_before + rows + guard_after, ld, dtype=dtype, device=device)
        view, sentinel = _BITS[dtype]
        if fill == "nan":
            if not dtype.is_floating_point:
                raise ValueError("only floating-point frames can be filled with NaN")
            self.buf.fill_(float("nan"))
        elif fill == "sentinel":
            self.buf.view(view).fill_(sentinel)
        else:
            raise ValueError(f"fill must be 'nan' or 'sentinel', not {fill!r}")
        if payload is not None:
            if tuple(payload.shape) != (rows, cols) or payload.dtype != dtype:
                raise ValueError(f"payload must be a {dtype} [{rows}, {cols}] tensor, got {payload.dtype} {tuple(payload.shape)}")
            self.window().copy_(payload)
        # what every element outside the payload must still be afterwards
        self._expected = bits(self.buf).clone()
        self._outside = torch.ones(self.buf.shape, dtype=torch.bool, device=self.buf.device)
        self._outside[guard_before:guard_before + rows, :cols] = False

    def window(self):
        """the payload rectangle as a (strided) view of the allocation"""
        return self.buf[self.guard_before:self.guard_before + self.rows, :self.cols]

    def payload(self):
        """a contiguous copy of the payload"""
        return self.window().contiguous()

    @property
    def ptr(self):
        """device pointer of the payload's first element"""
        return self.buf.data_ptr() + self.guard_before * self.ld * self.buf.element_size()

    def first_touched(self):
        """(row, col) of the first element outside the payload rectangle that changed, relative to the payload's origin (rows < 0:
        the guard in front; cols >= self.cols: the gap), in memory order; None if the frame is intact"""
        bad = (bits(self.buf) != self._expected) & self._outside
        if not bool(bad.any()):
            return None
        flat = int(torch.nonzero(bad.reshape(-1))[0])
        return flat // self.ld - self.guard_before, flat % self.ld

    def assert_frame_untouched(self, what="frame"):
        hit = self.first_touched()
        if hit is not None:
            r, c = hit
            got = int(bits(self.buf)[r + self.guard_before, c]) & ((1 << (8 * self.buf.element_size())) - 1)
            raise AssertionError(f"{what}: element (row {r}, col {c}) outside the payload [{self.rows}, {self.cols}] (ld {self.ld}, "
                                 f"{self.dtype}) was written: bits 0x{got:x}")


def framed(rows, cols, ld=None, dtype=torch.float32, payload=None, fill="sentinel", device=None,
           guard_before=GUARD_BEFORE, guard_after=GUARD_AFTER):
    """One allocation [guard_before + rows + guard_after, ld], filled with `fill` ('nan' for inputs, 'sentinel' for outputs), the
    payload (a [rows, cols] tensor, or None) written into [guard_before : guard_before + rows, :cols].  ld None: default_ld(cols).
    ld == cols gives a contiguous payload with guard rows only (arrays the ABI has no leading dimension for); the guards then
    hold at least FLAT_GUARD_ELEMS elements."""
    ld = default_ld(cols) if ld is None else ld
    if payload is not None and device is None:
        device = payload.device
    extra = (FLAT_GUARD_ELEMS + ld - 1) // ld
    return Frame(rows, cols, ld, dtype, payload, fill, device, max(guard_before, extra), max(guard_after, extra))


def _arg(a):
    if isinstance(a, Frame):
        return C.c_void_p(a.ptr)
    if isinstance(a, torch.Tensor):
        return C.c_void_p(a.data_ptr())
    return a


def call(name, *args):
    """lib.<name>(*args, current stream): Frames and tensors become their device pointers, everything else goes through as it is
    (None = NULL).  Raises PmhipError on a non-zero return, like paintmind_amd.ops."""
    from paintmind_amd import _lib
    lib = _lib.load()
    check_kinds(name, args, _lib.PROTOTYPES[name][1][:-1])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(getattr(lib, name)(*[_arg(a) for a in args], stream), name)


def check_kinds(name, args, argtypes):
    """ctypes takes a plain integer for a void*: a count slipped into a pointer's place would be launched as an address.  Pointers
    must come as Frames, tensors, ctypes objects or None; numbers as numbers."""
    if len(args) != len(argtypes):
        raise TypeError(f"{name}: {len(args)} arguments for {len(argtypes)} parameters (the stream is appended by call)")
    for i, (a, ty) in enumerate(zip(args, argtypes)):
        number = isinstance(a, (int, float)) and not isinstance(a, bool)
        if ty in (C.c_int, C.c_int64, C.c_uint64, C.c_uint32, C.c_size_t):
            ok = isinstance(a, int) and not isinstance(a, bool)
        elif ty is C.c_float:
            ok = number
        else:
            ok = not number and not isinstance(a, bool)
        if not ok:
            raise TypeError(f"{name}: argument {i} is {a!r}, the prototype wants {ty.__name__}")
