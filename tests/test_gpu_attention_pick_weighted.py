"""pmhip_attention_pick_weighted: the weighted cross-attention for the images a `pick` array names, the third
launch beside the two of pmhip_attention_pick.  Operator level, no tolerance anywhere: a served image equals, bit for bit, its rows of
``ops.attention(key_segments=, query_segments=, key_weights=)`` on the same inputs, a skipped image keeps every byte it had, and
three launches -- the length form with want 0, the per-query form with want 1, the weighted form with want 2 -- fill one buffer
with each image's own scalar result.

The frame is that of tests/test_gpu_attention_pick.py (tests/abi_frames.py: guard rows, a gap beside every row, a NaN-payload
sentinel in the window).  The data are those of tests/test_gpu_attention_weights.py (tests/weight_ref.py ``inputs``: its three
layouts, weights from {0, 1/8, 1, 8}, NaN in the K rows and V^T columns of padding keys and of keys with weight 0, image 2's loud
keys at 512).  The weighted launch sees exactly those; the other two launches see the same data with the rows that reach no result
zeroed (they attend to them).  Every launch sees NaN in ALL of Q / K / V^T -- and, the weighted one, in the weights -- of the images
it skips.

Shapes: B = 3, heads = 2, Nq = 80 at 1 / 65 / 416 keys (dim_head 64 in bf16 and fp32, both softmax modes; dim_head 32 and 128 on the
plain path) with every pick pattern of three images over the three kinds; and the two shapes of the picked test that reach the larger
workgroup (the weighted bf16 kernel then runs 128 queries per workgroup: B, heads and Nq decide)."""
import itertools

import numpy as np
import pytest
import torch

import attention_probes as P
import weight_ref as W
from abi_frames import bits, framed
from gpu_common import dev, t
from paintmind_amd import _lib, ops

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
MODES = pytest.mark.parametrize("exp2", [True, False], ids=["exp2", "exp"])
B, H, NQ = 3, 2, 80
NKVS = (1, 65, 416)
PATTERNS = list(itertools.product((0, 1, 2), repeat=3))        # pick[b] of three images over the three kinds
SENTINEL = {BF: 0x7FA5, F32: 0x7FA5C3E1}                      # NaN with a payload no kernel produces, as the integer view's value
_VIEW = {BF: torch.int16, F32: torch.int32}


class Case:
    """one shape's data on the device and the three references, computed once"""

    def __init__(self, nkv, dtype, exp2, dh=64, batch=B, heads=H, nq=NQ):
        self.dtype, self.exp2, self.batch, self.nq, self.nkv, self.width = dtype, exp2, batch, nq, nkv, heads * dh
        d = W.inputs(P.gauss, nkv, dh, batch=batch, heads=heads, nq=nq)
        assert nkv == 1 or (np.isnan(d["k"]).any() and (d["w"] == 0).any())
        pad = -(-nkv // 64) * 64
        kp, vtp = P.pad_kv(d["k"], d["v"], pad)                  # what the weighted launch sees: NaN where w == 0 or the key is padding
        kzp, vtzp = P.pad_kv(d["kz"], d["vz"], pad)              # what the other two see: those rows zeroed
        self.q = t(d["q"], dtype)
        self.nan_kv, self.zero_kv = (t(kp, dtype), t(vtp, dtype)), (t(kzp, dtype), t(vtzp, dtype))
        self.lens = t(np.array([max(1, nkv - 7 * (b % 5)) for b in range(batch)], np.int32))
        self.ks, self.qm, self.w = t(d["ks"]), t(d["qm"].view(np.int32)), t(d["w"].astype(np.float32))
        a0 = (self.q, *self.zero_kv, nkv)
        self.ref = [ops.attention(*a0, use_exp2=exp2, kv_lens=self.lens).view(batch, nq, -1),
                    ops.attention(*a0, use_exp2=exp2, key_segments=self.ks, query_segments=self.qm).view(batch, nq, -1),
                    ops.attention(self.q, *self.nan_kv, nkv, use_exp2=exp2, key_segments=self.ks, query_segments=self.qm,
                                  key_weights=self.w).view(batch, nq, -1)]
        assert all(torch.isfinite(r).all() for r in self.ref)

    def poisoned(self, kv, skipped):
        """(q, k, vt, w) with NaN in every element of the images in `skipped` (a bool [B] tensor)"""
        nan = lambda x: torch.where(skipped.view(-1, *[1] * (x.dim() - 1)), torch.full_like(x, float("nan")), x)
        return nan(self.q), nan(kv[0]), nan(kv[1]), nan(self.w)

    def frame(self):
        f = framed(self.batch * self.nq, self.width, dtype=self.dtype, device=dev())
        f.window().view(_VIEW[self.dtype]).fill_(SENTINEL[self.dtype])
        return f

    def rows(self, f):
        return bits(f.window()).view(self.batch, self.nq, -1)

    def launch(self, kind, pick, f):
        """the launch of one kind into the frame, NaN in the images it skips"""
        skipped = pick != kind
        q, k, vt, w = self.poisoned(self.nan_kv if kind == 2 else self.zero_kv, skipped)
        kw = dict(kv_lens=self.lens) if kind == 0 else dict(key_segments=self.ks, query_segments=self.qm)
        if kind == 2:
            kw["key_weights"] = w
        out = ops.attention_pick(q, k, vt, self.nkv, pick, kind, f.window(), use_exp2=self.exp2, **kw)
        assert out.data_ptr() == f.ptr

    def run(self, pattern):
        """the weighted launch alone into a sentinel window, then the three launches into one window"""
        pick = torch.tensor([pattern[b % 3] for b in range(self.batch)], dtype=torch.uint8, device=dev())
        f = self.frame()
        sent = torch.full_like(self.rows(f), SENTINEL[self.dtype])
        counted = ops.attention_fallbacks()
        self.launch(2, pick, f)
        assert ops.attention_fallbacks() == counted, f"pick {pattern}: the weighted form counted a fallback"
        want = torch.where((pick == 2).view(-1, 1, 1), bits(self.ref[2]), sent)
        assert torch.equal(self.rows(f), want), f"pick {pattern}: the weighted form alone (want 2)"
        f.assert_frame_untouched(f"pick {pattern}, weighted form alone")
        f = self.frame()
        for kind in (0, 1, 2):
            self.launch(kind, pick, f)
            want = torch.where((pick == kind).view(-1, 1, 1), bits(self.ref[kind]), want if kind else sent)
            assert torch.equal(self.rows(f), want), f"pick {pattern}: launch of kind {kind} into the shared buffer"
            f.assert_frame_untouched(f"pick {pattern}, launch of kind {kind}")
        mine = torch.stack([self.ref[pattern[b % 3]][b] for b in range(self.batch)])
        assert torch.equal(self.rows(f), bits(mine)), f"pick {pattern}: every image its own scalar result"


@DTYPES
@MODES
def test_tuned_kernels_every_pick_pattern(dtype, exp2):
    """dim_head 64: attention_seg_bias_pick_kernel (f32) and attention_bf16_seg_bias_pick_kernel at 64 queries per workgroup"""
    for nkv in NKVS:
        case = Case(nkv, dtype, exp2)
        if nkv >= 3:                                                      # the three forms differ: a launch of the wrong kind is seen
            assert not torch.equal(case.ref[2], case.ref[1]) and not torch.equal(case.ref[1], case.ref[0])
        for pattern in PATTERNS:
            case.run(pattern)


@pytest.mark.parametrize("dh", [32, 128])
@DTYPES
@MODES
def test_plain_path_every_pick_pattern(dh, dtype, exp2):
    """attention_dh_seg_bias_pick_kernel"""
    for nkv in NKVS:
        case = Case(nkv, dtype, exp2, dh=dh)
        for pattern in PATTERNS:
            case.run(pattern)


@pytest.mark.parametrize("batch,heads,nq", [(16, 16, 130), (32, 16, 80)], ids=["two-blocks", "one-ragged-block"])
def test_the_128_query_form_of_the_bf16_kernel(batch, heads, nq):
    """B * heads * ceil(Nq / 128) >= 512: the weighted launcher's rule picks 128 queries per workgroup, as for its twin; the module's
    base shape runs 64"""
    qf = lambda b, h, n_: 2 if b * h * -(-n_ // 128) >= 512 else 1
    assert qf(batch, heads, nq) == 2 and qf(B, H, NQ) == 1
    case = Case(65, BF, True, batch=batch, heads=heads, nq=nq)
    for pattern in ((0, 1, 2), (2, 0, 1), (2, 2, 2), (0, 0, 0), (1, 2, 1)):
        case.run(pattern)


def test_these_launches_never_count_a_fallback_and_a_skipped_image_is_read_nowhere():
    """image 2's loud keys (K rows of 512 under positive queries, no query allowing them) would push a fast path out of range; the
    weighted form has none, served or skipped.  A launch that serves no image leaves every byte of the buffer"""
    case = Case(416, BF, True)
    ops.attention_fallbacks(reset=True)
    f = case.frame()
    before = bits(f.buf).clone()
    for want, pick in ((2, (0, 1, 0)), (5, (2, 2, 2))):
        p = torch.tensor(pick, dtype=torch.uint8, device=dev())
        q, k, vt, w = case.poisoned(case.nan_kv, torch.ones(B, dtype=torch.bool, device=dev()))
        ops.attention_pick(q, k, vt, 416, p, want, f.window(), use_exp2=True, key_segments=case.ks, query_segments=case.qm, key_weights=w)
    torch.cuda.synchronize()
    assert torch.equal(bits(f.buf), before)
    ops.attention_pick(case.q, *case.nan_kv, 416, torch.full((B,), 2, dtype=torch.uint8, device=dev()), 2, f.window(), use_exp2=True,
                       key_segments=case.ks, query_segments=case.qm, key_weights=case.w)
    assert torch.equal(case.rows(f), bits(case.ref[2]))
    assert ops.attention_fallbacks(reset=True) == 0


def test_key_weights_alone_build_the_neutral_arrays():
    """ops.attention_pick(key_weights=) without segment arrays is ops.attention(key_weights=) without them"""
    case = Case(65, F32, False)
    w = torch.where(case.ks == W.PAD, torch.zeros_like(case.w), case.w)
    w[:, 0] = 1
    want = ops.attention(case.q, *case.nan_kv, 65, key_weights=w)
    out = torch.zeros_like(want)
    ops.attention_pick(case.q, *case.nan_kv, 65, torch.full((B,), 2, dtype=torch.uint8, device=dev()), 2, out, key_weights=w)
    assert torch.equal(bits(out), bits(want)) and torch.isfinite(out).all()


def test_the_arguments_are_checked():
    case = Case(65, F32, False)
    out = torch.empty(B * NQ, H * 64, device=dev())
    pick = torch.zeros(B, dtype=torch.uint8, device=dev())
    a = (case.q, *case.zero_kv, 65)
    seg = dict(key_segments=case.ks, query_segments=case.qm)
    with pytest.raises(ValueError, match="exclude"):
        ops.attention_pick(*a, pick, 2, out, kv_lens=case.lens, key_weights=case.w)
    with pytest.raises(ValueError, match="come together"):
        ops.attention_pick(*a, pick, 2, out, key_segments=case.ks, key_weights=case.w)
    with pytest.raises(ValueError, match="key_weights"):
        ops.attention_pick(*a, pick, 2, out, key_weights=case.w[:, :64].contiguous(), **seg)
    with pytest.raises(ValueError, match="key_weights"):
        ops.attention_pick(*a, pick, 2, out, key_weights=case.w.double(), **seg)
    with pytest.raises(_lib.PmhipError, match="want=256"):
        ops.attention_pick(*a, pick, 256, out, key_weights=case.w, **seg)
    lib, p = _lib.load(), ops._p
    bias = ops.key_bias(case.w, False)
    full = dict(ks=p(case.ks), qm=p(case.qm), bias=p(bias), pick=p(pick))
    call = lambda ldo=H * 64, **kw: lib.pmhip_attention_pick_weighted(_lib.F32, p(case.q), p(case.zero_kv[0]), p(case.zero_kv[1]), p(out), ldo, B,
                                                                      H, 64, NQ, 65, 128, 0, kw["ks"], kw["qm"], kw["bias"], kw["pick"], 2, None)
    assert call(**full) == _lib.PMHIP_OK
    for name, text in (("pick", b"pick is NULL"), ("ks", b"key_bias is NULL"), ("qm", b"key_bias is NULL"), ("bias", b"key_bias is NULL")):
        assert call(**dict(full, **{name: None})) == _lib.PMHIP_EINVAL and text in lib.pmhip_last_error(), name
    # the family's own checks follow under the entry's name: an output row stride below heads * dim_head
    assert call(ldo=64, **full) == _lib.PMHIP_EINVAL and b"attention_pick_weighted: ldo=64" in lib.pmhip_last_error()
