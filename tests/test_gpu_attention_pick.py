"""pmhip_attention_pick: the per-image-length form and the per-query form of the cross-attention, each for the
images a `pick` array names, two launches filling one buffer.  Operator level, no tolerance anywhere: a served image equals, bit for
bit, its rows of the existing entry (``ops.attention(kv_lens=)`` / ``ops.attention(key_segments=, query_segments=)``) on the same
inputs, a skipped image keeps every byte it had.

The output is a framed window (tests/abi_frames.py: guard rows around it, a gap beside every row) pre-filled with a NaN-payload
sentinel, so a store of any value -- zero and a canonical NaN included -- into a skipped image's rows or outside the rows is seen.
Padding keys hold NaN in K and V^T, and every launch sees NaN in ALL of Q / K / V^T of the images it skips: neither reaches an
output.  The segments are the layouts of tests/region_ref.py (``layout``: global | region 1 | region 2, 255 behind an image's total);
an image's per-image length is that total, so one data set serves both forms.

Shapes: B = 3, heads = 2, Nq = 80 at 1 / 65 / 416 keys (dim_head 64 in bf16 and fp32, both softmax modes; dim_head 32 and 128 on the
plain path) with every pick pattern of three images, none and all included; and one shape per workgroup form the bf16 dispatcher can
choose (attention_bf16.hip: 256 / 128 / 64 queries for the length form, 128 / 64 for the per-query form; B, heads and Nq decide)."""
import itertools

import numpy as np
import pytest
import torch

import attention_probes as P
import region_ref as R
from abi_frames import bits, framed
from gpu_common import dev, t
from paintmind_amd import _lib, ops

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
MODES = pytest.mark.parametrize("exp2", [True, False], ids=["exp2", "exp"])
B, H, NQ = 3, 2, 80
NKVS = (1, 65, 416)
PATTERNS = list(itertools.product((0, 1), repeat=3))           # pick[b] of three images: none regional ... all regional
SENTINEL = {BF: 0x7FA5, F32: 0x7FA5C3E1}                      # NaN with a payload no kernel produces, as the integer view's value


def layouts(nkv, nq):
    """region_ref.layout on a g x g grid with g * g >= nq (its first nq tokens are the queries): image 0 = global | two overlapping
    regions filling all nkv keys, image 1 = global | one region over about half of them, image 2 = one global row.  With fewer
    than three keys there are no regions.  -> (key_seg uint8 [3, nkv], query_mask uint32 [3, nq], totals int32 [3])"""
    g = int(np.ceil(np.sqrt(nq)))
    left, mid = np.zeros((g, g), bool), np.zeros((g, g), bool)
    left[:, :g // 2 + 1] = True
    mid[g // 3:, g // 3:2 * g // 3 + 1] = True
    rows = lambda count: torch.zeros(count, 1)
    if nkv >= 3:
        a, b_ = nkv // 2, nkv // 3
        glob = [rows(a), rows((nkv + 1) // 2 - (nkv + 1) // 4), rows(1)]
        regions = [[(rows(b_), left), (rows(nkv - a - b_), mid)], [(rows((nkv + 1) // 4), mid)], []]
    else:
        glob, regions = [rows(nkv), rows(1), rows(1)], [[], [], []]
    _, ks, qm = R.layout(glob, regions, g, 1)
    assert ks.shape == (3, nkv) and R.allowed(ks, qm).any(-1).all()
    totals = (ks != R.PAD).sum(1).astype(np.int32)
    assert totals[0] == nkv and (ks[np.arange(nkv)[None] >= totals[:, None]] == R.PAD).all()
    return ks, np.ascontiguousarray(qm[:, :nq]), totals


class Case:
    """one shape's data on the device (clean, and per launch with NaN in the skipped images) and the two references, computed once"""

    def __init__(self, nkv, dtype, exp2, dh=64, batch=B, heads=H, nq=NQ):
        self.dtype, self.exp2, self.batch, self.nq, self.nkv, self.width = dtype, exp2, batch, nq, nkv, heads * dh
        d = P.gauss((batch, heads), nq, nkv, 4.0, dh)
        ks3, qm3, tot3 = layouts(nkv, nq)
        img = np.arange(batch) % 3
        ks, qm, self.totals = ks3[img], qm3[img], tot3[img]
        k, v = d["k"].copy(), d["v"].copy()
        for b in range(batch):                                   # padding keys: NaN, also inside [0, Nkv)
            k[b][:, self.totals[b]:] = np.nan
            v[b][:, self.totals[b]:] = np.nan
        kp, vtp = P.pad_kv(k, v, -(-nkv // 64) * 64)
        self.q, self.k, self.vt = t(d["q"], dtype), t(kp, dtype), t(vtp, dtype)
        self.lens, self.ks, self.qm = t(self.totals), t(ks), t(qm.view(np.int32))
        self.ref_lens = ops.attention(self.q, self.k, self.vt, nkv, use_exp2=exp2, kv_lens=self.lens).view(batch, nq, -1)
        self.ref_seg = ops.attention(self.q, self.k, self.vt, nkv, use_exp2=exp2, key_segments=self.ks,
                                     query_segments=self.qm).view(batch, nq, -1)
        assert torch.isfinite(self.ref_lens).all() and torch.isfinite(self.ref_seg).all()

    def poisoned(self, skipped):
        """(q, k, vt) with NaN in every row of the images in `skipped` (a bool [B] tensor)"""
        if not bool(skipped.any()):
            return self.q, self.k, self.vt
        return tuple(torch.where(skipped.view(-1, 1, 1, 1), torch.full_like(x, float("nan")), x) for x in (self.q, self.k, self.vt))

    def frame(self):
        f = framed(self.batch * self.nq, self.width, dtype=self.dtype, device=dev())
        f.window().view(_VIEW[self.dtype]).fill_(SENTINEL[self.dtype])
        return f

    def rows(self, f):
        return bits(f.window()).view(self.batch, self.nq, -1)

    def run(self, pattern):
        """both launches for one pick pattern (image b's kind = pattern[b % 3]); every claim of the module docstring"""
        pick = torch.tensor([pattern[b % 3] for b in range(self.batch)], dtype=torch.uint8, device=dev())
        regional = pick.bool()
        f = self.frame()
        sent = torch.full_like(self.rows(f), SENTINEL[self.dtype])
        q, k, vt = self.poisoned(regional)
        out = ops.attention_pick(q, k, vt, self.nkv, pick, 0, f.window(), use_exp2=self.exp2, kv_lens=self.lens)
        assert out.data_ptr() == f.ptr
        want = torch.where(regional.view(-1, 1, 1), sent, bits(self.ref_lens))
        assert torch.equal(self.rows(f), want), f"pick {pattern}: the length form (want 0)"
        f.assert_frame_untouched(f"pick {pattern}, length form")
        q, k, vt = self.poisoned(~regional)
        ops.attention_pick(q, k, vt, self.nkv, pick, 1, f.window(), use_exp2=self.exp2, key_segments=self.ks, query_segments=self.qm)
        want = torch.where(regional.view(-1, 1, 1), bits(self.ref_seg), bits(self.ref_lens))
        assert torch.equal(self.rows(f), want), f"pick {pattern}: the per-query form (want 1) behind the length form"
        f.assert_frame_untouched(f"pick {pattern}, per-query form")


_VIEW = {BF: torch.int16, F32: torch.int32}


@DTYPES
@MODES
def test_tuned_kernels_every_pick_pattern(dtype, exp2):
    """dim_head 64: attention_lens_pick_kernel / attention_seg_pick_kernel (f32) and the bf16 pair at 64 queries per workgroup"""
    for nkv in NKVS:
        case = Case(nkv, dtype, exp2)
        if nkv >= 3:
            assert not torch.equal(case.ref_lens, case.ref_seg)          # the two forms differ: a launch of the wrong kind is seen
        for pattern in PATTERNS:
            case.run(pattern)


@pytest.mark.parametrize("dh", [32, 128])
@DTYPES
@MODES
def test_plain_path_every_pick_pattern(dh, dtype, exp2):
    """attention_dh_lens_pick_kernel / attention_dh_seg_pick_kernel"""
    for nkv in NKVS:
        case = Case(nkv, dtype, exp2, dh=dh)
        for pattern in PATTERNS:
            case.run(pattern)


def _qf(batch, heads, nq, seg):
    """the bf16 launchers' rule (attention_bf16.hip): the largest workgroup that still gives 512 of them; no 256-query per-query form"""
    bh = batch * heads
    if not seg and bh * -(-nq // 256) >= 512:
        return 4
    return 2 if bh * -(-nq // 128) >= 512 else 1


@pytest.mark.parametrize("batch,heads,nq,forms", [(16, 16, 130, (2, 2)), (32, 16, 80, (4, 2))], ids=["128-128", "256-128"])
def test_every_workgroup_form_of_the_bf16_kernels(batch, heads, nq, forms):
    """the smallest B / heads / Nq that reach 128 queries per workgroup in both forms (B * heads = 256, two 128-query blocks, the
    second ragged), and 256 in the length form (B * heads = 512; the per-query form then runs 128).  64 / 64 is the module's base shape."""
    assert (_qf(batch, heads, nq, False), _qf(batch, heads, nq, True)) == forms and (_qf(B, H, NQ, False), _qf(B, H, NQ, True)) == (1, 1)
    case = Case(65, BF, True, batch=batch, heads=heads, nq=nq)
    for pattern in ((0, 1, 0), (1, 0, 1), (0, 0, 0), (1, 1, 1)):
        case.run(pattern)


def test_a_launch_that_skips_every_image_counts_no_fallback_and_reads_nothing():
    """NaN everywhere, 1e4-sized scores in the clean copy: a served workgroup of the length form would leave the fast path; a skipped
    one never gets that far"""
    case = Case(416, BF, True)
    loud = case.k.clone()
    loud[:, :, 200:204] = 512.0
    ops.attention(case.q.abs(), loud, case.vt, 416, use_exp2=True, kv_lens=case.lens)
    assert ops.attention_fallbacks(reset=True) > 0                       # the data does what the docstring says
    f = case.frame()
    before = bits(f.buf).clone()
    pick = torch.ones(B, dtype=torch.uint8, device=dev())
    nan = lambda x: torch.full_like(x, float("nan"))
    ops.attention_pick(nan(case.q), nan(loud), nan(case.vt), 416, pick, 0, f.window(), use_exp2=True, kv_lens=case.lens)
    ops.attention_pick(nan(case.q), nan(loud), nan(case.vt), 416, pick, 3, f.window(), use_exp2=True, key_segments=case.ks,
                       query_segments=case.qm)
    torch.cuda.synchronize()
    assert ops.attention_fallbacks() == 0
    assert torch.equal(bits(f.buf), before)
    # served, the same launch counts as pmhip_attention_lens does
    ops.attention_pick(case.q.abs(), loud, case.vt, 416, pick, 1, f.window(), use_exp2=True, kv_lens=case.lens)
    assert ops.attention_fallbacks(reset=True) > 0


def test_the_arguments_are_checked():
    case = Case(65, F32, False)
    out = torch.empty(B * NQ, H * 64, device=dev())
    pick = torch.zeros(B, dtype=torch.uint8, device=dev())
    a = (case.q, case.k, case.vt, 65)
    with pytest.raises(ValueError, match="exactly one"):
        ops.attention_pick(*a, pick, 0, out)
    with pytest.raises(ValueError, match="exactly one"):
        ops.attention_pick(*a, pick, 0, out, kv_lens=case.lens, key_segments=case.ks, query_segments=case.qm)
    with pytest.raises(ValueError, match="come together"):
        ops.attention_pick(*a, pick, 0, out, key_segments=case.ks)
    with pytest.raises(ValueError, match="pick must be"):
        ops.attention_pick(*a, pick.int(), 0, out, kv_lens=case.lens)
    with pytest.raises(ValueError, match="pick must be"):
        ops.attention_pick(*a, pick[:2], 0, out, kv_lens=case.lens)
    with pytest.raises(ValueError, match="out must be"):
        ops.attention_pick(*a, pick, 0, out[:, :64], kv_lens=case.lens)
    with pytest.raises(ValueError, match="out must be"):
        ops.attention_pick(*a, pick, 0, out.to(BF), kv_lens=case.lens)
    with pytest.raises(ValueError, match="out must be"):
        ops.attention_pick(*a, pick, 0, out.t(), kv_lens=case.lens)
    with pytest.raises(ValueError, match="key_segments"):
        ops.attention_pick(*a, pick, 1, out, key_segments=case.ks[:, :64].contiguous(), query_segments=case.qm)
    with pytest.raises(_lib.PmhipError, match="want=256"):
        ops.attention_pick(*a, pick, 256, out, kv_lens=case.lens)
    with pytest.raises(_lib.PmhipError):
        ops.attention_pick(*a, pick.cpu(), 0, out, kv_lens=case.lens)                 # host memory: no CPU fallback
    lib, p = _lib.load(), ops._p
    null = lambda **kw: lib.pmhip_attention_pick(_lib.F32, p(case.q), p(case.k), p(case.vt), p(out), H * 64, B, H, 64, NQ, 65, 128, 0,
                                                 kw.get("lens"), kw.get("ks"), kw.get("qm"), kw.get("pick"), 0, None)
    assert null(lens=p(case.lens)) == _lib.PMHIP_EINVAL and b"pick is NULL" in lib.pmhip_last_error()
    assert null(pick=p(pick)) == _lib.PMHIP_EINVAL and b"exactly one" in lib.pmhip_last_error()
    assert null(pick=p(pick), ks=p(case.ks)) == _lib.PMHIP_EINVAL and b"go together" in lib.pmhip_last_error()
    # the family's own checks follow under the entry's name: an output row stride below heads * dim_head
    assert lib.pmhip_attention_pick(_lib.F32, p(case.q), p(case.k), p(case.vt), p(out), 64, B, H, 64, NQ, 65, 128, 0, p(case.lens), None,
                                    None, p(pick), 0, None) == _lib.PMHIP_EINVAL
    assert b"attention_pick: ldo=64" in lib.pmhip_last_error()
