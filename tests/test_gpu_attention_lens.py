"""pmhip_attention_lens: a key count per image.  The contract is the scalar entry's, per image: the rows of image b equal, bit
for bit, ``ops.attention`` on that image alone with ``n_kv = lens[b]`` -- the same kernel body with the key count read once per
workgroup -- and K rows / V^T columns at or beyond ``lens[b]`` (NaN here) never reach a result.  The scalar entry itself is held
to float64 by tests/test_gpu_attention_probes.py; the bf16 / dim_head 64 case is held to the same element-wise bound here too,
at each image's own length."""
import numpy as np
import pytest
import torch

import attention_probes as P
from gpu_common import dev, n, t
from paintmind_amd import _lib, ops

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
MODES = pytest.mark.parametrize("exp2", [True, False], ids=["exp2", "exp"])

NKV, NKV_PAD = 416, 448


def _shuffled_edges():
    lens = np.array(P.EDGE_NKV)
    return lens[np.random.default_rng(5).permutation(len(lens))]          # neighbours differ


def _poisoned(d, lens, nkv_pad):
    """K [B,H,nkv_pad,dh] / V^T [B,H,dh,nkv_pad] with NaN in image b's K rows and V^T columns at or beyond lens[b]"""
    B = d["q"].shape[0]
    kp = np.empty(d["k"].shape[:2] + (nkv_pad, d["k"].shape[-1]), np.float32)
    vtp = np.empty(d["v"].shape[:2] + (d["v"].shape[-1], nkv_pad), np.float32)
    for b in range(B):
        kp[b], vtp[b] = P.pad_kv(d["k"][b, :, :lens[b]], d["v"][b, :, :lens[b]], nkv_pad)
    return kp, vtp


def _per_image_failures(out, q, k, vt, lens, exp2, what):
    """out [B * Nq, H * dh] against the scalar entry on every image alone with n_kv = lens[b], bit for bit"""
    B, _, Nq, _ = q.shape
    out = out.view(B, Nq, -1)
    failures = []
    if not torch.isfinite(out).all():
        failures.append(f"{what}: {int((~torch.isfinite(out)).sum())} elements are not finite")
    for b in range(B):
        alone = ops.attention(q[b:b + 1].contiguous(), k[b:b + 1].contiguous(), vt[b:b + 1].contiguous(), int(lens[b]), use_exp2=exp2)
        if not torch.equal(out[b], alone):
            bad = torch.nonzero(out[b] != alone)
            failures.append(f"{what}: image {b} (len {int(lens[b])}) differs from itself alone in {len(bad)} elements, first (query, head * dh "
                            f"+ column) = {bad[0].tolist()}")
    return failures


@DTYPES
@MODES
def test_every_key_count_edge_dim_head_64(dtype, exp2):
    """B = 27 images whose lengths are the edge list in a shuffled order, H = 2, Nq = 80 (a full and a ragged block of 64 queries),
    Nkv = 416 in a layout of 448; bf16 additionally against float64 at each image's own length"""
    lens = _shuffled_edges()
    B, H, Nq = len(lens), 2, 80
    assert B == 27 and lens.max() == NKV
    d = P.gauss((B, H), Nq, NKV, 4.0)
    kp, vtp = _poisoned(d, lens, NKV_PAD)
    q, k, vt = t(d["q"], dtype), t(kp, dtype), t(vtp, dtype)
    out = ops.attention(q, k, vt, NKV, use_exp2=exp2, kv_lens=t(lens.astype(np.int32)))
    failures = _per_image_failures(out, q, k, vt, lens, exp2, f"{dtype} exp2={exp2}")
    if dtype == BF:
        o = P.from_out_layout(n(out), B, H, Nq, 64)
        worst = 0.0
        for b in range(B):
            qb, kb, vb = d["q"][b], d["k"][b, :, :lens[b]], d["v"][b, :, :lens[b]]
            ref, A, s = P.reference(qb, kb, vb, exp2)
            Bd = P.bound("bf16", ref, A, P.score_error(qb, kb, s, exp2), int(lens[b]))
            ratio, msg = P.check_bound(o[b], ref, Bd, s, f"image {b} len {int(lens[b])}")
            worst = max(worst, ratio)
            if msg:
                failures.append(msg)
        print(f"lens edge walk bf16 {'exp2' if exp2 else 'exp'}: largest err / B {worst:.3f}")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])


@pytest.mark.parametrize("dh,H", [(16, 4), (128, 2)])
@DTYPES
@MODES
def test_every_key_count_edge_other_dim_head(dh, H, dtype, exp2):
    """the plain path (attention_dh_lens_kernel): the same 27 lengths, Nq = 80"""
    lens = _shuffled_edges()
    B, Nq = len(lens), 80
    d = P.gauss((B, H), Nq, NKV, 4.0, dh)
    kp, vtp = _poisoned(d, lens, NKV_PAD)
    q, k, vt = t(d["q"], dtype), t(kp, dtype), t(vtp, dtype)
    out = ops.attention(q, k, vt, NKV, use_exp2=exp2, kv_lens=t(lens.astype(np.int32)))
    failures = _per_image_failures(out, q, k, vt, lens, exp2, f"dim_head {dh} {dtype} exp2={exp2}")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])


def _qf(B, H, Nq):
    """the bf16 launcher's rule: the largest workgroup (64 * QF queries) that still gives 512 workgroups; B, H and Nq only"""
    return 4 if B * H * -(-Nq // 256) >= 512 else 2 if B * H * -(-Nq // 128) >= 512 else 1


@pytest.mark.parametrize("qf,B,H,Nq", [(4, 32, 16, 64), (2, 32, 8, 160), (1, 2, 2, 80)])
@MODES
def test_every_workgroup_form_of_the_bf16_kernel(qf, B, H, Nq, exp2):
    """256, 128 and 64 queries per workgroup, lengths cycling through the edge list: every image equals, bit for bit, the scalar
    entry on that image alone (which runs 64 queries per workgroup: the forms are bit-identical per 16-query tile)"""
    assert _qf(B, H, Nq) == qf
    lens = np.array([P.EDGE_NKV[(7 * b + 3) % len(P.EDGE_NKV)] for b in range(B)])
    g = torch.Generator(device=dev()).manual_seed(31 * B + H)
    rand = lambda *s: torch.randn(*s, device=dev(), generator=g)
    q = (rand(B, H, Nq, 64) * 0.5).to(BF)
    k, vt = rand(B, H, NKV_PAD, 64).to(BF), rand(B, H, 64, NKV_PAD).to(BF)
    for b in range(B):
        k[b, :, int(lens[b]):] = float("nan")
        vt[b, :, :, int(lens[b]):] = float("nan")
    ops.attention_fallbacks(reset=True)
    out = ops.attention(q, k, vt, NKV, use_exp2=exp2, kv_lens=t(lens.astype(np.int32)))
    failures = _per_image_failures(out, q, k, vt, lens, exp2, f"QF {qf} exp2={exp2}")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])
    assert ops.attention_fallbacks(reset=True) == 0


@pytest.mark.parametrize("dh,H", [(64, 2), (16, 4)])
@DTYPES
def test_full_and_clamped_lengths(dh, H, dtype):
    """lens all Nkv IS the entry without lengths; 0 behaves as 1 and Nkv + 5 (inside the layout, where K / V^T hold NaN) as Nkv"""
    B, Nq = 3, 80
    exp2 = dtype == BF
    d = P.gauss((B, H), Nq, NKV, 4.0, dh)
    kp, vtp = P.pad_kv(d["k"], d["v"], NKV_PAD)                        # NaN in [Nkv, Nkv_pad)
    q, k, vt = t(d["q"], dtype), t(kp, dtype), t(vtp, dtype)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev())
    want = ops.attention(q, k, vt, NKV, use_exp2=exp2)
    assert torch.isfinite(want).all()
    assert torch.equal(ops.attention(q, k, vt, NKV, use_exp2=exp2, kv_lens=i32(NKV, NKV, NKV)), want)
    assert torch.equal(ops.attention(q, k, vt, NKV, use_exp2=exp2, kv_lens=i32(NKV + 5, NKV, NKV + 5)), want)
    low = ops.attention(q, k, vt, NKV, use_exp2=exp2, kv_lens=i32(0, NKV, -7))
    assert torch.equal(low, ops.attention(q, k, vt, NKV, use_exp2=exp2, kv_lens=i32(1, NKV, 1)))
    failures = _per_image_failures(low, q, k, vt, [1, NKV, 1], exp2, "clamped to 1")
    assert not failures, "\n".join(failures)
    # one key: the output row is that key's V row, whatever the query
    v0 = t(d["v"][0, :, 0], dtype)                                      # [H, dh]
    assert torch.equal(low.view(B, Nq, H, dh)[0], v0[None].expand(Nq, H, dh))


def test_lengths_are_required_and_checked():
    q = torch.zeros(2, 1, 16, 64, device=dev())
    k, vt = torch.zeros(2, 1, 64, 64, device=dev()), torch.zeros(2, 1, 64, 64, device=dev())
    with pytest.raises(ValueError):
        ops.attention(q, k, vt, 64, kv_lens=torch.ones(3, dtype=torch.int32, device=dev()))
    with pytest.raises(ValueError):
        ops.attention(q, k, vt, 64, kv_lens=torch.ones(2, dtype=torch.int64, device=dev()))
    with pytest.raises(_lib.PmhipError):
        ops.attention(q, k, vt, 64, kv_lens=torch.ones(2, dtype=torch.int32))        # host memory: no CPU fallback
