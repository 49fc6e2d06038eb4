"""pmhip_attention_segments: a key SET per query.  B = 3, heads = 2, Nq = 80 (the last query tile is ragged),
key counts 1 / 63 / 64 / 65 / 129 / 416, six mask layouts spread over the three images of ONE launch:

  image 0   (a) queries that allow everything, (b) query 5 allowed only key 0, (c) query 70 allowed only the LAST key -- every
            earlier tile is fully denied to it, its running max is still "none" when they end
  image 1   (d) the 16-query fragment 16..31 denied the whole middle tile (keys 64..127, where there is one), (e) the other keys
            alternate between two segments and the queries between allowing one, the other, or both
  image 2   (f) keys of a segment NO query allows carry scores of about +1e4, padding keys (255) carry NaN in K and V: neither may
            reach a result or raise a running max

held element-wise to the bounds of tests/attention_probes.py against the float64 restatement of tests/region_ref.py; bit-exact
selector probes (equal scores, one-hot V rows: the output states which keys were averaged); every image alone equals its rows in
the batch, bit for bit; prefix-shaped masks agree with pmhip_attention_lens within the same bounds; and the counter-check -- the
same inputs through the unmasked entry -- must exceed 100 x the bound, so nothing here passes with the masks ignored."""
import numpy as np
import pytest
import torch

import attention_probes as P
import region_ref as R
from gpu_common import dev, n, t
from paintmind_amd import _lib, ops

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
MODES = pytest.mark.parametrize("exp2", [True, False], ids=["exp2", "exp"])
B, H, NQ = 3, 2, 80
NKVS = (1, 63, 64, 65, 129, 416)
ALL = 0xFFFFFFFF
S_FIRST, S_LAST, S_MID, S_EVEN, S_ODD, S_LOUD = 1, 2, 3, 4, 5, 6


def layouts(nkv, nq=NQ, seed=0):
    """-> (key_seg uint8 [3, nkv], query_mask uint32 [3, nq]) of the module docstring.  A query that the construction would leave
    without any key (only at the smallest key counts) allows everything instead."""
    rng = np.random.default_rng([seed, nkv])
    ks = np.zeros((3, nkv), np.uint8)
    qm = np.full((3, nq), ALL, np.uint32)
    # image 0
    ks[0, nkv - 1] = S_LAST
    ks[0, 0] = S_FIRST
    qm[0, 5] = 1 << S_FIRST
    qm[0, 70 % nq] = 1 << (S_LAST if nkv > 1 else S_FIRST)
    # image 1
    j = np.arange(nkv)
    ks[1] = np.where(j % 2 == 0, S_EVEN, S_ODD)
    if nkv > 128:
        ks[1, 64:128] = S_MID
    i = np.arange(nq)
    qm[1] = np.where(i % 3 == 0, ALL, np.where(i % 3 == 1, (1 << S_EVEN) | (1 << S_MID), (1 << S_ODD) | (1 << S_MID)))
    qm[1, 16:32] = (1 << S_EVEN) | (1 << S_ODD)
    # image 2: key 0 is text; the rest is text, loud or padding at random; no query allows the loud segment
    ks[2] = rng.choice(np.array([0, S_LOUD, R.PAD], np.uint8), size=nkv)
    ks[2, 0] = 0
    qm[2] = ALL & ~(1 << S_LOUD)
    ok = R.allowed(ks, qm)
    qm[~ok.any(-1)] = ALL
    qm[2] &= ~np.uint32(1 << S_LOUD)
    assert R.allowed(ks, qm).any(-1).all()
    return ks, qm


def inputs(nkv, dh=64, batch=3, heads=H, nq=NQ):
    """gauss data (sigma 4) under the layouts, image b using layout b % 3; image-2 layouts get positive queries, K rows of 512 on the
    loud keys (scores of 512 * sum q, about 1e4 at dim_head 64) and NaN K / V rows on the padding keys.
    -> dict(q, k, v: what the kernels see; kz, vz: the same with loud and padding rows zeroed, for the bound; ks, qm)"""
    d = P.gauss((batch, heads), nq, nkv, 4.0, dh)
    ks3, qm3 = layouts(nkv, nq)
    ks, qm = ks3[np.arange(batch) % 3], qm3[np.arange(batch) % 3]
    q, k, v = d["q"].copy(), d["k"].copy(), d["v"].copy()
    kz, vz = k.copy(), v.copy()
    for b in range(2, batch, 3):
        q[b] = np.abs(q[b])
        loud, pad = ks[b] == S_LOUD, ks[b] == R.PAD
        k[b][:, loud] = 512.0
        k[b][:, pad] = np.nan
        v[b][:, pad] = np.nan
        kz[b][:, loud | pad] = 0.0
        vz[b][:, pad] = 0.0
    return dict(q=q, k=k, v=v, kz=kz, vz=vz, ks=ks, qm=qm)


def attend(d, dtype, exp2, masked=True, rows=slice(None)):
    """the launch: K / V^T laid out with NaN in [Nkv, Nkv_pad) -> out [B, H, Nq, dh] as numpy"""
    nkv, dh = d["k"].shape[-2:]
    kp, vtp = P.pad_kv(d["k"][rows], d["v"][rows], -(-nkv // 64) * 64)
    q = d["q"][rows]
    kw = dict(key_segments=t(d["ks"][rows]), query_segments=t(d["qm"][rows].view(np.int32))) if masked else {}
    out = ops.attention(t(q, dtype), t(kp, dtype), t(vtp, dtype), nkv, use_exp2=exp2, **kw)
    return out, P.from_out_layout(n(out), q.shape[0], q.shape[1], q.shape[2], dh)


def bounds(d, kind, exp2):
    """-> (ref, Bd, s) of region_ref under the derivation of attention_probes.bound; the score error is taken over the rows that can
    reach a result (a loud row's magnitude belongs to no score that does)"""
    nkv = d["k"].shape[-2]
    ref, A, s = R.attention(d["q"], d["kz"], d["vz"], d["ks"], d["qm"], exp2)
    e_s = P.score_error(d["q"], d["kz"], np.where(np.isfinite(s), s, 0.0), exp2)
    return ref, P.bound(kind, ref, A, e_s, nkv), s


def held(d, o, kind, exp2, what, failures):
    ref, Bd, s = bounds(d, kind, exp2)
    ratio, msg = P.check_bound(o, ref, Bd, np.where(np.isfinite(s), s, -1e300), what)
    if msg:
        failures.append(msg)
    return ratio, ref, Bd


@DTYPES
@MODES
def test_tuned_kernels_hold_the_bounds_and_the_unmasked_entry_does_not(dtype, exp2):
    """dim_head 64: attention_seg_kernel (f32) and attention_bf16_seg_kernel at 64 queries per workgroup (B * heads = 6 picks it)"""
    kind = "bf16" if dtype == BF else "f32"
    worst, failures = {}, []
    for nkv in NKVS:
        d = inputs(nkv)
        _, o = attend(d, dtype, exp2)
        worst[nkv], ref, Bd = held(d, o, kind, exp2, f"{kind} exp2={exp2} Nkv={nkv}", failures)
        # the counter-check: the masks ignored.  Finite inputs (the NaN rows zeroed), every key attended to
        loose = dict(d, k=np.where(np.isnan(d["k"]), 0.0, d["k"]).astype(np.float32), v=d["vz"])
        _, o_un = attend(loose, dtype, exp2, masked=False)
        gap, _ = P.worst_ratio(o_un, ref, Bd)
        print(f"Nkv={nkv}: masked err / B {worst[nkv]:.3f}, unmasked {gap:.3g}")
        if nkv > 1 and not gap > 100.0:              # (one key: every query attends to it, masked or not)
            failures.append(f"Nkv={nkv}: the unmasked entry stays within {gap:.3g} x the bound: the layouts do not bite")
    ops.attention_fallbacks(reset=True)              # (the unmasked runs may have met the loud keys on the fast path)
    print(f"segments {kind} {'exp2' if exp2 else 'exp'}: largest err / B", {k: round(v, 3) for k, v in worst.items()})
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])


@pytest.mark.parametrize("dh,heads", [(32, 2), (128, 2)])
@DTYPES
@MODES
def test_plain_path_holds_the_bounds(dh, heads, dtype, exp2):
    """attention_dh_seg_kernel at dim_head 32 and 128"""
    kind = "bf16_dh" if dtype == BF else "f32"
    worst, failures = {}, []
    for nkv in NKVS:
        d = inputs(nkv, dh, heads=heads)
        _, o = attend(d, dtype, exp2)
        worst[nkv], _, _ = held(d, o, kind, exp2, f"dim_head {dh} {kind} exp2={exp2} Nkv={nkv}", failures)
    print(f"segments dim_head {dh} {kind} {'exp2' if exp2 else 'exp'}: largest err / B", {k: round(v, 3) for k, v in worst.items()})
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])


@pytest.mark.parametrize("dh", [64, 32])
@DTYPES
def test_selector_probes_state_which_keys_were_averaged(dh, dtype):
    """Q = 0: every allowed probability is exactly 1, l = the number of allowed keys, and with V[j, j % dh] = 1 column c of the
    output is count_c / count -- formed as the kernels form it, O * (1 / l) in f32, then one rounding to the output type.  Bit for
    bit; a key more, fewer or other than the mask says moves a column by 1 / count.  Padding rows hold NaN."""
    exp2 = dtype == BF
    failures = []
    for nkv in NKVS:
        ks, qm = layouts(nkv)
        u = P.uniform((B, H), NQ, nkv, dh)
        k, v = u["k"].copy(), u["v"].copy()
        k[2][:, ks[2] == R.PAD] = np.nan
        v[2][:, ks[2] == R.PAD] = np.nan
        _, o = attend(dict(q=u["q"], k=k, v=v, ks=ks, qm=qm), dtype, exp2)
        ok = R.allowed(ks, qm)                                                             # [B, Nq, Nkv]
        onehot = np.zeros((nkv, dh), np.float32)
        onehot[np.arange(nkv), np.arange(nkv) % dh] = 1.0
        count_c = (ok.astype(np.float32) @ onehot).astype(np.float32)                     # [B, Nq, dh]: exact small integers
        inv = np.float32(1.0) / ok.sum(-1).astype(np.float32)
        want = (count_c * inv[..., None]).astype(np.float32)
        if dtype == BF:
            want = P.bf16_round(want)
        want = np.broadcast_to(want[:, None], o.shape)
        if not np.array_equal(o, want):
            bad = np.argwhere(o != want)[0]
            failures.append(f"dim_head {dh} Nkv={nkv}: {int((o != want).sum())} elements differ, first (batch, head, query, column) = "
                            f"{bad.tolist()}: got {o[tuple(bad)]!r}, want {want[tuple(bad)]!r}; allowed keys "
                            f"{np.flatnonzero(ok[bad[0], bad[2]]).tolist()[:12]}")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])


@pytest.mark.parametrize("dh", [64, 32])
@DTYPES
@MODES
def test_an_image_alone_equals_its_rows_in_the_batch(dh, dtype, exp2):
    for nkv in (65, 416):
        d = inputs(nkv, dh)
        out, _ = attend(d, dtype, exp2)
        out = out.view(B, NQ, -1)
        assert torch.isfinite(out).all()
        for b in range(B):
            alone, _ = attend(d, dtype, exp2, rows=slice(b, b + 1))
            assert torch.equal(out[b], alone), (nkv, b)


def _qf(batch, heads, nq):
    """the bf16 launcher's rule for segmented launches: 128 queries per workgroup where that still gives 512 workgroups, else 64"""
    return 2 if batch * heads * -(-nq // 128) >= 512 else 1


@MODES
def test_both_workgroup_forms_of_the_bf16_kernel(exp2):
    """128 queries per workgroup (B = 32, heads = 16: 512 workgroups; Nq = 80 leaves its second half ragged) against every image
    alone, which runs 64 per workgroup: the forms are bit-identical per 16-query tile.  Image 0..2 also held to the bound."""
    batch, heads, nkv = 32, 16, 129
    assert _qf(batch, heads, NQ) == 2 and _qf(1, heads, NQ) == 1 and _qf(B, H, NQ) == 1
    d = inputs(nkv, batch=batch, heads=heads)
    ops.attention_fallbacks(reset=True)
    out, o = attend(d, BF, exp2)
    out = out.view(batch, NQ, -1)
    assert torch.isfinite(out).all()
    for b in range(batch):
        alone, _ = attend(d, BF, exp2, rows=slice(b, b + 1))
        assert torch.equal(out[b], alone), b
    failures = []
    first = {key: val[:3] for key, val in d.items()}
    held(first, o[:3], "bf16", exp2, f"128 queries per workgroup exp2={exp2}", failures)
    assert not failures, "\n".join(failures)
    assert ops.attention_fallbacks(reset=True) == 0


@pytest.mark.parametrize("dh", [64, 32])
@DTYPES
def test_prefix_shaped_masks_agree_with_the_per_image_lengths(dh, dtype):
    """keys [0, len_b) in segment 0, the rest padding, every query allowing segment 0: pmhip_attention_lens's problem.  Both within
    the bound of the same reference (the lens entry's fast path differs: bit equality is not asked for)."""
    exp2 = dtype == BF
    kind = ("bf16" if dtype == BF else "f32") if dh == 64 else ("bf16_dh" if dtype == BF else "f32")
    nkv, lens = 416, np.array([1, 129, 416], np.int32)
    d = P.gauss((B, H), NQ, nkv, 4.0, dh)
    ks = np.where(np.arange(nkv)[None, :] < lens[:, None], 0, R.PAD).astype(np.uint8)
    qm = np.ones((B, NQ), np.uint32)
    k, v = d["k"].copy(), d["v"].copy()
    for b in range(B):
        k[b][:, lens[b]:] = np.nan
        v[b][:, lens[b]:] = np.nan
    dd = dict(q=d["q"], k=k, v=v, kz=np.nan_to_num(k), vz=np.nan_to_num(v), ks=ks, qm=qm)
    _, o = attend(dd, dtype, exp2)
    kp, vtp = P.pad_kv(k, v, 448)
    o_lens = ops.attention(t(d["q"], dtype), t(kp, dtype), t(vtp, dtype), nkv, use_exp2=exp2, kv_lens=t(lens))
    o_lens = P.from_out_layout(n(o_lens), B, H, NQ, dh)
    failures = []
    held(dd, o, kind, exp2, "segments", failures)
    held(dd, o_lens, kind, exp2, "lens", failures)
    assert not failures, "\n".join(failures)


def test_a_query_without_any_key_gets_a_finite_row_and_the_arguments_are_checked():
    d = inputs(65)
    qm = d["qm"].copy()
    qm[0, 3] = 0                                                        # the contract's "unspecified but finite"
    qm[2, 7] = 1 << S_LOUD if (d["ks"][2] == S_LOUD).any() else 0
    for dtype in (BF, F32):
        out, _ = attend(dict(d, qm=qm), dtype, dtype == BF)
        assert torch.isfinite(out).all()
    q = torch.zeros(2, 1, 16, 64, device=dev())
    k, vt = torch.zeros(2, 1, 64, 64, device=dev()), torch.zeros(2, 1, 64, 64, device=dev())
    ks, qs = torch.zeros(2, 64, dtype=torch.uint8, device=dev()), torch.ones(2, 16, dtype=torch.int32, device=dev())
    assert torch.equal(ops.attention(q, k, vt, 64, key_segments=ks, query_segments=qs), torch.zeros(32, 64, device=dev()))
    with pytest.raises(ValueError, match="come together"):
        ops.attention(q, k, vt, 64, key_segments=ks)
    with pytest.raises(ValueError, match="exclude"):
        ops.attention(q, k, vt, 64, key_segments=ks, query_segments=qs, kv_lens=torch.ones(2, dtype=torch.int32, device=dev()))
    with pytest.raises(ValueError, match="key_segments"):
        ops.attention(q, k, vt, 64, key_segments=ks[:, :63].contiguous(), query_segments=qs)
    with pytest.raises(ValueError, match="query_segments"):
        ops.attention(q, k, vt, 64, key_segments=ks, query_segments=qs.long())
    with pytest.raises(_lib.PmhipError):
        ops.attention(q, k, vt, 64, key_segments=ks.cpu(), query_segments=qs)       # host memory: no CPU fallback
