"""pmhip_attention_weighted and pmhip_key_bias: a WEIGHT per key on top of the key set per query.  B = 3,
heads = 2, Nq = 80 (the last query tile is ragged), key counts 1 / 63 / 64 / 65 / 129 / 416, the three layouts of
tests/test_gpu_attention_segments.py rebuilt in tests/weight_ref.py with weights drawn from {0, 1/8, 1, 8} over them and NaN K / V rows
where the weight is 0:

  held element-wise to attention_probes.bound with the score error of weight_ref.score_error against the float64 restatement;
  the counter-check -- the same finite inputs through pmhip_attention_segments, the weights ignored -- beyond 100 x the bound;
  weights of 1 equal the segmented entry, rows of weight 0 equal the same rows marked 255, every image alone equals its rows in the
  batch and the 64- and the 128-query form of the bf16 kernel agree, all bit for bit;
  integer weights equal repeated rows across a tile edge, within the sum of the two bounds;
  the edges of the weight range; and the conversion kernel itself."""
import numpy as np
import pytest
import torch

import attention_probes as P
import region_ref as R
import weight_ref as W
from gpu_common import dev, n, t
from paintmind_amd import _lib, ops

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
MODES = pytest.mark.parametrize("exp2", [True, False], ids=["exp2", "exp"])
B, H, NQ = 3, 2, 80


def attend(d, dtype, exp2, weighted=True, rows=slice(None), ks=None, w=None):
    """the launch: K / V^T laid out with NaN in [Nkv, Nkv_pad) -> (out tensor, out [B, H, Nq, dh] as numpy)"""
    nkv, dh = d["k"].shape[-2:]
    kp, vtp = P.pad_kv(d["k"][rows], d["v"][rows], -(-nkv // 64) * 64)
    q = d["q"][rows]
    kw = dict(key_segments=t((d["ks"] if ks is None else ks)[rows]), query_segments=t(d["qm"][rows].view(np.int32)))
    if weighted:
        kw["key_weights"] = t((d["w"] if w is None else w)[rows].astype(np.float32))
    out = ops.attention(t(q, dtype), t(kp, dtype), t(vtp, dtype), nkv, use_exp2=exp2, **kw)
    return out, P.from_out_layout(n(out), q.shape[0], q.shape[1], q.shape[2], dh)


def held(d, o, kind, exp2, what, failures):
    ref, Bd, s = W.bounds(P, d, kind, exp2)
    ratio, msg = P.check_bound(o, ref, Bd, np.where(np.isfinite(s), s, -1e300), what)
    if msg:
        failures.append(msg)
    return ratio, ref, Bd


@DTYPES
@MODES
def test_tuned_kernels_hold_the_bounds_and_the_unweighted_entry_does_not(dtype, exp2):
    """dim_head 64: attention_seg_bias_kernel (f32) and attention_bf16_seg_bias_kernel at 64 queries per workgroup"""
    kind = "bf16" if dtype == BF else "f32"
    worst, failures = {}, []
    ops.attention_fallbacks(reset=True)
    for nkv in W.NKVS:
        d = W.inputs(P.gauss, nkv)
        _, o = attend(d, dtype, exp2)
        worst[nkv], ref, Bd = held(d, o, kind, exp2, f"{kind} exp2={exp2} Nkv={nkv}", failures)
        # the counter-check: the weights ignored.  Finite inputs (the NaN rows zeroed), the same segments
        loose = dict(d, k=np.nan_to_num(d["k"]).astype(np.float32), v=d["vz"])
        _, o_un = attend(loose, dtype, exp2, weighted=False)
        gap, _ = P.worst_ratio(o_un, ref, Bd)
        print(f"Nkv={nkv}: weighted err / B {worst[nkv]:.3f}, unweighted {gap:.3g}")
        if nkv > 1 and not gap > 100.0:              # (one key: its weight cancels)
            failures.append(f"Nkv={nkv}: the unweighted entry stays within {gap:.3g} x the bound: the weights do not bite")
    assert ops.attention_fallbacks(reset=True) == 0  # every half-tile on the exact path: these launches are never counted
    print(f"weighted {kind} {'exp2' if exp2 else 'exp'}: largest err / B", {k: round(v, 3) for k, v in worst.items()})
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])


@pytest.mark.parametrize("dh,heads", [(32, 2), (128, 2)])
@DTYPES
@MODES
def test_plain_path_holds_the_bounds(dh, heads, dtype, exp2):
    """attention_dh_seg_bias_kernel at dim_head 32 and 128"""
    kind = "bf16_dh" if dtype == BF else "f32"
    worst, failures = {}, []
    for nkv in W.NKVS:
        d = W.inputs(P.gauss, nkv, dh, heads=heads)
        _, o = attend(d, dtype, exp2)
        worst[nkv], _, _ = held(d, o, kind, exp2, f"dim_head {dh} {kind} exp2={exp2} Nkv={nkv}", failures)
    print(f"weighted dim_head {dh} {kind} {'exp2' if exp2 else 'exp'}: largest err / B", {k: round(v, 3) for k, v in worst.items()})
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])


@pytest.mark.parametrize("dh", [64, 32])
@DTYPES
@MODES
def test_bit_identities(dh, dtype, exp2):
    """(3) w == 1 everywhere is the segmented entry; (4) rows of weight 0 are the same rows marked 255; (5) every image alone equals
    its rows in the batch; and key_weights alone is key_weights beside the neutral arrays -- all bit for bit"""
    for nkv in (65, 416):
        d = W.inputs(P.gauss, nkv, dh)
        finite = dict(d, k=np.nan_to_num(d["k"]).astype(np.float32), v=d["vz"])
        ones, _ = attend(finite, dtype, exp2, w=np.ones_like(d["w"]))
        seg, _ = attend(finite, dtype, exp2, weighted=False)
        assert torch.equal(ones, seg), (nkv, "weights of 1")
        out, _ = attend(d, dtype, exp2)
        assert torch.isfinite(out).all()
        marked, _ = attend(d, dtype, exp2, ks=np.where(d["w"] == 0, R.PAD, d["ks"]).astype(np.uint8), w=np.where(d["w"] == 0, 1, d["w"]))
        assert torch.equal(out, marked), (nkv, "weight 0 against segment 255")
        out = out.view(B, NQ, -1)
        for b in range(B):
            alone, _ = attend(d, dtype, exp2, rows=slice(b, b + 1))
            assert torch.equal(out[b], alone), (nkv, b)
        # alone: the neutral arrays are built by ops.attention
        kp, vtp = P.pad_kv(d["k"], d["v"], -(-nkv // 64) * 64)
        w = np.where(d["ks"] == R.PAD, 0, d["w"]).astype(np.float32)
        w[:, 0] = 1
        args = (t(d["q"], dtype), t(kp, dtype), t(vtp, dtype), nkv)
        a = ops.attention(*args, use_exp2=exp2, key_weights=t(w))
        b_ = ops.attention(*args, use_exp2=exp2, key_weights=t(w), key_segments=t(np.zeros((B, nkv), np.uint8)),
                           query_segments=t(np.ones((B, NQ), np.int32)))
        assert torch.equal(a, b_) and torch.isfinite(a).all()


@MODES
def test_both_workgroup_forms_of_the_bf16_kernel(exp2):
    """128 queries per workgroup (B = 32, heads = 16: 512 workgroups; Nq = 80 leaves its second half ragged) against every image
    alone, which runs 64 per workgroup: the forms are bit-identical per 16-query tile.  Image 0..2 also held to the bound."""
    batch, heads, nkv = 32, 16, 129
    qf = lambda b, h, nq: 2 if b * h * -(-nq // 128) >= 512 else 1          # the launcher's rule: B, heads and Nq only
    assert qf(batch, heads, NQ) == 2 and qf(1, heads, NQ) == 1 and qf(B, H, NQ) == 1
    d = W.inputs(P.gauss, nkv, batch=batch, heads=heads)
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
@MODES
def test_integer_weights_are_repeated_rows_across_a_tile_edge(dh, dtype, exp2):
    """(6) Nkv 63 -> 66 and 127 -> 130: weights 2 and 3 on two rows against the context with those rows repeated behind the last one
    (through the existing segmented entry): |weighted - duplicated| <= the sum of the two bounds, the two float64 references equal"""
    kind = ("bf16" if dtype == BF else "f32") if dh == 64 else ("bf16_dh" if dtype == BF else "f32")
    failures = []
    for nkv in (63, 127):
        g = P.gauss((B, H), NQ, nkv, 4.0, dh)
        ks = np.tile((np.arange(nkv) % 3).astype(np.uint8), (B, 1))
        qm = np.tile((1 | (np.uint32(2) << (np.arange(NQ, dtype=np.uint32) % 2))).astype(np.uint32), (B, 1))
        i, j = 7, nkv - 1
        w = np.ones((B, nkv), np.float32)
        w[:, i], w[:, j] = 2, 3
        d = dict(q=g["q"], k=g["k"], v=g["v"], kz=g["k"], vz=g["v"], ks=ks, qm=qm, w=w)
        rep = lambda a, ax: np.concatenate([a, np.take(a, [i, j, j], axis=ax)], axis=ax)
        dd = dict(q=g["q"], k=rep(g["k"], 2), v=rep(g["v"], 2), ks=rep(ks, 1), qm=qm)
        _, o_w = attend(d, dtype, exp2)
        _, o_d = attend(dd, dtype, exp2, weighted=False)
        ref_w, Bd_w, _ = W.bounds(P, d, kind, exp2)
        ref_d, A_d, s_d = R.attention(dd["q"], dd["k"], dd["v"], dd["ks"], dd["qm"], exp2)
        Bd_d = P.bound(kind, ref_d, A_d, P.score_error(dd["q"], dd["k"], np.where(np.isfinite(s_d), s_d, 0.0), exp2), nkv + 3)
        assert np.abs(ref_w - ref_d).max() < 1e-12
        ratio, idx = P.worst_ratio(o_w, o_d.astype(np.float64), Bd_w + Bd_d)
        print(f"dim_head {dh} {kind} exp2={exp2} Nkv {nkv} -> {nkv + 3}: |weighted - duplicated| / (sum of the bounds) = {ratio:.3f}")
        if ratio > 1.0:
            failures.append(f"Nkv={nkv}: weighted {o_w[idx]!r} duplicated {o_d[idx]!r} at {idx}, {ratio:.3g} x the sum of the bounds")
        _, plain = attend(d, dtype, exp2, weighted=False)
        assert P.worst_ratio(plain, ref_w, Bd_w)[0] > 100.0                   # and the weights matter here
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("dh", [64, 32])
@DTYPES
@MODES
def test_the_edges_of_the_weight_range(dh, dtype, exp2):
    """(7) image 0: the query whose only allowed key is the LAST one, with w = 2^-20 there -- every earlier tile denied, the running
    max still "none" when the tiny weight arrives; image 2: the loud keys, which no query allows, at w = 2^20; image 1: a key at
    w = 2^20 with the lowest score of every row"""
    kind = ("bf16" if dtype == BF else "f32") if dh == 64 else ("bf16_dh" if dtype == BF else "f32")
    failures = []
    for nkv in (129, 416):
        d = W.inputs(P.gauss, nkv, dh)
        d = {key: val.copy() for key, val in d.items()}
        w = d["w"]
        w[0, nkv - 1] = 2.0 ** -20
        loud = d["ks"][2] == W.S_LOUD
        assert loud.any()
        w[2, loud] = 2.0 ** 20
        d["k"][2][:, loud] = 512.0                                            # (finite again where the draw had given weight 0)
        d["v"][2][:, loud] = 1.0
        d["kz"][2][:, loud] = 0.0
        d["vz"][2][:, loud] = 1.0
        j0 = 70                                                               # a key of image 1's middle tile (second tile, first half)
        d["q"][1] = np.abs(d["q"][1])
        for name in ("k", "kz"):
            d[name][1][:, j0] = -3.0
        for name in ("v", "vz"):
            d[name][1][:, j0] = np.nan_to_num(d[name][1][:, j0])
        w[1, j0] = 2.0 ** 20
        ref, Bd, s = W.bounds(P, d, kind, exp2)
        plain = np.einsum("bhqd,bhkd->bhqk", d["q"].astype(np.float64), d["kz"].astype(np.float64))[1]
        live = np.isfinite(s[1])
        assert (np.where(live, plain, np.inf).argmin(-1)[live[..., j0]] == j0).all()      # the lowest score of every row that allows it
        _, o = attend(d, dtype, exp2)
        ratio, msg = P.check_bound(o, ref, Bd, np.where(np.isfinite(s), s, -1e300), f"dim_head {dh} {kind} exp2={exp2} Nkv={nkv}")
        print(f"dim_head {dh} {kind} exp2={exp2} Nkv={nkv}: edges of the weight range, err / B {ratio:.3f}")
        if msg:
            failures.append(msg)
        q70 = o[0, :, 70]                                                     # that query's row IS the last key's V row
        want = d["v"][0][:, nkv - 1]
        assert np.allclose(q70, want, rtol=2.0 ** -7 if dtype == BF else 1e-5, atol=0), "the query with one tiny-weight key"
    assert not failures, "\n".join(failures)


@MODES
def test_key_bias(exp2):
    """(8) exact at 0 and 1; elsewhere within the error the reference counts"""
    rng = np.random.default_rng(3)
    w = np.exp2(rng.uniform(-20, 20, size=4099)).astype(np.float32)
    w[:8] = [0.0, 1.0, 0.125, 8.0, 2.0 ** -20, 2.0 ** 20, 1.4, 0.5]
    w = np.clip(w, 2.0 ** -20, 2.0 ** 20) * (w > 0)
    got = n(ops.key_bias(t(w), exp2))
    assert got[0] == -np.inf and got[1] == 0.0 and not np.signbit(got[1])
    live = w > 0
    exact = np.log2(w[live].astype(np.float64)) * (1.0 if exp2 else W.LN2)
    err = np.abs(got[live].astype(np.float64) - exact)
    tol = W.bias_error(w[live], exp2)
    assert (err <= tol).all(), (float((err / np.maximum(tol, 1e-300)).max()), w[live][np.argmax(err - tol)])
    if exp2:
        assert got[2] == -3.0 and got[3] == 3.0 and got[4] == -20.0 and got[5] == 20.0
    got2 = n(ops.key_bias(t(w.reshape(-1, 1)), exp2))
    assert got2.shape == (4099, 1) and np.array_equal(got2.reshape(-1), got, equal_nan=True)


def test_the_arguments_are_checked():
    q = torch.zeros(2, 1, 16, 64, device=dev())
    k, vt = torch.zeros(2, 1, 64, 64, device=dev()), torch.zeros(2, 1, 64, 64, device=dev())
    ks, qs = torch.zeros(2, 64, dtype=torch.uint8, device=dev()), torch.ones(2, 16, dtype=torch.int32, device=dev())
    w = torch.ones(2, 64, device=dev())
    assert torch.equal(ops.attention(q, k, vt, 64, key_segments=ks, query_segments=qs, key_weights=w), torch.zeros(32, 64, device=dev()))
    with pytest.raises(ValueError, match="exclude"):
        ops.attention(q, k, vt, 64, key_weights=w, kv_lens=torch.ones(2, dtype=torch.int32, device=dev()))
    with pytest.raises(ValueError, match="come together"):
        ops.attention(q, k, vt, 64, key_segments=ks, key_weights=w)
    with pytest.raises(ValueError, match="key_weights"):
        ops.attention(q, k, vt, 64, key_weights=w[:, :63].contiguous())
    with pytest.raises(ValueError, match="key_weights"):
        ops.attention(q, k, vt, 64, key_weights=w.double())
    with pytest.raises(_lib.PmhipError):
        ops.attention(q, k, vt, 64, key_weights=w.cpu())                                       # host memory: no CPU fallback
    lib = _lib.load()
    args = (_lib.F32, q.data_ptr(), k.data_ptr(), vt.data_ptr(), torch.empty(32, 64, device=dev()).data_ptr(), 64, 2, 1, 64, 16, 64, 64, 0)
    for arrays in ((None, qs.data_ptr(), w.data_ptr()), (ks.data_ptr(), None, w.data_ptr()), (ks.data_ptr(), qs.data_ptr(), None)):
        assert lib.pmhip_attention_weighted(*args, *arrays, None) == _lib.PMHIP_EINVAL
    assert lib.pmhip_key_bias(None, w.data_ptr(), 4, 1, None) == _lib.PMHIP_EINVAL
