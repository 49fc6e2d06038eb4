"""Every form of the attention kernels against float64, ELEMENT by element, at the key counts where the kernels change shape.

The comparisons of test_gpu_ops.py / test_gpu_fuzz.py are max |err| / max |ref| over the whole output: one wrong key of several
hundred stays below their 4e-2 in bf16.  Here every element is held to the derived bound of tests/attention_probes.py (no
factor on top of it), the selector probe must come out bit for bit, and tests/test_attention_probes_cpu.py shows on the CPU that
these checks reject a single dropped, added, exchanged or shifted key.  K rows and V^T columns in [Nkv, Nkv_pad) hold NaN.

Both modes of both dtypes run: use_exp2 = 0 in bf16 (attention_bf16_kernel<false, QF>: expf on the fast path, the overflow vote in
nats) and use_exp2 = 1 in f32 (attention_kernel<true, 2>: the deferred running-max rescale) have no caller in the
product, which always passes use_exp2 = (dtype is bf16), but are public forms of pmhip_attention / pmhip_attention_dh.
"""
import numpy as np
import pytest
import torch

import attention_probes as P
from gpu_common import dev, n, t
from paintmind_amd import ops

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
MODES = pytest.mark.parametrize("exp2", [True, False], ids=["exp2", "exp"])


def _attend(d, dtype, exp2):
    """one launch on a family's arrays, NaN in the padding -> [B, H, Nq, dh] float"""
    B, H, Nq, dh = d["q"].shape
    nkv = d["k"].shape[-2]
    kp, vtp = P.pad_kv(d["k"], d["v"], -(-nkv // 64) * 64)
    out = n(ops.attention(t(d["q"], dtype), t(kp, dtype), t(vtp, dtype), nkv, use_exp2=exp2))
    return P.from_out_layout(out, B, H, Nq, dh)


def _held_to_bound(kind, name, d, out, exp2, worst, failures):
    nkv = d["k"].shape[-2]
    ref, A, s = P.reference(d["q"], d["k"], d["v"], exp2)
    Bd = P.bound(kind, ref, A, P.score_error(d["q"], d["k"], s, exp2), nkv)
    ratio, msg = P.check_bound(out, ref, Bd, s, f"{name} Nkv={nkv}")
    worst[name] = max(worst.get(name, 0.0), ratio)
    if msg:
        failures.append(msg)


def _selector_bit_for_bit(d, out, nkv, failures):
    bad = np.argwhere((out != d["expect"]).any(-1))
    if len(bad):
        b, h, i = (int(x) for x in bad[0])
        failures.append(f"selector Nkv={nkv}: {len(bad)} rows are not their target's V row bit for bit; first (batch, head, query) = "
                        f"{(b, h, i)}, target key {int(d['target'][b, h, i])}: got {out[b, h, i, :4]} want {d['expect'][b, h, i, :4]}")


@DTYPES
@MODES
def test_edge_walk_on_the_smallest_launch(dtype, exp2):
    """B = 2, H = 3, Nq = 80 (one full and one ragged block of 64 queries; in bf16 the 64-query workgroup and the grid map for a
    (batch, head) count that is no multiple of 8) at every key count of the edge list, three families (the selector with
    Nq = Nkv).  The selector's conditions are asserted before it runs; in bf16 it must come out bit for bit and no workgroup
    may fall back to the exact path in any family."""
    B, H, Nq = 2, 3, 80
    bf = dtype == BF
    kind = "bf16" if bf else "f32"
    worst, failures = {}, []
    if bf:
        ops.attention_fallbacks(reset=True)
    for nkv in P.EDGE_NKV:
        fams = {"selector": P.selector((B, H), nkv, exp2), "uniform": P.uniform((B, H), Nq, nkv),
                "gauss0.3": P.gauss((B, H), Nq, nkv, 0.3), "gauss4": P.gauss((B, H), Nq, nkv, 4.0)}
        mass, log2_l = P.selector_conditions(fams["selector"]["codes"], fams["selector"]["c"], exp2)
        assert mass <= 2.0 ** -12 and log2_l <= 60.0, (nkv, mass, log2_l)
        for name, d in fams.items():
            out = _attend(d, dtype, exp2)
            _held_to_bound(kind, name, d, out, exp2, worst, failures)
            if bf and name == "selector":
                _selector_bit_for_bit(d, out, nkv, failures)
        if bf:
            fb = ops.attention_fallbacks(reset=True)
            if fb:
                failures.append(f"Nkv={nkv}: {fb} workgroups fell back to the exact path, none is due")
    print(f"edge walk {kind} {'exp2' if exp2 else 'exp'}: largest err / B", {k: round(v, 3) for k, v in worst.items()})
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])


@MODES
@pytest.mark.parametrize("nkv", [65, 193])
def test_f32_grouped_grid_map_and_second_query_block(nkv, exp2):
    """The f32 cases of the edge walk run B * H = 6 and Nq = 80: the plain grid map and one workgroup per (batch, head).  Here
    B = 2, H = 4 (B * H % 8 == 0: attention_kernel's XCD-grouped map) and Nq = 144 (a full block of 128 queries and a ragged one
    of 16), at Nkv = 65 (a ragged second tile) and 193 (four tiles: the 3-stage K / V^T ring wraps), both gauss families, held
    to the same f32 bound."""
    worst, failures = {}, []
    for name, sigma in (("gauss0.3", 0.3), ("gauss4", 4.0)):
        d = P.gauss((2, 4), 144, nkv, sigma)
        _held_to_bound("f32", name, d, _attend(d, F32, exp2), exp2, worst, failures)
    print(f"f32 grouped map Nkv={nkv} {'exp2' if exp2 else 'exp'}: largest err / B", {k: round(v, 3) for k, v in worst.items()})
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])


def _qf(B, H, Nq):
    """pm_attention_bf16's rule: the largest workgroup (64 * QF queries) that still gives kFill = 512 workgroups"""
    return 4 if B * H * -(-Nq // 256) >= 512 else 2 if B * H * -(-Nq // 128) >= 512 else 1


@pytest.mark.parametrize("qf,B,H,Nq", [(4, 64, 8, 272), (4, 73, 7, 272), (2, 32, 8, 144), (2, 257, 1, 144)])
def test_every_workgroup_size_and_both_grid_maps_bf16(qf, B, H, Nq):
    """pm_attention_bf16 takes QF = 4 (256 queries per workgroup) when B * H * ceil(Nq / 256) reaches kFill = 512 workgroups, else
    QF = 2 when B * H * ceil(Nq / 128) does, else QF = 1:
        (64, 8, 272): 512 * 2 >= 512 -> QF 4, B * H % 8 == 0: the XCD-grouped grid map     (73, 7, 272): 511 * 2 -> QF 4, the plain map
        (32, 8, 144): 256 * 1 < 512, 256 * 2 >= 512 -> QF 2, grouped map                   (257, 1, 144): 257, 514 -> QF 2, plain map
    and the first two images alone (16, 14, 16, 2 (batch, head)s) run QF = 1 in the grouped, plain, grouped, plain map.  The timing
    families count launches per family only, not per workgroup size, so the split is asserted by the rule.  Nq has one full
    workgroup and a ragged one of 16 queries.  At every key count of the edge list, in both modes, on overflow-free gauss data
    (score sigma 4), the first two images of the batch equal bit for bit what they are alone: with the edge walk above, which
    holds QF = 1 to float64, that pins QF = 4 and 2.  At Nkv = 128, 257, 384, 416 the selector runs on the whole batch, with a
    permutation and values per (batch, head), against the gather (one code book: its conditions are checked once on its Gram
    matrix)."""
    assert _qf(B, H, Nq) == qf and _qf(2, H, Nq) == 1
    BH, npad = B * H, 448
    g = torch.Generator(device=dev()).manual_seed(17 * B + H)
    rand = lambda *s: torch.randn(*s, device=dev(), generator=g)
    q = (rand(B, H, Nq, 64) * 0.5).to(BF)
    k, vt = rand(B, H, npad, 64).to(BF), rand(B, H, 64, npad).to(BF)
    vsel = t(P.selector_values(np.arange(BH)[:, None, None], np.arange(npad)[None, :, None], np.arange(64)[None, None, :]), BF)
    bh = torch.arange(BH, device=dev())[:, None]
    failures = []
    ops.attention_fallbacks(reset=True)
    for nkv in P.EDGE_NKV:
        nkp = -(-nkv // 64) * 64
        kk, vv = k[:, :, :nkp].clone(), vt[:, :, :, :nkp].clone()
        kk[:, :, nkv:] = float("nan")
        vv[:, :, :, nkv:] = float("nan")
        for exp2 in (True, False):
            full = ops.attention(q, kk, vv, nkv, use_exp2=exp2).view(B, Nq, H * 64)
            alone = ops.attention(q[:2], kk[:2], vv[:2], nkv, use_exp2=exp2).view(2, Nq, H * 64)
            if not (torch.isfinite(full).all() and torch.equal(full[:2], alone)):
                bad = torch.nonzero((full[:2] != alone) | ~torch.isfinite(full[:2]))
                failures.append(f"gauss Nkv={nkv} exp2={exp2}: images 0, 1 differ from themselves alone in {len(bad)} elements, first "
                                f"(image, query, head * 64 + column) = {bad[0].tolist() if len(bad) else 'not finite elsewhere'}")
            if nkv not in (128, 257, 384, 416):
                continue
            codes = np.random.default_rng([3, nkv]).integers(0, 2, (nkv, 64)).astype(np.float32) * 2 - 1
            c = P.selector_scale(exp2)
            mass, log2_l = P.selector_conditions(codes, c, exp2)
            assert mass <= 2.0 ** -12 and log2_l <= 60.0, (nkv, mass, log2_l)
            target = torch.rand(BH, nkv, device=dev(), generator=g).argsort(-1)[:, torch.arange(Nq, device=dev()) % nkv]     # [BH, Nq]
            ks = torch.full((BH, nkp, 64), float("nan"), device=dev(), dtype=BF)
            ks[:, :nkv] = t(codes, BF)
            qs = (ks[bh, target].float() * c).to(BF).view(B, H, Nq, 64)
            vs = torch.full((BH, 64, nkp), float("nan"), device=dev(), dtype=BF)
            vs[:, :, :nkv] = vsel[:, :nkv].transpose(1, 2)
            out = ops.attention(qs, ks.view(B, H, nkp, 64), vs.view(B, H, 64, nkp), nkv, use_exp2=exp2)
            want = vsel[bh, target].view(B, H, Nq, 64).permute(0, 2, 1, 3).reshape(B * Nq, H * 64)
            if not torch.equal(out, want):
                bad = torch.nonzero((out != want).view(B, Nq, H, 64).any(-1))
                b, i, h = bad[0].tolist()
                failures.append(f"selector Nkv={nkv} exp2={exp2}: {len(bad)} rows are not their target's V row; first (batch, head, query) = "
                                f"{(b, h, i)}, target key {int(target[b * H + h, i])}")
    fb = ops.attention_fallbacks(reset=True)
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])
    assert fb == 0, fb


@pytest.mark.parametrize("dh,H", [(16, 4), (128, 2)])
@DTYPES
@MODES
def test_other_dim_head_is_held_to_the_bounds(dh, H, dtype, exp2):
    """pmhip_attention_dh (attention_dh_kernel: online softmax on the vector ALU, P in f32 in both dtypes), dim_head 16 and 128,
    both dtypes, both modes: B = 1, Nq = 70 (a full and a ragged block of 64 queries), Nkv in {1, 63, 64, 65, 130}, the gauss
    and uniform families with codes of length dim_head.  dim_head 128 runs H = 2; dim_head 16 runs H = 4, the fewest heads the
    entry point accepts there (heads * dim_head must be a multiple of 64)."""
    kind = "bf16_dh" if dtype == BF else "f32"
    worst, failures = {}, []
    for nkv in (1, 63, 64, 65, 130):
        fams = {"uniform": P.uniform((1, H), 70, nkv, dh), "gauss0.3": P.gauss((1, H), 70, nkv, 0.3, dh), "gauss4": P.gauss((1, H), 70, nkv, 4.0, dh)}
        for name, d in fams.items():
            _held_to_bound(kind, name, d, _attend(d, dtype, exp2), exp2, worst, failures)
    print(f"dim_head {dh} {kind} {'exp2' if exp2 else 'exp'}: largest err / B", {k: round(v, 3) for k, v in worst.items()})
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])
