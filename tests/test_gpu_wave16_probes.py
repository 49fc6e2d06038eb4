"""The wave-per-16-query attention kernels and the text towers' row operators on the cases of tests/wave16_probes.py, the cases
tests/test_wave16_probes_cpu.py shows to reject every named fault of its numpy emulation (DESIGN.md sections 4zk and 4zl).

Per attention case (family x L x L_pad x kv_lens triple x dtype): within the derived bound of tests/t5_ref.py / tests/clip_ref.py
against float64; the exact rows of the selector bit for bit; NaN padding and zero padding give the same bits; two launches give the same
bits; an image alone equals its rows in the batch; the raw entry writes the same bits into a framed output and nothing outside it.
Every comparison prints its worst |error| / bound before it asserts.  No fault runs here: faults exist only in the emulation."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_frames as AF
import clip_ref as RC
import t5_ref as RT
import wave16_probes as W
from gpu_common import dev
from paintmind_amd import _lib, ops

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
PM = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}
NAME = {torch.float32: "f32", torch.bfloat16: "bf16"}


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def launch(c, dtype, L_pad, lens=None, pad=W.NAN, images=None, framed=False):
    """the case's operands (tests/wave16_probes.layouts) through ops.attention_*; framed: through the raw entry into a framed output"""
    q, K, Vt = (torch.from_numpy(np.array(a)).to(device=dev(), dtype=dtype) for a in W.layouts(c, L_pad, lens, pad, images))
    nb, nh, L, _ = q.shape
    lens_dev = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev())
    table = None if c["table"] is None else torch.from_numpy(np.array(c["table"])).to(dev())
    if not framed:
        return ops.attention_causal(q, K, Vt) if c["kind"] == "causal" else ops.attention_relbias(q, K, Vt, table, lens_dev)
    out = AF.framed(nb * L, nh * 64, dtype=dtype, device=dev())
    assert out.ld > nh * 64
    if c["kind"] == "causal":
        AF.call("pmhip_attention_causal", PM[dtype], q, K, Vt, out, out.ld, nb, nh, L, L_pad)
    else:
        AF.call("pmhip_attention_relbias", PM[dtype], q, K, Vt, out, out.ld, nb, nh, L, L_pad, table, lens_dev)
    out.assert_frame_untouched(f"{c['kind']} {c['family']} L={L} L_pad={L_pad} {dtype}")
    return out.payload()


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("L", W.LS)
@pytest.mark.parametrize("kind", ["relbias", "causal"])
def test_attention_cases(kind, L, dtype):
    worst = {}
    exact_rows = 0
    for fam in W.FAMILIES[kind]:
        c = W.case(kind, fam, L)
        for lens in (W.lens_sets(L) if kind == "relbias" else [None]):
            r = W.reference(c, lens)
            ref, bound = r[NAME[dtype]]
            for L_pad in W.pads(L):
                what = (kind, fam, L, L_pad, lens, NAME[dtype])
                got = launch(c, dtype, L_pad, lens)
                assert got.shape == (W.NB * L, W.NH * 64) and got.dtype == dtype
                ratio = W.worst_ratio(f64(got), ref, bound)
                group = fam.split("_")[0]
                worst[group] = max(worst.get(group, 0.0), ratio)
                assert ratio <= 1.0, (what, ratio)
                assert W.exact_mismatch(f64(got), r) == 0, what                              # bit for bit: small integers
                exact_rows += int(r["rows"].sum())
                bits = AF.bits(got)
                assert torch.equal(AF.bits(launch(c, dtype, L_pad, lens, pad=0.0)), bits), what     # the padding reaches nothing
                assert torch.equal(AF.bits(launch(c, dtype, L_pad, lens)), bits), what              # two launches, the same bits
                if L_pad == W.pads(L)[0]:
                    assert torch.equal(AF.bits(launch(c, dtype, L_pad, lens, framed=True)), bits), what
                    for b in range(W.NB):                                                    # an image alone: its rows of the batch
                        alone = launch(c, dtype, L_pad, None if lens is None else lens[b:b + 1], images=slice(b, b + 1))
                        assert torch.equal(AF.bits(alone), bits[b * L:(b + 1) * L]), (what, b)
    print(f"{kind} L={L} {NAME[dtype]}: worst |error| / bound =", {k: round(v, 3) for k, v in worst.items()})
    assert exact_rows >= L


# ---------------------------------------------------------------------------------------------------------------------------------
# row operators
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("M", W.RMSNORM_MS)
@pytest.mark.parametrize("D", W.RMSNORM_DS)
def test_rmsnorm_at_the_dispatch_and_row_tail_edges(D, M, out_dtype):
    """D on both sides of the NV4 = 4 / 8 / 16 thresholds and at the last float4 of each; M = 4 fills a workgroup, M = 5 starts the next"""
    x, w, eps = W.rmsnorm_case(D, M)
    src = AF.framed(M, D, ld=D, dtype=torch.float32, payload=torch.from_numpy(x).to(dev()), fill="nan")
    out = AF.framed(M, D, ld=D, dtype=out_dtype, device=dev())
    AF.call("pmhip_rmsnorm", src, torch.from_numpy(w).to(dev()), float(eps), out, PM[out_dtype], M, D)
    out.assert_frame_untouched(f"rmsnorm D={D} M={M} {out_dtype}")
    ref = RT.rmsnorm(x, w, eps)
    got = f64(out.payload())
    ratio = float((np.abs(got - ref) / RT.rmsnorm_bound(ref, D, out_dtype == torch.bfloat16)).max())
    print(f"rmsnorm D={D} M={M} {NAME[out_dtype]}: worst |error| / bound = {ratio:.3f}")
    assert np.isfinite(got).all() and ratio <= 1.0, (D, M, ratio)
    assert not got[3].any()                                                                  # the all-zero row
    assert torch.equal(AF.bits(ops.rmsnorm(torch.from_numpy(x).to(dev()), torch.from_numpy(w).to(dev()), eps, out_dtype)), AF.bits(out.payload()))


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("kinds", [(0, 1, 2), (2, 0, 1)], ids=["QKV", "VQK"])
def test_split_heads_with_three_heads_three_images_and_a_short_padding(kinds, dtype):
    s = W.SPLIT_SHAPE
    heads, nb, tokens, tp = s["heads"], s["images"], s["tokens"], s["tokens_pad"]
    u = W.split_case(kinds)
    N = len(kinds) * heads * 64
    src = AF.framed(nb * tokens, N, dtype=torch.float32, payload=torch.from_numpy(u).to(dev()), fill="nan")
    shapes = {0: (nb * heads * tokens, 64), 1: (nb * heads * tp, 64), 2: (nb * heads * 64, tp)}
    outs = [AF.framed(*shapes[kd], ld=shapes[kd][1], dtype=dtype, device=dev(), guard_before=256) for kd in kinds]   # 256 rows of 20: 16-byte aligned
    assert all(o.ptr % 16 == 0 for o in outs)
    before = [AF.bits(o.payload()).clone().cpu() for o in outs]
    AF.call("pmhip_split_heads", PM[dtype], src, src.ld, nb * tokens, heads, tokens, tp, len(kinds), (C.c_int * len(kinds))(*kinds),
            (C.c_void_p * len(kinds))(*[o.ptr for o in outs]), 0.125)
    want = RC.split_heads(u, heads, tokens, len(kinds), 0.125, kinds)
    for o, kd, w, s0 in zip(outs, kinds, want, before):
        o.assert_frame_untouched(f"split_heads part {'QKV'[kd]} {dtype}")
        w = torch.from_numpy(w).to(dtype)
        got = o.payload().cpu()
        if kd == 0:
            assert torch.equal(AF.bits(got.view(nb, heads, tokens, 64)), AF.bits(w))
        elif kd == 1:
            got, s0 = got.view(nb, heads, tp, 64), s0.view(nb, heads, tp, 64)
            assert torch.equal(AF.bits(got[:, :, :tokens]), AF.bits(w))
            assert torch.equal(AF.bits(got[:, :, tokens:]), s0[:, :, tokens:])                # the padding keeps what it held
        else:
            got, s0 = got.view(nb, heads, 64, tp), s0.view(nb, heads, 64, tp)
            assert torch.equal(AF.bits(got[..., :tokens]), AF.bits(w))
            assert torch.equal(AF.bits(got[..., tokens:]), s0[..., tokens:].contiguous())
