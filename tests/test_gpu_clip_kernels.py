"""The three OpenCLIP text-tower operators on the GPU (paintmind_amd/csrc/clipops.hip) against the float64
restatements and the derived element-wise bounds of tests/clip_ref.py: pmhip_attention_causal, pmhip_split_heads, pmhip_gelu.  Every
comparison prints its worst |error| / bound before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import abi_frames as AF
import clip_ref as R
from gpu_common import dev
from paintmind_amd import _lib, ops

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
PM = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}


def f64(t):
    if isinstance(t, np.ndarray):
        return t.astype(np.float64)
    return t.detach().float().cpu().numpy().astype(np.float64)


def within(got, ref, bound, what):
    err = np.abs(f64(got) - ref)
    ratio = float((err / bound).max())
    print(f"{what}: worst |error| / bound = {ratio:.3f}")
    assert np.isfinite(f64(got)).all(), what
    assert ratio <= 1.0, (what, ratio)
    return ratio


def bf16_np(a):
    return torch.from_numpy(np.asarray(a, np.float32)).bfloat16().float().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# causal attention
# ---------------------------------------------------------------------------------------------------------------------------------
B, H = 2, 2
LS = [1, 15, 16, 17, 32, 33, 77]          # the 16-query tile edge and the key-block edges (16 keys in f32, 32 in bf16)
NAN = float("nan")


def pads(L):
    return [ops.round_up(L, 4), ops.round_up(L, 4) + 12]


def layouts(q, k, v, dtype, Lp, poison_from=None, pad=NAN):
    """q, k, v float [B, H, L, 64] -> the kernel's operands: Q [B,H,L,64], K [B,H,Lp,64], V^T [B,H,64,Lp].  The padding [L, Lp) holds
    `pad`; poison_from = j: K rows >= j and V^T columns >= j hold NaN as well"""
    nb, nh, L, _ = q.shape
    K = torch.full((nb, nh, Lp, 64), pad)
    Vt = torch.full((nb, nh, 64, Lp), pad)
    K[:, :, :L] = torch.from_numpy(np.asarray(k, np.float32))
    Vt[:, :, :, :L] = torch.from_numpy(np.asarray(v, np.float32)).transpose(-1, -2)
    if poison_from is not None:
        K[:, :, poison_from:] = NAN
        Vt[:, :, :, poison_from:] = NAN
    Q = torch.from_numpy(np.asarray(q, np.float32))
    return tuple(t.to(device=dev(), dtype=dtype).contiguous() for t in (Q, K, Vt))


def run(q, k, v, dtype, Lp, **kw):
    return ops.attention_causal(*layouts(q, k, v, dtype, Lp, **kw))


@functools.lru_cache(maxsize=None)
def value_case(L, reach):
    """random bf16-representable Q, K, V; reach None: scores of order 1, else Q scaled so that max |s| is about reach"""
    rng = np.random.default_rng(11 * L + (0 if reach is None else 1))
    q, k, v = (bf16_np(rng.standard_normal((B, H, L, 64))) for _ in range(3))
    if reach is None:
        q = bf16_np(q / 8)
    else:
        q = bf16_np(q * (reach / np.abs(np.tril(q.astype(np.float64) @ k.astype(np.float64).transpose(0, 1, 3, 2))).max()))
    out = {None: (q, k, v)}
    for name, bf in (("f32", False), ("bf16", True)):
        out[name] = R.attention_causal(q, k, v, bf)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("reach", [None, 100.0])
@pytest.mark.parametrize("wide", [False, True], ids=["pad4", "pad_wide"])
@pytest.mark.parametrize("L", LS)
def test_value_probe_is_within_the_derived_bound(L, wide, reach, dtype):
    case = value_case(L, reach)
    q, k, v = case[None]
    ref, bound = case["bf16" if dtype == torch.bfloat16 else "f32"]
    Lp = pads(L)[wide]
    if reach is not None and L > 1:
        s = np.tril(q.astype(np.float64) @ k.astype(np.float64).transpose(0, 1, 3, 2))
        assert np.abs(s).max() > 88                                                    # exp(s) without the maximum overflows float32
    got = run(q, k, v, dtype, Lp)
    assert got.shape == (B * L, H * 64) and got.dtype == dtype
    within(got, ref.reshape(B * L, -1), bound.reshape(B * L, -1), f"value probe L={L} L_pad={Lp} reach={reach} {dtype}")
    assert torch.equal(AF.bits(run(q, k, v, dtype, Lp)), AF.bits(got))                  # two launches, the same bits
    assert torch.equal(AF.bits(run(q, k, v, dtype, Lp, pad=0.0)), AF.bits(got))         # the padding reaches nothing
    for b in range(B):                                                                  # an image alone: its rows of the batch
        alone = run(q[b:b + 1], k[b:b + 1], v[b:b + 1], dtype, Lp)
        assert torch.equal(AF.bits(alone), AF.bits(got[b * L:(b + 1) * L]))


def index_case(L):
    """K[k] = 8 e_k, Q[q] = 8 e_t(q): the one matching key scores 64, every other 0; V bf16-representable with 1 <= |v| < 2.
    t differs per head: a stride walk and the mirror image, so about half of the queries point above the diagonal"""
    rng = np.random.default_rng(L)
    maps = [(7 * np.arange(L) + 3) % L, L - 1 - np.arange(L)]
    q = np.zeros((B, H, L, 64))
    k = np.zeros((B, H, L, 64))
    k[:, :, np.arange(L), np.arange(L)] = 8.0
    for h, tq in enumerate(maps):
        q[:, h, np.arange(L), tq] = 8.0
    v = (1.0 + rng.integers(0, 128, (B, H, L, 64)) / 128.0) * rng.choice([-1.0, 1.0], (B, H, L, 64))
    return q, k, v, maps


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [17, 33])
def test_index_probe_is_exact_below_the_diagonal_and_a_mean_above(L, dtype):
    q, k, v, maps = index_case(L)
    assert np.array_equal(bf16_np(v), v) and np.abs(v).min() >= 1 and np.abs(v).max() < 2
    ref, bound = R.attention_causal(q, k, v, dtype == torch.bfloat16)
    for Lp in pads(L):
        got = f64(run(q, k, v, dtype, Lp))
        within(got, ref.reshape(B * L, -1), bound.reshape(B * L, -1), f"index probe L={L} L_pad={Lp} {dtype}")
        got = got.reshape(B, L, H, 64)
        hits = above = 0
        for h, tq in enumerate(maps):
            for r in range(L):
                if tq[r] <= r:
                    hits += 1
                    assert np.array_equal(got[:, r, h], v[:, h, tq[r]]), (L, h, r)      # bit for bit
                else:
                    above += 1
                    mean = v[:, h, :r + 1].mean(1)
                    assert np.all(np.abs(got[:, r, h] - mean) <= bound.reshape(B, L, H, 64)[:, r, h]), (L, h, r)
        assert hits > L // 4 and above > L // 4


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [15, 16, 17, 32, 33, 77])
def test_nothing_behind_the_diagonal_reaches_a_row(L, dtype):
    q, k, v = value_case(L, None)[None]
    Lp = pads(L)[1]
    clean = run(q, k, v, dtype, Lp, pad=0.0)
    for j in sorted({j for j in (1, 16, 17, 32, L - 1) if 1 <= j < L}):
        got = run(q, k, v, dtype, Lp, poison_from=j)
        rows = got.view(B, L, H * 64)[:, :j]
        assert torch.isfinite(rows.float()).all(), (L, j)
        assert torch.equal(AF.bits(rows), AF.bits(clean.view(B, L, H * 64)[:, :j])), (L, j)
        assert torch.isnan(got.view(B, L, H * 64)[:, j:].float()).all(), (L, j)         # and the rows that may see the NaN do


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [17, 77])
def test_out_is_written_in_exactly_its_extent(L, dtype):
    q, k, v = value_case(L, None)[None]
    Q, K, Vt = layouts(q, k, v, dtype, pads(L)[0])
    out = AF.framed(B * L, H * 64, dtype=dtype, device=dev())
    assert out.ld > H * 64
    AF.call("pmhip_attention_causal", PM[dtype], Q, K, Vt, out, out.ld, B, H, L, K.shape[2])
    out.assert_frame_untouched(f"attention_causal L={L} {dtype}")
    assert torch.equal(AF.bits(out.payload()), AF.bits(ops.attention_causal(Q, K, Vt)))


def test_entry_refusals_name_their_argument():
    q, k, v = value_case(17, None)[None]
    Q, K, Vt = layouts(q, k, v, torch.float32, 20)
    out = torch.empty(B * 17, H * 64 + 2, device=dev())
    for args, message in [((PM[torch.float32], Q, K, Vt, out, H * 64 + 2, B, H, 17, 20), "ldo=130"),
                          ((PM[torch.float32], Q, K, Vt, out, H * 64, B, H, 17, 18), "L_pad=18"),
                          ((PM[torch.float32], Q, K, Vt, out, H * 64, B, H, 17, 16), "L_pad=16"),
                          ((PM[torch.float32], Q, K, Vt, out, H * 64, B, H, 0, 20), "L=0"),
                          ((7, Q, K, Vt, out, H * 64, B, H, 17, 20), "dtype"),
                          ((PM[torch.float32], Q, None, Vt, out, H * 64, B, H, 17, 20), "null"),
                          ((PM[torch.float32], Q, K.view(-1)[2:], Vt, out, H * 64, B, H, 17, 20), "aligned")]:
        with pytest.raises(_lib.PmhipError, match=message):
            AF.call("pmhip_attention_causal", *args)
    with pytest.raises(ValueError, match="dim_head"):
        ops.attention_causal(Q[..., :32].contiguous(), K, Vt)


# ---------------------------------------------------------------------------------------------------------------------------------
# head split
# ---------------------------------------------------------------------------------------------------------------------------------
HEADS = 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("q_scale", [1.0, 0.125])
@pytest.mark.parametrize("kinds", [(0,), (1,), (2,), (0, 1, 2), (2, 0, 1), (1, 2, 0)], ids=lambda k: "".join("QKV"[i] for i in k))
@pytest.mark.parametrize("tokens, tokens_pad", [(5, 8), (77, 80)])
def test_split_heads_is_exact_and_leaves_padding_and_guards_alone(tokens, tokens_pad, kinds, q_scale, dtype):
    nb, N = 2, len(kinds) * HEADS * 64
    rng = np.random.default_rng(tokens + len(kinds))
    u = (rng.standard_normal((nb * tokens, N)) * np.exp(3 * rng.standard_normal((nb * tokens, 1)))).astype(np.float32)
    src = AF.framed(nb * tokens, N, dtype=torch.float32, payload=torch.from_numpy(u).to(dev()), fill="nan")
    assert src.ld > N
    shapes = {0: (nb * HEADS * tokens, 64), 1: (nb * HEADS * tokens_pad, 64), 2: (nb * HEADS * 64, tokens_pad)}
    outs = [AF.framed(*shapes[kd], ld=shapes[kd][1], dtype=dtype, device=dev()) for kd in kinds]
    sentinel = [AF.bits(o.payload()).clone() for o in outs]
    AF.call("pmhip_split_heads", PM[dtype], src, src.ld, nb * tokens, HEADS, tokens, tokens_pad, len(kinds), (C.c_int * len(kinds))(*kinds),
            (C.c_void_p * len(kinds))(*[o.ptr for o in outs]), q_scale)
    want = R.split_heads(u, HEADS, tokens, len(kinds), q_scale, kinds)
    for o, kd, w, s in zip(outs, kinds, want, sentinel):
        o.assert_frame_untouched(f"split_heads part {'QKV'[kd]} tokens={tokens} {dtype}")
        w = torch.from_numpy(w).to(dtype)                                               # bf16: round to nearest even, once
        got = o.payload().cpu()
        s = s.cpu()
        if kd == 0:
            assert torch.equal(AF.bits(got.view(nb, HEADS, tokens, 64)), AF.bits(w))
        elif kd == 1:
            got, s = got.view(nb, HEADS, tokens_pad, 64), s.view(nb, HEADS, tokens_pad, 64)
            assert torch.equal(AF.bits(got[:, :, :tokens]), AF.bits(w))
            assert torch.equal(AF.bits(got[:, :, tokens:]), s[:, :, tokens:])            # the padding keeps what it held
        else:
            got, s = got.view(nb, HEADS, 64, tokens_pad), s.view(nb, HEADS, 64, tokens_pad)
            assert torch.equal(AF.bits(got[..., :tokens]), AF.bits(w))
            assert torch.equal(AF.bits(got[..., tokens:]), s[..., tokens:].contiguous())
    # the wrapper on a contiguous tensor: the same values, the padding zero
    parts = ops.split_heads(torch.from_numpy(u).to(dev()), HEADS, tokens, list(kinds), q_scale=q_scale, dtype=dtype)
    for part, kd, w in zip(parts, kinds, want):
        w = torch.from_numpy(w).to(dtype)
        part = part.cpu()
        if kd == 0:
            assert torch.equal(AF.bits(part), AF.bits(w))
        elif kd == 1:
            assert part.shape[2] == ops.round_up(tokens, 64) and torch.equal(AF.bits(part[:, :, :tokens]), AF.bits(w)) and not part[:, :, tokens:].any()
        else:
            assert torch.equal(AF.bits(part[..., :tokens]), AF.bits(w)) and not part[..., tokens:].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# the GELUs
# ---------------------------------------------------------------------------------------------------------------------------------
SPECIAL = np.array([0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0, 6.0, -6.0, 40.0, -40.0, 1e30, -1e30, 3e38, -3e38, 2.0 ** -120, -2.0 ** -120,
                    13.5, -13.5, 9.0, -9.0], np.float32)


@pytest.mark.parametrize("out_dtype", DTYPES)
@pytest.mark.parametrize("kind", ["erf", "quick"])
@pytest.mark.parametrize("F", [4, 260])
def test_gelu_is_within_the_derived_bound_inside_its_frame(F, kind, out_dtype):
    M = 3
    rng = np.random.default_rng(F)
    u = (3.0 * rng.standard_normal((M, F))).astype(np.float32)
    count = min(SPECIAL.size, M * F)
    u.reshape(-1)[:count] = SPECIAL[:count]                                             # F = 4: 0, +-tiny, +-1, +-6, +-40, +-1e30
    src = AF.framed(M, F, dtype=torch.float32, payload=torch.from_numpy(u).to(dev()), fill="nan")
    out = AF.framed(M, F, dtype=out_dtype, device=dev())
    assert src.ld > F and out.ld > F
    AF.call("pmhip_gelu", src, src.ld, out, out.ld, PM[out_dtype], M, F, ops.GELU_KINDS[kind])
    out.assert_frame_untouched(f"gelu {kind} F={F} {out_dtype}")
    ref = R.gelu(u, kind)
    assert np.isfinite(ref).all()
    within(out.payload(), ref, R.gelu_bound(u, kind, out_dtype == torch.bfloat16), f"gelu {kind} F={F} {out_dtype}")
    assert torch.equal(AF.bits(ops.gelu(torch.from_numpy(u).to(dev()), out_dtype, kind)), AF.bits(out.payload()))


def test_gelu_refuses_an_unknown_kind():
    u = torch.zeros(3, 8, device=dev())
    with pytest.raises(ValueError, match="kind"):
        ops.gelu(u, torch.float32, "tanh")
    with pytest.raises(_lib.PmhipError, match="kind 2"):
        AF.call("pmhip_gelu", u, 8, torch.empty_like(u), 8, PM[torch.float32], 3, 8, 2)
