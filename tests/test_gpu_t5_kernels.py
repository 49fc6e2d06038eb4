"""The three Flan-T5 operators on the GPU (paintmind_amd/csrc/t5ops.hip) against the float64 restatements and the
derived element-wise bounds of tests/t5_ref.py: pmhip_rmsnorm, pmhip_geglu, pmhip_attention_relbias.  Every comparison prints its worst
|error| / bound before it asserts."""
import functools

import numpy as np
import pytest
import torch

import abi_frames as AF
import t5_ref as R
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


# ---------------------------------------------------------------------------------------------------------------------------------
# rmsnorm
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", DTYPES)
@pytest.mark.parametrize("M", [1, 3, 155])
@pytest.mark.parametrize("D", [4, 64, 100, 2048, 4096])
def test_rmsnorm_is_within_the_derived_bound(D, M, out_dtype):
    rng = np.random.default_rng(D * 1000 + M)
    scale = np.array([1.0, 2.0 ** 20, 2.0 ** -20])[np.arange(M) % 3][:, None]            # neighbouring rows differ by 2^+-20
    x = (rng.standard_normal((M, D)) * scale).astype(np.float32)
    if M > 1:
        x[M // 2] = 0.0                                                                 # an all-zero row gives 0, not NaN
    w = (1.0 + 0.5 * rng.standard_normal(D)).astype(np.float32)
    got = ops.rmsnorm(torch.from_numpy(x).to(dev()), torch.from_numpy(w).to(dev()), 1e-6, out_dtype)
    assert got.dtype == out_dtype and got.shape == (M, D)
    ref = R.rmsnorm(x, w, 1e-6)
    within(got, ref, R.rmsnorm_bound(ref, D, out_dtype == torch.bfloat16), f"rmsnorm D={D} M={M} {out_dtype}")
    if M > 1:
        assert not f64(got)[M // 2].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# geglu
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", DTYPES)
@pytest.mark.parametrize("M", [1, 155])
@pytest.mark.parametrize("F", [64, 192, 2816])
def test_geglu_is_within_the_derived_bound_inside_its_frame(F, M, out_dtype):
    rng = np.random.default_rng(F + M)
    u = (3.0 * rng.standard_normal((M, 2 * F))).astype(np.float32)
    special = np.array([30.0, -30.0, 1e13, -1e13, 0.0, -0.0, 6.0, -6.0, 12.0, -12.0], np.float32)
    u[0, :special.size] = special                                                       # gates: saturated, overflowing x^3, zero
    u[0, F + 20:F + 20 + special.size] = special                                        # and the same values as the linear factor
    u[-1, F - special.size:F] = special[::-1]
    src = AF.framed(M, 2 * F, dtype=torch.float32, payload=torch.from_numpy(u).to(dev()), fill="nan")
    out = AF.framed(M, F, dtype=out_dtype, device=dev())
    assert src.ld > 2 * F and out.ld > F
    AF.call("pmhip_geglu", src, src.ld, out, out.ld, PM[out_dtype], M, F)
    out.assert_frame_untouched(f"geglu F={F} M={M} {out_dtype}")
    ref = R.geglu(u, F)
    assert np.isfinite(ref).all()
    within(out.payload(), ref, R.geglu_bound(u, F, out_dtype == torch.bfloat16), f"geglu F={F} M={M} {out_dtype}")
    # the wrapper on contiguous tensors gives the same bits
    assert torch.equal(AF.bits(ops.geglu(torch.from_numpy(u).to(dev()), out_dtype)), AF.bits(out.payload()))


# ---------------------------------------------------------------------------------------------------------------------------------
# attention with the relative-position bias
# ---------------------------------------------------------------------------------------------------------------------------------
B, H = 2, 3
LS = [1, 2, 15, 16, 17, 63, 64, 65, 77, 128, 129, 512]


def bf16_np(a):
    return torch.from_numpy(np.asarray(a, np.float32)).bfloat16().float().numpy()


def layouts(q, k, v, dtype, lens=None, poison=True):
    """q, k, v float [B, H, L, 64] -> the kernel's operands: Q [B,H,L,64], K [B,H,Lp,64], V^T [B,H,64,Lp]; K rows and V^T columns at
    [L, Lp) and behind lens[b] (clamped as the kernel clamps) hold NaN (poison) or zeros"""
    nb, nh, L, _ = q.shape
    Lp = ops.round_up(L, 64)
    fill = float("nan") if poison else 0.0
    K = torch.full((nb, nh, Lp, 64), fill)
    Vt = torch.full((nb, nh, 64, Lp), fill)
    for b in range(nb):
        n = L if lens is None else min(max(int(lens[b]), 1), L)
        K[b, :, :n] = torch.from_numpy(np.asarray(k[b, :, :n], np.float32))
        Vt[b, :, :, :n] = torch.from_numpy(np.asarray(v[b, :, :n], np.float32)).transpose(-1, -2)
    Q = torch.from_numpy(np.asarray(q, np.float32))
    return tuple(t.to(device=dev(), dtype=dtype).contiguous() for t in (Q, K, Vt))


def run(q, k, v, table, dtype, lens=None, poison=True):
    Q, K, Vt = layouts(q, k, v, dtype, lens, poison)
    lens_dev = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev())
    return ops.attention_relbias(Q, K, Vt, torch.from_numpy(np.asarray(table, np.float32)).to(dev()), lens_dev)


def index_case(L, deltas, nb=B):
    """Q = 0, table[h] = +64 at delta deltas[h] and 0 elsewhere, V small integers >= 1 that encode (key, image, head)"""
    nh = len(deltas)
    q = np.zeros((nb, nh, L, 64))
    k = np.random.default_rng(L).standard_normal((nb, nh, L, 64))                       # multiplied by Q = 0
    key = np.arange(L)
    v = np.empty((nb, nh, L, 64))
    v[..., 0::2] = (key % 128 + 1)[None, None, :, None]
    v[..., 1::2] = (key // 128 + 1)[None, None, :, None] + (np.arange(nb)[:, None] * nh + np.arange(nh)[None, :])[:, :, None, None]
    table = np.zeros((nh, 2 * L - 1))
    for h, d in enumerate(deltas):
        table[h, d + L - 1] = 64.0
    return q, bf16_np(k), v, table


def check_index(L, deltas, dtype, lens):
    q, k, v, table = index_case(L, deltas)
    got = f64(run(q, k, v, table, dtype, lens)).reshape(B, L, len(deltas), 64)
    ref, bound = R.attention(q, k, v, table, lens, dtype == torch.bfloat16)
    within(got.reshape(B, L, -1), ref, bound, f"index probe L={L} deltas={deltas} {dtype}")
    hits = 0
    for b in range(B):
        n = L if lens is None else min(max(int(lens[b]), 1), L)
        for h, d in enumerate(deltas):
            rows = [r for r in range(L) if 0 <= r + d < n]
            hits += len(rows)
            want = v[b, h, [r + d for r in rows]]
            assert np.array_equal(got[b, rows, h], want), (L, b, h, d)                  # bit for bit: the values are small integers
    return hits


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", LS)
def test_index_probe_is_exact(L, dtype):
    deltas = (0, min(L - 1, max(L // 3, 1)), -min(L - 1, max(L // 2, 1)))
    assert check_index(L, deltas, dtype, None) > 0
    assert check_index(L, deltas, dtype, [L, max(1, L // 2)]) > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_index_probe_sweeps_every_delta_at_17(dtype):
    for d0 in range(-16, 17, 3):
        check_index(17, (d0, d0 + 1, d0 + 2), dtype, None)


@functools.lru_cache(maxsize=None)
def value_case(L, reach):
    """random bf16-representable Q, K, V and a random table; reach None: scores of order 1, else Q scaled so that max |s| is about reach"""
    rng = np.random.default_rng(7 * L + (0 if reach is None else 1))
    q, k, v = (bf16_np(rng.standard_normal((B, H, L, 64))) for _ in range(3))
    table = rng.standard_normal((H, 2 * L - 1)).astype(np.float32).astype(np.float64)
    if reach is None:
        q = bf16_np(q / 8)
    else:
        q = bf16_np(q * (reach / np.abs(q.astype(np.float64) @ k.astype(np.float64).transpose(0, 1, 3, 2)).max()))
    out = {None: (q, k, v, table)}
    for name, bf in (("f32", False), ("bf16", True)):
        out[name] = R.attention(q, k, v, table, None, bf)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("reach", [None, 500.0])
@pytest.mark.parametrize("L", LS)
def test_value_probe_is_within_the_derived_bound(L, reach, dtype):
    case = value_case(L, reach)
    q, k, v, table = case[None]
    ref, bound = case["bf16" if dtype == torch.bfloat16 else "f32"]
    if reach is not None and L > 1:
        s = q.astype(np.float64) @ k.astype(np.float64).transpose(0, 1, 3, 2)
        assert np.abs(s).max() > 400                                                   # exp(s) without the maximum overflows float32
    got = run(q, k, v, table, dtype)
    within(got, ref.reshape(B * L, -1), bound.reshape(B * L, -1), f"value probe L={L} reach={reach} {dtype}")
    assert torch.equal(AF.bits(run(q, k, v, table, dtype)), AF.bits(got))               # two launches, the same bits
    for b in range(B):                                                                  # an image alone: its rows of the batch
        alone = run(q[b:b + 1], k[b:b + 1], v[b:b + 1], table, dtype)
        assert torch.equal(AF.bits(alone), AF.bits(got[b * L:(b + 1) * L]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", LS)
def test_kv_lens_clamp_and_keep_poison_out(L, dtype):
    q, k, v, table = value_case(L, None)[None]
    lens = [1, L - 1, L, 0, L + 5]                                                      # 0 clamps to 1, L + 5 to L
    rep = [0, 1, 0, 1, 0]
    q5, k5, v5 = q[rep], k[rep], v[rep]
    got = run(q5, k5, v5, table, dtype, lens, poison=True)
    clean = run(q5, k5, v5, table, dtype, lens, poison=False)
    assert torch.isfinite(got.float()).all() and torch.equal(AF.bits(got), AF.bits(clean))
    ref, bound = R.attention(q5, k5, v5, table, lens, dtype == torch.bfloat16)
    within(got, ref.reshape(5 * L, -1), bound.reshape(5 * L, -1), f"kv_lens L={L} {dtype}")
    # kv_lens == L everywhere is the call without kv_lens
    full = run(q, k, v, table, dtype, [L, L])
    assert torch.equal(AF.bits(full), AF.bits(run(q, k, v, table, dtype)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [1, 17, 77, 129])
def test_out_is_written_in_exactly_its_extent(L, dtype):
    q, k, v, table = value_case(L, None)[None]
    Q, K, Vt = layouts(q, k, v, dtype)
    out = AF.framed(B * L, H * 64, dtype=dtype, device=dev())
    assert out.ld > H * 64
    AF.call("pmhip_attention_relbias", PM[dtype], Q, K, Vt, out, out.ld, B, H, L, K.shape[2],
            torch.from_numpy(table.astype(np.float32)).to(dev()), None)
    out.assert_frame_untouched(f"attention_relbias L={L} {dtype}")
    assert torch.equal(AF.bits(out.payload()), AF.bits(run(q, k, v, table, dtype)))
