"""rowops.hip and loss.hip held to the row probes (tests/rowop_probes.py; tests/test_rowop_probes_cpu.py shows what each case rejects).

Every LayerNorm-group entry is compared element by element with a float64 reference built from exactly what the kernel is given,
inside the bound derived in the probe module; pmhip_ln_coef_parts additionally with the bits of its restatement around the hardware's
square root; pmhip_masked_ce row by row and on the scalar; pmhip_random_mask and the row utilities exactly.  The shapes are the
smallest that reach each arm: the register-resident widths of layernorm_kernel (512, 768, 1024) and the generic one on both sides of
every multiple of 256, the ragged last group of hilo_rows_kernel, the clamped rows of ln_coef_kernel's four-rows-per-wave tail, a
partly live second workgroup of ln_coef_parts_kernel, the four widths of masked_ce_rows_kernel at both sides of their thresholds, the
reduce loop at 1024 / 1025 rows, and random_mask up to the 128 KiB of dynamic LDS its entry point admits.  The worst ratio of
every entry is printed (pytest -s).
"""
import numpy as np
import pytest
import torch

import rowop_probes as P
from abi_frames import bits, call, framed
from gpu_common import dev, n, t
from paintmind_amd import _lib, ops

pytestmark = pytest.mark.gpu

F = np.float32
INT64_MIN = -2 ** 63
WORST = {}


def note(entry, r):
    WORST[entry] = max(WORST.get(entry, 0.0), r)


def teardown_module(module):
    print("\nworst |error| / bound per entry on the GPU:")
    for k in sorted(WORST):
        print(f"    {k:24s} {WORST[k]:.3f}")


def tb(a):
    """float32 array of bf16 values -> bf16 tensor (exact)"""
    return t(a, torch.bfloat16)


def pair(hi, lo):
    return n(hi).astype(np.float64) + n(lo).astype(np.float64)


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 64, 252, 256, 260, 512, 768, 1024, 1028, 1280, 2052])
def test_layernorm(D):
    for M in (1, 13):
        fam = P.ln_family(M, D)
        x, ga, be = fam["x"], fam["gamma"], fam["beta"]
        xt, gt, bt = t(x), t(ga), t(be)
        for eps in P.EPS_VALUES:
            want = P.ln_ref(x, ga, be, eps)
            for out, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
                got = n(ops.layernorm(xt, gt, bt, eps, dt))
                note(f"layernorm {out}", P.assert_within(got, want, P.ln_bound(x, ga, be, eps, out), f"layernorm D={D} M={M} eps={eps} {out}",
                                                         fam["kinds"]))


@pytest.mark.parametrize("D", [4, 72, 252, 256, 260, 768, 1020, 1024])
def test_hilo_row_operators(D):
    fam = P.hilo_family(13, D)
    hi, lo, ga, be, kinds = fam["hi"], fam["lo"], fam["gamma"], fam["beta"], fam["kinds"]
    ht, lt, gt, bt, xt = tb(hi), tb(lo), t(ga), t(be), t(fam["x"])
    x64 = P.hilo_value(hi, lo)
    e_in = P.hilo_input_error(hi, lo)
    for eps in P.EPS_VALUES:
        want = P.ln_ref(x64, ga, be, eps)
        for out, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            got = n(ops.layernorm_hilo(ht, lt, gt, bt, eps, dt))
            note(f"layernorm_hilo {out}", P.assert_within(got, want, P.ln_bound(x64, ga, be, eps, out, e_in),
                                                          f"layernorm_hilo D={D} eps={eps} {out}", kinds))
        oh, ol = ops.layernorm_to_hilo(xt, gt, bt, eps)
        x = fam["x"]
        note("layernorm_to_hilo", P.assert_within(pair(oh, ol), P.ln_ref(x, ga, be, eps), P.ln_bound(x, ga, be, eps, "hilo"),
                                                  f"layernorm_to_hilo D={D} eps={eps}", kinds))
    # split: hi is torch's cast, bit for bit; the pair is x to 2^-17 on rows that mix 1e-6 and 1e4
    xm = P.mixed_magnitudes(13, D)
    xmt = t(xm)
    sh, sl = ops.split_hilo(xmt)
    assert torch.equal(bits(sh), bits(xmt.to(torch.bfloat16))), f"split_hilo D={D}: hi is not torch's bf16 cast"
    note("split_hilo", P.assert_within(pair(sh, sl), xm, P.split_bound(xm), f"split_hilo D={D}"))
    mh, ml = n(sh), n(sl)
    note("join_hilo", P.assert_within(n(ops.join_hilo(sh, sl)), P.hilo_value(mh, ml), P.join_bound(mh, ml), f"join_hilo D={D}"))
    ml = np.roll(ml, 1, axis=1)                                 # lo planes of the neighbouring column: hi + lo has to be rounded
    note("join_hilo", P.assert_within(n(ops.join_hilo(sh, tb(ml))), P.hilo_value(mh, ml), P.join_bound(mh, ml), f"join_hilo D={D}, foreign lo"))
    # unshift: the centred pair plus shift[row], against float64 hi + lo + shift
    c = P.hilo_family(13, D, centred=True)
    uh, ul = ops.unshift_hilo(tb(c["hi"]), tb(c["lo"]), t(c["shift"]))
    note("unshift_hilo", P.assert_within(pair(uh, ul), P.hilo_value(c["hi"], c["lo"], c["shift"]), P.unshift_bound(c["hi"], c["lo"], c["shift"]),
                                         f"unshift_hilo D={D}", kinds))


@pytest.mark.parametrize("D", [1028, 6])
def test_hilo_row_operators_refuse_other_widths(D):
    x = torch.zeros(2, D, device=dev())
    h, v = x.to(torch.bfloat16), torch.zeros(D, device=dev())
    match = rf"hi/lo row operator: D={D} must be a multiple of 4, <= 1024"
    for f in (lambda: ops.layernorm_hilo(h, h, v, v, 1e-5, torch.float32), lambda: ops.layernorm_hilo(h, h, v, v, 1e-5, torch.bfloat16),
              lambda: ops.layernorm_to_hilo(x, v, v), lambda: ops.split_hilo(x), lambda: ops.join_hilo(h, h),
              lambda: ops.unshift_hilo(h, h, torch.zeros(2, device=dev()))):
        with pytest.raises(_lib.PmhipError, match=match):
            f()


@pytest.mark.parametrize("D", [8, 72, 248, 256, 264, 520, 1016, 1024])
def test_ln_coef(D):
    for M in (1, 13, 17):                                      # 13, 17: the last wave's four rows are clamped to row M - 1
        hi = P.hilo_family(M, D)["hi"]
        ht = tb(hi)
        for eps in P.EPS_VALUES:
            note("ln_coef", P.assert_within(n(ops.ln_coef(ht, eps)), P.coef_ref(hi, eps), P.coef_bound(hi, eps), f"ln_coef D={D} M={M} eps={eps}"))


def test_ln_coef_refuses_other_widths():
    with pytest.raises(_lib.PmhipError, match=r"ln_coef: D=68 must be a multiple of 8, <= 1024"):
        ops.ln_coef(torch.zeros(2, 68, device=dev(), dtype=torch.bfloat16))


@pytest.mark.parametrize("nparts", range(1, 17))
def test_ln_coef_parts(nparts):
    for M in (1, 13, 33):                                      # 33 rows: 8 lanes each, the second workgroup has one live row
        parts = P.make_parts(P.ln_family(M, 64 * nparts)["x"], nparts)
        pt = t(parts)
        for eps in P.EPS_VALUES:
            got = n(ops.ln_coef_parts(pt, eps))
            want, bound = P.parts_ref(parts, eps)
            note("ln_coef_parts", P.assert_within(got, want, bound, f"ln_coef_parts nparts={nparts} M={M} eps={eps}"))
            why = P.parts_bits_match(got, parts, eps)
            assert why is None, f"ln_coef_parts nparts={nparts} M={M} eps={eps}: {why}"


def test_ln_coef_parts_refuses_17_parts():
    with pytest.raises(_lib.PmhipError, match=r"ln_coef_parts: nparts=17 must be in \[1,16\]"):
        ops.ln_coef_parts(torch.zeros(2, 17, 2, device=dev()))


# ---- masked_ce -------------------------------------------------------------------------------------------------------------------
def _check_ce(fam, eps, what, framed_logits=False):
    logits, labels, mask = fam["logits"], fam["labels"], fam["mask"]
    M, V = logits.shape
    rows, drow, loss, dloss = P.ce_ref(logits, labels, mask, eps)
    if framed_logits:                                          # a leading dimension of V + 72, NaN in the gap and around
        fx = framed(M, V, ld=V + 72, payload=t(logits), fill="nan")
        got_rows = torch.empty(M, device=dev())
        got_loss = torch.empty(1, device=dev())
        call("pmhip_masked_ce", fx, fx.ld, t(labels), t(mask), float(eps), got_rows, got_loss, M, V)
        torch.cuda.synchronize()
    else:
        got_loss, got_rows = ops.masked_ce(t(logits), t(labels), t(mask), eps)
    note("masked_ce rows", P.assert_within(n(got_rows), rows, drow, f"{what}: rows"))
    note("masked_ce loss", P.assert_within(n(got_loss)[0], loss, dloss, f"{what}: loss"))


@pytest.mark.parametrize("V", [4, 64, 256, 260, 1024, 1028, 8192, 8196, 16384])
def test_masked_ce(V):
    for kind in P.CE_FAMILIES:
        fam = P.ce_family(kind, 5, V)
        for eps in (0.0, 0.1, 1.0):
            _check_ce(fam, eps, f"masked_ce {kind} V={V} eps={eps}")
    _check_ce(P.ce_family("mixed", 5, V), 0.1, f"masked_ce mixed V={V} ldl={V + 72}", framed_logits=True)


@pytest.mark.parametrize("M", [1024, 1025, 2500])
def test_masked_ce_reduce_rows(M):
    _check_ce(P.ce_family("mixed", M, 64), 0.1, f"masked_ce M={M}")


@pytest.mark.parametrize("V,match", [(16388, r"V=16388 > 16384 unsupported"), (6, r"masked_ce: bad shape M=2 V=6")])
def test_masked_ce_refuses_other_widths(V, match):
    with pytest.raises(_lib.PmhipError, match=match):
        ops.masked_ce(torch.zeros(2, V, device=dev()), torch.zeros(2, device=dev(), dtype=torch.int64), torch.ones(2, device=dev()), 0.1)


# ---- random_mask -----------------------------------------------------------------------------------------------------------------
def _check_mask(B, N, E, kind, keeps):
    fam = P.mask_family(B, N, E, kind)
    zt, nt, tt = t(fam["z"]), t(fam["noise"]), t(fam["mask_token"])
    for keep in keeps:
        x, mask = ops.random_mask(zt, nt, tt, keep)
        xr, mr = P.mask_ref(fam["z"], fam["noise"], fam["mask_token"], keep)
        what = f"random_mask N={N} E={E} {kind} len_keep={keep}"
        assert np.array_equal(n(mask), mr), f"{what}: mask differs at {np.argwhere(n(mask) != mr)[:3].tolist()}"
        assert np.array_equal(n(x), xr), f"{what}: x differs at {np.argwhere(n(x) != xr)[:3].tolist()}"


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1023, 1024, 1025, 8192])
def test_random_mask(N):
    for kind in P.NOISE_KINDS:
        for E in (1, 4, 5):
            _check_mask(2, N, E, kind, sorted({0, 1, N - 1, N}))


@pytest.mark.parametrize("N", [8256, 16384])
def test_random_mask_beyond_64_kib_of_lds(N):
    """2 N floats of dynamic LDS: 64.5 KiB and 128 KiB of a CU's 160 KiB.  The runtime accepts the launch as it is (no
    hipFuncSetAttribute in the entry point); N = 16384 stays the entry point's limit"""
    for kind in ("uniform", "heavy_ties"):
        _check_mask(1, N, 4, kind, (0, 1, N - 1, N))


def test_random_mask_limit_is_16384():
    with pytest.raises(_lib.PmhipError, match=r"random_mask: N=16385 > 16384"):
        ops.random_mask(torch.zeros(1, 16385, 4, device=dev()), torch.zeros(1, 16385, device=dev()), torch.zeros(4, device=dev()), 5)


# ---- row utilities: exact ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,Pp", [(16, 40, 8), (16, 48, 16)])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_patchify_rectangular(H, W, Pp, C):
    B = 2
    img = np.random.default_rng(H + W + C).standard_normal((B, C, H, W)).astype(F)
    want = P.patchify_ref(img, Pp)
    rows, K = want.shape
    for dt in (torch.float32, torch.bfloat16):
        out = framed(rows, K, ld=K, dtype=dt, device=dev())
        call("pmhip_patchify", t(img), out, ops.pm_dtype(dt), B, C, H, W, Pp)
        torch.cuda.synchronize()
        out.assert_frame_untouched(f"patchify {H}x{W} P={Pp} C={C} {dt}")
        ref = t(want).to(dt)
        assert torch.equal(bits(out.payload()), bits(ref)), f"patchify {H}x{W} P={Pp} C={C} {dt}"


@pytest.mark.parametrize("H,W,Pp", [(16, 40, 8), (16, 48, 16), (8, 20, 4)])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_unpatchify_clamp_rectangular(H, W, Pp, C):
    B = 2
    rows, K = B * (H // Pp) * (W // Pp), C * Pp * Pp
    y = np.random.default_rng(3 * H + W + C).uniform(-0.5, 1.0, (rows, K)).astype(F)
    flat = y.reshape(-1)
    flat[::11] = 0.5                                            # exactly on the upper bound
    flat[3::11] = 0.0                                           # exactly on the lower bound
    flat[5::13] = np.nan                                        # a NaN pixel stays NaN (torch.clamp)
    flat[7::17] = np.inf
    flat[8::17] = -np.inf
    for lo, hi in ((0.0, 0.5), (-np.inf, np.inf)):
        img = framed(B * C * H, W, ld=W, device=dev())
        call("pmhip_unpatchify_clamp", t(y), img, B, C, H, W, Pp, float(lo), float(hi))
        torch.cuda.synchronize()
        img.assert_frame_untouched(f"unpatchify {H}x{W} P={Pp} C={C}")
        got = n(img.payload()).reshape(B, C, H, W)
        want = P.unpatchify_ref(y, B, C, H, W, Pp, lo, hi)
        assert np.isnan(want).sum() == np.isnan(y).sum() > 0
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"unpatchify {H}x{W} P={Pp} C={C} [{lo}, {hi}]: a NaN pixel did not stay NaN"
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"unpatchify {H}x{W} P={Pp} C={C} [{lo}, {hi}]"


@pytest.mark.parametrize("K", [1, 3, 5, 30, 33, 63])
def test_convert_pad_ragged_widths(K):
    """K % 4 != 0: the rows of `in` start at 4-byte multiples only, and the last group of a row goes through the scalar tail"""
    x = np.random.default_rng(K).standard_normal((7, K)).astype(F)
    want = P.convert_pad_ref(x, 64)
    for dt in (torch.float32, torch.bfloat16):
        got = ops.convert_pad(t(x), 64, dt)
        assert torch.equal(bits(got), bits(t(want).to(dt))), f"convert_pad K={K} {dt}"


def test_embed_rows_clamps_ids():
    V, E = 7, 8
    table = np.random.default_rng(0).standard_normal((V, E)).astype(F)
    ids = np.array([-1, V, 2 ** 40, INT64_MIN, 3, 0, V - 1], dtype=np.int64)
    want = P.embed_rows_ref(table, ids, 16)
    assert np.array_equal(want[:4, :E], table[[0, V - 1, V - 1, 0]])
    for dt in (torch.float32, torch.bfloat16):
        got = ops.embed_rows(t(table), t(ids), 16, dt)
        assert torch.equal(bits(got), bits(t(want).to(dt))), f"embed_rows {dt}"


def test_add_rows_wraps_the_table():
    rng = np.random.default_rng(1)
    x, table = rng.standard_normal((50, 12)).astype(F), rng.standard_normal((16, 12)).astype(F)
    assert np.array_equal(n(ops.add_rows(t(x), t(table))), P.add_rows_ref(x, table))
