"""What tests/rowop_probes.py can tell apart, without a GPU: the clean float32 restatement of every kernel entry stays within the
element-wise bound against the float64 reference in every case the GPU file launches (the worst ratio per entry is printed: pytest -s,
and recorded in the probe module's docstring), and every planted fault is rejected in a named case by at least 8 times the bound, with
outputs that differ from the clean ones.  A fault that no case rejects is a missing case."""
import numpy as np
import pytest

import rowop_probes as P

F = np.float32
LN_D = (4, 64, 252, 256, 260, 512, 768, 1024, 1028, 1280, 2052)
HILO_D = (4, 72, 252, 256, 260, 768, 1020, 1024)
COEF_D = (8, 72, 248, 256, 264, 520, 1016, 1024)
CE_V = (4, 64, 256, 260, 1024, 1028, 8192, 8196, 16384)
CE_EPS = (0.0, 0.1, 1.0)
REJECT = 8.0
WORST = {}


def note(entry, r):
    assert r <= 1.0, (entry, r)
    WORST[entry] = max(WORST.get(entry, 0.0), r)


def teardown_module(module):
    print("\nworst |error| / bound of the clean restatement per entry:")
    for k in sorted(WORST):
        print(f"    {k:24s} {WORST[k]:.3f}")


def pair_value(pair):
    return pair[0].astype(np.float64) + pair[1].astype(np.float64)


# ---- clean restatements stay within every bound ----------------------------------------------------------------------------------
@pytest.mark.parametrize("D", LN_D)
def test_clean_layernorm(D):
    for M in (1, 13):
        fam = P.ln_family(M, D)
        x, ga, be = fam["x"], fam["gamma"], fam["beta"]
        for eps in P.EPS_VALUES:
            want = P.ln_ref(x, ga, be, eps)
            for out in ("f32", "bf16"):
                got = P.emulate_layernorm(x, ga, be, eps, out)
                note(f"layernorm {out}", P.assert_within(got, want, P.ln_bound(x, ga, be, eps, out), f"D={D} M={M} eps={eps} {out}", fam["kinds"]))


@pytest.mark.parametrize("D", HILO_D)
def test_clean_hilo_family(D):
    fam = P.hilo_family(13, D)
    hi, lo, ga, be, kinds = fam["hi"], fam["lo"], fam["gamma"], fam["beta"], fam["kinds"]
    x64 = P.hilo_value(hi, lo)
    e_in = P.hilo_input_error(hi, lo)
    for eps in P.EPS_VALUES:
        want = P.ln_ref(x64, ga, be, eps)
        for out in ("f32", "bf16"):
            got = P.emulate_layernorm_hilo(hi, lo, ga, be, eps, out)
            note(f"layernorm_hilo {out}", P.assert_within(got, want, P.ln_bound(x64, ga, be, eps, out, e_in), f"hilo D={D} eps={eps} {out}", kinds))
        x = fam["x"]
        got = pair_value(P.emulate_layernorm(x, ga, be, eps, "hilo"))
        note("layernorm_to_hilo", P.assert_within(got, P.ln_ref(x, ga, be, eps), P.ln_bound(x, ga, be, eps, "hilo"), f"to_hilo D={D} eps={eps}", kinds))
    xm = P.mixed_magnitudes(13, D)
    h, l = P.split_hilo(xm)
    note("split_hilo", P.assert_within(pair_value((h, l)), xm, P.split_bound(xm), f"split D={D}"))
    note("join_hilo", P.assert_within(P.emulate_join(h, l), P.hilo_value(h, l), P.join_bound(h, l), f"join D={D}"))
    l = np.roll(l, 1, axis=1)                                   # lo planes of the neighbouring column: hi + lo has to be rounded
    note("join_hilo", P.assert_within(P.emulate_join(h, l), P.hilo_value(h, l), P.join_bound(h, l), f"join D={D}, foreign lo"))
    c = P.hilo_family(13, D, centred=True)
    got = pair_value(P.emulate_unshift(c["hi"], c["lo"], c["shift"]))
    note("unshift_hilo", P.assert_within(got, P.hilo_value(c["hi"], c["lo"], c["shift"]), P.unshift_bound(c["hi"], c["lo"], c["shift"]),
                                         f"unshift D={D}", kinds))


@pytest.mark.parametrize("D", COEF_D)
def test_clean_ln_coef(D):
    for M in (1, 13, 17):
        hi = P.hilo_family(M, D)["hi"]
        for eps in P.EPS_VALUES:
            note("ln_coef", P.assert_within(P.emulate_ln_coef(hi, eps), P.coef_ref(hi, eps), P.coef_bound(hi, eps), f"ln_coef D={D} M={M} eps={eps}"))


@pytest.mark.parametrize("nparts", range(1, 17))
def test_clean_ln_coef_parts(nparts):
    for M in (1, 13, 33):
        parts = P.make_parts(P.ln_family(M, 64 * nparts)["x"], nparts)
        for eps in P.EPS_VALUES:
            want, bound = P.parts_ref(parts, eps)
            note("ln_coef_parts", P.assert_within(P.emulate_ln_coef_parts(parts, eps), want, bound, f"parts nparts={nparts} M={M} eps={eps}"))


@pytest.mark.parametrize("V", CE_V)
def test_clean_masked_ce(V):
    for kind in P.CE_FAMILIES:
        fam = P.ce_family(kind, 5, V)
        for eps in CE_EPS:
            rows, drow, loss, dloss = P.ce_ref(fam["logits"], fam["labels"], fam["mask"], eps)
            got_rows, got_loss = P.emulate_masked_ce(fam["logits"], fam["labels"], fam["mask"], eps)
            note("masked_ce rows", P.assert_within(got_rows, rows, drow, f"ce rows {kind} V={V} eps={eps}"))
            note("masked_ce loss", P.assert_within(got_loss, loss, dloss, f"ce loss {kind} V={V} eps={eps}"))
        assert fam["labels"].min() >= 0 and fam["labels"].max() < V


def test_ce_labels_cover_the_edge_columns():
    seen = set()
    for kind in P.CE_FAMILIES:
        seen |= set(int(c) for c in P.ce_family(kind, 5, 1028)["labels"])
    assert seen == {0, 3, 4, 255, 256, 1024, 1027}


@pytest.mark.parametrize("M", [1024, 1025, 2500])
def test_clean_masked_ce_many_rows(M):
    fam = P.ce_family("mixed", M, 64)
    rows, drow, loss, dloss = P.ce_ref(fam["logits"], fam["labels"], fam["mask"], 0.1)
    got_rows, got_loss = P.emulate_masked_ce(fam["logits"], fam["labels"], fam["mask"], 0.1)
    note("masked_ce rows", P.assert_within(got_rows, rows, drow, f"ce rows M={M}"))
    note("masked_ce loss", P.assert_within(got_loss, loss, dloss, f"ce loss M={M}"))


@pytest.mark.parametrize("N", [1, 63, 64, 65])
def test_clean_random_mask(N):
    for kind in P.NOISE_KINDS:
        for E in (1, 4, 5):
            fam = P.mask_family(2, N, E, kind)
            for keep in sorted({0, 1, N - 1, N}):
                x, mask = P.emulate_random_mask(fam["z"], fam["noise"], fam["mask_token"], keep)
                xr, mr = P.mask_ref(fam["z"], fam["noise"], fam["mask_token"], keep)
                assert np.array_equal(mask, mr) and np.array_equal(x, xr), (N, kind, E, keep)
                assert int(mask.sum()) == 2 * (N - keep)


# ---- every fault is rejected in a named case -------------------------------------------------------------------------------------
def rejected(got, want, bound, clean):
    differs = not np.array_equal(np.asarray(got), np.asarray(clean), equal_nan=True)
    return differs and P.ratio(got, want, bound) >= REJECT


# fault -> ((D, M) of pmhip_layernorm, D of the hi/lo entries (M = 13), D of pmhip_ln_coef (M = 13), eps): cases the GPU file launches
LN_CASES = {
    "one_pass_variance": ((768, 13), 768, 1016, 1e-5),       # the offset rows: mean 1000 with sigma 1, mean -30 with sigma 0.01
    "eps_outside_sqrt": ((768, 13), 768, 1016, 1e-2),        # the tiny and constant rows: var << eps
    "eps_ignored": ((256, 13), 256, 256, 1e-2),
    "unbiased_variance": ((64, 13), 72, 72, 1e-5),
    "stats_from_next_row": ((512, 13), 256, 520, 1e-5),
    "tail_columns_dropped": ((260, 13), 260, 264, 1e-5),     # the spike in the last column is outside 256 floor(D / 256)
    "divide_by_padded_width": ((260, 13), 260, 264, 1e-5),
    "gamma_shifted_4": ((1024, 1), 1024, None, 1e-6),
}


@pytest.mark.parametrize("fault", P.LN_FAULTS)
def test_layernorm_fault_is_rejected(fault):
    (D, M), Dh, Dc, eps = LN_CASES[fault]
    fam = P.ln_family(M, D)
    x, ga, be = fam["x"], fam["gamma"], fam["beta"]
    want = P.ln_ref(x, ga, be, eps)
    for out in ("f32", "bf16"):
        clean = P.emulate_layernorm(x, ga, be, eps, out)
        bad = P.emulate_layernorm(x, ga, be, eps, out, fault)
        assert rejected(bad, want, P.ln_bound(x, ga, be, eps, out), clean), (fault, out, P.ratio(bad, want, P.ln_bound(x, ga, be, eps, out)))
    h = P.hilo_family(13, Dh)
    hi, lo, ga, be = h["hi"], h["lo"], h["gamma"], h["beta"]
    x64, e_in = P.hilo_value(hi, lo), P.hilo_input_error(hi, lo)
    for out in ("f32", "bf16"):
        bound = P.ln_bound(x64, ga, be, eps, out, e_in)
        assert rejected(P.emulate_layernorm_hilo(hi, lo, ga, be, eps, out, fault), P.ln_ref(x64, ga, be, eps), bound,
                        P.emulate_layernorm_hilo(hi, lo, ga, be, eps, out)), (fault, out)
    x = h["x"]
    assert rejected(pair_value(P.emulate_layernorm(x, ga, be, eps, "hilo", fault)), P.ln_ref(x, ga, be, eps), P.ln_bound(x, ga, be, eps, "hilo"),
                    pair_value(P.emulate_layernorm(x, ga, be, eps, "hilo"))), fault
    if Dc is not None:
        hi = P.hilo_family(13, Dc)["hi"]
        assert rejected(P.emulate_ln_coef(hi, eps, fault), P.coef_ref(hi, eps), P.coef_bound(hi, eps), P.emulate_ln_coef(hi, eps)), fault


def test_eps_values_are_told_apart_at_every_width():
    """a kernel that ignores its eps argument fails at eps = 1e-6 too (the tiny rows), not only at 1e-2"""
    fam = P.ln_family(13, 768)
    x, ga, be = fam["x"], fam["gamma"], fam["beta"]
    bad = P.emulate_layernorm(x, ga, be, 1e-6, "f32", "eps_ignored")
    assert P.ratio(bad, P.ln_ref(x, ga, be, 1e-6), P.ln_bound(x, ga, be, 1e-6)) >= REJECT


def test_lo_plane_ignored_is_rejected():
    fam = P.hilo_family(13, 768)                      # offset rows: hi alone resolves 1000 to 4 and -30 to 0.125
    hi, lo, ga, be = fam["hi"], fam["lo"], fam["gamma"], fam["beta"]
    x64 = P.hilo_value(hi, lo)
    bound = P.ln_bound(x64, ga, be, 1e-5, "f32", P.hilo_input_error(hi, lo))
    assert rejected(P.emulate_layernorm_hilo(hi, lo, ga, be, 1e-5, "f32", "lo_plane_ignored"), P.ln_ref(x64, ga, be, 1e-5), bound,
                    P.emulate_layernorm_hilo(hi, lo, ga, be, 1e-5, "f32"))
    h, l = P.split_hilo(P.mixed_magnitudes(13, 72))
    assert rejected(P.emulate_join(h, l, "lo_plane_ignored"), P.hilo_value(h, l), P.join_bound(h, l), P.emulate_join(h, l))
    c = P.hilo_family(13, 260, centred=True)
    want, bound = P.hilo_value(c["hi"], c["lo"], c["shift"]), P.unshift_bound(c["hi"], c["lo"], c["shift"])
    assert rejected(pair_value(P.emulate_unshift(c["hi"], c["lo"], c["shift"], "lo_plane_ignored")), want, bound,
                    pair_value(P.emulate_unshift(c["hi"], c["lo"], c["shift"])))


@pytest.mark.parametrize("fault", ["shift_ignored", "shift_from_next_row"])
def test_shift_fault_is_rejected(fault):
    c = P.hilo_family(13, 260, centred=True)
    want, bound = P.hilo_value(c["hi"], c["lo"], c["shift"]), P.unshift_bound(c["hi"], c["lo"], c["shift"])
    assert rejected(pair_value(P.emulate_unshift(c["hi"], c["lo"], c["shift"], fault)), want, bound,
                    pair_value(P.emulate_unshift(c["hi"], c["lo"], c["shift"])))


@pytest.mark.parametrize("fault", P.PARTS_FAULTS)
def test_parts_fault_is_rejected(fault):
    parts = P.make_parts(P.ln_family(13, 768)["x"], 12)          # 12 parts: four of them in the upper half, 768 != 1024
    want, bound = P.parts_ref(parts, 1e-5)
    assert rejected(P.emulate_ln_coef_parts(parts, 1e-5, fault), want, bound, P.emulate_ln_coef_parts(parts, 1e-5)), fault


def test_parts_bits_match_allows_the_square_root_only():
    parts = P.make_parts(P.ln_family(13, 768)["x"], 12)
    coef, mean = P.emulate_ln_coef_parts(parts, 1e-5, return_mean=True)
    assert P.parts_bits_match(coef, parts, 1e-5) is None
    up = coef.copy()
    up[:, 0] = np.nextafter(np.nextafter(coef[:, 0], F(np.inf)), F(np.inf))      # a square root one ulp off: rstd two ulp off
    up[:, 1] = (-up[:, 0]) * mean
    assert P.parts_bits_match(up, parts, 1e-5) is None
    far = up.copy()
    far[:, 0] = coef[:, 0] + 4 * np.spacing(coef[:, 0])
    far[:, 1] = (-far[:, 0]) * mean
    assert "ulp" in P.parts_bits_match(far, parts, 1e-5)
    other = coef.copy()                                                          # another mean: another product
    other[:, 1] = (-coef[:, 0]) * np.nextafter(mean, F(np.inf)) * F(1 + 2.0 ** -20)
    assert "mean of row" in P.parts_bits_match(other, parts, 1e-5)


# fault -> (family, V, label smoothing)
CE_CASES = {
    "no_max_subtraction": ("minus3000", 64, 0.1),                 # exp(-3000) = 0: log(0); 'plus100' overflows instead (below)
    "smoothing_mean_over_padded_width": ("base", 260, 0.1),       # 260 columns in 1024 lanes' worth
    "eps_weights_swapped": ("peaky", 1028, 0.1),
    "mean_over_all_rows": ("base", 64, 0.1),                      # rows 1 and 4 of 5 are not masked
    "label_from_next_row": ("base", 8196, 0.0),
}


@pytest.mark.parametrize("fault", P.CE_FAULTS)
def test_masked_ce_fault_is_rejected(fault):
    kind, V, eps = CE_CASES[fault]
    fam = P.ce_family(kind, 5, V)
    rows, drow, loss, dloss = P.ce_ref(fam["logits"], fam["labels"], fam["mask"], eps)
    clean_rows, clean_loss = P.emulate_masked_ce(fam["logits"], fam["labels"], fam["mask"], eps)
    bad_rows, bad_loss = P.emulate_masked_ce(fam["logits"], fam["labels"], fam["mask"], eps, fault)
    assert rejected(bad_loss, loss, dloss, clean_loss), (fault, bad_loss, loss)
    if fault != "mean_over_all_rows":
        assert rejected(bad_rows, rows, drow, clean_rows), fault


def test_no_max_subtraction_overflows_at_plus_100():
    fam = P.ce_family("plus100", 5, 256)
    rows, drow, _, _ = P.ce_ref(fam["logits"], fam["labels"], fam["mask"], 0.1)
    bad_rows, _ = P.emulate_masked_ce(fam["logits"], fam["labels"], fam["mask"], 0.1, "no_max_subtraction")
    assert P.ratio(bad_rows, rows, drow) >= REJECT


def test_label_smoothing_one_tells_the_weights_apart():
    """at label_smoothing = 1 the row is the smoothing term alone: the label must not matter"""
    fam = P.ce_family("peaky", 5, 256)
    rows, _, _, _ = P.ce_ref(fam["logits"], fam["labels"], fam["mask"], 1.0)
    other, _, _, _ = P.ce_ref(fam["logits"], (fam["labels"] + 1) % 256, fam["mask"], 1.0)
    assert np.array_equal(rows, other)


# fault -> (noise, N, E, len_keep)
MASK_CASES = {
    "ties_to_larger_index": ("all_equal", 65, 4, 1),              # keeps position 0; the fault keeps position 64
    "rank_off_by_one": ("uniform", 64, 1, 63),
    "token_column_from_row": ("uniform", 63, 5, 0),
}


@pytest.mark.parametrize("fault", P.MASK_FAULTS)
def test_random_mask_fault_is_rejected(fault):
    kind, N, E, keep = MASK_CASES[fault]
    fam = P.mask_family(2, N, E, kind)
    xr, mr = P.mask_ref(fam["z"], fam["noise"], fam["mask_token"], keep)
    x, mask = P.emulate_random_mask(fam["z"], fam["noise"], fam["mask_token"], keep, fault)
    assert not np.array_equal(x, xr), fault
    if fault != "token_column_from_row":
        assert not np.array_equal(mask, mr), fault


def test_signed_zeros_are_ties():
    fam = P.mask_family(1, 64, 1, "signed_zeros")
    nz = fam["noise"][0]
    assert np.signbit(nz).any() and (~np.signbit(nz) & (nz == 0)).any()
    _, mask = P.mask_ref(fam["z"], fam["noise"], fam["mask_token"], 5)
    zeros = np.nonzero(nz == 0)[0]
    assert np.array_equal(np.nonzero(mask[0] == 0)[0], zeros[:5])          # the first five zeros of either sign, by index


# ---- the number formats ---------------------------------------------------------------------------------------------------------
def test_bf16_half_ulp():
    """round to nearest of bf16 errs by up to 2^-8 |y|, not 2^-9 |y|: why the bf16 term of ln_bound is half an ulp"""
    import torch
    y = np.array([1.0 + 2.0 ** -8 + 2.0 ** -20], dtype=F)
    cast = torch.from_numpy(y).to(torch.bfloat16).float().numpy()
    assert cast[0] == F(1.0 + 2.0 ** -7) and np.array_equal(P.bf16_round(y), cast)
    err = abs(float(cast[0]) - float(y[0]))
    assert 2.0 ** -9 * y[0] < err <= P.half_ulp_bf16(y)[0] == 2.0 ** -8
    x = np.random.default_rng(0).standard_normal(4096).astype(F) * F(100)
    assert np.array_equal(P.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    assert (np.abs(P.bf16_round(x).astype(np.float64) - x) <= P.half_ulp_bf16(x)).all()


def test_row_utility_references():
    img = np.arange(2 * 3 * 16 * 40, dtype=F).reshape(2, 3, 16, 40)
    out = P.patchify_ref(img, 8)
    assert out.shape == (2 * 2 * 5, 3 * 64) and out[7, 64 + 8 * 3 + 5] == img[0, 1, 8 + 3, 2 * 8 + 5]  # m = 7: b 0, ph 1, pw 2
    y = np.random.default_rng(1).standard_normal((2 * 2 * 5, 4 * 4 * 3)).astype(F)
    y[3, 5] = np.nan
    y[4, 6] = 0.5
    im = P.unpatchify_ref(y, 2, 3, 8, 20, 4, 0.0, 0.5)
    assert im.shape == (2, 3, 8, 20) and np.isnan(im).sum() == 1 and np.nanmax(im) == 0.5 and np.nanmin(im) == 0.0
    assert im[0, 5 % 3, 1 // 4, 3 * 4 + 1] != im[0, 5 % 3, 1 // 4, 3 * 4 + 1]                            # (i P + j) C + c = 5: i 0, j 1, c 2
    ids = np.array([-1, 7, 2 ** 40, np.iinfo(np.int64).min, 3])
    table = np.arange(28, dtype=F).reshape(7, 4)
    assert np.array_equal(P.embed_rows_ref(table, ids, 8)[:, :4], table[[0, 6, 6, 0, 3]])
