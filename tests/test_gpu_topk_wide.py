"""Top-k above 64, up to the whole codebook, on the GPU: sample_wide_kernel against the CPU oracle in every
size class, at ties that straddle position k, against the existing row kernel's confidence bits, on the Philox stream, through the
C entry with strides and aliasing, and through every form of the engine's step -- the engine cases bit for bit.

Comparisons against ``O.sample_rows`` want the prediction and the merged ids exact and the score within rtol 1e-4 / atol 1e-6 (the
tolerance of tests/test_gpu_fuzz.py for this operator).  A row is exempt from the id comparison only where the ORACLE's own winner
leads its runner-up by less than 1e-5 relative in perturbed value (device logf and numpy may round apart there), and at most 1 % of
a case's rows may be: with the 1..9 rows of the cases below that is no row at all.  The seeds below were chosen on the CPU; with
them the oracle exempts 0 rows in the size classes (768 calls), 0 at the threshold ties, 0 on the Philox stream and 0 in the
-inf / stride cases, so every comparison in this file is exact.
"""
import copy
import itertools

import numpy as np
import pytest
import torch

import paintmind_amd as pm
from abi_frames import bits, call, framed
from gpu_common import dev, n, t
from oracle import paintmind_oracle as O
from paintmind_amd import ops
from paintmind_amd.generate import Pipeline, num_token_masked

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [68, 256, 260, 1024, 1028, 8192, 8196, 16384]       # NV4 = 1, 1, 4, 4, 32, 32, 64, 64: full and ragged last groups
ROWS = [1, 5, 9]                                             # a partial workgroup, one and a bit, more than two (4 rows each)
TEMPS = [0.0, 0.3, 1.0, 2.5]
SCALES = [0.5, 20.0]


def oracle_exempt(logits, topk, temperature, noise):
    """rows where the oracle's winner leads its runner-up by less than 1e-5 relative in perturbed value"""
    order = O.order_desc_then_index(logits)[:, :topk]
    filt = np.full_like(logits, -np.inf)
    np.put_along_axis(filt, order, np.take_along_axis(logits, order, 1), 1)
    pert = filt / F(max(temperature, 1e-10)) + O.gumbel_from_uniform(noise.astype(F))
    top = -np.partition(-pert, 1, axis=1)[:, :2]
    with np.errstate(invalid="ignore"):
        return (top[:, 0] - top[:, 1]) < 1e-5 * np.abs(top[:, 0])


def check_against_oracle(got, logits, ids, mask_id, topk, temperature, noise, what, exact_ties=False):
    """-> the number of exempt rows (asserted to be at most 1 % of the case's rows).  exact_ties: equal perturbed values in the
    case come from equal logits under equal noise -- the same bits on the device too -- so no row is exempt."""
    pred, merged, score = (n(x) for x in got)
    pr, mr, sr = O.sample_rows(logits, ids, mask_id, topk, temperature, noise)
    exempt = np.zeros(len(pr), bool) if exact_ties else oracle_exempt(logits, topk, temperature, noise)
    assert exempt.sum() <= len(exempt) // 100, (what, int(exempt.sum()))
    keep = ~exempt
    assert np.array_equal(pred[keep], pr[keep]), (what, np.flatnonzero(pred != pr)[:8], pred[pred != pr][:8], pr[pred != pr][:8])
    assert np.array_equal(merged[keep], mr[keep]), what
    assert np.allclose(score[keep], sr[keep], rtol=1e-4, atol=1e-6), (what, np.abs(score - sr).max())
    return int(exempt.sum())


def size_class_cases(V):
    """(M, topk, temperature, scale, logits, ids, noise) for one class count: every combination, inputs from one seed per V"""
    rng = np.random.default_rng(7000 + V)
    ks = sorted({65, (65 + V) // 2, V - 1, V})
    for M, topk, temp, scale in itertools.product(ROWS, ks, TEMPS, SCALES):
        logits = (rng.standard_normal((M, V)) * scale).astype(F)
        ids = rng.integers(0, V + 1, M).astype(np.int64)        # V = mask id
        noise = rng.random((M, V)).astype(F)
        yield M, topk, temp, scale, logits, ids, noise


# ------------------------------------------------------------------------------------------------------------------------------
# a. every size class
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", SIZES)
def test_size_classes_against_the_oracle(V):
    exempt = 0
    for M, topk, temp, scale, logits, ids, noise in size_class_cases(V):
        got = ops.sample_rows(t(logits), t(ids), V, topk, temp, noise=t(noise))
        exempt += check_against_oracle(got, logits, ids, V, topk, temp, noise, (V, M, topk, temp, scale))
    print(f"V={V}: {exempt} exempt rows")


# ------------------------------------------------------------------------------------------------------------------------------
# b. a plateau of equal values that straddles position k
# ------------------------------------------------------------------------------------------------------------------------------
PLATEAU, ABOVE = 40, 70


def plateau_rows(V, M, seed):
    """quantised logits: ABOVE elements above a plateau of PLATEAU equal values, everything else below (with ties of its own);
    -> (logits, the plateau's columns per row in column order).  The plateau covers all four components of a float4 and, beyond
    V = 256, many lanes and groups."""
    rng = np.random.default_rng(seed)
    logits = np.round(rng.standard_normal((M, V)) * 2).astype(F).clip(-6, 1)          # below: integers <= 1
    cols = []
    for r in range(M):
        pick = rng.permutation(V)[:PLATEAU + ABOVE]
        pl = np.sort(pick[:PLATEAU])
        while len({int(c) & 3 for c in pl}) < 4 or len({int(c) >> 8 for c in pl}) < min(4, V // 256):
            pick = rng.permutation(V)[:PLATEAU + ABOVE]
            pl = np.sort(pick[:PLATEAU])
        logits[r, pl] = 2.0
        logits[r, pick[PLATEAU:]] = rng.integers(3, 6, ABOVE).astype(F)               # above: 3, 4 or 5
        cols.append(pl)
    return logits, cols


@pytest.mark.parametrize("r", [1, 20, 39])
@pytest.mark.parametrize("V", [8192, 1028, 16384, 260])
def test_ties_at_the_threshold(V, r):
    M, k = 5, ABOVE + r
    logits, cols = plateau_rows(V, M, 100 * r + V)
    ids = np.full(M, V, np.int64)
    first_max = logits.argmax(1)
    near_one = F(1.0 - 2.0 ** -24)
    for case, which in (("kept", r - 1), ("dropped", r)):
        noise = np.full((M, V), 0.5, F)
        hot = np.array([cols[m][which] for m in range(M)])
        noise[np.arange(M), hot] = near_one                    # gumbel = 16.6: wins against everything, if it is kept at all
        got = ops.sample_rows(t(logits), t(ids), V, k, 1.0, noise=t(noise))
        assert check_against_oracle(got, logits, ids, V, k, 1.0, noise, (V, r, case), exact_ties=True) == 0
        assert np.array_equal(n(got[0]), hot if case == "kept" else first_max), (V, r, case)


# ------------------------------------------------------------------------------------------------------------------------------
# c. the normaliser is the row kernel's: the same confidence bits at k = 64 and beyond
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [8192, 1028])
def test_confidence_bits_continue_the_row_kernel(V):
    M = 9
    rng = np.random.default_rng(V)
    logits = t((rng.standard_normal((M, V)) * 3).astype(F))
    ids = torch.full((M,), V, dtype=torch.long, device=dev())
    noise = torch.full((M, V), 0.5, device=dev())
    ref = ops.sample_rows(logits, ids, V, 64, 0.7, noise=noise)          # sample_rows_kernel
    assert torch.equal(ref[0], logits.argmax(1))
    for k in (9, 65, V - 1, V):
        got = ops.sample_rows(logits, ids, V, k, 0.7, noise=noise)
        for a, b in zip(got, ref):
            assert torch.equal(bits(a), bits(b)), k


# ------------------------------------------------------------------------------------------------------------------------------
# d. the Philox stream: a uniform belongs to (seed, step, row, column), never to k
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,row_base", [(1028, 12345), (8192, 2 ** 32 + 77), (256, 2 ** 40 + 3)])
def test_philox_stream_is_the_oracles(V, row_base):
    M, seed, step = 9, 0xFEDCBA9876543210, 5
    rng = np.random.default_rng(V + 1)
    logits = (rng.standard_normal((M, V)) * 2).astype(F)
    ids = rng.integers(0, V + 1, M).astype(np.int64)
    u = O.philox_uniform(seed, step, (row_base + np.arange(M, dtype=np.uint64))[:, None], np.arange(V, dtype=np.uint64)[None, :])
    assert u.shape == (M, V)
    for k in (V, 100):
        got = ops.sample_rows(t(logits), t(ids), V, k, 1.0, seed=seed, step=step, row_base=row_base)
        assert check_against_oracle(got, logits, ids, V, k, 1.0, u, (V, k)) == 0
        given = ops.sample_rows(t(logits), t(ids), V, k, 1.0, noise=t(u))
        assert all(torch.equal(a, b) for a, b in zip(got, given))        # the same uniforms, bit for bit, whichever way they come


# ------------------------------------------------------------------------------------------------------------------------------
# e. strides, aliasing, -inf
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,topk", [(1028, 100), (8192, 8192), (260, 259)])
def test_strided_logits_and_ids_in_place_through_the_c_entry(V, topk):
    M = 9
    rng = np.random.default_rng(3 * V)
    logits = (rng.standard_normal((M, V)) * 3).astype(F)
    ids = rng.integers(0, V + 1, M).astype(np.int64)
    noise = rng.random((M, V)).astype(F)
    fx = framed(M, V, dtype=torch.float32, payload=t(logits), fill="nan")             # ld > V, NaN in the gap and around
    fi = framed(M, 1, ld=1, dtype=torch.int64, payload=t(ids).reshape(M, 1))          # ids_in AND ids_out
    fp = framed(M, 1, ld=1, dtype=torch.int64, device=dev())
    fs = framed(M, 1, ld=1, dtype=torch.float32, device=dev())
    call("pmhip_sample_rows", fx, fx.ld, fi, V, topk, 0.8, t(noise), 0, 0, 0, fp, fi, fs, M, V)
    for f, what in ((fx, "logits"), (fi, "ids"), (fp, "pred"), (fs, "score")):
        f.assert_frame_untouched(what)
    got = (fp.payload().reshape(M), fi.payload().reshape(M), fs.payload().reshape(M))
    assert check_against_oracle(got, logits, ids, V, topk, 0.8, noise, (V, topk)) == 0


@pytest.mark.parametrize("temp", [0.0, 1.0])
def test_rows_of_minus_infinity(temp):
    V, M, k, finite = 1028, 5, 100, 70
    rng = np.random.default_rng(11)
    logits = np.full((M, V), -np.inf, F)
    noise = rng.random((M, V)).astype(F)
    for m in range(M):
        cols = rng.permutation(V)[:finite]
        logits[m, cols] = rng.standard_normal(finite).astype(F) * 2
        lowest_inf = int(np.flatnonzero(np.isinf(logits[m]))[0])
        noise[m, lowest_inf] = F(1.0 - 2.0 ** -24)             # a kept -inf element with the best noise there is: it still loses
    ids = np.full(M, V, np.int64)
    got = ops.sample_rows(t(logits), t(ids), V, k, temp, noise=t(noise))
    assert check_against_oracle(got, logits, ids, V, k, temp, noise, temp) == 0
    assert np.isfinite(logits[np.arange(M), n(got[0])]).all()


# ------------------------------------------------------------------------------------------------------------------------------
# f. through the engine: a tiny pipeline with 256 classes (the tiny configurations stop at 64)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide_pipe():
    vq = copy.deepcopy(pm.ver2cfg["tiny-vqgan"])
    vq["n_embed"] = 256
    pm.ver2cfg["tiny-vqgan-256"] = vq
    pm.ver2cfg["tiny-pipeline-256"] = dict(pm.ver2cfg["tiny-pipeline"], stage1="tiny-vqgan-256")
    try:
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(256)
            pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline-256"]), stage1_pretrained=False)
            pipe.transformer.to_logits.weight.data.mul_(8.0)   # logits that spread: a top-k filter then matters
        yield pipe.to(dev()).eval()
    finally:
        del pm.ver2cfg["tiny-vqgan-256"], pm.ver2cfg["tiny-pipeline-256"]


@pytest.fixture(params=[torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def pipe(request, wide_pipe):
    wide_pipe.set_compute_dtype(request.param)
    yield wide_pipe
    wide_pipe.set_compute_dtype(torch.float32)


def _start(pipe, B, seed=0):
    """a partially given start: about a third of the positions hold an id"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((B, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long)
    given = torch.rand(B, pipe.num_tokens, generator=g) < 0.3
    return torch.where(given, torch.randint(0, pipe.mask_token_id, ids.shape, generator=g), ids).to(dev())


def _compose(pipe, ids0, logits, k, temperature, nm, noise=None, seed=0, step=0, image_base=0, choice_temperature=0.0):
    B, N, V = ids0.shape[0], pipe.num_tokens, pipe.mask_token_id
    if noise is not None:
        noise = noise.reshape(B * N, V)
    _, merged, score = ops.sample_rows(logits.reshape(B * N, V), ids0.reshape(-1), V, k, temperature, noise=noise, seed=seed, step=step,
                                       row_base=image_base * N)
    return ops.remask(merged.reshape(B, N), score.reshape(B, N), nm, V, choice_temperature=choice_temperature, seed=seed, step=step,
                      row_base=image_base * N)              # (the re-masking's own Philox draws, when it has a choice temperature)


def test_sample_equals_the_operator_composition(pipe):
    B, N, V = 3, pipe.num_tokens, pipe.mask_token_id
    assert V == 256
    ctx = pipe.text_model(["a", "b", "c"]).to(dev())
    ids0 = _start(pipe, B)
    noise = torch.rand(B, N, V, generator=torch.Generator().manual_seed(4)).to(dev())
    nm = num_token_masked(np.float64(0.5), N)
    for text in (ctx, None):
        logits = pipe.engine().forward(pipe.ids2tokens(ids0), text)
        for k in (100, 256, None):
            got, img = pipe.sample(ids0, np.float64(0.5), text=text, topk=k, temperature=0.8, noise=noise)
            assert torch.equal(got, _compose(pipe, ids0, logits, V if k is None else k, 0.8, nm, noise=noise)), k
            assert img.shape[0] == B and bool(torch.isfinite(img).all())


def _loop_of_samples(pipe, context, B, T, temperature, topk, seed, base):
    """the loop as one native step per call, under the loop's seed"""
    temps, nmask = pipe._schedule(T, temperature)
    ids = pipe._start_ids(B, None, dev())
    eng = pipe.engine()
    for step in range(T):
        ids, _, _, _ = eng.sample(None, ids, context, topk, temps[step], nmask[step], seed=seed, step=step, image_base=base, want_img=False)
    return ids


def test_generate_ids_eager_graph_and_step_loop_agree(pipe):
    B, T, k = 4, 4, 200
    context = pipe.text_model(["a", "b", "c", "d"]).to(dev())
    flags = [False] * T
    want = _loop_of_samples(pipe, context, B, T, 1.0, k, 77, 12)
    eager, _ = pipe.generate_ids(context, B, T, 1.0, k, flags, 77, image_base=12, use_graph=False, streams=1)
    assert torch.equal(eager, want)
    for _ in range(3):                                           # eager once, capture, replay
        graph, _ = pipe.generate_ids(context, B, T, 1.0, k, flags, 77, image_base=12, use_graph=True, streams=1)
        assert torch.equal(graph, want)
    none, _ = pipe.generate_ids(context, B, T, 1.0, None, flags, 77, image_base=12, use_graph=True, streams=1)
    full, _ = pipe.generate_ids(context, B, T, 1.0, 256, flags, 77, image_base=12, use_graph=False, streams=1)
    assert torch.equal(none, full)


@pytest.mark.parametrize("mode", ["guided", "choice", "context_lens"])
def test_other_step_forms_equal_their_compositions(pipe, mode):
    B, N, V, k = 3, pipe.num_tokens, pipe.mask_token_id, 100
    ctx = pipe.text_model(["a", "b", "c"]).to(dev())
    ids0 = _start(pipe, B, 2)
    nm = num_token_masked(np.float64(0.5), N)
    tok = pipe.ids2tokens(ids0)
    common = dict(text=ctx, topk=k, temperature=0.8, seed=9, step=2, image_base=5)
    if mode == "guided":
        got, _ = pipe.sample(ids0, np.float64(0.5), guidance_scale=2, **common)
        want, _ = pipe._sample_guided_composed(ids0, nm, ctx, k, 0.8, None, 9, 2, 5, 2.0)
    elif mode == "choice":
        got, _ = pipe.sample(ids0, np.float64(0.5), choice_temperature=4.5, **common)
        want = _compose(pipe, ids0, pipe.engine().forward(tok, ctx), k, 0.8, nm, seed=9, step=2, image_base=5, choice_temperature=4.5)
    else:
        L = ctx.shape[1]
        lens = [1, L, min(2, L)]
        got, _ = pipe.sample(ids0, np.float64(0.5), context_lens=lens, **common)
        want = _compose(pipe, ids0, pipe.engine().forward(tok, ctx, context_lens=lens), k, 0.8, nm, seed=9, step=2, image_base=5)
    assert torch.equal(got, want)


def test_shared_step0_logits_serve_the_wide_kernel(pipe):
    """an unconditional loop from the all-mask state samples its step 0 from ONE image's logits (the PERIOD form of the kernel);
    an explicit all-mask start keeps the full path: the same ids"""
    B, T, k = 5, 3, 200
    flags = [False] * T
    full, _ = pipe.generate_ids(None, B, T, 1.0, k, flags, 31, image_base=3, use_graph=False, streams=1, ids0=pipe._start_ids(B, None, dev()))
    hits0 = pipe.engine().step0_shared()[1]
    for use_graph in (False, False, True, True, True):
        shared, _ = pipe.generate_ids(None, B, T, 1.0, k, flags, 31, image_base=3, use_graph=use_graph, streams=1)
        assert torch.equal(shared, full), use_graph
    assert pipe.engine().step0_shared()[1] > hits0              # the shared logits WERE sampled from
