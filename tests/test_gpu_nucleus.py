"""The nucleus (top-p) filter on the GPU: sample_nucleus_kernel against the float64 restatement of
tests/nucleus_ref.py in every size class, at the mass threshold of every row, at plateaus of equal weights, against the row kernels'
confidence bits, on the Philox stream, through the C entry with strides and aliasing, and through every form of the engine's step
-- the engine cases bit for bit.

Against the restatement a row's prediction must be the winner over MUST plus some prefix (in the kept order) of the band MAY \\ MUST
(nucleus_ref.check: the kernel's fp32 sums may put an element whose mass above lies within 1e-4 Z of the cut on either side),
the merged id must follow and the score lie within rtol 1e-4 / atol 1e-6.  No row is exempt.  The inputs were chosen on the CPU so
that no allowed draw is decided by less than 1e-5 relative in perturbed value (where device and numpy logarithms may round apart):
nucleus_ref.check asserts that about the inputs before it looks at the result.
"""
import copy
import itertools

import numpy as np
import pytest
import torch

import nucleus_ref as R
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
TOPKS = [1, 5, 8, 9, 64, 65, None]                           # None: V.  Both sides of the other kernels' limits: all one kernel here
PS = [1e-3, 0.1, 0.5, 0.9, 1 - 2.0 ** -20]
TEMPS = [0.0, 0.3, 1.0, 2.5]
SCALES = [0.5, 3.0, 20.0]
NEAR_ONE = F(1.0 - 2.0 ** -24)                               # gumbel = 16.6: wins against everything, if it is kept at all
SEED0 = 9000                                                 # (the size-class inputs: chosen on the CPU, see the module docstring)


def size_class_cases(V):
    """(M, topk, top_p, temperature, scale, logits, ids, noise) for one class count: every (M, topk, top_p), the temperature and
    the logit scale rotating through all their 12 combinations along the way; inputs from one seed per V"""
    rng = np.random.default_rng(SEED0 + V)
    for i, (M, topk, p) in enumerate(itertools.product(ROWS, TOPKS, PS)):
        temp, scale = TEMPS[i % 4], SCALES[(i // 4) % 3]
        logits = (rng.standard_normal((M, V)) * scale).astype(F)
        ids = rng.integers(0, V + 1, M).astype(np.int64)        # V = mask id
        noise = rng.random((M, V)).astype(F)
        yield M, V if topk is None else topk, p, temp, scale, logits, ids, noise


def run(logits, ids, V, topk, top_p, temp, noise=None, **kw):
    return tuple(n(x) for x in ops.sample_rows(t(logits), t(ids), V, topk, temp, noise=None if noise is None else t(noise), top_p=top_p, **kw))


# ------------------------------------------------------------------------------------------------------------------------------
# a. every size class
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", SIZES)
def test_size_classes_against_the_restatement(V):
    banded = rows = 0
    for M, topk, p, temp, scale, logits, ids, noise in size_class_cases(V):
        got = run(logits, ids, V, topk, p, temp, noise)
        banded += R.check(got, logits, ids, V, topk, p, temp, noise, (V, M, topk, p, temp, scale))
        rows += M
    print(f"V={V}: {banded} of {rows} rows had a non-empty band")


# ------------------------------------------------------------------------------------------------------------------------------
# b. the threshold of every row, from both sides
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("V,topk", [(8192, 8192), (8192, 1024), (1028, 1028), (1028, 1024)])
def test_boundary_probes_pin_the_threshold_into_the_band(V, topk, p):
    """u = 0.5 everywhere but on one column, which gets the best noise there is: the last MUST element is drawn; the first element
    outside MAY is not (the row's first maximum is, as u = 0.5 gives).  Logits of scale 1.5: no logit is 16 below the maximum, so
    the hot column wins whenever it is kept."""
    M = 9
    rng = np.random.default_rng(V + topk + int(100 * p))
    logits = (rng.standard_normal((M, V)) * 1.5).astype(F)
    assert (logits.max(1) - logits.min(1)).max() < 16.0
    ids = np.full(M, V, np.int64)
    _, must, may, order = R.sets(logits, topk, p)
    first_max = logits.argmax(1)
    last_must = np.array([[c for c in order[r] if must[r, c]][-1] for r in range(M)])
    full = O.order_desc_then_index(logits)                      # an element outside MAY: inside K where there is one, else K's successor
    first_out = np.array([[c for c in full[r] if not may[r, c]][0] for r in range(M)])
    for hot, want in ((last_must, last_must), (first_out, first_max)):
        noise = np.full((M, V), 0.5, F)
        noise[np.arange(M), hot] = NEAR_ONE
        pred, merged, score = run(logits, ids, V, topk, p, 1.0, noise)
        assert np.array_equal(pred, want), (V, topk, p, np.flatnonzero(pred != want))
        assert np.array_equal(merged, want)
        assert np.allclose(score, 1 - O.softmax(logits)[np.arange(M), want], rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------------------
# c. plateaus of equal weights
# ------------------------------------------------------------------------------------------------------------------------------
PLATEAU, ABOVE = 40, 70


def plateau_row(V, seed):
    """quantised logits: ABOVE elements (3, 4 or 5) above a plateau of PLATEAU values 2.0, everything else integers <= 1;
    -> (row [V], the plateau's columns ascending, a column of the next lower value).  The plateau covers all four components of a
    float4 and, beyond V = 256, several lanes and groups."""
    rng = np.random.default_rng(seed)
    row = np.round(rng.standard_normal(V) * 2).astype(F).clip(-6, 1)
    while True:
        pick = rng.permutation(V)[:PLATEAU + ABOVE]
        pl = np.sort(pick[:PLATEAU])
        if len({int(c) & 3 for c in pl}) == 4 and len({int(c) >> 8 for c in pl}) >= min(4, V // 256):
            break
    row[pl] = 2.0
    row[pick[PLATEAU:]] = rng.integers(3, 6, ABOVE).astype(F)
    lower = int(np.flatnonzero(row == 1.0)[0])
    return row, pl, lower


def hot_rows(row, cols):
    """one copy of the row per column of `cols`, u = 0.5 but for that column"""
    M, V = len(cols), len(row)
    noise = np.full((M, V), 0.5, F)
    noise[np.arange(M), cols] = NEAR_ONE
    return np.tile(row, (M, 1)), np.full(M, V, np.int64), noise


@pytest.mark.parametrize("V", [8192, 260])
def test_a_plateau_is_kept_or_dropped_whole(V):
    row, pl, lower = plateau_row(V, 50 + V)
    w = np.exp(row.astype(np.float64) - row.max())
    Z, front, mass = w.sum(), w[row > 2.0].sum(), w[row == 2.0].sum()
    first_max = int(row.argmax())
    probe = np.append(pl, lower)
    logits, ids, noise = hot_rows(row, probe)
    inside, just_above, just_below = (front + mass / 2) / Z, (front + 15 * R.DELTA * Z) / Z, (front - 15 * R.DELTA * Z) / Z
    assert F(just_above) * Z - front >= 10 * R.DELTA * Z and front - F(just_below) * Z >= 10 * R.DELTA * Z and just_above < inside
    for p in (inside, just_above):                               # the cut inside the plateau, or just behind its front: all 40 drawable
        pred, _, _ = run(logits, ids, V, V, float(F(p)), 1.0, noise)
        assert np.array_equal(pred[:PLATEAU], pl), p
        assert pred[PLATEAU] == first_max                        # ... and the next lower value is not
    pred, _, _ = run(logits, ids, V, V, float(F(just_below)), 1.0, noise)
    assert (pred == first_max).all()                             # the cut just in front of it: none of the plateau


@pytest.mark.parametrize("V", [8192, 260])
def test_the_plateau_rule_composes_with_a_topk_that_cuts_it_by_column(V):
    row, pl, lower = plateau_row(V, 60 + V)
    r = 20
    w = np.exp(row.astype(np.float64) - row.max())
    front, each = w[row > 2.0].sum(), w[pl[0]]
    Zk = front + r * each                                        # the mass of K = ABOVE + the r lowest columns of the plateau
    first_max = int(row.argmax())
    logits, ids, noise = hot_rows(row, pl)
    pred, _, _ = run(logits, ids, V, ABOVE + r, float(F((front + r * each / 2) / Zk)), 1.0, noise)
    assert np.array_equal(pred[:r], pl[:r])                      # the top-k's columns of the plateau: kept whole by the weight rule
    assert (pred[r:] == first_max).all()                         # the others fell to the top-k: never drawn
    pred, _, _ = run(logits, ids, V, ABOVE + r, float(F((front - 15 * R.DELTA * Zk) / Zk)), 1.0, noise)
    assert (pred == first_max).all()


# ------------------------------------------------------------------------------------------------------------------------------
# d. the normaliser is the row kernels': the same confidence bits
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [8192, 1028])
def test_confidence_bits_continue_the_row_kernels(V):
    M = 9
    rng = np.random.default_rng(V)
    logits = t((rng.standard_normal((M, V)) * 3).astype(F))
    ids = torch.full((M,), V, dtype=torch.long, device=dev())
    noise = torch.full((M, V), 0.5, device=dev())
    refs = [ops.sample_rows(logits, ids, V, k, 0.7, noise=noise) for k in (64, 65)]       # sample_rows_kernel, sample_wide_kernel
    assert torch.equal(refs[0][0], logits.argmax(1))
    for k, p in itertools.product((1, 5, 9, 64, 65, V - 1, V), (1e-3, 0.5, 0.9, 1 - 2.0 ** -20)):
        got = ops.sample_rows(logits, ids, V, k, 0.7, noise=noise, top_p=p)
        for ref in refs:
            for a, b in zip(got, ref):
                assert torch.equal(bits(a), bits(b)), (k, p)


# ------------------------------------------------------------------------------------------------------------------------------
# e. the Philox stream; strides, aliasing, -inf; top_p = 1
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,row_base", [(1028, 2 ** 32 + 77), (8192, 2 ** 40 + 3)])
def test_philox_stream_is_the_oracles(V, row_base):
    M, seed, step = 9, 0xFEDCBA9876543210, 5
    rng = np.random.default_rng(V + 2)
    logits = (rng.standard_normal((M, V)) * 2).astype(F)
    ids = rng.integers(0, V + 1, M).astype(np.int64)
    u = O.philox_uniform(seed, step, (row_base + np.arange(M, dtype=np.uint64))[:, None], np.arange(V, dtype=np.uint64)[None, :])
    for k, p in ((V, 0.9), (100, 0.5)):
        got = run(logits, ids, V, k, p, 1.0, seed=seed, step=step, row_base=row_base)
        R.check(got, logits, ids, V, k, p, 1.0, u, (V, k, p))
        given = run(logits, ids, V, k, p, 1.0, u)
        assert all(np.array_equal(a, b) for a, b in zip(got, given))       # the same uniforms, bit for bit, whichever way they come


@pytest.mark.parametrize("V,topk,p", [(1028, 100, 0.5), (8192, 8192, 0.9), (260, 259, 0.1)])
def test_strided_logits_and_ids_in_place_through_the_c_entry(V, topk, p):
    M = 9
    rng = np.random.default_rng(3 * V + 1)
    logits = (rng.standard_normal((M, V)) * 3).astype(F)
    ids = rng.integers(0, V + 1, M).astype(np.int64)
    noise = rng.random((M, V)).astype(F)
    fx = framed(M, V, dtype=torch.float32, payload=t(logits), fill="nan")             # ld > V, NaN in the gap and around
    fi = framed(M, 1, ld=1, dtype=torch.int64, payload=t(ids).reshape(M, 1))          # ids_in AND ids_out
    fp = framed(M, 1, ld=1, dtype=torch.int64, device=dev())
    fs = framed(M, 1, ld=1, dtype=torch.float32, device=dev())
    call("pmhip_sample_rows_nucleus", fx, fx.ld, fi, V, topk, p, 0.8, t(noise), 0, 0, 0, fp, fi, fs, M, V)
    for f, what in ((fx, "logits"), (fi, "ids"), (fp, "pred"), (fs, "score")):
        f.assert_frame_untouched(what)
    got = (n(fp.payload().reshape(M)), n(fi.payload().reshape(M)), n(fs.payload().reshape(M)))
    R.check(got, logits, ids, V, topk, p, 0.8, noise, (V, topk, p))


@pytest.mark.parametrize("temp", [0.0, 1.0])
def test_rows_of_minus_infinity(temp):
    V, M, finite = 1028, 5, 70
    rng = np.random.default_rng(12)
    logits = np.full((M, V), -np.inf, F)
    noise = rng.random((M, V)).astype(F)
    for m in range(M):
        cols = rng.permutation(V)[:finite]
        logits[m, cols] = rng.standard_normal(finite).astype(F) * 2
        noise[m, int(np.flatnonzero(np.isinf(logits[m]))[0])] = NEAR_ONE   # a weight of 0 with the best noise there is: never kept
    ids = np.full(M, V, np.int64)
    for k, p in ((100, 1 - 2.0 ** -20), (V, 0.9), (5, 0.5)):
        got = run(logits, ids, V, k, p, temp, noise)
        R.check(got, logits, ids, V, k, p, temp, noise, (temp, k, p))
        assert np.isfinite(logits[np.arange(M), got[0]]).all()


@pytest.mark.parametrize("topk", [5, 64, 100])
def test_top_p_one_through_the_new_entry_is_the_old_entry(topk):
    M, V = 9, 1024
    rng = np.random.default_rng(topk)
    logits, ids, noise = t((rng.standard_normal((M, V)) * 3).astype(F)), t(rng.integers(0, V + 1, M).astype(np.int64)), t(rng.random((M, V)).astype(F))
    want = ops.sample_rows(logits, ids, V, topk, 0.8, noise=noise)
    outs = [torch.empty(M, dtype=torch.int64, device=dev()), torch.empty(M, dtype=torch.int64, device=dev()), torch.empty(M, device=dev())]
    call("pmhip_sample_rows_nucleus", logits, V, ids, V, topk, 1.0, 0.8, noise, 0, 0, 0, outs[0], outs[1], outs[2], M, V)
    for a, b in zip(outs, want):
        assert torch.equal(bits(a), bits(b))
    for a, b in zip(ops.sample_rows(logits, ids, V, topk, 0.8, noise=noise, top_p=1.0), want):
        assert torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------------------------
# f. through the engine: a tiny pipeline with 256 classes (the recipe of tests/test_gpu_topk_wide.py)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide_pipe():
    vq = copy.deepcopy(pm.ver2cfg["tiny-vqgan"])
    vq["n_embed"] = 256
    pm.ver2cfg["tiny-vqgan-256n"] = vq
    pm.ver2cfg["tiny-pipeline-256n"] = dict(pm.ver2cfg["tiny-pipeline"], stage1="tiny-vqgan-256n")
    try:
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(256)
            pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline-256n"]), stage1_pretrained=False)
            pipe.transformer.to_logits.weight.data.mul_(2.0)   # rows of which 30 % of the mass is 4 classes and 70 % is 31: top_p matters
        yield pipe.to(dev()).eval()
    finally:
        del pm.ver2cfg["tiny-vqgan-256n"], pm.ver2cfg["tiny-pipeline-256n"]


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


def _compose(pipe, ids0, logits, k, p, temperature, nm, noise=None, seed=0, step=0, image_base=0, choice_temperature=0.0):
    B, N, V = ids0.shape[0], pipe.num_tokens, pipe.mask_token_id
    if noise is not None:
        noise = noise.reshape(B * N, V)
    _, merged, score = ops.sample_rows(logits.reshape(B * N, V), ids0.reshape(-1), V, k, temperature, noise=noise, seed=seed, step=step,
                                       row_base=image_base * N, top_p=p)
    return ops.remask(merged.reshape(B, N), score.reshape(B, N), nm, V, choice_temperature=choice_temperature, seed=seed, step=step,
                      row_base=image_base * N)


def test_sample_equals_the_operator_composition(pipe):
    B, N, V = 3, pipe.num_tokens, pipe.mask_token_id
    assert V == 256
    ctx = pipe.text_model(["a", "b", "c"]).to(dev())
    ids0 = _start(pipe, B)
    noise = torch.rand(B, N, V, generator=torch.Generator().manual_seed(4)).to(dev())
    nm = num_token_masked(np.float64(0.5), N)
    for text in (ctx, None):
        logits = pipe.engine().forward(pipe.ids2tokens(ids0), text)
        for k in (5, 100, None):
            got, img = pipe.sample(ids0, np.float64(0.5), text=text, topk=k, temperature=0.8, noise=noise, top_p=0.5)
            assert torch.equal(got, _compose(pipe, ids0, logits, V if k is None else k, 0.5, 0.8, nm, noise=noise)), k
            assert img.shape[0] == B and bool(torch.isfinite(img).all())


def _loop_of_samples(pipe, context, B, T, temperature, topk, seed, base, **kw):
    """the loop as one native step per call, under the loop's seed"""
    temps, nmask = pipe._schedule(T, temperature)
    ids = pipe._start_ids(B, None, dev())
    eng = pipe.engine()
    for step in range(T):
        ids, _, _, _ = eng.sample(None, ids, context, topk, temps[step], nmask[step], seed=seed, step=step, image_base=base, want_img=False, **kw)
    return ids


def test_generate_ids_eager_graph_and_step_loop_agree(pipe):
    B, T, k = 4, 4, 200
    context = pipe.text_model(["a", "b", "c", "d"]).to(dev())
    flags = [False] * T
    want = {p: _loop_of_samples(pipe, context, B, T, 1.0, k, 77, 12, top_p=p) for p in (0.7, 0.3)}
    assert not torch.equal(want[0.7], want[0.3])
    eager, _ = pipe.generate_ids(context, B, T, 1.0, k, flags, 77, image_base=12, use_graph=False, streams=1, top_p=0.7)
    assert torch.equal(eager, want[0.7])
    # two values, two graphs: captured and replayed in turn, neither ever answers for the other
    for _ in range(3):                                           # eager once, capture, replay
        for p in (0.7, 0.3):
            graph, _ = pipe.generate_ids(context, B, T, 1.0, k, flags, 77, image_base=12, use_graph=True, streams=1, top_p=p)
            assert torch.equal(graph, want[p]), p
    lanes, _ = pipe.generate_ids(context, B, T, 1.0, k, flags, 77, image_base=12, use_graph=True, streams=2, top_p=0.7)
    assert torch.equal(lanes, want[0.7])


def test_top_p_none_loops_are_the_calls_without_the_keyword(pipe):
    B, T = 3, 3
    context = pipe.text_model(["a", "b", "c"]).to(dev())
    flags = [False] * T
    for k in (5, 100):
        for use_graph in (False, True, True):
            old, _ = pipe.generate_ids(context, B, T, 1.0, k, flags, 21, image_base=2, use_graph=use_graph, streams=1)
            for p in (None, 1.0):
                new, _ = pipe.generate_ids(context, B, T, 1.0, k, flags, 21, image_base=2, use_graph=use_graph, streams=1, top_p=p)
                assert torch.equal(new, old), (k, use_graph, p)
        ids0 = _start(pipe, B, 1)
        old, img_old = pipe.sample(ids0, np.float64(0.5), text=context, topk=k, temperature=0.8, seed=4, step=1)
        for p in (None, 1.0):
            new, img_new = pipe.sample(ids0, np.float64(0.5), text=context, topk=k, temperature=0.8, seed=4, step=1, top_p=p)
            assert torch.equal(new, old) and torch.equal(img_new, img_old)


@pytest.mark.parametrize("mode", ["guided", "choice", "context_lens"])
def test_other_step_forms_equal_their_compositions(pipe, mode):
    B, N, V, k, p = 3, pipe.num_tokens, pipe.mask_token_id, 100, 0.6
    ctx = pipe.text_model(["a", "b", "c"]).to(dev())
    ids0 = _start(pipe, B, 2)
    nm = num_token_masked(np.float64(0.5), N)
    tok = pipe.ids2tokens(ids0)
    eng = pipe.engine()
    common = dict(text=ctx, topk=k, temperature=0.8, seed=9, step=2, image_base=5, top_p=p)
    if mode == "guided":
        got, _ = pipe.sample(ids0, np.float64(0.5), guidance_scale=2, **common)
        logits = ops.guidance_combine(eng.forward(tok, ctx), eng.forward(tok, None), 2.0)
        want = _compose(pipe, ids0, logits, k, p, 0.8, nm, seed=9, step=2, image_base=5)
    elif mode == "choice":
        got, _ = pipe.sample(ids0, np.float64(0.5), choice_temperature=4.5, **common)
        want = _compose(pipe, ids0, eng.forward(tok, ctx), k, p, 0.8, nm, seed=9, step=2, image_base=5, choice_temperature=4.5)
    else:
        L = ctx.shape[1]
        lens = [1, L, min(2, L)]
        got, _ = pipe.sample(ids0, np.float64(0.5), context_lens=lens, **common)
        want = _compose(pipe, ids0, eng.forward(tok, ctx, context_lens=lens), k, p, 0.8, nm, seed=9, step=2, image_base=5)
    assert torch.equal(got, want)


def test_shared_step0_logits_serve_the_nucleus_kernel(pipe):
    """an unconditional loop from the all-mask state samples its step 0 from ONE image's logits (the PERIOD form of the kernel);
    an explicit all-mask start keeps the full path: the same ids"""
    B, T, k, p = 5, 3, 200, 0.8
    flags = [False] * T
    full, _ = pipe.generate_ids(None, B, T, 1.0, k, flags, 31, image_base=3, use_graph=False, streams=1, ids0=pipe._start_ids(B, None, dev()),
                                top_p=p)
    hits0 = pipe.engine().step0_shared()[1]
    for use_graph in (False, False, True, True, True):
        shared, _ = pipe.generate_ids(None, B, T, 1.0, k, flags, 31, image_base=3, use_graph=use_graph, streams=1, top_p=p)
        assert torch.equal(shared, full), use_graph
    assert pipe.engine().step0_shared()[1] > hits0              # the shared logits WERE sampled from
