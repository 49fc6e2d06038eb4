"""Per-image decode state on the GPU (ABI 11): the slots forms of the sampling tail against the scalar entries they restate, and
the contract of paintmind_amd/serve.py -- a request in slot j of an S-slot session computes, bit for bit, what row j of
``Pipeline.generate_ids(B=S, ..., image_base=k - j, use_graph=False, streams=1)`` computes on the unchanged scalar path, whenever
it is admitted and whatever shares the batch with it."""
import numpy as np
import pytest
import torch

import paintmind_amd as pm
from gpu_common import dev, n, t
from oracle import paintmind_oracle as O
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline
from util import load_golden, maxabs, to_torch_sd

pytestmark = pytest.mark.gpu

TOL = 1e-3                      # the north_star tolerance of tests/test_gpu_model.py


# ------------------------------------------------------------------------------------------------------------------------------
# operator level
# ------------------------------------------------------------------------------------------------------------------------------
def _operator_slots(N):
    """(seed, image_index, temperature, topk, num_mask, step) per image; one idle.  Temperature 0, top-k 1 and 8, num_mask 1 and N,
    a row counter beyond 32 bits and a seed with both words set are all in."""
    return [(0x0123456789ABCDEF, 7, 0.0, 1, 1, 0),
            (77, 2 ** 33 + 5, 0.8, 8, N, 3),
            None,
            (0xFEDCBA9876543210, 4096, 1.3, 5, max(N // 2, 1), 17),
            (5, 1, 0.5, 3, 3, 1)]


@pytest.mark.parametrize("V", [64, 8192])
@pytest.mark.parametrize("N", [16, 1024])
def test_slots_operators_match_the_scalar_entries_and_the_restatement(V, N):
    rng = np.random.default_rng(1000 * V + N)
    B, M = 5, 5 * N
    recs = _operator_slots(N)
    logits = (rng.standard_normal((M, V)) * 2.0).astype(np.float32)
    ids = rng.integers(0, V, M).astype(np.int64)
    ids[rng.random(M) < 0.6] = V
    x, ids_t = t(logits), t(ids)
    slots = ops.pack_slots(recs, dev())
    same, stats = ops.guidance_combine(x, x, 1.0, with_stats=True)
    assert torch.equal(same, x)

    dense = ops.sample_rows_slots(x, ids_t, V, slots, N)
    sparse = ops.sample_rows_slots(x, ids_t, V, slots, N, block_stats=stats)
    for a, b in zip(dense, sparse):
        assert torch.equal(a, b)
    pred, merged, score = dense
    remasked = ops.remask_slots(merged.reshape(B, N).clone(), score.reshape(B, N), slots, V)

    cols = np.broadcast_to(np.arange(V), (N, V))
    for b, rec in enumerate(recs):
        r = slice(b * N, (b + 1) * N)
        if rec is None:                                           # idle: nothing drawn, the row keeps its ids
            assert torch.equal(pred[r], ids_t[r]) and torch.equal(merged[r], ids_t[r])
            assert torch.equal(score[r], torch.full((N,), -1e5, device=dev()))
            assert torch.equal(remasked[b], ids_t[r])
            continue
        seed, k, temp, topk, nm, step = rec
        # the scalar entry, this image alone, with and without statistics: bit for bit
        for st in (None, stats[r].contiguous()):
            one = ops.sample_rows(x[r], ids_t[r], V, topk, temp, seed=seed, step=step, row_base=k * N, block_stats=st)
            for got, want in zip((pred[r], merged[r], score[r]), one):
                assert torch.equal(got, want), (b, st is None)
        want = ops.remask(merged[r].reshape(1, N).clone(), score[r].reshape(1, N), nm, V)
        assert torch.equal(remasked[b], want[0]), b
        # the numpy restatement fed this image's Philox uniforms
        rows = np.broadcast_to((np.uint64(k) * np.uint64(N) + np.arange(N, dtype=np.uint64))[:, None], (N, V))
        noise = O.philox_uniform(seed, step, rows, cols)
        pred_r, merged_r, score_r = O.sample_rows(logits[r], ids[r], V, topk, temp, noise)
        assert np.array_equal(n(pred[r]), pred_r) and np.array_equal(n(merged[r]), merged_r)
        assert np.max(np.abs(n(score[r]) - score_r)) < 2e-6
        assert np.array_equal(n(remasked[b]), O.remask(n(merged[r]).reshape(1, N), n(score[r]).reshape(1, N), min(nm, N), V)[0])


# ------------------------------------------------------------------------------------------------------------------------------
# the contract
# ------------------------------------------------------------------------------------------------------------------------------
def reference_run(pipe, S, j, T, temperature, topk, seed, k, ctx_row):
    """row j of the scalar path at B = S: final ids and last image from generate_ids (eager, one stream), the per-step pred and
    score from the scalar one-step entry (pmhip_pipeline_sample: the same kernels), whose ids must end where generate_ids ends."""
    context = None
    if ctx_row is not None:
        context = torch.zeros(S, ctx_row.shape[0], ctx_row.shape[1], device=dev())
        context[j] = ctx_row
    ids_ref, imgs = pipe.generate_ids(context, S, T, temperature, topk, [False] * (T - 1) + [True], seed, image_base=k - j,
                                      use_graph=False, streams=1)
    eng = pipe.engine()
    temps, nmask = pipe._schedule(T, temperature)
    ids = torch.full((S, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long, device=dev())
    preds, scores = [], []
    for step in range(T):
        ids, _, pred, score = eng.sample(None, ids, context, topk, temps[step], nmask[step], seed=seed, step=step, image_base=k - j,
                                         want_img=False, want_aux=True)
        preds.append(pred[j].clone())
        scores.append(score[j].clone())
    assert torch.equal(ids, ids_ref)
    return ids_ref[j].clone(), preds, scores, imgs[0][j].clone()


def run_session(pipe, S, conditional, use_graph, plan, contexts):
    """plan: {tick: [(T, temperature, topk, seed, k), ...]} -> submitted at that tick (before its step).  Returns
    [(request parameters, Finished, the group of Finished it was decoded with)]"""
    s = pipe.decode_session(slots=S, conditional=conditional, use_graph=use_graph, record_steps=True)
    out, tick, number = [], 0, 0
    last = max(plan)
    while tick <= last or not s.idle():
        for req in plan.get(tick, []):
            T, temp, topk, seed, k = req
            h = s.submit(context=contexts[number] if conditional else None, timesteps=T, temperature=temp, topk=topk, seed=seed,
                         image_index=k)
            h.params, h.ctx_row = req, (contexts[number] if conditional else None)
            number += 1
        done = s.step()
        assert s.tick == tick + 1
        out += [(f.handle.params, f, done) for f in done]
        tick += 1
    assert s.idle() and len(out) == number
    return out


def check_contract(pipe, S, conditional, use_graph, plan, contexts, fp32, refs):
    for params, f, group in run_session(pipe, S, conditional, use_graph, plan, contexts):
        T, temp, topk, seed, k = params
        h = f.handle
        assert h.retired == h.admitted + T - 1 and len(h.trace) == T
        key = (params, h.slot)
        if key not in refs:
            refs[key] = reference_run(pipe, S, h.slot, T, temp, topk, seed, k, h.ctx_row)
        ids_ref, preds, scores, img_ref = refs[key]
        for step in range(T):
            assert torch.equal(h.trace[step][0], preds[step]), (params, h.slot, step, "pred")
            assert torch.equal(h.trace[step][1], scores[step]), (params, h.slot, step, "score")
        assert torch.equal(f.ids, ids_ref), (params, h.slot)
        # the image: the decode of the last predictions (the rows that finished together are decoded together)
        together = pipe.vqgan.decode_from_indice(torch.stack([g.handle.trace[-1][0] for g in group]))
        assert torch.equal(f.image, together[[g.handle for g in group].index(h)])
        alone = pipe.vqgan.decode_from_indice(h.trace[-1][0][None])[0]
        err_alone, err_ref = maxabs(n(f.image), n(alone)), maxabs(n(f.image), n(img_ref))
        print(f"{params} slot {h.slot}: image max |session - decoded alone| {err_alone:.2e}, |session - reference run| {err_ref:.2e}")
        if fp32:
            assert err_alone < TOL and err_ref < TOL


@pytest.fixture(scope="module")
def tiny_pipe():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False)
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("text_model") for k in missing.missing_keys)
    return pipe.to(dev()).eval()


# 7 requests, (T, temperature, topk, seed, image index k >= S), admitted staggered into 3 slots
TINY_PLAN = {0: [(6, 1.0, 5, 101, 3), (2, 0.7, 1, 102, 9)],
             1: [(4, 1.3, 3, 103, 4), (7, 0.0, 4, 104, 30)],
             3: [(2, 0.9, 2, 105, 5)],
             6: [(4, 1.0, 5, 106, 2 ** 33 + 1), (6, 0.5, 2, 107, 8)]}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("conditional", [True, False], ids=["conditional", "unconditional"])
def test_session_contract_tiny_pipeline(tiny_pipe, dtype, conditional):
    pipe = tiny_pipe
    contexts = list(pipe.text_model([f"p{i}" for i in range(7)]).to(dev()))
    refs = {}
    try:
        pipe.set_compute_dtype(dtype)
        check_contract(pipe, 3, conditional, False, TINY_PLAN, contexts, dtype == torch.float32, refs)
        # the graph path: this handle's first slots step with the flag runs eagerly, the second captures, the rest replay;
        # a second session then replays from its first step on
        for _ in range(2):
            check_contract(pipe, 3, conditional, True, TINY_PLAN, contexts, dtype == torch.float32, refs)
    finally:
        pipe.set_compute_dtype(torch.float32)


@pytest.fixture(scope="module")
def chain_pipe():
    from gpu_common import scaled_chain_pipeline
    return scaled_chain_pipeline()[0]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_session_contract_full_size(chain_pipe, dtype):
    """12L/d512, 1024 tokens, 8192 classes, trained-like logits; S = 4, T in {4, 8}, admitted at ticks 0 and 2"""
    pipe = chain_pipe
    plan = {0: [(4, 1.0, 5, 201, 4), (8, 1.0, 5, 202, 5), (4, 0.6, 3, 203, 6)],
            2: [(8, 1.2, 8, 204, 7), (4, 1.0, 1, 205, 8), (8, 0.9, 5, 206, 2 ** 32 + 9)]}
    refs = {}
    try:
        pipe.set_compute_dtype(dtype)
        for use_graph in (False, True):
            check_contract(pipe, 4, False, use_graph, plan, None, dtype == torch.float32, refs)
    finally:
        pipe.set_compute_dtype(torch.float32)


def test_uniform_session_equals_generate_ids(tiny_pipe):
    """all slots hold the same parameters and are admitted together: the session IS the batch decode loop"""
    pipe, S, T = tiny_pipe, 3, 6
    ctx = pipe.text_model(["a", "b", "c"]).to(dev())
    for conditional in (True, False):
        want, _ = pipe.generate_ids(ctx if conditional else None, S, T, 0.9, 4, [False] * T, 77, image_base=12, use_graph=True, streams=1)
        for use_graph in (False, True, True):
            s = pipe.decode_session(slots=S, conditional=conditional, use_graph=use_graph)
            for j in range(S):
                s.submit(context=ctx[j] if conditional else None, timesteps=T, temperature=0.9, topk=4, seed=77, image_index=12 + j)
            done = s.drain()
            assert s.tick == T and [f.handle.slot for f in done] == [0, 1, 2]
            assert torch.equal(torch.stack([f.ids for f in done]), want)


def test_generate_ids_start_ids_may_be_a_strided_view(tiny_pipe):
    pipe, N = tiny_pipe, tiny_pipe.num_tokens
    wide = torch.arange(2 * 2 * N, dtype=torch.long, device=dev()).reshape(2, 2 * N) % 65
    view = wide[:, ::2]
    assert not view.is_contiguous()
    a, _ = pipe.generate_ids(None, 2, 4, 1.0, 3, [False] * 4, 5, ids0=view)
    b, _ = pipe.generate_ids(None, 2, 4, 1.0, 3, [False] * 4, 5, ids0=view.contiguous())
    assert torch.equal(a, b) and torch.equal(wide[:, ::2], view)
    with pytest.raises(ValueError):
        pipe.generate_ids(None, 2, 4, 1.0, 3, [False] * 4, 5, ids0=wide)


def test_step_slots_error_paths(tiny_pipe):
    pipe = tiny_pipe
    eng = pipe.engine().clone()                                    # a handle no slots call has touched
    N = pipe.num_tokens
    ids = torch.full((2, N), pipe.mask_token_id, dtype=torch.long, device=dev())
    good = (1, 0, 1.0, 3, 4, 0)

    def records(*recs):
        arr = (_lib.Slot * len(recs))()
        for i, r in enumerate(recs):
            if r is None:
                arr[i].step = _lib.SLOT_IDLE
            else:
                arr[i] = _lib.Slot(*r)
        return arr

    with pytest.raises(_lib.PmhipError) as e:                      # keep-context before any context was prepared
        eng.step_slots(ids, None, records(good, good), keep_context=True)
    assert e.value.code == _lib.PMHIP_ESTATE
    for bad in ((1, 0, 1.0, 9, 4, 0), (1, 0, 1.0, 0, 4, 0), (1, 0, 1.0, 3, 0, 0)):      # topk 9, topk 0, num_mask 0
        with pytest.raises(_lib.PmhipError) as e:
            eng.step_slots(ids, None, records(good, bad))
        assert e.value.code == _lib.PMHIP_EINVAL
    assert torch.equal(ids, torch.full_like(ids, pipe.mask_token_id))          # nothing ran
    # the same values on an IDLE slot are not looked at, and after one prepared step keep-context is served ...
    idle_bad = (1, 0, 1.0, 9, 0, _lib.SLOT_IDLE)
    eng.step_slots(ids, None, records(good, idle_bad))
    assert torch.equal(ids[1], torch.full_like(ids[1], pipe.mask_token_id)) and int((ids[0] != pipe.mask_token_id).sum()) == N - 4
    eng.step_slots(ids, None, records((1, 0, 1.0, 3, 2, 1), None), keep_context=True)
    # ... but not for another batch size, nor after another entry point prepared a context of its own
    with pytest.raises(_lib.PmhipError) as e:
        eng.step_slots(ids[:1].contiguous(), None, records(good), keep_context=True)
    assert e.value.code == _lib.PMHIP_ESTATE
    eng.sample(None, ids.clone(), None, 3, 1.0, 2, want_img=False)
    with pytest.raises(_lib.PmhipError) as e:
        eng.step_slots(ids, None, records(good, good), keep_context=True)
    assert e.value.code == _lib.PMHIP_ESTATE
