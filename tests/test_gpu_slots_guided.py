"""Per-request guidance in decode sessions on the GPU: pmhip_guidance_combine_slots against the scalar combination it restates,
and the contract of paintmind_amd/serve.py with a guidance scale per request -- a request (T, temperature, topk, seed, k, context,
scale s) in slot j of an S-slot conditional session computes, bit for bit, what row j of ``Pipeline.generate_ids(B=S, ...,
image_base=k - j, use_graph=False, streams=1, guidance_scale=s)`` computes on the unchanged scalar path, whenever it is admitted
and whatever mix of guided, unguided and idle slots shares the batch with it."""
import numpy as np
import pytest
import torch

import paintmind_amd as pm
from abi_frames import bits, call, framed
from gpu_common import dev, n, t
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline
from util import load_golden, maxabs, to_torch_sd

pytestmark = pytest.mark.gpu

TOL = 1e-3                      # the north_star tolerance of tests/test_gpu_model.py


# ------------------------------------------------------------------------------------------------------------------------------
# operator level
# ------------------------------------------------------------------------------------------------------------------------------
GUIDES = [3.0, None, 2.0, 0.0, -1.5]                 # image 2 is IDLE: its scale must not be looked at
B_OP = 5


def _operator_slots(N):
    """(seed, image_index, temperature, topk, num_mask, step) per image, image 2 idle"""
    return [(0x0123456789ABCDEF, 7, 0.0, 1, 1, 0), (77, 2 ** 33 + 5, 0.8, 8, N, 3), None,
            (0xFEDCBA9876543210, 4096, 1.3, 5, max(N // 2, 1), 17), (5, 1, 0.5, 3, 3, 1)]


def _guided(b, recs):
    return recs[b] is not None and GUIDES[b] is not None


@pytest.fixture(scope="module")
def operator_case():
    """per shape, computed once and left unchanged: the planes, the records, and per guided image the scalar combination"""
    cache = {}

    def get(V, N):
        if (V, N) not in cache:
            rng = np.random.default_rng(7000 * V + N)
            M = B_OP * N
            cond = t((rng.standard_normal((M, V)) * 2.0).astype(np.float32))
            unc = t((rng.standard_normal((M, V)) * 2.0).astype(np.float32))
            recs = _operator_slots(N)
            same, stats0 = ops.guidance_combine(cond, cond, 1.0, with_stats=True)         # what the logits GEMM would have left
            assert torch.equal(same, cond)
            want = {}
            for b in range(B_OP):
                if _guided(b, recs):
                    r = slice(b * N, (b + 1) * N)
                    want[b] = ops.guidance_combine(cond[r].contiguous(), unc[r].contiguous(), GUIDES[b], with_stats=True)
            ids = rng.integers(0, V, M).astype(np.int64)
            ids[rng.random(M) < 0.6] = V
            cache[(V, N)] = dict(cond=cond, unc=unc, recs=recs, stats0=stats0, want=want, ids=t(ids),
                                 slots=ops.pack_slots(recs, dev()), guides=ops.pack_slot_guides(GUIDES, dev()))
        return cache[(V, N)]
    return get


def _check_planes(case, N, out, prior_out, stats, prior_stats):
    """guided images: the scalar call's bits; every other image: the bytes that were there before"""
    for b in range(B_OP):
        r = slice(b * N, (b + 1) * N)
        if b in case["want"]:
            logits, st = case["want"][b]
            assert torch.equal(bits(out[r]), bits(logits)), b
            if stats is not None:
                assert torch.equal(bits(stats[r]), bits(st)), b
        else:
            assert torch.equal(bits(out[r]), bits(prior_out[r])), b
            if stats is not None:
                assert torch.equal(bits(stats[r]), bits(prior_stats[r])), b


# (64, 5): four rows per wave, image boundaries inside waves; (8192, 64): 10 MiB per plane, the grid-stride loop iterates
SHAPES = [(64, 5), (192, 16), (8192, 16), (8192, 64)]


@pytest.mark.parametrize("with_stats", [True, False], ids=["stats", "plain"])
@pytest.mark.parametrize("in_place", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("V,N", SHAPES)
def test_guidance_combine_slots_matches_the_scalar_combination_per_image(operator_case, V, N, in_place, with_stats):
    case = operator_case(V, N)
    cond, unc = case["cond"], case["unc"]
    if in_place:
        out = cond.clone()
        prior_out = cond
        src = out
    else:
        out = torch.empty_like(cond)
        out.view(torch.int32).fill_(0x5A5A5A5A)                        # a sentinel plane
        prior_out = out.clone()
        src = cond
    stats = case["stats0"].clone() if with_stats else None
    got = ops.guidance_combine_slots(src, unc, case["guides"], case["slots"], N, out=out, block_stats=stats)
    assert (got[0] is out and got[1] is stats) if with_stats else got is out
    _check_planes(case, N, out, prior_out, stats, case["stats0"])
    assert torch.equal(unc, case["unc"]) and (in_place or torch.equal(bits(src), bits(cond)))


@pytest.mark.parametrize("V,N", SHAPES)
def test_guidance_combine_slots_in_place_respects_its_extents(operator_case, V, N):
    """the in-place call through framed buffers: guard bands intact, outputs written in exactly [M, V] and [M, V/64, 2]"""
    case = operator_case(V, N)
    M = B_OP * N
    out = framed(M, V, ld=V, payload=case["cond"], fill="sentinel")
    unc = framed(M, V, ld=V, payload=case["unc"], fill="nan")
    nst = V // 64 * 2
    stats = framed(M, nst, ld=nst, payload=case["stats0"].reshape(M, nst), fill="sentinel")
    slots = framed(B_OP, 32, ld=32, dtype=torch.uint8, payload=case["slots"], fill="sentinel")
    guides = framed(B_OP, 8, ld=8, dtype=torch.uint8, payload=case["guides"], fill="sentinel")
    call("pmhip_guidance_combine_slots", out, unc, guides, slots, N, out, stats, M, V)
    torch.cuda.synchronize()
    for f, what in ((out, "out"), (stats, "block_stats"), (unc, "uncond"), (slots, "slots"), (guides, "guides")):
        f.assert_frame_untouched(what)
    _check_planes(case, N, out.payload(), case["cond"], stats.payload().reshape(M, V // 64, 2), case["stats0"])
    assert torch.equal(bits(unc.payload()), bits(case["unc"]))


@pytest.mark.parametrize("V,N", SHAPES)
def test_sampling_from_the_combined_planes_equals_every_image_alone(operator_case, V, N):
    case = operator_case(V, N)
    out = case["cond"].clone()                                       # in place, like the engine: unguided rows stay the cond tower's
    out, stats = ops.guidance_combine_slots(out, case["unc"], case["guides"], case["slots"], N, out=out, block_stats=case["stats0"].clone())
    out2, stats2 = out.clone(), stats.clone()
    ops.guidance_combine_slots(out2, case["unc"], ops.pack_slot_guides([None] * B_OP, dev()), case["slots"], N, out=out2,
                               block_stats=stats2)                   # nobody guided: nothing moves
    assert torch.equal(bits(out2), bits(out)) and torch.equal(bits(stats2), bits(stats))
    pred, merged, score = ops.sample_rows_slots(out, case["ids"], V, case["slots"], N, block_stats=stats)
    for b, rec in enumerate(case["recs"]):
        if rec is None:
            continue
        r = slice(b * N, (b + 1) * N)
        seed, k, temp, topk, nm, step = rec
        rows = case["want"][b][0] if b in case["want"] else case["cond"][r].contiguous()
        one = ops.sample_rows(rows, case["ids"][r], V, topk, temp, seed=seed, step=step, row_base=k * N)
        for got, want in zip((pred[r], merged[r], score[r]), one):
            assert torch.equal(got, want), b


# ------------------------------------------------------------------------------------------------------------------------------
# the contract
# ------------------------------------------------------------------------------------------------------------------------------
def reference_run(pipe, S, j, T, temperature, topk, seed, k, ctx_row, scale):
    """row j of the scalar path at B = S: final ids and last image from generate_ids (eager, one stream), the per-step pred and
    score from the scalar one-step entry (pmhip_pipeline_sample(_guided): the same kernels), whose ids must end where generate_ids
    ends."""
    context = torch.zeros(S, ctx_row.shape[0], ctx_row.shape[1], device=dev())
    context[j] = ctx_row
    ids_ref, imgs = pipe.generate_ids(context, S, T, temperature, topk, [False] * (T - 1) + [True], seed, image_base=k - j,
                                      use_graph=False, streams=1, guidance_scale=scale)
    eng = pipe.engine()
    temps, nmask = pipe._schedule(T, temperature)
    ids = torch.full((S, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long, device=dev())
    preds, scores = [], []
    for step in range(T):
        ids, _, pred, score = eng.sample(None, ids, context, topk, temps[step], nmask[step], seed=seed, step=step, image_base=k - j,
                                         want_img=False, want_aux=True, guidance_scale=scale)
        preds.append(pred[j].clone())
        scores.append(score[j].clone())
    assert torch.equal(ids, ids_ref)
    return ids_ref[j].clone(), preds, scores, imgs[0][j].clone()


def run_session(pipe, S, use_graph, plan, contexts, plain_entry=False):
    """plan: {tick: [(T, temperature, topk, seed, k, scale), ...]} -> submitted at that tick (before its step).  plain_entry: the
    session steps through pmhip_pipeline_step_slots (no guide records).  Returns ([(request parameters, Finished, the group of
    Finished it was decoded with)], the handle's (one-pass, two-pass) slots steps of this run)"""
    s = pipe.decode_session(slots=S, conditional=True, use_graph=use_graph, record_steps=True)
    if plain_entry:
        s._guides = None
    before = pipe.engine().slots_steps()
    out, tick, number = [], 0, 0
    last = max(plan)
    while tick <= last or not s.idle():
        for req in plan.get(tick, []):
            T, temp, topk, seed, k, scale = req
            h = s.submit(context=contexts[number], timesteps=T, temperature=temp, topk=topk, seed=seed, image_index=k,
                         guidance_scale=scale)
            h.params, h.ctx_row = req, contexts[number]
            number += 1
        done = s.step()
        assert s.tick == tick + 1
        out += [(f.handle.params, f, done) for f in done]
        tick += 1
    assert s.idle() and len(out) == number
    after = pipe.engine().slots_steps()
    return out, (after[0] - before[0], after[1] - before[1])


def check_contract(pipe, S, use_graph, plan, contexts, fp32, refs):
    run, (one_pass, two_pass) = run_session(pipe, S, use_graph, plan, contexts)
    handles = [f.handle for _, f, _ in run]
    ticks = max(h.retired for h in handles) + 1
    busy = [tk for tk in range(ticks) if any(h.admitted <= tk <= h.retired for h in handles)]
    guided = [tk for tk in busy if any(h.admitted <= tk <= h.retired and h.guidance_scale is not None for h in handles)]
    # the host decision: two tower passes exactly in the ticks with an active guided slot
    assert (one_pass, two_pass) == (len(busy) - len(guided), len(guided))
    for params, f, group in run:
        T, temp, topk, seed, k, scale = params
        h = f.handle
        assert h.retired == h.admitted + T - 1 and len(h.trace) == T and h.guidance_scale == scale
        key = (params, h.slot)
        if key not in refs:
            refs[key] = reference_run(pipe, S, h.slot, T, temp, topk, seed, k, h.ctx_row, scale)
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
    return run


@pytest.fixture(scope="module")
def tiny_pipe():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False)
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("text_model") for k in missing.missing_keys)
    return pipe.to(dev()).eval()


# tests/test_gpu_slots.py's TINY_PLAN with a guidance scale per request: 7 requests, (T, temperature, topk, seed, image index
# k >= S, scale), admitted staggered into 3 slots.  Ticks 3 .. 5 hold guided, unguided and idle slots side by side; the last ticks
# hold guided requests only.
TINY_PLAN = {0: [(6, 1.0, 5, 101, 3, 2.5), (2, 0.7, 1, 102, 9, None)],
             1: [(4, 1.3, 3, 103, 4, 0.0), (7, 0.0, 4, 104, 30, 4.0)],
             3: [(2, 0.9, 2, 105, 5, None)],
             6: [(4, 1.0, 5, 106, 2 ** 33 + 1, 1.0), (6, 0.5, 2, 107, 8, 3.0)]}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_guided_session_contract_tiny_pipeline(tiny_pipe, dtype):
    pipe = tiny_pipe
    contexts = list(pipe.text_model([f"p{i}" for i in range(7)]).to(dev()))
    refs = {}
    try:
        pipe.set_compute_dtype(dtype)
        eager = check_contract(pipe, 3, False, TINY_PLAN, contexts, dtype == torch.float32, refs)
        # guidance did something: a guided request's ids differ from its unguided twin's
        params, f, _ = next(x for x in eager if x[0][5] == 2.5)
        twin = reference_run(pipe, 3, f.handle.slot, *params[:5], f.handle.ctx_row, None)
        assert not torch.equal(f.ids, twin[0])
        # the graph path: the first two-pass step with the flag runs eagerly, the second captures, the rest replay (likewise the
        # one-pass steps, under their own key); a second session then replays from its first step on
        for _ in range(2):
            check_contract(pipe, 3, True, TINY_PLAN, contexts, dtype == torch.float32, refs)
    finally:
        pipe.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_an_unguided_session_is_the_plain_slots_step(tiny_pipe, use_graph):
    """no request guided: the guided entry runs exactly pmhip_pipeline_step_slots -- the same results, no second tower pass"""
    pipe = tiny_pipe
    contexts = list(pipe.text_model([f"p{i}" for i in range(7)]).to(dev()))
    plan = {tick: [r[:5] + (None,) for r in reqs] for tick, reqs in TINY_PLAN.items()}
    runs = []
    for plain_entry in (True, False, False):
        run, (one_pass, two_pass) = run_session(pipe, 3, use_graph, plan, contexts, plain_entry=plain_entry)
        assert two_pass == 0 and one_pass == max(f.handle.retired for _, f, _ in run) + 1
        runs.append(run)
    for other in runs[1:]:
        for (pa, fa, _), (pb, fb, _) in zip(runs[0], other):
            assert pa == pb and fa.handle.slot == fb.handle.slot
            assert torch.equal(fa.ids, fb.ids) and torch.equal(fa.image, fb.image)
            for (p1, s1), (p2, s2) in zip(fa.handle.trace, fb.handle.trace):
                assert torch.equal(p1, p2) and torch.equal(s1, s2)


def _same_session_runs(got, want):
    for (pa, fa, _), (pb, fb, _) in zip(got, want):
        assert pa == pb and fa.handle.slot == fb.handle.slot and len(fa.handle.trace) == len(fb.handle.trace)
        assert torch.equal(fa.ids, fb.ids) and torch.equal(fa.image, fb.image)
        for (p1, s1), (p2, s2) in zip(fa.handle.trace, fb.handle.trace):
            assert torch.equal(p1, p2) and torch.equal(s1, s2)
    assert len(got) == len(want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_session_and_generate_graphs_share_one_handle_through_workspace_growth(tiny_pipe, dtype):
    """The slots step and Pipeline.generate capture into ONE handle's graph cache, on its one capture stream, and every graph
    bakes workspace pointers in: a guided step that allocates "s2.logits_u" / "slots.guides", and a session of twice the slots
    that grows every "s2.*" buffer, leave the graphs captured before them stale.  Each run -- first eager, then captured, then
    replayed, then re-captured after the growth -- must give the bits of its eager (use_graph=False) run."""
    pipe = tiny_pipe
    contexts = list(pipe.text_model([f"p{i}" for i in range(7)]).to(dev()))
    texts = ["a", "b", "c"]
    # (T, temperature, topk, seed, image index, scale): 4 steps of 3 slots = eager, capture, replay, replay
    plain3 = {0: [(4, 1.0, 5, 301, 3, None), (4, 0.7, 2, 302, 4, None), (4, 1.2, 8, 303, 5, None)]}
    plain6 = {0: [(3, 1.0, 5, 310 + i, 6 + i, None) for i in range(6)]}

    def generate(use_graph):
        imgs, ids = pipe.generate(texts, timesteps=4, topk=3, save_interval=2, seed=21, return_ids=True, use_graph=use_graph, streams=1)
        return [im.clone() for im in imgs], ids.clone()

    def runs(use_graph):
        out = {"a": run_session(pipe, 3, use_graph, plain3, contexts)[0],
               "b": run_session(pipe, 3, use_graph, TINY_PLAN, contexts)[0],
               "c": [generate(use_graph) for _ in range(3)],
               "d": run_session(pipe, 6, use_graph, plain6, contexts)[0]}
        if use_graph:                                                  # every graph captured so far now holds stale pointers
            out["e"] = (run_session(pipe, 3, True, plain3, contexts)[0], run_session(pipe, 3, True, TINY_PLAN, contexts)[0],
                        [generate(True) for _ in range(3)])
        return out

    try:
        pipe.set_compute_dtype(dtype)
        want = runs(False)
        assert all(torch.equal(i1, i2) for i1, i2 in zip(want["c"][0][0], want["c"][1][0])) and torch.equal(want["c"][0][1], want["c"][1][1])
        pipe.invalidate_engines()                                      # one fresh engine pair: nothing sized, nothing captured
        got = runs(True)
        for a, b, c in ((got["a"], got["b"], got["c"]), got["e"]):
            _same_session_runs(a, want["a"])
            _same_session_runs(b, want["b"])
            for imgs, ids in c:
                assert torch.equal(ids, want["c"][0][1]) and len(imgs) == len(want["c"][0][0]) == 2
                assert all(torch.equal(i1, i2) for i1, i2 in zip(imgs, want["c"][0][0]))
        _same_session_runs(got["d"], want["d"])
    finally:
        pipe.set_compute_dtype(torch.float32)
        pipe.invalidate_engines()


def _records(*recs):
    arr = (_lib.Slot * len(recs))()
    for i, r in enumerate(recs):
        if r is None:
            arr[i].step = _lib.SLOT_IDLE
        else:
            arr[i] = _lib.Slot(*r)
    return arr


def _guide_records(*scales):
    arr = (_lib.SlotGuide * len(scales))()
    for i, sc in enumerate(scales):
        if sc is not None:
            arr[i] = _lib.SlotGuide(sc, 1)
    return arr


def test_guided_step_error_paths(tiny_pipe):
    pipe = tiny_pipe
    eng = pipe.engine().clone()                                    # a handle no slots call has touched
    N = pipe.num_tokens
    ids = torch.full((2, N), pipe.mask_token_id, dtype=torch.long, device=dev())
    start = ids.clone()
    good = (1, 0, 1.0, 3, 4, 0)
    ctx = pipe.text_model(["a", "b"]).to(dev())

    def refused(context, keep, guides, recs=None):
        with pytest.raises(_lib.PmhipError) as e:
            eng.step_slots(ids, context, recs or _records(good, good), keep_context=keep, guides=guides)
        return e.value

    # no context at all, without and with keep-context in force (nothing prepared, then prepared WITHOUT a context)
    for keep in (False, True):
        e = refused(None, keep, _guide_records(None, 2.0))
        assert e.code == _lib.PMHIP_EINVAL and "guidance needs a context" in str(e)
    eng.step_slots(ids.clone(), None, _records(good, good))
    e = refused(None, True, _guide_records(2.0, None))
    assert e.code == _lib.PMHIP_EINVAL and "guidance needs a context" in str(e)
    e = refused(ctx, False, _guide_records(float("nan"), None))
    assert e.code == _lib.PMHIP_EINVAL and "finite" in str(e)
    assert torch.equal(ids, start) and eng.slots_steps() == (1, 0)             # nothing of the refused calls ran
    # the same values on an IDLE slot are not looked at: one tower pass, and the step is the plain one
    one = ids.clone()
    eng.step_slots(one, None, _records(good, None), guides=_guide_records(None, float("nan")))
    plain = ids.clone()
    eng.step_slots(plain, None, _records(good, None))
    assert torch.equal(one, plain) and eng.slots_steps() == (3, 0)
    # with a context the guided step runs, and keep-context then serves a guided step too
    eng.step_slots(ids, ctx, _records(good, good), guides=_guide_records(2.0, None))
    eng.step_slots(ids, ctx, _records((1, 0, 1.0, 3, 2, 1), (1, 0, 1.0, 3, 2, 1)), keep_context=True, guides=_guide_records(2.0, 1.0))
    assert eng.slots_steps() == (3, 2)
    with pytest.raises(ValueError):
        eng.step_slots(ids, ctx, _records(good, good), guides=_guide_records(2.0))


@pytest.fixture(scope="module")
def chain_pipe():
    from gpu_common import scaled_chain_pipeline
    return scaled_chain_pipeline()[0]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_guided_session_contract_full_size(chain_pipe, dtype):
    """12L/d512, 1024 tokens, 8192 classes, trained-like logits, a seeded random [77, 512] context per request; S = 4, T in {4, 8},
    admitted at ticks 0 and 2"""
    pipe = chain_pipe
    plan = {0: [(4, 1.0, 5, 201, 4, 3.0), (8, 1.0, 5, 202, 5, None), (4, 0.6, 3, 203, 6, 1.5)],
            2: [(8, 1.2, 8, 204, 7, None), (4, 1.0, 1, 205, 8, 0.0), (8, 0.9, 5, 206, 2 ** 32 + 9, 5.0)]}
    g = torch.Generator().manual_seed(77)
    contexts = [torch.randn(77, 512, generator=g).to(dev()) for _ in range(6)]
    refs = {}
    try:
        pipe.set_compute_dtype(dtype)
        for use_graph in (False, True):
            check_contract(pipe, 4, use_graph, plan, contexts, dtype == torch.float32, refs)
    finally:
        pipe.set_compute_dtype(torch.float32)
