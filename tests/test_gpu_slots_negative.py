"""A negative prompt and a guidance schedule per request in decode sessions, on the GPU: pmhip_guidance_combine_slots_which against
the scalar combination it restates, and the contract of paintmind_amd/serve.py -- a request (T, temperature, topk, seed, k, context,
scale or schedule s, negative n of Ln_r rows) in slot j of an S-slot session computes, bit for bit, what row j of
``Pipeline.generate_ids(B=S, ..., image_base=k - j, use_graph=False, streams=1, guidance_scale=s, negative_context=[S, capacity_n, D]
with n in row j, negative_lens with Ln_r in row j)`` computes on the unchanged scalar path, whatever shares the batch with it."""
import ctypes as C

import numpy as np
import pytest
import torch

from abi_frames import bits
from gpu_common import dev, n, t
from paintmind_amd import _lib, ops
from test_gpu_slots_guided import SHAPES, TOL, _records, chain_pipe, tiny_pipe  # noqa: F401  (the two are fixtures)
from util import maxabs

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------------------
# operator level
# ------------------------------------------------------------------------------------------------------------------------------
B_OP = 5
# (scale, on) per image; image 2 is IDLE: its record (on = 2) must not be looked at.  One on = 0, two on = 1, one on = 2; the scales
# differ and include 0 and a negative value
KINDS = [(3.0, 1), (9.0, 0), (7.0, 2), (0.0, 1), (-1.5, 2)]
IDLE = 2


def _slots(N):
    return [(0x0123456789ABCDEF, 7, 0.0, 1, 1, 0), (77, 2 ** 33 + 5, 0.8, 8, N, 3), None,
            (0xFEDCBA9876543210, 4096, 1.3, 5, max(N // 2, 1), 17), (5, 1, 0.5, 3, 3, 1)]


def _guides(kinds):
    return ops.pack_slot_guides([sc for sc, _ in kinds], dev(), kinds=[on for _, on in kinds])


def _sentinel_like(x):
    out = torch.empty_like(x)
    out.view(torch.int32).fill_(0x5A5A5A5A)
    return out


@pytest.fixture(scope="module")
def operator_case():
    """per shape, computed once and left unchanged: the planes, the records, and per active guided image the scalar combination,
    with and without statistics"""
    cache = {}

    def get(V, N):
        if (V, N) not in cache:
            rng = np.random.default_rng(9000 * V + N)
            M = B_OP * N
            cond = t((rng.standard_normal((M, V)) * 2.0).astype(np.float32))
            other = t((rng.standard_normal((M, V)) * 2.0).astype(np.float32))
            want = {}
            for b, (scale, on) in enumerate(KINDS):
                if b != IDLE and on:
                    r = slice(b * N, (b + 1) * N)
                    c, o = cond[r].contiguous(), other[r].contiguous()
                    want[b] = (ops.guidance_combine(c, o, scale), ops.guidance_combine(c, o, scale, with_stats=True))
            cache[(V, N)] = dict(cond=cond, other=other, want=want, slots=ops.pack_slots(_slots(N), dev()), guides=_guides(KINDS))
        return cache[(V, N)]
    return get


@pytest.mark.parametrize("with_stats", [True, False], ids=["stats", "plain"])
@pytest.mark.parametrize("in_place", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("V,N", SHAPES)
def test_combine_of_one_kind_matches_the_scalar_combination_and_leaves_the_rest(operator_case, V, N, which, in_place, with_stats):
    case = operator_case(V, N)
    cond, other = case["cond"], case["other"]
    out = cond.clone() if in_place else _sentinel_like(cond)
    prior = out.clone()
    stats = _sentinel_like(torch.empty(B_OP * N, V // 64, 2, device=dev())) if with_stats else None
    prior_stats = stats.clone() if with_stats else None
    got = ops.guidance_combine_slots(out if in_place else cond, other, case["guides"], case["slots"], N, out=out, block_stats=stats,
                                     which=which)
    assert (got[0] is out and got[1] is stats) if with_stats else got is out
    combined = [b for b, (_, on) in enumerate(KINDS) if b != IDLE and on == which]
    assert combined == ([0, 3] if which == 1 else [4])
    for b in range(B_OP):
        r = slice(b * N, (b + 1) * N)
        if b in combined:
            plain, (logits, st) = case["want"][b]
            assert torch.equal(bits(logits), bits(plain))                # the scalar call's logits do not depend on with_stats
            assert torch.equal(out[r], logits) and torch.equal(bits(out[r]), bits(logits)), b
            if with_stats:
                assert torch.equal(stats[r], st) and torch.equal(bits(stats[r]), bits(st)), b
        else:                                                            # idle, unguided, or of the other kind: not one byte moved
            assert torch.equal(bits(out[r]), bits(prior[r])), b
            if with_stats:
                assert torch.equal(bits(stats[r]), bits(prior_stats[r])), b
    assert torch.equal(bits(other), bits(case["other"])) and (in_place or torch.equal(bits(cond), bits(case["cond"])))


@pytest.mark.parametrize("with_stats", [True, False], ids=["stats", "plain"])
@pytest.mark.parametrize("V,N", SHAPES)
def test_which_one_over_records_of_the_first_kind_is_the_entry_without_a_selector(operator_case, V, N, with_stats):
    case = operator_case(V, N)
    guides = _guides([(sc, min(on, 1)) for sc, on in KINDS])             # on in {0, 1}
    planes = []
    for which in (None, 1):
        out = _sentinel_like(case["cond"])
        stats = _sentinel_like(torch.empty(B_OP * N, V // 64, 2, device=dev())) if with_stats else None
        ops.guidance_combine_slots(case["cond"], case["other"], guides, case["slots"], N, out=out, block_stats=stats, which=which)
        planes.append((out, stats))
    assert torch.equal(bits(planes[0][0]), bits(planes[1][0]))
    assert not with_stats or torch.equal(bits(planes[0][1]), bits(planes[1][1]))
    # ... and nothing of the second kind is there to combine
    out = _sentinel_like(case["cond"])
    ops.guidance_combine_slots(case["cond"], case["other"], guides, case["slots"], N, out=out, which=2)
    assert torch.equal(bits(out), bits(_sentinel_like(out)))
    with pytest.raises(ValueError):
        ops.guidance_combine_slots(case["cond"], case["other"], guides, case["slots"], N, which=3)
    with pytest.raises(_lib.PmhipError):                                 # the native entry refuses it too
        _lib.check(_lib.load().pmhip_guidance_combine_slots_which(
            C.c_void_p(case["cond"].data_ptr()), C.c_void_p(case["other"].data_ptr()), C.c_void_p(guides.data_ptr()),
            C.c_void_p(case["slots"].data_ptr()), 0, N, C.c_void_p(out.data_ptr()), None, B_OP * N, V, None))
    assert torch.equal(bits(out), bits(_sentinel_like(out)))


# ------------------------------------------------------------------------------------------------------------------------------
# the contract
# ------------------------------------------------------------------------------------------------------------------------------
CAP_N = 5                                # the sessions' max_negative_len


def _scale_at(scale, step):
    return scale[step] if isinstance(scale, (list, tuple)) else scale


def reference_run(pipe, S, j, T, temperature, topk, seed, k, ctx_row, scale, neg_row, cap_n=CAP_N):
    """row j of the scalar path at B = S: final ids and last image from generate_ids (eager, one stream), the per-step pred and
    score from the scalar one-step entry with the step's scale (the same kernels), whose ids must end where generate_ids ends"""
    context = torch.zeros(S, ctx_row.shape[0], ctx_row.shape[1], device=dev())
    context[j] = ctx_row
    kw = {}
    if neg_row is not None:
        neg = torch.zeros(S, cap_n, neg_row.shape[1], device=dev())
        neg[j, :neg_row.shape[0]] = neg_row
        lens = [cap_n] * S
        lens[j] = neg_row.shape[0]
        kw = dict(negative_context=neg, negative_lens=lens)
    ids_ref, imgs = pipe.generate_ids(context, S, T, temperature, topk, [False] * (T - 1) + [True], seed, image_base=k - j,
                                      use_graph=False, streams=1, guidance_scale=list(scale) if isinstance(scale, tuple) else scale, **kw)
    eng = pipe.engine()
    temps, nmask = pipe._schedule(T, temperature)
    ids = torch.full((S, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long, device=dev())
    preds, scores = [], []
    for step in range(T):
        ids, _, pred, score = eng.sample(None, ids, context, topk, temps[step], nmask[step], seed=seed, step=step, image_base=k - j,
                                         want_img=False, want_aux=True, guidance_scale=_scale_at(scale, step), **kw)
        preds.append(pred[j].clone())
        scores.append(score[j].clone())
    assert torch.equal(ids, ids_ref)
    return ids_ref[j].clone(), preds, scores, imgs[0][j].clone()


def run_session(pipe, S, use_graph, plan, contexts, negatives, cap_n=CAP_N):
    """plan: {tick: [(T, temperature, topk, seed, k, scale or schedule (a tuple), index into `negatives` or None), ...]} ->
    submitted at that tick (before its step).  Returns ([(request parameters, Finished, the group it was decoded with)], the
    handle's (one, two, three)-pass slots steps of this run)"""
    s = pipe.decode_session(slots=S, conditional=True, use_graph=use_graph, record_steps=True, max_negative_len=cap_n)
    before = pipe.engine().slots_passes()
    out, tick, number = [], 0, 0
    last = max(plan)
    while tick <= last or not s.idle():
        for req in plan.get(tick, []):
            T, temp, topk, seed, k, scale, neg = req
            h = s.submit(context=contexts[number], timesteps=T, temperature=temp, topk=topk, seed=seed, image_index=k,
                         guidance_scale=list(scale) if isinstance(scale, tuple) else scale,
                         negative_context=None if neg is None else negatives[neg])
            h.params, h.ctx_row, h.neg_row = req, contexts[number], None if neg is None else negatives[neg]
            assert h.guidance_scale == (list(scale) if isinstance(scale, tuple) else scale)      # Request keeps what was passed
            number += 1
        done = s.step()
        assert s.tick == tick + 1
        out += [(f.handle.params, f, done) for f in done]
        tick += 1
    assert s.idle() and len(out) == number
    after = pipe.engine().slots_passes()
    return out, tuple(a - b for a, b in zip(after, before))


def expected_passes(handles):
    """the host decision, from the plan's ticks: the conditional pass, one more where an occupied slot is guided without a negative
    prompt, one more where one is guided with it -> (one-pass, two-pass, three-pass) ticks"""
    counts = [0, 0, 0]
    for tk in range(max(h.retired for h in handles) + 1):
        live = [h for h in handles if h.admitted <= tk <= h.retired]
        if live:
            unc = any(h.guidance_scale is not None and h.neg_row is None for h in live)
            neg = any(h.neg_row is not None for h in live)
            counts[int(unc) + int(neg)] += 1
    return tuple(counts)


def check_contract(pipe, S, use_graph, plan, contexts, negatives, fp32, refs, cap_n=CAP_N):
    run, passes = run_session(pipe, S, use_graph, plan, contexts, negatives, cap_n)
    handles = [f.handle for _, f, _ in run]
    assert passes == expected_passes(handles), (passes, expected_passes(handles))
    one, two = pipe.engine().slots_steps()
    assert (one, two) == pipe.engine().slots_passes()[:2]                # the older counter keeps reporting one and exactly two
    for params, f, group in run:
        T, temp, topk, seed, k, scale, _ = params
        h = f.handle
        assert h.retired == h.admitted + T - 1 and len(h.trace) == T
        key = (params, h.slot)
        if key not in refs:
            refs[key] = reference_run(pipe, S, h.slot, T, temp, topk, seed, k, h.ctx_row, scale, h.neg_row, cap_n)
        ids_ref, preds, scores, img_ref = refs[key]
        for step in range(T):
            assert torch.equal(h.trace[step][0], preds[step]), (params, h.slot, step, "pred")
            assert torch.equal(h.trace[step][1], scores[step]), (params, h.slot, step, "score")
        assert torch.equal(f.ids, ids_ref), (params, h.slot)
        together = pipe.vqgan.decode_from_indice(torch.stack([g.handle.trace[-1][0] for g in group]))
        assert torch.equal(f.image, together[[g.handle for g in group].index(h)])
        alone = pipe.vqgan.decode_from_indice(h.trace[-1][0][None])[0]
        err_alone, err_ref = maxabs(n(f.image), n(alone)), maxabs(n(f.image), n(img_ref))
        print(f"{params} slot {h.slot}: image max |session - decoded alone| {err_alone:.2e}, |session - reference run| {err_ref:.2e}")
        if fp32:
            assert err_alone < TOL and err_ref < TOL
    return run


def _tiny_inputs(pipe, count):
    contexts = list(pipe.text_model([f"p{i}" for i in range(count)]).to(dev()))
    D = contexts[0].shape[1]
    g = torch.Generator().manual_seed(4242)
    # negative contexts of 5 (the capacity), 1 and 3 rows
    negatives = [torch.randn(rows, D, generator=g).to(dev()) for rows in (CAP_N, 1, 3)]
    return contexts, negatives


# (T, temperature, topk, seed, image index k, scale or schedule, negative or None), admitted staggered into 3 slots.
#   tick 0      A (negative, capacity rows) + B (unguided)                          two passes (negative)
#   tick 1      A + B + C (scheduled scale, no negative)                            three
#   tick 2      A + C, slot 1 IDLE                                                  three
#   ticks 3-4   A + D (negative, 1 row) + C                                         three
#   tick 5      A + D                                                               two (negative; lengths travel: D has 1 row)
#   ticks 6-7   E (unguided) + F (negative of 3 rows, scheduled scale), slot 2 idle two (negative)
#   ticks 8-9   G (scalar scale, no negative) + F                                   three
#   tick 10     H (unguided) + I (scalar scale, no negative)                        two (no context)
#   tick 11     H                                                                   one
PLAN = {0: [(6, 1.0, 5, 401, 3, 2.5, 0), (2, 0.7, 1, 402, 9, None, None)],
        1: [(4, 1.3, 3, 403, 4, (4.0, 0.0, -1.0, 2.0), None)],
        3: [(3, 0.0, 4, 404, 30, 4.0, 1)],
        6: [(2, 0.9, 2, 405, 5, None, None), (4, 1.0, 5, 406, 2 ** 33 + 1, (1.0, 3.0, 3.0, 0.5), 2)],
        8: [(2, 0.5, 2, 407, 8, 1.0, None)],
        10: [(2, 1.1, 8, 408, 11, None, None), (1, 1.0, 3, 409, 12, 3.0, None)]}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_negative_session_contract_tiny_pipeline(tiny_pipe, dtype):
    pipe = tiny_pipe
    contexts, negatives = _tiny_inputs(pipe, 9)
    refs = {}
    try:
        pipe.set_compute_dtype(dtype)
        eager = check_contract(pipe, 3, False, PLAN, contexts, negatives, dtype == torch.float32, refs)
        assert expected_passes([f.handle for _, f, _ in eager]) == (1, 5, 6)
        # the negative prompt did something: the ids differ from the twin that is guided without it
        params, f, _ = next(x for x in eager if x[0][3] == 401)
        twin = reference_run(pipe, 3, f.handle.slot, *params[:5], f.handle.ctx_row, params[5], None)
        assert not torch.equal(f.ids, twin[0])
        # the graph path: per pass set the first step with the flag runs eagerly, the second captures, the rest replay; a second
        # session then replays from its first step on
        for _ in range(2):
            check_contract(pipe, 3, True, PLAN, contexts, negatives, dtype == torch.float32, refs)
    finally:
        pipe.set_compute_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------------------------------------
# degenerate cases
# ------------------------------------------------------------------------------------------------------------------------------
def _one_request(pipe, S, use_graph, slot, cap_n, **submit):
    """a session in which `slot` holds the request and the slots below it hold unguided fillers -> the request's Finished"""
    s = pipe.decode_session(slots=S, conditional=True, use_graph=use_graph, record_steps=True, max_negative_len=cap_n)
    filler = submit["context"]
    for i in range(slot):
        s.submit(context=filler, timesteps=submit["timesteps"], temperature=1.0, topk=2, seed=900 + i, image_index=50 + i)
    h = s.submit(**submit)
    done = s.drain()
    return next(f for f in done if f.handle is h)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_a_negative_equal_to_the_context_is_the_unguided_request(tiny_pipe, use_graph):
    """rows and length alike: cond - neg is exactly 0, so every scale gives the unguided request's predictions, scores and ids"""
    pipe = tiny_pipe
    ctx = pipe.text_model(["same"]).to(dev())[0]
    base = dict(context=ctx, timesteps=4, temperature=0.9, topk=4, seed=77, image_index=21)
    plain = _one_request(pipe, 3, use_graph, 1, ctx.shape[0], **base)
    for scale in (7.0, -2.0, [0.0, 1.0, 50.0, 3.0]):
        got = _one_request(pipe, 3, use_graph, 1, ctx.shape[0], guidance_scale=scale, negative_context=ctx.clone(), **base)
        assert torch.equal(got.ids, plain.ids), scale
        for (p1, s1), (p2, s2) in zip(got.handle.trace, plain.handle.trace):
            assert torch.equal(p1, p2) and torch.equal(s1, s2), scale


@pytest.mark.parametrize("with_negative", [False, True], ids=["uncond", "negative"])
def test_a_schedule_of_one_value_is_the_scalar_scale(tiny_pipe, with_negative):
    pipe = tiny_pipe
    contexts, negatives = _tiny_inputs(pipe, 1)
    base = dict(context=contexts[0], timesteps=5, temperature=1.0, topk=5, seed=31, image_index=14,
                negative_context=negatives[2] if with_negative else None)
    scalar = _one_request(pipe, 3, False, 2, CAP_N, guidance_scale=2.5, **base)
    sched = _one_request(pipe, 3, False, 2, CAP_N, guidance_scale=[2.5] * 5, **base)
    assert sched.handle.guidance_scale == [2.5] * 5 and scalar.handle.guidance_scale == 2.5
    assert torch.equal(sched.ids, scalar.ids) and torch.equal(sched.image, scalar.image)
    for (p1, s1), (p2, s2) in zip(sched.handle.trace, scalar.handle.trace):
        assert torch.equal(p1, p2) and torch.equal(s1, s2)


def _guide_records(*kinds):
    arr = (_lib.SlotGuide * len(kinds))()
    for i, k in enumerate(kinds):
        if k is not None:
            arr[i] = _lib.SlotGuide(*k)
    return arr


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_without_a_negative_request_the_step_is_the_one_it_was(tiny_pipe, use_graph):
    """the same plan through step_slots without the new keywords and with them (a negative context prepared, then kept, that no
    slot is guided against): the same predictions, scores, ids and pass counts -- and none of three passes"""
    pipe = tiny_pipe
    N = pipe.num_tokens
    ctx = pipe.text_model(["a", "b", "c"]).to(dev())
    neg = torch.randn(3, 4, ctx.shape[2], generator=torch.Generator().manual_seed(5)).to(dev())
    temps, nmask = pipe._schedule(4, 1.0)
    runs = []
    for keywords in (False, True):
        eng = pipe.engine().clone()
        ids = torch.full((3, N), pipe.mask_token_id, dtype=torch.long, device=dev())
        trace = []
        for step in range(4):
            recs = _records((11, 3, temps[step], 5, nmask[step], step), None if step == 1 else (12, 4, temps[step], 2, nmask[step], step),
                            (13, 5, temps[step], 8, nmask[step], step))
            # step 3 is unguided altogether: one pass
            guides = _guide_records((2.0, 1), None, (0.5 * step, 1)) if step < 3 else _guide_records(None, None, None)
            kw = dict(negative_context=neg, negative_lens=[4, 2, 1], keep_negative=step > 0) if keywords else {}
            _, pred, score = eng.step_slots(ids, ctx, recs, use_graph=use_graph, keep_context=step > 0, guides=guides, **kw)
            trace.append((ids.clone(), pred.clone(), score.clone()))
        assert eng.slots_passes() == (1, 3, 0) and eng.slots_steps() == (1, 3)
        runs.append(trace)
    for a, b in zip(*runs):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------------------
# error paths
# ------------------------------------------------------------------------------------------------------------------------------
def test_negative_step_error_paths(tiny_pipe):
    pipe = tiny_pipe
    eng = pipe.engine().clone()                                          # a handle no slots call has touched
    N = pipe.num_tokens
    ids = torch.full((2, N), pipe.mask_token_id, dtype=torch.long, device=dev())
    start = ids.clone()
    good = (1, 0, 1.0, 3, 4, 0)
    ctx = pipe.text_model(["a", "b"]).to(dev())
    Ln = 3
    neg = torch.randn(2, Ln, ctx.shape[2], generator=torch.Generator().manual_seed(6)).to(dev())

    def native(guides, neg_context, neg_lens, flags=0):
        """the entry itself: the Python wrapper checks lengths before the native call would"""
        lens = None if neg_lens is None else (C.c_int * 2)(*neg_lens)
        with pytest.raises(_lib.PmhipError) as e:
            _lib.check(eng.lib.pmhip_pipeline_step_slots_negative(
                eng.handle, C.c_void_p(ids.data_ptr()), C.c_void_p(ctx.data_ptr()), ctx.shape[1], 2, None, _records(good, good), guides, None,
                None if neg_context is None else C.c_void_p(neg_context.data_ptr()), Ln, lens, flags, None, None,
                C.c_void_p(torch.cuda.current_stream().cuda_stream)), "pmhip_pipeline_step_slots_negative")
        return e.value

    # on = 2 without a negative set, through the wrapper (a record of the second kind selects the entry that knows it)
    with pytest.raises(_lib.PmhipError) as e:
        eng.step_slots(ids, ctx, _records(good, good), guides=_guide_records((2.0, 2), None))
    assert e.value.code == _lib.PMHIP_EINVAL and "slot 0" in str(e.value) and "negative context" in str(e.value)
    # on = 3
    with pytest.raises(_lib.PmhipError) as e:
        eng.step_slots(ids, ctx, _records(good, good), guides=_guide_records(None, (2.0, 3)), negative_context=neg)
    assert e.value.code == _lib.PMHIP_EINVAL and "slot 1" in str(e.value) and "0, 1 or 2" in str(e.value)
    # a length of 0 and one of Ln + 1: the message names the slot
    for lens, slot in (([Ln, 0], 1), ([Ln + 1, 1], 0)):
        err = native(_guide_records((2.0, 2), (1.0, 2)), neg, lens)
        assert err.code == _lib.PMHIP_EINVAL and f"slot {slot}" in str(err) and f"Ln={Ln}" in str(err), str(err)
        with pytest.raises(ValueError):
            eng.step_slots(ids, ctx, _records(good, good), guides=_guide_records((2.0, 2), (1.0, 2)), negative_context=neg, negative_lens=lens)
    # lengths without a set
    err = native(_guide_records((2.0, 1), None), None, [1, 1])
    assert err.code == _lib.PMHIP_EINVAL and "without a negative context" in str(err)
    with pytest.raises(ValueError):
        eng.step_slots(ids, ctx, _records(good, good), negative_lens=[1, 1])
    # a non-finite scale of a slot guided against the negative context
    with pytest.raises(_lib.PmhipError) as e:
        eng.step_slots(ids, ctx, _records(good, good), guides=_guide_records((float("inf"), 2), None), negative_context=neg)
    assert e.value.code == _lib.PMHIP_EINVAL and "finite" in str(e.value)
    # keep-negative before anything was prepared
    with pytest.raises(_lib.PmhipError) as e:
        eng.step_slots(ids, ctx, _records(good, good), guides=_guide_records((2.0, 2), None), negative_context=neg, keep_negative=True)
    assert e.value.code == _lib.PMHIP_ESTATE
    torch.cuda.synchronize()
    assert torch.equal(ids, start) and eng.slots_passes() == (0, 0, 0)   # nothing of the refused calls ran
    # prepared, the set is kept across a step -- also one that prepares a new context -- but not for another Ln, nor after a step
    # that neither brought nor kept it
    eng.step_slots(ids, ctx, _records(good, good), guides=_guide_records((2.0, 2), (1.0, 1)), negative_context=neg, negative_lens=[2, 3])
    nxt = (1, 0, 1.0, 3, 2, 1)
    eng.step_slots(ids, ctx, _records(nxt, nxt), guides=_guide_records((2.0, 2), None), negative_context=neg, keep_negative=True)
    assert eng.slots_passes() == (0, 1, 1)
    held = ids.clone()
    with pytest.raises(_lib.PmhipError) as e:
        eng.step_slots(ids, ctx, _records(nxt, nxt), guides=_guide_records((2.0, 2), None), negative_context=neg[:, :2], keep_negative=True)
    assert e.value.code == _lib.PMHIP_ESTATE
    eng.step_slots(ids.clone(), ctx, _records(nxt, nxt), keep_context=True)
    with pytest.raises(_lib.PmhipError) as e:
        eng.step_slots(ids, ctx, _records(nxt, nxt), guides=_guide_records((2.0, 2), None), negative_context=neg, keep_context=True,
                       keep_negative=True)
    assert e.value.code == _lib.PMHIP_ESTATE
    torch.cuda.synchronize()
    assert torch.equal(ids, held) and eng.slots_passes() == (1, 1, 1)


# ------------------------------------------------------------------------------------------------------------------------------
# full size
# ------------------------------------------------------------------------------------------------------------------------------
def test_negative_session_contract_full_size(chain_pipe):
    """12L/d512, 1024 tokens, 8192 classes, trained-like logits, a seeded random [77, 512] context per request; S = 3 with one slot
    of each kind (unguided, guided without and with a negative prompt of 40 of 77 rows), T = 2, bf16, eager and graph"""
    pipe = chain_pipe
    plan = {0: [(2, 1.0, 5, 501, 4, None, None), (2, 0.8, 3, 502, 5, (3.0, 1.5), None), (2, 1.0, 5, 503, 2 ** 32 + 6, 4.0, 0)]}
    g = torch.Generator().manual_seed(78)
    contexts = [torch.randn(77, 512, generator=g).to(dev()) for _ in range(3)]
    negatives = [torch.randn(40, 512, generator=g).to(dev())]
    refs = {}
    try:
        pipe.set_compute_dtype(torch.bfloat16)
        for use_graph in (False, True):
            run = check_contract(pipe, 3, use_graph, plan, contexts, negatives, False, refs, cap_n=77)
            assert expected_passes([f.handle for _, f, _ in run]) == (0, 0, 2)
    finally:
        pipe.set_compute_dtype(torch.float32)
