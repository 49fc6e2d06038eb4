"""The sampler filters per request in decode sessions, on the GPU: pmhip_sample_rows_slots_filter against
the scalar entries it restates slot by slot, and the contract of paintmind_amd/serve.py -- a request (T, temperature, topk, top_p,
seed, k, ...) in slot j of an S-slot FilterSession computes, bit for bit, what row j of ``Pipeline.generate_ids(B=S, ..., topk=topk,
top_p=top_p, image_base=k - j, use_graph=False, streams=1)`` computes on the unchanged scalar path, whatever shares the batch with
it.  Both sides of every comparison run the same kernels: there is no tolerance in this file."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import paintmind_amd as pm
from abi_frames import bits, call, framed
from gpu_common import dev, t
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline, loop_schedule

pytestmark = pytest.mark.gpu

TOKENS = 4
IDLE = 7                                 # the idle slot of the operator cases


# ------------------------------------------------------------------------------------------------------------------------------
# operator level
# ------------------------------------------------------------------------------------------------------------------------------
def _filters(V):
    """(topk, top_p) per slot: the class boundaries 8 | 9 and 64 | 65, no filter at all, a nucleus under a narrow and under no
    top-k, one idle slot (its values must not be looked at)"""
    f = [(1, 1.0), (8, 1.0), (9, 1.0), (64, 1.0), (65, 1.0), (V - 1, 1.0), (V, 1.0), (3, 0.5), (V, 0.999)]
    f.insert(IDLE, None)
    return f


def _records(V):
    """(seed, image_index, temperature, topk, num_mask, step) per slot, all different: a temperature of 0, image indices whose row
    counters pass 2^32 and 2^34, a seed with both words set"""
    temps = [0.7, 0.0, 1.3, 0.5, 1.0, 0.9, 2.0, 0.0, 1.1, 0.8]
    index = [7, 2 ** 33 + 5, 4096, 2 ** 32, 1, 2 ** 32 + 3, 12, 0, 2 ** 31, 99]
    recs = []
    for b, f in enumerate(_filters(V)):
        recs.append(None if f is None else (0x0123456789ABCDEF + 1000003 * b, index[b], temps[b], f[0], 1, 3 * b + 1))
    return recs


def _sentinel(shape, dtype):
    out = torch.empty(shape, dtype=dtype, device=dev())
    out.view(torch.int32 if dtype == torch.float32 else torch.int64).fill_(0x5A5A5A5A if dtype == torch.float32 else 0x5A5A5A5A5A5A5A5A)
    return out


def _scalar_rows(x, ids, V, rec, top_p, stats, row_base=None):
    """the scalar entry on one image's rows with its slot's values: pmhip_sample_rows, _stats (statistics given and topk <= 8) or
    _nucleus"""
    seed, k, temp, topk, _, step = rec
    st = stats if (stats is not None and topk <= 8 and top_p == 1.0) else None
    return ops.sample_rows(x, ids, V, topk, temp, seed=seed, step=step, row_base=k * TOKENS if row_base is None else row_base,
                           block_stats=st, top_p=None if top_p == 1.0 else top_p)


@pytest.fixture(scope="module")
def operator_case():
    """per V, computed once and left unchanged: logits, partly given ids, statistics, the records, and per active slot the scalar
    entry's (pred, ids, score), with statistics handed in and without"""
    cache = {}

    def get(V):
        if V not in cache:
            rng = np.random.default_rng(31 * V)
            filt, recs = _filters(V), _records(V)
            S = len(recs)
            M = S * TOKENS
            x = t((rng.standard_normal((M, V)) * 3.0).astype(np.float32))
            ids = rng.integers(0, V, M).astype(np.int64)
            ids[rng.random(M) < 0.6] = V
            ids = t(ids)
            same, stats = ops.guidance_combine(x, x, 1.0, with_stats=True)
            assert torch.equal(same, x)
            want = {}
            for b, rec in enumerate(recs):
                if rec is not None:
                    r = slice(b * TOKENS, (b + 1) * TOKENS)
                    want[b] = {ws: _scalar_rows(x[r], ids[r], V, rec, filt[b][1], stats[r].contiguous() if ws else None) for ws in (True, False)}
            top_p = torch.tensor([1.0 if f is None else f[1] for f in filt], dtype=torch.float32, device=dev())
            top_p[IDLE] = float("nan")                                   # an idle slot's mass is not looked at
            cache[V] = dict(x=x, ids=ids, stats=stats, recs=recs, filt=filt, want=want, slots=ops.pack_slots(recs, dev()), top_p=top_p)
        return cache[V]
    return get


# V: the four register classes of the row kernels (256, 1024, 8192 | 8256), ragged last groups (1088, 8256) and exact ones; 8192:
# two blocks per lane in the block-statistics kernel
@pytest.mark.parametrize("with_stats", [True, False], ids=["stats", "dense"])
@pytest.mark.parametrize("V", [256, 1024, 1088, 8256, 8192])
def test_every_slot_equals_its_scalar_entry_and_every_row_is_written_once(operator_case, V, with_stats):
    case = operator_case(V)
    S = len(case["recs"])
    M = S * TOKENS
    pred, merged, score = _sentinel((M,), torch.int64), _sentinel((M,), torch.int64), _sentinel((M,), torch.float32)
    call("pmhip_sample_rows_slots_filter", case["x"], V, case["stats"] if with_stats else None, case["ids"], V, case["slots"], case["top_p"],
         TOKENS, pred, merged, score, M, V)
    for out in (pred, merged, score):
        assert not bool((bits(out) == bits(_sentinel((M,), out.dtype))).any())          # no row was left out
    for b, rec in enumerate(case["recs"]):
        r = slice(b * TOKENS, (b + 1) * TOKENS)
        if rec is None:
            assert torch.equal(pred[r], case["ids"][r]) and torch.equal(merged[r], case["ids"][r])
            assert torch.equal(score[r], torch.full((TOKENS,), -1e5, device=dev()))
            continue
        for got, want in zip((pred[r], merged[r], score[r]), case["want"][b][with_stats]):
            assert torch.equal(bits(got), bits(want)), (V, b, case["filt"][b])
    # the Python operator is the same call
    again = ops.sample_rows_slots(case["x"], case["ids"], V, case["slots"], TOKENS, block_stats=case["stats"] if with_stats else None,
                                  top_p=case["top_p"], filters=True)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again, (pred, merged, score)))


def test_without_a_nucleus_array_every_slot_has_none_and_class_t_is_the_entry_without_filters(operator_case):
    V = 1024
    case = operator_case(V)
    none = ops.sample_rows_slots(case["x"], case["ids"], V, case["slots"], TOKENS, filters=True)
    for b, rec in enumerate(case["recs"]):
        if rec is not None:
            r = slice(b * TOKENS, (b + 1) * TOKENS)
            want = _scalar_rows(case["x"][r], case["ids"][r], V, rec, 1.0, None)
            assert all(torch.equal(bits(g[r]), bits(w)) for g, w in zip(none, want)), b
    # records of class T only: the four launches give what the one launch of pmhip_sample_rows_slots gives
    recs = [None if rec is None else rec[:3] + (1 + b % 8,) + rec[4:] for b, rec in enumerate(case["recs"])]
    slots = ops.pack_slots(recs, dev())
    a = ops.sample_rows_slots(case["x"], case["ids"], V, slots, TOKENS, block_stats=case["stats"])
    b = ops.sample_rows_slots(case["x"], case["ids"], V, slots, TOKENS, block_stats=case["stats"], filters=True)
    assert all(torch.equal(bits(p), bits(q)) for p, q in zip(a, b))
    with pytest.raises(ValueError):
        ops.sample_rows_slots(case["x"], case["ids"], V, slots, TOKENS, top_p=case["top_p"])          # top_p without filters


def test_rows_of_minus_infinity_and_plateaus_in_wide_and_nucleus_slots():
    """row 0 of an image: -inf but for a few columns; row 1: a plateau of 40 equal values behind 70 larger ones, so that top-k 100
    cuts it and the column order decides; rows 2 and 3 random.  The images sit in a W and an N slot beside slots of the other
    classes."""
    V, K = 1024, 100
    rng = np.random.default_rng(5)
    filt = [(5, 1.0), (K, 1.0), (K, 0.9), (40, 1.0), (V, 0.5)]
    S = len(filt)
    logits = (rng.standard_normal((S * TOKENS, V)) * 2.0).astype(np.float32)
    for b in range(S):
        row = np.full(V, -np.inf, np.float32)
        cols = rng.permutation(V)[:6]
        row[cols] = rng.standard_normal(6).astype(np.float32)
        logits[b * TOKENS] = row
        plateau = np.round(rng.standard_normal(V) * 2).astype(np.float32).clip(-6, 1)
        pick = rng.permutation(V)[:110]
        plateau[pick[:40]] = 2.0
        plateau[pick[40:]] = rng.integers(3, 6, 70).astype(np.float32)
        logits[b * TOKENS + 1] = plateau
    x = t(logits)
    ids = torch.full((S * TOKENS,), V, dtype=torch.long, device=dev())
    recs = [(900 + b, 2 ** 32 + b, [1.0, 0.0, 0.8, 1.0, 1.5][b], filt[b][0], 1, b) for b in range(S)]
    top_p = torch.tensor([p for _, p in filt], dtype=torch.float32, device=dev())
    got = ops.sample_rows_slots(x, ids, V, ops.pack_slots(recs, dev()), TOKENS, top_p=top_p, filters=True)
    for b, rec in enumerate(recs):
        r = slice(b * TOKENS, (b + 1) * TOKENS)
        want = _scalar_rows(x[r], ids[r], V, rec, filt[b][1], None)
        assert all(torch.equal(bits(g[r]), bits(w)) for g, w in zip(got, want)), b
        assert bool(torch.isfinite(x[b * TOKENS, got[0][b * TOKENS]]))                   # a -inf column is never drawn
    # slot 1 at temperature 0 draws the plateau row's maximum: the first of the largest values in column order
    assert int(got[0][TOKENS + 1]) == int(np.flatnonzero(logits[TOKENS + 1] == logits[TOKENS + 1].max())[0])


def test_the_c_entry_keeps_strides_aliasing_and_extents(operator_case):
    V = 1088
    case = operator_case(V)
    S = len(case["recs"])
    M = S * TOKENS
    fx = framed(M, V, dtype=torch.float32, payload=case["x"], fill="nan")             # ldl > V, NaN in the gap and around
    fi = framed(M, 1, ld=1, dtype=torch.int64, payload=case["ids"].reshape(M, 1))     # ids_in AND ids_out
    fp = framed(M, 1, ld=1, dtype=torch.int64, device=dev())
    fs = framed(M, 1, ld=1, dtype=torch.float32, device=dev())
    fst = framed(M, (V // 64) * 2, ld=(V // 64) * 2, dtype=torch.float32, payload=case["stats"].reshape(M, -1), fill="nan")
    assert fx.ld > V
    call("pmhip_sample_rows_slots_filter", fx, fx.ld, fst, fi, V, case["slots"], case["top_p"], TOKENS, fp, fi, fs, M, V)
    for f, what in ((fx, "logits"), (fi, "ids"), (fp, "pred"), (fs, "score"), (fst, "stats")):
        f.assert_frame_untouched(what)
    assert torch.equal(bits(fx.payload()), bits(case["x"]))                              # the inputs are inputs
    want = ops.sample_rows_slots(case["x"], case["ids"], V, case["slots"], TOKENS, block_stats=case["stats"], top_p=case["top_p"], filters=True)
    for f, w in zip((fp, fi, fs), want):
        assert torch.equal(bits(f.payload().reshape(M)), bits(w))


# ------------------------------------------------------------------------------------------------------------------------------
# the contract, on a tiny pipeline with 256 classes (the tiny configurations stop at 64)
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
            pipe.transformer.to_logits.weight.data.mul_(8.0)   # logits that spread: a filter then matters
        yield pipe.to(dev()).eval()
    finally:
        del pm.ver2cfg["tiny-vqgan-256"], pm.ver2cfg["tiny-pipeline-256"]


@pytest.fixture(params=[torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def pipe(request, wide_pipe):
    wide_pipe.set_compute_dtype(request.param)
    yield wide_pipe
    wide_pipe.set_compute_dtype(torch.float32)


S = 3
CAP_N = 4                                # the sessions' max_negative_len


def rq(T, temperature, topk, top_p, seed, k, short=False, scale=None, neg=False, choice=None):
    """a request: short: its context has 2 rows instead of the capacity; scale: a number or a schedule (a tuple); neg: a negative
    context of 3 of the CAP_N rows; choice: a choice temperature.  Conditional sessions only use the last four."""
    return (T, temperature, topk, top_p, seed, k, short, scale, neg, choice)


# 8 requests admitted staggered into 3 slots; image indices >= S.  Classes by tick (slot 0 | 1 | 2):
#   0      T k=1            | R k=9, guided     | -
#   1      T                | R                 | W k=65, choice temperature, short context
#   2      T                | N k=None p=0.9, schedule + negative | W
#   3      T                | N                 | W
#   4      T                | N                 | W
#   5      N k=8 p=0.5      | R k=64, short     | T k=8             <- the one tick with three classes and no W
#   6      N                | R                 | T
#   7      W k=200          | R                 | -                 (slot 2 idle)
#   8, 9   W                | R / -             | -
PLAN = {0: [rq(5, 1.0, 1, None, 601, 3), rq(2, 0.7, 9, None, 602, 9, scale=2.5)],
        1: [rq(4, 1.3, 65, None, 603, 4, short=True, choice=4.5)],
        2: [rq(3, 0.9, None, 0.9, 604, 2 ** 33 + 1, scale=(4.0, 0.0, 2.0), neg=True)],
        5: [rq(2, 1.0, 8, 0.5, 605, 5), rq(4, 0.0, 64, None, 606, 30, short=True), rq(2, 0.8, 8, None, 607, 8)],
        7: [rq(3, 1.1, 200, None, 608, 11)]}


def _inputs(pipe):
    ctx = pipe.text_model([f"p{i}" for i in range(8)]).to(dev())
    g = torch.Generator().manual_seed(99)
    return list(ctx), torch.randn(3, ctx.shape[2], generator=g).to(dev())


def reference_run(pipe, j, req, ctx_row, neg_row, conditional, cap):
    """row j of the scalar path at B = S: final ids from generate_ids (eager, one stream), the per-step pred and score from the
    scalar one-step entry with the step's values (the same kernels), whose ids must end where generate_ids ends"""
    T, temperature, topk, top_p, seed, k, short, scale, neg, choice = req
    V = pipe.mask_token_id
    topk = V if topk is None else topk
    context, kw = None, {}
    if conditional:
        context = torch.zeros(S, cap, ctx_row.shape[1], device=dev())
        context[j, :ctx_row.shape[0]] = ctx_row
        if ctx_row.shape[0] != cap:                                      # the request's own length; the other rows are not looked at
            lens = [cap] * S
            lens[j] = ctx_row.shape[0]
            kw["context_lens"] = lens
        if neg_row is not None:
            negc = torch.zeros(S, CAP_N, neg_row.shape[1], device=dev())
            negc[j, :neg_row.shape[0]] = neg_row
            nl = [CAP_N] * S
            nl[j] = neg_row.shape[0]
            kw.update(negative_context=negc, negative_lens=nl)
    else:
        scale = None
    ids_ref, _ = pipe.generate_ids(context, S, T, temperature, topk, [False] * T, seed, image_base=k - j, use_graph=False, streams=1,
                                   guidance_scale=list(scale) if isinstance(scale, tuple) else scale, choice_temperature=choice, top_p=top_p,
                                   **kw)
    eng = pipe.engine()
    temps, nmask, ctemps = loop_schedule(T, temperature, pipe.num_tokens, choice)
    ids = torch.full((S, pipe.num_tokens), V, dtype=torch.long, device=dev())
    preds, scores = [], []
    for step in range(T):
        ids, _, pred, score = eng.sample(None, ids, context, topk, temps[step], nmask[step], seed=seed, step=step, image_base=k - j,
                                         want_img=False, want_aux=True, guidance_scale=scale[step] if isinstance(scale, tuple) else scale,
                                         choice_temperature=ctemps[step] if ctemps else None, top_p=top_p, **kw)
        preds.append(pred[j].clone())
        scores.append(score[j].clone())
    assert torch.equal(ids, ids_ref)
    return ids_ref[j].clone(), preds, scores


def run_session(pipe, conditional, use_graph, plan, filters=True):
    contexts, neg_row = _inputs(pipe)
    cap = contexts[0].shape[0]
    s = pipe.decode_session(slots=S, conditional=conditional, use_graph=use_graph, record_steps=True, decode=False,
                            max_context_len=cap if conditional else None, max_negative_len=CAP_N, filters=filters)
    before = pipe.engine().slots_filter_steps()
    out, tick, number = [], 0, 0
    while tick <= max(plan) or not s.idle():
        for req in plan.get(tick, []):
            T, temperature, topk, top_p, seed, k, short, scale, neg, choice = req
            kw = {}
            if conditional:
                kw = dict(context=contexts[number][:2] if short else contexts[number], negative_context=neg_row if neg else None,
                          guidance_scale=list(scale) if isinstance(scale, tuple) else scale)
            if filters:
                kw["top_p"] = top_p
            h = s.submit(timesteps=T, temperature=temperature, topk=topk, seed=seed, image_index=k, choice_temperature=choice, **kw)
            h.params, h.ctx_row, h.neg_row, h.cap = req, kw.get("context"), kw.get("negative_context"), cap
            number += 1
        out += [f for f in s.step()]
        tick += 1
    assert s.idle() and len(out) == number
    after = pipe.engine().slots_filter_steps()
    return out, tuple(a - b for a, b in zip(after, before))


def expected_forms(handles):
    """(tiles_only, chain) ticks, from the plan: the chain exactly where an occupied slot is of another class than T"""
    counts = [0, 0]
    for tk in range(max(h.retired for h in handles) + 1):
        live = [h for h in handles if h.admitted <= tk <= h.retired]
        if live:
            counts[int(any(h.topk > 8 or h.top_p < 1.0 for h in live))] += 1
    return tuple(counts)


def check_contract(pipe, conditional, use_graph, plan, refs):
    done, forms = run_session(pipe, conditional, use_graph, plan)
    handles = [f.handle for f in done]
    assert forms == expected_forms(handles), (forms, expected_forms(handles))
    for f in done:
        h = f.handle
        assert h.retired == h.admitted + h.timesteps - 1 and len(h.trace) == h.timesteps
        key = (h.params, h.slot, conditional)
        if key not in refs:
            refs[key] = reference_run(pipe, h.slot, h.params, h.ctx_row, h.neg_row, conditional, h.cap)
        ids_ref, preds, scores = refs[key]
        for step in range(h.timesteps):
            assert torch.equal(h.trace[step][0], preds[step]), (h.params, h.slot, step, "pred")
            assert torch.equal(bits(h.trace[step][1]), bits(scores[step])), (h.params, h.slot, step, "score")
        assert torch.equal(f.ids, ids_ref), (h.params, h.slot)
    return done, forms


@pytest.mark.parametrize("conditional", [True, False], ids=["conditional", "unconditional"])
def test_filter_session_contract(pipe, conditional):
    assert pipe.mask_token_id == 256
    refs = {}
    eager, forms = check_contract(pipe, conditional, False, PLAN, refs)
    assert forms == (0, 10)
    assert [(f.handle.topk, f.handle.top_p) for f in sorted(eager, key=lambda f: f.handle.number)] == \
        [(1, 1.0), (9, 1.0), (65, 1.0), (256, 0.9), (8, 0.5), (64, 1.0), (8, 1.0), (200, 1.0)]
    # the graph path: the chain form's first step with the flag runs eagerly, the second captures, the rest replay; a second
    # session then replays from its first step on
    for _ in range(2):
        check_contract(pipe, conditional, True, PLAN, refs)


# ------------------------------------------------------------------------------------------------------------------------------
# the new range costs a session that does not use it nothing
# ------------------------------------------------------------------------------------------------------------------------------
T_PLAN = {0: [rq(4, 1.0, 5, None, 701, 3), rq(2, 0.7, 1, None, 702, 9, scale=2.0)],
          1: [rq(3, 1.3, 8, None, 703, 4, short=True, choice=2.0)],
          3: [rq(2, 0.9, 2, None, 704, 5, scale=(1.0, 3.0), neg=True)]}


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_a_session_of_class_t_requests_is_the_default_session(wide_pipe, use_graph):
    pipe = wide_pipe
    runs = []
    for filters in (False, True):
        done, forms = run_session(pipe, True, use_graph, T_PLAN, filters=filters)
        assert forms == ((5, 0) if filters else (0, 0))                  # every step: the form with the one launch
        runs.append(done)
    for a, b in zip(*runs):
        assert a.handle.params == b.handle.params and torch.equal(a.ids, b.ids)
        for (p1, s1), (p2, s2) in zip(a.handle.trace, b.handle.trace):
            assert torch.equal(p1, p2) and torch.equal(bits(s1), bits(s2))


def test_the_step_after_the_last_wide_request_retired_is_the_one_launch_again(wide_pipe):
    plan = {0: [rq(2, 1.0, 100, None, 801, 3), rq(5, 0.8, 4, None, 802, 4)], 1: [rq(1, 1.0, 3, 0.7, 803, 5)]}
    done, forms = run_session(wide_pipe, False, False, plan)
    assert forms == (3, 2) == expected_forms([f.handle for f in done])   # ticks 0, 1 carry the W and the N request; 2, 3, 4 do not


# ------------------------------------------------------------------------------------------------------------------------------
# error paths
# ------------------------------------------------------------------------------------------------------------------------------
def _slot_records(*recs):
    arr = (_lib.Slot * len(recs))()
    for i, r in enumerate(recs):
        if r is None:
            arr[i].step = _lib.SLOT_IDLE
        else:
            arr[i] = _lib.Slot(*r)
    return arr


def test_filter_step_error_paths(wide_pipe):
    pipe = wide_pipe
    eng = pipe.engine().clone()                                          # a handle no slots call has touched
    N, V = pipe.num_tokens, pipe.mask_token_id
    ids = torch.full((2, N), V, dtype=torch.long, device=dev())
    start = ids.clone()
    good = (1, 0, 1.0, 3, 4, 0)

    def native(records, top_p):
        with pytest.raises(_lib.PmhipError) as e:
            _lib.check(eng.lib.pmhip_pipeline_step_slots_filter(
                eng.handle, C.c_void_p(ids.data_ptr()), None, 0, 2, None, records, None, None, None, 0, None, (C.c_float * 2)(*top_p), 0, None,
                None, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "pmhip_pipeline_step_slots_filter")
        return e.value

    for topk in (0, V + 1):
        with pytest.raises(_lib.PmhipError) as e:
            eng.step_slots(ids, None, _slot_records(good, (1, 0, 1.0, topk, 4, 0)), top_p=[1.0, 1.0])
        assert e.value.code == _lib.PMHIP_EINVAL and "slot 1" in str(e.value) and f"topk={topk}" in str(e.value)
    for bad in (0.0, 1.5, float("nan"), float("inf")):
        err = native(_slot_records((1, 0, 1.0, 200, 4, 0), good), [bad, 1.0])
        assert err.code == _lib.PMHIP_EINVAL and "slot 0" in str(err) and "top_p" in str(err), str(err)
        with pytest.raises(ValueError, match="slot 0"):                  # the wrapper checks it like ops.sample_rows does
            eng.step_slots(ids, None, _slot_records((1, 0, 1.0, 200, 4, 0), good), top_p=[bad, 1.0])
    with pytest.raises(ValueError):
        eng.step_slots(ids, None, _slot_records(good, good), top_p=[1.0])
    # without top_p= the step keeps its limit: this is the boundary between the two
    with pytest.raises(_lib.PmhipError) as e:
        eng.step_slots(ids, None, _slot_records(good, (1, 0, 1.0, 9, 4, 0)))
    assert e.value.code == _lib.PMHIP_EINVAL and "[1, 8]" in str(e.value)
    torch.cuda.synchronize()
    assert torch.equal(ids, start) and eng.slots_filter_steps() == (0, 0) and eng.slots_passes() == (0, 0, 0)      # nothing ran
    # the same values on an IDLE slot are not looked at -- by the wrapper and by the entry
    idle_bad = (1, 0, 1.0, V + 1, 0, _lib.SLOT_IDLE)
    eng.step_slots(ids, None, _slot_records((1, 0, 1.0, 200, 4, 0), idle_bad), top_p=[1.0, float("nan")])
    assert torch.equal(ids[1], start[1]) and int((ids[0] != V).sum()) == N - 4
    assert eng.slots_filter_steps() == (0, 1)
    rc = eng.lib.pmhip_pipeline_step_slots_filter(
        eng.handle, C.c_void_p(ids.data_ptr()), None, 0, 2, None, _slot_records((1, 0, 1.0, 3, 2, 1), idle_bad), None, None, None, 0, None,
        (C.c_float * 2)(1.0, 7.0), _lib.SLOTS_KEEP_CONTEXT, None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.PMHIP_OK and eng.slots_filter_steps() == (1, 1) and int((ids[0] != V).sum()) == N - 2
