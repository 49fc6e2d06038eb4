"""Prompt weights per request in decode sessions, on the GPU: the contract of paintmind_amd/serve.py.  A
weighted request in slot j of an S-slot session computes, bit for bit, the per-step predictions, the scores and the final ids of row j
of ``generate_ids(context [S, capacity, D] with its rows in row j, context_segments / token_segments / context_weights with its layout
and weights in row j and neutral rows elsewhere, B=S, ..., image_base=k - j, streams=1)``; the plain and the regional requests beside
it still compute their ``context_lens=`` / segment rows; all whatever shares the batch.  Tiny pipeline (16 tokens), S = 4, T = 3 and
4, fp32-verify and bf16, eager and with PMHIP_SLOTS_GRAPH.  A context row of weight 0 holds NaN wherever a request brings one.  There
is no tolerance in this file except the project's fp32 bar against the CPU branch."""
import numpy as np
import pytest
import torch

import paintmind_amd as pm
from abi_frames import bits
from gpu_common import dev
from paintmind_amd import _lib
from paintmind_amd.generate import Pipeline, loop_schedule, region_layout
from util import load_golden, to_torch_sd

pytestmark = pytest.mark.gpu
TOL = 1e-3                       # the project's float bar (tests/test_gpu_regions.py, tests/test_weights_cpu.py)
S, CAP, CAP_N, D = 4, 40, 6, 96
WEIGHTS = np.array([0.0, 0.125, 1.0, 8.0], np.float32)


def _tiny():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False)
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("text_model") for k in missing.missing_keys)
    return pipe.eval()


@pytest.fixture(scope="module")
def tiny():
    return _tiny().to(dev())


@pytest.fixture(params=[torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def pipe(request, tiny):
    tiny.set_compute_dtype(request.param)
    yield tiny
    tiny.set_compute_dtype(torch.float32)


def _seed(name):
    return sum(ord(c) * 131 ** i for i, c in enumerate(name))


def rows(name, count):
    """`count` context rows of N(0, 1) keyed by the name"""
    return torch.randn(count, D, generator=torch.Generator().manual_seed(_seed(name)))


def drawn(name, count):
    """`count` weights drawn from {0, 1/8, 1, 8} keyed by the name; the first one above 0, and at least one of each kind of value"""
    w = np.random.default_rng(_seed(name)).choice(WEIGHTS, size=count).astype(np.float32)
    w[0], w[1 % count] = 8.0, 0.125
    if count > 3:
        w[2], w[3] = 0.0, 1.0
    return w


def masks():
    """token masks on the 4 x 4 grid: the left half, a centre block that overlaps it, the bottom row"""
    left, centre, bottom = (torch.zeros(4, 4, dtype=torch.bool) for _ in range(3))
    left[:, :2] = True
    centre[1:3, 1:3] = True
    bottom[3] = True
    return left, centre, bottom


class Rq:
    """a request: `w` None = no weights on the global rows, else float32 [rows of glob] (a row of weight 0 is made NaN here);
    `regions` None = none, else (rows, mask) or (rows, mask, weight) items; scale a number, a tuple (a schedule) or None; neg the
    negative context's rows"""

    def __init__(self, name, T, temperature, topk, seed, k, glob, w=None, regions=None, scale=None, neg=None, top_p=None):
        self.name, self.T, self.temperature, self.topk, self.seed, self.k = name, T, temperature, topk, seed, k
        self.w, self.regions, self.scale, self.neg, self.top_p = w, regions, scale, neg, top_p
        self.glob = glob.clone()
        if w is not None:
            self.glob[torch.from_numpy(w == 0)] = float("nan")

    def submit(self, session):
        kw = dict(context=self.glob if self.w is None else (self.glob, self.w), timesteps=self.T, temperature=self.temperature,
                  topk=self.topk, seed=self.seed, image_index=self.k)
        if self.regions is not None:
            kw["regions"] = self.regions
        if self.scale is not None:
            kw["guidance_scale"] = list(self.scale) if isinstance(self.scale, tuple) else self.scale
        if self.neg is not None:
            kw["negative_context"] = self.neg
        if self.top_p is not None:
            kw["top_p"] = self.top_p
        h = session.submit(**kw)
        h.rq = self
        return h

    def row_weights(self):
        """the weights of the request's whole context (global rows, then every region's), or None when every one is 1"""
        parts = [np.ones(self.glob.shape[0], np.float32) if self.w is None else self.w]
        for item in self.regions or []:
            parts.append(np.full(item[0].shape[0], item[2] if len(item) == 3 else 1.0, np.float32))
        w = np.concatenate(parts)
        return w if (w != 1).any() else None


LEFT, CENTRE, BOTTOM = masks()
# the requests of the issue: weighted / weighted and regional (a weighted item, weights on the global rows) / plain with a short
# context that frees its slot after two steps / weighted, guided against a negative prompt under a schedule / a weighted one admitted
# into the freed slot at tick 2 / a regional one that outlives every weighted one (its last tick runs the two-launch form)
WA = Rq("WA", 4, 1.0, 5, 701, 7, rows("a", 10), drawn("a", 10))
WR = Rq("WR", 3, 0.9, 4, 702, 2 ** 33 + 1, rows("r", 8), drawn("r", 8), [(rows("r1", 12), LEFT, 0.125), (rows("r2", 9), CENTRE)])
P_ = Rq("P", 2, 0.8, 3, 703, 3, rows("p", 7))
GW = Rq("GW", 4, 1.1, 8, 704, 11, rows("g", 9), drawn("g", 9), scale=(0.5, 1.5, 2.5, 3.0), neg=rows("n", 4))
E = Rq("E", 3, 0.9, 4, 705, 13, rows("e", 12), drawn("e", 12))
R_ = Rq("R", 3, 1.0, 5, 706, 14, rows("q", 10), None, [(rows("q1", 15), BOTTOM)])
PLAN = [(0, WA), (0, WR), (0, P_), (0, GW), (2, E), (3, R_)]
WHERE = {"WA": (0, 0), "WR": (1, 0), "P": (2, 0), "GW": (3, 0), "E": (2, 2), "R": (1, 3)}       # (slot, admitted)
# another set of weights and another layout around P, GW, E and R: the same pass set and form per tick, so the same graphs
WA2 = Rq("WA2", 4, 1.0, 5, 701, 7, rows("a", 10), drawn("a2", 10))
WR2 = Rq("WR2", 3, 0.9, 4, 702, 2 ** 33 + 1, rows("r", 8), None, [(rows("r3", 30), BOTTOM, 8.0)])
OTHER_WEIGHTS = [(0, WA2), (0, WR2), (0, P_), (0, GW), (2, E), (3, R_)]
# the neighbours of WA made plain: regional without weights, guided without weights, plain
WR0 = Rq("WR0", 3, 0.9, 4, 702, 2 ** 33 + 1, rows("r", 8), None, [(rows("r1", 12), LEFT), (rows("r2", 9), CENTRE)])
G0 = Rq("G0", 4, 1.1, 8, 704, 11, rows("g", 9), scale=(0.5, 1.5, 2.5, 3.0), neg=rows("n", 4))
E0 = Rq("E0", 3, 0.9, 4, 705, 13, rows("e", 12))
OTHER_KINDS = [(0, WA), (0, WR0), (0, P_), (0, G0), (2, E0), (3, R_)]


def layout_of(pipe, rq):
    """-> (context rows [L_total, D], key_seg uint8 [L_total] or None, query_mask uint32 [N] or None, weights f32 [L_total] or None)"""
    w = rq.row_weights()
    if rq.regions is None:
        return rq.glob, None, None, w
    ctx, ks, qm = region_layout([[rq.glob] + [item[0] for item in rq.regions]], [[item[1] for item in rq.regions]], pipe.image_size,
                                pipe.patch_size)
    return ctx[0], ks[0], qm[0], w


def _scale_at(scale, step):
    return scale[step] if isinstance(scale, tuple) else scale


def reference_run(pipe, j, rq):
    """row j of the scalar path at B = S, eager, one stream: the final ids from generate_ids, the per-step pred and score from the
    scalar one-step entry with the step's values (the same kernels), whose ids must end where the loop ends"""
    V, N, eng = pipe.mask_token_id, pipe.num_tokens, pipe.engine()
    ctx_rows, ks_row, qm_row, w_row = layout_of(pipe, rq)
    L = ctx_rows.shape[0]
    context = torch.zeros(S, CAP, D, device=dev())
    context[j, :L] = ctx_rows.to(dev())
    if ks_row is None and w_row is None:
        lens = [CAP] * S
        lens[j] = L
        kw = dict(context_lens=lens)
    else:
        ks = np.zeros((S, CAP), np.uint8)                       # the other rows: one segment, every token attending to it, weights of 1
        qm = np.ones((S, N), np.uint32)
        ks[j, L:] = 255
        if ks_row is not None:
            ks[j, :L], qm[j] = ks_row, qm_row
        kw = dict(context_segments=ks, token_segments=qm)
        if w_row is not None:
            w = np.ones((S, CAP), np.float32)
            w[j, :L] = w_row
            kw["context_weights"] = w
    if rq.neg is not None:
        neg = torch.zeros(S, CAP_N, D, device=dev())
        neg[j, :rq.neg.shape[0]] = rq.neg.to(dev())
        nlens = [CAP_N] * S
        nlens[j] = rq.neg.shape[0]
        kw.update(negative_context=neg, negative_lens=nlens)
    topk = V if rq.topk is None else rq.topk
    ids_ref, _ = pipe.generate_ids(context, S, rq.T, rq.temperature, topk, [False] * rq.T, rq.seed, image_base=rq.k - j, use_graph=False,
                                   streams=1, guidance_scale=list(rq.scale) if isinstance(rq.scale, tuple) else rq.scale, top_p=rq.top_p, **kw)
    temps, nmask, _ = loop_schedule(rq.T, rq.temperature, N)
    ids = torch.full((S, N), V, dtype=torch.long, device=dev())
    preds, scores = [], []
    for step in range(rq.T):
        ids, _, pred, score = eng.sample(None, ids, context, topk, temps[step], nmask[step], seed=rq.seed, step=step, image_base=rq.k - j,
                                         want_img=False, want_aux=True, guidance_scale=_scale_at(rq.scale, step), top_p=rq.top_p, **kw)
        preds.append(pred[j].clone())
        scores.append(score[j].clone())
    assert torch.equal(ids, ids_ref)
    return ids_ref[j].clone(), preds, scores


def counters(eng):
    return eng.slots_passes(), eng.slots_filter_steps(), eng.slots_edit_steps(), eng.slots_region_steps(), eng.slots_weight_steps()


def run_session(pipe, use_graph, plan, filters=False, regions=True, weights=True, poison_at=None):
    """plan: [(tick, request)]: submitted at that tick, before its step.  poison_at: behind that tick's step NaN goes into every row
    of the session's context tensor that no request owns (behind an occupied slot's total, and all of an idle slot's), and the
    cross K/V are prepared again.  -> (the Finished list, (steps of the two-launch form, steps of the three-launch form) this
    session ran, ticks it took)"""
    s = pipe.decode_session(slots=S, conditional=True, use_graph=use_graph, record_steps=True, max_context_len=CAP, max_negative_len=CAP_N,
                            filters=filters, regions=regions, weights=weights)
    eng = pipe.engine()
    before = counters(eng)[3:]
    done, pending = [], sorted(plan, key=lambda x: x[0])
    while pending or not s.idle():
        while pending and pending[0][0] <= s.tick:
            pending.pop(0)[1].submit(s)
        done += s.step()
        if poison_at is not None and s.tick - 1 == poison_at:
            for j, r in enumerate(s.occupied):
                s._ctx[j, (0 if r is None else r.context.shape[0]):] = float("nan")
            s._ctx_dirty = True
    assert len(done) == len(plan)
    return done, tuple(np.subtract(counters(eng)[3:], before).tolist()), s.tick


def form_ticks(handles, ticks):
    """(ticks with a regional and no weighted slot occupied, ticks with a weighted slot occupied)"""
    live = lambda tk, pred: any(pred(h) and h.admitted <= tk <= h.retired for h in handles)
    weighted = [live(tk, lambda h: h.weights is not None) for tk in range(ticks)]
    regional = [live(tk, lambda h: h.segments is not None) for tk in range(ticks)]
    return sum(r and not w for r, w in zip(regional, weighted)), sum(weighted)


def check_contract(pipe, use_graph, plan, refs, **kw):
    done, steps, ticks = run_session(pipe, use_graph, plan, **kw)
    handles = [f.handle for f in done]
    assert steps == form_ticks(handles, ticks), (steps, form_ticks(handles, ticks))
    vq = pipe.vqgan.engine()
    for f in done:
        h = f.handle
        assert h.retired == h.admitted + h.timesteps - 1 and len(h.trace) == h.timesteps
        assert (h.segments is not None) == (h.rq.regions is not None) and (h.weights is not None) == (h.rq.row_weights() is not None)
        if h.weights is not None:
            assert np.array_equal(h.weights, h.rq.row_weights())
        key = (h.rq.name, h.slot, pipe.compute_dtype)
        if key not in refs:
            refs[key] = reference_run(pipe, h.slot, h.rq)
        ids_ref, preds, scores = refs[key]
        for step in range(h.timesteps):
            assert torch.equal(h.trace[step][0], preds[step]), (h.rq.name, h.slot, step, "pred")
            assert torch.equal(bits(h.trace[step][1]), bits(scores[step])), (h.rq.name, h.slot, step, "score")
        assert torch.equal(f.ids, ids_ref), (h.rq.name, h.slot)
        assert torch.equal(f.image, vq.decode_indices(h.trace[-1][0][None].contiguous())[0])
    return {f.handle.rq.name: f for f in done}


@pytest.fixture(scope="module")
def refs():
    """the scalar runs, computed once per (request, slot, dtype) and shared by every test below"""
    return {}


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_session_contract_and_the_neighbours_do_not_matter(pipe, refs, use_graph):
    eng = pipe.engine()
    # with the graph flag a form's first step runs eagerly, its second captures, the rest replay: the second and third session replay
    for _ in range(3 if use_graph else 1):
        done = check_contract(pipe, use_graph, PLAN, refs)
    assert {name: (f.handle.slot, f.handle.admitted) for name, f in done.items()} == WHERE      # the freed slot is taken at tick 2
    assert done["WR"].handle.context.shape[0] == 29 and bool(torch.isnan(done["WA"].handle.context).any())
    graphs = eng.graph_count()
    # another set of weights and another layout beside them: P, GW, E and R keep their scalar rows, and no graph-cache entry is added
    other = check_contract(pipe, use_graph, OTHER_WEIGHTS, refs)
    assert eng.graph_count() == graphs
    assert not torch.equal(other["WA2"].ids, done["WA"].ids)                # the weights were seen
    for name in ("P", "GW", "E", "R"):
        assert torch.equal(other[name].ids, done[name].ids)
    # plain neighbours in place of the weighted ones: WA keeps its scalar row (the reference is keyed by request and slot)
    kinds = check_contract(pipe, use_graph, OTHER_KINDS, refs)
    assert eng.graph_count() == graphs
    assert torch.equal(kinds["WA"].ids, done["WA"].ids)
    assert not (torch.equal(kinds["WR0"].ids, done["WR"].ids) and torch.equal(kinds["G0"].ids, done["GW"].ids) and
                torch.equal(kinds["E0"].ids, done["E"].ids))


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_nan_behind_a_total_and_in_idle_slots_reaches_nothing(pipe, refs, use_graph):
    """WA (weighted, NaN in its rows of weight 0) and P (plain) in slots 0 and 1, slots 2 and 3 idle; behind the first step NaN is
    written into every context row no request owns and the K/V are prepared again: the results are those of the scalar runs"""
    assert (WA.w == 0).any() and bool(torch.isnan(WA.glob).any())
    check_contract(pipe, use_graph, [(0, WA), (0, P_)], refs, poison_at=0)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_a_weights_session_without_a_weighted_request_runs_what_the_default_session_runs(tiny, refs, use_graph):
    plan = [(0, P_), (0, G0), (0, Rq("F", 2, 1.0, 2, 707, 12, rows("f", CAP))), (1, E0)]
    eng = tiny.engine()
    deltas, results = [], []
    for weights in (False, True):
        graphs, before = eng.graph_count(), counters(eng)
        for _ in range(3 if use_graph else 1):
            done, steps, _ = run_session(tiny, use_graph, plan, regions=False, weights=weights)
        assert steps == (0, 0)
        deltas.append(tuple(np.subtract(a, b).tolist() for a, b in zip(counters(eng), before)))
        results.append({f.handle.rq.name: f.ids for f in done})
        if weights:
            assert eng.graph_count() == graphs                              # ... through the graphs the default session captured
    assert deltas[0] == deltas[1] and deltas[1][3:] == (0, 0)
    assert all(torch.equal(results[0][name], results[1][name]) for name in results[0])


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_with_the_filters_as_well(tiny, refs, use_graph):
    """weights=True composes with filters=True: a weighted request without a top-k, at a nucleus mass of 0.9, beside a plain one"""
    wide = Rq("W9", 3, 1.0, None, 801, 21, rows("a", 10), drawn("a", 10), top_p=0.9)
    for _ in range(3 if use_graph else 1):
        done = check_contract(tiny, use_graph, [(0, wide), (0, P_)], refs, filters=True, regions=False)
    assert (done["W9"].handle.topk, done["W9"].handle.top_p) == (tiny.mask_token_id, 0.9)
    twin = reference_run(tiny, 0, Rq("W5", 3, 1.0, 5, 801, 21, rows("a", 10), drawn("a", 10)))[0]
    assert not torch.equal(twin, done["W9"].ids)                            # the filters were seen


def _cpu_scores(cpu, rq, pred, with_weights=True):
    """1 - p(pred) of the all-mask state under the request's context on the plain-torch branch"""
    ctx, ks, qm, w = layout_of(cpu, rq)
    L = ctx.shape[0]
    ks = np.zeros((1, L), np.uint8) if ks is None else ks[None]
    qm = np.ones((1, cpu.num_tokens), np.uint32) if qm is None else qm[None]
    tok = cpu.ids2tokens(torch.full((1, cpu.num_tokens), cpu.mask_token_id, dtype=torch.long))
    kw = dict(context_weights=w[None]) if with_weights else {}
    with torch.no_grad():
        logits = cpu.tokens2logits(tok, (ctx if with_weights else torch.nan_to_num(ctx))[None], context_segments=ks, token_segments=qm, **kw)
    return 1 - logits.softmax(-1)[0].gather(1, pred[:, None])[:, 0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_first_step_scores_against_the_cpu_branch(tiny, dtype):
    """the score of a session's first step is 1 - p(pred) under the weighted logits: against the plain-torch branch of the same model
    on request WA's weights.  fp32-verify is gated at the project's float bar, the bf16 figure and the figure without the weights are
    printed.  On the CPU alone: the weights move the scores well beyond the bar (10 x)."""
    tiny.set_compute_dtype(dtype)
    try:
        s = tiny.decode_session(slots=S, conditional=True, use_graph=False, record_steps=True, max_context_len=CAP, weights=True)
        h = WA.submit(s)
        P_.submit(s)
        s.step()
        pred, score = h.trace[0][0].cpu(), h.trace[0][1].cpu()
    finally:
        tiny.set_compute_dtype(torch.float32)
    cpu = _tiny()
    want, loose = _cpu_scores(cpu, WA, pred), _cpu_scores(cpu, WA, pred, with_weights=False)
    err, gap = float((score - want).abs().max()), float((loose - want).abs().max())
    print(f"{dtype}: max |score GPU session - score CPU branch| at step 0 of a weighted request = {err:.3e}; CPU without the weights {gap:.3e}")
    assert gap > 10 * TOL
    if dtype == torch.float32:
        assert err < TOL


def test_step_entry_refuses_bad_arrays_before_anything_runs(tiny):
    pipe = tiny
    eng = pipe.engine().clone()                                             # a handle no slots call has touched
    N, V = pipe.num_tokens, pipe.mask_token_id
    ids = torch.full((2, N), V, dtype=torch.long, device=dev())
    start = ids.clone()
    ctx = torch.randn(2, 5, D, device=dev())
    recs = (_lib.Slot * 2)(_lib.Slot(1, 0, 1.0, 3, 4, 0), _lib.Slot(2, 1, 1.0, 3, 4, 0))
    ks = np.array([[0, 1, 1, 255, 255], [0, 0, 0, 0, 0]], np.uint8)
    qm = np.ones((2, N), np.uint32)
    qm[0, 3] = 3
    w = np.array([[1, 0, 8, 1, 1], [1, 1, 1, 1, 1]], np.float32)
    kinds = np.array([2, 0], np.uint8)
    dead = qm.copy()
    dead[0, 9] = 0b10                                                       # segment 1: row 1 has weight 0 ...
    w_dead = w.copy()
    w_dead[0, 2] = 0                                                        # ... and now row 2 as well
    big = w.copy()
    big[0, 4] = 2.0 ** 21                                                   # (a padding row: the range holds for every row of the slot)
    for segments, weights, words in (((ks, dead, kinds), w_dead, ("slot 0", "token 9", "allows no context row with a weight above 0")),
                                     ((ks, qm, kinds), big, ("slot 0", "context row 4", "must be 0 or in")),
                                     ((ks, qm, np.array([2, 3], np.uint8)), w, ("slot 1", "region_host=3")),
                                     (None, w, ("ctx_w_host given without",))):
        with pytest.raises(_lib.PmhipError) as e:
            eng.step_slots(ids, ctx, recs, segments=segments, weights=weights)
        assert e.value.code == _lib.PMHIP_EINVAL and all(x in str(e.value) for x in words), str(e.value)
    with pytest.raises(_lib.PmhipError) as e:                               # kind 2 without the weights array
        eng.step_slots(ids, ctx, recs, segments=(ks, qm, kinds))
    assert e.value.code == _lib.PMHIP_EINVAL and "region_host=2" in str(e.value)
    with pytest.raises(ValueError, match="weights"):
        eng.step_slots(ids, ctx, recs, segments=(ks, qm, kinds), weights=w[:, :4])
    torch.cuda.synchronize()
    assert torch.equal(ids, start) and counters(eng) == ((0, 0, 0), (0, 0), 0, 0, 0)                 # nothing ran
    # no slot of kind 2: the step of the entry without the weights (garbage in them is not looked at); then slot 0 weighted
    junk = np.full((2, 5), np.nan, np.float32)
    eng.step_slots(ids, ctx, recs, segments=(ks, qm, np.array([1, 0], np.uint8)), weights=junk)
    assert (eng.slots_region_steps(), eng.slots_weight_steps()) == (1, 0)
    regional = ids.clone()
    ids.copy_(start)
    eng.step_slots(ids, ctx, recs, segments=(ks, qm, np.array([1, 0], np.uint8)))
    assert torch.equal(ids, regional)
    ids.copy_(start)
    junk[0] = w[0]
    eng.step_slots(ids, ctx, recs, segments=(ks, qm, kinds), weights=junk)
    assert (eng.slots_region_steps(), eng.slots_weight_steps()) == (2, 1) and torch.equal(ids[1], regional[1])   # slot 1: its plain row


def test_the_three_launch_form_has_one_further_graph_key_for_every_mix(tiny):
    eng = tiny.engine().clone()
    N, V = tiny.num_tokens, tiny.mask_token_id
    ids = torch.full((2, N), V, dtype=torch.long, device=dev())
    ctx = torch.randn(2, 5, D, device=dev())
    recs = (_lib.Slot * 2)(_lib.Slot(1, 0, 1.0, 3, 4, 0), _lib.Slot(2, 1, 1.0, 3, 4, 0))
    ks = np.array([[0, 1, 1, 255, 255], [0, 0, 0, 1, 255]], np.uint8)
    qm = np.full((2, N), 3, np.uint32)
    w = np.array([[1, 0.125, 8, 1, 1], [8, 1, 0, 1, 1]], np.float32)
    for _ in range(3):                                                      # eager, capture, replay: the two-launch form
        eng.step_slots(ids, ctx, recs, use_graph=True, context_lens=[3, 4], segments=(ks, qm, np.array([1, 0], np.uint8)))
    entries, captured = eng.graph_count()
    assert captured >= 1
    n = 0
    for kinds in ([2, 0], [0, 2], [2, 1], [2, 2], [1, 2]):
        for lens, wts in (([3, 4], w), (None, w[::-1].copy())):
            for _ in range(2):
                eng.step_slots(ids, ctx, recs, use_graph=True, context_lens=lens, segments=(ks, qm, np.array(kinds, np.uint8)), weights=wts)
                n += 1
    assert eng.graph_count() == (entries + 1, captured + 1) and (eng.slots_region_steps(), eng.slots_weight_steps()) == (3, n)
    eng.step_slots(ids, ctx, recs, use_graph=True, context_lens=[3, 4], segments=(ks, qm, np.array([1, 0], np.uint8)), weights=w)
    assert eng.graph_count() == (entries + 1, captured + 1) and (eng.slots_region_steps(), eng.slots_weight_steps()) == (4, n)
