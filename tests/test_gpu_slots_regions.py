"""Regional prompts per request in decode sessions, on the GPU: the contract of paintmind_amd/serve.py.  A
regional request in slot j of an S-slot session computes, bit for bit, the per-step predictions, the scores and the final ids of row j
of ``generate_ids(context [S, capacity, D] with its rows in row j, context_segments / token_segments with its layout in row j and a
one-segment layout in the other rows, B=S, ..., image_base=k - j, streams=1)``; a request without regions beside it still computes row
j of ``generate_ids(..., context_lens=...)``; both whatever shares the batch.  Tiny pipeline (16 tokens), S = 4, fp32-verify and
bf16, eager and with PMHIP_SLOTS_GRAPH.  There is no tolerance in this file except the project's fp32 bar against the CPU branch."""
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
TOL = 1e-3                       # the project's float bar (tests/test_gpu_regions.py)
S, CAP, CAP_N, D = 4, 40, 6, 96


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


def rows(name, count):
    """`count` context rows of N(0, 1) keyed by the name"""
    return torch.randn(count, D, generator=torch.Generator().manual_seed(sum(ord(c) * 131 ** i for i, c in enumerate(name))))


def masks():
    """token masks on the 4 x 4 grid: the left half, a centre block that overlaps it, the bottom row"""
    left, centre, bottom = (torch.zeros(4, 4, dtype=torch.bool) for _ in range(3))
    left[:, :2] = True
    centre[1:3, 1:3] = True
    bottom[3] = True
    return left, centre, bottom


class Rq:
    """a request: `regions` None = a plain one; scale a number, a tuple (a schedule) or None; neg the negative context's rows"""

    def __init__(self, name, T, temperature, topk, seed, k, glob, regions=None, scale=None, neg=None, top_p=None):
        self.name, self.T, self.temperature, self.topk, self.seed, self.k = name, T, temperature, topk, seed, k
        self.glob, self.regions, self.scale, self.neg, self.top_p = glob, regions, scale, neg, top_p

    def submit(self, session):
        kw = dict(context=self.glob, timesteps=self.T, temperature=self.temperature, topk=self.topk, seed=self.seed, image_index=self.k)
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


LEFT, CENTRE, BOTTOM = masks()
# the requests of the issue: two overlapping regions / plain with a short context / regional, guided against a negative prompt under a
# schedule / a filler that frees its slot after two steps / a regional one admitted into that slot at tick 2
A = Rq("A", 4, 1.0, 5, 501, 7, rows("a", 10), [(rows("a1", 12), LEFT), (rows("a2", 9), CENTRE)])
P_ = Rq("P", 3, 0.8, 3, 502, 2 ** 33 + 1, rows("p", 7))
G = Rq("G", 4, 1.1, 8, 503, 11, rows("g", 8), [(rows("g1", 15), BOTTOM)], scale=(0.5, 1.5, 2.5, 3.0), neg=rows("n", 4))
FILL = Rq("F", 2, 1.0, 2, 504, 12, rows("f", CAP))
E = Rq("E", 3, 0.9, 4, 505, 13, rows("e", 5), [(rows("e1", 6), CENTRE), (rows("e2", 3), LEFT), (rows("e3", 20), BOTTOM)])
PLAN = [(0, A), (0, P_), (0, G), (0, FILL), (2, E)]
WHERE = {"A": (0, 0), "P": (1, 0), "G": (2, 0), "F": (3, 0), "E": (3, 2)}                 # (slot, admitted)
# other layouts around P, G and E: the same pass set per tick, so the same graphs
A2 = Rq("A2", 4, 1.0, 5, 501, 7, rows("a", 3), [(rows("a2", 30), BOTTOM)])
OTHER_LAYOUT = [(0, A2), (0, P_), (0, G), (0, FILL), (2, E)]
# the neighbours of A exchanged: regional where there was a plain one, plain and unguided where there were regional ones
P2 = Rq("P2", 3, 0.8, 3, 502, 2 ** 33 + 1, rows("p", 7), [(rows("p1", 33), LEFT)])
G2 = Rq("G2", 4, 1.1, 8, 503, 11, rows("g", 8))
E2 = Rq("E2", 3, 0.9, 4, 505, 13, rows("e", 5))
OTHER_KINDS = [(0, A), (0, P2), (0, G2), (0, FILL), (2, E2)]


def layout_of(pipe, rq):
    """-> (context rows [L_total, D], key_seg uint8 [L_total] or None, query_mask uint32 [N] or None)"""
    if rq.regions is None:
        return rq.glob, None, None
    ctx, ks, qm = region_layout([[rq.glob] + [r for r, _ in rq.regions]], [[m for _, m in rq.regions]], pipe.image_size, pipe.patch_size)
    return ctx[0], ks[0], qm[0]


def _scale_at(scale, step):
    return scale[step] if isinstance(scale, tuple) else scale


def reference_run(pipe, j, rq):
    """row j of the scalar path at B = S, eager, one stream: the final ids from generate_ids, the per-step pred and score from the
    scalar one-step entry with the step's values (the same kernels), whose ids must end where the loop ends"""
    V, N, eng = pipe.mask_token_id, pipe.num_tokens, pipe.engine()
    ctx_rows, ks_row, qm_row = layout_of(pipe, rq)
    L = ctx_rows.shape[0]
    context = torch.zeros(S, CAP, D, device=dev())
    context[j, :L] = ctx_rows.to(dev())
    if ks_row is None:
        lens = [CAP] * S
        lens[j] = L
        kw = dict(context_lens=lens)
    else:
        ks = np.zeros((S, CAP), np.uint8)                       # the other rows: one segment, every token attending to it
        qm = np.ones((S, N), np.uint32)
        ks[j, :L], ks[j, L:], qm[j] = ks_row, 255, qm_row
        kw = dict(context_segments=ks, token_segments=qm)
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


def run_session(pipe, use_graph, plan, filters=False, regions=True, poison_at=None):
    """plan: [(tick, request)]: submitted at that tick, before its step.  poison_at: behind that tick's step NaN goes into every row
    of the session's context tensor that no request owns (behind an occupied slot's total, and all of an idle slot's), and the
    cross K/V are prepared again.  -> (the Finished list, steps of the two-launch form this session ran, ticks it took)"""
    s = pipe.decode_session(slots=S, conditional=True, use_graph=use_graph, record_steps=True, max_context_len=CAP, max_negative_len=CAP_N,
                            filters=filters, regions=regions)
    eng = pipe.engine()
    before = eng.slots_region_steps()
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
    return done, eng.slots_region_steps() - before, s.tick


def regional_ticks(handles, ticks):
    return sum(1 for tk in range(ticks) if any(h.segments is not None and h.admitted <= tk <= h.retired for h in handles))


def check_contract(pipe, use_graph, plan, refs, **kw):
    done, region_steps, ticks = run_session(pipe, use_graph, plan, **kw)
    handles = [f.handle for f in done]
    assert region_steps == regional_ticks(handles, ticks), (region_steps, regional_ticks(handles, ticks))
    vq = pipe.vqgan.engine()
    for f in done:
        h = f.handle
        assert h.retired == h.admitted + h.timesteps - 1 and len(h.trace) == h.timesteps
        assert (h.segments is not None) == (h.rq.regions is not None)
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
    assert done["A"].handle.context.shape[0] == 31 and done["E"].handle.context.shape[0] == 34
    graphs = eng.graph_count()
    # another layout beside them: P, G and E keep their scalar rows, and no graph-cache entry is added
    other = check_contract(pipe, use_graph, OTHER_LAYOUT, refs)
    assert eng.graph_count() == graphs
    assert not torch.equal(other["A2"].ids, done["A"].ids)
    for name in ("P", "G", "E"):
        assert torch.equal(other[name].ids, done[name].ids)
    # regional neighbours made plain and the plain one regional: A keeps its scalar row (the reference is keyed by request and slot)
    kinds = check_contract(pipe, use_graph, OTHER_KINDS, refs)
    assert torch.equal(kinds["A"].ids, done["A"].ids)
    assert not torch.equal(kinds["P2"].ids, done["P"].ids)                  # the regions were seen
    assert not torch.equal(kinds["E2"].ids, done["E"].ids) or not torch.equal(kinds["G2"].ids, done["G"].ids)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_nan_behind_a_total_and_in_idle_slots_reaches_nothing(pipe, refs, use_graph):
    """A (regional) and P (plain) in slots 0 and 1, slots 2 and 3 idle; behind the first step NaN is written into every context row
    no request owns and the K/V are prepared again: the results are those of the scalar runs"""
    check_contract(pipe, use_graph, [(0, A), (0, P_)], refs, poison_at=0)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_a_regions_session_without_a_regional_request_runs_what_the_default_session_runs(tiny, refs, use_graph):
    plan = [(0, P_), (0, G2), (0, FILL), (1, E2)]
    counters = lambda e: (e.slots_passes(), e.slots_filter_steps(), e.slots_edit_steps(), e.slots_region_steps())
    eng = tiny.engine()
    deltas, results = [], []
    for regions in (False, True):
        graphs, before = eng.graph_count(), counters(eng)
        for _ in range(3 if use_graph else 1):
            done, region_steps, _ = run_session(tiny, use_graph, plan, regions=regions)
        assert region_steps == 0
        after = counters(eng)
        deltas.append(tuple(np.subtract(a, b).tolist() for a, b in zip(after, before)))
        results.append({f.handle.rq.name: f.ids for f in done})
        if regions:
            assert eng.graph_count() == graphs                              # ... through the graphs the default session captured
    assert deltas[0] == deltas[1] and deltas[1][3] == 0
    assert all(torch.equal(results[0][name], results[1][name]) for name in results[0])


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_with_the_filters_as_well(tiny, refs, use_graph):
    """regions=True composes with filters=True: a regional request without a top-k, at a nucleus mass of 0.9, beside a plain one"""
    wide = Rq("W", 3, 1.0, None, 601, 21, rows("a", 10), A.regions, top_p=0.9)
    for _ in range(3 if use_graph else 1):
        done = check_contract(tiny, use_graph, [(0, wide), (0, P_)], refs, filters=True)
    assert (done["W"].handle.topk, done["W"].handle.top_p) == (tiny.mask_token_id, 0.9)
    twin = reference_run(tiny, 0, Rq("W5", 3, 1.0, 5, 601, 21, rows("a", 10), A.regions))[0]
    assert not torch.equal(twin, done["W"].ids)                             # the filters were seen


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_first_step_scores_against_the_cpu_branch(tiny, dtype):
    """the score of a session's first step is 1 - p(pred) under the regional logits: against the plain-torch branch of the same
    model on request A's layout.  fp32-verify is gated at the project's float bar, the bf16 figure is printed.  Counter-check: the
    CPU branch WITHOUT the arrays is far from it."""
    tiny.set_compute_dtype(dtype)
    try:
        s = tiny.decode_session(slots=S, conditional=True, use_graph=False, record_steps=True, max_context_len=CAP, regions=True)
        h = A.submit(s)
        P_.submit(s)
        s.step()
        pred, score = h.trace[0][0].cpu(), h.trace[0][1].cpu()
    finally:
        tiny.set_compute_dtype(torch.float32)
    cpu = _tiny()
    ctx, ks, qm = layout_of(cpu, A)
    tok = cpu.ids2tokens(torch.full((1, cpu.num_tokens), cpu.mask_token_id, dtype=torch.long))
    with torch.no_grad():
        want = 1 - cpu.tokens2logits(tok, ctx[None], context_segments=ks[None], token_segments=qm[None]).softmax(-1)[0].gather(1, pred[:, None])[:, 0]
        loose = 1 - cpu.tokens2logits(tok, ctx[None]).softmax(-1)[0].gather(1, pred[:, None])[:, 0]
    err, gap = float((score - want).abs().max()), float((loose - want).abs().max())
    print(f"{dtype}: max |score GPU session - score CPU branch| at step 0 of a two-region request = {err:.3e}; CPU without the arrays {gap:.3e}")
    if dtype == torch.float32:
        assert err < TOL
        assert gap > 10 * err


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
    flags = np.array([1, 0], np.uint8)
    no_key = qm.copy()
    no_key[0, 9] = 0b100                                                    # segment 2: no row of slot 0 has it
    for segments, context, words in (((ks, no_key, flags), ctx, ("slot 0", "token 9", "allows no segment")),
                                     ((ks, qm, np.array([1, 2], np.uint8)), ctx, ("slot 1", "region_host=2")),
                                     ((ks[:, :0], qm, flags), None, ("without a context",))):
        with pytest.raises(_lib.PmhipError) as e:
            eng.step_slots(ids, context, recs, segments=segments)
        assert e.value.code == _lib.PMHIP_EINVAL and all(w in str(e.value) for w in words), str(e.value)
    with pytest.raises(ValueError, match="segments"):
        eng.step_slots(ids, ctx, recs, segments=(ks[:, :4], qm, flags))
    torch.cuda.synchronize()
    assert torch.equal(ids, start) and eng.slots_region_steps() == 0 and eng.slots_passes() == (0, 0, 0)        # nothing ran
    # flags of 0 everywhere: the step of the entry without the arrays (garbage in them is not looked at); then slot 0 regional
    junk = np.full((2, 5), 77, np.uint8)
    eng.step_slots(ids, ctx, recs, segments=(junk, np.zeros((2, N), np.uint32), np.zeros(2, np.uint8)))
    assert eng.slots_region_steps() == 0 and eng.slots_passes() == (1, 0, 0)
    plain = ids.clone()
    ids.copy_(start)
    eng.step_slots(ids, ctx, recs)
    assert torch.equal(ids, plain)
    ids.copy_(start)
    junk[0] = ks[0]
    eng.step_slots(ids, ctx, recs, segments=(junk, qm, flags))
    assert eng.slots_region_steps() == 1 and torch.equal(ids[1], plain[1])                    # slot 1: its row of the plain step


def test_the_two_launch_form_has_one_further_graph_key_for_every_mix(tiny):
    eng = tiny.engine().clone()
    N, V = tiny.num_tokens, tiny.mask_token_id
    ids = torch.full((2, N), V, dtype=torch.long, device=dev())
    ctx = torch.randn(2, 5, D, device=dev())
    recs = (_lib.Slot * 2)(_lib.Slot(1, 0, 1.0, 3, 4, 0), _lib.Slot(2, 1, 1.0, 3, 4, 0))
    ks = np.array([[0, 1, 1, 255, 255], [0, 0, 0, 1, 255]], np.uint8)
    qm = np.full((2, N), 3, np.uint32)
    for _ in range(3):                                                      # eager, capture, replay
        eng.step_slots(ids, ctx, recs, use_graph=True, context_lens=[3, 4])
    entries, captured = eng.graph_count()
    assert captured >= 1
    for flags in ([1, 0], [0, 1], [1, 1], [1, 0]):
        for lens in ([3, 4], None):
            for _ in range(2):
                eng.step_slots(ids, ctx, recs, use_graph=True, context_lens=lens, segments=(ks, qm, np.array(flags, np.uint8)))
    assert eng.graph_count() == (entries + 1, captured + 1) and eng.slots_region_steps() == 16
    eng.step_slots(ids, ctx, recs, use_graph=True, context_lens=[3, 4], segments=(ks, qm, np.zeros(2, np.uint8)))
    assert eng.graph_count() == (entries + 1, captured + 1) and eng.slots_region_steps() == 16      # no regional slot: the plain step's graph
