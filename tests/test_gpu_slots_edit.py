"""Edit requests in decode sessions, on the GPU: the re-masking kernels that take the step values from a
slot record AND a count per slot, against the existing entries include/pmhip.h names for each row; and the contract of
paintmind_amd/serve.py -- an edit request (T, temperature, topk[, top_p], seed, k, context, choice temperature, guidance) with start
ids x (m mask ids) in slot j of an S-slot session computes, bit for bit, the per-step predictions and scores and the final ids of row
j of ``Pipeline.edit_ids(ids with x in row j, counts with m in row j, ..., B=S, image_base=k - j, use_graph=False)``, whatever shares
the batch with it, and a generation beside it still computes its ``generate_ids`` row.  Both sides of every comparison run the same
selection code: there is no tolerance in this file."""
import ctypes as C

import pytest
import torch

import paintmind_amd as pm
from abi_frames import bits, call, framed
from edit_ref import MASK_ID, scores_with_ties
from gpu_common import dev, t
from negative_ref import PromptRows
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline, edit_schedule, loop_schedule
from util import load_golden, to_torch_sd

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------------------------
# operator level
# ------------------------------------------------------------------------------------------------------------------------------
IDLE = 6                                 # the idle slot of the operator cases; its count and choice temperature are garbage
B_OP = 10


def _counts(N):
    """-1, 0, 1, N/3, N-1, N, N+5, -1, 0 over the nine active slots"""
    c = [-1, 0, 1, N // 3, N - 1, N, N + 5, -1, 0]
    c.insert(IDLE, 0x7FFFFFF0)
    return c


def _records(N):
    """(seed, image_index, temperature, topk, num_mask, step) per slot, all different: image indices whose row counters pass 2^32
    (and 2^64 / N), a seed with both words set; the record's own count is 0 in slot 0 (the clamp to 1) and N/2 in slot 8 -- the two
    slots at -1 -- and something the kernel must not use everywhere else"""
    index = [7, 2 ** 33 + 5, 4096, 2 ** 32, 1, 2 ** 32 + 3, 12, 2 ** 62 + 1, 2 ** 31, 99]
    nm = [0, 3, 5, 1, 2, 7, 4, 9, max(N // 2, 1), 6]
    recs = [(0x0123456789ABCDEF + 1000003 * b, index[b], 1.0, 5, nm[b], 3 * b + 1) for b in range(B_OP)]
    recs[IDLE] = None
    return recs


CHOICE = [4.5, 0.0, 2.0, 0.0, 1.0, 1000.0, float("nan"), 0.5, 3.0, 0.0]


@pytest.fixture(scope="module")
def operator_case():
    """per N, computed once and left unchanged: ids, scores with planted ties and given ids, records, counts, choice values, and per
    row what the entry the header names for it leaves (plain and choice)"""
    cache = {}

    def get(N):
        if N in cache:
            return cache[N]
        ids_np, scores_np = scores_with_ties(B_OP, N, seed=7 * N + 1)
        ids, scores = t(ids_np), t(scores_np)
        recs, counts = _records(N), _counts(N)
        slots = ops.pack_slots(recs, dev())
        cd = torch.tensor(counts, dtype=torch.int32, device=dev())
        choice = torch.tensor(CHOICE, dtype=torch.float32, device=dev())
        want = {}
        for with_choice in (False, True):
            rows = []
            for b, (rec, c) in enumerate(zip(recs, counts)):
                row, sc = ids[b:b + 1].clone(), scores[b:b + 1].clone()
                if rec is None or c == 0:
                    pass                                                   # its input
                elif c < 0:                                                # the slots entry on that row: the record's num_mask
                    ops.remask_slots(row, sc, slots[b:b + 1].contiguous(), MASK_ID, choice=choice[b:b + 1].contiguous() if with_choice else None)
                else:                                                      # the counts entry on that row ALONE with the slot's values
                    seed, k, _, _, _, step = rec
                    ops.remask_counts(row, sc, cd[b:b + 1].contiguous(), MASK_ID, choice_temperature=CHOICE[b] if with_choice else 0.0,
                                      seed=seed, step=step, row_base=(k * N) & (2 ** 64 - 1))
                rows.append(row)
            want[with_choice] = torch.cat(rows)
        cache[N] = dict(ids=ids, scores=scores, recs=recs, counts=counts, slots=slots, cd=cd, choice=choice, want=want)
        return cache[N]
    return get


# N: 16 (E = 1), 1000 and 1024 (E = 4: a ragged and a full last thread), and one N per further instantiated class: 500 (E = 2), 2000
# (E = 8), 4096 (E = 16)
@pytest.mark.parametrize("with_choice", [False, True], ids=["plain", "choice"])
@pytest.mark.parametrize("N", [16, 1000, 1024, 500, 2000, 4096])
def test_every_row_equals_the_entry_the_header_names_for_it(operator_case, N, with_choice):
    case = operator_case(N)
    fi = framed(B_OP, N, ld=N, dtype=torch.int64, payload=case["ids"])
    fs = framed(B_OP, N, ld=N, dtype=torch.float32, payload=case["scores"], fill="nan")
    fr = framed(B_OP, 32, ld=32, dtype=torch.uint8, payload=case["slots"])
    fc = framed(B_OP, 1, ld=1, dtype=torch.int32, payload=case["cd"].reshape(B_OP, 1))
    fh = framed(B_OP, 1, ld=1, dtype=torch.float32, payload=case["choice"].reshape(B_OP, 1), fill="nan")
    if with_choice:
        call("pmhip_remask_choice_slots_counts", fi, fs, fr, fh, fc, MASK_ID, B_OP, N)
    else:
        call("pmhip_remask_slots_counts", fi, fs, fr, fc, MASK_ID, B_OP, N)
    for f, what in ((fi, "ids"), (fs, "scores"), (fr, "slots"), (fc, "counts"), (fh, "choice")):
        f.assert_frame_untouched(what)
    assert torch.equal(bits(fs.payload()), bits(case["scores"])) and torch.equal(fc.payload().reshape(-1), case["cd"])     # inputs are inputs
    got, want, ids = fi.payload(), case["want"][with_choice], case["ids"]
    for b, c in enumerate(case["counts"]):
        assert torch.equal(got[b], want[b]), (N, b, c)
        masked = int((got[b] == MASK_ID).sum())
        if b == IDLE or c == 0:
            assert torch.equal(got[b], ids[b]) and masked == 0, (N, b)             # bitwise untouched
        elif c > 0:
            assert masked == min(c, N), (N, b, c)                                   # exactly c; above N: the row
        else:
            assert masked == max(case["recs"][b][4], 1), (N, b)                     # the record's, with the clamp to 1
    # the Python operator is the same call
    again = ops.remask_slots_counts(ids.clone(), case["scores"], case["slots"], case["cd"], MASK_ID, choice=case["choice"] if with_choice else None)
    assert torch.equal(again, got)
    if with_choice:
        # a choice array of zeros IS the plain form, and the noise was seen where a slot has a temperature
        zero = ops.remask_slots_counts(ids.clone(), case["scores"], case["slots"], case["cd"], MASK_ID, choice=torch.zeros(B_OP, device=dev()))
        assert torch.equal(zero, case["want"][False])
        if N >= 500:
            assert not torch.equal(got, case["want"][False])


def test_einval_cases_launch_nothing(operator_case):
    N = 16
    case = operator_case(N)
    ids = case["ids"].clone()
    ok = (ids, case["scores"], case["slots"], case["choice"], case["cd"])
    for name, args in (("pmhip_remask_slots_counts", ok[:3] + ok[4:]), ("pmhip_remask_choice_slots_counts", ok)):
        for hole in range(len(args)):
            with pytest.raises(_lib.PmhipError) as e:
                call(name, *[None if i == hole else a for i, a in enumerate(args)], MASK_ID, B_OP, N)
            assert e.value.code == _lib.PMHIP_EINVAL and "null pointer" in str(e.value)
        for B, n in ((0, N), (B_OP, 0), (B_OP, 4097), (-3, N)):
            with pytest.raises(_lib.PmhipError) as e:
                call(name, *args, MASK_ID, B, n)
            assert e.value.code == _lib.PMHIP_EINVAL and "bad shape" in str(e.value)
    torch.cuda.synchronize()
    assert torch.equal(ids, case["ids"])
    with pytest.raises(ValueError):
        ops.remask_slots_counts(ids, case["scores"], case["slots"], case["cd"].to(torch.int64), MASK_ID)
    with pytest.raises(ValueError):
        ops.remask_slots_counts(ids, case["scores"], case["slots"], case["cd"][:-1].contiguous(), MASK_ID)


# ------------------------------------------------------------------------------------------------------------------------------
# the contract, on the tiny pipeline (16 tokens)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    p, _ = load_golden("tiny_pipeline.npz")
    cfg = pm.Config(pm.ver2cfg["tiny-pipeline"])
    pipe = Pipeline(cfg, stage1_pretrained=False, text_model=PromptRows(cfg.context_dim, 7, 3))
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("text_model") for k in missing.missing_keys)
    return pipe.to(dev()).eval()


@pytest.fixture(params=[torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def pipe(request, tiny):
    tiny.set_compute_dtype(request.param)
    yield tiny
    tiny.set_compute_dtype(torch.float32)


S = 5


def rq(T, temperature, topk, seed, k, m=None, scale=None, choice=None, top_p=None):
    """a request: m None: a generation; else an edit over m masked positions of an encoded image.  scale: conditional sessions only"""
    return (T, temperature, topk, seed, k, m, scale, choice, top_p)


# seven requests into five slots, submitted at once: the first five are admitted at tick 0, the last two wait for a slot.
#   slot 0   edit m = 5, T = 8 (schedule [4,3,2,1,0,0,0,0])                    ticks 0..7
#   slot 1   generation T = 3                ticks 0..2, then generation T = 5  ticks 3..7
#   slot 2   edit m = N, T = 4               ticks 0..3
#   slot 3   edit m = 0, T = 2               ticks 0..1, then edit m = 1, T = 3  ticks 2..4
#   slot 4   edit m = 7 with guidance and a choice temperature, T = 5            ticks 0..4
PLAN = [rq(8, 1.0, 5, 901, 7, m=5), rq(3, 0.7, 3, 902, 9), rq(4, 1.0, 5, 903, 2 ** 33 + 1, m=16), rq(2, 1.3, 1, 904, 11, m=0),
        rq(5, 0.9, 8, 905, 30, m=7, scale=2.5, choice=4.5), rq(3, 1.0, 4, 906, 12, m=1), rq(5, 1.1, 5, 907, 13)]
# the same shape of session with other masks, seeds and areas: it must go through the graphs PLAN captured
OTHER = [rq(8, 1.0, 5, 911, 7, m=9), rq(3, 0.7, 3, 912, 9), rq(4, 1.0, 5, 913, 2 ** 33 + 1, m=15), rq(2, 1.3, 1, 914, 11, m=2),
         rq(5, 0.9, 8, 915, 30, m=3, scale=2.5, choice=4.5), rq(3, 1.0, 4, 916, 12, m=16), rq(5, 1.1, 5, 917, 13)]
SLOTS_OF_PLAN = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (3, 2), (1, 3)]               # (slot, admitted) of every request


def _starts(pipe, plan, seed):
    """per request None (a generation) or its start ids [N]: an encoded random image with m random positions masked"""
    N = pipe.num_tokens
    g = torch.Generator().manual_seed(seed)
    img = (torch.rand(len(plan), 3, pipe.image_size, pipe.image_size, generator=g) * 2 - 1).to(dev())
    enc = pipe.to_latent(img)[1].reshape(len(plan), N).clone()
    out = []
    for i, req in enumerate(plan):
        m = req[5]
        if m is None:
            out.append(None)
            continue
        x = enc[i].clone()
        x[torch.randperm(N, generator=g)[:m].to(dev())] = pipe.mask_token_id
        out.append(x)
    return out


def _contexts(pipe, n):
    return list(pipe.text_model([f"p{i}" for i in range(n)]).to(dev()))


def reference_run(pipe, j, req, start, ctx_row):
    """row j of the scalar path at B = S, eager: the final ids from edit_ids / generate_ids; the per-step pred and score from the
    scalar one-step entry with the step's values (the same kernels) and, for an edit, ops.remask on every row ALONE with its count --
    whose ids must end where the loop ends"""
    T, temperature, topk, seed, k, m, scale, choice, top_p = req
    V, N, eng = pipe.mask_token_id, pipe.num_tokens, pipe.engine()
    context = None
    if ctx_row is not None:
        context = torch.zeros(S, *ctx_row.shape, device=dev())
        context[j] = ctx_row
    else:
        scale = None
    topk = V if topk is None else topk
    temps, nmask, ctemps = loop_schedule(T, temperature, N, choice)
    preds, scores = [], []
    if m is None:
        ids_ref, _ = pipe.generate_ids(context, S, T, temperature, topk, [False] * T, seed, image_base=k - j, use_graph=False, streams=1,
                                       guidance_scale=scale, choice_temperature=choice, top_p=top_p)
        ids = torch.full((S, N), V, dtype=torch.long, device=dev())
        for step in range(T):
            ids, _, pred, score = eng.sample(None, ids, context, topk, temps[step], nmask[step], seed=seed, step=step, image_base=k - j,
                                             want_img=False, want_aux=True, guidance_scale=scale,
                                             choice_temperature=ctemps[step] if ctemps else None, top_p=top_p)
            preds.append(pred[j].clone())
            scores.append(score[j].clone())
        assert torch.equal(ids, ids_ref)
        return ids_ref[j].clone(), preds, scores
    ids0 = torch.full((S, N), V, dtype=torch.long, device=dev())
    ids0[j] = start
    counts = [N] * S
    counts[j] = m
    opts = pipe._options(topk, top_p, scale, None, choice, context, S, None, None, T)
    ids_ref, _ = pipe.edit_ids(ids0, counts, context, T, temperature, opts, seed, image_base=k - j, use_graph=False)
    per_image = [edit_schedule(c, T) for c in counts]
    ids = ids0.clone()
    for step in range(T):
        _, _, pred, score = eng.sample(None, ids.clone(), context, opts.topk, temps[step], 1, seed=seed, step=step, image_base=k - j,
                                       want_img=False, want_aux=True, guidance_scale=opts.step_scale(step), top_p=opts.top_p)
        preds.append(pred[j].clone())
        scores.append(score[j].clone())
        ids = torch.where(ids == V, pred, ids)
        for b in range(S):
            if per_image[b][step] > 0:
                row = ids[b:b + 1].clone()
                ops.remask(row, score[b:b + 1].clone(), per_image[b][step], V, choice_temperature=ctemps[step] if ctemps else 0.0, seed=seed,
                           step=step, row_base=((k - j + b) * N) & (2 ** 64 - 1))
                ids[b] = row[0]
    assert torch.equal(ids, ids_ref)
    return ids_ref[j].clone(), preds, scores


def run_session(pipe, conditional, use_graph, plan, starts, filters=False):
    contexts = _contexts(pipe, len(plan)) if conditional else [None] * len(plan)
    s = pipe.decode_session(slots=S, conditional=conditional, use_graph=use_graph, record_steps=True,
                            max_context_len=contexts[0].shape[0] if conditional else None, filters=filters)
    before = pipe.engine().slots_edit_steps()
    for i, req in enumerate(plan):
        T, temperature, topk, seed, k, m, scale, choice, top_p = req
        kw = dict(context=contexts[i], guidance_scale=scale) if conditional else {}
        if filters:
            kw["top_p"] = top_p
        if m is not None:
            kw.update(ids0=starts[i], keep_given=True)
        h = s.submit(timesteps=T, temperature=temperature, topk=topk, seed=seed, image_index=k, choice_temperature=choice, **kw)
        h.params, h.start, h.ctx_row = req, starts[i], contexts[i]
    done = s.drain()
    assert s.idle() and len(done) == len(plan)
    return done, pipe.engine().slots_edit_steps() - before


def edit_ticks(handles):
    """ticks with an occupied edit request: the steps that take the form with a count per slot"""
    return sum(1 for tk in range(max(h.retired for h in handles) + 1) if any(h.edit and h.admitted <= tk <= h.retired for h in handles))


def check_contract(pipe, conditional, use_graph, plan, starts, refs, filters=False):
    done, edit_steps = run_session(pipe, conditional, use_graph, plan, starts, filters)
    handles = [f.handle for f in done]
    assert edit_steps == edit_ticks(handles), (edit_steps, edit_ticks(handles))
    vq = pipe.vqgan.engine()
    for f in done:
        h = f.handle
        assert h.retired == h.admitted + h.timesteps - 1 and len(h.trace) == h.timesteps
        key = (h.params, h.slot, conditional)
        if key not in refs:
            refs[key] = reference_run(pipe, h.slot, h.params, h.start, h.ctx_row)
        ids_ref, preds, scores = refs[key]
        for step in range(h.timesteps):
            assert torch.equal(h.trace[step][0], preds[step]), (h.params, h.slot, step, "pred")
            assert torch.equal(bits(h.trace[step][1]), bits(scores[step])), (h.params, h.slot, step, "score")
        assert torch.equal(f.ids, ids_ref), (h.params, h.slot)
        if h.edit:
            keep = h.start != pipe.mask_token_id
            assert torch.equal(f.ids[keep], h.start[keep])                           # a given id is never re-masked
            assert not bool((f.ids == pipe.mask_token_id).any())                     # no mask id is left
            assert torch.equal(f.image, vq.decode_indices(f.ids[None].contiguous())[0])      # the image: the merged ids
        else:
            assert torch.equal(f.image, vq.decode_indices(h.trace[-1][0][None].contiguous())[0])
    return done


@pytest.mark.parametrize("conditional", [True, False], ids=["text", "no-text"])
def test_session_contract_eager_captured_replayed(pipe, conditional):
    refs = {}
    starts = _starts(pipe, PLAN, seed=3)
    done = check_contract(pipe, conditional, False, PLAN, starts, refs)
    by_number = sorted(done, key=lambda f: f.handle.number)
    assert [(f.handle.slot, f.handle.admitted) for f in by_number] == SLOTS_OF_PLAN          # slots are reused mid-flight
    assert by_number[0].handle.nmask == [4, 3, 2, 1, 0, 0, 0, 0] and by_number[3].handle.nmask == [0, 0]
    assert [f.handle.edit for f in by_number] == [True, False, True, True, True, True, False]
    # the graph path: a form's first step with the flag runs eagerly, the second captures, the rest replay; a second session then
    # replays from its first step on -- and a session with OTHER masks goes through the same graphs
    for _ in range(2):
        check_contract(pipe, conditional, True, PLAN, starts, refs)
    other = check_contract(pipe, conditional, True, OTHER, _starts(pipe, OTHER, seed=4), {})
    assert not all(torch.equal(a.ids, b.ids) for a, b in zip(done, other))
    check_contract(pipe, conditional, True, PLAN, starts, refs)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_a_session_without_an_edit_request_runs_what_it_ran_before(tiny, use_graph):
    plan = [rq(4, 1.0, 5, 701, 6), rq(2, 0.7, 1, 702, 9, scale=2.0), rq(3, 1.3, 8, 703, 8, choice=2.0), rq(5, 0.9, 2, 704, 5),
            rq(1, 1.0, 3, 705, 10), rq(2, 1.0, 4, 706, 14), rq(3, 0.8, 5, 707, 15)]
    refs = {}
    for _ in range(3 if use_graph else 1):
        done, edit_steps = run_session(tiny, True, use_graph, plan, [None] * len(plan))
        assert edit_steps == 0                                                       # no step took the form with a count per slot
        for f in done:
            h = f.handle
            key = (h.params, h.slot)
            if key not in refs:
                refs[key] = reference_run(tiny, h.slot, h.params, None, h.ctx_row)
            ids_ref, preds, scores = refs[key]
            assert torch.equal(f.ids, ids_ref) and not h.edit
            for step in range(h.timesteps):
                assert torch.equal(h.trace[step][0], preds[step]) and torch.equal(bits(h.trace[step][1]), bits(scores[step]))


def test_filter_session_edit_without_topk_with_a_nucleus_beside_a_generation(tiny):
    plan = [rq(4, 1.0, None, 801, 6, m=6, top_p=0.9), rq(3, 0.8, 3, 802, 7)]
    starts = _starts(tiny, plan, seed=8)
    refs = {}
    for use_graph in (False, True, True, True):
        done = check_contract(tiny, False, use_graph, plan, starts, refs, filters=True)
    h = next(f.handle for f in done if f.handle.edit)
    assert (h.topk, h.top_p) == (tiny.mask_token_id, 0.9)
    # the filters were seen: the same edit at the default top-k without a nucleus ends elsewhere
    twin, _, _ = reference_run(tiny, 0, rq(4, 1.0, 5, 801, 6, m=6), starts[0], None)
    assert not torch.equal(twin, next(f.ids for f in done if f.handle.edit))


# ------------------------------------------------------------------------------------------------------------------------------
# image= with mask= / token_mask=
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preserve", ["tokens", "pixels"])
def test_image_requests_equal_pipeline_edit(tiny, preserve):
    pipe = tiny
    g, p, H = pipe.image_size // pipe.patch_size, pipe.patch_size, pipe.image_size
    gen = torch.Generator().manual_seed(21)
    img = (torch.rand(3, 3, H, H, generator=gen) * 2 - 1).to(dev())
    pix = torch.zeros(H, H, dtype=torch.uint8)
    pix[3:13, 9:22] = 1                                                              # a rectangle that cuts through patches
    pix[H - 1, 0] = 255                                                              # and one lit pixel in a corner patch
    tm = torch.rand(g, g, generator=gen) < 0.4
    empty = torch.zeros(g, g, dtype=torch.bool)
    cases = [dict(mask=pix), dict(token_mask=tm), dict(token_mask=empty)]
    s = pipe.decode_session(slots=S, conditional=True, use_graph=True)
    handles = [s.submit(text=f"e{i}", image=img[i], timesteps=4, topk=5, seed=40 + i, image_index=20 + i, preserve=preserve, **kw)
               for i, kw in enumerate(cases)]
    s.submit(text="g", timesteps=3, seed=50)                                         # a generation rides along
    done = {f.handle.number: f for f in s.drain()}
    for i, kw in enumerate(cases):
        want_img, want_ids = pipe.edit(img[i:i + 1], text=[f"e{i}"], timesteps=4, topk=5, seed=40 + i, image_base=20 + i, preserve=preserve,
                                       return_ids=True, **kw)
        assert handles[i].edit
        assert torch.equal(done[i].ids, want_ids[0]) and torch.equal(bits(done[i].image), bits(want_img[0])), (i, preserve)
    enc = pipe.to_latent(img)[1].reshape(3, -1)
    assert torch.equal(done[2].ids, enc[2])                                          # an empty mask: the encoded ids
    if preserve == "pixels":
        sel = (pix != 0)[None].expand(3, H, H).to(dev())
        assert torch.equal(bits(done[0].image[~sel]), bits(img[0][~sel]))            # bitwise the input outside the pixel mask
        sel_t = tm.repeat_interleave(p, 0).repeat_interleave(p, 1)[None].expand(3, H, H).to(dev())
        assert torch.equal(bits(done[1].image[~sel_t]), bits(img[1][~sel_t]))
        assert torch.equal(bits(done[2].image), bits(img[2]))


def test_step_entry_refuses_bad_counts_before_anything_runs(tiny):
    pipe = tiny
    eng = pipe.engine().clone()                                                      # a handle no slots call has touched
    N, V = pipe.num_tokens, pipe.mask_token_id
    ids = torch.full((2, N), V, dtype=torch.long, device=dev())
    start = ids.clone()

    def records(*recs):
        arr = (_lib.Slot * len(recs))()
        for i, r in enumerate(recs):
            arr[i] = _lib.Slot(*r)
        return arr
    good = (1, 0, 1.0, 3, 4, 0)
    for bad in (-2, N + 1):
        with pytest.raises(ValueError, match="slot 1"):
            eng.step_slots(ids, None, records(good, good), counts=[0, bad])
        rc = eng.lib.pmhip_pipeline_step_slots_edit(eng.handle, C.c_void_p(ids.data_ptr()), None, 0, 2, None, records(good, good), None, None,
                                                    None, 0, None, None, (C.c_int * 2)(0, bad), 0, None, None,
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == _lib.PMHIP_EINVAL and b"slot 1" in eng.lib.pmhip_last_error()
    with pytest.raises(ValueError):
        eng.step_slots(ids, None, records(good, good), counts=[0])
    torch.cuda.synchronize()
    assert torch.equal(ids, start) and eng.slots_edit_steps() == 0 and eng.slots_passes() == (0, 0, 0)              # nothing ran
    # counts of -1 everywhere: the step without counts; then one slot with a count of its own: the other keeps its record's
    eng.step_slots(ids, None, records(good, good), counts=[-1, -1])
    assert eng.slots_edit_steps() == 0 and (ids == V).sum(1).tolist() == [4, 4]
    ids.copy_(start)
    eng.step_slots(ids, None, records(good, (1, 0, 1.0, 3, 0, 0)), counts=[-1, 9])
    assert eng.slots_edit_steps() == 1 and (ids == V).sum(1).tolist() == [4, 9]
