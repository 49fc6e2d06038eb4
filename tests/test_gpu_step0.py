"""The shared step 0 of unconditional decode loops (include/pmhip.h, PMHIP_GENERATE_FROM_MASK).

``generate_ids(ids0=None)`` tells the native loop that it starts from the all-mask state; without a context its step 0 then
samples every image from the logits of ONE all-mask image, which the handle computed once.  ``generate_ids(ids0=<explicit
all-mask tensor>, streams=1)`` does not set the flag and runs the tower of every step: it is the reference of every comparison
here, and every comparison is ``torch.equal`` -- ids and every decoded image.  Every case runs in fp32-verify and in bf16."""
import contextlib

import pytest
import torch

import paintmind_amd as pm
from gpu_common import dev
from paintmind_amd import ops
from paintmind_amd.config import ver2cfg
from paintmind_amd.generate import Pipeline
from util import load_golden, to_torch_sd

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(torch.float32, id="fp32"), pytest.param(torch.bfloat16, id="bf16")]


def make_tiny():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False)
    pipe.load_state_dict(to_torch_sd(p), strict=False)
    return pipe.to(dev()).eval()


@pytest.fixture(scope="module")
def tiny():
    return make_tiny()


@pytest.fixture(scope="module")
def pipe512():
    torch.manual_seed(0)
    return Pipeline(pm.Config(ver2cfg["bench-uncond-12L-d512"]), stage1_pretrained=False).to(dev()).eval()


@contextlib.contextmanager
def fresh(pipe, dtype):
    """the pipeline in `dtype` with NEW native handles (no shared logits, no graphs, counters at zero)"""
    pipe.set_compute_dtype(dtype)
    pipe.invalidate_engines()
    try:
        yield pipe
    finally:
        pipe.set_compute_dtype(torch.float32)
        pipe.invalidate_engines()
        torch.cuda.empty_cache()


def all_mask(pipe, B):
    return torch.full((B, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long, device=dev())


def full(pipe, B, T, topk, flags, seed, context=None, **kw):
    """the unflagged loop: explicit all-mask start ids, one stream, eager -- the tower of every step runs"""
    return pipe.generate_ids(context, B, T, 1.0, topk, flags, seed=seed, streams=1, use_graph=False, ids0=all_mask(pipe, B), **kw)


def shared(pipe, B, T, topk, flags, seed, context=None, **kw):
    return pipe.generate_ids(context, B, T, 1.0, topk, flags, seed=seed, **kw)


def same(a, b):
    if not torch.equal(a[0], b[0]):
        return False
    if a[1] is None or b[1] is None:
        return a[1] is None and b[1] is None
    return a[1].shape == b[1].shape and torch.equal(a[1], b[1])


def check_all_paths(pipe, B, T, topk, flags, seed, lanes=(1,), replays=3, **kw):
    """flagged loop == unflagged loop: eager, then the graph path's eager warm pass, its capture and `replays` replays"""
    ref = full(pipe, B, T, topk, flags, seed, **kw)
    assert int((ref[0] == pipe.mask_token_id).sum()) == B                 # the loop ran: one re-masked token per image is left
    for streams in lanes:
        assert same(shared(pipe, B, T, topk, flags, seed, streams=streams, use_graph=False, **kw), ref), ("eager", streams)
        for rep in range(2 + replays):
            assert same(shared(pipe, B, T, topk, flags, seed, streams=streams, use_graph=True, **kw), ref), ("graph", streams, rep)
    return ref


# ---- the premise ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_premise_all_mask_rows_are_the_same_for_every_image(pipe512, tiny, dtype):
    """on the FULL path the logits of an all-mask batch repeat image 0's rows bit for bit: B = 33 and 31 (the bench's lanes), 3"""
    for pipe, sizes in ((pipe512, (33, 31, 3)), (tiny, (33, 31, 3))):
        with fresh(pipe, dtype):
            first = None
            for B in sizes:
                logits = pipe.tokens2logits(pipe.ids2tokens(all_mask(pipe, B)), None)
                assert torch.isfinite(logits).all()
                assert torch.equal(logits, logits[:1].expand_as(logits)), B
                first = logits[:1].clone() if first is None else first
                assert torch.equal(logits[:1], first), B                     # ... and the same at every batch size
                del logits


# ---- equivalence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_pipeline_equivalence(tiny, dtype):
    with fresh(tiny, dtype) as pipe:
        a = check_all_paths(pipe, 3, 4, 3, [True, False, True, True], seed=1)
        b = check_all_paths(pipe, 3, 4, 3, [True, False, True, True], seed=2)                       # a second seed
        assert not torch.equal(a[0], b[0])
        c = check_all_paths(pipe, 3, 4, 3, [True, False, True, True], seed=1, image_base=7)         # a non-zero image_base
        assert not torch.equal(a[0], c[0])
        check_all_paths(pipe, 5, 5, 2, [False, True, False, False, True], seed=3)                   # decode flags with gaps
        check_all_paths(pipe, 4, 3, 2, [False, False, False], seed=3)                               # no decode at all
        check_all_paths(pipe, 3, 3, 16, [True, True, True], seed=4)                                 # top-k 16: the row kernel
        check_all_paths(pipe, 3, 1, 3, [True], seed=5)                                              # T = 1
        check_all_paths(pipe, 9, 4, 3, [True] * 4, seed=6, lanes=(2, 3))                            # lanes: one handle each
        # the native call writes the all-mask state itself: what `ids` holds on entry is ignored
        eng, vq = pipe.engine(), pipe.vqgan.engine()
        temps, nmask = pipe._schedule(4, 1.0)
        junk = torch.randint(0, pipe.mask_token_id, (3, pipe.num_tokens), device=dev())
        for graph in (False, True, True, True):
            ids, imgs = eng.generate(vq, junk.clone(), None, temps, nmask, [True, False, True, True], 3, seed=1, use_graph=graph,
                                     from_mask=True)
            assert same((ids, imgs), a), graph


@pytest.mark.parametrize("dtype", DTYPES)
def test_bench_configuration_equivalence(pipe512, dtype):
    """vit-s + 12L/d512, B = 64, T = 8, top-k 5, every step decoded: eager, graph capture and three replays, one and two lanes"""
    with fresh(pipe512, dtype) as pipe:
        check_all_paths(pipe, 64, 8, 5, [True] * 8, seed=1000, lanes=(1, 2), replays=3)
        for e, _, _ in pipe._lanes(2):                                       # the primary handle and the second lane's clone
            fills, hits = e.step0_shared()
            assert fills == 1 and hits >= 5, (fills, hits)


@pytest.mark.parametrize("dtype", DTYPES)
def test_full_size_variants(pipe512, dtype):
    with fresh(pipe512, dtype) as pipe:
        a = check_all_paths(pipe, 5, 4, 5, [True, False, False, True], seed=1, replays=1)            # decode flags with gaps
        b = check_all_paths(pipe, 5, 4, 5, [True, False, False, True], seed=2, replays=1)            # a second seed
        c = check_all_paths(pipe, 5, 4, 5, [True, False, False, True], seed=1, image_base=64, replays=1)
        assert not torch.equal(a[0], b[0]) and not torch.equal(a[0], c[0])
        check_all_paths(pipe, 4, 3, 16, [False, False, True], seed=3, replays=1)                     # top-k 16: the row kernel
        check_all_paths(pipe, 6, 1, 5, [True], seed=4, replays=1)                                    # T = 1
        assert pipe.engine().step0_shared()[0] == 1


# ---- the cache across batch sizes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["tiny", "d512"])
def test_cache_filled_at_one_batch_size_serves_another(request, which, dtype):
    pipe = request.getfixturevalue("tiny" if which == "tiny" else "pipe512")
    with fresh(pipe, dtype):
        flags = [True, False, True, True]
        assert same(shared(pipe, 3, 4, 5, flags, seed=8, streams=1), full(pipe, 3, 4, 5, flags, seed=8))
        assert pipe.engine().step0_shared() == (1, 0)
        ref = full(pipe, 16, 4, 5, flags, seed=9)
        for graph in (False, True, True, True):
            assert same(shared(pipe, 16, 4, 5, flags, seed=9, streams=1, use_graph=graph), ref), graph
        assert pipe.engine().step0_shared() == (1, 4)


# ---- invalidation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_and_mask_token_edits_invalidate_the_cache(dtype):
    pipe = make_tiny()
    pipe.set_compute_dtype(dtype)
    flags = [True, True, True]
    g = torch.Generator().manual_seed(5)
    old = shared(pipe, 4, 3, 3, flags, seed=2, streams=1)
    assert same(old, full(pipe, 4, 3, 3, flags, seed=2)) and pipe.engine().step0_shared() == (1, 0)
    handle = pipe.engine()
    edits = [(pipe.transformer.layers[0].attn1.to_out[0].weight, 0.3), (pipe.mask_token, 1.0)]
    for param, scale in edits:
        with torch.no_grad():
            param.add_(scale * torch.randn(param.shape, generator=g).to(dev()))                     # in place: bumps _version
        assert pipe.engine() is not handle                                                          # a new handle, an empty cache
        handle = pipe.engine()
        assert handle.step0_shared() == (0, 0)
        new = shared(pipe, 4, 3, 3, flags, seed=2, streams=1)
        assert handle.step0_shared() == (1, 0)
        again = shared(pipe, 4, 3, 3, flags, seed=2, streams=1, use_graph=True)
        assert same(new, full(pipe, 4, 3, 3, flags, seed=2)) and same(again, new)
        assert not torch.equal(new[1], old[1]), "the edit did not reach the step-0 logits"
        old = new


# ---- counters ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_counters_show_when_the_shortcut_ran(tiny, dtype):
    with fresh(tiny, dtype) as pipe:
        eng = pipe.engine()
        flags = [True, False, True]
        assert eng.step0_shared() == (0, 0)
        ref = full(pipe, 3, 3, 3, flags, seed=1)
        assert eng.step0_shared() == (0, 0)                                  # the unflagged loop never touches the cache
        # per-kernel timing on: the tower of EVERY step runs, nothing is counted, same result
        ops.timing_reset()
        ops.timing_enable(True)
        try:
            timed = shared(pipe, 3, 3, 3, flags, seed=1, streams=1, use_graph=True)
            torch.cuda.synchronize()
        finally:
            ops.timing_enable(False)
        launches_timed = ops.timing_get("attention")[0]
        assert same(timed, ref) and eng.step0_shared() == (0, 0)
        # with a context, and with guidance: the flag only fills the ids
        ctx = pipe.text_model(["a", "b", "c"]).to(dev())
        for graph in (False, True, True):
            for scale in (None, 1.5):
                got = shared(pipe, 3, 3, 3, flags, seed=1, context=ctx, streams=1, use_graph=graph, guidance_scale=scale)
                assert same(got, full(pipe, 3, 3, 3, flags, seed=1, context=ctx, guidance_scale=scale)), (graph, scale)
        assert eng.step0_shared() == (0, 0)
        # the shortcut: one fill, then one hit per loop, eager or graph (warm pass, capture, replays)
        assert same(shared(pipe, 3, 3, 3, flags, seed=1, streams=1), ref) and eng.step0_shared() == (1, 0)
        assert same(shared(pipe, 3, 3, 3, flags, seed=1, streams=1), ref) and eng.step0_shared() == (1, 1)
        for rep in range(4):
            assert same(shared(pipe, 3, 3, 3, flags, seed=1, streams=1, use_graph=True), ref)
            assert eng.step0_shared() == (1, 2 + rep)
        assert pipe.engine() is eng
        # the timed flagged loop above launched exactly what the unflagged loop launches
        ops.timing_reset()
        ops.timing_enable(True)
        try:
            full(pipe, 3, 3, 3, flags, seed=1)
            torch.cuda.synchronize()
        finally:
            ops.timing_enable(False)
        assert launches_timed == ops.timing_get("attention")[0] > 0
        assert eng.step0_shared() == (1, 5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_effect_with_a_context(tiny, dtype):
    """text-conditional loops: flagged == unflagged on every path, lanes included"""
    with fresh(tiny, dtype) as pipe:
        ctx = pipe.text_model(["a", "b", "c", "d", "e", "f", "g", "h", "i"]).to(dev())
        ref = full(pipe, 9, 4, 3, [True] * 4, seed=3, context=ctx)
        for streams in (1, 2):
            for graph in (False, True, True, True):
                assert same(shared(pipe, 9, 4, 3, [True] * 4, seed=3, context=ctx, streams=streams, use_graph=graph), ref)
        assert all(e.step0_shared() == (0, 0) for e, _, _ in pipe._lanes(2))
