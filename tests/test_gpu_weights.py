"""Prompt weights at the model level (the *_weights entries of include/pmhip.h) on the tiny pipeline, B = 3:
weights alone (beside per-image lengths) and beside two regions, drawn from {0, 1/8, 1, 8, 1.3, 0.5} with NaN in the context rows
that may reach nothing.  ``tokens2logits`` and one ``sample`` step against the plain-torch branch of the same model; the native loop,
eager and captured, against the per-step composition; weights of 1 against the call without them, bit for bit; guidance and a
negative prompt against the operator composition; two sets of weights through one captured graph; the engine's own messages."""
import ctypes as C

import numpy as np
import pytest
import torch

import paintmind_amd as pm
import region_ref as R
from gpu_common import dev
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline
from util import load_golden, to_torch_sd

pytestmark = pytest.mark.gpu

TOL = 1e-3                      # the project's float bar (tests/test_gpu_context_lens.py)
B, T, TOPK, TEMP, SEED = 3, 3, 4, 1.0, 77
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
FORMS = pytest.mark.parametrize("form", ["alone", "regions"])


def _tiny():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False)
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("text_model") for k in missing.missing_keys)
    return pipe.eval()


@pytest.fixture(scope="module")
def cpu_pipe():
    return _tiny()


@pytest.fixture(scope="module")
def tiny_pipe():
    return _tiny().to(dev())


def _weights(ks, seed):
    rng = np.random.default_rng(seed)
    w = rng.choice(np.array([0, 0.125, 1, 8, 1.3, 0.5], np.float32), size=ks.shape).astype(np.float32)
    for b in range(ks.shape[0]):                                      # every segment keeps a row that counts
        for sg in np.unique(ks[b][ks[b] < 32]):
            w[b, np.flatnonzero(ks[b] == sg)[0]] = (8, 0.125, 1.3)[int(sg) % 3]
    return w


def _case(pipe, form, seed=1):
    """-> dict(ctx with NaN where a row may reach nothing, finite: the same with zeros there, w, kw: the keywords that carry the
    layout -- context_lens alone, or the two segment arrays of two regions --, ks / qm: the layout as arrays either way)"""
    rows = pipe.text_model(["a", "b", "c", "d", "e", "f"]).cpu()
    if form == "alone":
        lens = [77, 50, 33]
        context = rows[:B].clone()
        ks = np.where(np.arange(77)[None, :] < np.asarray(lens)[:, None], 0, R.PAD).astype(np.uint8)
        qm = np.full((B, pipe.num_tokens), 0xFFFFFFFF, np.uint32)
        kw = dict(context_lens=lens)
    else:
        S, g = pipe.image_size, pipe.image_size // pipe.patch_size
        left = torch.zeros(S, S)
        left[:, :S // 2] = 1
        tm = torch.zeros(g, g, dtype=torch.bool)
        tm[1:3, 1:3] = True
        regions = [[(rows[3, :40], left), (rows[4, :9], tm)], [(rows[5, :25], tm)], []]
        context, ks, qm = R.layout([rows[b] for b in range(B)], regions, pipe.image_size, pipe.patch_size)
        kw = dict(context_segments=ks, token_segments=qm)
    w = _weights(ks, seed)
    dead = torch.from_numpy((ks == R.PAD) | (w == 0))
    ctx = context.clone()
    ctx[dead] = float("nan")
    finite = context.clone()
    finite[dead] = 0.0
    return dict(ctx=ctx, finite=finite, w=w, kw=kw, ks=ks, qm=qm)


@pytest.fixture(scope="module")
def data(tiny_pipe):
    pipe = tiny_pipe
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, pipe.mask_token_id, (B, pipe.num_tokens), generator=g)
    ids[torch.rand(B, pipe.num_tokens, generator=g) < 0.5] = pipe.mask_token_id
    out = dict(ids=ids.to(dev()), alone=_case(pipe, "alone"), regions=_case(pipe, "regions"))
    out["tok"] = pipe.ids2tokens(out["ids"])
    out["neg"] = pipe.text_model(["n0", "n1", "n2"])[:, :33].contiguous().to(dev())
    out["noise"] = torch.rand(B, pipe.num_tokens, pipe.mask_token_id, generator=g)
    return out


class in_dtype:
    def __init__(self, pipe, dtype):
        self.pipe, self.dtype = pipe, dtype

    def __enter__(self):
        self.pipe.set_compute_dtype(self.dtype)

    def __exit__(self, *exc):
        self.pipe.set_compute_dtype(torch.float32)


@FORMS
@DTYPES
def test_logits_and_one_step_against_the_cpu_branch_of_the_same_model(tiny_pipe, cpu_pipe, data, form, dtype):
    """fp32-verify is gated at the project's float bar, logits and the step's decoded image (from the predictions at all positions, with
    given noise); the bf16 figures are printed, not gated.  Counter-check: the same (finite)
    context WITHOUT the weights is beyond the bar, so this cannot pass with the weights ignored."""
    c = data[form]                                                    # (ratio 0.2: 3 positions re-masked, fewer than any image has masked)
    with torch.no_grad():
        want = cpu_pipe.tokens2logits(data["tok"].cpu(), c["ctx"], context_weights=c["w"], **c["kw"])
        ids_cpu, img_cpu = cpu_pipe.sample(data["ids"].cpu(), 0.2, text=c["ctx"], topk=TOPK, temperature=0.8, noise=data["noise"],
                                           context_weights=c["w"], **c["kw"])
    with in_dtype(tiny_pipe, dtype):
        got = tiny_pipe.tokens2logits(data["tok"], c["ctx"].to(dev()), context_weights=c["w"], **c["kw"]).cpu()
        loose = tiny_pipe.tokens2logits(data["tok"], c["finite"].to(dev()), **c["kw"]).cpu()
        ids_gpu, img_gpu = tiny_pipe.sample(data["ids"], 0.2, text=c["ctx"].to(dev()), topk=TOPK, temperature=0.8, noise=data["noise"].to(dev()),
                                            context_weights=c["w"], **c["kw"])
    assert torch.isfinite(got).all() and torch.isfinite(img_gpu).all()
    err, gap = float((got - want).abs().max()), float((loose - want).abs().max())
    same = float((ids_gpu.cpu() == ids_cpu).float().mean())
    img_err = float((img_gpu.cpu() - img_cpu).abs().max())
    print(f"{form} {dtype}: max |logits GPU - logits CPU branch| under weights = {err:.3e}; without the weights {gap:.3e}; one step: "
          f"{same:.3f} of the ids equal, max |img GPU - img CPU| = {img_err:.3e}")
    if dtype == torch.float32:                                        # (the ids are printed, not gated: the re-masking SORTS confidences,
        assert err < TOL and img_err < TOL                            # where a difference far below the bar can swap two neighbours)
    assert gap > TOL


def _steps(pipe, ctx, c, w, **kw):
    """the loop step by step through the one-step entry with the same arrays -> final ids"""
    eng = pipe.engine()
    temps, nmask = pipe._schedule(T, TEMP)
    ids = torch.full((B, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long, device=dev())
    for step in range(T):
        ids, _, _, _ = eng.sample(None, ids, ctx, TOPK, temps[step], nmask[step], seed=SEED, step=step, want_img=False,
                                  context_weights=w, **c["kw"], **kw)
    return ids


def _loop(pipe, ctx, c, w, **kw):
    kw = {**dict(use_graph=False, streams=1), **c["kw"], **kw}
    return pipe.generate_ids(ctx, B, T, TEMP, TOPK, [False] * (T - 1) + [True], SEED, context_weights=w, **kw)


@FORMS
@DTYPES
def test_the_native_loop_is_the_per_step_composition_and_two_lanes_agree(tiny_pipe, data, form, dtype):
    pipe, c = tiny_pipe, data[form]
    ctx = c["ctx"].to(dev())
    with in_dtype(pipe, dtype):
        want = _steps(pipe, ctx, c, c["w"])
        for use_graph in (False, True, True):                         # first call eager, second captures, third replays
            ids, imgs = _loop(pipe, ctx, c, c["w"], use_graph=use_graph)
            assert torch.isfinite(imgs).all() and torch.equal(ids, want), use_graph
        lanes = _loop(pipe, ctx, c, c["w"], streams=2)
        assert torch.equal(lanes[0], ids) and torch.equal(lanes[1], imgs)
        plain, _ = pipe.generate_ids(c["finite"].to(dev()), B, T, TEMP, TOPK, [False] * T, SEED, use_graph=False, streams=1, **c["kw"])
        assert not torch.equal(plain, want)                            # and the weights matter


@FORMS
@DTYPES
def test_weights_of_one_are_the_call_without_them(tiny_pipe, data, form, dtype):
    """bit for bit: beside regions that call is the segmented call, otherwise the call with the neutral segments (segment 0 below an
    image's length, 255 behind, every token allowing everything) -- which is also what the engine stages on its own when it gets
    weights without segment arrays"""
    pipe, c = tiny_pipe, data[form]
    ctx, ones = c["finite"].to(dev()), np.ones_like(c["w"])
    seg_kw = dict(context_segments=c["ks"], token_segments=c["qm"])
    with in_dtype(pipe, dtype):
        eng = pipe.engine()
        a = pipe.tokens2logits(data["tok"], ctx, context_weights=ones, **c["kw"])
        b = pipe.tokens2logits(data["tok"], ctx, **seg_kw)
        assert torch.equal(a, b)
        ids_a, imgs_a = _loop(pipe, ctx, c, ones)
        ids_b, imgs_b = pipe.generate_ids(ctx, B, T, TEMP, TOPK, [False] * (T - 1) + [True], SEED, use_graph=False, streams=1, **seg_kw)
        assert torch.equal(ids_a, ids_b) and torch.equal(imgs_a, imgs_b)
        if form == "alone":
            # the engine's neutral staging: weights beside NULL segment arrays (and beside ctx_lens_host where the entry has it)
            w = c["w"]
            want = pipe.tokens2logits(data["tok"], ctx, context_weights=w, **seg_kw)
            live = np.where(c["ks"] == R.PAD, 0, w).astype(np.float32)                 # the forward entry has no lengths: weight 0 instead
            assert torch.equal(eng.forward(data["tok"], ctx, context_weights=live), want)
            ids0 = torch.full((B, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long, device=dev())
            one = lambda **kw: eng.sample(None, ids0.clone(), ctx, TOPK, 1.0, 8, seed=SEED, want_img=False, context_weights=w, **kw)[0]
            assert torch.equal(one(context_lens=c["kw"]["context_lens"]), one(**seg_kw))


@DTYPES
def test_guidance_and_a_negative_prompt_compose(tiny_pipe, data, dtype):
    """ids of the native guided step == the operator composition: the forward under weights, the forward of the negative context
    WITHOUT them, the combine, the draw and the re-masking"""
    pipe, c = tiny_pipe, data["regions"]
    ctx, N = c["ctx"].to(dev()), pipe.num_tokens
    with in_dtype(pipe, dtype):
        eng = pipe.engine()
        for neg in (None, data["neg"]):
            ids = data["ids"].clone()
            got, _, _, _ = eng.sample(None, ids.clone(), ctx, TOPK, 0.9, 5, seed=SEED, step=1, want_img=False, guidance_scale=3.0,
                                      negative_context=neg, context_weights=c["w"], **c["kw"])
            cond = eng.forward(data["tok"], ctx, context_weights=c["w"], **c["kw"])
            uncond = eng.forward(data["tok"], neg)
            logits = ops.guidance_combine(cond, uncond, 3.0, out=cond)
            _, merged, score = ops.sample_rows(logits.reshape(B * N, -1), ids.reshape(-1), pipe.mask_token_id, TOPK, 0.9, seed=SEED, step=1)
            want = ops.remask(merged.reshape(B, N), score.reshape(B, N), 5, pipe.mask_token_id)
            assert torch.equal(got, want), neg is None
            plain, _, _, _ = eng.sample(None, ids.clone(), c["finite"].to(dev()), TOPK, 0.9, 5, seed=SEED, step=1, want_img=False,
                                        guidance_scale=3.0, negative_context=neg, **c["kw"])
            assert not torch.equal(plain, got)


@FORMS
@DTYPES
def test_a_second_set_of_weights_adds_no_graph(tiny_pipe, data, form, dtype):
    pipe, c = tiny_pipe, data[form]
    ctx = c["ctx"].to(dev())
    w2 = np.where(c["w"] == 0, 0, np.roll(np.where(c["w"] == 0, 1, c["w"]), 1, axis=1) * 0.5 + 0.25).astype(np.float32)
    with in_dtype(pipe, dtype):
        eng = pipe.engine()
        want1, want2 = _loop(pipe, ctx, c, c["w"]), _loop(pipe, ctx, c, w2)
        assert not torch.equal(want1[0], want2[0])
        for _ in range(2):                                            # eager under the key, then captured
            got = _loop(pipe, ctx, c, c["w"], use_graph=True)
        assert torch.equal(got[0], want1[0]) and torch.equal(got[1], want1[1])
        entries, captured = eng.graph_count()
        assert captured >= 1
        got = _loop(pipe, ctx, c, w2, use_graph=True)                 # a replay with weights the capture never saw
        assert torch.equal(got[0], want2[0]) and torch.equal(got[1], want2[1])
        assert eng.graph_count() == (entries, captured)
        # the loop without weights at the same (B, L) has a key of its own: ONE further key for the weighted form
        pipe.generate_ids(c["finite"].to(dev()), B, T, TEMP, TOPK, [False] * (T - 1) + [True], SEED, use_graph=True, streams=1, **c["kw"])
        assert eng.graph_count()[0] == entries + 1


def test_the_engine_validates_before_it_launches(tiny_pipe, data):
    pipe, c = tiny_pipe, data["regions"]
    eng = pipe.engine()
    ctx = c["finite"].to(dev()).contiguous()
    L = ctx.shape[1]
    logits = torch.empty(B, pipe.num_tokens, eng.n_embed, device=dev())
    f32p, u8p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_ubyte), C.POINTER(C.c_uint32)

    def forward(w, ks=c["ks"], qm=c["qm"], context=ctx):
        w = np.ascontiguousarray(w, np.float32)
        return eng.lib.pmhip_s2_forward_weights(eng.handle, data["tok"].data_ptr(), None if context is None else context.data_ptr(),
                                                L if context is not None else 0, B,
                                                None if ks is None else np.ascontiguousarray(ks).ctypes.data_as(u8p),
                                                None if qm is None else np.ascontiguousarray(qm).ctypes.data_as(u32p),
                                                w.ctypes.data_as(f32p), logits.data_ptr(), None)

    assert forward(c["w"]) == _lib.PMHIP_OK
    for bad in (-1.0, float("nan"), float("inf"), 2.0 ** -21, 2.0 ** 21):
        w = c["w"].copy()
        w[1, 7] = bad
        assert forward(w) == _lib.PMHIP_EINVAL
        msg = eng.lib.pmhip_last_error()
        assert b"s2_forward_weights: image 1: context row 7: weight" in msg and b"[2^-20, 2^20]" in msg, msg
    w = c["w"].copy()
    w[2, c["ks"][2] == 0] = 0                                         # image 2 has the global prompt only
    assert forward(w) == _lib.PMHIP_EINVAL and b"image 2: token 0 allows no context row with a weight above 0" in eng.lib.pmhip_last_error()
    w = c["w"].copy()
    w[0, c["ks"][0] == 2] = 0                                         # region 2 of image 0 silenced: its tokens still see the global prompt
    assert forward(w) == _lib.PMHIP_OK
    assert forward(c["w"], ks=None, qm=None, context=None) == _lib.PMHIP_EINVAL
    assert b"weights given without a context" in eng.lib.pmhip_last_error()
    assert forward(c["w"], qm=None) == _lib.PMHIP_EINVAL and b"come together" in eng.lib.pmhip_last_error()
    assert forward(np.ones((B, L), np.float32), ks=None, qm=None) == _lib.PMHIP_OK          # weights alone: neutral segments
    # weights beside explicit segments and lengths stay refused, as for segments; and the Python layer says so first
    with pytest.raises(ValueError, match="exclude each other"):
        pipe.tokens2logits(data["tok"], ctx, context_lens=[L] * B, context_weights=c["w"], **c["kw"])
    lens = (C.c_int * B)(*[L] * B)
    ids = torch.full((B, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long, device=dev())
    rc = eng.lib.pmhip_pipeline_sample_weights(eng.handle, None, ids.data_ptr(), ctx.data_ptr(), L, B, lens, TOPK, 1.0, 4, None, 1, 0, 0, None, None,
                                               None, 0, 0.0, 0.0, None, 1.0, None, 0, None, np.ascontiguousarray(c["ks"]).ctypes.data_as(u8p),
                                               np.ascontiguousarray(c["qm"]).ctypes.data_as(u32p),
                                               np.ascontiguousarray(c["w"]).ctypes.data_as(f32p), None)
    assert rc == _lib.PMHIP_EINVAL and b"exclude each other" in eng.lib.pmhip_last_error()
    assert torch.equal(ids, torch.full_like(ids, pipe.mask_token_id))                        # nothing was launched
