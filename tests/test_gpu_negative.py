"""Negative prompts and the per-step guidance schedule on the MI355X: the device-scale combine against the scalar entry bit for
bit, the native step against the operator composition and against the oracle, the native loop (eager, captured, replayed, two
lanes) against the stepwise chain, handle state after a call with a negative context, and refusals on a real handle."""
import ctypes as C

import numpy as np
import pytest
import torch

import paintmind_amd as pm
from abi_frames import bits, call, framed
from gpu_common import dev, n, t
from negative_ref import PromptRows, composed_step, oracle_negative_step
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline, linear_guidance, mask_schedule
from paintmind_amd.ops import _p, stream_ptr
from util import load_golden, maxabs, to_torch_sd

pytestmark = pytest.mark.gpu
TOL = 1e-3                                   # the suite's float bar (tests/test_gpu_model.py)
f32 = torch.float32
L, LN = 7, 3


@pytest.fixture(scope="module")
def tiny():
    p, d = load_golden("tiny_pipeline.npz")
    cfg = pm.Config(pm.ver2cfg["tiny-pipeline"])
    pipe = Pipeline(cfg, stage1_pretrained=False, text_model=PromptRows(cfg.context_dim, L, LN))
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("text_model") for k in missing.missing_keys)
    return pipe.to(dev()).eval(), p, d


# ---------------------------------------------------------------------------------------------------------------------------------
# the operator: pmhip_guidance_combine_dev == pmhip_guidance_combine / _stats, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
GRID_CAP_FLOATS = 256 * 8 * 256 * 4          # rowops.hip grid_for: 256 * 8 workgroups of 256 float4s, the rest by the grid-stride loop


@pytest.mark.parametrize("size", [64, 64 * 5, GRID_CAP_FLOATS + 64 * 5], ids=["one-block", "partial-wave", "second-trip"])
def test_device_scale_combine_equals_the_scalar_entry(size):
    rows = size // 64
    g = torch.Generator().manual_seed(size)
    cond, unc = (2 * torch.randn(rows, 64, generator=g)).to(dev()), (2 * torch.randn(rows, 64, generator=g)).to(dev())
    for scale in (0.0, 1.0, 2.5, -1.0):
        want, want_stats = ops.guidance_combine(cond, unc, scale, with_stats=True)
        assert torch.equal(bits(want), bits(ops.guidance_combine(cond, unc, scale)))
        sd = torch.tensor([scale], dtype=f32, device=dev())
        for stats in (False, True):
            for place in ("out", "cond", "uncond"):
                fc = framed(rows, 64, ld=64, payload=cond, fill="sentinel" if place == "cond" else "nan")
                fu = framed(rows, 64, ld=64, payload=unc, fill="sentinel" if place == "uncond" else "nan")
                fo = {"out": framed(rows, 64, ld=64, device=dev()), "cond": fc, "uncond": fu}[place]
                fs = framed(rows, 2, ld=2, device=dev()) if stats else None
                call("pmhip_guidance_combine_dev", fc, fu, sd, fo, size, fs)
                what = f"n={size} scale={scale} stats={stats} out={place}"
                assert torch.equal(bits(fo.payload()), bits(want)), what
                for fr in (fc, fu, fo) + ((fs,) if stats else ()):
                    fr.assert_frame_untouched(what)
                if stats:
                    assert torch.equal(bits(fs.payload()), bits(want_stats.reshape(rows, 2))), what
                if place != "cond":
                    assert torch.equal(bits(fc.payload()), bits(cond)), what
                if place != "uncond":
                    assert torch.equal(bits(fu.payload()), bits(unc)), what
        # the Python operator: the same call
        got, got_stats = ops.guidance_combine_dev(cond, unc, sd, with_stats=True)
        assert torch.equal(bits(got), bits(want)) and torch.equal(bits(got_stats), bits(want_stats))
        assert torch.equal(bits(ops.guidance_combine_dev(cond.clone(), unc, sd)), bits(want))


# ---------------------------------------------------------------------------------------------------------------------------------
# the native step
# ---------------------------------------------------------------------------------------------------------------------------------
def _step_case(pipe):
    """B = 3, a context of 7 rows (lengths 7, 2, 5), a negative context of 3 rows with lengths (1, 3, 2) and NaN behind each"""
    B, N, V, D = 3, pipe.num_tokens, pipe.mask_token_id, pipe.text_model.context_dim
    g = torch.Generator().manual_seed(21)
    ids = torch.randint(0, V, (B, N), generator=g)
    ids[torch.rand(B, N, generator=g) < 0.6] = V
    ctx, neg = torch.randn(B, L, D, generator=g), torch.randn(B, LN, D, generator=g)
    neg_lens = [1, 3, 2]
    for b, k in enumerate(neg_lens):
        neg[b, k:] = float("nan")
    return dict(B=B, ids=ids.to(dev()), ctx=ctx.to(dev()), ctx_lens=[7, 2, 5], neg=neg.to(dev()), neg_lens=neg_lens,
                noise=torch.rand(B, N, V, generator=g).to(dev()))


def test_native_step_equals_the_operator_composition(tiny):
    pipe, _, _ = tiny
    c = _step_case(pipe)
    try:
        for dtype in (torch.float32, torch.bfloat16):
            pipe.set_compute_dtype(dtype)
            for scale, noise, step in ((2.5, None, 2), (-1.0, c["noise"], 0), (0.0, None, 1)):
                kw = dict(text=c["ctx"], topk=4, temperature=0.8, noise=noise, seed=13, step=step, image_base=5, guidance_scale=scale,
                          context_lens=c["ctx_lens"])
                ids, img = pipe.sample(c["ids"], 0.5, negative_text=c["neg"], negative_context_lens=c["neg_lens"], **kw)
                want, want_img = composed_step(pipe, c["ids"], 8, c["ctx"], c["ctx_lens"], c["neg"], c["neg_lens"], 4, 0.8, noise, 13, step, 5, scale)
                assert torch.equal(ids, want) and torch.equal(img, want_img), (dtype, scale)
                assert bool(torch.isfinite(img).all()), (dtype, scale)               # the NaN behind the negative lengths never appears
                if scale == 2.5:                                                      # the negative context is seen: not the plain guided step
                    plain = pipe.engine().sample(None, c["ids"].clone(), c["ctx"], 4, 0.8, 8, noise=noise, seed=13, step=step, image_base=5,
                                                 want_img=False, want_aux=True, guidance_scale=scale, context_lens=c["ctx_lens"])
                    mine = pipe.engine().sample(None, c["ids"].clone(), c["ctx"], 4, 0.8, 8, noise=noise, seed=13, step=step, image_base=5,
                                                want_img=False, want_aux=True, guidance_scale=scale, context_lens=c["ctx_lens"],
                                                negative_context=c["neg"], negative_lens=c["neg_lens"])
                    assert not torch.equal(plain[3], mine[3]), dtype
            # the context as its own negative: cond - neg is exactly 0, the UNGUIDED step for any scale
            kw = dict(text=c["ctx"], topk=4, temperature=0.8, seed=13, step=1, context_lens=c["ctx_lens"])
            want, want_img = pipe.sample(c["ids"], 0.5, **kw)
            for scale in (0.0, 3.0, -2.0):
                ids, img = pipe.sample(c["ids"], 0.5, guidance_scale=scale, negative_text=c["ctx"], negative_context_lens=c["ctx_lens"], **kw)
                assert torch.equal(ids, want) and torch.equal(img, want_img), (dtype, scale)
    finally:
        pipe.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("scale", [1.0, 2.5])
def test_native_step_against_the_oracle(tiny, scale):
    """fp32, the golden's captured noise, full lengths: ids equal the numpy composition of the oracle's transformer run twice and
    its existing tail, the image within the suite's bar"""
    pipe, p, d = tiny
    vcfg, scfg = pm.ver2cfg["tiny-vqgan"], pm.ver2cfg["tiny-pipeline"]
    neg = np.random.default_rng(5).standard_normal((d["ids0"].shape[0], LN, d["context"].shape[2])).astype(np.float32)
    ids, img = pipe.sample(t(d["ids0"]), np.float64(0.5), text=t(d["context"]), topk=5, temperature=0.7, noise=t(d["s5_ctx_noise"]),
                           guidance_scale=scale, negative_text=t(neg))
    ids_o, img_o = oracle_negative_step(d["ids0"], np.float64(0.5), d["context"], neg, 5, 0.7, d["s5_ctx_noise"], p, vcfg, scfg, scale)
    assert np.array_equal(n(ids), ids_o)
    assert maxabs(n(img), img_o) < TOL


# ---------------------------------------------------------------------------------------------------------------------------------
# the native loop
# ---------------------------------------------------------------------------------------------------------------------------------
def _chain(pipe, ctx, ctx_lens, neg, neg_lens, T, topk, seed, scales):
    ids = torch.full((ctx.shape[0], pipe.num_tokens), pipe.mask_token_id, dtype=torch.long, device=dev())
    imgs = []
    for step in range(T):
        ids, img = pipe.sample(ids, mask_schedule((step + 1) / T), text=ctx, topk=topk, temperature=1.0 * (1 - step / T), seed=seed, step=step,
                               guidance_scale=scales[step], context_lens=ctx_lens, negative_text=neg, negative_context_lens=neg_lens)
        imgs.append(img.cpu())
    return ids.cpu(), imgs


def test_native_loop_equals_the_stepwise_chain_and_one_graph_serves_every_schedule(tiny):
    pipe, _, _ = tiny
    B, T, topk, seed = 9, 5, 4, 77
    texts, negs = [f"t{i}" for i in range(B)], [f"not n{i}" for i in range(B)]
    sched_a, sched_b = [0.5, 3.0, 1.25, -0.75, 2.0], linear_guidance(T, 4.0)
    try:
        for dtype in (torch.float32, torch.bfloat16):
            pipe.set_compute_dtype(dtype)
            ctx, ctx_lens = pipe.text_model(texts, return_lens=True)
            neg, neg_lens = pipe.text_model(negs, return_lens=True)
            assert neg.shape[1] == LN and ctx.shape[1] == L and len(set(neg_lens.tolist())) > 1
            ref_a = _chain(pipe, ctx, ctx_lens, neg, neg_lens, T, topk, seed, sched_a)
            ref_b = _chain(pipe, ctx, ctx_lens, neg, neg_lens, T, topk, seed, sched_b)
            assert not torch.equal(ref_a[0], ref_b[0])
            kw = dict(timesteps=T, topk=topk, save_interval=1, seed=seed, return_ids=True, negative_text=negs, mask_padding=True)
            modes = (dict(use_graph=False, streams=1), dict(), dict(), dict(), dict(use_graph=True, streams=2), dict(use_graph=True, streams=2),
                     dict(use_graph=True, streams=2))
            for mode in modes:
                imgs, ids = pipe.generate(texts, guidance_scale=sched_a, **kw, **mode)
                assert torch.equal(ids.cpu(), ref_a[0]), (dtype, mode)
                assert len(imgs) == T and all(torch.equal(a, b) for a, b in zip(imgs, ref_a[1])), (dtype, mode)
            # another schedule on the same shapes, through the graphs captured above: the scales are read, not baked in
            for mode in (dict(), dict(use_graph=True, streams=2)):
                imgs, ids = pipe.generate(texts, guidance_scale=sched_b, **kw, **mode)
                assert torch.equal(ids.cpu(), ref_b[0]), (dtype, mode)
                assert all(torch.equal(a, b) for a, b in zip(imgs, ref_b[1])), (dtype, mode)
            # one value T times is the scalar-scale loop, with and without the negative prompt: the device-scale combine at loop level
            for extra in (dict(negative_text=negs, mask_padding=True), dict()):
                base = dict(timesteps=T, topk=topk, save_interval=1, seed=seed, return_ids=True, **extra)
                for mode in (dict(use_graph=False, streams=1), dict(), dict()):
                    f_imgs, f_ids = pipe.generate(texts, guidance_scale=2.5, **base, **mode)
                    l_imgs, l_ids = pipe.generate(texts, guidance_scale=[2.5] * T, **base, **mode)
                    assert torch.equal(f_ids, l_ids) and all(torch.equal(a, b) for a, b in zip(f_imgs, l_imgs)), (dtype, mode, bool(extra))
    finally:
        pipe.set_compute_dtype(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# handle state and refusals on a real handle
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_later_call_never_runs_against_a_stale_negative_set(tiny):
    pipe, _, _ = tiny
    c = _step_case(pipe)
    eng, vq = pipe.engine(), pipe.vqgan.engine()
    kw = dict(seed=3, step=1, guidance_scale=2.0, context_lens=c["ctx_lens"])
    eng.sample(vq, c["ids"].clone(), c["ctx"], 4, 0.8, 8, negative_context=c["neg"], negative_lens=c["neg_lens"], **kw)
    after = eng.sample(vq, c["ids"].clone(), c["ctx"], 4, 0.8, 8, **kw)                    # straight after: the plain guided step
    fresh = eng.clone().sample(vq, c["ids"].clone(), c["ctx"], 4, 0.8, 8, **kw)
    assert torch.equal(after[0], fresh[0]) and torch.equal(after[1], fresh[1])
    # the loop too
    temps, nmask = [1.0, 0.5], [8, 1]
    eng.generate(vq, c["ids"].clone(), c["ctx"], temps, nmask, [True, True], 4, seed=3, guidance_scale=2.0, negative_context=c["neg"],
                 guidance_scales=[1.0, 2.0])
    after = eng.generate(vq, c["ids"].clone(), c["ctx"], temps, nmask, [True, True], 4, seed=3, guidance_scale=2.0)
    fresh = eng.clone().generate(vq, c["ids"].clone(), c["ctx"], temps, nmask, [True, True], 4, seed=3, guidance_scale=2.0)
    assert torch.equal(after[0], fresh[0]) and torch.equal(after[1], fresh[1])
    # a slots step may keep the context a slots step prepared, never the one a negative call left behind
    slots = (_lib.Slot * c["B"])(*[_lib.Slot(7, b, 0.8, 4, 8, 0) for b in range(c["B"])])
    eng.step_slots(c["ids"].clone(), c["ctx"], slots)
    eng.step_slots(c["ids"].clone(), c["ctx"], slots, keep_context=True)
    eng.sample(vq, c["ids"].clone(), c["ctx"], 4, 0.8, 8, negative_context=c["neg"], **kw)
    with pytest.raises(_lib.PmhipError) as e:
        eng.step_slots(c["ids"].clone(), c["ctx"], slots, keep_context=True)
    assert e.value.code == _lib.PMHIP_ESTATE


def test_refusals_on_a_real_handle_leave_the_ids_alone(tiny):
    pipe, _, _ = tiny
    c = _step_case(pipe)
    eng, vq = pipe.engine(), pipe.vqgan.engine()
    lib, B = eng.lib, c["B"]
    ids = c["ids"].clone()
    ctx, neg = c["ctx"].contiguous(), torch.nan_to_num(c["neg"]).contiguous()
    arr = lambda *v: (C.c_int * len(v))(*v)
    fl = lambda *v: (C.c_float * len(v))(*v)
    T2 = (fl(1.0, 0.5), arr(8, 1), (C.c_ubyte * 2)(0, 0))

    def sample(context, Lc, guided, negative, Ln, nl):
        with torch.cuda.device(dev()):
            return lib.pmhip_pipeline_sample_negative(eng.handle, vq.handle, _p(ids), _p(context), Lc, B, None, 4, 0.8, 8, None, 1, 0, 0, None, None,
                                                      None, guided, 2.0, 0.0, None, 1.0, _p(negative), Ln, nl, stream_ptr(dev()))

    def generate(context, Lc, guided, negative, Ln, nl, gs):
        with torch.cuda.device(dev()):
            return lib.pmhip_pipeline_generate_negative(eng.handle, vq.handle, _p(ids), _p(context), Lc, B, None, 2, *T2, 4, 1, 0, None, 0,
                                                        stream_ptr(dev()), None, 0, None, guided, 2.0, None, 1.0, _p(negative), Ln, nl, gs)

    cases = [
        (lambda: sample(ctx, L, 0, neg, LN, None), "pipeline_sample_negative", "needs guidance"),
        (lambda: sample(None, 0, 1, neg, LN, None), "pipeline_sample_negative", "a context"),
        (lambda: sample(ctx, L, 1, neg, 0, None), "pipeline_sample_negative", "Ln=0"),
        (lambda: sample(ctx, L, 1, neg, LN, arr(1, LN + 1, 2)), "pipeline_sample_negative", "image 1"),
        (lambda: sample(ctx, L, 1, None, 0, arr(1, 1, 1)), "pipeline_sample_negative", "without a negative context"),
        (lambda: generate(ctx, L, 0, neg, LN, None, None), "pipeline_generate_negative", "needs guidance"),
        (lambda: generate(ctx, L, 1, neg, LN, arr(0, 1, 1), None), "pipeline_generate_negative", "image 0"),
        (lambda: generate(ctx, L, 0, None, 0, None, fl(1.0, 2.0)), "pipeline_generate_negative", "needs guidance"),
        (lambda: generate(ctx, L, 1, None, 0, None, fl(1.0, float("nan"))), "pipeline_generate_negative", "step 1"),
        (lambda: generate(ctx, L, 1, neg, LN, None, fl(float("inf"), 1.0)), "pipeline_generate_negative", "step 0"),
    ]
    for run, who, word in cases:
        rc = run()
        msg = lib.pmhip_last_error().decode()
        assert rc == _lib.PMHIP_EINVAL and who in msg and word in msg, (rc, msg)
    torch.cuda.synchronize()
    assert torch.equal(ids, c["ids"])
    # the handle still works
    got = eng.sample(vq, ids.clone(), ctx, 4, 0.8, 8, seed=3, guidance_scale=2.0, negative_context=neg)
    assert bool(torch.isfinite(got[1]).all()) and not torch.equal(got[0], ids)
