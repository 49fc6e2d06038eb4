"""Regional prompts at the model level (the *_segments entries of include/pmhip.h) on the tiny pipeline, B = 3:
image 0 with two regions, image 1 with one, image 2 with none beside the global prompt, so the images' totals differ and two of
them carry padding (NaN here).  ``tokens2logits`` against the plain-torch branch of the same model; the native loop, eager and
captured, against the per-step composition with the same arrays, also guided and with a negative prompt; two layouts through one
captured graph; two lanes against one; and ``CrossAttention`` itself at width 512 (dim_head 64) and at dim_head 32."""
import numpy as np
import pytest
import torch

import paintmind_amd as pm
import region_ref as R
from gpu_common import dev
from paintmind_amd.generate import Pipeline
from paintmind_amd.modules.attention import CrossAttention
from util import load_golden, to_torch_sd

pytestmark = pytest.mark.gpu

TOL = 1e-3                      # the project's float bar (tests/test_gpu_context_lens.py)
B, T, TOPK, TEMP, SEED = 3, 3, 4, 1.0, 77
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


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


def _layout(pipe, which):
    """two layouts of regions over the same prompts' rows: (context [3, 126, 96] with NaN padding, key_seg, query_mask)"""
    S, g = pipe.image_size, pipe.image_size // pipe.patch_size
    left = torch.zeros(S, S)
    left[:, :S // 2] = 1
    corner = torch.zeros(S, S)
    corner[S // 2:, S // 2:] = 1
    tm = torch.zeros(g, g, dtype=torch.bool)
    tm[1:3, 1:3] = True
    rows = pipe.text_model(["a", "b", "c", "d", "e", "f"]).cpu()
    if which == 0:
        regions = [[(rows[3, :40], left), (rows[4, :9], corner)], [(rows[5, :25], tm)], []]
    else:                                                             # other masks, other lengths, the same longest total
        regions = [[(rows[3, :9], corner), (rows[4, :40], tm)], [], [(rows[5, :49], left)]]
    context, ks, qm = R.layout([rows[b] for b in range(B)], regions, pipe.image_size, pipe.patch_size)
    context[torch.from_numpy(ks == R.PAD)] = float("nan")
    return context, ks, qm


@pytest.fixture(scope="module")
def data(tiny_pipe):
    pipe = tiny_pipe
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, pipe.mask_token_id, (B, pipe.num_tokens), generator=g)
    ids[torch.rand(B, pipe.num_tokens, generator=g) < 0.5] = pipe.mask_token_id
    out = dict(ids=ids.to(dev()), layouts=[_layout(pipe, 0), _layout(pipe, 1)])
    out["tok"] = pipe.ids2tokens(out["ids"])
    out["neg"] = pipe.text_model(["n0", "n1", "n2"])[:, :33].contiguous().to(dev())
    assert out["layouts"][0][0].shape == out["layouts"][1][0].shape == (B, 126, 96)
    return out


class in_dtype:
    def __init__(self, pipe, dtype):
        self.pipe, self.dtype = pipe, dtype

    def __enter__(self):
        self.pipe.set_compute_dtype(self.dtype)

    def __exit__(self, *exc):
        self.pipe.set_compute_dtype(torch.float32)


@DTYPES
def test_logits_against_the_cpu_branch_of_the_same_model(tiny_pipe, cpu_pipe, data, dtype):
    """fp32-verify is gated at the project's float bar; the bf16 figure is printed, not gated.  Counter-check: the same (finite)
    context WITHOUT the arrays is far beyond 100 x the bar, so this cannot pass with the masks ignored."""
    context, ks, qm = data["layouts"][0]
    with torch.no_grad():
        want = cpu_pipe.tokens2logits(data["tok"].cpu(), context, context_segments=ks, token_segments=qm)
    with in_dtype(tiny_pipe, dtype):
        got = tiny_pipe.tokens2logits(data["tok"], context.to(dev()), context_segments=ks, token_segments=qm).cpu()
        loose = tiny_pipe.tokens2logits(data["tok"], torch.nan_to_num(context).to(dev())).cpu()
    assert torch.isfinite(got).all()
    err, gap = float((got - want).abs().max()), float((loose - want).abs().max())
    print(f"{dtype}: max |logits GPU - logits CPU branch| with two regions and a global prompt = {err:.3e}; without the arrays {gap:.3e}")
    if dtype == torch.float32:
        assert err < TOL
    assert gap > 100 * TOL


def _steps(pipe, ctx, ks, qm, **kw):
    """the loop step by step through the one-step entry with the same arrays -> final ids"""
    eng = pipe.engine()
    temps, nmask = pipe._schedule(T, TEMP)
    ids = torch.full((B, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long, device=dev())
    for step in range(T):
        ids, _, _, _ = eng.sample(None, ids, ctx, TOPK, temps[step], nmask[step], seed=SEED, step=step, want_img=False,
                                  context_segments=ks, token_segments=qm, **kw)
    return ids


def _loop(pipe, ctx, ks, qm, **kw):
    kw = {**dict(use_graph=False, streams=1), **kw}
    return pipe.generate_ids(ctx, B, T, TEMP, TOPK, [False] * (T - 1) + [True], SEED, context_segments=ks, token_segments=qm, **kw)


@DTYPES
def test_the_native_loop_is_the_per_step_composition(tiny_pipe, data, dtype):
    pipe = tiny_pipe
    context, ks, qm = data["layouts"][0]
    ctx = context.to(dev())
    with in_dtype(pipe, dtype):
        results = []
        for step_kw, loop_kw in ((dict(), dict()), (dict(guidance_scale=3.0), dict(guidance_scale=3.0)),
                                 (dict(guidance_scale=3.0, negative_context=data["neg"]), dict(guidance_scale=3.0, negative_context=data["neg"]))):
            want = _steps(pipe, ctx, ks, qm, **step_kw)
            for use_graph in (False, True, True):                     # first call eager, second captures, third replays
                ids, imgs = _loop(pipe, ctx, ks, qm, use_graph=use_graph, **loop_kw)
                assert torch.isfinite(imgs).all()
                assert torch.equal(ids, want), (step_kw.keys(), use_graph)
            results.append(want)
        assert not torch.equal(results[0], results[1]) and not torch.equal(results[1], results[2])
        # and the masks matter: the loop on the same (finite) context without them ends elsewhere
        plain, _ = pipe.generate_ids(torch.nan_to_num(ctx), B, T, TEMP, TOPK, [False] * T, SEED, use_graph=False, streams=1)
        assert not torch.equal(plain, results[0])


@DTYPES
def test_two_layouts_run_through_one_captured_graph(tiny_pipe, data, dtype):
    pipe = tiny_pipe
    (c0, ks0, qm0), (c1, ks1, qm1) = data["layouts"]
    with in_dtype(pipe, dtype):
        eng = pipe.engine()
        want0, want1 = _loop(pipe, c0.to(dev()), ks0, qm0), _loop(pipe, c1.to(dev()), ks1, qm1)
        assert not torch.equal(want0[0], want1[0])
        for _ in range(2):                                            # eager under the key, then captured
            got = _loop(pipe, c0.to(dev()), ks0, qm0, use_graph=True)
        assert torch.equal(got[0], want0[0]) and torch.equal(got[1], want0[1])
        entries, captured = eng.graph_count()
        assert captured >= 1
        got = _loop(pipe, c1.to(dev()), ks1, qm1, use_graph=True)     # a replay with a layout the capture never saw
        assert torch.equal(got[0], want1[0]) and torch.equal(got[1], want1[1])
        assert eng.graph_count() == (entries, captured)
        # the unmasked loop at the same (B, L) has a key of its own
        pipe.generate_ids(torch.nan_to_num(c0).to(dev()), B, T, TEMP, TOPK, [False] * (T - 1) + [True], SEED, use_graph=True, streams=1)
        assert eng.graph_count()[0] == entries + 1


@DTYPES
def test_two_lanes_agree_with_one(tiny_pipe, data, dtype):
    pipe = tiny_pipe
    context, ks, qm = data["layouts"][0]
    with in_dtype(pipe, dtype):
        want = _loop(pipe, context.to(dev()), ks, qm)
        for use_graph in (False, True, True):
            got = _loop(pipe, context.to(dev()), ks, qm, use_graph=use_graph, streams=2)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), use_graph


def test_generate_with_regions_runs_the_native_loop(tiny_pipe, cpu_pipe):
    """the public call: prompts and masks in, images out; its ids are those of generate_ids on the arrays it builds"""
    pipe = tiny_pipe
    S = pipe.image_size
    left = torch.zeros(S, S)
    left[:, :S // 2] = 1
    texts, regions = ["a", "b", "c"], [[("d", left)], [], [("e", left), ("f", 1 - left)]]
    imgs, ids = pipe.generate(texts, timesteps=T, topk=TOPK, save_interval=1, seed=SEED, return_ids=True, regions=regions, use_graph=False, streams=1)
    context, ks, qm = pipe._region_context(texts, regions, False)
    assert context.shape[1] == 3 * 77 and len(imgs) == T and torch.isfinite(imgs[-1]).all()
    want, _ = pipe.generate_ids(context.to(dev()), B, T, TEMP, TOPK, [False] * T, SEED, context_segments=ks, token_segments=qm)
    assert torch.equal(ids, want)
    # the native check stands behind the Python one: image 1 has no region, so a token of it that allows segment 1 alone has no key
    from paintmind_amd import _lib
    eng, bad = pipe.engine(), qm.copy()
    bad[1, 2] = 2
    tok, ctx = pipe.ids2tokens(want), context.to(dev()).contiguous()
    logits = torch.empty(B, pipe.num_tokens, eng.n_embed, device=dev())
    rc = eng.lib.pmhip_s2_forward_segments(eng.handle, tok.data_ptr(), ctx.data_ptr(), ctx.shape[1], B, np.ctypeslib.as_ctypes(ks.reshape(-1).copy()),
                                           np.ctypeslib.as_ctypes(bad.reshape(-1)), logits.data_ptr(), None)
    assert rc == _lib.PMHIP_EINVAL and b"image 1: token 2" in eng.lib.pmhip_last_error()


@pytest.mark.parametrize("width,heads,dh", [(512, 8, 64), (128, 4, 32)])
@DTYPES
def test_cross_attention_module_at_dim_head_64_and_32(width, heads, dh, dtype):
    """``CrossAttention`` itself on the device against the float64 restatement: N = 80 tokens, L = 129 rows in three segments and
    padding (NaN), fp32 gated at the float bar, bf16 printed; the run without masks is far beyond it"""
    torch.manual_seed(7)
    attn = CrossAttention(width, width, heads=heads, dim_head=dh).eval()
    N, L = 80, 129
    g = torch.Generator().manual_seed(5)
    x, ctx = torch.randn(B, N, width, generator=g), 4 * torch.randn(B, L, width, generator=g)
    ks = np.where(np.arange(L)[None, :] < np.array([129, 100, 65])[:, None], (np.arange(L) // 43)[None, :], R.PAD).astype(np.uint8)
    qm = (1 | (np.uint32(2) << (np.arange(N, dtype=np.uint32) % 2)[None, :])).repeat(B, 0).astype(np.uint32)      # global + one of two
    want = R.cross_attention(attn, x, ctx, ks, qm)
    poisoned = ctx.clone()
    poisoned[torch.from_numpy(ks == R.PAD)] = float("nan")
    attn = attn.to(dev())
    got = attn.run(x.to(dev()).to(dtype), poisoned.to(dev()).to(dtype), context_segments=ks, token_segments=qm).float().cpu()
    loose = attn.run(x.to(dev()).to(dtype), torch.where(torch.from_numpy(ks == R.PAD)[:, :, None], torch.zeros_like(ctx), ctx).to(dev()).to(dtype)).float().cpu()
    err, gap = float((got.double() - want).abs().max()), float((loose.double() - want).abs().max())
    print(f"CrossAttention width {width} dim_head {dh} {dtype}: max |GPU - float64| = {err:.3e}; without the masks {gap:.3e}")
    assert torch.isfinite(got).all()
    if dtype == torch.float32:
        assert err < TOL
    assert gap > 100 * TOL
