"""Prompt-to-prompt at the model level (pmhip_s2_forward_control, ``S2Engine.forward_control``, ``Pipeline.control_ids``; DESIGN.md
section 4za) on the tiny pipeline, 2 pairs, ids from seed 11, context lengths 77 / 50 (source) and 60 / 33 (edited), NaN in every
context row behind its length -- the recipe of tests/test_gpu_maps.py.

The source half's logits are those of the existing forward on the source alone, bit for bit, and a forward behind a forward_control
runs what it ran before; the edited half is held to the plain-torch branch of the same model at the project's float bar in
fp32-verify (bf16 printed), with counter-checks that give the bar teeth; the engine validates before it launches."""
import ctypes as C

import numpy as np
import pytest
import torch

import control_ref as R
import paintmind_amd as pm
from gpu_common import dev
from paintmind_amd import _lib
from paintmind_amd.generate import Pipeline
from util import load_golden, to_torch_sd

pytestmark = pytest.mark.gpu

TOL = 1e-3                      # the project's float bar (tests/test_gpu_context_lens.py)
B = 2                           # pairs
LENS_SRC, LENS_EDIT = [77, 50], [60, 33]
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


@pytest.fixture(scope="module")
def data(cpu_pipe):
    pipe = cpu_pipe
    rows = pipe.text_model(["a", "b", "c", "d"]).cpu()
    lens = LENS_SRC + LENS_EDIT
    for b, n in enumerate(lens):
        rows[b, n:] = float("nan")
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, pipe.mask_token_id, (2 * B, pipe.num_tokens), generator=g)
    ids[torch.rand(2 * B, pipe.num_tokens, generator=g) < 0.5] = pipe.mask_token_id
    rm, bl, gn = R.controls(B, 77, 77, seed=3)                 # repeats, -1, blends in {0, .3, .5, 1}, gains in {0, .5, 1, 1.7, 2}
    rm = np.where(rm >= 77, 76, rm).astype(np.int32)           # (the model level refuses entries at or above L; 76 is behind pair 1's 50)
    return dict(ctx=rows, lens=lens, ids=ids, tok=pipe.ids2tokens(ids), rm=rm, bl=bl, gn=gn)


@pytest.fixture(scope="module")
def cpu_logits(cpu_pipe, data):
    """the plain-torch branch's logits per (cross layers, self layers): computed once, shared, never modified"""
    cache = {}

    def get(cross, inject, rm=None):
        key = (tuple(cross), tuple(inject), rm is not None)
        if key not in cache:
            ctl = dict(cross_layers=cross, self_layers=inject)
            if cross:
                ctl.update(row_map=data["rm"] if rm is None else rm, blend=data["bl"], gain=data["gn"])
            with torch.no_grad():
                cache[key] = cpu_pipe.transformer(data["tok"], data["ctx"], context_lens=data["lens"], control=ctl)
        return cache[key]
    return get


class in_dtype:
    def __init__(self, pipe, dtype):
        self.pipe, self.dtype = pipe, dtype

    def __enter__(self):
        self.pipe.set_compute_dtype(self.dtype)

    def __exit__(self, *exc):
        self.pipe.set_compute_dtype(torch.float32)


def _ctl(data):
    return dict(row_map=data["rm"], blend=data["bl"], gain=data["gn"])


@DTYPES
def test_the_source_half_is_the_plain_forward_and_a_later_forward_is_unchanged(tiny_pipe, data, dtype):
    tok, ctx, lens = data["tok"].to(dev()), data["ctx"].to(dev()), data["lens"]
    with in_dtype(tiny_pipe, dtype):
        eng = tiny_pipe.engine()
        count = eng.graph_count()
        first = eng.forward(tok, ctx, context_lens=lens)
        alone = eng.forward(tok[:B], ctx[:B], context_lens=lens[:B])
        assert torch.equal(first[:B], alone)
        for cross, inject in (([0], []), ([1], [1]), ([0, 1], [0]), ([], [1])):
            got = eng.forward_control(tok, ctx, cross_layers=cross, self_layers=inject, context_lens=lens, **(_ctl(data) if cross else {}))
            assert torch.equal(got[:B], alone), (cross, inject)
            assert torch.isfinite(got).all() and not torch.equal(got[B:], first[B:]), (cross, inject)
        assert torch.equal(eng.forward(tok, ctx, context_lens=lens), first)
        assert eng.graph_count() == count                                 # eager only: no key added to the graph cache
        # without lengths (finite rows): the same identities
        fin = torch.nan_to_num(ctx)
        got = eng.forward_control(tok, fin, cross_layers=[0, 1], **_ctl(data))
        assert torch.equal(got[:B], eng.forward(tok[:B], fin[:B]))
        # blend 0 and gain 1 is the plain forward within the float bar; both halves alike under injection give one result twice
        same = eng.forward_control(tok, ctx, cross_layers=[0, 1], context_lens=lens, row_map=data["rm"], blend=np.zeros_like(data["bl"]),
                                   gain=np.ones_like(data["gn"]))
        gap = float((same - first).abs().max())
        print(f"{dtype}: blend 0, gain 1 against the plain forward: {gap:.3e}")
        assert dtype != torch.float32 or gap < TOL
        twice_tok, twice_ctx = torch.cat([tok[:B], tok[:B]]), torch.cat([ctx[:B], ctx[:B]])
        twin = eng.forward_control(twice_tok, twice_ctx, self_layers=[0, 1], context_lens=lens[:B] * 2)
        assert torch.equal(twin[:B], twin[B:])                            # the edited half read the source half's Q and K: its own


@DTYPES
def test_the_edited_half_against_the_cpu_branch_of_the_same_model(tiny_pipe, cpu_logits, data, dtype):
    """fp32-verify is gated at the project's float bar; the bf16 figures are printed, not gated.  Counter-checks: the control dropped,
    another layer, the map reversed, the injection dropped -- all beyond the bar by a printed factor"""
    tok, ctx, lens = data["tok"].to(dev()), data["ctx"].to(dev()), data["lens"]
    rev = np.where(data["rm"] >= 0, 76 - data["rm"], data["rm"]).astype(np.int32)
    with in_dtype(tiny_pipe, dtype):
        eng = tiny_pipe.engine()
        for cross, inject in (([0], []), ([1], []), ([0, 1], []), ([1], [0]), ([], [0, 1])):
            got = eng.forward_control(tok, ctx, cross_layers=cross, self_layers=inject, context_lens=lens, **(_ctl(data) if cross else {})).cpu()
            err = float((got - cpu_logits(cross, inject)).abs().max())
            print(f"{dtype} cross={cross} self={inject}: max |logits GPU - logits CPU branch| = {err:.3e}")
            if dtype == torch.float32:
                assert err < TOL, (cross, inject, err)
        if dtype == torch.float32:
            got = eng.forward_control(tok, ctx, cross_layers=[1], self_layers=[0], context_lens=lens, **_ctl(data)).cpu()
            wrong = {"control dropped": eng.forward(tok, ctx, context_lens=lens).cpu(),
                     "another layer": cpu_logits([0], [0]), "map reversed": cpu_logits([1], [0], rm=rev), "injection dropped": cpu_logits([1], [])}
            for what, other in wrong.items():
                miss = float((got[B:] - other[B:]).abs().max())
                print(f"{what}: misses the bar by a factor of {miss / TOL:.1f}")
                assert miss > TOL, what
        # the operator composition of the same model on the GPU (modules/attention.py: ops.attention on the source half's Q and K
        # and the edited half's V^T, ops.attention_control) agrees with the engine
        with torch.no_grad():
            comp = tiny_pipe.transformer(tok, ctx, context_lens=lens, control=dict(cross_layers=[1], self_layers=[0], **_ctl(data)))
        gap = float((comp - eng.forward_control(tok, ctx, cross_layers=[1], self_layers=[0], context_lens=lens, **_ctl(data))).abs().max())
        print(f"{dtype}: engine against the operator composition: {gap:.3e}")
        assert dtype != torch.float32 or gap == 0.0                       # fp32-verify: the same kernels in the same order, bit for bit


def test_the_engine_validates_before_it_launches(tiny_pipe, data):
    pipe = tiny_pipe
    eng = pipe.engine()
    tok, ctx = data["tok"].to(dev()).contiguous(), torch.nan_to_num(data["ctx"]).to(dev()).contiguous()
    L, N = ctx.shape[1], pipe.num_tokens
    sentinel = 12345.0
    logits = torch.full((2 * B, N, eng.n_embed), sentinel, device=dev())
    i32p, f32p = C.POINTER(C.c_int), C.POINTER(C.c_float)
    count = eng.graph_count()
    arr = lambda x, dt, p: None if x is None else np.ascontiguousarray(x, dt).ctypes.data_as(p)

    def call(context=ctx, lens=None, cross=1, inject=0, rm=data["rm"], bl=data["bl"], gn=data["gn"], pairs=B):
        keep = [np.ascontiguousarray(rm, np.int32) if rm is not None else None, np.ascontiguousarray(bl, np.float32) if bl is not None else None,
                np.ascontiguousarray(gn, np.float32) if gn is not None else None]
        return eng.lib.pmhip_s2_forward_control(eng.handle, tok.data_ptr(), None if context is None else context.data_ptr(),
                                                L if context is not None else 0, pairs, None if lens is None else (C.c_int * (2 * B))(*lens),
                                                cross, inject, None if keep[0] is None else keep[0].ctypes.data_as(i32p),
                                                None if keep[1] is None else keep[1].ctypes.data_as(f32p),
                                                None if keep[2] is None else keep[2].ctypes.data_as(f32p), logits.data_ptr(), None)

    nan_gain, big_map = data["gn"].copy(), data["rm"].copy()
    nan_gain[1, 3], big_map[0, 5] = float("nan"), L
    for kwargs, text in ((dict(context=None), b"a context is required"), (dict(cross=0), b"select no layer"), (dict(cross=4), b"at or above depth=2"),
                         (dict(cross=0, inject=(1 << 63)), b"at or above depth"), (dict(rm=None), b"required with cross_bits"),
                         (dict(gn=None), b"required with cross_bits"), (dict(cross=0, inject=1), b"refused without"),
                         (dict(lens=[0, 1, 1, 1]), b"context length 0 must be in"), (dict(rm=big_map), b"must be below L"),
                         (dict(bl=data["bl"] + 0.8), b"must be in [0, 1]"), (dict(bl=-data["bl"] - 0.1), b"must be in [0, 1]"),
                         (dict(gn=nan_gain), b"finite and >= 0"), (dict(gn=-data["gn"] - 1), b"finite and >= 0"), (dict(pairs=0), b"bad arguments")):
        assert call(**kwargs) == _lib.PMHIP_EINVAL, kwargs
        msg = eng.lib.pmhip_last_error()
        assert b"s2_forward_control" in msg and text in msg, (kwargs, msg)
    torch.cuda.synchronize()
    assert bool((logits == sentinel).all())                               # nothing was launched
    assert call() == _lib.PMHIP_OK and call(cross=0, inject=3, rm=None, bl=None, gn=None) == _lib.PMHIP_OK and call(cross=3, inject=2, lens=[L, 5, 1, 9]) == _lib.PMHIP_OK
    torch.cuda.synchronize()
    assert bool(torch.isfinite(logits).all()) and not bool((logits == sentinel).any()) and eng.graph_count() == count
    for bad in (dict(cross_layers=[2], **_ctl(data)), dict(cross_layers=[0]), dict(self_layers=[0], **_ctl(data)), dict(**_ctl(data)),
                dict(cross_layers=[0, 0], **_ctl(data))):
        with pytest.raises(ValueError):
            eng.forward_control(tok, ctx, **bad)
    with pytest.raises(ValueError, match="context is required"):
        eng.forward_control(tok, None, self_layers=[0])
    # the control is cleared on the error path too: a forward behind a failed call equals one before it
    before = eng.forward(tok, ctx)
    assert call(cross=4) == _lib.PMHIP_EINVAL
    assert torch.equal(eng.forward(tok, ctx), before)


@DTYPES
def test_control_ids(tiny_pipe, data, dtype):
    """ids_src is generate_ids on the source alone, bit for bit, with and without guidance; without controlled steps ids_edit is the
    plain run of the edited context; with them it is another image"""
    pipe = tiny_pipe
    ctx = data["ctx"].to(dev())
    src, edit = ctx[:B].contiguous(), ctx[B:].contiguous()
    T, seed = 4, 7
    with in_dtype(pipe, dtype):
        plain = lambda c, n, **kw: pipe.generate_ids(c, B, T, 1.0, 3, [False] * T, seed, use_graph=False, streams=1, context_lens=n, **kw)[0]
        args = (src, edit, LENS_SRC, LENS_EDIT, data["rm"], data["bl"], data["gn"], B, T, 1.0, 3, seed)
        a, b = pipe.control_ids(*args, cross_steps=0.8, self_steps=0.5)
        assert torch.equal(a, plain(src, LENS_SRC))
        a0, b0 = pipe.control_ids(*args, cross_steps=0, self_steps=0)
        assert torch.equal(a0, a) and torch.equal(b0, plain(edit, LENS_EDIT))
        assert not torch.equal(b, b0)
        ag, bg = pipe.control_ids(*args, guidance_scale=3.0, cross_steps=0.5)
        assert torch.equal(ag, plain(src, LENS_SRC, guidance_scale=3.0))
        ag0, bg0 = pipe.control_ids(*args, guidance_scale=3.0, cross_steps=0, self_steps=0)
        assert torch.equal(ag0, ag) and torch.equal(bg0, plain(edit, LENS_EDIT, guidance_scale=3.0))
        a5, _ = pipe.control_ids(*args, image_base=5, top_p=0.9, choice_temperature=2.0)
        assert torch.equal(a5, plain(src, LENS_SRC, image_base=5, top_p=0.9, choice_temperature=2.0))
        ids_s, ids_e, img_s, img_e = pipe.control_ids(*args, want_imgs=True)
        S = pipe.image_size
        assert torch.equal(ids_s, a) and tuple(img_e.shape) == (B, 3, S, S) and torch.isfinite(img_e).all() and torch.isfinite(img_s).all()


def test_an_injected_layer_is_ops_attention_on_the_source_halfs_q_and_k(tiny_pipe, data, monkeypatch):
    """fp32-verify, source and edited tokens and contexts DIFFERENT: the operator composition of the same model runs the injected
    layer's edited half as ops.attention(q_src, k_src, v_edit) -- seen by wrapping ops.attention --, and the engine's logits equal the
    composition's bit for bit; the composition without the injection ends elsewhere"""
    from paintmind_amd import ops
    tok, ctx, lens = data["tok"].to(dev()), data["ctx"].to(dev()), data["lens"]
    assert not torch.equal(tok[:B], tok[B:])
    calls, real = [], ops.attention

    def spy(q, k, vt, n_kv, **kw):
        out = real(q, k, vt, n_kv, **kw)
        calls.append((q, k, vt, out))
        return out

    tiny_pipe.set_compute_dtype(torch.float32)
    eng = tiny_pipe.engine()
    for inject, cross in (([0], []), ([1], [1]), ([0, 1], [0])):
        ctl = dict(self_layers=inject, cross_layers=cross, **(_ctl(data) if cross else {}))
        calls.clear()
        monkeypatch.setattr(ops, "attention", spy)
        with torch.no_grad():
            comp = tiny_pipe.transformer(tok, ctx, context_lens=lens, control=ctl)
        monkeypatch.setattr(ops, "attention", real)
        pairs = [(a, b) for a, b in zip(calls, calls[1:]) if b[0].data_ptr() == a[0].data_ptr() and b[1].data_ptr() == a[1].data_ptr()]
        assert len(pairs) == len(inject)                                  # per injected layer: two launches on ONE q and k, the source half's
        for (q, k, vt_src, _), (_, _, vt_edit, out) in pairs:
            assert q.shape[0] == B and vt_edit.data_ptr() == vt_src.data_ptr() + vt_src.numel() * vt_src.element_size()
            assert torch.equal(out, real(q, k, vt_edit, tiny_pipe.num_tokens))
        got = eng.forward_control(tok, ctx, context_lens=lens, **ctl)
        assert torch.equal(got, comp), (inject, cross, float((got - comp).abs().max()))
        with torch.no_grad():
            other = tiny_pipe.transformer(tok, ctx, context_lens=lens, control=dict(ctl, self_layers=[])) if cross else \
                tiny_pipe.transformer(tok, ctx, context_lens=lens)
        assert not torch.equal(other[B:], comp[B:]) and torch.equal(other[:B], comp[:B])


@DTYPES
def test_control_ids_under_guidance_is_the_operator_composition(tiny_pipe, data, dtype):
    """guidance 3, controlled steps: both halves' ids equal the loop composed here from the operator-level calls -- forward_control,
    forward without a context, guidance_combine, sample_rows and remask once per half under the same seed, step and image base; in
    fp32-verify also with the logits of the CondTransformer operator composition instead of the engine's"""
    from paintmind_amd import ops
    pipe = tiny_pipe
    ctx = data["ctx"].to(dev())
    T, seed, N = 4, 7, pipe.num_tokens
    n_cross, n_self = 3, 2                                                # ceil(0.7 * 4), ceil(0.5 * 4)
    with in_dtype(pipe, dtype):
        eng = pipe.engine()
        temps, nmask = pipe._schedule(T, 1.0)
        got = pipe.control_ids(ctx[:B].contiguous(), ctx[B:].contiguous(), LENS_SRC, LENS_EDIT, data["rm"], data["bl"], data["gn"], B, T, 1.0, 3,
                               seed, image_base=2, guidance_scale=3.0, cross_steps=0.7, self_steps=0.5)
        for module in ((False, True) if dtype == torch.float32 else (False,)):
            ids = torch.full((2 * B, N), pipe.mask_token_id, dtype=torch.long, device=dev())
            for step in range(T):
                tok = pipe.ids2tokens(ids)
                cross, inject = ([0, 1] if step < n_cross else []), ([0, 1] if step < n_self else [])
                ctl = dict(cross_layers=cross, self_layers=inject, **(_ctl(data) if cross else {}))
                if module:
                    with torch.no_grad():
                        cond = pipe.transformer(tok, ctx, context_lens=data["lens"], **(dict(control=ctl) if cross or inject else {})).contiguous()
                        uncond = pipe.transformer(tok, None).contiguous()
                else:
                    cond = eng.forward_control(tok, ctx, context_lens=data["lens"], **ctl) if cross or inject else \
                        eng.forward(tok, ctx, context_lens=data["lens"])
                    uncond = eng.forward(tok, None)
                logits = ops.guidance_combine(cond, uncond, 3.0).reshape(2 * B * N, -1)
                for h in range(2):
                    rows = slice(h * B * N, (h + 1) * B * N)
                    _, merged, score = ops.sample_rows(logits[rows], ids.reshape(-1)[rows], pipe.mask_token_id, 3, temps[step], seed=seed, step=step,
                                                       row_base=2 * N)
                    ids[h * B:(h + 1) * B] = ops.remask(merged.reshape(B, N), score.reshape(B, N), nmask[step], pipe.mask_token_id)
            assert torch.equal(got[0], ids[:B]) and torch.equal(got[1], ids[B:]), (dtype, module)
        plain = pipe.control_ids(ctx[:B].contiguous(), ctx[B:].contiguous(), LENS_SRC, LENS_EDIT, data["rm"], data["bl"], data["gn"], B, T, 1.0, 3,
                                 seed, image_base=2, guidance_scale=3.0, cross_steps=0, self_steps=0)
        assert torch.equal(plain[0], got[0]) and not torch.equal(plain[1], got[1])


def _near_tie_audit(pipe, cpu_pipe, data, noise, T, topk, ctl_steps):
    """The loop step by step on the GPU's ids: the GPU's step and the CPU branch's step from the SAME ids and noise must agree, and a
    position where they do not must be a near-tie -- the top-2 gap of its perturbed logits below 1e-3 (an arg-max flip), or its
    re-masking score within 1e-4 of the step's cut.  -> the number of such positions"""
    from paintmind_amd import ops
    eng, N, V = pipe.engine(), pipe.num_tokens, pipe.mask_token_id
    temps, nmask = pipe._schedule(T, 1.0)
    ids = torch.full((2 * B, N), V, dtype=torch.long, device=dev())
    ctx, lens, ties = data["ctx"], data["lens"], 0
    for step in range(T):
        on = step < ctl_steps
        ctl = dict(cross_layers=[0, 1] if on else [], self_layers=[], **(_ctl(data) if on else {}))
        tok = pipe.ids2tokens(ids)
        lg = eng.forward_control(tok, ctx.to(dev()), context_lens=lens, **ctl) if on else eng.forward(tok, ctx.to(dev()), context_lens=lens)
        with torch.no_grad():
            lc = cpu_pipe.transformer(tok.cpu(), ctx, context_lens=lens, **(dict(control=ctl) if on else {}))
        nxt = ids.clone()
        for h in range(2):
            rows, u = slice(h * B, (h + 1) * B), noise[step]
            _, merged, score = ops.sample_rows(lg[rows].reshape(B * N, -1), ids[rows].reshape(-1), V, topk, temps[step],
                                               noise=u.to(dev()).reshape(B * N, -1).contiguous())
            nxt[rows] = ops.remask(merged.reshape(B, N), score.reshape(B, N), nmask[step], V)
            want = cpu_pipe._tail_cpu(ids[rows].cpu(), lc[rows], nmask[step], topk, temps[step], u, None, counts=[nmask[step]] * B)[0]
            bad = (nxt[rows].cpu() != want).nonzero()
            if len(bad):
                val, ind = lc[rows].topk(topk, dim=-1)
                z = torch.full_like(lc[rows], float("-inf")).scatter_(2, ind, val) / temps[step] - torch.log(-torch.log(u.clamp(min=1e-20)).clamp(min=1e-20))
                top2 = z.topk(2, dim=-1).values
                gap = top2[..., 0] - top2[..., 1]
                s = 1 - lc[rows].softmax(-1).gather(2, z.argmax(-1, keepdim=True))[..., 0]
                s = s.masked_fill(ids[rows].cpu() != V, -1e5)
                cut = s.topk(nmask[step], dim=-1).values[:, -1:]
                for b, i in bad.tolist():
                    assert float(gap[b, i]) < 1e-3 or abs(float(s[b, i] - cut[b, 0])) < 1e-4 or any(float(gap[b, j]) < 1e-3 for j in range(N)), \
                        (step, h, b, i, float(gap[b, i]), float(s[b, i]), float(cut[b, 0]))
                ties += len(bad)
        ids = nxt
    return ties


def test_control_ids_against_the_cpu_branch_in_fp32(tiny_pipe, cpu_pipe, data):
    """fp32-verify, the same uniforms on both sides: the ids of the CPU branch exactly, unless a near-tie explains a difference (then
    the loop is audited step by step from the GPU's ids)"""
    T, topk = 4, 3
    noise = torch.rand(T, B, tiny_pipe.num_tokens, tiny_pipe.mask_token_id, generator=torch.Generator().manual_seed(5))
    ctx = data["ctx"]
    args = (LENS_SRC, LENS_EDIT, data["rm"], data["bl"], data["gn"], B, T, 1.0, topk, 9)
    ties = _near_tie_audit(tiny_pipe, cpu_pipe, data, noise, T, topk, ctl_steps=3)
    print(f"positions explained by a near-tie: {ties}")
    got = tiny_pipe.control_ids(ctx[:B].to(dev()), ctx[B:].to(dev()), *args, cross_steps=0.75, noise=noise)
    want = cpu_pipe.control_ids(ctx[:B], ctx[B:], *args, cross_steps=0.75, noise=noise)
    other = cpu_pipe.control_ids(ctx[:B], ctx[B:], *args, cross_steps=0, noise=noise)
    assert torch.equal(other[0], want[0]) and not torch.equal(other[1], want[1])          # the control moves the edited image
    if ties == 0:
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])


# ------------------------------------------------------------------------------------------------------------- prompt_to_prompt

class CharTokenizer:
    """one id per character (2 + ord % 100), pad 0, end-of-sequence 1; both call forms the embedder uses"""
    pad_token_id, eos_token_id = 0, 1

    @staticmethod
    def ids_of(s):
        return [2 + ord(c) % 100 for c in s]

    def __call__(self, text, max_length=77, add_special_tokens=True, **kw):
        if isinstance(text, str):
            return {"input_ids": self.ids_of(text) + ([1] if add_special_tokens else [])}
        out = torch.zeros(len(text), max_length, dtype=torch.long)
        for i, s in enumerate(text):
            row = self.ids_of(s)[:max_length - 1] + [1]
            out[i, :len(row)] = torch.tensor(row)
        return {"input_ids": out}


def test_prompt_to_prompt_end_to_end_with_an_injected_t5():
    from paintmind_amd.modules.encoder import T5TextEmbedder
    from text_stubs import tiny_t5
    p, _ = load_golden("tiny_pipeline.npz")
    t5 = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False,
                  text_model=T5TextEmbedder(tokenizer=CharTokenizer(), transformer=tiny_t5(), max_length=24))
    t5.load_state_dict(to_torch_sd(p), strict=False)
    t5 = t5.eval().to(dev())
    calls, control_ids = [], t5.control_ids
    t5.control_ids = lambda *a, **kw: (calls.append(a), control_ids(*a, **kw))[1]
    text, edit = ["a red barn", "the cow"], ["a red church", "the big cow"]
    kw = dict(mode="replace", reweight={"church": 2.0, "big": 0.5}, timesteps=3, seed=5)
    img_s, img_e = t5.prompt_to_prompt(text, edit, **kw)
    S = t5.image_size
    assert img_s.is_cuda and tuple(img_s.shape) == tuple(img_e.shape) == (2, 3, S, S) and torch.isfinite(img_e).all() and torch.isfinite(img_s).all()
    lens_s, lens_e, rm, bl, gn = calls[0][2:7]
    assert lens_s == [11, 8] and lens_e == [13, 12]                              # always under the non-pad lengths
    assert rm[0, :13].tolist() == [0, 1, 2, 3, 4, 5, 6, 6, 7, 8, 9, 9, 10] and (rm[0, 13:] == -1).all() and (bl[0, :13] == 1).all()
    assert gn[0].tolist() == [1.0] * 6 + [2.0] * 6 + [1.0] * 12                  # the gain sits on the rows phrase_rows finds
    assert torch.equal(torch.from_numpy(gn[0] != 1), t5.text_model.phrase_rows(edit[:1], "church")[2][0])
    assert rm[1, :12].tolist() == [0, 1, 2, 3, -1, -1, -1, -1, 4, 5, 6, 7] and gn[1].tolist() == [1.0] * 4 + [0.5] * 3 + [1.0] * 17
    ids_s, ids_e = t5.prompt_to_prompt(text, edit, return_ids=True, **kw)
    ctx, lens = t5.text_model(text, return_lens=True)
    plain, imgs = t5.generate_ids(ctx.to(dev()), 2, 3, 1.0, 5, [False, False, True], 5, use_graph=False, streams=1, context_lens=lens)
    assert torch.equal(ids_s, plain) and not torch.equal(ids_e, ids_s)           # the source is the plain image, the edit another
    assert float((img_s - imgs[-1]).abs().max()) < 1e-4                           # (decoded by the module here, by the native loop there)
    one, _ = t5.prompt_to_prompt(text, edit, return_ids=True, **dict(kw, reweight=None))
    assert torch.equal(one, ids_s)
    _, weak = t5.prompt_to_prompt(text, edit, return_ids=True, **dict(kw, reweight={"church": 0.0}))
    assert not torch.equal(weak, ids_e)                                          # the gain reaches the kernel
    for bad in (dict(negative_text=["x", "y"]), dict(regions=[]), dict(prompt_weights=True), dict(context_weights=np.ones((2, 24))),
                dict(context_segments=np.zeros((2, 24))), dict(guidance_scale=[1.0, 2.0, 3.0]), dict(reweight={"zebra": 2.0}), dict(mode="swap")):
        with pytest.raises(ValueError):
            t5.prompt_to_prompt(text, edit, timesteps=3, seed=5, **bad)
    with pytest.raises(ValueError, match="text condition"):
        t5.prompt_to_prompt(None, edit, timesteps=2, seed=1)
