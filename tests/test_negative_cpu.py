"""Negative prompts and the per-step guidance schedule without a GPU: the plain-torch branch of a CPU pipeline (the rule, the
identity with the unguided step, the schedule against the stepwise chain), the routing of ``S2Engine.sample`` / ``generate`` on a
stub library, every ``ValueError`` of the public calls, and the refusals of the native entries before anything is launched."""
import contextlib
import ctypes as C
import itertools

import pytest
import torch

import paintmind_amd as pm
from paintmind_amd import _lib, engine as engine_mod, ops
from paintmind_amd.generate import Pipeline, _Options, linear_guidance, loop_schedule
from util import load_golden, to_torch_sd

NEW = ("pmhip_guidance_combine_dev", "pmhip_pipeline_sample_negative", "pmhip_pipeline_generate_negative")
L, LN = 7, 3


@pytest.fixture(scope="module")
def pipe():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False).eval()
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not [k for k in missing.missing_keys if not k.startswith("text_model")]
    return pipe


@pytest.fixture(scope="module")
def case(pipe):
    """B = 3 images of a half-masked state, a context of 7 rows, a negative context of 3 rows with lengths (1, 3, 2) and NaN planted
    behind every length, and the uniforms of one step"""
    B, N, V, D = 3, pipe.num_tokens, pipe.mask_token_id, pipe.text_model.context_dim
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, V, (B, N), generator=g)
    ids[torch.rand(B, N, generator=g) < 0.5] = V
    ctx, neg = torch.randn(B, L, D, generator=g), torch.randn(B, LN, D, generator=g)
    lens = [1, 3, 2]
    for b, n in enumerate(lens):
        neg[b, n:] = float("nan")
    return dict(B=B, ids=ids, ctx=ctx, neg=neg, lens=lens, noise=torch.rand(B, N, V, generator=g))


def _tail(pipe, logits, ids, nm, topk, temperature, noise):
    """the step behind its logits, as Pipeline._sample_cpu writes it (generate.py:163-179 of the reference)"""
    val, ind = logits.topk(topk, dim=-1)
    filtered = torch.full_like(logits, float("-inf")).scatter_(2, ind, val)
    gumbel = -torch.log((-torch.log(noise.clamp(min=1e-20))).clamp(min=1e-20))
    pred = (filtered / max(temperature, 1e-10) + gumbel).argmax(dim=-1)
    is_mask = ids == pipe.mask_token_id
    merged = torch.where(is_mask, pred, ids)
    scores = (1 - logits.softmax(dim=-1).gather(2, pred[..., None])[..., 0]).masked_fill(~is_mask, -1e5)
    return merged.scatter(1, scores.topk(nm, dim=-1).indices, pipe.mask_token_id), pipe.vqgan.decode_from_indice(pred)


def test_new_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.pmhip_abi_version() == 11 == _lib.ABI_VERSION
    header = open(_lib._HERE + "/../include/pmhip.h").read()
    for name in NEW:
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None and f"int {name}(" in header
    # the negative entries are the nucleus entries' argument lists plus the new arguments
    P = _lib.PROTOTYPES
    assert P["pmhip_pipeline_sample_negative"][1] == P["pmhip_pipeline_sample_nucleus"][1][:-1] + [_lib.vp, _lib.i32, C.POINTER(_lib.i32), _lib.vp]
    assert P["pmhip_pipeline_generate_negative"][1] == P["pmhip_pipeline_generate_nucleus"][1] + [_lib.vp, _lib.i32, C.POINTER(_lib.i32),
                                                                                                 C.POINTER(_lib.f32)]


@torch.no_grad()
@pytest.mark.parametrize("scale", [0.0, 1.0, 2.5, -1.0])
def test_the_rule_two_forwards_one_addcmul_and_the_tail(pipe, case, scale):
    c = case
    got, img = pipe.sample(c["ids"], 0.5, text=c["ctx"], topk=5, temperature=0.7, noise=c["noise"], guidance_scale=scale,
                           negative_text=c["neg"], negative_context_lens=c["lens"])
    tok = pipe.ids2tokens(c["ids"])
    cond, negl = pipe.tokens2logits(tok, c["ctx"]), pipe.tokens2logits(tok, c["neg"], c["lens"])
    assert bool(torch.isfinite(negl).all())                              # the NaN rows behind the lengths never reach a result
    logits = torch.addcmul(negl, cond - negl, torch.tensor(float(scale)))
    want, want_img = _tail(pipe, logits, c["ids"], 8, 5, 0.7, c["noise"])
    assert torch.equal(got, want) and torch.equal(img, want_img)
    if scale == 2.5:                                                     # ... and it is not the step without the negative prompt
        plain, _ = pipe.sample(c["ids"], 0.5, text=c["ctx"], topk=5, temperature=0.7, noise=c["noise"], guidance_scale=scale)
        uncond = pipe.tokens2logits(tok, None)
        assert not torch.equal(logits, torch.addcmul(uncond, cond - uncond, torch.tensor(scale)))
        assert plain.shape == got.shape


@torch.no_grad()
@pytest.mark.parametrize("scale", [0.0, 3.0, -2.0])
def test_the_context_as_its_own_negative_is_the_unguided_step(pipe, case, scale):
    """cond - neg is exactly 0 and fma(s, 0, u) == u: the same tensor and lengths on both sides give the unguided step's ids and
    image for any scale"""
    c = case
    lens = [7, 2, 5]
    kw = dict(text=c["ctx"], topk=4, temperature=0.9, noise=c["noise"], context_lens=lens)
    want, want_img = pipe.sample(c["ids"], 0.5, **kw)
    got, img = pipe.sample(c["ids"], 0.5, **kw, guidance_scale=scale, negative_text=c["ctx"], negative_context_lens=lens)
    assert torch.equal(got, want) and torch.equal(img, want_img)


def test_linear_guidance_and_the_schedule_keeps_its_signature():
    assert linear_guidance(4, 2.0) == [0.5, 1.0, 1.5, 2.0]
    assert linear_guidance(1, 3.0) == [3.0]
    temps, nmask, ctemps = loop_schedule(4, 1.0, 16)
    assert len(temps) == len(nmask) == 4 and ctemps is None
    assert _Options._fields[:5] == ("topk", "top_p", "guidance_scale", "lens", "choice_temperature")     # the new fields are appended
    assert _Options._fields[5:] == ("negative", "negative_lens", "guidance_scales")


@torch.no_grad()
def test_a_constant_schedule_is_the_float_and_a_varying_one_is_the_stepwise_chain(pipe):
    texts, T, seed = ["a", "b"], 4, 5
    kw = dict(timesteps=T, topk=3, save_interval=1, seed=seed, return_ids=True)
    f_imgs, f_ids = pipe.generate(texts, guidance_scale=1.5, **kw)
    l_imgs, l_ids = pipe.generate(texts, guidance_scale=[1.5] * T, **kw)
    assert torch.equal(f_ids, l_ids) and all(torch.equal(a, b) for a, b in zip(f_imgs, l_imgs))
    # a varying schedule with a negative prompt: the chain of steps, each with its own scale
    ctx = pipe.text_model(texts)
    neg = pipe.text_model(["n", "m", "o"])[1:, :LN].contiguous()         # rows of another prompt index: not the context's
    scales = [0.25, 2.0, -0.5, 3.0]
    opts = pipe._options(3, None, scales, None, None, ctx, 2, neg, [2, 3], T)
    assert opts.guidance_scale is None and opts.guidance_scales == scales and opts.negative_lens == [2, 3]
    imgs, ids = pipe._generate_cpu(ctx, 2, T, 1.0, opts, 1, seed, True)
    temps, nmask, _ = loop_schedule(T, 1.0, pipe.num_tokens)
    chain = torch.full((2, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long)
    for step in range(T):
        chain, img = pipe._sample_cpu(chain, nmask[step], ctx, 3, temps[step], None, seed + step, scales[step], None, 0.0, None, 1.0, neg, [2, 3])
        assert torch.equal(img, imgs[step]), step
    assert torch.equal(chain, ids)
    other = pipe._generate_cpu(ctx, 2, T, 1.0, opts._replace(guidance_scales=[3.0] * T), 1, seed, True)[1]
    assert not torch.equal(other, ids)                                   # the scales are read, step by step
    # Pipeline.generate: one negative string for every image or a list of B; mask_padding brings its lengths too
    a = pipe.generate(texts, guidance_scale=scales, negative_text="blurry", mask_padding=True, **kw)[1]
    b = pipe.generate(texts, guidance_scale=scales, negative_text=["blurry", "blurry"], **kw)[1]
    assert torch.equal(a, b)
    # lanes slice the negative context and its lengths with the rest
    lane = opts.lane(1, 2)
    assert torch.equal(lane.negative, neg[1:2]) and lane.negative_lens == [3] and lane.guidance_scales == scales
    assert opts._replace(negative=None, negative_lens=None).lane(0, 1).negative is None


def stub_engine(lib, monkeypatch):
    """an S2Engine over `lib` instead of the native library: no handle, no device (tests/test_step0_cpu.py)"""
    e = object.__new__(engine_mod.S2Engine)
    e.__dict__.update(lib=lib, handle=None, device=torch.device("cpu"), tokens=16, n_embed=64, context_dim=8)
    monkeypatch.setattr(engine_mod, "stream_ptr", lambda device: None)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    return e


def test_engine_methods_route_to_the_negative_entry_only_with_the_new_options(monkeypatch):
    calls = []

    class Lib:
        def __getattr__(self, name):
            def entry(*args):
                calls.append((name, args))
                return 0
            return entry

    def only_call(name, n_args):
        assert len(calls) == 1 and calls[0][0] == name and len(calls[0][1]) == n_args, [(c[0], len(c[1])) for c in calls]
        return calls.pop()[1]

    def null(arg):
        return getattr(arg, "value", arg) is None

    def plain_values(args):                                              # pointers by address, host arrays by content
        return [list(x) if isinstance(x, C.Array) else getattr(x, "value", x) for x in args]

    e = stub_engine(Lib(), monkeypatch)
    B, N = 2, 16
    ids, ctx, neg = torch.zeros(B, N, dtype=torch.long), torch.zeros(B, L, 8), torch.ones(B, LN, 8)
    # without the new options: the entries and argument counts as before
    e.sample(None, ids, ctx, 5, 0.7, 4, seed=9, want_img=False, guidance_scale=2.5)
    plain = only_call("pmhip_pipeline_sample_nucleus", 23)
    e.generate(None, ids, ctx, [1.0, 0.6, 0.3], [8, 4, 1], [False] * 3, 5, seed=9, guidance_scale=2.5)
    plain_gen = only_call("pmhip_pipeline_generate_nucleus", 24)
    for nl in (None, [1, 3]):
        e.sample(None, ids, ctx, 5, 0.7, 4, seed=9, want_img=False, guidance_scale=2.5, negative_context=neg, negative_lens=nl)
        a = only_call("pmhip_pipeline_sample_negative", 26)
        assert plain_values(a[:22]) == plain_values(plain[:22])     # the nucleus entry's list, then:
        assert a[22].value is not None and a[23] == LN and (null(a[24]) if nl is None else list(a[24]) == nl) and a[25] is None
        assert (a[17], a[18]) == (1, 2.5)
    for with_neg, nl, sched in itertools.product((False, True), (None, [1, 3]), (None, [0.5, 1.0, 1.5])):
        if not with_neg and nl is not None:
            continue
        if not with_neg and sched is None:
            continue
        e.generate(None, ids, ctx, [1.0, 0.6, 0.3], [8, 4, 1], [False] * 3, 5, seed=9, guidance_scale=None if sched else 2.5,
                   negative_context=neg if with_neg else None, negative_lens=nl, guidance_scales=sched)
        a = only_call("pmhip_pipeline_generate_negative", 28)
        case = (with_neg, nl, sched)
        assert plain_values(a[:20]) == plain_values(plain_gen[:20]), case
        assert a[20] == 1 and a[21] == (0.0 if sched else 2.5) and null(a[22]) and a[23] == 1.0, case
        assert (a[24].value is not None and a[25] == LN) if with_neg else (null(a[24]) and a[25] == 0), case
        assert (null(a[26]) if nl is None else list(a[26]) == nl), case
        assert (null(a[27]) if sched is None else list(a[27]) == sched), case
    # checked before the native call: lengths without a negative, a schedule of the wrong length, a non-finite scale
    with pytest.raises(ValueError, match="negative_lens"):
        e.sample(None, ids, ctx, 5, 0.7, 4, want_img=False, guidance_scale=2.5, negative_lens=[1, 1])
    with pytest.raises(ValueError, match="2 scales for 3 steps"):
        e.generate(None, ids, ctx, [1.0, 0.6, 0.3], [8, 4, 1], [False] * 3, 5, guidance_scales=[1.0, 2.0])
    with pytest.raises(ValueError, match="step 1"):
        e.generate(None, ids, ctx, [1.0, 0.6, 0.3], [8, 4, 1], [False] * 3, 5, guidance_scales=[1.0, float("inf"), 2.0])
    assert calls == []


def test_value_errors_where_the_options_are_checked(pipe, monkeypatch):
    """raised where Pipeline._options raises, before anything runs: no step is reached"""
    monkeypatch.setattr(Pipeline, "_sample_cpu", lambda *a, **k: pytest.fail("a step ran"))
    texts, T = ["a", "b"], 3
    ctx = pipe.text_model(texts)
    neg = pipe.text_model(["c", "d"])[:, :LN].contiguous()
    ids = torch.full((2, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long)
    inf, nan = float("inf"), float("nan")
    step = lambda **kw: pipe.sample(ids, 0.5, **{"text": ctx, **kw})
    loop = lambda **kw: pipe.generate(texts, timesteps=T, **kw)
    loop_ids = lambda **kw: pipe.generate_ids(ctx, 2, T, 1.0, 3, [True] * T, 1, **kw)
    for call, kw, word in (
            # negative without guidance_scale
            (step, dict(negative_text=neg), "needs guidance_scale"),
            (loop, dict(negative_text="blurry"), "needs guidance_scale"),
            (loop_ids, dict(negative_context=neg), "needs guidance_scale"),
            # negative or guidance without a text condition
            (step, dict(text=None, negative_text=neg, guidance_scale=2.0), "text condition"),
            (step, dict(text=None, guidance_scale=2.0), "text condition"),
            # a scale sequence of the wrong length or with a non-finite entry
            (loop, dict(guidance_scale=[1.0, 2.0]), "2 scales for 3 steps"),
            (loop, dict(guidance_scale=[1.0, nan, 2.0]), "step 1"),
            (loop, dict(guidance_scale=(1.0, 2.0, inf)), "step 2"),
            (loop_ids, dict(guidance_scale=torch.tensor([1.0, 2.0, 3.0, 4.0])), "4 scales for 3 steps"),
            (step, dict(guidance_scale=[1.0, 2.0]), "one step takes one scale"),
            # negative lengths without a negative, and lengths out of range
            (step, dict(guidance_scale=2.0, negative_context_lens=[1, 1]), "needs a negative text"),
            (loop, dict(guidance_scale=2.0, negative_context_lens=[1, 1]), "needs a negative text"),
            (step, dict(guidance_scale=2.0, negative_text=neg, negative_context_lens=[1, LN + 1]), "image 1"),
            (step, dict(guidance_scale=2.0, negative_text=neg[:1]), "must be a context tensor"),
            (loop, dict(guidance_scale=2.0, negative_text=["x"]), "1 prompts for a batch of 2")):
        with pytest.raises(ValueError, match=word):
            call(**kw)


def test_native_entries_refuse_bad_arguments_before_a_launch():
    """NULL handles where the check comes first, fake non-null pointers where a context has to be named: a call that got past the
    checks would not return PMHIP_EINVAL with these messages"""
    lib = _lib.load()
    p = C.c_void_p(64)
    arr = lambda *v: (C.c_int * len(v))(*v)
    fl = lambda *v: (C.c_float * len(v))(*v)
    T2 = (fl(1.0, 0.5), arr(8, 1), (C.c_ubyte * 2)(0, 0))

    def sample(context, Lc, guided, neg, Ln, nl):
        return lib.pmhip_pipeline_sample_negative(None, None, None, context, Lc, 3, None, 3, 1.0, 4, None, 1, 0, 0, None, None, None, guided, 2.0,
                                                  0.0, None, 1.0, neg, Ln, nl, None)

    def generate(context, Lc, guided, neg, Ln, nl, gs, T=2):
        return lib.pmhip_pipeline_generate_negative(None, None, None, context, Lc, 3, None, T, *T2, 3, 1, 0, None, 0, None, None, 0, None, guided,
                                                    2.0, None, 1.0, neg, Ln, nl, gs)

    def refused(rc, who, *words):
        msg = lib.pmhip_last_error().decode()
        assert rc == _lib.PMHIP_EINVAL and who in msg and all(w in msg for w in words), (rc, msg)

    for who, call in (("pipeline_sample_negative", sample), ("pipeline_generate_negative", lambda *a: generate(*a, None))):
        refused(call(p, L, 0, p, LN, None), who, "needs guidance")                     # a negative context without guidance
        refused(call(None, 0, 1, p, LN, None), who, "a context")                       # ... without a context
        refused(call(p, L, 1, p, 0, None), who, "Ln=0")
        refused(call(p, L, 1, p, LN, arr(1, 0, 2)), who, "image 1", "Ln=3")
        refused(call(p, L, 1, p, LN, arr(1, 2, LN + 1)), who, "image 2", str(LN + 1))
        refused(call(p, L, 1, None, 0, arr(1, 1, 1)), who, "without a negative context")
    who = "pipeline_generate_negative"
    refused(generate(p, L, 0, None, 0, None, fl(1.0, 2.0)), who, "needs guidance")     # a schedule without guidance
    refused(generate(None, 0, 1, None, 0, None, fl(1.0, 2.0)), who, "a context")
    refused(generate(p, L, 1, None, 0, None, fl(1.0, float("inf"))), who, "step 1", "finite")
    refused(generate(p, L, 1, p, LN, None, fl(float("nan"), 1.0)), who, "step 0", "finite")
    # without the new arguments the entries are the nucleus entries: their refusals, their texts
    assert sample(None, 0, 0, None, 0, None) == _lib.PMHIP_EINVAL
    neg_msg = lib.pmhip_last_error()
    assert lib.pmhip_pipeline_sample_nucleus(None, None, None, None, 0, 3, None, 3, 1.0, 4, None, 1, 0, 0, None, None, None, 0, 2.0, 0.0, None, 1.0,
                                             None) == _lib.PMHIP_EINVAL
    assert lib.pmhip_last_error() == neg_msg
    assert generate(None, 0, 0, None, 0, None, None) == _lib.PMHIP_EINVAL
    neg_msg = lib.pmhip_last_error()
    assert lib.pmhip_pipeline_generate_nucleus(None, None, None, None, 0, 3, None, 2, *T2, 3, 1, 0, None, 0, None, None, 0, None, 0, 2.0, None,
                                               1.0) == _lib.PMHIP_EINVAL
    assert lib.pmhip_last_error() == neg_msg
    # the operator: the scalar entry's shape rules and NULL refusals, and its own scale pointer
    assert lib.pmhip_guidance_combine_dev(p, p, None, p, 64, None, None) == _lib.PMHIP_EINVAL and b"scale" in lib.pmhip_last_error()
    assert lib.pmhip_guidance_combine_dev(None, p, p, p, 64, None, None) == _lib.PMHIP_EINVAL and b"null pointer" in lib.pmhip_last_error()
    assert lib.pmhip_guidance_combine_dev(p, p, p, p, 6, None, None) == _lib.PMHIP_EINVAL and b"multiple of 4" in lib.pmhip_last_error()
    assert lib.pmhip_guidance_combine_dev(p, p, p, p, 32, p, None) == _lib.PMHIP_EINVAL and b"multiple of 64" in lib.pmhip_last_error()


def test_keywords_exist_with_default_none():
    import inspect
    for fn, names in ((Pipeline.sample, ("negative_text", "negative_context_lens")), (Pipeline.generate, ("negative_text", "negative_context_lens")),
                      (Pipeline.generate_ids, ("negative_context", "negative_lens")),
                      (engine_mod.S2Engine.sample, ("negative_context", "negative_lens")),
                      (engine_mod.S2Engine.generate, ("negative_context", "negative_lens", "guidance_scales"))):
        sig = inspect.signature(fn).parameters
        assert all(sig[n].default is None for n in names), fn
    assert callable(ops.guidance_combine_dev)
    for fn in (Pipeline.inpaint, Pipeline.outpaint):                     # no guidance there, so no negative prompt either
        assert "negative_text" not in inspect.signature(fn).parameters
