"""Cross-attention maps at the model level (pmhip_s2_forward_maps, ``S2Engine.forward_maps``, ``Pipeline.attention_maps``; DESIGN.md
section 4y) on the tiny pipeline, B = 3, ids from seed 11, context lengths 77 / 50 / 33 -- the recipe of tests/test_gpu_weights.py.
Forms: lengths, two regions, weights (beside the lengths), NaN in every context row that may reach nothing.

The logits are those of the existing forward, bit for bit, and a forward behind a forward_maps runs what it ran before; the maps are
held to the plain-torch branch of the same model at the project's float bar in fp32-verify (bf16 printed), with counter-checks that
give the bar teeth; rows that take no part are exactly 0; the engine validates before it launches."""
import ctypes as C

import numpy as np
import pytest
import torch

import paintmind_amd as pm
import region_ref as R
from gpu_common import dev
from paintmind_amd import _lib
from paintmind_amd.generate import Pipeline
from util import load_golden, to_torch_sd

pytestmark = pytest.mark.gpu

TOL = 1e-3                      # the project's float bar (tests/test_gpu_context_lens.py)
B = 3
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
FORMS = pytest.mark.parametrize("form", ["lens", "regions", "weights"])


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


def _case(pipe, form):
    """-> dict(ctx with NaN where a row may reach nothing, finite: zeros there, kw: the keywords of the form, plain_kw: the same
    without the weights, dead bool [B, L]: the rows that take part in no softmax)"""
    rows = pipe.text_model(["a", "b", "c", "d", "e", "f"]).cpu()
    if form in ("lens", "weights"):
        lens = [77, 50, 33]
        context = rows[:B].clone()
        ks = np.where(np.arange(77)[None, :] < np.asarray(lens)[:, None], 0, R.PAD).astype(np.uint8)
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
    plain_kw = dict(kw)
    dead = ks == R.PAD
    if form == "weights":
        w = np.random.default_rng(1).choice(np.array([0, 0.125, 1, 8, 1.3, 0.5], np.float32), size=ks.shape).astype(np.float32)
        w[:, 0] = 8                                                    # every image keeps a row that counts
        kw["context_weights"] = w
        dead = dead | (w == 0)
    dead = torch.from_numpy(dead)
    ctx, finite = context.clone(), context.clone()
    ctx[dead] = float("nan")
    finite[dead] = 0.0
    return dict(ctx=ctx, finite=finite, kw=kw, plain_kw=plain_kw, dead=dead)


@pytest.fixture(scope="module")
def data(tiny_pipe):
    pipe = tiny_pipe
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, pipe.mask_token_id, (B, pipe.num_tokens), generator=g)
    ids[torch.rand(B, pipe.num_tokens, generator=g) < 0.5] = pipe.mask_token_id
    out = dict(ids=ids.to(dev()), lens=_case(pipe, "lens"), regions=_case(pipe, "regions"), weights=_case(pipe, "weights"))
    out["tok"] = pipe.ids2tokens(out["ids"])
    return out


@pytest.fixture(scope="module")
def cpu_maps(cpu_pipe, data):
    """the plain-torch branch's maps, computed once per (form, layers) and shared (never modified)"""
    cache = {}

    def get(form, layers):
        key = (form, None if layers is None else tuple(layers))
        if key not in cache:
            c = data[form]
            with torch.no_grad():
                cache[key] = cpu_pipe.attention_maps(data["ids"].cpu(), c["ctx"], layers=layers, **c["kw"])
        return cache[key]
    return get


class in_dtype:
    def __init__(self, pipe, dtype):
        self.pipe, self.dtype = pipe, dtype

    def __enter__(self):
        self.pipe.set_compute_dtype(self.dtype)

    def __exit__(self, *exc):
        self.pipe.set_compute_dtype(torch.float32)


@FORMS
@DTYPES
def test_the_logits_are_those_of_forward_and_a_later_forward_is_unchanged(tiny_pipe, data, form, dtype):
    c = data[form]
    ctx = c["ctx"].to(dev())
    with in_dtype(tiny_pipe, dtype):
        eng = tiny_pipe.engine()
        count = eng.graph_count()
        first = eng.forward(data["tok"], ctx, **c["kw"])
        for layers in ([0], [1], [0, 1]):
            logits, maps = eng.forward_maps(data["tok"], ctx, layers, **c["kw"])
            assert torch.equal(logits, first), (form, layers)
            assert maps.shape == (B, tiny_pipe.num_tokens, ctx.shape[1]) and maps.dtype == torch.float32 and torch.isfinite(maps).all()
        third = eng.forward(data["tok"], ctx, **c["kw"])
        assert torch.equal(first, third)
        assert eng.graph_count() == count                                 # eager only: no key added to the graph cache
        got, lg = tiny_pipe.attention_maps(data["ids"], ctx, return_logits=True, **c["kw"])
        assert torch.equal(lg, tiny_pipe.tokens2logits(data["tok"], ctx, **c["kw"]))


@FORMS
@DTYPES
def test_maps_against_the_cpu_branch_of_the_same_model(tiny_pipe, cpu_maps, data, form, dtype):
    """fp32-verify is gated at the project's float bar; the bf16 figures are printed, not gated.  Counter-checks: another layer, all
    layers against one, and (under weights) the call without the weights are all beyond the bar."""
    c = data[form]
    ctx = c["ctx"].to(dev())
    g = tiny_pipe.image_size // tiny_pipe.patch_size
    with in_dtype(tiny_pipe, dtype):
        got = {key: tiny_pipe.attention_maps(data["ids"], ctx, layers=key and list(key), **c["kw"]).cpu() for key in (None, (0,), (1,), (1, 0))}
        loose = tiny_pipe.attention_maps(data["ids"], c["finite"].to(dev()), **c["plain_kw"]).cpu() if form == "weights" else None
    for key, m in got.items():
        want = cpu_maps(form, key and list(key))
        assert m.shape == want.shape == (B, ctx.shape[1], g, g) and torch.isfinite(m).all()
        err = float((m - want).abs().max())
        print(f"{form} {dtype} layers={key}: max |maps GPU - maps CPU branch| = {err:.3e}")
        if dtype == torch.float32:
            assert err < TOL, (form, key, err)
        # rows behind a length, of segment 255 or of weight 0: exactly 0, with NaN in those context rows
        assert bool((m[c["dead"]] == 0).all()), (form, key)
        assert float((m.sum(1) - 1).abs().max()) < 1e-4                   # over the context a token's values sum to 1
    d01 = float((got[(0,)] - got[(1,)]).abs().max())
    dall = float((got[None] - got[(0,)]).abs().max())
    print(f"{form} {dtype}: |maps([0]) - maps([1])| = {d01:.3f}, |maps(all) - maps([0])| = {dall:.3f}")
    assert d01 > TOL and dall > TOL
    assert float((got[(1, 0)] - got[None]).abs().max()) < 1e-6            # the order of the layers does not matter beyond rounding
    if loose is not None:
        gap = float((loose - cpu_maps(form, None)).abs().max())
        print(f"{form} {dtype}: without the weights {gap:.3e}")
        assert gap > TOL


def test_the_engine_validates_before_it_launches(tiny_pipe, data):
    pipe, c = tiny_pipe, data["regions"]
    eng = pipe.engine()
    ctx = c["finite"].to(dev()).contiguous()
    L, N = ctx.shape[1], pipe.num_tokens
    sentinel = 12345.0
    logits = torch.full((B, N, eng.n_embed), sentinel, device=dev())
    maps = torch.full((B, N, L), sentinel, device=dev())
    u8p, u32p, f32p = C.POINTER(C.c_ubyte), C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    ks, qm = np.ascontiguousarray(c["kw"]["context_segments"]), np.ascontiguousarray(c["kw"]["token_segments"])
    count = eng.graph_count()

    def call(context=ctx, lens=None, seg=True, w=None, bits=1, out=maps):
        return eng.lib.pmhip_s2_forward_maps(eng.handle, data["tok"].data_ptr(), None if context is None else context.data_ptr(),
                                             L if context is not None else 0, B, None if lens is None else (C.c_int * B)(*lens),
                                             ks.ctypes.data_as(u8p) if seg else None, qm.ctypes.data_as(u32p) if seg else None,
                                             None if w is None else np.ascontiguousarray(w, np.float32).ctypes.data_as(f32p), bits,
                                             logits.data_ptr(), None if out is None else out.data_ptr(), None)

    for kwargs, text in ((dict(context=None, seg=False), b"a context is required"), (dict(bits=0), b"selects no layer"),
                         (dict(bits=4), b"at or above depth=2"), (dict(bits=(1 << 63)), b"at or above depth"),
                         (dict(out=None), b"maps_out is NULL"), (dict(lens=[L] * B), b"exclude each other"),
                         (dict(seg=False, lens=[0, 1, 1]), b"context length 0 must be in"),
                         (dict(w=np.full((B, L), 3e7)), b"[2^-20, 2^20]")):
        assert call(**kwargs) == _lib.PMHIP_EINVAL, kwargs
        msg = eng.lib.pmhip_last_error()
        assert b"s2_forward_maps" in msg and text in msg, (kwargs, msg)
    torch.cuda.synchronize()
    assert bool((logits == sentinel).all()) and bool((maps == sentinel).all())      # nothing was launched
    assert call() == _lib.PMHIP_OK and call(bits=3, w=np.ones((B, L))) == _lib.PMHIP_OK
    assert call(seg=False, lens=[L, 5, 1], w=np.ones((B, L))) == _lib.PMHIP_OK        # weights beside lengths: the neutral segments
    torch.cuda.synchronize()
    assert bool(torch.isfinite(maps).all()) and not bool((maps == sentinel).any()) and eng.graph_count() == count
    assert bool((maps[1, :, 5:] == 0).all()) and bool((maps[2, :, 1:] == 0).all()) and bool((maps[2, :, 0] == 1).all())
    with pytest.raises(ValueError, match="layers"):
        eng.forward_maps(data["tok"], ctx, [2])
    with pytest.raises(ValueError, match="context is required"):
        eng.forward_maps(data["tok"], None, [0])
    # the tap is cleared on the error path too: a forward behind a failed call equals one before it
    before = eng.forward(data["tok"], ctx, **c["kw"])
    assert call(bits=4) == _lib.PMHIP_EINVAL
    assert torch.equal(eng.forward(data["tok"], ctx, **c["kw"]), before)
