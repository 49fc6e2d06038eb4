"""The nucleus (top-p) filter without a GPU: the float64 restatement of tests/nucleus_ref.py against an
independent one and against hand-made rows, the plain-torch branch of the pipeline against it, the validation at every layer
(Python and, through the built library with pointers that are never dereferenced, the C ABI), and None / 1.0 leaving every
existing call as it was."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import nucleus_ref as R
import paintmind_amd as pm
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline, nucleus_keep, num_token_masked
from util import load_golden, to_torch_sd

F = np.float32


@pytest.fixture(scope="module")
def tiny():
    p, d = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False).eval()
    pipe.load_state_dict(to_torch_sd(p), strict=False)
    return pipe, d


# ------------------------------------------------------------------------------------------------------------------------------
# the restatement itself
# ------------------------------------------------------------------------------------------------------------------------------
def _untied(logits):
    """the same rows with every repeated value moved up by single fp32 steps until no two elements of a row are equal"""
    for row in logits:
        while True:
            first = np.unique(row, return_index=True)[1]
            if len(first) == len(row):
                break
            again = np.setdiff1d(np.arange(len(row)), first)
            row[again] = np.nextafter(row[again], F(np.inf))
    return logits


@pytest.mark.parametrize("scale", [0.5, 3.0, 20.0])
@pytest.mark.parametrize("V", [256, 8192])
def test_restatement_against_sort_and_cumsum(V, scale):
    """rows without ties; and what the issue's derivation of the band claims about such rows: MAY \\ MUST holds at most 3
    elements, MUST is never empty, and the filter changes the winner in 1..99 % of the rows"""
    rng = np.random.default_rng(int(V + 10 * scale))
    M = 200
    logits = _untied((rng.standard_normal((M, V)) * scale).astype(F))
    noise = rng.random((M, V)).astype(F)
    ids = np.full(M, V, np.int64)
    for p in (0.1, 0.5, 0.9):
        for topk in (V, V // 4):
            kept, must, may, order = R.sets(logits, topk, p)
            assert np.array_equal(kept, R.torch_restatement(logits, topk, p)), (p, topk)
            assert not (must & ~kept).any() and not (kept & ~may).any()
            assert (may & ~must).sum(1).max() <= 3 and must.sum(1).min() >= 1
            assert kept[np.arange(M), logits.argmax(1)].all()
            assert not kept[np.arange(M), order[:, -1]].all()
        changed = (R.sample_rows(logits, ids, V, V, p, 1.0, noise)[0] != R.sample_masked(logits, ids, V, np.ones_like(kept), 1.0, noise)[0]).mean()
        assert 0.01 <= changed <= 0.99, (p, changed)


def hand_row():
    """masses 0.4 / 0.2 / 0.1 / 0.1 (a tie) / 0.08 / 0.06 / 0.04 / 0.02 at shuffled columns, exact enough in fp32 logits that
    every cut below sits 0.01 away from a step"""
    mass = np.array([0.4, 0.2, 0.1, 0.1, 0.08, 0.06, 0.04, 0.02])
    cols = np.array([5, 2, 7, 1, 0, 6, 3, 4])                   # the tie sits at columns 7 and 1
    row = np.zeros(8, F)
    row[cols] = np.log(mass).astype(F)
    return row[None, :], cols


def test_hand_made_row_on_both_sides_of_every_step():
    logits, cols = hand_row()
    # mass strictly above: 0, .4, .6, .6 (the plateau), .8, .88, .94, .98 -> kept count by top_p
    for p, count in ((0.39, 1), (0.41, 2), (0.59, 2), (0.61, 4), (0.79, 4), (0.81, 5), (0.87, 5), (0.89, 6), (0.93, 6), (0.95, 7),
                     (0.97, 7), (0.99, 8), (1e-3, 1)):
        kept, must, may, _ = R.sets(logits, 8, p)
        assert np.array_equal(np.flatnonzero(kept[0]), np.sort(cols[:count])), (p, count)
        assert np.array_equal(kept, must) and np.array_equal(kept, may)
        assert np.array_equal(nucleus_keep(torch.from_numpy(logits).topk(8).values, float(F(p))).numpy()[0], np.arange(8) < count), p
    # the plateau whole or not at all: no top_p keeps exactly three elements
    assert all(R.sets(logits, 8, p)[0].sum() != 3 for p in np.linspace(0.55, 0.65, 41))
    # top-k first: with topk = 3 the mass is 0.7 and the tie is cut by COLUMN (column 1 before column 7); then the weight rule
    kept = R.sets(logits, 3, 0.9)[0]                           # P = 0.63: mass above the third element 0.6 < 0.63
    assert np.array_equal(np.flatnonzero(kept[0]), [1, 2, 5])
    kept = R.sets(logits, 3, 0.8)[0]                           # P = 0.56 < 0.6
    assert np.array_equal(np.flatnonzero(kept[0]), [2, 5])


def test_a_tiny_top_p_keeps_one_element_and_zero_weights_never_stay():
    rng = np.random.default_rng(5)
    logits = (rng.standard_normal((50, 260)) * 3).astype(F)
    kept = R.sets(logits, 260, 1e-3)[0]
    assert (kept.sum(1) == 1).all() and kept[np.arange(50), logits.argmax(1)].all()
    logits[:, 100:] = -np.inf                                   # weight 0: never kept below top_p = 1, however close to it
    kept = R.sets(logits, 260, 1 - 2.0 ** -20)[0]
    assert not kept[:, 100:].any() and kept[:, :100].sum(1).min() >= 50
    assert not nucleus_keep(torch.from_numpy(logits).topk(260).values, float(F(1 - 2.0 ** -20)))[:, 100:].any()


# ------------------------------------------------------------------------------------------------------------------------------
# the plain-torch branch of the pipeline
# ------------------------------------------------------------------------------------------------------------------------------
def test_none_and_one_leave_the_cpu_branch_unchanged(tiny):
    pipe, d = tiny
    ids0, ctx, noise = torch.from_numpy(d["ids0"]), torch.from_numpy(d["context"]), torch.from_numpy(d["s5_ctx_noise"])
    for kw in ({}, {"top_p": None}, {"top_p": 1.0}, {"top_p": 1}):
        ids5, img5 = pipe.sample(ids0, np.float64(0.5), text=ctx, topk=5, temperature=0.7, noise=noise, **kw)
        assert np.array_equal(ids5.numpy(), d["s5_ctx_ids"]), kw           # the parent's result, recorded
        assert np.allclose(img5.numpy(), d["s5_ctx_img"], atol=1e-4), kw
    a, ia = pipe.generate(["a", "b"], timesteps=6, topk=5, save_interval=2, seed=5, return_ids=True)
    for p in (None, 1.0):
        b, ib = pipe.generate(["a", "b"], timesteps=6, topk=5, save_interval=2, seed=5, return_ids=True, top_p=p)
        assert torch.equal(ia, ib) and all(torch.equal(x, y) for x, y in zip(a, b))
        b, ib = pipe.generate(["a", "b"], timesteps=4, topk=None, save_interval=2, seed=5, return_ids=True, guidance_scale=2.0, top_p=p)
        c, ic = pipe.generate(["a", "b"], timesteps=4, topk=None, save_interval=2, seed=5, return_ids=True, guidance_scale=2.0)
        assert torch.equal(ic, ib) and all(torch.equal(x, y) for x, y in zip(b, c))
    img = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(2)) * 2 - 1
    coord = (pipe.patch_size, pipe.patch_size, 2 * pipe.patch_size, 2 * pipe.patch_size)
    for timesteps in (1, 3):
        a, ia = pipe.inpaint(img, coord, timesteps=timesteps, topk=4, temperature=1.0, seed=3, return_ids=True)
        b, ib = pipe.inpaint(img, coord, timesteps=timesteps, topk=4, temperature=1.0, seed=3, return_ids=True, top_p=1.0)
        assert torch.equal(ia, ib) and torch.equal(a, b)


@pytest.mark.parametrize("topk", [5, 40, None])
def test_sample_cpu_equals_the_restatement_composed_with_the_step(tiny, topk):
    """top_p = 0.5: the kept set is the restatement's (no element of these rows lies in the band), and the step behind it is the
    existing CPU step -- draw among the kept, confidence from the unfiltered softmax, the same re-masking"""
    pipe, d = tiny
    ids0, ctx, noise = torch.from_numpy(d["ids0"]), torch.from_numpy(d["context"]), torch.from_numpy(d["s5_ctx_noise"])
    B, N = ids0.shape
    V = pipe.mask_token_id
    k = V if topk is None else topk
    logits = pipe.tokens2logits(pipe.ids2tokens(ids0), ctx).detach()
    flat = logits.reshape(B * N, V).numpy()
    kept, must, may, _ = R.sets(flat, k, 0.5)
    assert np.array_equal(must, may)                            # a property of the inputs: nothing is left to rounding
    assert kept.sum() < min(k, V) * B * N                       # ... and the filter does cut
    filtered = torch.where(torch.from_numpy(kept).reshape(B, N, V), logits, torch.full_like(logits, float("-inf")))
    gumbel = -torch.log((-torch.log(noise.clamp(min=1e-20))).clamp(min=1e-20))
    pred = (filtered / 0.7 + gumbel).argmax(dim=-1)
    is_mask = ids0 == V
    scores = (1 - logits.softmax(dim=-1).gather(2, pred[..., None])[..., 0]).masked_fill(~is_mask, -1e5)
    nm = num_token_masked(np.float64(0.5), N)
    want = torch.where(is_mask, pred, ids0).scatter(1, scores.topk(nm, dim=-1).indices, V)
    got, img = pipe.sample(ids0, np.float64(0.5), text=ctx, topk=topk, temperature=0.7, noise=noise, top_p=0.5)
    assert torch.equal(got, want)
    assert torch.equal(img, pipe.vqgan.decode_from_indice(pred))
    plain, _ = pipe.sample(ids0, np.float64(0.5), text=ctx, topk=topk, temperature=0.7, noise=noise)
    if topk is None:
        assert not torch.equal(plain, got)                      # (the filter does matter on these logits)


def test_generate_ids_and_inpaint_on_the_cpu_follow_the_step(tiny):
    """the CPU loops hand top_p to every step: a loop equals the steps it is made of"""
    pipe, _ = tiny
    T, V = 4, pipe.mask_token_id
    a, ia = pipe.generate(["a", "b"], timesteps=T, topk=None, save_interval=2, seed=5, return_ids=True, top_p=0.3)
    a2, ia2 = pipe.generate(["a", "b"], timesteps=T, topk=None, save_interval=2, seed=5, return_ids=True, top_p=0.3)
    plain, ip = pipe.generate(["a", "b"], timesteps=T, topk=None, save_interval=2, seed=5, return_ids=True)
    assert torch.equal(ia, ia2) and not torch.equal(ia, ip) and len(a) == len(plain) == 2
    ctx = pipe.text_model(["a", "b"])
    ids = torch.full((2, pipe.num_tokens), V, dtype=torch.long)
    temps, nmask = pipe._schedule(T, 1.0)
    for step in range(T):
        ids, _ = pipe._sample_cpu(ids, nmask[step], ctx, V, temps[step], None, 5 + step, top_p=0.3)
    assert torch.equal(ids, ia)
    g, ig = pipe.generate(["a", "b"], timesteps=T, topk=None, save_interval=2, seed=5, return_ids=True, top_p=0.3, guidance_scale=2.0)
    assert not torch.equal(ig, pipe.generate(["a", "b"], timesteps=T, topk=None, save_interval=2, seed=5, return_ids=True, guidance_scale=2.0)[1])
    img = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(2)) * 2 - 1
    coord = (pipe.patch_size, pipe.patch_size, 2 * pipe.patch_size, 2 * pipe.patch_size)
    for fn in (pipe.inpaint, pipe.outpaint):
        for timesteps in (1, 3):
            x, ix = fn(img, coord, timesteps=timesteps, topk=None, temperature=1.0, seed=3, return_ids=True, top_p=1e-3)
            y, iy = fn(img, coord, timesteps=timesteps, topk=1, temperature=1.0, seed=3, return_ids=True)
            assert torch.equal(ix, iy) and torch.equal(x, y)   # one kept element: the arg-max, whatever the noise


# ------------------------------------------------------------------------------------------------------------------------------
# validation
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, 0.0, -0.1, 1.5, float("nan"), float("inf")])
def test_python_validation_before_anything_runs(tiny, bad, monkeypatch):
    pipe, d = tiny
    ids0 = torch.from_numpy(d["ids0"])

    def never(*a, **k):
        raise AssertionError("the model ran before the range check")
    monkeypatch.setattr(pipe, "tokens2logits", never)
    monkeypatch.setattr(pipe, "to_latent", never)
    monkeypatch.setattr(pipe, "engine", never)
    with pytest.raises(ValueError, match="top_p"):
        ops.nucleus_p(bad)
    with pytest.raises(ValueError, match="top_p"):
        ops.sample_rows(torch.zeros(2, 64), torch.zeros(2, dtype=torch.long), 64, 5, 1.0, top_p=bad)
    with pytest.raises(ValueError, match="top_p"):
        pipe.sample(ids0, 0.5, top_p=bad)
    with pytest.raises(ValueError, match="top_p"):
        pipe.generate(["a"], timesteps=2, top_p=bad)
    with pytest.raises(ValueError, match="top_p"):
        pipe.generate_ids(None, 1, 2, 1.0, 5, [False, False], 1, top_p=bad)
    for fn in (pipe.inpaint, pipe.outpaint):
        with pytest.raises(ValueError, match="top_p"):
            fn(torch.zeros(1, 3, 32, 32), (0, 0, 16, 16), top_p=bad)
    monkeypatch.setattr(pipe, "_on_cpu", lambda: False)         # the GPU branch checks at the same place
    with pytest.raises(ValueError, match="top_p"):
        pipe.sample(ids0, 0.5, top_p=bad)
    with pytest.raises(ValueError, match="top_p"):
        pipe.generate(["a"], timesteps=2, top_p=bad)


def test_native_entries_refuse_bad_arguments_before_a_launch():
    lib = _lib.load()
    for what, rc in R.bad_argument_calls(lib, C.c_void_p(256)):
        assert rc == _lib.PMHIP_EINVAL, (what, rc, lib.pmhip_last_error())
    # a valid top_p passes its check and is refused by the next one
    assert lib.pmhip_sample_rows_nucleus(None, 64, None, 64, 5, 0.5, 1.0, None, 1, 0, 0, None, None, None, 4, 64, None) == _lib.PMHIP_EINVAL
    assert b"null" in lib.pmhip_last_error()
    # top_p == 1 through the pipeline entries is the _choice entry, with its messages
    assert lib.pmhip_pipeline_sample_nucleus(None, None, None, None, 0, 2, None, 3, 1.0, 4, None, 1, 0, 0, None, None, None, 0, 0.0, 0.0, None, 1.0,
                                             None) == _lib.PMHIP_EINVAL
    assert b"pipeline_sample_lens" in lib.pmhip_last_error()


class _StepSource(C.Structure):
    """mirror of PmStepSource (paintmind_amd/csrc/common.h), the argument of the library's one sampling launcher"""
    _fields_ = [("kind", C.c_int), ("topk", C.c_int), ("temperature", C.c_float), ("num_mask", C.c_int), ("seed", C.c_uint64),
                ("step", C.c_uint32), ("row_base", C.c_uint64), ("gp", C.c_void_p), ("slots", C.c_void_p), ("tokens", C.c_int),
                ("choice_t", C.c_float), ("choice_noise", C.c_void_p), ("choice_dev", C.c_void_p), ("choice_params", C.c_bool),
                ("top_p", C.c_float)]


def test_a_slots_source_with_a_nucleus_is_refused():
    """no C entry can say it (pmhip_sample_rows_slots has no top_p), so the launcher itself is asked, by its C++ name"""
    lib = _lib.load()
    fn = getattr(lib, "_Z14pm_sample_rowsPKfiS0_iPKllS0_PlS3_PfiiRK12PmStepSourcePv")
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                   C.c_int, C.POINTER(_StepSource), C.c_void_p]
    p = C.c_void_p(256)
    BATCH, SLOTS = 0, 2

    def src(kind, top_p, topk=5):
        return _StepSource(kind=kind, topk=topk, temperature=1.0, slots=256 if kind == SLOTS else None, tokens=4, top_p=top_p)
    assert fn(p, 64, None, 0, p, 64, None, p, p, p, 8, 64, C.byref(src(SLOTS, 0.5)), None) == _lib.PMHIP_EINVAL
    assert b"top_p" in lib.pmhip_last_error() and b"slots" in lib.pmhip_last_error()
    # the layout of the mirror is the library's: the same call is refused for its top_p VALUE when that is out of range, and a
    # batch source for its top-k, which sits at the other end of the record
    assert fn(p, 64, None, 0, p, 64, None, p, p, p, 8, 64, C.byref(src(SLOTS, 1.5)), None) == _lib.PMHIP_EINVAL
    assert b"(0, 1]" in lib.pmhip_last_error()
    assert fn(p, 64, None, 0, p, 64, None, p, p, p, 8, 64, C.byref(src(BATCH, 0.5, topk=65)), None) == _lib.PMHIP_EINVAL
    assert b"topk=65" in lib.pmhip_last_error()


def test_keywords_exist_with_default_none():
    from paintmind_amd.engine import S2Engine
    from paintmind_amd.serve import DecodeSession
    for fn in (ops.sample_rows, S2Engine.sample, S2Engine.generate, Pipeline.sample, Pipeline.generate, Pipeline.generate_ids,
               Pipeline.inpaint, Pipeline.outpaint):
        assert inspect.signature(fn).parameters["top_p"].default is None, fn.__qualname__
    assert "top_p" not in inspect.signature(DecodeSession.submit).parameters
    assert C.sizeof(_lib.Slot) == 32
    assert _lib.ABI_VERSION == 11
    for name in ("pmhip_sample_rows_nucleus", "pmhip_pipeline_sample_nucleus", "pmhip_pipeline_generate_nucleus"):
        assert name in _lib.PROTOTYPES
    assert "(0, 1]" in ops.sample_rows.__doc__ or "0 < top_p" in ops.sample_rows.__doc__
