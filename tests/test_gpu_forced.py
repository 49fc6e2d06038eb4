"""The teacher-forced source pass on the GPU.

pmhip_sample_rows_forced at V in {64, 1000, 8192, 16384} -- the four NV4 classes of the row kernels; 1000 leaves the last register
group ragged -- M = 2 * (rows per workgroup) + 1 = 9, ldl = V + 8 with NaN in the padding, every buffer inside guard bands
(tests/abi_frames.py).  Inputs, float64 restatement and element-wise bound are those of tests/forced_ref.py;
tests/test_forced_cpu.py proves on the CPU that the bound rejects the named faults at exactly these inputs.  Then the bit contract
against the draw, the out-of-range targets (a test of the guard: nothing here is expected to fault), the argument checks, and the
loops and the surface on the tiny pipeline against their invariants and against the CPU branch."""
import math

import numpy as np
import pytest
import torch

import forced_ref as R
from abi_frames import call, framed
from gpu_common import dev, n, t
from paintmind_amd import _lib, ops
from paintmind_amd.generate import loop_schedule
from test_forced_cpu import (AUDIT_CAP, LOOP, LOOP_SEED, LOOP_T, LOOP_TOPK, SCORE_REL, check_reveal, check_source_half, loop_noise, source_tokens,
                             t5_pipe)
from test_gpu_control import LENS_EDIT, LENS_SRC, cpu_pipe, data, in_dtype, tiny_pipe      # noqa: F401
from test_local_blend_cpu import phrase_rows

pytestmark = pytest.mark.gpu
F32, I64 = torch.float32, torch.int64
PAIRS = 2
VS = pytest.mark.parametrize("V", R.VS)
_REF = {}


def ref(V, variant):
    """the case with its float64 reference and bound: computed once, shared, never modified"""
    if (V, variant) not in _REF:
        d = R.case(V, variant)
        d["want"] = R.reference(d["logits"], d["ids"], d["target"], V)[:3]
        d["B"] = R.bound(d["logits"], d["target"])
        for a in d["want"] + (d["B"],):
            a.setflags(write=False)
        _REF[(V, variant)] = d
    return _REF[(V, variant)]


def flat(x, dtype):
    return framed(len(x), 1, ld=1, dtype=dtype, payload=None if x is None else t(np.array(x)).reshape(-1, 1), device=dev())


def launch(logits, ids, target, mask_id, in_place=False, null=False):
    """the C entry on framed buffers -> (pred, merged, score) tensors [M] (None where the output was NULL); asserts the memory contract:
    nothing outside the [M] extents written, logits / target (and ids_in, unless in place) as they were"""
    M, V = logits.shape
    fx = framed(M, V, ld=V + 8, dtype=F32, payload=t(np.array(logits)), fill="nan")                          # NaN in the padding columns and around
    fi, ft = flat(ids, I64), flat(target, I64)
    fp, fs = (None, None) if null else (framed(M, 1, ld=1, dtype=I64, device=dev()), framed(M, 1, ld=1, dtype=F32, device=dev()))
    fo = fi if in_place else framed(M, 1, ld=1, dtype=I64, device=dev())
    call("pmhip_sample_rows_forced", fx, fx.ld, fi, ft, int(mask_id), fp, fo, fs, M, V)
    torch.cuda.synchronize()
    for f, what in ((fx, "logits"), (fi, "ids_in"), (ft, "target"), (fp, "pred_out"), (fo, "ids_out"), (fs, "score_out")):
        if f is not None:
            f.assert_frame_untouched(f"V={V} {what}")
    assert np.array_equal(n(fx.payload()), logits, equal_nan=True) and np.array_equal(n(ft.payload()).reshape(M), target)
    if not in_place:
        assert np.array_equal(n(fi.payload()).reshape(M), ids)
    return tuple(None if f is None else f.payload().reshape(M) for f in (fp, fo, fs))


# ------------------------------------------------------------------------------------------------------------- the operator

@VS
def test_the_operator_holds_the_bound(V):
    worst_all = 0.0
    for variant in (0, 1):
        d = ref(V, variant)
        got = launch(d["logits"], d["ids"], d["target"], V)
        fails, worst = R.check(tuple(n(x) for x in got), d["want"], d["B"])
        print(f"V={V} variant {variant}: worst err / bound {worst:.4f}")
        worst_all = max(worst_all, worst)
        assert not fails, fails
        assert np.array_equal(n(got[0]), d["target"])                             # pred = target
        # the operator of paintmind_amd.ops: the same bits
        via = ops.sample_rows_forced(t(np.array(d["logits"])), t(np.array(d["ids"])), t(np.array(d["target"])), V)
        assert all(torch.equal(a.view(torch.int32) if a.dtype == F32 else a, b.view(torch.int32) if b.dtype == F32 else b) for a, b in zip(via, got))
    print(f"V={V}: the forced kernel's worst err / bound {worst_all:.4f}")


@VS
def test_in_place_null_outputs_and_repeatable(V):
    d = ref(V, 0)
    a = launch(d["logits"], d["ids"], d["target"], V)
    b = launch(d["logits"], d["ids"], d["target"], V)
    same = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.dtype == F32 else torch.equal(x, y)
    assert all(same(x, y) for x, y in zip(a, b)), "two launches differ"
    pred, merged, score = launch(d["logits"], d["ids"], d["target"], V, in_place=True)
    assert same(pred, a[0]) and same(merged, a[1]) and same(score, a[2])
    none_p, merged, none_s = launch(d["logits"], d["ids"], d["target"], V, null=True)
    assert none_p is None and none_s is None and same(merged, a[1])
    _, merged, _ = launch(d["logits"], d["ids"], d["target"], V, in_place=True, null=True)
    assert same(merged, a[1])


# ------------------------------------------------------------------------------------------------------------- the bit contract

def draw_inputs(V, M=R.M, seed=0):
    """trained-like rows (a dominant class over a Gaussian floor, some nearly flat), about half the ids given"""
    rng = np.random.default_rng([V, 23, seed])
    x = rng.standard_normal((M, V)).astype(np.float32)
    x[::3] *= np.float32(0.05)
    x[np.arange(M), rng.integers(0, V, M)] += np.float32(6.0)
    ids = np.where(rng.uniform(size=M) < 0.5, rng.integers(0, V, M), V).astype(np.int64)
    return x, ids


def bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == F32 else x, y.view(torch.int32) if y.dtype == F32 else y) for x, y in zip(a, b))


@pytest.mark.parametrize("V,topk,top_p", [(8192, 9, None), (8192, 64, None), (8192, 65, None), (8192, 8192, None), (8192, 5, 0.9), (1000, 5, None),
                                          (16384, 9, None), (16384, 16384, None), (64, 9, None), (64, 64, None), (1000, 65, None), (1000, 5, 0.9)],
                         ids=lambda v: str(v))
def test_the_forced_triple_is_the_draws_triple_bit_for_bit(V, topk, top_p):
    """row kernel (8 < top-k <= 64, or V % 64 != 0), selection kernel (top-k > 64) and nucleus kernel (top_p < 1)"""
    x, ids = draw_inputs(V)
    X, I = t(x), t(ids)
    drawn = ops.sample_rows(X, I, V, topk, 0.9, seed=5, step=2, row_base=77, top_p=top_p)
    forced = ops.sample_rows_forced(X, I, drawn[0].clone(), V)
    assert bits_equal(forced, drawn), (V, topk, top_p, n(forced[2] - drawn[2]))
    taken = n(I) == V
    assert taken.any() and (~taken).any() and (n(drawn[2])[taken] >= 0).all()


@pytest.mark.parametrize("V", [8192, 64])
def test_against_the_block_statistics_draw_the_scores_agree_to_twice_the_bound(V):
    """top-k 5 with V % 64 == 0 runs on the block-statistics kernel, which rounds its confidence by another route: ids equal, scores
    within twice the element-wise bound of each other"""
    x, ids = draw_inputs(V)
    X, I = t(x), t(ids)
    pred, merged, score = ops.sample_rows(X, I, V, 5, 0.9, seed=5, step=2, row_base=77)
    f_pred, f_merged, f_score = ops.sample_rows_forced(X, I, pred.clone(), V)
    assert torch.equal(f_pred, pred) and torch.equal(f_merged, merged)
    B = R.bound(x, n(pred))
    taken = n(I) == V
    err = np.abs(n(f_score).astype(np.float64) - n(score).astype(np.float64))
    assert (n(f_score)[~taken] == R.GIVEN_SCORE).all() and (n(score)[~taken] == R.GIVEN_SCORE).all()
    ratio = float((err[taken] / (2 * B[taken])).max())
    print(f"V={V}: forced against the block-statistics draw: worst |difference| / (2 x bound) {ratio:.4f}")
    assert ratio < 1.0


# ------------------------------------------------------------------------------------------------------------- out-of-range targets

@VS
def test_a_target_outside_the_codebook_leaves_its_row_undrawn(V):
    """the guard in front of the load: -1, V, the mask id and 2^40, on masked and on given rows -> pred = merged = ids_in, score = -1e5;
    the rows between them are scored as ever; the frames stay intact and the call returns PMHIP_OK (``call`` raises otherwise)"""
    d = ref(V, 0)
    target = np.array(d["target"])
    ids = np.array(d["ids"])
    mask_id = V
    outside = {0: -1, 1: V, 2: mask_id, 3: 2 ** 40, 4: -2 ** 40, 5: V + 1, 6: 2 ** 31 + 3, 7: -(2 ** 31)}
    for r, v in outside.items():
        target[r] = v
    assert {bool(ids[r] == V) for r in outside} == {True, False}                   # on masked and on given rows
    pred, merged, score = (n(x) for x in launch(d["logits"], ids, target, mask_id))
    want = R.reference(d["logits"], ids, target, mask_id)
    fails, _ = R.check((pred, merged, score), want[:3], R.bound(d["logits"], target))
    assert not fails, fails
    for r in outside:
        assert pred[r] == ids[r] and merged[r] == ids[r] and score[r] == R.GIVEN_SCORE, (r, outside[r])
    assert pred[8] == target[8] and (score[8] == R.GIVEN_SCORE) == (ids[8] != V)
    in_place = launch(d["logits"], ids, target, mask_id, in_place=True, null=True)[1]
    assert np.array_equal(n(in_place), merged)


# ------------------------------------------------------------------------------------------------------------- argument checks

def test_the_arguments_are_checked():
    lib = _lib.load()
    M, V = 9, 64
    X = torch.zeros(M, V + 8, device=dev())
    I = torch.full((M,), V, dtype=I64, device=dev())
    T = torch.zeros(M, dtype=I64, device=dev())
    sentinel = 12345
    P, O, S = (torch.full((M,), sentinel, dtype=dt, device=dev()) for dt in (I64, I64, F32))
    ptr = lambda x: None if x is None else x.data_ptr()

    def rc(logits=X, ldl=V + 8, ids_in=I, target=T, pred=P, ids_out=O, score=S, M_=M, V_=V):
        return lib.pmhip_sample_rows_forced(ptr(logits), ldl, ptr(ids_in), ptr(target), V, ptr(pred), ptr(ids_out), ptr(score), M_, V_, None)
    for bad, text in ((dict(logits=None), b"logits"), (dict(ids_in=None), b"ids_in"), (dict(target=None), b"target"), (dict(ids_out=None), b"ids_out"),
                      (dict(M_=0), b"M=0"), (dict(V_=0), b"V=0"), (dict(V_=16388, ldl=16388), b"V=16388"), (dict(V_=62), b"V=62"),
                      (dict(ldl=70), b"ldl=70"), (dict(ldl=60), b"ldl=60")):
        assert rc(**bad) == _lib.PMHIP_EINVAL, bad
        msg = lib.pmhip_last_error()
        assert b"sample_rows_forced" in msg and text in msg, (bad, msg)
    torch.cuda.synchronize()
    assert all(bool((x == sentinel).all()) for x in (P, O, S)), "a refused call wrote to an output"
    assert rc() == _lib.PMHIP_OK and rc(pred=None, score=None) == _lib.PMHIP_OK
    torch.cuda.synchronize()
    assert bool((P == 0).all()) and bool((O == 0).all()) and float((S - (1 - 1 / V)).abs().max()) < 1e-6       # a flat row: p = 1 / V
    for bad in (dict(logits=X[:, :V].double().contiguous()), dict(ids=I.int()), dict(target=T[:M - 1]), dict(target=T.int()), dict(logits=X[:, :V].contiguous()[0])):
        kw = dict(logits=X[:, :V].contiguous(), ids=I, target=T)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.sample_rows_forced(kw["logits"], kw["ids"], kw["target"], V)
    with pytest.raises(_lib.PmhipError):
        ops.sample_rows_forced(X[:, :V].contiguous().cpu(), I, T, V)              # host memory: no CPU fallback


# ------------------------------------------------------------------------------------------------------------- the loops

DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


class GpuRecorder:
    """wraps the operators of the GPU tail (the attributes ``generate`` looks up at call time): every forced step, draw, blend and
    re-masking, in call order"""
    NAMES = ("sample_rows_forced", "sample_rows", "blend_tokens", "remask")

    def __init__(self):
        self.forced, self.draws, self.blends, self.remasks, self.after = [], [], [], [], []
        self.real = {k: getattr(ops, k) for k in self.NAMES}

    def __enter__(self):
        real, keep = self.real, lambda d: tuple(x.clone() for x in d)
        ops.sample_rows_forced = lambda *a, **kw: (lambda d: (self.forced.append(keep(d)), d)[1])(real["sample_rows_forced"](*a, **kw))
        ops.sample_rows = lambda *a, **kw: (lambda d: (self.draws.append(keep(d)), d)[1])(real["sample_rows"](*a, **kw))
        ops.blend_tokens = lambda mask, *a: (lambda d: (self.blends.append((mask.clone() != 0, keep(d))), d)[1])(real["blend_tokens"](mask, *a))

        def remask(ids, scores, *a, **kw):
            self.remasks.append((ids.clone(), scores.clone()))
            out = real["remask"](ids, scores, *a, **kw)
            self.after.append(out.clone())
            return out
        ops.remask = remask
        return self

    def __exit__(self, *exc):
        for k in self.NAMES:
            setattr(ops, k, self.real[k])


@DTYPES
def test_the_invariants_on_the_gpu(tiny_pipe, data, dtype):
    pipe = tiny_pipe
    ctx = data["ctx"].to(dev())
    src, edit = ctx[:PAIRS].contiguous(), ctx[PAIRS:].contiguous()
    T, seed, N, V = 4, 7, pipe.num_tokens, pipe.mask_token_id
    g = math.isqrt(N)
    s = source_tokens(pipe).to(dev())
    args = (src, edit, LENS_SRC, LENS_EDIT, data["rm"], data["bl"], data["gn"], PAIRS, T, 1.0, 3, seed)
    with in_dtype(pipe, dtype):
        for ct in (None, 4.0):
            kw = dict(cross_steps=0.8, choice_temperature=ct, source_ids=s)
            with GpuRecorder() as rec:
                alone, revealed = pipe.forced_ids(s, src, PAIRS, T, seed, choice_temperature=ct, context_lens=LENS_SRC, return_steps=True)
            assert len(rec.forced) == T and not rec.draws
            check_source_half(pipe, s, alone, T)
            check_reveal(pipe, s, rec.after, revealed, T)
            plain = pipe.control_ids(*args, **kw)
            assert torch.equal(plain[0], alone)                                   # invariant 2
            assert not torch.equal(pipe.control_ids(*args, cross_steps=0.8, choice_temperature=ct)[0], alone)
            block = torch.zeros(PAIRS, g, g, dtype=torch.bool)
            block[:, 1:3, 1:3] = True
            ones, zeros = torch.ones_like(block), torch.zeros_like(block)
            for name, blend in (("false", dict(blend_mask=zeros)), ("true", dict(blend_mask=ones)), ("block", dict(blend_mask=block)),
                                ("rows", dict(blend_rows=phrase_rows(), blend_threshold=0.9, blend_grow=0))):
                with GpuRecorder() as rec:
                    ids_s, ids_e, img_s, img_e, mask = pipe.control_ids(*args, **kw, **blend, blend_start=0.0, want_imgs=True, return_mask=True)
                assert torch.equal(ids_s, alone), (name, ct)                      # invariant 2: whatever the edited half does
                check_source_half(pipe, s, ids_s, T)                              # invariant 3
                assert torch.equal(img_s, pipe.vqgan.decode_from_indice(s)) and bool(torch.isfinite(img_e).all())
                assert len(rec.forced) == T and len(rec.draws) == T and len(rec.blends) == T and len(rec.remasks) == 2 * T
                for step in range(T):                                             # invariant 4
                    pred_s, merged_s, score_s = rec.forced[step]
                    region, (pred_b, merged_b, score_b) = rec.blends[step]
                    region = region.reshape(-1)
                    (ms, ss), (me, se) = rec.remasks[2 * step], rec.remasks[2 * step + 1]
                    assert torch.equal(pred_s, s.reshape(-1)) and torch.equal(ms.reshape(-1), merged_s) and torch.equal(ss.reshape(-1), score_s)
                    assert torch.equal(me.reshape(-1), merged_b) and torch.equal(se.reshape(-1), score_b)
                    out = ~region
                    assert torch.equal(pred_b[out], s.reshape(-1)[out]) and torch.equal(merged_b[out], merged_s[out])
                    assert torch.equal(score_b[out].view(torch.int32), score_s[out].view(torch.int32))
                out = ~mask.reshape(PAIRS, N).to(dev())
                assert bool(((ids_e[out] == s[out]) | (ids_e[out] == V)).all()), (name, ct)
                if name == "false":
                    assert torch.equal(ids_e, ids_s) and not bool(mask.any())
                if name == "true":
                    assert torch.equal(ids_e, plain[1]) and bool(mask.all())
        ag = pipe.forced_ids(s, src, PAIRS, T, seed, guidance_scale=3.0, context_lens=LENS_SRC, image_base=2)
        a, _ = pipe.control_ids(*args, image_base=2, guidance_scale=3.0, source_ids=s, blend_rows=phrase_rows(), blend_start=0.0)
        assert torch.equal(a, ag)
        check_source_half(pipe, s, ag, T)


def test_the_loops_against_the_cpu_branch_in_fp32(tiny_pipe, cpu_pipe, data):
    """fp32-verify, the same source tokens and the same uniforms on both sides.  The forced half has no arg-max to tie; what can differ
    is a re-masking cut, a draw of the edited half or the region.  Differences are audited step by step from the GPU's own states: a
    differing position must lie within 1e-4 of its step's re-masking cut (the rule of tests/test_gpu_control.py's audit), and no
    more than AUDIT_CAP positions -- what tests/test_gpu_local_blend.py allows its loop: none -- may differ at all.
    tests/test_forced_cpu.py shows on the CPU that these inputs keep every decision further from flipping than the float bar moves it."""
    pipe, V, N = tiny_pipe, tiny_pipe.mask_token_id, tiny_pipe.num_tokens
    s, noise, rows = source_tokens(cpu_pipe), loop_noise(cpu_pipe), phrase_rows()
    ctx = data["ctx"]
    nmask = loop_schedule(LOOP_T, 1.0, N)[1]
    # forced_ids, step by step from the GPU's ids
    with GpuRecorder() as rec:
        got = pipe.forced_ids(s.to(dev()), ctx[:PAIRS].to(dev()), PAIRS, LOOP_T, LOOP_SEED, context_lens=LENS_SRC)
    want = cpu_pipe.forced_ids(s, ctx[:PAIRS], PAIRS, LOOP_T, LOOP_SEED, context_lens=LENS_SRC)
    audited = 0
    before = torch.full((PAIRS, N), V, dtype=I64)
    for step in range(LOOP_T):
        after = rec.after[step].cpu()
        with torch.no_grad():
            logits = cpu_pipe.transformer(cpu_pipe.ids2tokens(before), ctx[:PAIRS], context_lens=LENS_SRC)
        _, merged, score, _ = cpu_pipe._forced_cpu(before, logits, s, None, None)
        gpu_score = rec.forced[step][2].cpu().reshape(PAIRS, N)
        taken = before == V
        # a logit within TOL moves a probability by at most expm1(2 TOL) of itself, and the score is 1 - p (rounded once more)
        ratio = float(((gpu_score[taken] - score[taken]).abs() / (SCORE_REL * (1 - score[taken]) + 2.0 ** -22)).max())
        print(f"forced_ids step {step}: |score GPU - score CPU branch| / what the float bar grants = {ratio:.4f}")
        assert ratio < 1.0
        cut = score.topk(nmask[step], dim=-1).values[:, -1:]
        cpu_after = cpu_pipe._remask_cpu(merged, score.clone(), nmask[step], None, 0.0, None, [nmask[step]] * PAIRS)
        for b, i in (after != cpu_after).nonzero().tolist():
            assert abs(float(score[b, i] - cut[b, 0])) < 1e-4, (step, b, i, float(score[b, i]), float(cut[b, 0]))
            audited += 1
        before = after
    audited += int((got.cpu() != want).sum())
    # control_ids with a forced source and a local blend by a phrase
    args = (LENS_SRC, LENS_EDIT, data["rm"], data["bl"], data["gn"], PAIRS, LOOP_T, 1.0, LOOP_TOPK, LOOP_SEED)
    kw = dict(cross_steps=0.75, noise=noise, blend_rows=rows, return_mask=True, **LOOP)
    g_s, g_e, g_m = pipe.control_ids(ctx[:PAIRS].to(dev()), ctx[PAIRS:].to(dev()), *args, source_ids=s.to(dev()), **kw)
    c_s, c_e, c_m = cpu_pipe.control_ids(ctx[:PAIRS], ctx[PAIRS:], *args, source_ids=s, **kw)
    invented = cpu_pipe.control_ids(ctx[:PAIRS], ctx[PAIRS:], *args, **kw)
    assert torch.equal(c_s, want) and not torch.equal(invented[0], c_s) and 0 < int(c_m.sum()) < c_m.numel()
    audited += int((g_s.cpu() != c_s).sum()) + int((g_e.cpu() != c_e).sum()) + int((g_m.cpu() != c_m).sum())
    print(f"positions that differ from the CPU branch: {audited}")
    assert audited <= AUDIT_CAP


def test_prompt_to_prompt_from_a_real_image_on_the_gpu():
    t5 = t5_pipe(dev())
    text, edit = ["a red barn", "the cow"], ["a red church", "the big cow"]
    S, N, V = t5.image_size, t5.num_tokens, t5.mask_token_id
    img = (torch.rand(2, 3, S, S, generator=torch.Generator().manual_seed(4)) * 2 - 1).to(dev())
    s = t5.to_latent(img)[1].reshape(2, N)
    kw = dict(mode="replace", timesteps=3, seed=5)
    img_s, img_e = t5.prompt_to_prompt(text, edit, img=img, **kw)
    assert img_s.is_cuda and torch.equal(img_s, t5.vqgan.decode_from_indice(s)) and tuple(img_e.shape) == (2, 3, S, S) and bool(torch.isfinite(img_e).all())
    ids_s, ids_e = t5.prompt_to_prompt(text, edit, img=img, return_ids=True, **kw)
    same = t5.prompt_to_prompt(text, edit, source_ids=s, return_ids=True, **kw)
    assert torch.equal(ids_s, same[0]) and torch.equal(ids_e, same[1])
    check_source_half(t5, s, ids_s, 3)
    ctx, lens = t5.text_model(text, return_lens=True)
    assert torch.equal(ids_s, t5.forced_ids(s, ctx.to(dev()), 2, 3, 5, context_lens=lens))
    a, b, mask = t5.prompt_to_prompt(text, edit, img=img, local_blend=[("barn", "church"), "cow"], blend_start=0.0, return_ids=True, return_mask=True, **kw)
    out = ~mask.reshape(2, N).to(dev())
    assert torch.equal(a, ids_s) and bool(((b[out] == s[out]) | (b[out] == V)).all())
    for bad in (dict(img=img, source_ids=s), dict(img=img[:1]), dict(source_ids=s.clone().fill_(V)), dict(source_ids=s.int())):
        with pytest.raises(ValueError):
            t5.prompt_to_prompt(text, edit, **dict(kw, **bad))
