"""Model likelihood on the GPU.

pmhip_token_logprob at V in {256, 1024, 8192, 16384} -- the four classes of the kernel --, 1000 (the last register group ragged) and 4
(one float4): M = 9 rows, ldl = V + 8 with NaN in the padding, every buffer inside guard bands (tests/abi_frames.py).  Inputs, float64
restatement and element-wise bound are those of tests/logprob_ref.py; tests/test_logprob_cpu.py proves on the CPU that the bound rejects
the named faults at exactly these inputs.  Then the exact properties (lp <= 0, ent >= 0, two launches, the guided form against
pmhip_guidance_combine), the kernels that already score a target, the operator of ``paintmind_amd.ops``, and ``token_scores`` / ``score`` /
``surprise_mask`` / ``best_of`` on the tiny pipeline against the float64 rule applied to the GPU's own logits."""
import numpy as np
import pytest
import torch

import logprob_ref as R
from abi_frames import bits, call, framed
from gpu_common import dev, n, t
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline, best_index, diff_draws
from test_control_cpu import PAIRS
from test_gpu_control import tiny_pipe      # noqa: F401
from test_logprob_cpu import check_maps, float64_maps, score_setting

pytestmark = pytest.mark.gpu
F32, I32, I64 = torch.float32, torch.int32, torch.int64
VS = pytest.mark.parametrize("V", R.VS)
OUTPUTS = ("logp0", "ent0", "rank0", "count0")
# which of entropy / rank / count are NULL: none, each alone, all three
NULLS = ((), ("ent0",), ("rank0",), ("count0",), ("ent0", "rank0", "count0"))
_REF = {}


def ref(V, variant, accumulate=False):
    """the case with its float64 reference and bound: computed once, shared, never modified"""
    key = (V, variant, accumulate)
    if key not in _REF:
        d = dict(R.case(V, variant))
        prev = {k: d[k] for k in OUTPUTS}
        d["want"] = R.reference(d["a"], d["ids"], V, d["target"], accumulate=accumulate, **prev)
        d["B"] = R.bound(d["a"], d["target"], **(dict(logp0=d["logp0"], ent0=d["ent0"]) if accumulate else {}))
        for x in d["want"] + d["B"]:
            x.setflags(write=False)
        _REF[key] = d
    return _REF[key]


def flat(x, dtype, M):
    return framed(M, 1, ld=1, dtype=dtype, payload=None if x is None else t(np.array(x)).reshape(-1, 1), device=dev())


class Inputs:
    """the read-only operands of a launch inside their frames: a (and b) with NaN in the padding columns and around, ids, target"""

    def __init__(self, a, ids, target, b=None):
        self.M, self.V = a.shape
        self.a, self.b, self.ids, self.target = a, b, ids, target
        self.fa = framed(self.M, self.V, ld=self.V + 8, dtype=F32, payload=t(np.array(a)), fill="nan")
        self.fb = None if b is None else framed(self.M, self.V, ld=self.V + 8, dtype=F32, payload=t(np.array(b)), fill="nan")
        self.fi = None if ids is None else flat(ids, I64, self.M)
        self.ft = flat(target, I64, self.M)

    def assert_unchanged(self, what):
        for f, x, name in ((self.fa, self.a, "a"), (self.fb, self.b, "b"), (self.fi, self.ids, "ids"), (self.ft, self.target, "target")):
            if f is not None:
                f.assert_frame_untouched(f"{what} {name}")
                assert np.array_equal(n(f.payload()).reshape(np.shape(x)), x, equal_nan=x.dtype.kind == "f"), f"{what}: {name} was written"


def launch(inp, mask_id, prev=None, accumulate=False, nulls=(), scale=0.0, out=None):
    """the C entry on framed buffers -> ([logp, entropy, rank, count] as [M] tensors, None where NULL; the output frames); asserts the
    memory contract: nothing outside the [M] extents written, the operands as they were"""
    M, V = inp.M, inp.V
    if out is None:
        out = [None if k in nulls else flat(None if prev is None else prev[k], F32 if k in ("logp0", "ent0") else I32, M) for k in OUTPUTS]
    call("pmhip_token_logprob", inp.fa, inp.fb, float(scale), inp.fa.ld, inp.fi, int(mask_id), inp.ft, out[0], out[1], out[2], out[3],
         int(accumulate), M, V)
    torch.cuda.synchronize()
    what = f"V={V} accumulate={accumulate} nulls={nulls}"
    inp.assert_unchanged(what)
    for f, k in zip(out, OUTPUTS):
        if f is not None:
            f.assert_frame_untouched(f"{what} {k}")
    return [None if f is None else f.payload().reshape(M) for f in out], out


def as_numpy(got):
    return [None if x is None else n(x) for x in got]


# ------------------------------------------------------------------------------------------------------------- the operator

@VS
def test_the_operator_holds_the_bound(V):
    worst_all = 0.0
    for variant in R.VARIANTS:
        d0 = ref(V, variant)
        inp = Inputs(d0["a"], d0["ids"], d0["target"])
        for accumulate in (False, True):
            d = ref(V, variant, accumulate)
            prev = {k: d[k] for k in OUTPUTS}
            full = None
            for nulls in NULLS:
                got, _ = launch(inp, V, prev=prev, accumulate=accumulate, nulls=nulls)
                fails, worst = R.check(as_numpy(got), d["want"], d["B"])
                print(f"V={V} variant {variant} accumulate {accumulate} NULL {nulls}: worst err / bound {worst:.4f}")
                worst_all = max(worst_all, worst)
                assert not fails, fails
                if not accumulate:                                      # lp <= 0 and ent >= 0 wherever they are numbers
                    lp, ent = n(got[0]), None if got[1] is None else n(got[1])
                    assert (lp[~np.isnan(lp)] <= 0).all() and (ent is None or (ent[~np.isnan(ent)] >= 0).all())
                if full is None:
                    full = got
                else:                                                   # a NULL output changes nothing of the others
                    assert all(g is None or torch.equal(bits(g), bits(f)) for g, f in zip(got, full))
            # the operator of paintmind_amd.ops on contiguous tensors: the bits of the framed call
            for entropy, rank in ((True, True), (False, True), (True, False)):
                keep = (True, entropy, rank, True)
                out = tuple(t(np.array(d[k])) if on else None for k, on in zip(OUTPUTS, keep)) if accumulate else None
                via = ops.token_logprob(t(np.array(d["a"])), t(np.array(d["target"])), ids=None if d["ids"] is None else t(np.array(d["ids"])),
                                        mask_id=None if d["ids"] is None else V, out=out, accumulate=accumulate, entropy=entropy, rank=rank)
                assert [None if v is None else v.dtype for v in via] == [dt if on else None for dt, on in zip((F32, F32, I32, I32), keep)]
                assert all((v is None) == (not on) and (v is None or torch.equal(bits(v), bits(f))) for v, f, on in zip(via, full, keep))
                if accumulate:
                    assert all(v is o for v, o in zip(via, out))
    print(f"V={V}: the token-logprob kernel's worst err / bound {worst_all:.4f}")


@VS
def test_two_launches_and_two_complementary_accumulated_launches(V):
    v0, v1 = ref(V, 0), ref(V, 1)
    assert (v0["want"][4] != v1["want"][4]).all()
    i0, i1 = Inputs(v0["a"], v0["ids"], v0["target"]), Inputs(v1["a"], v1["ids"], v1["target"])
    one, _ = launch(i0, V)
    two, _ = launch(i0, V)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(one, two)), "two launches differ"
    # every row is scored in exactly one variant: the accumulated pair is the two single launches, row by row
    other, _ = launch(i1, V)
    zeros = dict(logp0=np.zeros(R.M, np.float32), ent0=np.zeros(R.M, np.float32), rank0=np.zeros(R.M, np.int32), count0=np.zeros(R.M, np.int32))
    _, out = launch(i0, V, prev=zeros, accumulate=True)
    acc, _ = launch(i1, V, accumulate=True, out=out)
    s0 = t(v0["want"][4])
    assert bool((acc[3] == 1).all())
    for k in range(3):
        single = torch.where(s0, one[k], other[k])
        nan = torch.isnan(single) if single.dtype == F32 else torch.zeros_like(s0)
        keep = ~nan & ~(t(np.isnan(v0["want"][0]) | np.isnan(v1["want"][0])) if k == 2 else nan)      # (the rank of a NaN row: unspecified)
        assert torch.equal(torch.isnan(acc[k].float()) if k < 2 else nan, nan) and torch.equal(bits(acc[k])[keep], bits(single)[keep]), k
    # an unscored row keeps what it held, NaN-filled logits or not; without accumulate it is zeroed
    sentinel = dict(logp0=np.full(R.M, 12345.5, np.float32), ent0=np.full(R.M, -7.25, np.float32), rank0=np.full(R.M, 777, np.int32),
                    count0=np.full(R.M, 555, np.int32))
    got, _ = launch(i0, V, prev=sentinel, accumulate=True)
    skipped = ~s0
    assert all(bool((g[skipped] == v).all()) for g, v in zip(got, (12345.5, -7.25, 777, 555))) and bool((got[3][s0] == 556).all())
    got, _ = launch(i0, V, prev=sentinel)
    assert all(bool((g[skipped] == 0).all()) for g in got) and bool((got[3][s0] == 1).all())


@VS
def test_the_guided_form_is_the_plain_form_on_guidance_combines_output(V):
    rng = np.random.default_rng([V, 37])
    for variant in (0, 2):
        d = ref(V, variant)
        b = (np.array(d["a"]) * np.float32(0.75) + rng.standard_normal((R.M, V)).astype(np.float32))
        b[np.isnan(b)] = 0.5                                            # (a's unscored and NaN rows: b finite, the combination NaN through a)
        b.setflags(write=False)
        guided_in = Inputs(d["a"], d["ids"], d["target"], b=b)
        for scale in (0.0, 1.0, 3.0, -0.5):
            x = ops.guidance_combine(t(np.array(d["a"])), t(b), scale)
            torch.cuda.synchronize()
            x = n(x)
            x.setflags(write=False)
            plain, _ = launch(Inputs(x, d["ids"], d["target"]), V)
            guided, _ = launch(guided_in, V, scale=scale)
            lp = plain[0]
            nan = torch.isnan(lp)
            assert int((~nan).sum()) >= 4
            for k, (g, p) in enumerate(zip(guided, plain)):
                keep = ~nan if k != 3 else torch.ones_like(nan)
                assert torch.equal(bits(g)[keep], bits(p)[keep]), (variant, scale, OUTPUTS[k], n(g), n(p))
            assert torch.equal(torch.isnan(guided[0]), nan) and torch.equal(torch.isnan(guided[1]), torch.isnan(plain[1]))


@VS
def test_against_the_kernels_that_already_score_a_target(V):
    """exp(lp) against 1 - score of pmhip_sample_rows_forced and -lp against row_loss of pmhip_masked_ce(label_smoothing=0), on the rows
    without -inf or NaN, within the sum of the two kernels' derived bounds (``logprob_ref.neighbours``)"""
    v0, v1, v2 = (R.case(V, k) for k in R.VARIANTS)
    a = np.concatenate([v2["a"], v0["a"][[0, 2, 4, 8]], v1["a"][[1, 3]]])
    target = np.concatenate([v2["target"], v0["target"][[0, 2, 4, 8]], v1["target"][[1, 3]]])
    rows = len(a)
    lp, _, _, _ = ops.token_logprob(t(a), t(target), entropy=False, rank=False)
    lp64, _, _ = R.values(a, target)
    B_lp = R.bound(a, target)[0]
    p64, B_p, nll64, B_nll = R.neighbours(a, target)
    masked = torch.full((rows,), V, dtype=I64, device=dev())
    _, _, score = ops.sample_rows_forced(t(a), masked, t(target), V)
    _, row_loss = ops.masked_ce(t(a), t(target), torch.ones(rows, device=dev()), label_smoothing=0.0)
    lp, score, row_loss = n(lp).astype(np.float64), n(score).astype(np.float64), n(row_loss).astype(np.float64)
    assert (np.abs(lp - lp64) < B_lp).all()
    gap_p = np.abs(np.exp(lp) - (1 - score))
    tol_p = p64 * np.expm1(B_lp) + B_p                                   # |exp(lp) - p64| <= p64 (e^B_lp - 1), |(1 - score) - p64| <= B_p
    gap_n = np.abs(-lp - row_loss)
    tol_n = B_lp + B_nll
    print(f"V={V}: exp(lp) vs 1 - forced score: worst gap / tolerance {(gap_p / tol_p).max():.4f}; -lp vs masked_ce row_loss: {(gap_n / tol_n).max():.4f}")
    assert (gap_p < tol_p).all() and (gap_n < tol_n).all()


def test_the_operator_serves_a_wide_row_stride_and_checks_its_arguments():
    V = 1000
    d = ref(V, 2)
    M = R.M
    a, target = t(np.array(d["a"])), t(np.array(d["target"]))
    want = ops.token_logprob(a, target)
    assert bool((want[3] == 1).all())
    wide = torch.full((2 * M, V + 8), float("nan"), device=dev())
    wide[:M, :V] = a
    wide[M:, :V] = 0.25 * a
    got = ops.token_logprob(wide[:M, :V], target)                       # a row stride wider than the row, NaN in the gap
    assert all(torch.equal(bits(g), bits(w)) for g, w in zip(got, want))
    guided = ops.token_logprob(wide[:M, :V], target, uncond=wide[M:, :V], scale=2.0)       # two halves of one tensor
    plain = ops.token_logprob(ops.guidance_combine(a, (0.25 * a).contiguous(), 2.0), target)
    assert all(torch.equal(bits(g), bits(w)) for g, w in zip(guided, plain))
    ok = (torch.zeros(M, device=dev()), torch.zeros(M, device=dev()), torch.zeros(M, dtype=I32, device=dev()), torch.zeros(M, dtype=I32, device=dev()))
    ids = torch.full((M,), V, dtype=I64, device=dev())
    for bad in (dict(out=ok[0]), dict(out=ok[:3]), dict(out=(ok[0], ok[1], ok[2].long(), ok[3])), dict(out=tuple(o[:M - 1] for o in ok)),
                dict(out=tuple(o.cpu() for o in ok)), dict(out=(ok[0].double(),) + ok[1:]), dict(out=(ok[0], None, ok[2], ok[3])),
                dict(out=ok, entropy=False), dict(out=ok, rank=False), dict(accumulate=True), dict(ids=ids), dict(ids=ids.cpu(), mask_id=V),
                dict(ids=ids.int(), mask_id=V), dict(target=target.cpu()), dict(target=target.int()), dict(uncond=a), dict(scale=1.0),
                dict(uncond=a.cpu(), scale=1.0), dict(uncond=a, scale=float("nan")), dict(uncond=wide[M:, :V], scale=1.0),
                dict(logits=a[:, 2:V - 2])):
        kw = dict(logits=a, target=target)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.token_logprob(**kw)
    with pytest.raises(_lib.PmhipError):
        ops.token_logprob(a.cpu(), target.cpu())                         # host memory: no CPU fallback
    torch.cuda.synchronize()
    assert all(bool((o == 0).all()) for o in ok), "a refused call wrote to an output"
    lib = _lib.load()
    assert lib.pmhip_token_logprob(a.data_ptr(), a.data_ptr(), float("inf"), V, None, V, target.data_ptr(), ok[0].data_ptr(), None, None, None, 0, M, V,
                                   None) == _lib.PMHIP_EINVAL
    assert b"scale=inf" in lib.pmhip_last_error()


# ------------------------------------------------------------------------------------------------------------- the pipeline

def combine_gpu(cond, uncond, scale):
    return ops.guidance_combine(cond.contiguous(), uncond.contiguous(), scale)


@pytest.mark.parametrize("scale", (None, 3.0))
def test_token_scores_is_the_float64_rule_on_the_gpus_own_logits(tiny_pipe, scale):
    """fp32-verify.  The logits are the GPU's own ``tokens2logits`` of the same masked ids (the guided row: ``ops.guidance_combine`` of the
    two), so what is compared is the new code alone: within the kernel's bound, the ranks exactly."""
    pipe = tiny_pipe
    img, ids, src, lens = score_setting(pipe, dev())
    N = pipe.num_tokens
    kw = dict(mask_ratio=0.4, draws=3, seed=7)
    masks = diff_draws(PAIRS, N, 0.4, 3, 7)
    got = pipe.token_scores(img, src, context_lens=lens, guidance_scale=scale, **kw)
    assert all(x.is_cuda and x.dtype == F32 for x in got)
    check_maps(got, *float64_maps(pipe, ids, src, lens, masks, scale, device=dev(), combine=combine_gpu), f"GPU, scale {scale}")
    again = pipe.token_scores(ids=ids.to(dev()), text=src.to(dev()), context_lens=lens, guidance_scale=scale, **kw)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(got, again))
    if scale is None:
        holes = ids.clone()
        holes[0, 3] = holes[1, 0] = pipe.mask_token_id
        mean, bound = float64_maps(pipe, holes, src, lens, masks, None, device=dev())
        check_maps(pipe.token_scores(ids=holes, text=src, context_lens=lens, **kw), mean, bound, "GPU, two mask ids")
        s = pipe.score(ids=holes, text=src, context_lens=lens, **kw)
        want = np.nansum(mean[0], axis=1) / (N - 1)
        assert np.abs(s.double().cpu().numpy() - want).max() < np.nansum(bound[0], axis=1).max() / (N - 1) + 2 * N * R.U * np.abs(want).max()
        check_maps(pipe.token_scores(img, None, **kw), *float64_maps(pipe, ids, None, None, masks, None, device=dev()), "GPU, unconditional")


def test_score_and_surprise_mask_on_the_gpu(tiny_pipe):
    pipe = tiny_pipe
    img, ids, src, lens = score_setting(pipe, dev())
    src = src.to(dev())
    g, N = pipe.image_size // pipe.patch_size, pipe.num_tokens
    kw = dict(context_lens=lens, mask_ratio=0.4, draws=3, seed=7)
    maps = pipe.token_scores(img, src, **kw)
    s = pipe.score(img, src, **kw)
    un = pipe.score(img, None, mask_ratio=0.4, draws=3, seed=7)
    assert s.is_cuda and s.dtype == F32 and tuple(s.shape) == (PAIRS,) and torch.equal(bits(s), bits(maps.logp.reshape(PAIRS, N).sum(1) / N))
    assert torch.equal(bits(pipe.score(img, src, relative=True, **kw)), bits(s - un))
    mask, sur = pipe.surprise_mask(img, src, threshold=0.9, grow=0, return_score=True, **kw)
    assert torch.equal(bits(sur), bits(-maps.logp)) and mask.is_cuda and mask.dtype == torch.bool and tuple(mask.shape) == (PAIRS, g, g)
    flat_s = sur.reshape(PAIRS, N).contiguous()
    assert torch.equal(mask.reshape(PAIRS, N), ops.phrase_region(flat_s, flat_s, g, 0.9, 0) != 0) and 0 < int(mask.sum()) < mask.numel()
    assert torch.equal(mask.reshape(PAIRS, N).cpu(), Pipeline._region_cpu(flat_s.cpu(), flat_s.cpu(), g, 0.9, 0))
    assert torch.equal(pipe.surprise_mask(img, src, **kw).reshape(PAIRS, N), ops.phrase_region(flat_s, flat_s, g, 0.5, 1) != 0)
    out, new = pipe.edit(img, token_mask=mask, text=src, context_lens=lens, timesteps=2, seed=3, return_ids=True)
    outside = ~mask.reshape(PAIRS, N)
    assert torch.equal(new[outside], ids.to(dev())[outside])


def test_best_of_on_the_gpu(tiny_pipe):
    pipe = tiny_pipe
    text = ["a red barn", "the cow"]
    gen = dict(timesteps=3, temperature=0.9, topk=4, seed=11, guidance_scale=1.5)
    imgs, index, scores, cands = pipe.best_of(text, 3, score_draws=2, score_seed=5, score_guidance=2.0, image_base=4, return_all=True, **gen)
    N = pipe.num_tokens
    assert cands.is_cuda and tuple(cands.shape) == (2, 3, N) and tuple(scores.shape) == (2, 3) and scores.dtype == F32 and imgs.is_cuda
    assert index.tolist() == best_index(scores).tolist() and bool(torch.isfinite(scores).all())
    ctx = pipe.text_model(text)
    distinct = 0
    for j in range(3):                                                   # candidate j: the run with image_base + j * B, bit for bit
        run, ids = pipe.generate(text, save_interval=1, image_base=4 + j * 2, return_ids=True, **gen)
        assert torch.equal(ids, cands[:, j])
        assert torch.equal(bits(scores[:, j]), bits(pipe.score(ids=ids, text=ctx, draws=2, seed=5, guidance_scale=2.0)))
        distinct += j > 0 and not torch.equal(cands[:, j], cands[:, 0])
        for b in range(2):
            if index[b] == j:
                assert torch.equal(bits(imgs[b].cpu()), bits(run[-1][b]))
    assert distinct == 2, "the image index keys the noise: the candidates differ"
    again = pipe.best_of(text, 3, score_draws=2, score_seed=5, score_guidance=2.0, image_base=4, return_all=True, **gen)
    assert all(torch.equal(bits(x) if x.dtype == F32 else x, bits(y) if y.dtype == F32 else y) for x, y in zip((imgs, index, scores, cands), again))
    one = pipe.best_of(text, 1, **gen)
    assert one[1].tolist() == [0, 0] and torch.equal(bits(one[0].cpu()), bits(pipe.generate(text, save_interval=1, **gen)[-1]))
