"""Mask-free editing on the GPU.

pmhip_logit_divergence at V in {64, 1000, 8192, 16384} -- the four classes of the kernel; 1000 leaves the last register group ragged --
both kinds, M = 9 row pairs, ldl = V + 8 with NaN in the padding, every buffer inside guard bands (tests/abi_frames.py).  Inputs, float64
restatement and element-wise bound are those of tests/divergence_ref.py; tests/test_divergence_cpu.py proves on the CPU that the bound
rejects the named faults at exactly these inputs.  Then the exact properties (a == b, the swap, two launches), the accumulation, the
operator of ``paintmind_amd.ops``, and ``diff_mask`` / ``diff_edit`` on the tiny pipelines against the CPU branch and their invariants."""
import numpy as np
import pytest
import torch

import divergence_ref as R
from abi_frames import bits, call, framed
from gpu_common import dev, n, t
from paintmind_amd import _lib, ops
from test_divergence_cpu import AUDIT_CAP, PAIRS, SCORE_REL, jeffreys_tol, photo, scores_in_float64, setting_call
from test_forced_cpu import t5_pipe
from test_gpu_control import cpu_pipe, in_dtype, tiny_pipe      # noqa: F401

pytestmark = pytest.mark.gpu
F32, I32, I64 = torch.float32, torch.int32, torch.int64
VS = pytest.mark.parametrize("V", R.VS)
KIND = {"tv": 0, "jeffreys": 1}
_REF = {}


def ref(V, kind, variant, accumulate=False, all_rows=False):
    """the case with its float64 reference and bound: computed once, shared, never modified"""
    key = (V, kind, variant, accumulate, all_rows)
    if key not in _REF:
        d = dict(R.case(V, kind, variant))
        d["want"] = R.reference(d["a"], d["b"], None if all_rows else d["ids"], V, kind, acc0=d["acc0"], count0=d["count0"], accumulate=accumulate)
        d["B"] = R.bound(d["a"], d["b"], kind, d["acc0"] if accumulate else None)
        for x in d["want"] + (d["B"],):
            x.setflags(write=False)
        _REF[key] = d
    return _REF[key]


def flat(x, dtype, M):
    return framed(M, 1, ld=1, dtype=dtype, payload=None if x is None else t(np.array(x)).reshape(-1, 1), device=dev())


def launch(a, b, ids, mask_id, kind, acc0=None, count0=None, accumulate=False, count_null=False, same_pointer=False, out=None):
    """the C entry on framed buffers -> (acc f32 [M], count int32 [M] or None, the output frames); asserts the memory contract: nothing
    outside the [M] extents written, a / b / ids as they were"""
    M, V = a.shape
    fa = framed(M, V, ld=V + 8, dtype=F32, payload=t(np.array(a)), fill="nan")                 # NaN in the padding columns and around
    fb = fa if same_pointer else framed(M, V, ld=V + 8, dtype=F32, payload=t(np.array(b)), fill="nan")
    fi = None if ids is None else flat(ids, I64, M)
    facc, fcount = out if out is not None else (flat(acc0, F32, M), None if count_null else flat(count0, I32, M))
    call("pmhip_logit_divergence", fa, fb, fa.ld, fi, int(mask_id), KIND[kind], facc, fcount, int(accumulate), M, V)
    torch.cuda.synchronize()
    for f, what in ((fa, "a"), (fb, "b"), (fi, "ids"), (facc, "acc"), (fcount, "count")):
        if f is not None:
            f.assert_frame_untouched(f"V={V} {kind} {what}")
    assert np.array_equal(n(fa.payload()), a, equal_nan=True) and np.array_equal(n(fb.payload()), a if same_pointer else b, equal_nan=True)
    if ids is not None:
        assert np.array_equal(n(fi.payload()).reshape(M), ids)
    return facc.payload().reshape(M), None if fcount is None else fcount.payload().reshape(M), (facc, fcount)


def finite_rows(d):
    """the case's rows without NaN: (a, b) of rows 0 .. 6"""
    return np.array(d["a"][:7]), np.array(d["b"][:7])


# ------------------------------------------------------------------------------------------------------------- the operator

@VS
def test_the_operator_holds_the_bound(V):
    worst_all = 0.0
    for kind in R.KINDS:
        for variant in (0, 1):
            for accumulate in (False, True):
                d = ref(V, kind, variant, accumulate)
                kw = dict(acc0=d["acc0"], count0=d["count0"]) if accumulate else {}
                acc, count, _ = launch(d["a"], d["b"], d["ids"], V, kind, accumulate=accumulate, **kw)
                fails, worst = R.check((n(acc), n(count)), d["want"], d["B"])
                print(f"V={V} {kind} variant {variant} accumulate {accumulate}: worst err / bound {worst:.4f}")
                worst_all = max(worst_all, worst)
                assert not fails, fails
                # the operator of paintmind_amd.ops on contiguous tensors: the bits of the framed call
                out = (t(np.array(d["acc0"])), t(np.array(d["count0"]))) if accumulate else None
                via = ops.logit_divergence(t(np.array(d["a"])), t(np.array(d["b"])), ids=t(np.array(d["ids"])), mask_id=V, kind=kind, out=out,
                                           accumulate=accumulate)
                assert via[0].dtype == F32 and via[1].dtype == I32
                assert torch.equal(bits(via[0]), bits(acc)) and torch.equal(via[1], count)
                if accumulate:
                    assert via[0] is out[0] and via[1] is out[1]
    print(f"V={V}: the divergence kernel's worst err / bound {worst_all:.4f}")


@VS
def test_the_exact_properties(V):
    d = ref(V, "tv", 0)
    for kind in R.KINDS:
        a, b = finite_rows(d)
        one, count, _ = launch(a, b, None, V, kind)                                 # ids NULL: every row is scored
        two, _, _ = launch(a, b, None, V, kind)
        assert torch.equal(bits(one), bits(two)), "two launches differ"
        assert bool((count == 1).all())
        swapped, _, _ = launch(b, a, None, V, kind)
        assert torch.equal(bits(swapped), bits(one)), f"swap(a, b) changes bits: {n(swapped) - n(one)}"
        for x in (a, b):
            same, _, _ = launch(x, x.copy(), None, V, kind)
            assert torch.equal(bits(same), torch.zeros_like(bits(same))), f"a == b is not exactly +0: {n(same)}"
            alias, _, _ = launch(x, x, None, V, kind, same_pointer=True)
            assert torch.equal(bits(alias), torch.zeros_like(bits(alias)))
        null, none, _ = launch(a, b, None, V, kind, count_null=True)                # count NULL is accepted
        assert none is None and torch.equal(bits(null), bits(one))
        # the -inf and NaN rules, exactly (every row scored)
        full = ref(V, kind, 0, all_rows=True)
        acc, count, _ = launch(full["a"], full["b"], None, V, kind)
        fails, _ = R.check((n(acc), n(count)), full["want"], full["B"])
        assert not fails, fails
        acc = n(acc)
        assert acc[0] == 0 and np.isfinite(acc[5]) and np.isnan(acc[7]) and np.isnan(acc[8]) and np.isfinite(acc[:7]).sum() == (7 if kind == "tv" else 6)
        assert acc[6] == np.inf if kind == "jeffreys" else np.isfinite(acc[6])


@VS
def test_two_complementary_accumulated_launches_are_the_single_launch(V):
    for kind in R.KINDS:
        v0, v1 = ref(V, kind, 0), ref(V, kind, 1)
        assert ((v0["ids"] == V) != (v1["ids"] == V)).all()
        single, _, _ = launch(v0["a"], v0["b"], None, V, kind)
        zeros = np.zeros(R.M, np.float32), np.zeros(R.M, np.int32)
        _, _, out = launch(v0["a"], v0["b"], v0["ids"], V, kind, acc0=zeros[0], count0=zeros[1], accumulate=True)
        acc, count, _ = launch(v1["a"], v1["b"], v1["ids"], V, kind, accumulate=True, out=out)
        assert bool((count == 1).all())                                            # every row is scored once
        nan = torch.isnan(single)
        assert torch.equal(torch.isnan(acc), nan) and torch.equal(bits(acc)[~nan], bits(single)[~nan])
        # an unscored row keeps what it held, NaN-filled logits or not
        sentinel = np.full(R.M, 12345.5, np.float32), np.full(R.M, 777, np.int32)
        acc, count, _ = launch(v0["a"], v0["b"], v0["ids"], V, kind, acc0=sentinel[0], count0=sentinel[1], accumulate=True)
        skipped = t(v0["ids"] != V)
        assert bool((acc[skipped] == 12345.5).all()) and bool((count[skipped] == 777).all()) and bool((count[~skipped] == 778).all())
        acc, count, _ = launch(v0["a"], v0["b"], v0["ids"], V, kind, acc0=sentinel[0], count0=sentinel[1])
        assert bool((acc[skipped] == 0).all()) and bool((count[skipped] == 0).all()) and bool((count[~skipped] == 1).all())


def test_the_operator_serves_two_halves_of_one_tensor_and_checks_its_arguments():
    V = 1000
    d = ref(V, "tv", 0)
    a, b = finite_rows(d)
    M = len(a)
    both = t(np.concatenate([a, b]))
    want, _, _ = launch(a, b, None, V, "tv")
    acc, count = ops.logit_divergence(both[:M], both[M:])
    assert torch.equal(bits(acc), bits(want)) and bool((count == 1).all())
    wide = torch.full((2 * M, V + 8), float("nan"), device=dev())
    wide[:, :V] = both
    acc, _ = ops.logit_divergence(wide[:M, :V], wide[M:, :V])                       # a common row stride wider than the row
    assert torch.equal(bits(acc), bits(want))
    A, Bt = both[:M], both[M:]
    ids = torch.full((M,), V, dtype=I64, device=dev())
    ok = (torch.zeros(M, device=dev()), torch.zeros(M, dtype=I32, device=dev()))
    for bad in (dict(out=ok[0]), dict(out=(ok[0],)), dict(out=(ok[0], ok[1].long())), dict(out=(ok[0][:M - 1], ok[1][:M - 1])), dict(out=(ok[0].cpu(), ok[1].cpu())),
                dict(out=(ok[0].double(), ok[1])), dict(accumulate=True), dict(kind="kl"), dict(ids=ids), dict(ids=ids.cpu(), mask_id=V),
                dict(ids=ids.int(), mask_id=V), dict(b=Bt.cpu()), dict(b=wide[M:, :V]), dict(a=both[:M, 2:V - 2], b=both[M:, 2:V - 2])):
        kw = dict(a=A, b=Bt)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.logit_divergence(**kw)
    with pytest.raises(_lib.PmhipError):
        ops.logit_divergence(A.cpu(), Bt.cpu())                                    # host memory: no CPU fallback
    torch.cuda.synchronize()
    assert bool((ok[0] == 0).all()) and bool((ok[1] == 0).all()), "a refused call wrote to an output"
    lib = _lib.load()
    assert lib.pmhip_logit_divergence(A.data_ptr(), Bt.data_ptr(), V, None, V, 2, ok[0].data_ptr(), None, 0, M, V, None) == _lib.PMHIP_EINVAL
    assert b"kind=2" in lib.pmhip_last_error()


# ------------------------------------------------------------------------------------------------------------- the pipeline

@pytest.fixture(scope="module")
def t5_gpu():
    return t5_pipe(dev())


@pytest.mark.parametrize("kind", R.KINDS)
def test_diff_mask_against_the_cpu_branch_in_fp32(tiny_pipe, cpu_pipe, kind):
    """fp32-verify.  The tolerance is derived, not chosen: the project's float bar TOL = 1e-3 is the gap granted between the two
    branches' logits, so a probability moves by at most eps = expm1(2 TOL) of itself (the existing SCORE_REL) and
        tv:        |d score| <= 1/2 sum (eps p + eps q) = eps
        jeffreys:  |d score| <= 2 eps (R + 4 TOL) + 8 TOL,   R = max |log p - log q| over the compared rows, from the float64 CPU values
    (``test_divergence_cpu.jeffreys_tol`` has the derivation).  At the setting tests/test_divergence_cpu.py shows to be further from
    every tie than that, the mask is the CPU branch's exactly: no audited position."""
    score64, r_max, mask_c, score_c = scores_in_float64(cpu_pipe, kind)
    tol = SCORE_REL if kind == "tv" else jeffreys_tol(r_max)
    mask_g, score_g = setting_call(tiny_pipe, kind, device=dev())
    g = tiny_pipe.image_size // tiny_pipe.patch_size
    assert mask_g.is_cuda and mask_g.dtype == torch.bool and tuple(mask_g.shape) == (PAIRS, g, g) and score_g.dtype == F32 and tuple(score_g.shape) == (PAIRS, g, g)
    err = float((score_g.cpu().double() - torch.from_numpy(score64).reshape(PAIRS, g, g)).abs().max())
    print(f"{kind}: R = {r_max:.3f}; |score GPU - score64 CPU branch| = {err:.3e}, {err / tol:.4f} of the tolerance {tol:.3e}")
    assert err <= tol
    differing = int((mask_g.cpu() != mask_c).sum())
    print(f"{kind}: positions of the mask that differ from the CPU branch: {differing}")
    assert differing <= AUDIT_CAP and 0 < int(mask_g.sum()) < mask_g.numel()
    again, score_again = setting_call(tiny_pipe, kind, device=dev())
    assert torch.equal(again, mask_g) and torch.equal(bits(score_again), bits(score_g))


def test_the_invariants_in_bf16(t5_gpu):
    pipe = t5_gpu
    N, V = pipe.num_tokens, pipe.mask_token_id
    g = pipe.image_size // pipe.patch_size
    img = photo(pipe).to(dev())
    text, edit = ["a red barn", "the cow"], ["a red church", "the big cow"]
    with in_dtype(pipe, torch.bfloat16):
        for kind in R.KINDS:
            mask, score = pipe.diff_mask(img, text, text, kind=kind, mask_padding=True, return_score=True)
            assert bool((score == 0).all()) and not bool(mask.any())               # identical prompts: an empty mask
            mask, score = pipe.diff_mask(img, text, edit, kind=kind, mask_padding=True, threshold=0.9, grow=0, return_score=True)
            again, score_again = pipe.diff_mask(img, text, edit, kind=kind, mask_padding=True, threshold=0.9, grow=0, return_score=True)
            assert torch.equal(mask, again) and torch.equal(bits(score), bits(score_again))            # the same run to run
            assert mask.is_cuda and mask.dtype == torch.bool and tuple(mask.shape) == (PAIRS, g, g)
            assert score.dtype == F32 and tuple(score.shape) == (PAIRS, g, g) and bool(torch.isfinite(score).all()) and bool((score > 0).all())
            assert bool(mask.reshape(PAIRS, -1).any(1).all())                      # (every image's maximum is in its region)
        kw = dict(threshold=0.9, grow=0, kind="tv", mask_ratio=0.5, draws=4)
        ekw = dict(timesteps=3, seed=5, return_ids=True, mask_padding=True)
        (out, ids), mask = pipe.diff_edit(img, text, edit, diff_seed=3, return_mask=True, **kw, **ekw)
        by_hand_mask = pipe.diff_mask(img, text, edit, seed=3, mask_padding=True, **kw)
        by_hand, by_hand_ids = pipe.edit(img, token_mask=by_hand_mask, text=edit, **ekw)
        assert torch.equal(mask, by_hand_mask) and torch.equal(ids, by_hand_ids) and torch.equal(out, by_hand)
        s = pipe.to_latent(img)[1].reshape(PAIRS, N).to(ids.device)
        outside = ~mask.reshape(PAIRS, N)
        assert torch.equal(ids[outside], s[outside]) and not bool((ids == V).any())
        ids_s, ids_e = pipe.prompt_to_prompt(text, edit, img=img, blend_mask=mask, blend_start=0.0, mode="replace", timesteps=3, seed=5, return_ids=True)
        assert bool(((ids_e[outside] == s[outside]) | (ids_e[outside] == V)).all())


def test_a_diff_mask_call_leaves_no_state_behind(t5_gpu):
    pipe = t5_gpu
    N = pipe.num_tokens
    img = photo(pipe).to(dev())
    text, edit = ["a red barn", "the cow"], ["a red church", "the big cow"]
    ctx, lens = pipe.text_model(text, return_lens=True)
    tok = pipe.ids2tokens(pipe.to_latent(img)[1].reshape(PAIRS, N).to(dev()))
    block = torch.zeros(PAIRS, 4, 4, dtype=torch.bool)
    block[:, 1:3, 1:3] = True

    def paths():
        return (pipe.tokens2logits(tok, ctx.to(dev()), context_lens=lens), pipe.edit(img, token_mask=block, text=edit, timesteps=3, seed=5),
                pipe.phrase_mask(img, text, ["barn", "cow"]))
    before = paths()
    for kind in R.KINDS:
        pipe.diff_mask(img, text, edit, kind=kind, mask_padding=True)
    after = paths()
    for x, y in zip(before, after):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int32) if x.dtype == F32 else x, y.view(torch.int32) if y.dtype == F32 else y)
