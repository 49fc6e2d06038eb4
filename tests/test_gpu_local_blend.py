"""The local blend on the GPU.

pmhip_attention_phrase_score: both dtypes, both score units, dim_head 64 (bf16: the MFMA kernel; f32: the vector-ALU kernel) and 32
in bf16, control given and NULL, overwriting (scale 1) and accumulating (scale 1/2), heads 2 and 3.  2 pairs, Nq = 80 (one full
64-query group and a tail), (Ls, Lt) in (1,1) (33,17) (77,77) (129,77) (77,129) (416,231), lengths absent, at 1 / mid and at mid /
full, NaN in every K row that may reach nothing, weights that are mostly 0 and partly behind the lengths.  The inputs, the float64
reference and the element-wise bound are those of tests/blend_ref.py; tests/test_local_blend_cpu.py proves on the CPU that the bound
rejects the named faults at exactly these inputs.

pmhip_phrase_region and pmhip_blend_tokens against their numpy restatements, bit for bit.  Then the engine entry, the loop and the
surface against the CPU branch."""
import numpy as np
import pytest
import torch

import abi_frames as A
import attention_probes as P
import attnmap_ref as M
import blend_ref as R
from gpu_common import dev, n, t
from paintmind_amd import _lib, ops
from test_local_blend_cpu import HEADS_SIGMA, SCALE_ACC

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
CONFIGS = pytest.mark.parametrize("dh,dtype", [(64, BF), (64, F32), (32, BF)], ids=["dh64-bf16", "dh64-f32", "dh32-bf16"])
MODES = pytest.mark.parametrize("exp2", [True, False], ids=["exp2", "exp"])
CONTROL = pytest.mark.parametrize("control", [True, False], ids=["control", "plain"])
B, NQ = 2, 80
_REF = {}


def gauss(Ls, Lt, dh, sigma, kind, H, control, exp2):
    """the case with the kernels' view of it and its float64 reference: computed once, shared by the tests below, never modified"""
    key = (Ls, Lt, dh, sigma, kind, H, control, exp2)
    if key not in _REF:
        d = R.case(Ls, Lt, dh, sigma, kind, H=H, control=control)
        d["ksp"], d["ktp"] = R.poison(d)
        d["r"] = R.reference(d, exp2)
        for x in list(d.values()) + list(d["r"].values()):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        _REF[key] = d
    return _REF[key]


def operands(d, dtype, rows=slice(None)):
    c = lambda x, dt=None: None if x is None else t(np.array(x[rows]), dt)
    return dict(qs=c(d["qs"], dtype), ks=c(d["ksp"], dtype), qt=c(d["qt"], dtype), kt=c(d["ktp"], dtype), w_src=c(d["w_s"]), w_tgt=c(d["w_t"]),
                row_map=c(d["row_map"]), blend=c(d["blend"]), gain=c(d["gain"]), lens_src=c(d["lens_s"]), lens_tgt=c(d["lens_t"]))


def launch(d, dtype, exp2, rows=slice(None), scale=1.0, into=None, **kw):
    """-> (score_s, score_t) tensors [pairs, Nq]; into: the pair of numpy arrays the launch accumulates onto"""
    o = operands(d, dtype, rows)
    o.update(kw)
    Ls, Lt = d["ks"].shape[2], d["kt"].shape[2]
    out = None if into is None else (t(np.array(into[0][rows])), t(np.array(into[1][rows])))
    return ops.attention_phrase_score(o.pop("qs"), o.pop("ks"), o.pop("qt"), o.pop("kt"), Ls, Lt, o.pop("w_src"), o.pop("w_tgt"),
                                      use_exp2=exp2, scale=scale, accumulate=into is not None, out=out, **o)


def every_case(dh, control, exp2, shapes=R.SHAPES):
    for Ls, Lt in shapes:
        for kind in R.LENS:
            for H, sigma in HEADS_SIGMA:
                yield (Ls, Lt, kind, H), gauss(Ls, Lt, dh, sigma, kind, H, control, exp2)


@CONFIGS
@MODES
@CONTROL
def test_gauss_family_holds_the_bound(dh, dtype, exp2, control):
    worst, failures = {}, []
    for name, d in every_case(dh, control, exp2):
        for scale, into in ((1.0, None), (SCALE_ACC, R.into_arrays(B, NQ))):
            got = tuple(n(x) for x in launch(d, dtype, exp2, scale=scale, into=into))
            want, Bd = R.expected(d["r"], scale, into), R.bound(d, d["r"], exp2, scale, into)
            ratio, idx = R.worst(got, want, Bd)
            print(f"{name} accumulate={into is not None}: err / B {ratio:.4f}")
            worst[into is not None] = max(worst.get(into is not None, 0.0), ratio)
            if ratio >= 1.0:
                failures.append(f"{name} accumulate={into is not None}: {ratio:.3g} x the bound at (which, pair, query) = {idx}")
    print(f"phrase score dim_head {dh} {dtype} exp2={exp2} control={control}: largest err / B by (accumulating) {worst}")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])


@CONFIGS
@MODES
@CONTROL
def test_exact_family_is_bit_exact(dh, dtype, exp2, control):
    """heads = 4, weights 0 / 1: every score is a multiple of 1/16, the same in both units and both dtypes"""
    into = tuple((np.round(x * 16) / 16).astype(np.float32) for x in R.into_arrays(B, NQ))
    for Ls, Lt in R.SHAPES:
        for kind in R.LENS:
            d = R.exact_case(Ls, Lt, dh, kind, control=control)
            d["ksp"], d["ktp"] = R.poison(d)
            r = R.reference(d, exp2)
            for scale, base in ((1.0, None), (0.5, into)):
                want = R.expected(r, scale, base)
                got = launch(d, dtype, exp2, scale=scale, into=base)
                for which in (0, 1):
                    assert np.array_equal(n(got[which]), want[which].astype(np.float32)), (Ls, Lt, kind, scale, "st"[which])


@CONFIGS
@MODES
def test_no_control_is_the_maps_contracted_with_the_weights(dh, dtype, exp2):
    """NULL control: against ops.attention_maps(kv_lens=) of each half, contracted with the weights in float64, within the SUM of this
    entry's bound and the maps' bound (attnmap_ref.bound) contracted the same way"""
    for name, d in every_case(dh, False, exp2):
        Ls, Lt, kind, H = name
        o = operands(d, dtype)
        got = tuple(n(x) for x in launch(d, dtype, exp2))
        Bd = R.bound(d, d["r"], exp2)
        for which, (q, k, L, lens, w, nx) in enumerate(((o["qs"], o["ks"], Ls, o["lens_src"], d["w_s"], d["r"]["ns"]),
                                                        (o["qt"], o["kt"], Lt, o["lens_tgt"], d["w_t"], d["r"]["nt"]))):
            kv = lens if lens is not None else torch.full((B,), L, dtype=torch.int32, device=dev())
            maps = n(ops.attention_maps(q, k, L, use_exp2=exp2, kv_lens=kv)).astype(np.float64)                  # [B, Nq, L]
            ok = np.broadcast_to((np.arange(L)[None, :] < nx[:, None])[:, None, :], (B, NQ, L))
            qn, kn = (d["qs"], d["ks"]) if which == 0 else (d["qt"], d["kt"])
            ref, p, s = M.reference(qn, np.where(ok[:, None, 0, :, None], kn, 0.0), ok, None, exp2)
            Bm = (M.bound(qn, np.where(ok[:, None, 0, :, None], kn, 0.0), ref, p, s, exp2) * w[:, None, :]).sum(-1)
            via = (maps * w.astype(np.float64)[:, None, :]).sum(-1)
            ratio, idx = P.worst_ratio(got[which], via, Bd[which] + Bm)
            print(f"{name} {'st'[which]}: |score - maps . w| / (B + B_maps) {ratio:.4f}")
            assert ratio < 1.0, (name, "st"[which], idx, ratio)


@CONFIGS
@CONTROL
def test_memory_contract(dh, dtype, control):
    """both outputs inside guard bands: nothing outside the two [B, Nq] extents is written, the payloads equal the plain launch bit for
    bit; under accumulate likewise"""
    lib_dtype = _lib.BF16 if dtype == BF else _lib.F32
    for Ls, Lt in ((33, 17), (129, 77)):
        for kind in ("full", "one_mid"):
            d = gauss(Ls, Lt, dh, 2.0, kind, 2, control, True)
            o = operands(d, dtype)
            for acc in (0, 1):
                base = tuple(t(x) for x in R.into_arrays(B, NQ)) if acc else (None, None)
                plain = launch(d, dtype, True, into=R.into_arrays(B, NQ) if acc else None)
                fs, ft = (A.framed(B, NQ, ld=NQ, dtype=F32, payload=base[i], device=dev()) for i in (0, 1))
                A.call("pmhip_attention_phrase_score", lib_dtype, o["qs"], o["ks"], o["qt"], o["kt"], B, 2, dh, NQ, Ls, o["ks"].shape[2], Lt,
                       o["kt"].shape[2], 1, o["row_map"], o["blend"], o["gain"], o["lens_src"], o["lens_tgt"], o["w_src"], o["w_tgt"], fs, ft,
                       1.0, acc)
                torch.cuda.synchronize()
                fs.assert_frame_untouched(f"phrase score_s Ls={Ls} Lt={Lt} {kind} accumulate={acc}")
                ft.assert_frame_untouched(f"phrase score_t Ls={Ls} Lt={Lt} {kind} accumulate={acc}")
                assert torch.equal(fs.payload(), plain[0]) and torch.equal(ft.payload(), plain[1]), (Ls, Lt, kind, acc)


@CONFIGS
@MODES
@CONTROL
def test_repeatable_and_independent_of_the_batch(dh, dtype, exp2, control):
    for Ls, Lt in ((77, 129), (416, 231)):
        for kind in R.LENS:
            d = gauss(Ls, Lt, dh, 8.0, kind, 3, control, exp2)
            a, b = launch(d, dtype, exp2), launch(d, dtype, exp2)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (Ls, Lt, kind, "the same launch twice")
            for pair in range(B):
                alone = launch(d, dtype, exp2, rows=slice(pair, pair + 1))
                assert torch.equal(alone[0], a[0][pair:pair + 1]) and torch.equal(alone[1], a[1][pair:pair + 1]), (Ls, Lt, kind, pair, "a pair alone")


def test_the_arguments_are_checked():
    z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device=dev())
    q, k = z(2, 2, 16, 64), z(2, 2, 64, 64)
    rm, bl, gn = z(2, 64, dt=torch.int32), z(2, 64), torch.ones(2, 64, device=dev())
    w = torch.ones(2, 64, device=dev())
    lens = torch.full((2,), 64, dtype=torch.int32, device=dev())
    ones = torch.ones(2, 16, device=dev())
    for kw in (dict(), dict(row_map=rm, blend=bl, gain=gn), dict(lens_src=lens, lens_tgt=lens)):        # uniform softmax, weights 1: exactly 1
        a, c = ops.attention_phrase_score(q, k, q, k, 64, 64, w, w, **kw)
        assert torch.equal(a, ones) and torch.equal(c, ones), kw
    for bad in (dict(row_map=rm), dict(row_map=rm, blend=bl), dict(row_map=rm.float(), blend=bl, gain=gn), dict(row_map=rm, blend=bl[:, :63], gain=gn),
                dict(lens_src=lens.long()), dict(lens_tgt=lens[:1]), dict(out=(torch.empty(2, 15, device=dev()), ones.clone())),
                dict(out=ones.clone()), dict(accumulate=True), dict(out=(ones.clone(), ones.double()))):
        with pytest.raises(ValueError):
            ops.attention_phrase_score(q, k, q, k, 64, 64, w, w, **bad)
    for ws, wt in ((None, w), (w, None), (w[:, :63], w), (w, w.double())):
        with pytest.raises(ValueError):
            ops.attention_phrase_score(q, k, q, k, 64, 64, ws, wt)
    with pytest.raises(ValueError):
        ops.attention_phrase_score(q[:, :1], k, q, k, 64, 64, w, w)
    with pytest.raises(_lib.PmhipError):
        ops.attention_phrase_score(q.cpu(), k, q, k, 64, 64, w, w)                                       # host memory: no CPU fallback
    lib = _lib.load()
    sentinel = 7.0
    os_, ot_ = torch.full((2, 16), sentinel, device=dev()), torch.full((2, 16), sentinel, device=dev())
    qb, kb = q.to(BF), k.to(BF)
    Pt = lambda x: None if x is None else x.data_ptr()

    def rc(dtype=_lib.F32, Qs=q, Ks=k, Qt=q, Kt=k, Bn=2, heads=2, dh=64, nq=16, ls=64, lsp=64, lt=64, ltp=64, rm_=None, bl_=None, gn_=None, ws=w,
           wt=w, S=os_, T=ot_, scale=1.0):
        return lib.pmhip_attention_phrase_score(dtype, Pt(Qs), Pt(Ks), Pt(Qt), Pt(Kt), Bn, heads, dh, nq, ls, lsp, lt, ltp, 0, Pt(rm_), Pt(bl_),
                                                Pt(gn_), None, None, Pt(ws), Pt(wt), Pt(S), Pt(T), scale, 0, None)

    bf = dict(dtype=_lib.BF16, Qs=qb, Ks=kb, Qt=qb, Kt=kb)
    for bad in (dict(dtype=7), dict(Qs=None), dict(Ks=None), dict(Qt=None), dict(Kt=None), dict(ws=None), dict(wt=None), dict(S=None), dict(T=None),
                dict(rm_=rm), dict(rm_=rm, bl_=bl), dict(bl_=bl, gn_=gn), dict(gn_=gn), dict(Bn=0), dict(heads=0), dict(heads=65), dict(dh=24),
                dict(dh=144), dict(nq=0), dict(ls=0), dict(lt=0), dict(lsp=63), dict(ltp=63), dict(Bn=40000), dict(scale=float("inf")),
                dict(scale=float("nan")), dict(bf, Qt=qb.view(-1)[4:]), dict(bf, Ks=kb.view(-1)[4:])):
        assert rc(**bad) == _lib.PMHIP_EINVAL, {k_: (v if not isinstance(v, torch.Tensor) else tuple(v.shape)) for k_, v in bad.items()}
    torch.cuda.synchronize()
    assert bool((os_ == sentinel).all()) and bool((ot_ == sentinel).all()), "a refused call wrote to an output"
    assert rc() == _lib.PMHIP_OK and rc(rm_=rm, bl_=bl, gn_=gn) == _lib.PMHIP_OK and rc(**bf) == _lib.PMHIP_OK
    torch.cuda.synchronize()
    assert torch.equal(os_, ones) and torch.equal(ot_, ones)


# ------------------------------------------------------------------------------------------------------------- region and blend

def region_scores(Bn, g, threshold, seed):
    """scores in (0.01, 0.5) under a maximum of 0.9 at token 0, with token 1 EXACTLY at float32(threshold) * max and token 2 one step
    below it, in both halves of every pair"""
    f = np.float32
    rng = np.random.default_rng([seed, g])
    s, u = rng.uniform(0.01, 0.5, (Bn, g * g)).astype(f), rng.uniform(0.01, 0.5, (Bn, g * g)).astype(f)
    cut = f(f(threshold) * f(0.9))
    for x in (s, u):
        x[:, 0], x[:, 1], x[:, 2] = f(0.9), cut, np.nextafter(cut, f(0))
    return s, u


@pytest.mark.parametrize("g", [4, 5, 32])
def test_phrase_region_is_the_numpy_rule(g):
    Bn = 3
    for threshold in (0.3, 0.5, 1.0):
        s, u = region_scores(Bn, g, threshold, 1)
        if threshold == 0.5:
            s[Bn - 1] = 0.0                                       # a zero row: its half of the mask is all true
        for grow in (0, 1, 3):
            got = n(ops.phrase_region(t(s), t(u), g, threshold, grow))
            want = R.region(s, u, g, threshold, grow)
            assert np.array_equal(got, want), (g, threshold, grow, np.argwhere(got != want)[:4].tolist())
            if grow == 0:
                assert want[0, :3].tolist() == [1, 1, 0] and 0 < want[0].sum() < g * g      # the tie is kept, the step below is not
        if threshold == 0.5:
            assert want[Bn - 1].all()
    frame = A.framed(Bn, g * g, ld=g * g, dtype=torch.uint8, device=dev())
    A.call("pmhip_phrase_region", t(s), t(u), frame, Bn, g, 0.3, 1)
    torch.cuda.synchronize()
    frame.assert_frame_untouched(f"phrase_region g={g}")
    assert np.array_equal(n(frame.payload()), R.region(s, u, g, 0.3, 1))
    for bad in (dict(threshold=0.0), dict(threshold=1.5), dict(grow=-1), dict(grow=1.5)):
        kw = dict(threshold=0.3, grow=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.phrase_region(t(s), t(u), g, **kw)
    lib = _lib.load()
    out = torch.full((Bn, g * g), 9, dtype=torch.uint8, device=dev())
    for a in ((None, t(u).data_ptr(), out.data_ptr(), Bn, g, 0.3, 1), (t(s).data_ptr(), t(u).data_ptr(), out.data_ptr(), Bn, 65, 0.3, 1),
              (t(s).data_ptr(), t(u).data_ptr(), out.data_ptr(), Bn, 0, 0.3, 1), (t(s).data_ptr(), t(u).data_ptr(), out.data_ptr(), 0, g, 0.3, 1),
              (t(s).data_ptr(), t(u).data_ptr(), None, Bn, g, 0.3, 1)):
        assert lib.pmhip_phrase_region(*a, None) == _lib.PMHIP_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 9).all())


def test_blend_tokens_is_exact_and_touches_nothing_else():
    Bn, N = 3, 1000                                               # (more than one workgroup, a ragged tail)
    rng = np.random.default_rng(5)
    mask = (rng.uniform(size=(Bn, N)) < 0.4).astype(np.uint8) * rng.integers(1, 255, (Bn, N)).astype(np.uint8)       # any non-zero byte keeps
    ints = lambda: rng.integers(0, 2 ** 40, (Bn, N)).astype(np.int64)
    ps, ms, pt, mt = ints(), ints(), ints(), ints()
    ss, st = rng.uniform(size=(Bn, N)).astype(np.float32), rng.uniform(size=(Bn, N)).astype(np.float32)
    want = R.blend(mask, ps, ms, ss, pt, mt, st)
    src = [t(ps), t(ms), t(ss)]
    frames = [A.framed(Bn, N, ld=N, dtype=x.dtype, payload=x) for x in (t(pt), t(mt), t(st))]
    A.call("pmhip_blend_tokens", t(mask), *src, *frames, Bn, N)
    torch.cuda.synchronize()
    for f, w, name in zip(frames, want, ("pred", "merged", "score")):
        f.assert_frame_untouched(f"blend_tokens {name}")
        assert np.array_equal(n(f.payload()), w), name
    assert np.array_equal(n(src[0]), ps) and np.array_equal(n(src[1]), ms) and np.array_equal(n(src[2]), ss)     # the source half is read only
    got = ops.blend_tokens(t(mask), *src, t(pt), t(mt), t(st))
    assert all(np.array_equal(n(g_), w) for g_, w in zip(got, want))
    assert 0 < int((mask != 0).sum()) < Bn * N
    with pytest.raises(ValueError):
        ops.blend_tokens(t(mask), *src, t(pt).int(), t(mt), t(st))
    with pytest.raises(ValueError):
        ops.blend_tokens(t(mask), *src, t(pt)[:, :9].contiguous(), t(mt), t(st))


# ------------------------------------------------------------------------------------------------------------- the engine entry

import ctypes as CT                                                              # noqa: E402
import math                                                                      # noqa: E402

from test_gpu_control import LENS_EDIT, LENS_SRC, TOL, _ctl, _near_tie_audit, cpu_pipe, data, in_dtype, tiny_pipe      # noqa: E402,F401
from test_local_blend_cpu import phrase_rows                                     # noqa: E402

DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
PAIRS = 2
# The float bar TOL grants the tower's activations -- the pre-softmax scores of a tapped layer among them -- an absolute error of TOL.
# A score error d moves every probability by a factor within exp(+-2 d) (numerator and denominator); blend in [0, 1], gain >= 0 and
# the weights >= 0 keep every term of the phrase score non-negative, so the phrase score moves by at most exp(2 TOL) - 1 of itself.
SCORE_REL = math.expm1(2 * TOL)


@DTYPES
def test_the_logits_are_those_of_the_entries_without_the_tap(tiny_pipe, data, dtype):
    tok, ctx, lens = data["tok"].to(dev()), data["ctx"].to(dev()), data["lens"]
    rows = phrase_rows()
    with in_dtype(tiny_pipe, dtype):
        eng = tiny_pipe.engine()
        count = eng.graph_count()
        first = eng.forward(tok, ctx, context_lens=lens)
        for cross, inject in (([0], []), ([1], [1]), ([0, 1], [0]), ([], [1])):
            kw = dict(cross_layers=cross, self_layers=inject, context_lens=lens, **(_ctl(data) if cross else {}))
            want = eng.forward_control(tok, ctx, **kw)
            for tapped in ([0], [1], [0, 1]):
                got, scores = eng.forward_control(tok, ctx, score_layers=tapped, score_weights=rows, **kw)
                assert torch.equal(got, want), (cross, inject, tapped)
                assert tuple(scores.shape) == (2 * PAIRS, tiny_pipe.num_tokens) and bool(torch.isfinite(scores).all()) and float(scores.min()) > 0
        got, scores = eng.forward_control(tok, ctx, context_lens=lens, score_layers=[0, 1], score_weights=rows)     # no control bits at all
        assert torch.equal(got, first)
        fin = torch.nan_to_num(ctx)
        got, _ = eng.forward_control(tok, fin, score_layers=[1], score_weights=rows)                                 # ... and without lengths
        assert torch.equal(got, eng.forward(tok, fin))
        twice = scores.clone()
        _, same = eng.forward_control(tok, ctx, context_lens=lens, score_layers=[0, 1], score_weights=rows, scores=twice)
        assert same.data_ptr() == twice.data_ptr() and float((twice - 2 * scores).abs().max()) <= 4 * 2.0 ** -23 * float(scores.max())
        assert torch.equal(eng.forward(tok, ctx, context_lens=lens), first)
        assert eng.graph_count() == count                                 # eager only: no key added to the graph cache


@DTYPES
def test_the_scores_are_the_operator_composition_and_the_cpu_branch(tiny_pipe, cpu_pipe, data, dtype):
    """fp32-verify: bit for bit the composition of ops.attention_phrase_score over the tapped layers (the operator-level
    CondTransformer.forward), and within SCORE_REL of the plain-torch branch; bf16 printed.  Counter-check: the weights of the other
    half miss the bar"""
    tok, ctx, lens = data["tok"].to(dev()), data["ctx"].to(dev()), data["lens"]
    rows = phrase_rows()
    with in_dtype(tiny_pipe, dtype):
        eng = tiny_pipe.engine()
        for cross, tapped in (([], [0, 1]), ([1], [0, 1]), ([0, 1], [1])):
            ctl = dict(cross_layers=cross, self_layers=[], **(_ctl(data) if cross else {}))
            _, got = eng.forward_control(tok, ctx, context_lens=lens, score_layers=tapped, score_weights=rows, **ctl)
            with torch.no_grad():
                _, comp = tiny_pipe.transformer(tok, ctx, context_lens=lens, control=dict(ctl, score_layers=tapped, score_weights=rows))
                _, want = cpu_pipe.transformer(data["tok"], data["ctx"], context_lens=lens, control=dict(ctl, score_layers=tapped, score_weights=rows))
                _, other = cpu_pipe.transformer(data["tok"], data["ctx"], context_lens=lens,
                                                control=dict(ctl, score_layers=tapped, score_weights=(rows[1], rows[0])))
            gap = float((got - comp).abs().max())
            ratio = float(((got.cpu() - want).abs() / (SCORE_REL * want)).max())
            miss = float(((got.cpu() - other).abs() / (SCORE_REL * want)).max())
            print(f"{dtype} cross={cross} tapped={tapped}: engine - composition {gap:.3e}; |GPU - CPU branch| / bound {ratio:.4f}; "
                  f"the other half's weights miss it by a factor of {miss:.1f}")
            if dtype == torch.float32:
                assert gap == 0.0 and ratio < 1.0 and miss > 1.0, (cross, tapped, gap, ratio, miss)


def test_the_scores_entry_validates_before_it_launches(tiny_pipe, data):
    eng = tiny_pipe.engine()
    tok, ctx = data["tok"].to(dev()).contiguous(), torch.nan_to_num(data["ctx"]).to(dev()).contiguous()
    L, N = ctx.shape[1], tiny_pipe.num_tokens
    sentinel = 12345.0
    logits = torch.full((2 * PAIRS, N, eng.n_embed), sentinel, device=dev())
    scores = torch.full((2 * PAIRS, N), sentinel, device=dev())
    i32p, f32p = CT.POINTER(CT.c_int), CT.POINTER(CT.c_float)
    count = eng.graph_count()
    w_src, w_edit = phrase_rows()
    as_p = lambda x, dt, p: None if x is None else np.ascontiguousarray(x, dt).ctypes.data_as(p)

    def call(lens=None, cross=1, inject=0, bits=3, ws=w_src, we=w_edit, out=scores, rm=data["rm"], bl=data["bl"], gn=data["gn"]):
        keep = [as_p(rm, np.int32, i32p), as_p(bl, np.float32, f32p), as_p(gn, np.float32, f32p), as_p(ws, np.float32, f32p), as_p(we, np.float32, f32p)]
        return eng.lib.pmhip_s2_forward_control_scores(eng.handle, tok.data_ptr(), ctx.data_ptr(), L, PAIRS,
                                                       None if lens is None else (CT.c_int * (2 * PAIRS))(*lens), cross, inject, keep[0], keep[1],
                                                       keep[2], bits, keep[3], keep[4], logits.data_ptr(), None if out is None else out.data_ptr(),
                                                       0, None)

    nan_w, neg_w, zero = w_src.copy(), w_edit.copy(), np.zeros_like(w_src)
    nan_w[1, 3], neg_w[0, 5] = float("nan"), -1.0
    behind = zero.copy()
    behind[:, 70:] = 1.0
    for kwargs, text in ((dict(bits=0), b"score_bits selects no layer"), (dict(bits=4), b"at or above depth=2"), (dict(ws=None), b"is NULL"),
                         (dict(we=None), b"is NULL"), (dict(out=None), b"is NULL"), (dict(ws=nan_w), b"finite and >= 0"),
                         (dict(we=neg_w), b"finite and >= 0"), (dict(ws=zero, we=zero), b"no row of the phrase"),
                         (dict(ws=behind, we=behind, lens=[77, 50, 60, 33]), b"pair 1: no row of the phrase"), (dict(cross=4), b"at or above depth=2"),
                         (dict(rm=None), b"required with cross_bits"), (dict(cross=0), b"refused without"), (dict(lens=[0, 1, 1, 1]), b"context length 0")):
        assert call(**kwargs) == _lib.PMHIP_EINVAL, kwargs
        msg = eng.lib.pmhip_last_error()
        assert b"s2_forward_control_scores" in msg and text in msg, (kwargs, msg)
    torch.cuda.synchronize()
    assert bool((logits == sentinel).all()) and bool((scores == sentinel).all())          # nothing was launched
    assert call() == _lib.PMHIP_OK and call(cross=0, inject=0, rm=None, bl=None, gn=None) == _lib.PMHIP_OK and \
        call(cross=3, inject=2, bits=2, lens=[L, 5, 1, 9], ws=behind * 0 + 1, we=w_edit) == _lib.PMHIP_OK
    torch.cuda.synchronize()
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(scores).all()) and not bool((scores == sentinel).any()) and eng.graph_count() == count
    for bad in (dict(score_layers=[2], score_weights=(w_src, w_edit)), dict(score_layers=[0]), dict(score_weights=(w_src, w_edit), cross_layers=[0], **_ctl(data)),
                dict(score_layers=[0], score_weights=(w_src, neg_w)), dict(score_layers=[0], score_weights=(w_src, w_edit), scores=torch.zeros(4, N)),
                dict(score_layers=[0, 0], score_weights=(w_src, w_edit))):
        with pytest.raises(ValueError):
            eng.forward_control(tok, ctx, **bad)
    # the tap is cleared on the error path too: a forward behind a failed call equals one before it
    before = eng.forward(tok, ctx)
    assert call(cross=4) == _lib.PMHIP_EINVAL
    assert torch.equal(eng.forward(tok, ctx), before)


# ------------------------------------------------------------------------------------------------------------- the loop

# The tiny tower's attention is nearly flat (a pair's scores span a factor of 1.5 over its 16 tokens), so a cut that decides something
# lies above 0.9 of the maximum.  NOISE_SEED and LOOP were chosen on the CPU, by a scan over seeds 1..8 and thresholds 0.80..0.99: with
# them no token's score lies within the bound of its cut at any of the three blended steps -- the closest is 2.24 bounds away -- and
# the regions hold 5 and 3 of 16 tokens.  The test asserts the condition again.
NOISE_SEED = 2
LOOP = dict(blend_threshold=0.96, blend_grow=0, blend_start=0.25)


def test_control_ids_with_blend_rows_against_the_cpu_branch_in_fp32(tiny_pipe, cpu_pipe, data):
    """fp32-verify, the same uniforms on both sides: the CPU branch's ids and region exactly.  Before that, two conditions on the inputs,
    met by the reference alone: at every blended step no token's float64 score lies within the derived bound of threshold * max
    (|s - t m| > SCORE_REL (s + t m): each side of the compare moves by at most SCORE_REL of itself), and the audit of
    tests/test_gpu_control.py finds no near-tie in the draw"""
    T, topk = 4, 3
    noise = torch.rand(T, PAIRS, tiny_pipe.num_tokens, tiny_pipe.mask_token_id, generator=torch.Generator().manual_seed(NOISE_SEED))
    ctx, rows = data["ctx"], phrase_rows()
    args = (LENS_SRC, LENS_EDIT, data["rm"], data["bl"], data["gn"], PAIRS, T, 1.0, topk, 9)
    seen, real = [], cpu_pipe._region_cpu
    cpu_pipe._region_cpu = lambda s, u, *a, **kw: (seen.append((s.double().numpy(), u.double().numpy())), real(s, u, *a, **kw))[1]
    try:
        want = cpu_pipe.control_ids(ctx[:PAIRS], ctx[PAIRS:], *args, cross_steps=0.75, noise=noise, blend_rows=rows, return_mask=True, **LOOP)
    finally:
        del cpu_pipe._region_cpu
    assert len(seen) == T - math.ceil(LOOP["blend_start"] * T)
    t_ = LOOP["blend_threshold"]
    closest = np.inf
    for step, halves in enumerate(seen):
        for s in halves:
            cut = t_ * s.max(1, keepdims=True)
            margin = np.abs(s - cut) / (SCORE_REL * (s + cut))
            closest = min(closest, float(margin.min()))
    print(f"the closest score to its cut: {closest:.2f} x the bound")
    assert closest > 1.0, "a token's score lies within the bound of threshold * max: choose another NOISE_SEED"
    ties = _near_tie_audit(tiny_pipe, cpu_pipe, data, noise, T, topk, ctl_steps=3)
    assert ties == 0, "a near-tie in the draw: choose another NOISE_SEED"
    got = tiny_pipe.control_ids(ctx[:PAIRS].to(dev()), ctx[PAIRS:].to(dev()), *args, cross_steps=0.75, noise=noise, blend_rows=rows, return_mask=True,
                                **LOOP)
    plain = cpu_pipe.control_ids(ctx[:PAIRS], ctx[PAIRS:], *args, cross_steps=0.75, noise=noise)
    assert torch.equal(plain[0], want[0]) and not torch.equal(plain[1], want[1])          # the blend moves the edited image
    assert 0 < int(want[2].sum()) < want[2].numel()
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]) and torch.equal(got[2].cpu(), want[2])


@DTYPES
def test_the_blend_identities_on_the_gpu(tiny_pipe, data, dtype):
    """ids_src is generate_ids on the source alone, bit for bit, whatever the blend; blend_mask all true is the call without a blend,
    all false makes ids_edit == ids_src"""
    pipe = tiny_pipe
    ctx = data["ctx"].to(dev())
    src, edit = ctx[:PAIRS].contiguous(), ctx[PAIRS:].contiguous()
    T, seed, N = 4, 7, pipe.num_tokens
    g = math.isqrt(N)
    rows = phrase_rows()
    with in_dtype(pipe, dtype):
        alone = pipe.generate_ids(src, PAIRS, T, 1.0, 3, [False] * T, seed, use_graph=False, streams=1, context_lens=LENS_SRC)[0]
        args = (src, edit, LENS_SRC, LENS_EDIT, data["rm"], data["bl"], data["gn"], PAIRS, T, 1.0, 3, seed)
        base = pipe.control_ids(*args, cross_steps=0.8)
        a, b, mask = pipe.control_ids(*args, cross_steps=0.8, blend_rows=rows, return_mask=True, **LOOP)
        assert torch.equal(a, alone) and torch.equal(base[0], alone) and tuple(mask.shape) == (PAIRS, g, g) and mask.dtype == torch.bool
        assert 0 < int(mask.sum()) < mask.numel() and tuple(b.shape) == tuple(a.shape)
        ones, zeros = torch.ones(PAIRS, g, g, dtype=torch.bool), torch.zeros(PAIRS, g, g, dtype=torch.bool)
        a1, b1 = pipe.control_ids(*args, cross_steps=0.8, blend_mask=ones)
        assert torch.equal(a1, alone) and torch.equal(b1, base[1])
        a0, b0, m0 = pipe.control_ids(*args, cross_steps=0.8, blend_mask=zeros, blend_start=0.0, return_mask=True)
        assert torch.equal(a0, alone) and torch.equal(b0, alone) and not bool(m0.any())
        ag, _ = pipe.control_ids(*args, guidance_scale=3.0, blend_rows=rows, **LOOP)
        assert torch.equal(ag, pipe.generate_ids(src, PAIRS, T, 1.0, 3, [False] * T, seed, use_graph=False, streams=1, context_lens=LENS_SRC,
                                                 guidance_scale=3.0)[0])
        ids_s, ids_e, img_s, img_e, m = pipe.control_ids(*args, blend_rows=rows, want_imgs=True, return_mask=True, **LOOP)
        assert torch.equal(ids_s, alone) and bool(torch.isfinite(img_e).all()) and img_e.shape[0] == PAIRS
