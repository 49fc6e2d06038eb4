"""The local blend on the CPU: the bound of tests/blend_ref.py against the float32 restatement of the kernels'
arithmetic, at the very inputs tests/test_gpu_local_blend.py runs -- the correct restatement stays below a stated fraction of the
bound, every named fault exceeds it -- and the exact family's expectation; the region rule on hand-written grids; then the CPU
branch of the model, the loop and the surface."""
import numpy as np
import pytest

import blend_ref as R
import control_ref as C

DHS = (64, 32)
HEADS_SIGMA = ((2, 2.0), (3, 8.0))                           # (heads, the scores' standard deviation)
SCALE_ACC = 0.5                                              # the scale of the accumulating launch (the other runs at 1)
# measured here, on the CPU, over every case below (the figures are in DESIGN.md 4zc): the f32 restatement reaches 0.0028 of the
# bound where the launch overwrites, 0.41 where it accumulates -- the bound grants that one addition 2^-23 of the stored value, a
# correctly rounded one errs by up to 2^-24 of it, half the grant, and the stored value dwarfs the rest of the bound
FRACTION = 0.01
FRACTION_ACCUMULATE = 0.55


def cases():
    for dh in DHS:
        for exp2 in (True, False):
            for Ls, Lt in R.SHAPES:
                for kind in R.LENS:
                    for H, sigma in HEADS_SIGMA:
                        for control in (True, False):
                            yield dh, exp2, Ls, Lt, kind, H, sigma, control


@pytest.fixture(scope="module")
def refs():
    """every case with its float64 reference: computed once, shared, never modified"""
    out = {}
    for key in cases():
        dh, exp2, Ls, Lt, kind, H, sigma, control = key
        d = R.case(Ls, Lt, dh, sigma, kind, H=H, control=control)
        out[key] = (d, R.reference(d, exp2))
    return out


def launches(d):
    """the two launches every case runs: (scale, into)"""
    B, _, nq, _ = d["qt"].shape
    return ((1.0, None), (SCALE_ACC, R.into_arrays(B, nq)))


def test_the_restatement_stays_below_a_fraction_of_the_bound(refs):
    worst = {}
    for key, (d, r) in refs.items():
        exp2 = key[1]
        for scale, into in launches(d):
            ratio, idx = R.worst(R.emulate(d, exp2, scale, into), R.expected(r, scale, into), R.bound(d, r, exp2, scale, into))
            worst[into is not None] = max(worst.get(into is not None, 0.0), ratio)
            assert ratio < (FRACTION if into is None else FRACTION_ACCUMULATE), (key, scale, idx, ratio)
    print("largest err / bound of the restatement by (accumulating):", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_named_fault_exceeds_the_bound(refs, fault):
    """in every case where the fault changes the arithmetic at all, under both launches"""
    least, n = np.inf, 0
    for key, (d, r) in refs.items():
        exp2 = key[1]
        for scale, into in launches(d):
            if not R.fault_applies(fault, d, into):
                continue
            ratio, idx = R.worst(R.emulate(d, exp2, scale, into, fault=fault), R.expected(r, scale, into), R.bound(d, r, exp2, scale, into))
            assert ratio > 1.0, (fault, key, scale, idx, ratio)
            least, n = min(least, ratio), n + 1
    print(f"{fault}: {n} cases, exceeds the bound by a factor of at least {least:.3g}")
    assert n >= 48, (fault, n)


def test_the_exact_family_is_exact():
    """the expectation is the same in both units and a multiple of 1/16, and the restatement meets it bit for bit, with and without
    control, overwriting and accumulating onto multiples of 1/16"""
    for Ls, Lt in R.SHAPES:
        for kind in R.LENS:
            for dh in DHS:
                for control in (True, False):
                    d = R.exact_case(Ls, Lt, dh, kind, control=control)
                    r = R.reference(d, True)
                    into = tuple(np.round(x * 16) / 16 for x in R.into_arrays(2, 80))
                    for scale, base in ((1.0, None), (0.5, into)):
                        want = R.expected(r, scale, base)
                        assert all(np.array_equal(a, c) for a, c in zip(want, R.expected(R.reference(d, False), scale, base)))
                        assert all(np.array_equal(x * 32, np.round(x * 32)) and np.abs(x).max() < 64 for x in want)
                        for exp2 in (True, False):
                            got = R.emulate(d, exp2, scale, base)
                            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (Ls, Lt, kind, dh, control, scale, exp2)
                    if Lt > 1:
                        assert r["ref_t"].max() > 0 and r["ref_s"].max() > 0


def test_the_inputs_reach_what_the_faults_need():
    d = R.case(77, 129, 32, 2.0, "one_mid")
    ns, nt = C.clamp(d["lens_s"], 2, 77), C.clamp(d["lens_t"], 2, 129)
    for b in range(2):
        assert (d["w_s"][b, ns[b]:] > 0).any() or ns[b] == 77         # weights behind a shortened length: dropped by a select
        assert (d["w_t"][b, nt[b]:] > 0).any() or nt[b] == 129
    assert (d["w_s"] == 0).mean() > 0.7 and set(np.unique(d["w_s"])) == {0.0, 0.5, 1.0} and set(np.unique(d["w_t"])) == {0.0, 1.0, 2.0}
    assert not np.array_equal(d["w_s"][0], d["w_s"][1]) and not np.array_equal(d["w_s"][:, :77], d["w_t"][:, :77])
    ksp, ktp = R.poison(d)
    for b in range(2):
        assert np.isfinite(ksp[b, :, :ns[b]]).all() and np.isnan(ksp[b, :, ns[b]:]).all()
        assert np.isfinite(ktp[b, :, :nt[b]]).all() and np.isnan(ktp[b, :, nt[b]:]).all()
    assert R.case(33, 17, 64, 2.0, "full", control=False)["row_map"] is None


# ------------------------------------------------------------------------------------------------------------- the region rule

def grid(rows):
    return np.array(rows, np.float32).reshape(1, -1)


def test_the_region_rule_on_hand_written_grids():
    z4 = np.zeros((1, 16), np.float32)
    corner = grid([[8, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]])
    # a corner: alone, grown once (clipped at the borders), grown over the whole grid; the other half adds nothing below its own cut
    assert R.region(corner, corner, 4, 0.5, 0).reshape(4, 4).tolist() == [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert R.region(corner, corner, 4, 0.5, 1).reshape(4, 4).tolist() == [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert R.region(corner, corner, 4, 0.5, 2).reshape(4, 4).tolist() == [[1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0], [0, 0, 0, 0]]
    assert R.region(corner, corner, 4, 0.5, 4).all() and R.region(corner, corner, 4, 0.5, 3).all()
    # the two halves are joined: the far corner comes from the other half, whose maximum is its own
    far = grid([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0.25]])
    assert R.region(corner, far, 4, 0.5, 0).reshape(4, 4).tolist() == [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]]
    # an edge on a 5 x 5 grid
    edge = np.zeros((5, 5), np.float32)
    edge[2, 4] = 3.0
    e1 = R.region(edge.reshape(1, 25), edge.reshape(1, 25), 5, 1.0, 1).reshape(5, 5)
    assert e1.tolist() == [[0] * 5, [0, 0, 0, 1, 1], [0, 0, 0, 1, 1], [0, 0, 0, 1, 1], [0] * 5]
    assert R.region(edge.reshape(1, 25), edge.reshape(1, 25), 5, 1.0, 5).all()
    # ties at the threshold: >= keeps a score equal to threshold * max; the product is ONE float32 rounding
    third = np.float32(0.3)
    top = np.float32(3.0)
    cut = np.float32(third * top)
    tie = grid([[top, cut, np.nextafter(cut, np.float32(0)), 0], [0] * 4, [0] * 4, [0] * 4])
    assert R.region(tie, tie, 4, 0.3, 0)[0, :4].tolist() == [1, 1, 0, 0]
    assert float(cut) != 0.3 * 3.0                                  # (the float64 product would draw the line elsewhere)
    # a zero row: 0 >= threshold * 0 everywhere
    assert R.region(z4, z4, 4, 0.3, 0).all() and R.region(z4, corner, 4, 0.5, 0).all()
    # more than one pair: each under its own maxima
    both = R.region(np.concatenate([corner, tie]), np.concatenate([corner, tie]), 4, 0.5, 0)
    assert both[0].tolist() == R.region(corner, corner, 4, 0.5, 0)[0].tolist() and both[1, :4].tolist() == [1, 0, 0, 0]


def test_the_token_blend_restated():
    mask = np.array([[1, 0, 0, 2]], np.uint8)
    a = R.blend(mask, np.array([[1, 2, 3, 4]]), np.array([[5, 6, 7, 8]]), np.array([[.1, .2, .3, .4]], np.float32),
                np.array([[9, 9, 9, 9]]), np.array([[7, 7, 7, 7]]), np.array([[.5, .5, .5, .5]], np.float32))
    assert a[0].tolist() == [[9, 2, 3, 9]] and a[1].tolist() == [[7, 6, 7, 7]] and a[2].tolist() == [[.5, np.float32(.2), np.float32(.3), .5]]


# ------------------------------------------------------------------------------------------------------------- the CPU branch

import math                                                                      # noqa: E402

import torch                                                                     # noqa: E402

from paintmind_amd.generate import Pipeline                                      # noqa: E402
from paintmind_amd.modules.encoder import T5TextEmbedder                         # noqa: E402
from test_control_cpu import LENS_EDIT, LENS_SRC, PAIRS, CharTokenizer, _tiny, pair_case      # noqa: E402
from text_stubs import tiny_t5                                                   # noqa: E402


@pytest.fixture(scope="module")
def pipe():
    return _tiny()


def phrase_rows(L=77):
    """the phrase's rows of the two halves: a run of ones each (pair 1's source run partly behind its length 50), one row of 1/2"""
    w_src, w_edit = np.zeros((PAIRS, L), np.float32), np.zeros((PAIRS, L), np.float32)
    w_src[0, 3:7], w_src[1, 47:53], w_edit[0, 5:8], w_edit[1, 2:4], w_edit[1, 30] = 1.0, 1.0, 1.0, 1.0, 0.5
    return w_src, w_edit


def test_the_region_twin_is_the_rule_of_phrase_mask_and_the_numpy_restatement():
    rng = np.random.default_rng(3)
    for g in (4, 5):
        s, u = rng.uniform(0, 1, (3, g * g)).astype(np.float32), rng.uniform(0, 1, (3, g * g)).astype(np.float32)
        s[:, 0], s[:, 1], s[:, 2] = 3.0, np.float32(np.float32(0.3) * np.float32(3.0)), np.nextafter(np.float32(np.float32(0.3) * np.float32(3.0)), np.float32(0))
        u[2] = 0.0
        for threshold in (0.3, 0.5, 1.0):
            for grow in (0, 1, g):
                got = Pipeline._region_cpu(torch.from_numpy(s), torch.from_numpy(u), g, threshold, grow)
                assert np.array_equal(got.numpy().astype(np.uint8), R.region(s, u, g, threshold, grow)), (g, threshold, grow)
        # phrase_mask's torch rule on one score, verbatim
        score = torch.from_numpy(s).reshape(3, g, g)
        mask = score >= 0.3 * score.amax(dim=(1, 2), keepdim=True)
        mask = torch.nn.functional.max_pool2d(mask[:, None].float(), 3, stride=1, padding=1)[:, 0] > 0
        low = np.full_like(s, -1.0)                                # the other half adds nothing: only its own maximum passes its cut,
        low[:, 0] = 1.0                                            # and that sits on the first half's maximum, token 0
        assert np.array_equal(R.region(s, low, g, 0.3, 1).reshape(3, g, g), mask.numpy().astype(np.uint8))
    a = Pipeline._blend_cpu(torch.tensor([[True, False]]), (torch.tensor([[1, 2]]), torch.tensor([[3, 4]]), torch.tensor([[.1, .2]])),
                            (torch.tensor([[5, 6]]), torch.tensor([[7, 8]]), torch.tensor([[.3, .4]])))
    assert a[0].tolist() == [[5, 2]] and a[1].tolist() == [[7, 4]] and torch.equal(a[2], torch.tensor([[.3, .2]]))


def test_the_cpu_branch_is_the_formula_from_each_tapped_layers_input(pipe):
    """an independent float64 restatement of the two scores from each tapped layer's own input (seen by wrapping attn2.run per
    instance) and its weights, under control in layer 1 and without in layer 0; the logits are those of the call without the tap"""
    src, edit, rm, bl, gn = pair_case(pipe)
    ctx, lens = torch.cat([src, edit]), LENS_SRC + LENS_EDIT
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, pipe.mask_token_id, (2 * PAIRS, pipe.num_tokens), generator=g)
    ids[torch.rand(2 * PAIRS, pipe.num_tokens, generator=g) < 0.5] = pipe.mask_token_id
    tok = pipe.ids2tokens(ids)
    tr = pipe.transformer
    w_src, w_edit = phrase_rows()
    seen = {}

    def tap(i, attn):
        run = attn.run
        def wrapped(x, context=None, residual=None, **kw):
            seen[i] = (x.detach().clone(), context.detach().clone(), dict(kw))
            return run(x, context, residual=residual, **kw)
        attn.run = wrapped

    for i, layer in enumerate(tr.layers):
        tap(i, layer.attn2)
    ctl = dict(row_map=rm, blend=bl, gain=gn, cross_layers=[1])
    try:
        with torch.no_grad():
            plain = tr(tok, ctx, context_lens=lens, control=ctl)
            got, scores = tr(tok, ctx, context_lens=lens, control=dict(ctl, score_layers=[0, 1], score_weights=(w_src, w_edit)))
            none, only = tr(tok, ctx, context_lens=lens, control=dict(score_layers=[1], score_weights=(w_src, w_edit)))
            again, twice = tr(tok, ctx, context_lens=lens, control=dict(ctl, score_layers=[0, 1], score_weights=(w_src, w_edit), scores=scores))
    finally:
        for layer in tr.layers:
            del layer.attn2.run
    assert torch.equal(got, plain) and torch.equal(again, plain) and torch.equal(none, tr(tok, ctx, context_lens=lens))
    assert tuple(scores.shape) == (2 * PAIRS, pipe.num_tokens) and scores.dtype == torch.float32
    f8 = lambda t: t.double().numpy()

    def heads(attn, x, w):
        y = f8(x) @ f8(w.detach()).T
        return y.reshape(y.shape[0], y.shape[1], attn.heads, attn.dim_head).transpose(0, 2, 1, 3)

    def softmax(s):
        e = np.exp(s - s.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)

    want = np.zeros((2 * PAIRS, pipe.num_tokens))
    live = np.arange(77)[None, :] < np.asarray(lens)[:, None]
    for i, layer in enumerate(tr.layers):
        x, c, kw = seen[i]
        a = layer.attn2
        assert kw.get("score") is not None and (kw.get("control") is not None) == (i == 1)
        q, k = heads(a, x, a.to_q.weight) * a.scale, heads(a, torch.nan_to_num(c), a.to_k.weight)
        p = softmax(np.where(live[:, None, None, :], q @ k.transpose(0, 1, 3, 2), -np.inf))
        P = p.copy()
        for b in range(PAIRS):
            for j in range(LENS_EDIT[b]):
                m, w = int(rm[b, j]), float(bl[b, j])
                pj = p[PAIRS + b, :, :, j]
                if i == 1:
                    if 0 <= m < LENS_SRC[b] and w != 0:
                        pj = (1 - w) * pj + w * p[b, :, :, m]
                    pj = float(gn[b, j]) * pj
                P[PAIRS + b, :, :, j] = pj
        wts = np.concatenate([w_src, w_edit]).astype(np.float64)
        want += 0.5 * (P * wts[:, None, None, :]).sum(-1).mean(1)
        if i == 1:                                                                # (the last layer: its input does not depend on its own control)
            want_only = (p * wts[:, None, None, :]).sum(-1).mean(1)
    err = float(np.abs(f8(scores) - want).max())
    print(f"phrase scores, CPU branch against the float64 restatement: {err:.3e} of at most {want.max():.3f}")
    assert err < 1e-6 and want.max() > 0.01
    assert float((twice - 2 * scores).abs().max()) < 1e-6                         # `scores=` is added to
    assert float(np.abs(f8(only) - want_only).max()) < 1e-6                       # one layer, no control: scale 1, P = pt
    for bad in (dict(score_layers=[2], score_weights=(w_src, w_edit)), dict(score_layers=[0]), dict(score_weights=(w_src, w_edit)),
                dict(score_layers=[0], score_weights=(w_src, -w_edit)), dict(score_layers=[0], score_weights=(w_src[:, :76], w_edit)),
                dict(score_layers=[0], score_weights=(np.zeros_like(w_src), np.zeros_like(w_edit))),
                dict(score_layers=[0], score_weights=(w_src, w_edit), scores=torch.zeros(3, 16)),
                dict(score_layers=[0], score_weights=(w_src * float("nan"), w_edit))):
        with pytest.raises(ValueError):
            tr(tok, ctx, context_lens=lens, control=bad)
    behind = np.zeros_like(w_src)
    behind[:, 70:] = 1.0                                                          # every weight behind the lengths 50 / 33 of pair 1
    with pytest.raises(ValueError, match="pair 1"):
        tr(tok, ctx, context_lens=lens, control=dict(score_layers=[0], score_weights=(behind, behind)))


def test_control_ids_with_a_local_blend_on_the_cpu(pipe):
    """the invariants of ``control_ids``, step by step, by wrapping the two halves of the tail: the source half is the plain loop; at every
    blended step the edited half's (pred, merged, score) equal the source half's outside the region; the all-true and all-false masks.
    (The tiny tower's attention is nearly flat -- a pair's scores span a factor of 1.5 --, so the threshold that decides something
    here is 0.9.)"""
    src, edit, rm, bl, gn = pair_case(pipe)
    T, seed, N = 5, 7, pipe.num_tokens
    g = int(math.isqrt(N))
    args = (src, edit, LENS_SRC, LENS_EDIT, rm, bl, gn, PAIRS, T, 1.0, 3, seed)
    rows = phrase_rows()
    plain = pipe.control_ids(*args, cross_steps=0.8)
    draws, remasks, regions = [], [], []
    real_draw, real_remask, real_region = pipe._draw_cpu, pipe._remask_cpu, pipe._region_cpu
    keep = lambda d: tuple(x.clone() if isinstance(x, torch.Tensor) else x for x in d)       # (the re-masking works in place on `merged`)
    pipe._draw_cpu = lambda *a, **kw: (lambda d: (draws.append(keep(d)), d)[1])(real_draw(*a, **kw))
    pipe._remask_cpu = lambda ids, scores, *a, **kw: (remasks.append((ids.clone(), scores.clone())), real_remask(ids, scores, *a, **kw))[1]
    pipe._region_cpu = lambda *a, **kw: (regions.append(real_region(*a, **kw)), regions[-1])[1]
    try:
        a, b, mask = pipe.control_ids(*args, cross_steps=0.8, blend_rows=rows, blend_threshold=0.9, blend_grow=0, blend_start=0.4, return_mask=True)
    finally:
        del pipe._draw_cpu, pipe._remask_cpu, pipe._region_cpu
    start = math.ceil(0.4 * T)
    assert torch.equal(a, plain[0]) and len(draws) == 2 * T and len(remasks) == 2 * T and len(regions) == T - start
    assert tuple(mask.shape) == (PAIRS, g, g) and mask.dtype == torch.bool and torch.equal(mask.reshape(PAIRS, N), regions[-1])
    assert 0 < int(mask.sum()) < mask.numel()                                     # (the case decides something)
    decided = 0
    for step in range(T):
        (pred_s, merged_s, score_s, _), (pred_e, merged_e, score_e, _) = draws[2 * step], draws[2 * step + 1]
        (ms, ss), (me, se) = remasks[2 * step], remasks[2 * step + 1]
        assert torch.equal(ms, merged_s) and torch.equal(ss, score_s)             # the source half never reads the edited half
        if step < start:
            assert torch.equal(me, merged_e) and torch.equal(se, score_e)
            continue
        out = ~regions[step - start]
        assert torch.equal(me[out], merged_s[out]) and torch.equal(se[out], score_s[out])          # outside: the source's, bit for bit
        assert torch.equal(me[~out], merged_e[~out]) and torch.equal(se[~out], score_e[~out])      # inside: untouched
        decided += int((merged_e[out] != merged_s[out]).sum())
    assert decided > 0                                                            # the blend changed tokens
    # the masks that are drawn
    ones, zeros = torch.ones(PAIRS, g, g, dtype=torch.bool), torch.zeros(PAIRS, g, g, dtype=torch.bool)
    a1, b1 = pipe.control_ids(*args, cross_steps=0.8, blend_mask=ones)
    assert torch.equal(a1, plain[0]) and torch.equal(b1, plain[1])
    a0, b0, m0 = pipe.control_ids(*args, cross_steps=0.8, blend_mask=zeros, blend_start=0.0, return_mask=True)
    assert torch.equal(a0, plain[0]) and torch.equal(b0, a0) and not m0.any()
    ids_s, ids_e, img_s, img_e, m = pipe.control_ids(*args, blend_rows=rows, want_imgs=True, return_mask=True)
    assert torch.equal(ids_s, plain[0]) and torch.isfinite(img_e).all() and tuple(m.shape) == (PAIRS, g, g)
    ag, bg = pipe.control_ids(*args, guidance_scale=3.0, blend_rows=rows)         # guidance composes; its second pass is never tapped
    assert torch.equal(ag, pipe.control_ids(*args, guidance_scale=3.0)[0])
    for bad in (dict(blend_rows=rows, blend_mask=ones), dict(return_mask=True), dict(blend_rows=rows, blend_threshold=0.0),
                dict(blend_rows=rows, blend_grow=-1), dict(blend_rows=rows, blend_start=1.0), dict(blend_rows=(rows[0],)),
                dict(blend_rows=(rows[0], -rows[1])), dict(blend_mask=ones[:1]), dict(blend_mask=ones.float()),
                dict(blend_rows=(np.zeros_like(rows[0]), np.zeros_like(rows[1])))):
        with pytest.raises(ValueError):
            pipe.control_ids(*args, **bad)


def test_prompt_to_prompt_with_a_local_blend_end_to_end_on_the_cpu():
    t5 = _tiny(text_model=T5TextEmbedder(tokenizer=CharTokenizer(), transformer=tiny_t5(), max_length=24))
    calls = []
    control_ids = t5.control_ids
    t5.control_ids = lambda *a, **kw: (calls.append((a, kw)), control_ids(*a, **kw))[1]
    text, edit = ["a red barn", "the cow"], ["a red church", "the big cow"]
    kw = dict(mode="replace", reweight={"church": 2.0, "big": 0.5}, timesteps=3, seed=5)
    S, g = t5.image_size, t5.image_size // t5.patch_size
    img_s, img_e, mask = t5.prompt_to_prompt(text, edit, local_blend=[("barn", "church"), "cow"], return_mask=True, **kw)
    assert tuple(img_s.shape) == tuple(img_e.shape) == (2, 3, S, S) and torch.isfinite(img_e).all() and tuple(mask.shape) == (2, g, g)
    a, k = calls[-1]
    w_src, w_edit = k["blend_rows"]
    assert w_src[0].nonzero()[0].tolist() == [6, 7, 8, 9] and w_edit[0].nonzero()[0].tolist() == [6, 7, 8, 9, 10, 11]      # barn / church
    assert w_src[1].nonzero()[0].tolist() == [4, 5, 6] and w_edit[1].nonzero()[0].tolist() == [8, 9, 10]                   # cow in both prompts
    assert a[6][0].tolist() == [1.0] * 6 + [2.0] * 6 + [1.0] * 12 and a[6][1].tolist() == [1.0] * 4 + [0.5] * 3 + [1.0] * 17   # the gains stay
    assert k["blend_threshold"] == 0.3 and k["blend_grow"] == 1 and k["blend_start"] == 0.2 and k["return_mask"] is True
    ids_s, ids_e = t5.prompt_to_prompt(text, edit, local_blend=[("barn", "church"), "cow"], return_ids=True, **kw)
    base_s, base_e = t5.prompt_to_prompt(text, edit, return_ids=True, **kw)
    assert torch.equal(ids_s, base_s) and tuple(ids_e.shape) == tuple(base_e.shape)
    # one phrase for all: the phrase in whichever prompt has it
    t5.prompt_to_prompt(["a cow", "the cow"], ["a big cow", "the dog"], local_blend="cow", return_ids=True, timesteps=2, seed=1)
    w_src, w_edit = calls[-1][1]["blend_rows"]
    assert w_src.sum(1).tolist() == [3.0, 3.0] and w_edit.sum(1).tolist() == [3.0, 0.0]
    # the phrase that is a reweight phrase too keeps its gain
    t5.prompt_to_prompt("a red barn", "a red church", reweight={"church": 2.0}, local_blend="church", return_ids=True, timesteps=2, seed=1)
    a, k = calls[-1]
    assert k["blend_rows"][0].sum() == 0 and k["blend_rows"][1][0].nonzero()[0].tolist() == [6, 7, 8, 9, 10, 11] and a[6][0, 6:12].tolist() == [2.0] * 6
    # a drawn mask
    ones = torch.ones(2, g, g, dtype=torch.bool)
    d_s, d_e = t5.prompt_to_prompt(text, edit, blend_mask=ones, return_ids=True, **kw)
    assert torch.equal(d_s, base_s) and torch.equal(d_e, base_e)
    for bad in (dict(local_blend="zebra"), dict(local_blend=("church", "barn")), dict(local_blend=["cow"]), dict(local_blend=3),
                dict(local_blend="barn", blend_mask=ones), dict(return_mask=True), dict(local_blend="barn", blend_threshold=2.0),
                dict(local_blend="r"), dict(local_blend=("barn", "red chu")), dict(local_blend="barn", negative_text=["x", "y"])):
        with pytest.raises(ValueError):
            t5.prompt_to_prompt(text, edit, **dict(kw, **bad))
    with pytest.raises(ValueError, match="no tokens below max_length"):
        t5.prompt_to_prompt("a" * 30 + " barn", "a" * 30 + " barn", local_blend="barn", timesteps=2, seed=1)
