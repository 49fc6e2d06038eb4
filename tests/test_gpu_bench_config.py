"""Correctness gates for the configuration bench.py times: bf16 compute, the decode loop replayed as a hipGraph, three
free-running micro-batch lanes, at the bench's full size (BASELINE.json configs[2]: vit-s-vqgan + 12L/d512, B=64, T=8;
and the north_star model 24L/d768 + 77x768 context at B=32).

(a) bf16 against fp32-verify on one full-size forward from the golden ids0 (reference generate.py:162):
    the bf16 logits must stay within a stated distance of the fp32 logits (which are themselves pinned to the
    reference's golden logits at 1e-3 in test_gpu_model.py), and a top-1 flip may only happen where the fp32 top-2
    gap is smaller than twice that distance.
(b) the exact timed path -- use_graph=True, streams=2 (and 3, the earlier default) -- must be BIT-identical, ids and every decoded image, to the
    eager single-stream loop in the same dtype, for two seeds (reference generate.py:183-198 has one code path; ours has
    three and they must agree)."""
import numpy as np
import pytest
import torch

import paintmind_amd as pm
from gpu_common import dev, n, t
from paintmind_amd.config import ver2cfg
from paintmind_amd.generate import Pipeline
from util import load_golden

pytestmark = pytest.mark.gpu

# measured on MI355X (round 2): max |bf16 - fp32| logit 0.0112, mean 0.00195, min row cosine 0.99997, top-1 agreement 0.990
# (logits std 0.32, median top-2 gap 0.025); asserted with ~2x head-room
BF16_LOGIT_MAXERR = 0.025
BF16_LOGIT_MEANERR = 0.004
BF16_ROW_COSINE = 0.9999


@pytest.fixture(scope="module")
def pipe512():
    torch.manual_seed(0)
    return Pipeline(pm.Config(ver2cfg["bench-uncond-12L-d512"]), stage1_pretrained=False).to(dev()).eval()


def test_bf16_one_step_against_fp32_verify_full_size(pipe512):
    """bf16 mode against fp32-verify on the 12L/d512 transformer.  Error thresholds are evaluated on the golden image as in
    rounds 1-2; the top-1 agreement is a COUNT statistic (a row flips when its fp32 top-2 gap is inside the bf16 noise: about
    1.8 % of the rows of this random-weight model) and is evaluated over 16 images -- on the golden image alone (1024 rows) its
    standard deviation is 0.004, so a 0.98 bar sat half a sigma from the mean of every arrangement (fp32 stream 0.9811,
    hi/lo 0.9819, hi/lo + fold 0.9823 over 16 images, tools/fold_accuracy_probe.py) and passed or failed by the draw."""
    pipe = pipe512
    _, d = load_golden("full_stage2.npz")
    ids0 = t(d["ids0"].astype(np.int64))
    g = torch.Generator().manual_seed(7)
    more = torch.randint(0, 8192, (15, ids0.shape[1]), generator=g)
    more[torch.rand(15, ids0.shape[1], generator=g) < 0.5] = pipe.mask_token_id
    ids16 = torch.cat([ids0, more.to(dev())])
    tok = pipe.ids2tokens(ids16)
    l32 = torch.cat([pipe.tokens2logits(tok[i:i + 4], None) for i in range(0, 16, 4)])
    pipe.set_compute_dtype(torch.bfloat16)
    try:
        l16 = pipe.tokens2logits(tok, None)
        ids_b, img16 = pipe.sample(ids0, np.float64(0.4), text=None, topk=1, temperature=1.0)
    finally:
        pipe.set_compute_dtype(torch.float32)
    ids_f, img32 = pipe.sample(ids0, np.float64(0.4), text=None, topk=1, temperature=1.0)
    err = (l16 - l32).abs()
    cos = torch.nn.functional.cosine_similarity(l16, l32, dim=-1)
    a16, a32 = l16.argmax(-1), l32.argmax(-1)
    top2 = torch.topk(l32, 2, dim=-1).values
    gap = (top2[..., 0] - top2[..., 1])
    flips = a16 != a32
    agree = 1.0 - float(flips.float().mean())
    print(f"bf16 vs fp32 logits over 16 images: max err {float(err.max()):.5f} (golden image {float(err[:1].max()):.5f}) mean err {float(err.mean()):.6f} "
          f"row cosine min {float(cos.min()):.6f} top-1 agreement {agree:.4f} (golden image {1.0 - float(flips[:1].float().mean()):.4f}) "
          f"img mean abs dev {float((img16 - img32).abs().mean()):.5f} ids agreement {float((ids_b == ids_f).float().mean()):.4f}")
    assert float(err.max()) < BF16_LOGIT_MAXERR and float(err.mean()) < BF16_LOGIT_MEANERR
    assert float(cos.min()) > BF16_ROW_COSINE and agree >= 0.975
    # a flip needs the two candidates closer than the two errors combined
    assert bool((gap[flips] < 2 * BF16_LOGIT_MAXERR).all())
    # and with this error level at most the rows whose gap is inside the noise may flip
    assert int(flips.sum()) <= int((gap < 2 * float(err.max())).sum())


@pytest.mark.parametrize("name,B,L", [("bench-uncond-12L-d512", 64, None), ("bench-text-24L-d768", 32, 77)])
def test_timed_path_graph_and_lanes_bit_identical_to_eager(name, B, L, pipe512):
    T = 8
    if name == "bench-uncond-12L-d512":
        pipe = pipe512
    else:
        torch.manual_seed(0)
        pipe = Pipeline(pm.Config(ver2cfg[name]), stage1_pretrained=False).to(dev()).eval()
    ctx = None
    if L is not None:
        ctx = torch.randn(B, L, ver2cfg[name]["context_dim"], generator=torch.Generator().manual_seed(1234)).to(dev())
    flags = [True] * T
    pipe.set_compute_dtype(torch.bfloat16)
    try:
        eager = {}
        for seed in (1000, 1001):
            ids, imgs = pipe.generate_ids(ctx, B, T, 1.0, 5, flags, seed=seed, use_graph=False, streams=1)
            eager[seed] = (ids.clone(), imgs.clone())
            assert torch.isfinite(imgs).all() and int((ids == pipe.mask_token_id).sum(1).max()) == 1
        assert not torch.equal(eager[1000][0], eager[1001][0])
        for lanes in (2, 3):                                   # 2 = what bench.py times (lanes of B/2 + 1 and B/2 - 1 images); 3 = round-2 default
            for seed in (1000, 1001, 1000, 1001):              # eager warm-up of the graph path, capture, two replays
                ids, imgs = pipe.generate_ids(ctx, B, T, 1.0, 5, flags, seed=seed, use_graph=True, streams=lanes)
                torch.cuda.synchronize()
                assert torch.equal(ids, eager[seed][0]), (name, lanes, seed, float((ids != eager[seed][0]).float().mean()))
                assert torch.equal(imgs, eager[seed][1]), (name, lanes, seed)
    finally:
        pipe.set_compute_dtype(torch.float32)


def test_cfg5_per_gpu_share_b64_properties_and_timed_path():
    """BASELINE configs[4] at its per-GPU share (vit-b-vqgan-512 + 24L/d1024, 77 x 768 context, B = 64), bf16, under pytest
    (only bench.py's self_check ran this size).  Property checks as test_full_vit_s_batch64_properties: finite,
    clamped, one residual mask token per image, and an image's result does not depend on the batch it rides in (B = 2 with the
    same seed and image base == the first two of B = 64, Philox keyed by the global image index); then the exact timed path --
    graph replay + two lanes -- is bit-identical to the eager single-stream loop.  T = 6 keeps it to a few seconds; the loop
    body is the T = 18 one."""
    name, B, T, L = "bench-text-24L-d1024-512px", 64, 6, 77
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(ver2cfg[name]), stage1_pretrained=False).to(dev()).eval()
    ctx = torch.randn(B, L, ver2cfg[name]["context_dim"], generator=torch.Generator().manual_seed(1234)).to(dev())
    flags = [False] * (T - 2) + [True, True]
    pipe.set_compute_dtype(torch.bfloat16)
    try:
        from paintmind_amd import ops
        ops.attention_fallbacks(reset=True)
        ids, imgs = pipe.generate_ids(ctx, B, T, 1.0, 5, flags, seed=77, use_graph=False, streams=1)
        ids, imgs = ids.clone(), imgs.clone()
        assert imgs.shape == (2, B, 3, 512, 512) and torch.isfinite(imgs).all() and float(imgs.abs().max()) <= 1.0
        assert ((ids == pipe.mask_token_id).sum(1) == 1).all() and int(ids.max()) <= pipe.mask_token_id and int(ids.min()) >= 0
        assert ops.attention_fallbacks() == 0
        ids2, imgs2 = pipe.generate_ids(ctx[:2].contiguous(), 2, T, 1.0, 5, flags, seed=77, use_graph=False, streams=1)
        assert torch.equal(ids2, ids[:2]) and torch.equal(imgs2, imgs[:, :2])
        for rep in range(3):                                   # eager warm-up of the graph path, capture, replay
            g_ids, g_imgs = pipe.generate_ids(ctx, B, T, 1.0, 5, flags, seed=77, use_graph=True, streams=2)
            torch.cuda.synchronize()
            assert torch.equal(g_ids, ids) and torch.equal(g_imgs, imgs), rep
    finally:
        pipe.set_compute_dtype(torch.float32)


def test_concurrent_lanes_are_deterministic_at_dim_1024():
    """Three lanes running the stage-2 forward concurrently must reproduce their sequential results bit for bit.
    dim 1024 / 16 heads is the shape whose LayerNorm lost rows (1 % of forwards) before the wave reductions moved from
    ds_bpermute to DPP: tools/lane_race_stress.py.  600 concurrent forwards here."""
    cfg = dict(ver2cfg["bench-text-24L-d768"], dim=1024, num_head=16, mlp_dim=4096, depth=2, context_dim=1024)
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(cfg), stage1_pretrained=False).to(dev()).eval()
    pipe.set_compute_dtype(torch.bfloat16)
    lanes = pipe._lanes(3)
    g = torch.Generator().manual_seed(3)
    toks = [torch.randn(2, 1024, 32, generator=g).to(dev()) for _ in range(3)]
    torch.cuda.synchronize()
    ref = [lanes[i][0].forward(toks[i], None).clone() for i in range(3)]
    torch.cuda.synchronize()
    bad = 0
    for rep in range(200):
        res = []
        for i, (e, v, st) in enumerate(lanes):
            with torch.cuda.stream(st):
                res.append(e.forward(toks[i], None))
        torch.cuda.synchronize()
        bad += sum(int(not torch.equal(a, b)) for a, b in zip(res, ref))
    assert bad == 0, f"{bad} / 600 concurrent forwards differ from the sequential result"


def test_operator_kernels_are_deterministic_under_concurrent_lanes():
    """The Section-4a corruption (a LayerNorm row short of a lane's partial sum, only with other kernels co-resident on
    the CU) was found by a bench self-check, not by a test.  This is the test: every kernel family of the decode loop
    -- attention (self, and the ragged 77-key cross form), the two-workgroups-per-CU residual GEMM, the 256x256 GEMMs
    (head split, SwiGLU, plain), LayerNorm, the sampling kernel and the re-mask sort -- at the dim-1024 / 16-head /
    512-px shapes runs on three streams at once, each stream a different kernel mix, 60 rounds; every result must be
    bit-identical to the same call on an idle device."""
    from paintmind_amd import ops
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dev())
    B, H, N, D = 4, 16, 1024, 1024
    M = B * N
    q = rnd(B, H, N, 64, scale=0.6).to(bf); k = rnd(B, H, N, 64).to(bf); vt = rnd(B, H, 64, N).to(bf)
    kc = rnd(B, H, 128, 64).to(bf); vtc = rnd(B, H, 64, 128).to(bf)                      # context of 77 keys, padded to 128
    x = rnd(M, D); a = rnd(M, D, scale=0.5).to(bf)
    wo = rnd(D, D, scale=D ** -0.5).to(bf); bo = rnd(D)
    wqkv = rnd(3 * D, D, scale=D ** -0.5).to(bf)
    w12 = rnd(2 * 2752, D, scale=D ** -0.5).to(bf); b12 = rnd(2 * 2752)
    gamma, beta = 1 + 0.1 * rnd(D), 0.1 * rnd(D)
    logits = rnd(2048, 8192)
    ids = torch.randint(0, 8192, (2048,), generator=torch.Generator().manual_seed(5)).to(dev())
    ids[::2] = 8192
    scores = rnd(2, 1024)

    def work(i):
        out = []
        if i == 0:
            out.append(ops.attention(q, k, vt, N, use_exp2=True))
            out.append(ops.gemm(a, wo, bias=bo, residual=x, out_dtype=torch.float32))      # K = 1024 residual GEMM: 256x256 kernel
            out.append(ops.layernorm(x, gamma, beta, out_dtype=bf))
            out += list(ops.sample_rows(logits, ids, 8192, 5, 0.7, seed=3, step=2))
        elif i == 1:
            out += list(ops.gemm_heads(a, wqkv, H, N, [ops.PART_Q, ops.PART_K, ops.PART_V], 0.125))
            out.append(ops.attention(q, kc, vtc, 77, use_exp2=True))
            out.append(ops.gemm(a[:, :512].contiguous(), wo[:, :512].contiguous(), bias=bo, residual=x, out_dtype=torch.float32))   # K = 512: gemm2b
            r = ids.reshape(2, 1024).clone()
            out.append(ops.remask(r, scores, 300, 8192))
        else:
            out.append(ops.gemm_swiglu(a, w12, b12))
            out.append(ops.layernorm(x, gamma, beta, out_dtype=bf))
            out.append(ops.attention(q, k, vt, N, use_exp2=True))
            out.append(ops.gemm(a, wqkv[: 2 * D].contiguous(), out_dtype=bf))
        return out

    ref = [work(i) for i in range(3)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(3)]
    bad = []
    for rep in range(60):
        res = []
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                res.append(work((i + rep) % 3))
        torch.cuda.synchronize()
        for i in range(3):
            for j, (got, want) in enumerate(zip(res[i], ref[(i + rep) % 3])):
                if not torch.equal(got, want):
                    bad.append((rep, (i + rep) % 3, j))
    assert not bad, f"{len(bad)} results differ under concurrency, first {bad[:5]}"


@pytest.mark.parametrize("name,B,T,L", [("bench-text-24L-d768", 8, 12, 77), ("bench-text-24L-d1024-512px", 8, 18, 77)])
def test_configs_4_and_5_graph_and_lanes_bit_identical_to_eager(name, B, T, L):
    """BASELINE configs[3] (T = 12) and configs[4] (vit-b 512 px, d1024, T = 18) at their full step counts, B = 8: segment
    graphs + two / three lanes against the eager single-stream loop, ids and every decoded image bit for bit
    (reference generate.py:183-198: one code path)."""
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(ver2cfg[name]), stage1_pretrained=False).to(dev()).eval()
    ctx = torch.randn(B, L, ver2cfg[name]["context_dim"], generator=torch.Generator().manual_seed(1234)).to(dev())
    flags = [step % 2 == 0 for step in range(T)]                # the reference's default save_interval
    pipe.set_compute_dtype(torch.bfloat16)
    try:
        eager = {}
        for seed in (7, 8):
            ids, imgs = pipe.generate_ids(ctx, B, T, 1.0, 5, flags, seed=seed, use_graph=False, streams=1)
            eager[seed] = (ids.clone(), imgs.clone())
            assert torch.isfinite(imgs).all() and int((ids == pipe.mask_token_id).sum(1).max()) == 1
        for lanes in (2, 3):
            for seed in (7, 8, 7):                              # eager warm-up of the graph path, capture, replay
                ids, imgs = pipe.generate_ids(ctx, B, T, 1.0, 5, flags, seed=seed, use_graph=True, streams=lanes)
                torch.cuda.synchronize()
                assert torch.equal(ids, eager[seed][0]), (name, lanes, seed)
                assert torch.equal(imgs, eager[seed][1]), (name, lanes, seed)
    finally:
        pipe.set_compute_dtype(torch.float32)
        del pipe
        torch.cuda.empty_cache()


def test_hilo_stream_and_layernorm_fold_full_size(pipe512, monkeypatch):
    """bf16 mode (default since round 3) keeps the residual stream as a bf16 hi/lo pair and folds every LayerNorm into the GEMM
    that consumes it (PMHIP_LN_UNFOLD=1: the pair, but pmhip_layernorm_hilo + plain GEMMs; PMHIP_HILO=0: the fp32 stream of
    rounds 1-2).  Against the fp32 stream: equally close to the fp32-verify logits, no more top-1 flips, fewer bytes through the
    LayerNorm family, batch-invariant, and the graph replay bit-identical to the eager loop.  Concurrent lanes are covered by
    test_timed_path_graph_and_lanes_bit_identical_to_eager / test_configs_4_and_5_... on the default (this) path."""
    from paintmind_amd import ops
    pipe = pipe512
    _, d = load_golden("full_stage2.npz")
    ids0 = t(np.repeat(d["ids0"].astype(np.int64), 16, axis=0))            # 16 images
    tok = pipe.ids2tokens(ids0)
    l32 = pipe.tokens2logits(tok[:1], None)
    g = torch.Generator().manual_seed(11)
    ids8 = torch.randint(0, 8192, (8, 1024), generator=g)
    ids8[torch.rand(8, 1024, generator=g) < 0.5] = pipe.mask_token_id
    tok8 = pipe.ids2tokens(ids8.to(dev()))
    l32_8 = torch.cat([pipe.tokens2logits(tok8[i:i + 4], None) for i in (0, 4)])
    pipe.set_compute_dtype(torch.bfloat16)
    try:
        res, ln, flips = {}, {}, {}
        for mode, env in (("f32", {"PMHIP_HILO": "0"}), ("unfold", {"PMHIP_LN_UNFOLD": "1"}), ("fold", {})):
            monkeypatch.delenv("PMHIP_HILO", raising=False)
            monkeypatch.delenv("PMHIP_LN_UNFOLD", raising=False)
            for k_, v_ in env.items():
                monkeypatch.setenv(k_, v_)
            pipe.invalidate_engines()                                      # the switches are read when a native handle is created
            res[mode] = pipe.tokens2logits(tok, None)
            ops.timing_reset(); ops.timing_enable(True)
            pipe.tokens2logits(tok, None)
            torch.cuda.synchronize(); ops.timing_enable(False)
            ln[mode] = ops.timing_get("layernorm")
            assert torch.equal(res[mode][:1], res[mode][7:8])              # batch-invariant
            assert torch.equal(pipe.tokens2logits(tok[:3], None), res[mode][:3])   # ... also across batch sizes (fold decision)
            flips[mode] = int((pipe.tokens2logits(tok8, None).argmax(-1) != l32_8.argmax(-1)).sum())
            flags = [True] * 4
            a = pipe.generate_ids(None, 16, 4, 1.0, 5, flags, seed=3, use_graph=False, streams=1)
            for _ in range(3):
                b = pipe.generate_ids(None, 16, 4, 1.0, 5, flags, seed=3, use_graph=True, streams=1)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), mode
        errs = {m: float((res[m][:1] - l32).abs().max()) for m in res}
        print(f"logits max err vs fp32: {errs}; top-1 flips on 8192 rows: {flips}; LayerNorm-family (launches, ms): {ln}")
        assert all(n_ == 37 for n_, _ in ln.values())                      # 12 layers x 3 + the final norm: one row pass each way
        assert errs["fold"] < BF16_LOGIT_MAXERR and errs["fold"] < 2.0 * errs["f32"] + 1e-3 and errs["unfold"] < 2.0 * errs["f32"] + 1e-3
        assert flips["fold"] <= 1.2 * flips["f32"] + 10 and flips["unfold"] <= 1.2 * flips["f32"] + 10
        assert ln["fold"][1] < 0.8 * ln["f32"][1]                          # the coefficient pass reads 2 of the 6 bytes per element
        # a folded consumer over more rows than one launch may address (32-bit byte offsets: 2M rows at dim 512) is cut into
        # launches of whole images; forced here with a cap of two images per launch: bit-identical to the single launch
        monkeypatch.setenv("PMHIP_FOLD_MAX_ROWS", "2048")
        pipe.invalidate_engines()
        assert torch.equal(pipe.tokens2logits(tok[:5], None), res["fold"][:5])
        b = pipe.generate_ids(None, 16, 4, 1.0, 5, [True] * 4, seed=3, use_graph=True, streams=1)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    finally:
        monkeypatch.delenv("PMHIP_FOLD_MAX_ROWS", raising=False)
        monkeypatch.delenv("PMHIP_HILO", raising=False)
        monkeypatch.delenv("PMHIP_LN_UNFOLD", raising=False)
        pipe.invalidate_engines()
        pipe.set_compute_dtype(torch.float32)


def test_bf16_tower_wider_than_the_hilo_row_operators():
    """dim = 1280 > 1024: the hi/lo row operators (one wave per row, the row in registers) do not serve it, so a bf16 tower of
    that width keeps the fp32 residual stream + pmhip_layernorm (engine.hip kHiloMaxDim) instead of failing on its first
    forward.  Checked against fp32-verify on the same weights."""
    cfg = dict(ver2cfg["bench-text-24L-d768"], dim=1280, num_head=20, mlp_dim=5120, depth=2, context_dim=1280)
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(cfg), stage1_pretrained=False).to(dev()).eval()
    g = torch.Generator().manual_seed(3)
    tok = torch.randn(2, 1024, 32, generator=g).to(dev())
    ctx = torch.randn(2, 77, 1280, generator=g).to(dev())
    l32 = pipe.tokens2logits(tok, ctx)
    pipe.set_compute_dtype(torch.bfloat16)
    l16 = pipe.tokens2logits(tok, ctx)
    l16_1 = pipe.tokens2logits(tok[:1], ctx[:1])
    assert torch.isfinite(l16).all() and torch.equal(l16[:1], l16_1)
    err = (l16 - l32).abs()
    print(f"dim 1280 bf16 vs fp32 logits: max {float(err.max()):.5f} mean {float(err.mean()):.6f} (logits std {float(l32.std()):.3f})")
    assert float(err.max()) < 0.05 and float(err.mean()) < 0.006


def test_centred_hi_plane_keeps_the_fold_accurate_on_offset_rows(monkeypatch):
    """Trained transformers carry residual rows whose common offset dwarfs their spread (massive activations); the folded
    LayerNorm rounds x to bf16 BEFORE the mean is subtracted and would lose 2^-9 |x| / std there.  Emulated on the 12L/d512
    transformer by a bias of +30 in the first out-projection (every later LayerNorm then sees rows of offset ~30, spread ~1).
    With the residual producers centring the hi plane (default) the bf16 logits stay as close to fp32-verify as on the
    unmodified model; with PMHIP_HILO_CENTER=0 they are several times worse.  LayerNorm is shift-invariant, so fp32-verify itself
    does not care."""
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(ver2cfg["bench-uncond-12L-d512"]), stage1_pretrained=False).to(dev()).eval()
    with torch.no_grad():
        pipe.transformer.layers.layer0.attn1.to_out[0].bias += 30.0
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(0, 8192, (4, 1024), generator=g)
    ids[torch.rand(4, 1024, generator=g) < 0.5] = pipe.mask_token_id
    tok = pipe.ids2tokens(ids.to(dev()))
    l32 = pipe.tokens2logits(tok, None)
    pipe.set_compute_dtype(torch.bfloat16)
    err = {}
    try:
        for mode in ("1", "0"):
            monkeypatch.setenv("PMHIP_HILO_CENTER", mode)
            pipe.invalidate_engines()
            l16 = pipe.tokens2logits(tok, None)
            assert torch.equal(l16[:1], pipe.tokens2logits(tok[:1], None))                   # batch-invariant either way
            e = (l16 - l32).abs()
            err[mode] = (float(e.max()), float(e.mean()), float((l16.argmax(-1) == l32.argmax(-1)).float().mean()))
    finally:
        monkeypatch.delenv("PMHIP_HILO_CENTER", raising=False)
        pipe.invalidate_engines()
        pipe.set_compute_dtype(torch.float32)
    print(f"rows of offset 30: bf16 vs fp32 logits (max err, mean err, top-1 agreement): centred {err['1']}, not centred {err['0']}")
    assert err["1"][0] < BF16_LOGIT_MAXERR * 2 and err["1"][1] < BF16_LOGIT_MEANERR * 2
    assert err["1"][1] < 0.6 * err["0"][1]


def test_small_batches_run_small_batch_kernels_and_give_the_large_batch_bits(pipe512):
    """Round 5: one or two images take small-batch forms of every hot kernel (64 / 128-query attention workgroups, the folded
    LayerNorm on the four-stage 128x128 GEMM with its coefficients computed in the prologue, eight-wave producers) and the
    graph-replayed loop defers each step's ViT decode to a side stream beside the next step's tower.  None of that may change
    a bit: the sampling noise is keyed by the global image index, so images 0 / 0-1 / 0-4 of a 40-image batch (large-batch
    kernels, no deferred decode) must equal the same images generated alone -- ids and every decoded image, bf16 mode, eager
    and graph replay (reference generate.py:183-198 has one code path and no batch dependence)."""
    pipe = pipe512
    pipe.set_compute_dtype(torch.bfloat16)
    try:
        T, flags = 4, [True] * 4
        ids40, imgs40 = pipe.generate_ids(None, 40, T, 1.0, 5, flags, seed=321, use_graph=False, streams=1)
        for nb in (1, 2, 5):
            for rep, graph in enumerate((False, True, True, True)):          # eager; graph: eager warm-up, capture, replay
                ids, imgs = pipe.generate_ids(None, nb, T, 1.0, 5, flags, seed=321, use_graph=graph, streams=1)
                assert torch.equal(ids, ids40[:nb]), (nb, rep)
                assert torch.equal(imgs, imgs40[:, :nb]), (nb, rep)
    finally:
        pipe.set_compute_dtype(torch.float32)


# ---- bf16 (the timed mode) on trained-like logits: the eight states of tests/golden/full_stage2_chain.npz ---------------------
# MEASURED on MI355X, 2026-10-17, this change on top of bab015c (profiles/bf16_chain_steps.txt), bf16 against the fp32-verify path of
# the same build: the eight fixture states plus the same eight steps with the unmasked positions refilled by torch.manual_seed(1..4)
# random tokens, five fillings in all; mean / sample sigma over the five:
#   top-1 agreement over 8 x 1024 rows        0.98936 / 0.0038   (fixture states 0.98889)
#   mean |score_bf16 - score_fp32|            0.004354 / 0.00080 (0.003581)     non-flipped masked rows
#   max  |score_bf16 - score_fp32|            0.02343 / 0.00723  (0.03215)
#   re-masked-set overlap, steps 0..6         0.99801 / 0, 0.99493 / 0.00293, 0.99224 / 0.00213, 0.98757 / 0.00618, 0.99296 / 0.00413,
#                                             0.98926 / 0.00554, 0.98593 / 0.00550
#   step 7 (num_mask = 1: a set of ONE, overlap is 0 or 1)   0.8 / 0.447 -- 0 on the fixture state: no bar can be set from this
# bf16 logits max error per step 0.18-0.23 (16 x the 0.011 of the unscaled model); no bf16 score was exactly 0 or 1 at any step and
# step 5 (entropy 0.16) is no outlier: nothing collapses on low-entropy rows.  Bars: two sigma on the safe side of the mean.
BF16_CHAIN_TOP1_AGREE = 0.9817
BF16_CHAIN_SCORE_MEAN_DEV = 0.00596
BF16_CHAIN_SCORE_MAX_DEV = 0.0379
BF16_CHAIN_REMASK_OVERLAP = [0.9980, 0.9890, 0.9879, 0.9752, 0.9847, 0.9781, 0.9749, 0.0]


@pytest.fixture(scope="module")
def chain_pipe():
    from gpu_common import scaled_chain_pipeline
    return scaled_chain_pipeline()


def _bf16_chain_step(pipe, ids_in, temp, nm):
    """one decode step on `ids_in` [1, N] in fp32-verify and in bf16 (folded final LayerNorm, the logits GEMM's block statistics,
    sample_tiles_kernel: the path bench.py times), topk = 1 -> per mode (logits, ids, pred, score) as numpy"""
    out = {}
    try:
        for dtype in (torch.float32, torch.bfloat16):
            pipe.set_compute_dtype(dtype)
            eng = pipe.engine()
            assert eng.dtype == dtype
            logits = pipe.tokens2logits(pipe.ids2tokens(ids_in), None)
            ids1, _, pred, score = eng.sample(pipe.vqgan.engine(), ids_in.clone(), None, 1, temp, nm, want_img=False, want_aux=True)
            out[dtype] = (logits[0], n(ids1)[0], n(pred)[0], n(score)[0])
    finally:
        pipe.set_compute_dtype(torch.float32)
    return out[torch.float32], out[torch.bfloat16]


def _bf16_chain_stats(pipe, d, fill_seed=None, verbose=True):
    """The eight chain states through both modes, with the hard assertions that need no measurement, -> the measured figures:
    (top-1 agreement over the 8 x 1024 rows, mean and max |score_bf16 - score_fp32| over non-flipped masked rows, [re-masked-set overlap
    per step]).  fill_seed: replace the tokens at the unmasked positions by torch.manual_seed(fill_seed)-seeded random ones (the
    spread the bars are set from); None: the fixture's states."""
    V, T = pipe.mask_token_id, 8
    flips_all, rows_all, devs, overlaps = 0, 0, [], []
    for step in range(T):
        ids_np = d[f"ids_in{step}"].astype(np.int64)
        nm = int(d[f"num_mask{step}"])
        if fill_seed is not None:
            torch.manual_seed(fill_seed)
            fill = torch.randint(0, V, ids_np.shape).numpy()
            ids_np = np.where(ids_np == V, V, fill)
        (l32, ids32, pred32, s32), (l16, ids16, pred16, s16) = _bf16_chain_step(pipe, t(ids_np), 1.0 * (1 - step / T), nm)
        masked = ids_np[0] == V
        err = float((l16 - l32).abs().max())
        top2 = torch.topk(l32, 2, dim=-1).values
        gap = n(top2[:, 0] - top2[:, 1])
        flips = pred16 != pred32
        # a flip needs the two candidates closer than the two errors combined, and at most the rows inside that noise may flip
        assert np.all(gap[flips] < 2 * err), (step, gap[flips], err)
        assert int(flips.sum()) <= int((gap < 2 * err).sum())
        assert (ids32 == V).sum() == (ids16 == V).sum() == nm
        assert np.isfinite(s16[masked]).all() and (s16[masked] >= 0).all() and (s16[masked] <= 1).all(), step
        assert np.array_equal(s16[~masked], np.full((~masked).sum(), -1e5, np.float32))
        ok = masked & ~flips
        dev_ = np.abs(s16.astype(np.float64) - s32)[ok]
        overlap = float(((ids16 == V) & (ids32 == V)).sum()) / nm
        sat = int(((s16[masked] == 0) | (s16[masked] == 1)).sum()), int(((s32[masked] == 0) | (s32[masked] == 1)).sum())
        if verbose:
            print(f"bf16 chain step {step}: logits max err {err:.4f}, {int(flips.sum())} flips ({int((gap < 2 * err).sum())} rows with gap < 2 err), "
                  f"score dev mean {dev_.mean():.2e} max {dev_.max():.2e}, re-mask overlap {overlap:.4f} of {nm}, "
                  f"scores exactly 0 or 1: bf16 {sat[0]} fp32 {sat[1]} of {int(masked.sum())}")
        flips_all += int(flips.sum())
        rows_all += flips.size
        devs.append(dev_)
        overlaps.append(overlap)
    devs = np.concatenate(devs)
    return 1.0 - flips_all / rows_all, float(devs.mean()), float(devs.max()), overlaps


def test_bf16_decode_steps_on_trained_like_logits(chain_pipe):
    """bf16 mode against fp32-verify of the same build on low-entropy, trained-like logits (row entropies 0.2-2.8 nats; the other
    bf16 tests run the flat logits of the random-weight model, std 0.3): the eight states of the reference's own decode chain.
    Hard: a prediction differs only where the fp32 top-2 gap is inside twice the step's measured logits error; both modes leave
    exactly num_mask mask ids; every bf16 score of a masked row is finite and in [0, 1].  Measured bars: see the constants."""
    pipe, d = chain_pipe
    agree, dev_mean, dev_max, overlaps = _bf16_chain_stats(pipe, d)
    print(f"bf16 chain, 8 x 1024 rows: top-1 agreement {agree:.5f}, score |dev| mean {dev_mean:.3e} max {dev_max:.3e}, "
          f"re-mask overlap per step {[round(o, 4) for o in overlaps]}")
    assert agree >= BF16_CHAIN_TOP1_AGREE, agree
    assert dev_mean <= BF16_CHAIN_SCORE_MEAN_DEV and dev_max <= BF16_CHAIN_SCORE_MAX_DEV, (dev_mean, dev_max)
    assert all(o >= bar for o, bar in zip(overlaps, BF16_CHAIN_REMASK_OVERLAP)), overlaps
