"""Model-level parity on the MI355X through the native engine: golden vectors captured from the
reference (tiny configs: every intermediate; full-size vit-s / 12L-d512: tokens, subsampled outputs)
and the CPU oracle on the same seeded inputs.

Tolerances (fp32-verify mode): token / id outputs bit-exact (a full-size token may differ only where the
reference's own best-vs-second distance gap is < 1e-5); floating-point outputs within 1e-3 absolute as
BASELINE.json's north_star states (observed ~1e-5)."""
import numpy as np
import pytest
import torch

import paintmind_amd as pm
from gpu_common import dev, n, t
from oracle import paintmind_oracle as O
from paintmind_amd.generate import Pipeline
from util import api_facts, load_golden, maxabs, to_torch_sd, vq_cfg

pytestmark = pytest.mark.gpu
TOL = 1e-3


@pytest.fixture(scope="module")
def tiny_vq():
    p, d = load_golden("tiny_vqgan.npz")
    m = pm.create_model(arch="vqgan", version="tiny-vqgan", pretrained=False)
    m.load_state_dict(to_torch_sd(p))
    return m.to(dev()).eval(), p, d


@pytest.fixture(scope="module")
def tiny_pipe():
    p, d = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False)
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("text_model") for k in missing.missing_keys)
    return pipe.to(dev()).eval(), p, d


def test_tiny_vqgan_encode_decode_golden(tiny_vq):
    m, p, d = tiny_vq
    x = t(d["x"])
    z, loss, idx = m.encode(x)
    assert z.shape == (3, 16, 32) and idx.dtype == torch.int64 and loss.shape == ()
    assert np.array_equal(n(idx), d["idx"])
    assert maxabs(n(z), d["z"]) < 1e-5
    assert abs(float(loss) - float(d["loss"])) < 1e-5
    assert maxabs(n(m.decode(t(d["z"]))), d["rec"]) < TOL
    assert maxabs(n(m.decode_from_indice(t(d["idx"]))), d["rec_from_idx"]) < TOL
    rec, loss2 = m(x)
    assert maxabs(n(rec), d["rec"]) < TOL
    eng = m.engine()
    assert maxabs(n(eng.encoder_forward(x)), d["enc_layer1"]) < 1e-4
    xq = O.linear(d["z"], p["post_quant.weight"], p["post_quant.bias"])
    assert maxabs(n(eng.decoder_forward(t(xq))), d["dec_unclamped"]) < TOL


def test_tiny_vqgan_operator_level_path_matches_engine(tiny_vq):
    """The Python composition of plug-in operators (Encoder.forward / Decoder.forward / attention / FFN
    classes) and the fused C++ engine are two routes to the same kernels."""
    m, p, d = tiny_vq
    x = t(d["x"])
    h = m.encoder(x)
    assert maxabs(n(h), d["enc_layer1"]) < 1e-4
    assert torch.equal(h, m.engine().encoder_forward(x))
    layer = m.encoder.transformer.layers[0]
    a = layer.attn1(t(d["l0_norm1"]))
    assert maxabs(n(a), d["l0_attn1"]) < 1e-5
    zq, loss, idx = m.quantize(t(d["prev_quant"]))
    assert np.array_equal(n(idx), d["idx"]) and maxabs(n(zq), d["z"]) < 1e-6
    xq = O.linear(d["z"], p["post_quant.weight"], p["post_quant.bias"])
    assert maxabs(n(m.decoder(t(xq))), d["dec_unclamped"]) < TOL
    assert maxabs(n(m.quantize.decode_from_indice(t(d["idx"]))), O.vq_decode_indices(d["idx"], p["quantize.embedding.weight"])) < 1e-6


def test_tiny_pipeline_logits_golden(tiny_pipe):
    pipe, p, d = tiny_pipe
    tok = pipe.ids2tokens(t(d["ids0"]))
    assert np.array_equal(n(tok), d["tokens"])
    assert maxabs(n(pipe.tokens2logits(tok, t(d["context"]))), d["logits_ctx"]) < TOL
    assert maxabs(n(pipe.tokens2logits(tok, None)), d["logits_noctx"]) < TOL
    # operator-level composition of the same transformer
    assert maxabs(n(pipe.transformer(tok, t(d["context"]))), d["logits_ctx"]) < TOL
    assert maxabs(n(pipe.transformer(tok, None)), d["logits_noctx"]) < TOL


@pytest.mark.parametrize("tag", ["ctx", "noctx"])
def test_tiny_pipeline_sample_golden(tiny_pipe, tag):
    pipe, p, d = tiny_pipe
    ctx = t(d["context"]) if tag == "ctx" else None
    ids0 = t(d["ids0"])
    ids1, img1 = pipe.sample(ids0, np.float64(0.5), text=ctx, topk=1, temperature=1.0)
    assert torch.equal(ids0, t(d["ids0"]))                      # input not modified, like the reference
    assert np.array_equal(n(ids1), d[f"s1_{tag}_ids"])
    assert maxabs(n(img1), d[f"s1_{tag}_img"]) < TOL
    ids5, img5 = pipe.sample(ids0, np.float64(0.5), text=ctx, topk=5, temperature=0.7, noise=t(d[f"s5_{tag}_noise"]))
    assert np.array_equal(n(ids5), d[f"s5_{tag}_ids"])
    assert maxabs(n(img5), d[f"s5_{tag}_img"]) < TOL


@pytest.mark.parametrize("scale", [0.0, 1.0, 3.0])
def test_guided_sample_step_against_oracle(tiny_pipe, scale):
    """logits = uncond + scale * (cond - uncond), uncond = the context=None forward the reference trains by
    dropping the text (utils/trainer.py:379,387-388).  The reference's sampling has no such option (unpinned: intended behaviour);
    the oracle restates it around the SAME reference-pinned pieces.  fp32-verify: ids exact with the reference's captured noise,
    image within 1e-3; scale 0 equals the unconditional step bit for bit; the guided generate() keeps the list structure."""
    pipe, p, d = tiny_pipe
    vcfg, scfg = pm.ver2cfg["tiny-vqgan"], pm.ver2cfg["tiny-pipeline"]
    ctx, ids0, noise = t(d["context"]), t(d["ids0"]), d["s5_ctx_noise"]
    ids1, img1 = pipe.sample(ids0, np.float64(0.5), text=ctx, topk=5, temperature=0.7, noise=t(noise), guidance_scale=scale)
    ids_o, img_o, aux = O.sample_step(d["ids0"], np.float64(0.5), d["context"], 5, 0.7, noise, p, vcfg, scfg, guidance_scale=scale)
    assert np.array_equal(n(ids1), ids_o) and maxabs(n(img1), img_o) < TOL
    if scale == 0.0:
        ids_u, img_u = pipe.sample(ids0, np.float64(0.5), text=None, topk=5, temperature=0.7, noise=t(d["s5_ctx_noise"]))
        assert torch.equal(ids1, ids_u) and torch.equal(img1, img_u)
    else:
        assert not np.array_equal(aux["logits"], O.cond_transformer(O.ids2tokens(d["ids0"], p), None, p, scfg))
    with pytest.raises(ValueError):
        pipe.sample(ids0, np.float64(0.5), text=None, guidance_scale=2.0)
    imgs, ids = pipe.generate(["a", "b"], timesteps=4, topk=3, save_interval=2, seed=9, guidance_scale=scale, return_ids=True)
    again = pipe.generate(["a", "b"], timesteps=4, topk=3, save_interval=2, seed=9, guidance_scale=scale)
    assert len(imgs) == 2 and imgs[0].device.type == "cpu" and all(torch.equal(a, b) for a, b in zip(imgs, again))
    assert int((ids == 64).sum(1).max()) == 1


def test_guided_native_loop_is_bit_identical_to_the_operator_composition(tiny_pipe):
    """Round 5: the guided step / loop run natively (pmhip_pipeline_sample_guided, pmhip_pipeline_generate_guided: both towers,
    the combine and the reference's tail inside the graph-captured, lane-able loop).  Its reference is the operator-level
    composition of the SAME C-ABI pieces (pmhip_s2_forward x 2, pmhip_guidance_combine, pmhip_sample_rows, decode,
    pmhip_remask) step by step in Python -- which test_guided_sample_step_against_oracle ties to the oracle: ids and every
    saved image bit-identical, in both precision modes, eager / graph capture / replay / two lanes."""
    from paintmind_amd.generate import mask_schedule, num_token_masked
    pipe, p, d = tiny_pipe
    texts = [f"t{i}" for i in range(9)]
    T, scale, topk, seed = 5, 2.5, 4, 77
    try:
        for dtype in (torch.float32, torch.bfloat16):
            pipe.set_compute_dtype(dtype)
            ctx = pipe.text_model(texts).to(dev())
            ids = torch.full((len(texts), pipe.num_tokens), pipe.mask_token_id, dtype=torch.long, device=dev())
            ref = []
            for step in range(T):
                nm = num_token_masked(mask_schedule((step + 1) / T), pipe.num_tokens)
                temp = 1.0 * (1 - step / T)
                one_ids, one_img = pipe.sample(ids, mask_schedule((step + 1) / T), text=ctx, topk=topk, temperature=temp, seed=seed,
                                               step=step, guidance_scale=scale)
                ids, img = pipe._sample_guided_composed(ids, nm, ctx, topk, temp, None, seed, step, 0, scale)
                assert torch.equal(one_ids, ids) and torch.equal(one_img, img), (dtype, step)      # the native guided STEP
                ref.append(img.cpu())
            kw = dict(timesteps=T, topk=topk, save_interval=1, seed=seed, guidance_scale=scale, return_ids=True)
            for mode in (dict(use_graph=False, streams=1), dict(), dict(), dict(), dict(use_graph=True, streams=2), dict(use_graph=True, streams=2),
                         dict(use_graph=True, streams=2)):
                imgs, gids = pipe.generate(texts, **kw, **mode)                                     # the native guided LOOP
                assert torch.equal(gids.cpu(), ids.cpu()), (dtype, mode)
                assert len(imgs) == T and all(torch.equal(a, b) for a, b in zip(imgs, ref)), (dtype, mode)
            # another scale is another graph, and scale 0 is the unconditional loop
            z0 = pipe.generate(texts, **{**kw, "guidance_scale": 0.0})
            z1 = pipe.generate(texts, **{**kw, "guidance_scale": 0.0})
            un = pipe.generate_ids(None, len(texts), T, 1.0, topk, [True] * T, seed, use_graph=False, streams=1)
            assert torch.equal(z0[1].cpu(), z1[1].cpu()) and torch.equal(z0[1].cpu(), un[0].cpu())
            assert all(torch.equal(a, b.cpu()) for a, b in zip(z1[0], un[1]))
    finally:
        pipe.set_compute_dtype(torch.float32)


def test_tiny_pipeline_decode_loop_golden(tiny_pipe):
    pipe, p, d = tiny_pipe
    ctx = t(d["context"])
    ids = torch.full((3, 16), 64, dtype=torch.long, device=dev())
    T = 4
    for step in range(T):
        r = O.mask_schedule((step + 1) / T)
        ids, img = pipe.sample(ids, r, text=ctx, topk=3, temperature=1.0 * (1 - step / T), noise=t(d[f"loop_noise{step}"]))
        assert np.array_equal(n(ids), d[f"loop_ids{step}"]), f"step {step}"
    assert maxabs(n(img), d["loop_img_last"]) < TOL


def test_generate_api_and_determinism(tiny_pipe):
    pipe, p, d = tiny_pipe
    facts = api_facts()
    imgs = pipe.generate(["a", "b"], timesteps=8, temperature=1.0, topk=5, save_interval=2, seed=5)
    assert len(imgs) == facts["generate_T8_si2_len"]
    assert list(imgs[0].shape) == facts["generate_img_shape"] and imgs[0].device.type == "cpu" and imgs[0].dtype == torch.float32
    imgs2, ids2 = pipe.generate(["a", "b"], timesteps=8, topk=5, save_interval=2, seed=5, return_ids=True)
    assert all(torch.equal(a, b) for a, b in zip(imgs, imgs2))
    assert int((ids2 == 64).sum(1).min()) == facts["residual_mask_tokens_after_T8"]      # one token stays masked
    imgs3 = pipe.generate(["a", "b"], timesteps=8, topk=5, save_interval=2, seed=6)
    assert not torch.equal(imgs[-1], imgs3[-1])
    # shard invariance: image 1 generated alone with image_base=1 equals image 1 of the batch
    pipe.text_model.base_index = 1
    solo = pipe.generate(["b"], timesteps=8, topk=5, save_interval=2, seed=5, image_base=1)
    pipe.text_model.base_index = 0
    assert all(torch.equal(a[1:2], b) for a, b in zip(imgs, solo))
    # torch.manual_seed governs the default seed
    torch.manual_seed(3)
    a = pipe.generate(["a"], timesteps=4, topk=5)
    torch.manual_seed(3)
    b = pipe.generate(["a"], timesteps=4, topk=5)
    assert torch.equal(a[-1], b[-1])


def test_generate_matches_stepwise_sample_with_philox_noise(tiny_pipe):
    """The native loop == T calls of Pipeline.sample fed with the Philox noise restated in numpy."""
    pipe, p, d = tiny_pipe
    B, N, V, T, seed = 2, 16, 64, 4, 77
    pipe.text_model.base_index = 0
    ctx = pipe.text_model(["x", "y"]).to(dev())
    imgs, ids_native = pipe.generate(["x", "y"], timesteps=T, temperature=1.0, topk=4, save_interval=1, seed=seed, return_ids=True)
    ids = torch.full((B, N), V, dtype=torch.long, device=dev())
    rows = np.broadcast_to(np.arange(B * N)[:, None], (B * N, V))
    cols = np.broadcast_to(np.arange(V), (B * N, V))
    for step in range(T):
        noise = O.philox_uniform(seed, step, rows, cols).reshape(B, N, V)
        ids, img = pipe.sample(ids, O.mask_schedule((step + 1) / T), text=ctx, topk=4, temperature=1.0 * (1 - step / T), noise=t(noise))
        assert torch.equal(img.cpu(), imgs[step])
    assert torch.equal(ids, ids_native)


def test_generate_hipgraph_replay_is_bit_identical(tiny_pipe):
    """eager pass, capture pass and replays of the graph-captured decode loop give the eager results for every seed"""
    pipe, p, d = tiny_pipe
    texts = ["a", "b", "c"]
    eager = {sd: pipe.generate(texts, timesteps=6, topk=4, save_interval=1, seed=sd, return_ids=True, use_graph=False, streams=1)
             for sd in (1, 2, 3, 4)}
    for sd in (1, 2, 3, 4, 2):          # 1: eager warm-up inside the graph path, 2: capture + launch, then replays
        imgs, ids = pipe.generate(texts, timesteps=6, topk=4, save_interval=1, seed=sd, return_ids=True, use_graph=True)
        assert torch.equal(ids, eager[sd][1]), sd
        assert all(torch.equal(a, b) for a, b in zip(imgs, eager[sd][0])), sd
    # a different schedule structure gets its own graph
    a = pipe.generate(texts, timesteps=4, topk=4, save_interval=2, seed=9, use_graph=True)
    b = pipe.generate(texts, timesteps=4, topk=4, save_interval=2, seed=9, use_graph=True)
    c = pipe.generate(texts, timesteps=4, topk=4, save_interval=2, seed=9, use_graph=False, streams=1)
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))


def test_generate_default_call_is_the_fast_path_and_matches_the_eager_loop(tiny_pipe):
    """Pipeline.generate() with no opt-ins (reference generate.py:183-198): segment graphs, lanes in bf16 mode, saved images
    copied to a pinned host buffer on a copy stream under the following steps.  The returned list must be bit-identical
    to the eager single-stream loop with blocking copies, for both save intervals, in both precision modes."""
    pipe, p, d = tiny_pipe
    texts = [f"t{i}" for i in range(9)]
    try:
        for dtype in (torch.float32, torch.bfloat16):
            pipe.set_compute_dtype(dtype)
            for si in (1, 2, 3):
                kw = dict(timesteps=7, topk=4, save_interval=si, seed=31 + si, return_ids=True)
                ref_dev, ref_ids = pipe.generate(texts, use_graph=False, streams=1, keep_on_device=True, **kw)
                ref = [im.cpu() for im in ref_dev]
                for rep in range(3):                              # eager pass, capture pass, replay
                    imgs, ids = pipe.generate(texts, **kw)
                    assert len(imgs) == len(ref) == len(range(0, 7, si))
                    assert torch.equal(ids, ref_ids), (dtype, si, rep)
                    for a, b in zip(imgs, ref):
                        assert a.device.type == "cpu" and a.dtype == torch.float32 and a.shape == b.shape
                        assert torch.equal(a, b), (dtype, si, rep)
        # earlier results stay valid after later calls (every call owns its host buffer)
        pipe.set_compute_dtype(torch.float32)
        first = pipe.generate(texts, timesteps=4, topk=3, seed=5)
        keep = [x.clone() for x in first]
        pipe.generate(texts, timesteps=4, topk=3, seed=6)
        assert all(torch.equal(a, b) for a, b in zip(first, keep))
    finally:
        pipe.set_compute_dtype(torch.float32)


def test_engine_cache_per_dtype_and_invalidate(tiny_vq):
    """one packed engine per compute dtype (autocast flips between two live engines); Parameter edits are seen through
    the version counter, edits through .data need invalidate_engines()"""
    m, p, d = tiny_vq
    x = t(d["x"])
    e32 = m.engine()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        e16 = m.engine()
        assert e16 is not e32 and e16.dtype == torch.bfloat16
    assert m.engine() is e32                                     # leaving autocast did not rebuild anything
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert m.engine() is e16
    idx0 = m.encode(x)[2].clone()
    with torch.no_grad():
        m.prev_quant.weight.mul_(-1.0)                           # in-place on the Parameter: version bump -> re-pack
    assert m.engine() is not e32 and not torch.equal(m.encode(x)[2], idx0)
    with torch.no_grad():
        m.prev_quant.weight.mul_(-1.0)
    assert torch.equal(m.encode(x)[2], idx0)
    # edits through .data are invisible to the fingerprint: a bf16 engine keeps serving its packed (converted) copy
    # until invalidate_engines() (an fp32 engine aliases the parameter storage, so it sees them at once)
    m.set_compute_dtype(torch.bfloat16)
    try:
        b0 = m.encode(x)[2].clone()
        m.prev_quant.weight.data.mul_(-1.0)
        assert torch.equal(m.encode(x)[2], b0)                   # stale packed copy
        m.invalidate_engines()
        assert not torch.equal(m.encode(x)[2], b0)
        m.prev_quant.weight.data.mul_(-1.0)
        m.invalidate_engines()
        assert torch.equal(m.encode(x)[2], b0)
    finally:
        m.set_compute_dtype(torch.float32)


def test_hipgraph_survives_workspace_growth(tiny_pipe):
    """A captured decode loop holds raw workspace pointers.  A later, larger call (bigger batch, longer context, a direct
    decode on the shared vqgan handle) reallocates those buffers; the next replay of the small graph must notice and
    re-capture instead of replaying into freed memory."""
    pipe, p, d = tiny_pipe
    small, big = ["a", "b", "c"], ["a", "b", "c", "d", "e", "f"]
    kw = dict(timesteps=5, topk=4, save_interval=1, return_ids=True)
    eager_small = pipe.generate(small, seed=21, use_graph=False, streams=1, **kw)
    eager_big = pipe.generate(big, seed=22, use_graph=False, streams=1, **kw)
    # a fresh engine pair so that the growth really happens after the capture
    pipe.invalidate_engines()
    for _ in range(3):                                        # eager warm-up, capture, replay
        got = pipe.generate(small, seed=21, use_graph=True, **kw)
    assert torch.equal(got[1], eager_small[1])
    got_big = pipe.generate(big, seed=22, use_graph=True, **kw)      # grows s2.* / dec.* / gen.* of the same handles
    assert torch.equal(got_big[1], eager_big[1])
    pipe.vqgan.decode_from_indice(torch.zeros(16, 16, dtype=torch.long, device=dev()))   # grows the vqgan workspace alone
    for _ in range(2):
        got = pipe.generate(small, seed=21, use_graph=True, **kw)    # stale graph -> re-captured
        assert torch.equal(got[1], eager_small[1])
        assert all(torch.equal(a, b) for a, b in zip(got[0], eager_small[0]))
    for _ in range(2):
        got_big = pipe.generate(big, seed=22, use_graph=True, **kw)
        assert torch.equal(got_big[1], eager_big[1]) and all(torch.equal(a, b) for a, b in zip(got_big[0], eager_big[0]))


def test_generate_concurrent_micro_batches_match_single_stream(tiny_pipe):
    pipe, p, d = tiny_pipe
    texts = ["a", "b", "c", "d", "e"]
    one = pipe.generate(texts, timesteps=5, topk=3, save_interval=1, seed=11, return_ids=True, use_graph=False, streams=1)
    for k in (2, 3, 5):
        for graph in (False, True, True):
            many = pipe.generate(texts, timesteps=5, topk=3, save_interval=1, seed=11, return_ids=True, streams=k, use_graph=graph)
            assert torch.equal(many[1], one[1]), (k, graph)
            assert all(torch.equal(a, b) for a, b in zip(many[0], one[0])), (k, graph)
    uneven = pipe.generate(texts, timesteps=5, topk=3, save_interval=1, seed=11, return_ids=True, streams=(1, 3, 1))
    assert torch.equal(uneven[1], one[1]) and all(torch.equal(a, b) for a, b in zip(uneven[0], one[0]))
    with pytest.raises(ValueError):
        pipe.generate(texts, timesteps=5, topk=3, save_interval=1, seed=11, streams=(2, 2))


def test_reconstruction_figure(tmp_path):
    """reference reconstruct.py:23-52: file -> transform -> encode -> decode -> 512x256 side-by-side figure.
    Left panel = the transformed input, right panel = restore(decode(encode(x))) checked against the oracle within
    1 LSB of the 8-bit image (restore truncates, so a 1e-5 float difference may move a pixel by one level)."""
    from PIL import Image
    from paintmind_amd.reconstruct import restore
    rng = np.random.default_rng(0)
    path = str(tmp_path / "in.png")
    Image.fromarray(rng.integers(0, 256, (300, 300, 3), dtype=np.uint8)).save(path)
    torch.manual_seed(0)
    fig = pm.reconstruction(path, model_name="vit-s-vqgan", pretrained=False, device="cuda")
    assert fig.size == (512, 256)
    left = np.asarray(fig.crop((0, 20, 256, 256)), dtype=np.int32)
    ref = np.asarray(Image.open(path).convert("RGB").resize((320, 320), Image.BICUBIC).crop((32, 32, 288, 288)).crop((0, 20, 256, 256)), dtype=np.int32)
    assert np.abs(left - ref).max() <= 1          # the left half is the (transformed) input
    # right half: the same weights (seed 0 construction) through the numpy oracle
    torch.manual_seed(0)
    m = pm.create_model(arch="vqgan", version="vit-s-vqgan", pretrained=False)
    p = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    x = pm.stage1_transform(is_train=False, scale=0.8)(Image.open(path).convert("RGB"))[None].numpy()
    z_o, _, idx_o = O.vqgan_encode(x, p, vq_cfg("vit-s-vqgan"))
    rec_o = O.vqgan_decode(z_o, p, vq_cfg("vit-s-vqgan"))
    want = np.asarray(restore(torch.from_numpy(rec_o[0])).crop((0, 20, 256, 256)), dtype=np.int32)
    right = np.asarray(fig.crop((256, 20, 512, 256)), dtype=np.int32)
    diff = np.abs(right - want)
    assert diff.max() <= 1, (int(diff.max()), float((diff > 0).mean()))


def test_checkpoint_round_trip_through_the_factory(tmp_path, vit_s):
    """factory.py:16-19 + vqmodel.py:43-44: a .pt file holding a reference-layout state_dict, loaded with
    create_model(pretrained=True, checkpoint_path=...), must reproduce the reference's golden tokens; same for a
    Pipeline checkpoint (generate.py:75-76) including mask_token and the transformer."""
    _, d = load_golden("full_vqgan.npz")
    torch.manual_seed(0)
    src = pm.create_model(arch="vqgan", version="vit-s-vqgan", pretrained=False)        # == the reference's seed-0 weights (sha-pinned)
    path = str(tmp_path / "vit-s-vqgan.pt")
    torch.save(src.state_dict(), path)
    torch.manual_seed(123)                                                               # different init, then overwritten by the file
    m = pm.create_model(arch="vqgan", version="vit-s-vqgan", pretrained=True, checkpoint_path=path).to(dev()).eval()
    x = (torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(100)) * 2 - 1).to(dev())
    z, loss, idx = m.encode(x)
    got, want = n(idx).reshape(-1), d["idx"].reshape(-1).astype(np.int64)
    mism = got != want
    assert mism.sum() <= 4 and np.all(d["gap"][mism] < 1e-5)
    assert torch.equal(idx, vit_s.encode(x)[2])                                          # == the directly constructed model
    assert maxabs(n(m.decode(t(d["z"])))[:, :, ::4, ::4], d["rec_sub"]) < TOL
    # Pipeline checkpoint: every non-text key round-trips, and the loaded pipeline samples the same ids
    torch.manual_seed(1)
    a = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False)
    ppath = str(tmp_path / "tiny-pipeline.pt")
    torch.save(a.state_dict(), ppath)
    pm.ver2cfg["tiny-pipeline-ckpt"] = pm.ver2cfg["tiny-pipeline"]
    torch.manual_seed(2)
    b = pm.create_model(arch="pipeline", version="tiny-pipeline-ckpt", pretrained=True, checkpoint_path=ppath)
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    a, b = a.to(dev()).eval(), b.to(dev()).eval()
    ia = a.generate(["x", "y"], timesteps=4, topk=3, seed=9, return_ids=True)[1]
    ib = b.generate(["x", "y"], timesteps=4, topk=3, seed=9, return_ids=True)[1]
    assert torch.equal(ia, ib)
    with pytest.raises(ValueError):
        pm.create_model(arch="nope", version="vit-s-vqgan", pretrained=False)


def test_t5_text_tower_feeds_generate_on_the_gpu():
    """f2: a (randomly initialised) Flan-T5-architecture tower as Pipeline.text_model: follows .to(device), produces
    (B, 77, ctx) on the GPU and Pipeline.generate consumes it (reference generate.py:58,188)."""
    from paintmind_amd.modules.encoder import T5TextEmbedder
    from text_stubs import StubTokenizer, tiny_t5
    emb = T5TextEmbedder(tokenizer=StubTokenizer(), transformer=tiny_t5(96))
    torch.manual_seed(4)
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False, text_model=emb).to(dev()).eval()
    ctx = pipe.text_model(["a cat", "a dog"])
    assert ctx.shape == (2, 77, 96) and ctx.is_cuda
    imgs, ids = pipe.generate(["a cat", "a dog"], timesteps=4, topk=3, seed=1, return_ids=True)
    assert len(imgs) == 2 and torch.isfinite(imgs[-1]).all()
    # the text really conditions the result: the oracle on the same context reproduces the first step
    p = {k: v.detach().cpu().numpy() for k, v in pipe.state_dict().items() if not k.startswith("text_model")}
    ids0 = torch.full((2, 16), 64, dtype=torch.long, device=dev())
    ids1, _ = pipe.sample(ids0, np.float64(0.5), text=ctx, topk=1, temperature=1.0)
    ids1_o, _, _ = O.sample_step(n(ids0), np.float64(0.5), n(ctx), 1, 1.0, np.full((2, 16, 64), 0.5, np.float32), p,
                                 pm.ver2cfg["tiny-vqgan"], pm.ver2cfg["tiny-pipeline"])
    assert np.array_equal(n(ids1), ids1_o)


def test_inpaint_outpaint_match_oracle_composition(tiny_pipe):
    """generate.py:200-236.  The reference itself raises here (float ids into nn.Embedding; api.json: inpaint_runs ==
    false), so there is no golden: the intended result is the composition encode -> integer keep-mask -> sample loop,
    restated as O.region_loop, and Pipeline.inpaint / outpaint must reproduce it (ids exact, image 1e-3)."""
    pipe, p, d = tiny_pipe
    assert api_facts()["inpaint_runs"] is False
    vcfg, scfg = pm.ver2cfg["tiny-vqgan"], pm.ver2cfg["tiny-pipeline"]
    x = load_golden("tiny_vqgan.npz")[1]["x"]
    ctx = d["context"]
    text_model = pipe.text_model
    pipe.text_model = torch.nn.Identity()               # to_latent passes `text` through the text tower (generate.py:129-130)
    try:
        for fn, keep_inside in ((pipe.inpaint, False), (pipe.outpaint, True)):
            for coord, T, use_ctx in (((8, 8, 16, 16), 1, False), ((0, 8, 24, 16), 3, True), ((16, 0, 8, 32), 2, True)):
                c = ctx if use_ctx else None
                img, ids = fn(t(x), coord, text=None if c is None else t(c), timesteps=T, return_ids=True)
                img_o, ids_o, aux = O.region_loop(x, coord, c, T, 1, 0, p, vcfg, scfg, keep_inside)
                assert np.array_equal(n(ids), ids_o), (fn.__name__, coord, T)
                assert maxabs(n(img), img_o) < TOL
                assert img.shape == (3, 3, 32, 32)
    finally:
        pipe.text_model = text_model
    # the default call (reference signature) returns the image only
    out = pipe.inpaint(t(x[:1]), (8, 8, 16, 16))
    assert out.shape == (1, 3, 32, 32) and torch.isfinite(out).all()
    # topk > 1: the Philox stream is drawn per call (torch.manual_seed governs it) and differs between calls
    torch.manual_seed(5)
    a = pipe.inpaint(t(x[:1]), (0, 0, 32, 32), timesteps=2, topk=8, temperature=2.0)
    torch.manual_seed(5)
    b = pipe.inpaint(t(x[:1]), (0, 0, 32, 32), timesteps=2, topk=8, temperature=2.0)
    c2 = pipe.inpaint(t(x[:1]), (0, 0, 32, 32), timesteps=2, topk=8, temperature=2.0)
    assert torch.equal(a, b) and not torch.equal(a, c2)
    # more than one step runs the NATIVE decode loop from the region's start ids (graph replay by default; round 6): bit for bit the
    # per-step composition the reference writes (one sample() per step), sampled steps included, eager and replayed
    z, ids0, _ = pipe.to_latent(t(x), None)
    ids0[:, 3:9] = pipe.mask_token_id
    for rep in range(3):                                       # eager warm-up of the graph path, capture, replay
        img_n, ids_n = None, None
        ids_n, imgs = pipe.generate_ids(None, ids0.shape[0], 3, 2.0, 4, [False, False, True], 99, use_graph=True, streams=1, ids0=ids0)
        img_c, ids_c = pipe._region_steps(ids0.clone(), None, 3, 4, 2.0, 99, return_ids=True)
        assert torch.equal(ids_n, ids_c) and torch.equal(imgs[0], img_c), rep
    assert int((ids0 == pipe.mask_token_id).sum()) == 6 * ids0.shape[0]          # the caller's start ids are not modified


# ------------------------------------------------------------------------------------------------
# full-size configurations (weights regenerated from the seed; checksum-pinned in test_abi_cpu.py)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vit_s():
    torch.manual_seed(0)
    return pm.create_model(arch="vqgan", version="vit-s-vqgan", pretrained=False).to(dev()).eval()


def test_full_vit_s_against_reference_golden(vit_s):
    _, d = load_golden("full_vqgan.npz")
    x = (torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(100)) * 2 - 1).to(dev())
    z, loss, idx = vit_s.encode(x)
    got, want = n(idx).reshape(-1), d["idx"].reshape(-1).astype(np.int64)
    mism = got != want
    assert mism.sum() <= 4 and np.all(d["gap"][mism] < 1e-5), (int(mism.sum()), d["gap"][mism])
    ok = ~mism.reshape(2, 1024)
    assert maxabs(n(z)[ok], d["z"][ok]) < 1e-5
    assert abs(float(loss) - float(d["loss"])) < 1e-5
    # VQ on the reference's own prev_quant output: bit-exact tokens
    zq, _, idx2 = vit_s.quantize(t(d["prev_quant"]))
    assert np.array_equal(n(idx2).reshape(-1), want)
    rec = vit_s.decode(t(d["z"]))
    assert maxabs(n(rec)[:, :, ::4, ::4], d["rec_sub"]) < TOL
    assert abs(float((rec.abs() == 1).float().mean()) - float(d["rec_clamped_frac"])) < 1e-3


def test_full_vit_s_batch64_properties(vit_s):
    """BASELINE config 2 size (B=64): per-image results do not depend on the batch they ride in, tokens
    survive a decode -> encode round trip of the codebook rows, outputs are clamped and finite."""
    x = (torch.rand(64, 3, 256, 256, generator=torch.Generator().manual_seed(100)) * 2 - 1).to(dev())
    z, loss, idx = vit_s.encode(x)
    z2, _, idx2 = vit_s.encode(x[:2].contiguous())
    assert torch.equal(idx[:2], idx2) and torch.equal(z[:2], z2)
    _, d = load_golden("full_vqgan.npz")
    mism = (n(idx[:2]).reshape(-1) != d["idx"].reshape(-1))
    assert mism.sum() <= 4
    rec = vit_s.decode(z)
    assert rec.shape == (64, 3, 256, 256) and torch.isfinite(rec).all() and float(rec.abs().max()) <= 1.0
    assert torch.equal(vit_s.decode_from_indice(idx)[:3], vit_s.decode_from_indice(idx[:3].contiguous()))
    # decode(z) with z = z + (zq - z) and decode_from_indice(idx) see the same latent up to 1 ulp
    assert float((vit_s.decode_from_indice(idx) - rec).abs().max()) < 1e-3
    # the quantiser is idempotent on its own outputs
    zq, _, idx3 = vit_s.quantize(z)
    assert torch.equal(idx3, idx)


def test_full_stage2_against_reference_golden():
    from paintmind_amd.config import ver2cfg
    _, d = load_golden("full_stage2.npz")
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(ver2cfg["bench-uncond-12L-d512"]), stage1_pretrained=False).to(dev()).eval()
    ids0 = t(d["ids0"].astype(np.int64))
    logits = pipe.tokens2logits(pipe.ids2tokens(ids0), None)
    assert maxabs(n(logits)[:, ::8, ::64], d["logits_sub"]) < TOL
    lse = torch.logsumexp(logits, -1)
    assert maxabs(n(lse), d["logits_lse"]) < TOL
    am = n(logits.argmax(-1))
    bad = am != d["logits_argmax"]
    assert np.all(d["logits_top2gap"][bad] < 1e-4), int(bad.sum())
    # topk=1 is deterministic.  One step through the native sample entry, with its predictions and scores:
    eng, V, m = pipe.engine(), pipe.mask_token_id, max(int(0.4 * 1024), 1)
    ids1, img1, pred, score = eng.sample(pipe.vqgan.engine(), ids0.clone(), None, 1, 1.0, m, want_img=True, want_aux=True)
    got, want = n(ids1)[0], d["ids1"].astype(np.int64)[0]
    pred, score, gap = n(pred)[0], n(score)[0], d["logits_top2gap"][0]
    assert np.array_equal(pred != d["logits_argmax"][0], bad[0])
    assert (got == V).sum() == (want == V).sum() == m
    # every id mismatch must be explained by a near-tie: an arg-max flip (top-2 logit gap < 1e-4) or a re-mask
    # decision on a confidence score within 1e-5 of the cut-off (the m-th largest score)
    cutoff = np.sort(score)[-m]
    mism = got != want
    flip = mism & (pred != d["logits_argmax"][0])
    edge = mism & ~flip
    # observed counts; the in-window count says how much the 1e-5 excuse below covers: on this model's flat logits (std 0.34) it
    # is most of the masked positions, so only the <= 8 cap binds here -- test_full_size_decode_chain_against_reference is the
    # test that binds the re-mask decision (scaled logits: every score distinct, windows from the reference's own deviation)
    print(f"full_stage2 one step: {int(mism.sum())} id mismatches ({int(flip.sum())} arg-max flips, {int(edge.sum())} edge decisions), "
          f"{int(bad.sum())} flipped rows, {int((np.abs(score - cutoff) < 1e-5).sum())} of {int((n(ids0)[0] == V).sum())} masked positions "
          f"inside the 1e-5 score window")
    assert np.all(gap[flip] < 1e-4), gap[flip]
    assert np.all(np.abs(score[edge] - cutoff) < 1e-5), (score[edge], cutoff)
    assert mism.sum() <= 8, int(mism.sum())
    # the image is decoded from the predictions at ALL positions (generate.py:165) == the reference's arg-max:
    # decode the GOLDEN ids so that the 1e-3 image check binds whatever the sampled ids are
    img_g = pipe.vqgan.decode_from_indice(t(d["logits_argmax"].astype(np.int64)))
    assert maxabs(n(img_g)[:, :, ::4, ::4], d["img1_sub"]) < TOL
    if not bad.any():
        assert maxabs(n(img1)[:, :, ::4, ::4], d["img1_sub"]) < TOL


@pytest.fixture(scope="module")
def chain_pipe():
    from gpu_common import scaled_chain_pipeline
    return scaled_chain_pipeline()


def test_full_size_decode_chain_against_reference(chain_pipe):
    """The reference's own 8-step decode loop at full size (1024 tokens, 8192 classes, B = 1, topk = 1, from the all-mask start;
    generate.py:189-194) on trained-like logits: tests/golden/full_stage2_chain.npz, the 12L/d512 model with to_logits.weight x 16
    (row entropies 0.2-2.8 nats, every confidence score of a step distinct).  fp32-verify mode.

    Teacher-forced: every step runs natively on the REFERENCE's input ids.  Logits / lse within 16 x TOL of the reference's float64
    evaluation (TOL times the exact scale factor); predictions and output ids equal the reference's at every DECIDABLE position --
    top-2 gap >= W * 2 * dlogit and |score - cut-off| >= W * 2 * dscore with dlogit / dscore the reference's own fp32-vs-float64
    deviation of that step and W = 8: at most 4 positions of a step are not (the generator's table in make_goldens.py) -- exactly
    num_mask mask ids (the cosine schedule's 1004 ... 199 and the final max(int(r * 1024), 1) = 1), no unmasked input id touched.
    Where the one-step full-size tests above excuse any mismatch within 1e-5 of the cut-off (hundreds of positions on the flat
    logits of the unscaled model), this chain binds the re-mask decision.

    Free-running: one Pipeline.sample per step from the all-mask state, as the reference's generate() composes them.  Up to the
    first step t* whose ids differ from the reference's, the inputs were the reference's, so every difference at t* must be at an
    undecidable position; the mask count follows the schedule at every step.  The native loop (graph replay and eager) gives the
    composition's final ids and image bit for bit.

    Observed on MI355X (2026-10-17): max |logit - logit64| 0.81-1.50 x and max |score - score64| 0.79-2.30 x the reference's own fp32
    deviation (inside W = 8, which stays); 0 id mismatches at steps 0-6, 1 at step 7 (an arg-max flip at an undecidable row, the same
    row the numpy oracle flips); t* = 7."""
    from paintmind_amd.generate import mask_schedule, num_token_masked
    pipe, d = chain_pipe
    eng, vq, V, T = pipe.engine(), pipe.vqgan.engine(), pipe.mask_token_id, 8
    assert eng.dtype == torch.float32
    temps = [1.0 * (1 - step / T) for step in range(T)]
    for step in range(T):
        nm = int(d[f"num_mask{step}"])
        assert num_token_masked(mask_schedule((step + 1) / T), pipe.num_tokens) == nm
        ids_in = t(d[f"ids_in{step}"].astype(np.int64))
        want, argmax, dec = d[f"ids_out{step}"].astype(np.int64)[0], d[f"argmax{step}"].astype(np.int64)[0], d[f"decidable{step}"][0]
        logits = pipe.tokens2logits(pipe.ids2tokens(ids_in), None)
        dl = maxabs(n(logits)[:, ::8, ::64], d[f"logits64_sub{step}"])
        lse = n(torch.logsumexp(logits.double(), -1))
        dlse = maxabs(lse, d[f"lse64{step}"])
        print(f"chain step {step}: max |logit - logit64| {dl:.2e} = {dl / float(d[f'dlogit{step}']):.2f} x the reference's own fp32 "
              f"deviation ({float(d[f'dlogit{step}']):.2e}; up to 2e-6 of the numerator is the fixture's float32 storage of logits64_sub), "
              f"max |lse - lse64| {dlse:.2e} = {dlse / float(d[f'dlogit{step}']):.2f} x (lse64 is stored as float64)")
        assert dl < 16 * TOL and dlse < 16 * TOL               # the scaling took, and the logits are the reference's
        last = step == T - 1
        ids1, img1, pred, score = eng.sample(vq, ids_in.clone(), None, 1, temps[step], nm, want_img=last, want_aux=True)
        got, pred, score, inp = n(ids1)[0], n(pred)[0], n(score)[0], n(ids_in)[0]
        masked = inp == V
        mism, flip = got != want, pred != argmax
        dscore = np.abs(score.astype(np.float64) - d[f"score64{step}"][0])
        print(f"chain step {step}: num_mask {nm}, {int(mism.sum())} id mismatches ({int((mism & ~dec).sum())} at undecidable positions; "
              f"{int((mism & flip).sum())} arg-max flips, {int((mism & ~flip).sum())} edge decisions), {int(flip.sum())} flipped rows, "
              f"{int((~dec).sum())} undecidable positions, max |score - score64| {dscore[masked].max():.2e} = "
              f"{dscore[masked].max() / float(d[f'dscore{step}']):.2f} x the reference's own")
        bad = (mism | flip) & dec
        assert not bad.any(), (step, np.nonzero(bad)[0], "|score - score64|", dscore[bad], "|lse - lse64|",
                               np.abs(lse[0] - d[f"lse64{step}"][0])[bad], "gap64", d[f"gap64{step}"][0][bad])
        assert (got == V).sum() == (want == V).sum() == nm
        assert np.array_equal(got[~masked], inp[~masked])       # score -1e5 and num_mask <= masked count: never re-masked
        assert np.array_equal(score[~masked], np.full((~masked).sum(), -1e5, np.float32))
        if last:
            img_g = pipe.vqgan.decode_from_indice(t(argmax[None]))
            assert maxabs(n(img_g)[:, :, ::4, ::4], d["img_last_sub"]) < TOL
            if not flip.any():
                assert maxabs(n(img1)[:, :, ::4, ::4], d["img_last_sub"]) < TOL
    # the free-running loop, composed as the reference composes it
    seed = 2024
    ids = torch.full((1, pipe.num_tokens), V, dtype=torch.long, device=dev())
    t_star = T
    for step in range(T):
        ids, img = pipe.sample(ids, mask_ratio=mask_schedule((step + 1) / T), text=None, topk=1, temperature=temps[step], seed=seed, step=step)
        assert int((ids == V).sum()) == int(d[f"num_mask{step}"]), step
        diff = n(ids)[0] != d[f"ids_out{step}"].astype(np.int64)[0]
        if t_star == T and diff.any():
            t_star = step
            assert not (diff & d[f"decidable{step}"][0]).any(), (step, np.nonzero(diff & d[f"decidable{step}"][0])[0])
            print(f"free-running loop: first difference from the reference at step {step}, {int(diff.sum())} undecidable positions")
    print(f"free-running loop: t* = {t_star} (8 = the reference's ids at every step)")
    for graph, reps in ((True, 3), (False, 1)):                  # graph: eager warm-up of the graph path, capture, replay
        for rep in range(reps):
            ids_n, imgs_n = pipe.generate_ids(None, 1, T, 1.0, 1, [False] * (T - 1) + [True], seed, use_graph=graph, streams=1)
            assert torch.equal(ids_n, ids) and torch.equal(imgs_n[0], img), (graph, rep)


@pytest.mark.parametrize("key,name,stride", [("bench-text-24L-d768", "full_stage2_d768", 4),
                                             ("bench-text-24L-d1024-512px", "full_stage2_d1024", 8)])
def test_north_star_size_stage2_against_reference_golden(key, name, stride):
    """vit-s-vqgan + 24L/d768 with a 77 x 768 context (the model north_star's target is quoted on; context_proj = Identity) and
    cfg 5 (vit-b-vqgan-512 + 24L/d1024, context_proj 768 -> 1024) against the REFERENCE's own tokens2logits + sample(topk=1) at
    that size (stage2/transformer.py:80-93, generate.py:159-181; tests/golden/make_goldens.py full_stage2_text), fp32-verify
    mode: logits / lse within 1e-3, arg-max equal except at near-ties, ids explained as in the 12L/d512 test, image within
    1e-3."""
    from paintmind_amd.config import ver2cfg
    _, d = load_golden(name + ".npz")
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(ver2cfg[key]), stage1_pretrained=False).to(dev()).eval()
    ids0 = t(d["ids0"].astype(np.int64))
    ctx = t(d["context"])
    logits = pipe.tokens2logits(pipe.ids2tokens(ids0), ctx)
    assert maxabs(n(logits)[:, ::8, ::64], d["logits_sub"]) < TOL
    assert maxabs(n(torch.logsumexp(logits, -1)), d["logits_lse"]) < TOL
    am = n(logits.argmax(-1))
    bad = am != d["logits_argmax"]
    assert np.all(d["logits_top2gap"][bad] < 1e-4), int(bad.sum())
    eng, V, m = pipe.engine(), pipe.mask_token_id, max(int(0.4 * 1024), 1)
    ids1, img1, pred, score = eng.sample(pipe.vqgan.engine(), ids0.clone(), ctx, 1, 1.0, m, want_img=True, want_aux=True)
    got, want = n(ids1)[0], d["ids1"].astype(np.int64)[0]
    pred, score, gap = n(pred)[0], n(score)[0], d["logits_top2gap"][0]
    assert np.array_equal(pred != d["logits_argmax"][0], bad[0])
    assert (got == V).sum() == (want == V).sum() == m
    cutoff = np.sort(score)[-m]
    mism = got != want
    flip = mism & (pred != d["logits_argmax"][0])
    edge = mism & ~flip
    # observed counts (see test_full_stage2_against_reference_golden: with most positions inside the window only the cap binds;
    # the re-mask decision itself is bound by test_full_size_decode_chain_against_reference)
    print(f"{name} one step: {int(mism.sum())} id mismatches ({int(flip.sum())} arg-max flips, {int(edge.sum())} edge decisions), "
          f"{int(bad.sum())} flipped rows, {int((np.abs(score - cutoff) < 1e-5).sum())} of {int((n(ids0)[0] == V).sum())} masked positions "
          f"inside the 1e-5 score window")
    assert np.all(gap[flip] < 1e-4), gap[flip]
    assert np.all(np.abs(score[edge] - cutoff) < 1e-5), (score[edge], cutoff)
    assert mism.sum() <= 8, int(mism.sum())
    img_g = pipe.vqgan.decode_from_indice(t(d["logits_argmax"].astype(np.int64)))
    assert maxabs(n(img_g)[:, :, ::stride, ::stride], d["img1_sub"]) < TOL
    if not bad.any():
        assert maxabs(n(img1)[:, :, ::stride, ::stride], d["img1_sub"]) < TOL
    # the SAMPLED step (topk = 5, temperature 0.7) under the noise the reference drew: only a row's k candidates can win, so the
    # fixture holds the reference's noise at its top-5 columns and the rest of the tensor is filler.  A row may differ from the
    # reference only where fp32 rounding can decide: the 5th / 6th logit closer than 1e-3 (another candidate set), the two best
    # perturbed candidates closer than 2e-3, or a re-mask decision on a score within 1e-5 of the cut-off.
    cols = torch.from_numpy(d["s5_cols"].astype(np.int64)).to(dev())
    noise = torch.full((1, 1024, V), 0.5, device=dev())
    noise.scatter_(2, cols, t(d["s5_noise"]))
    ids5, _, pred5, score5 = eng.sample(pipe.vqgan.engine(), ids0.clone(), ctx, 5, 0.7, m, noise=noise, want_img=False, want_aux=True)
    got5, want5 = n(ids5)[0], d["s5_ids"].astype(np.int64)[0]
    assert (got5 == V).sum() == (want5 == V).sum() == m
    cand = logits.gather(2, cols)[0].double() / 0.7 - torch.log(-torch.log(t(d["s5_noise"])[0].double().clamp_min(1e-20)).clamp_min(1e-20))
    top2 = torch.topk(cand, 2, dim=-1).values
    margin = n(top2[:, 0] - top2[:, 1])
    score5 = n(score5)[0]
    cut5 = np.sort(score5)[-m]
    mism5 = got5 != want5
    explained = (margin < 2e-3) | (d["s5_gap56"][0] < 1e-3) | (np.abs(score5 - cut5) < 1e-5)
    print(f"{name} sampled step (topk 5): {int(mism5.sum())} id mismatches, {int((np.abs(score5 - cut5) < 1e-5).sum())} positions inside the "
          f"1e-5 score window, {int((margin < 2e-3).sum())} rows with a candidate margin < 2e-3")
    assert np.all(explained[mism5]), (int(mism5.sum()), margin[mism5], d["s5_gap56"][0][mism5])
    assert mism5.sum() <= 8, int(mism5.sum())
    masked0 = n(ids0)[0] == V
    assert np.array_equal(n(pred5)[0][masked0 & (want5 != V) & ~mism5], want5[masked0 & (want5 != V) & ~mism5])


def test_vit_b_512_against_reference_golden():
    """BASELINE cfg 5's stage 1 as assumed here (vit-b-vqgan-512: image 512, patch 16, dim 768, depth 12, 12 heads, mlp 3072): the
    reference's own classes on that config (tests/golden/make_goldens.py full_vqgan_b512), fp32-verify mode.  Tokens exact except at
    VQ near-ties (distance gap < 1e-5), z / loss 1e-5, the quantiser on the reference's own prev_quant output bit-exact, image 1e-3."""
    _, d = load_golden("full_vqgan_b512.npz")
    torch.manual_seed(0)
    m = pm.create_model(arch="vqgan", version="vit-b-vqgan-512", pretrained=False).to(dev()).eval()
    x = (torch.rand(1, 3, 512, 512, generator=torch.Generator().manual_seed(101)) * 2 - 1).to(dev())
    z, loss, idx = m.encode(x)
    got, want = n(idx).reshape(-1), d["idx"].reshape(-1).astype(np.int64)
    mism = got != want
    assert mism.sum() <= 4 and np.all(d["gap"][mism] < 1e-5), (int(mism.sum()), d["gap"][mism])
    ok = ~mism.reshape(1, 1024)
    assert maxabs(n(z)[ok], d["z"][ok]) < 1e-5
    assert abs(float(loss) - float(d["loss"])) < 1e-5
    zq, _, idx2 = m.quantize(t(d["prev_quant"]))
    assert np.array_equal(n(idx2).reshape(-1), want)
    rec = m.decode(t(d["z"]))
    assert rec.shape == (1, 3, 512, 512)
    assert maxabs(n(rec)[:, :, ::8, ::8], d["rec_sub"]) < TOL
    assert abs(float((rec.abs() == 1).float().mean()) - float(d["rec_clamped_frac"])) < 1e-3


def test_full_size_inpaint_outpaint_against_oracle(vit_s):
    """vit-s-vqgan + 12L/d512 at B=1: Pipeline.inpaint / outpaint against O.region_loop.  Token ids from the encoder must
    equal the oracle's except at near-ties of the VQ distance (gap < 1e-5); the loop itself is compared on identical
    start tokens: predicted ids equal wherever the oracle's top-2 logit gap is >= 1e-4, re-mask decisions equal
    wherever the score is not within 1e-5 of the cut-off, image of the oracle's predictions within 1e-3."""
    from paintmind_amd.config import ver2cfg
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(ver2cfg["bench-uncond-12L-d512"]), stage1_pretrained=False).eval()
    p = {k: v.detach().numpy() for k, v in pipe.state_dict().items() if not k.startswith("text_model")}
    vq_p = {k[len("vqgan."):]: v for k, v in p.items() if k.startswith("vqgan.")}
    scfg, vcfg = ver2cfg["bench-uncond-12L-d512"], ver2cfg["vit-s-vqgan"]
    pipe = pipe.to(dev())
    x = (torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(7)) * 2 - 1)
    V = vcfg["n_embed"]
    _, _, idx_gpu = pipe.vqgan.encode(x.to(dev()))
    ze = O.vqgan_encode(x.numpy(), vq_p, vcfg, return_pre=True)
    idx_o = ze[2]
    mism = n(idx_gpu) != idx_o
    assert mism.sum() <= 2, int(mism.sum())
    for fn, keep_inside, coord in ((pipe.inpaint, False, (64, 32, 96, 128)), (pipe.outpaint, True, (64, 32, 96, 128))):
        img, ids = fn(x.to(dev()), coord, timesteps=1, return_ids=True)
        img_o, ids_o, aux = O.region_loop(x.numpy(), coord, None, 1, 1, 0, p, vcfg, scfg, keep_inside, ids=n(idx_gpu))
        keep = O.region_keep_mask(coord, 256, 8, keep_inside)
        assert int((~keep).sum()) == (12 * 16 if not keep_inside else 1024 - 12 * 16)
        top2 = -np.sort(-aux["logits"], axis=-1)[..., :2]
        gap = (top2[..., 0] - top2[..., 1])
        got = n(ids)
        m = aux["num_mask"]
        cutoff = np.sort(aux["score"][0])[-m]
        near = (gap < 1e-4) | (np.abs(aux["score"] - cutoff) < 1e-5)
        bad = (got != ids_o) & ~near
        # observed counts (the chain test binds the re-mask decision; here most masked positions are inside the window)
        mism_r = got != ids_o
        flip_r = mism_r & (gap < 1e-4)
        print(f"{fn.__name__} one step: {int(mism_r.sum())} id mismatches ({int(flip_r.sum())} at near-tie arg-maxes, {int((mism_r & ~flip_r).sum())} "
              f"edge decisions), {int((np.abs(aux['score'] - cutoff) < 1e-5).sum())} of {int((~keep).sum())} masked positions inside the 1e-5 "
              f"score window, num_mask {m}")
        assert not bad.any(), int(bad.sum())
        assert (got == V).sum() == (ids_o == V).sum() == m
        assert np.array_equal(got[keep & (got != V)], n(idx_gpu)[keep & (got != V)])         # kept tokens survive unless re-masked
        img_pred = pipe.vqgan.decode_from_indice(torch.from_numpy(aux["pred"]).to(dev()))
        assert maxabs(n(img_pred), img_o) < TOL
        if np.array_equal(got, ids_o):
            assert maxabs(n(img), img_o) < TOL


# bf16 mode of the ViT towers against fp32-verify, measured on MI355X (round 4, hi/lo stream + folded LayerNorm;
# tools/bf16_vit_stats.py, seeds 100..107 at B = 4, bench inputs 0..2 at B = 64): token agreement 0.9858-0.9912 at B = 4 (a count
# statistic over 4096 tokens: sigma 0.0017) and 0.98843-0.98895 at B = 64 (sigma 0.0004); bf16 decode of the SAME fp32 latent:
# mean |dev| 0.00311-0.00333, max 0.0245-0.0304; end to end with each mode's own tokens: mean 0.0040-0.0048.
# Bars: two sigma below the measured mean / 10 % and 30 % above the measured maxima.
BF16_VIT_TOKEN_AGREE = {4: 0.9850, 64: 0.9875}
BF16_VIT_REC_MEAN_DEV = 0.0036
BF16_VIT_REC_MAX_DEV = 0.040


def _bf16_vit_stats(vit_s, x, chunk=8):
    """(token agreement, mean / max |rec_bf16 - rec_fp32| decoding the SAME fp32 latent, the same with each mode's own
    tokens).  fp32-verify runs in chunks (the exact-f32 matrix core path is 15x slower and is only the checker here)."""
    z32, idx32, rec32 = [], [], []
    for i in range(0, x.shape[0], chunk):
        z, _, idx = vit_s.encode(x[i:i + chunk])
        z32.append(z); idx32.append(idx); rec32.append(vit_s.decode(z))
    z32, idx32, rec32 = torch.cat(z32), torch.cat(idx32), torch.cat(rec32)
    vit_s.set_compute_dtype(torch.bfloat16)
    try:
        z16, _, idx16 = vit_s.encode(x)
        rec16 = vit_s.decode(z32)
        rec16_own = vit_s.decode(z16)
    finally:
        vit_s.set_compute_dtype(torch.float32)
    agree = float((idx16 == idx32).float().mean())
    d = (rec16 - rec32).abs()
    return agree, float(d.mean()), float(d.max()), float((rec16_own - rec32).abs().mean())


@pytest.mark.parametrize("B", [4, 64])
def test_bf16_perf_mode_deviation_is_bounded(vit_s, B):
    """bf16 mode is graded on throughput; its deviation from the fp32 path is measured and bounded here at the batch the
    reconstruction bench times (BASELINE.json configs[1]: B = 64, bf16) and at B = 4, with bars two sigma from the
    measured values (the reference under torch.autocast(bfloat16) flips 3.0 % of tokens)."""
    seed = 100 if B == 4 else 0
    x = (torch.rand(B, 3, 256, 256, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(dev())
    agree, dev_mean, dev_max, dev_own = _bf16_vit_stats(vit_s, x)
    print(f"B={B}: bf16 token agreement {agree:.4f}, reconstruction |dev| mean {dev_mean:.5f} max {dev_max:.4f} (same latent), "
          f"mean {dev_own:.5f} (own tokens)")
    assert agree >= BF16_VIT_TOKEN_AGREE[B], agree
    assert dev_mean <= BF16_VIT_REC_MEAN_DEV and dev_max <= BF16_VIT_REC_MAX_DEV, (dev_mean, dev_max)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert vit_s.compute_dtype == torch.bfloat16


def test_paintmindv1_preset_sample_step_and_fast_path():
    """The reference's only pipeline preset (config.py:70-82, the default of factory.py:6): 12L / d1024 / 16 heads with T5-L
    features of width 1024, so context_proj is nn.Identity (stage2/transformer.py:58).  The T5 tower itself is a pretrained
    third-party model that is not in this image: the synthetic (B, 77, 1024) embedder stands in for it.
    (a) fp32-verify: logits within 1e-3 of the numpy oracle, one sample step (generate.py:159-181) with topk=1: kept ids equal
        the oracle's arg-max except at near-ties, image of the oracle's predictions within 1e-3;
    (b) bf16: the default generate() path (graph replay + two lanes) is bit-identical to the eager single-stream loop."""
    from paintmind_amd.config import ver2cfg
    from paintmind_amd.modules.encoder import SyntheticTextEmbedder
    scfg, vcfg = ver2cfg["paintmindv1"], ver2cfg["vit-s-vqgan"]
    torch.manual_seed(5)
    pipe = Pipeline(pm.Config(scfg), stage1_pretrained=False, text_model=SyntheticTextEmbedder(1024)).eval()
    assert isinstance(pipe.transformer.context_proj, torch.nn.Identity)
    p = {k: v.detach().numpy() for k, v in pipe.state_dict().items() if not k.startswith("text_model")}
    pipe = pipe.to(dev())
    N, V = pipe.num_tokens, vcfg["n_embed"]
    g = torch.Generator().manual_seed(9)
    ids0 = torch.randint(0, V, (1, N), generator=g)
    ids0[torch.rand(1, N, generator=g) < 0.6] = V
    ctx = pipe.text_model(["a prompt"]).cpu()
    assert ctx.shape == (1, 77, 1024)
    ocfg = dict(scfg, context_dim=1024)
    logits = pipe.tokens2logits(pipe.ids2tokens(ids0.to(dev())), ctx.to(dev()))
    ref = O.cond_transformer(O.ids2tokens(ids0.numpy(), p), ctx.numpy(), p, ocfg)
    assert maxabs(n(logits), ref) < TOL
    ids1, img1 = pipe.sample(ids0.to(dev()), np.float64(0.3), text=ctx.to(dev()), topk=1, temperature=1.0)
    top2 = -np.sort(-ref, axis=-1)[..., :2]
    pred_ref = ref.argmax(-1)
    got = n(ids1)
    kept = (ids0.numpy() == V) & (got != V)
    bad = kept & (got != pred_ref)
    assert np.all((top2[..., 0] - top2[..., 1])[bad] < 1e-4), int(bad.sum())
    assert int((got == V).sum()) == max(int(0.3 * N), 1)
    vq_p = {k[len("vqgan."):]: v for k, v in p.items() if k.startswith("vqgan.")}
    img_ref = O.vqgan_decode_indices(pred_ref, vq_p, vcfg)
    assert maxabs(n(pipe.vqgan.decode_from_indice(torch.from_numpy(pred_ref).to(dev()))), img_ref) < TOL
    if not bad.any() and np.array_equal(n(ids1)[ids0.numpy() != V], ids0.numpy()[ids0.numpy() != V]):
        assert img1.shape == (1, 3, 256, 256)
    # (b) the call a user of the preset makes, in bf16
    pipe.set_compute_dtype(torch.bfloat16)
    text = [f"prompt {i}" for i in range(8)]
    eager = pipe.generate(text, timesteps=6, seed=11, return_ids=True, use_graph=False, streams=1)
    for _ in range(3):                                          # eager warm-up of the graph path, capture, replay
        fast = pipe.generate(text, timesteps=6, seed=11, return_ids=True)
        assert len(fast[0]) == len(eager[0]) == 3
        assert torch.equal(fast[1], eager[1])
        assert all(torch.equal(a, b) for a, b in zip(fast[0], eager[0]))
    assert torch.isfinite(eager[0][-1]).all() and int((eager[1] == V).sum(1).max()) == 1


@pytest.mark.parametrize("name,B", [("bench-text-24L-d768", 2), ("bench-text-24L-d1024-512px", 1)])
def test_large_text_configs_against_oracle(name, B):
    """BASELINE configs 4 and 5 (synthetic sizes the reference does not define): one MaskGIT step in fp32-verify mode
    against the numpy oracle on the same seeded weights -- logits within 1e-3, sampled ids equal wherever the
    oracle's top-2 logit gap is not a near-tie, and the vit decode of the oracle's ids within 1e-3."""
    from paintmind_amd.config import ver2cfg
    torch.manual_seed(3)
    pipe = Pipeline(pm.Config(ver2cfg[name]), stage1_pretrained=False).eval()
    p = {k: v.detach().numpy() for k, v in pipe.state_dict().items() if not k.startswith("text_model")}
    scfg, vcfg = ver2cfg[name], ver2cfg[ver2cfg[name]["stage1"]]
    pipe = pipe.to(dev())
    N, V = pipe.num_tokens, vcfg["n_embed"]
    g = torch.Generator().manual_seed(5)
    ids0 = torch.randint(0, V, (B, N), generator=g)
    ids0[torch.rand(B, N, generator=g) < 0.7] = V
    ctx = torch.randn(B, 77, scfg["context_dim"], generator=g)
    logits = pipe.tokens2logits(pipe.ids2tokens(ids0.to(dev())), ctx.to(dev()))
    ref = O.cond_transformer(O.ids2tokens(ids0.numpy(), p), ctx.numpy(), p, scfg)
    assert maxabs(n(logits), ref) < TOL
    ids1, img1 = pipe.sample(ids0.to(dev()), np.float64(0.3), text=ctx.to(dev()), topk=1, temperature=1.0)
    top2 = -np.sort(-ref, axis=-1)[..., :2]
    pred_ref = ref.argmax(-1)
    is_mask = ids0.numpy() == V
    got = n(ids1)
    # positions that stayed unmasked after the re-mask must carry the oracle's arg-max unless it is a near-tie
    kept = is_mask & (got != V)
    bad = kept & (got != pred_ref)
    assert np.all((top2[..., 0] - top2[..., 1])[bad] < 1e-4), int(bad.sum())
    vq_p = {k[len("vqgan."):]: v for k, v in p.items() if k.startswith("vqgan.")}
    img_ref = O.vqgan_decode_indices(pred_ref[:1], vq_p, vcfg)
    img_gpu = pipe.vqgan.decode_from_indice(torch.from_numpy(pred_ref[:1]).to(dev()))
    assert maxabs(n(img_gpu), img_ref) < TOL


# ---- masked-token objective, forward only (generate.py:78-146) ---------------------------------------
def test_tiny_pipeline_forward_loss_golden(tiny_pipe):
    pipe, p, _ = tiny_pipe
    tf = load_golden("tiny_forward.npz")[1]
    for i in range(4):
        x, mask = pipe.random_masking(t(tf["rm_x"]), float(tf[f"rm{i}_ratio"]), noise=t(tf[f"rm{i}_noise"]))
        assert np.array_equal(n(mask), tf[f"rm{i}_mask"]) and np.array_equal(n(x), tf[f"rm{i}_x"])
    loss = pipe.loss(t(tf["ce_logit"]), t(tf["ce_label"]), t(tf["ce_mask"]))
    assert loss.shape == () and abs(float(loss) - float(tf["ce_loss"])) < 1e-4
    text_model = pipe.text_model
    pipe.text_model = torch.nn.Identity()
    try:
        for tag, ctx in (("ctx", t(tf["context"])), ("noctx", None)):
            for j in range(2):
                loss = pipe(t(tf["img"]), ctx, mask_ratio=float(tf[f"fw_{tag}{j}_ratio"]), noise=t(tf[f"fw_{tag}{j}_noise"]))
                assert abs(float(loss) - float(tf[f"fw_{tag}{j}_loss"])) < TOL
        # default noise path: torch.rand on the device, loss of an untrained model is about log(V)
        assert 0.5 * np.log(64) < float(pipe(t(tf["img"]), None)) < 2 * np.log(64)
    finally:
        pipe.text_model = text_model


def test_generate_lane_failure_does_not_poison_the_host_pool(tiny_pipe, monkeypatch):
    """Pipeline.generate() with two lanes: when one lane raises, the call waits for the other lane and for every copy stream
    before the exception leaves, the pinned buffer of the failed call is never handed out again, and the next call is correct.
    PMHIP_GENERATE_STREAMS=1 is the process-wide opt-out of the lane default."""
    from paintmind_amd import generate as G
    pipe, _, _ = tiny_pipe
    text = [f"p{i}" for i in range(8)]
    pipe.set_compute_dtype(torch.bfloat16)
    try:
        want = pipe.generate(text, timesteps=4, seed=5, use_graph=False, streams=1)
        want = [w.clone() for w in want]
        pipe.generate(text, timesteps=4, seed=5, streams=2)
        lanes = pipe._lanes(2)
        eng1 = lanes[1][0]
        real = eng1.generate
        seen = []

        def boom(*a, **k):
            seen.append(k.get("host"))
            raise RuntimeError("injected lane failure")
        monkeypatch.setattr(eng1, "generate", boom)
        with pytest.raises(RuntimeError, match="injected lane failure"):
            pipe.generate(text, timesteps=4, seed=5, streams=2)
        failed_host = seen[0][0]
        assert all(b.untyped_storage().data_ptr() != failed_host.untyped_storage().data_ptr() for b in G._pinned_pool.bufs)
        monkeypatch.setattr(eng1, "generate", real)
        got = pipe.generate(text, timesteps=4, seed=5, streams=2)
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
        assert got[0].untyped_storage().data_ptr() != failed_host.untyped_storage().data_ptr()
        monkeypatch.setenv("PMHIP_GENERATE_STREAMS", "1")
        calls = []
        real_ids = pipe.generate_ids

        def spy(*a, **k):
            calls.append(k.get("streams"))
            return real_ids(*a, **k)
        monkeypatch.setattr(pipe, "generate_ids", spy)
        got = pipe.generate(text, timesteps=4, seed=5)
        assert calls == [1] and all(torch.equal(a, b) for a, b in zip(got, want))
    finally:
        pipe.set_compute_dtype(torch.float32)
