"""The native Flan-T5 tower on the GPU (paintmind_amd/modules/t5_native.py): fp32-verify against the float64
restatement of tests/t5_ref.py, bf16 against Hugging Face's own bf16 tower measured on the same restatement, and T5TextEmbedder(native=True)
through every entry that calls the tower, up to Pipeline.generate and a decode session.

Measured on an MI355X: fp32 max abs 1.7e-6 .. 3.9e-6 (bound 1e-3); bf16 RMS error native / Hugging Face bf16, both against float64:
tiny [2,77] 3.57e-3 / 6.69e-3 = 0.534, tiny [3,24] 4.04e-3 / 6.90e-3 = 0.584, four layers [2,77] 5.26e-3 / 9.38e-3 = 0.560, four layers
[3,24] 5.56e-3 / 9.82e-3 = 0.566, one XL-shaped layer [2,77] 2.59e-3 / 5.02e-3 = 0.517 (condition: <= 1)."""
import copy

import numpy as np
import pytest
import torch

import paintmind_amd as pm
import t5_ref as R
from gpu_common import dev, n
from oracle import paintmind_oracle as O
from paintmind_amd.generate import Pipeline
from paintmind_amd.modules.encoder import T5TextEmbedder
from paintmind_amd.modules.t5_native import NativeT5Encoder
from t5_stubs import CharTokenizer, gated_t5, params_of

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-3                      # the project's fp32 contract
FOUR_LAYER = dict(d_model=192, num_heads=3, d_ff=320, num_layers=4)
XL_LAYER = dict(d_model=2048, num_heads=32, d_ff=5120, num_layers=1)


def ids_of(shape, seed=5):
    return torch.randint(0, 128, shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("kw", [{}, FOUR_LAYER], ids=["tiny", "four_layer"])
@pytest.mark.parametrize("shape", [(2, 77), (3, 24)])
def test_fp32_tower_matches_the_float64_restatement(kw, shape):
    model = gated_t5(**kw)
    ids = ids_of(shape)
    ref = R.encoder(params_of(model), ids.numpy(), num_heads=model.config.num_heads)
    got = NativeT5Encoder(model.to(dev()))(ids.to(dev()), dtype=torch.float32)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    err = float(np.abs(n(got) - ref).max())
    print(f"native f32 vs float64 {kw or 'tiny'} {shape}: max abs {err:.3g}, output RMS {R.rms(n(got)):.4f}")
    assert err <= FP32_TOL
    assert abs(R.rms(n(got)) - 1.0) < 0.05 * max(1.0, float(np.abs(n(model.encoder.final_layer_norm.weight) - 1).max()) * 20)
    # a key count per prompt: Hugging Face's attention_mask in the restatement
    lens = [shape[1], 5, 1][:shape[0]]
    ref = R.encoder(params_of(model), ids.numpy(), num_heads=model.config.num_heads, kv_lens=lens)
    got = NativeT5Encoder(model)(ids.to(dev()), kv_lens=torch.tensor(lens, dtype=torch.int32), dtype=torch.float32)
    assert float(np.abs(n(got) - ref).max()) <= FP32_TOL


def bf16_ratio(model, ids, what):
    """(RMS error of the native bf16 tower) / (RMS error of Hugging Face's bf16 tower on the CPU), both against the float64 restatement"""
    ref = R.encoder(params_of(model), ids.numpy(), num_heads=model.config.num_heads)
    with torch.no_grad():
        hf = copy.deepcopy(model).to(torch.bfloat16)(input_ids=ids).last_hidden_state.float().numpy()
    got = n(NativeT5Encoder(model.to(dev()))(ids.to(dev()), dtype=torch.bfloat16))
    assert got.dtype == np.float32 and np.isfinite(got).all()
    e_nat, e_hf = R.rms(got - ref), R.rms(hf - ref)
    print(f"bf16 {what}: native RMS error {e_nat:.3g} (max {np.abs(got - ref).max():.3g}), HF bf16 RMS error {e_hf:.3g} "
          f"(max {np.abs(hf - ref).max():.3g}), ratio {e_nat / e_hf:.3f}")
    return e_nat / e_hf


@pytest.mark.parametrize("kw, shape", [({}, (2, 77)), ({}, (3, 24)), (FOUR_LAYER, (2, 77)), (FOUR_LAYER, (3, 24))],
                         ids=["tiny_77", "tiny_24", "four_layer_77", "four_layer_24"])
def test_bf16_tower_is_no_worse_than_hugging_faces_bf16(kw, shape):
    """native keeps the residual stream and every accumulation in f32 where Hugging Face's bf16 tower rounds the stream at every
    operator: RMS error of native <= RMS error of HF bf16, both against float64"""
    assert bf16_ratio(gated_t5(**kw), ids_of(shape), f"{kw or 'tiny'} {shape}") <= 1.0


def test_bf16_one_xl_shaped_layer():
    """d_model 2048, 32 heads, d_ff 5120: the smallest case that runs the D = 2048 rows and the K = 2048 / 5120 GEMM shapes"""
    assert bf16_ratio(gated_t5(**XL_LAYER), ids_of((2, 77)), "one XL-shaped layer (2, 77)") <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the public interface
# ---------------------------------------------------------------------------------------------------------------------------------
TEXT = ["a cat on a mat", "dog"]


def embedders(**kw):
    a = T5TextEmbedder(tokenizer=CharTokenizer(), transformer=gated_t5(), **kw).to(dev())
    b = T5TextEmbedder(tokenizer=CharTokenizer(), transformer=gated_t5(), native=True, **kw).to(dev())
    return a, b


def close(x, y):
    assert x.shape == y.shape and x.dtype == y.dtype == torch.float32 and x.is_cuda and y.is_cuda
    err = float((x - y).abs().max())
    assert err <= FP32_TOL, err


def test_native_embedder_serves_every_entry_that_calls_the_tower():
    a, b = embedders()
    assert list(a.state_dict()) == list(b.state_dict())
    close(a(TEXT), b(TEXT))
    (ca, la), (cb, lb) = a(TEXT, return_lens=True), b(TEXT, return_lens=True)
    close(ca, cb)
    assert torch.equal(la, lb)
    wa, wb = a(["a (cat:1.5) on a mat", "dog"], weighted=True), b(["a (cat:1.5) on a mat", "dog"], weighted=True)
    close(wa[0], wb[0])
    assert torch.equal(wa[1], wb[1]) and torch.equal(wa[2], wb[2])
    pa, pb = a.phrase_rows(TEXT, ["cat", "dog"]), b.phrase_rows(TEXT, ["cat", "dog"])
    close(pa[0], pb[0])
    assert torch.equal(pa[1], pb[1]) and torch.equal(pa[2], pb[2])
    fa, fb = a.fragment_ids([["a ", "cat"], ["dog"]]), b.fragment_ids([["a ", "cat"], ["dog"]])
    close(fa[0], fb[0])
    assert torch.equal(fa[1], fb[1]) and fa[2:] == fb[2:]


def test_padding_mask_reaches_the_native_tower_as_kv_lens():
    a, b = embedders(encoder_padding_mask=True)
    plain = T5TextEmbedder(tokenizer=CharTokenizer(), transformer=gated_t5(), native=True).to(dev())
    close(a(TEXT), b(TEXT))
    assert float((b(TEXT) - plain(TEXT)).abs().max()) > 1e-2                            # a short prompt's context differs


def test_load_state_dict_repacks_and_autocast_switches_the_mode():
    _, b = embedders()
    first = b(TEXT)
    other = gated_t5(seed=11)
    b.transformer.load_state_dict(other.state_dict())
    want = T5TextEmbedder(tokenizer=CharTokenizer(), transformer=other).to(dev())(TEXT)
    close(b(TEXT), want)
    assert float((b(TEXT) - first).abs().max()) > 1e-2
    packs = b._native._packs
    assert [k[1] for k in packs] == [torch.float32]
    assert list(next(iter(packs.values()))[1]["tables"]) == [77]                        # the bias table, one per L, lives with the packing
    f32_pack = next(iter(packs.values()))[1]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert b.compute_dtype == torch.bfloat16
        low = b(TEXT)
    assert b.compute_dtype == torch.float32 and low.dtype == torch.float32
    assert sorted(str(k[1]) for k in b._native._packs) == ["torch.bfloat16", "torch.float32"]
    assert next(v[1] for k, v in b._native._packs.items() if k[1] == torch.float32) is f32_pack      # the f32 packing is alive
    diff = float((low - want).abs().max())
    assert 1e-5 < diff < 0.25, diff                                                     # bf16 arithmetic, the same function
    close(b(TEXT), want)


def test_native_tower_feeds_generate_and_a_decode_session():
    """the check test_t5_text_tower_feeds_generate_on_the_gpu makes for the Hugging Face tower, on the native context"""
    emb = T5TextEmbedder(tokenizer=CharTokenizer(), transformer=gated_t5(), native=True)
    torch.manual_seed(4)
    cfg = dict(pm.ver2cfg["tiny-pipeline"], context_dim=128)
    pipe = Pipeline(pm.Config(cfg), stage1_pretrained=False, text_model=emb).to(dev()).eval()
    ctx = pipe.text_model(["a cat", "a dog"])
    assert ctx.shape == (2, 77, 128) and ctx.is_cuda
    imgs, ids = pipe.generate(["a cat", "a dog"], timesteps=4, topk=3, seed=1, return_ids=True)
    assert len(imgs) == 2 and torch.isfinite(imgs[-1]).all()
    p = {k: v.detach().cpu().numpy() for k, v in pipe.state_dict().items() if not k.startswith("text_model")}
    ids0 = torch.full((2, 16), 64, dtype=torch.long, device=dev())
    ids1, _ = pipe.sample(ids0, np.float64(0.5), text=ctx, topk=1, temperature=1.0)
    ids1_o, _, _ = O.sample_step(n(ids0), np.float64(0.5), n(ctx), 1, 1.0, np.full((2, 16, 64), 0.5, np.float32), p,
                                 pm.ver2cfg["tiny-vqgan"], cfg)
    assert np.array_equal(n(ids1), ids1_o)
    # a decode session's submit(text=) equals its generate_ids row
    session = pipe.decode_session(slots=2, conditional=True)
    requests = [("a cat", 4, 21), ("a dog", 3, 22)]
    for tx, T, seed in requests:
        session.submit(text=tx, timesteps=T, topk=3, seed=seed, image_index=0)      # generate([tx]) draws image 0's noise
    done = session.drain()
    assert sorted(f.handle.number for f in done) == [0, 1]
    for f in done:
        tx, T, seed = requests[f.handle.number]
        _, want = pipe.generate([tx], timesteps=T, topk=3, save_interval=1, seed=seed, return_ids=True)
        assert torch.equal(f.ids, want[0]), f.handle
