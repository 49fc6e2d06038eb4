"""The native OpenCLIP text tower on the GPU (paintmind_amd/modules/clip_native.py): fp32-verify against the
float64 restatement of tests/clip_ref.py, bf16 against the stock tower in bf16 measured on the same restatement, and
CLIPTextEmbedder(native=True) up to Pipeline.generate.

Measured on an MI355X: fp32 max abs 7.1e-7 .. 1.7e-6 (bound 1e-3); bf16 RMS error native / stock bf16, both against float64: width 128
x 2 layers [2,77] 0.234 (erf) / 0.230 (quick), [3,24] 0.273 / 0.270; width 192 x 4 layers [2,77] 0.277 / 0.274, [3,24] 0.296 / 0.299; one
ViT-L-shaped layer [2,77] 0.194 (condition: <= 1).  Every test prints its own figures."""
import copy

import numpy as np
import pytest
import torch

import clip_ref as R
import paintmind_amd as pm
from clip_stubs import Tokenizer, clip_tower, params_of, run_stock
from gpu_common import dev, n
from paintmind_amd.generate import Pipeline
from paintmind_amd.modules.clip_native import NativeClipText
from paintmind_amd.modules.encoder import CLIPTextEmbedder

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-3                      # the project's fp32 contract
TOWERS = [(128, 2), (192, 4)]
SHAPES = [(2, 77), (3, 24)]
KINDS = [False, True]


def ids_of(shape, seed=5):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed))


def kind_of(quick):
    return "quick" if quick else "erf"


@pytest.mark.parametrize("layer", ["last", "penultimate"])
@pytest.mark.parametrize("quick", KINDS, ids=["erf", "quick"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("width, layers", TOWERS)
def test_fp32_tower_matches_the_float64_restatement(width, layers, shape, quick, layer):
    tower = clip_tower(width, layers, quick, n_ctx=shape[1])
    ids = ids_of(shape)
    skip = {"last": 0, "penultimate": 1}[layer]
    ref = R.tower(params_of(tower), ids.numpy(), kind_of(quick), skip_last=skip)
    got = NativeClipText(tower.to(dev()), skip)(ids.to(dev()), dtype=torch.float32)
    assert got.dtype == torch.float32 and got.shape == ref.shape and got.is_cuda
    err = float(np.abs(n(got) - ref).max())
    print(f"native f32 vs float64 W={width} x{layers} {shape} {kind_of(quick)} {layer}: max abs {err:.3g}, output RMS {R.rms(n(got)):.4f}")
    assert err <= FP32_TOL


def bf16_ratio(tower, ids, kind, what, skip=0):
    """(RMS error of the native bf16 tower) / (RMS error of the stock tower in bf16 on the CPU), both against the float64 restatement"""
    ref = R.tower(params_of(tower), ids.numpy(), kind, skip_last=skip)
    stock = run_stock(copy.deepcopy(tower).to(torch.bfloat16), ids, skip).float().numpy()
    got = n(NativeClipText(tower.to(dev()), skip)(ids.to(dev()), dtype=torch.bfloat16))
    assert got.dtype == np.float32 and np.isfinite(got).all()
    e_nat, e_stock = R.rms(got - ref), R.rms(stock - ref)
    print(f"bf16 {what}: native RMS error {e_nat:.3g} (max {np.abs(got - ref).max():.3g}), stock bf16 RMS error {e_stock:.3g} "
          f"(max {np.abs(stock - ref).max():.3g}), ratio {e_nat / e_stock:.3f}")
    return e_nat / e_stock


@pytest.mark.parametrize("quick", KINDS, ids=["erf", "quick"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("width, layers", TOWERS)
def test_bf16_tower_is_no_worse_than_the_stock_tower_in_bf16(width, layers, shape, quick):
    """native keeps the residual stream and every accumulation in f32 where the stock bf16 tower rounds the stream at every operator:
    RMS error of native <= RMS error of stock bf16, both against float64"""
    tower = clip_tower(width, layers, quick, n_ctx=shape[1])
    assert bf16_ratio(tower, ids_of(shape), kind_of(quick), f"W={width} x{layers} {shape} {kind_of(quick)}") <= 1.0


def test_bf16_one_vit_l_shaped_layer():
    """width 768, 12 heads, MLP 3072: the smallest case that runs the ViT-L-14 text tower's GEMM shapes"""
    assert bf16_ratio(clip_tower(768, 1), ids_of((2, 77)), "erf", "one ViT-L-shaped layer (2, 77)") <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the public interface
# ---------------------------------------------------------------------------------------------------------------------------------
TEXT = ["a cat on a mat", "dog"]


def embedders(**kw):
    a = CLIPTextEmbedder(model=clip_tower(), tokenizer=Tokenizer(), **kw).to(dev())
    b = CLIPTextEmbedder(model=clip_tower(), tokenizer=Tokenizer(), native=True, **kw)
    return a, b.to(dev())


def close(x, y):
    assert x.shape == y.shape and x.dtype == y.dtype == torch.float32 and x.is_cuda and y.is_cuda
    err = float((x - y).abs().max())
    assert err <= FP32_TOL, err


@pytest.mark.parametrize("layer", ["last", "penultimate"])
def test_native_embedder_follows_to_and_equals_the_direct_call(layer):
    a, b = embedders(layer=layer)                                                       # b was built on the CPU and moved: it re-packs
    assert list(a.state_dict()) == list(b.state_dict()) and b.native
    close(a(TEXT), b(TEXT))
    (ca, la), (cb, lb) = a(TEXT, return_lens=True), b(TEXT, return_lens=True)
    close(ca, cb)
    assert torch.equal(la, lb)
    tokens = Tokenizer()(TEXT).to(dev())
    direct = NativeClipText(b.model, b.skip_last)(tokens, dtype=torch.float32)
    assert torch.equal(b(TEXT), direct) and torch.equal(b.encode_with_transformer(tokens), direct)
    if layer == "last":
        assert float((b(TEXT) - CLIPTextEmbedder(model=b.model, tokenizer=Tokenizer(), layer="penultimate", native=True)(TEXT)).abs().max()) > 1e-2
    # native off on the GPU is the stock path, bit for bit
    b.use_native(False)
    assert not b.native and torch.equal(b(TEXT), a(TEXT)) and torch.equal(a(TEXT), run_stock(a.model, tokens, a.skip_last))
    # a tower that is replaced after use_native() is wrapped again
    b.use_native()
    b.model = clip_tower(seed=11).to(dev())
    close(b(TEXT), CLIPTextEmbedder(model=clip_tower(seed=11), tokenizer=Tokenizer(), layer=layer).to(dev())(TEXT))
    assert b._native.model is b.model


def test_rows_before_j_do_not_change_with_the_tokens_from_j():
    _, b = embedders()
    tokens = ids_of((2, 77)).to(dev())
    for dtype in (torch.float32, torch.bfloat16):
        b._pm_dtype = dtype
        base = b.encode_with_transformer(tokens)
        for j in (1, 16, 17, 40, 76):
            other = tokens.clone()
            other[:, j:] = (other[:, j:] + 7) % 256
            moved = b.encode_with_transformer(other)
            assert torch.equal(moved[:, :j], base[:, :j]), (dtype, j)                   # bit for bit
            assert not torch.equal(moved[:, j:], base[:, j:])


def test_load_state_dict_repacks_and_both_dtype_switches_work():
    _, b = embedders()
    first = b(TEXT)
    other = clip_tower(seed=11)
    b.model.load_state_dict(other.state_dict())
    want = CLIPTextEmbedder(model=other, tokenizer=Tokenizer()).to(dev())(TEXT)
    close(b(TEXT), want)
    assert float((b(TEXT) - first).abs().max()) > 1e-2
    assert [k[1] for k in b._native._packs] == [torch.float32]
    f32_pack = next(iter(b._native._packs.values()))[1]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert b.compute_dtype == torch.bfloat16
        low = b(TEXT)
    assert b.compute_dtype == torch.float32 and low.dtype == torch.float32
    assert sorted(str(k[1]) for k in b._native._packs) == ["torch.bfloat16", "torch.float32"]
    assert next(v[1] for k, v in b._native._packs.items() if k[1] == torch.float32) is f32_pack      # the f32 packing is alive
    diff = float((low - want).abs().max())
    assert 1e-5 < diff < 0.25, diff                                                     # bf16 arithmetic, the same function
    close(b(TEXT), want)
    # Pipeline.set_compute_dtype reaches the embedder
    cfg = pm.Config(dict(pm.ver2cfg["tiny-pipeline"], context_dim=128))
    pipe = Pipeline(cfg, stage1_pretrained=False, text_model=b).to(dev()).eval()
    pipe.set_compute_dtype(torch.bfloat16)
    assert b.compute_dtype == torch.bfloat16 and torch.equal(b(TEXT), low)
    pipe.set_compute_dtype(torch.float32)
    close(b(TEXT), want)
    with pytest.raises(ValueError, match="positional_embedding has 77 rows"):
        b.encode_with_transformer(ids_of((2, 24)).to(dev()))


def test_native_tower_feeds_generate():
    emb = CLIPTextEmbedder(model=clip_tower(), tokenizer=Tokenizer(), native=True)
    torch.manual_seed(4)
    cfg = dict(pm.ver2cfg["tiny-pipeline"], context_dim=128)
    pipe = Pipeline(pm.Config(cfg), stage1_pretrained=False, text_model=emb).to(dev()).eval()
    ctx = pipe.text_model(["a cat", "a dog"])
    assert ctx.shape == (2, 77, 128) and ctx.is_cuda and emb.native
    imgs, ids = pipe.generate(["a cat", "a dog"], timesteps=4, topk=3, seed=1, return_ids=True)
    assert len(imgs) == 2 and torch.isfinite(imgs[-1]).all()
    # the same pipeline with the stock tower: the contexts agree to the fp32 contract
    emb.use_native(False)
    close(pipe.text_model(["a cat", "a dog"]), ctx)
