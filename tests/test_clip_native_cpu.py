"""The native OpenCLIP text tower without a GPU: the float64 restatement (tests/clip_ref.py) against the stub
tower run by torch, the C ABI of the three new operators (prototypes, exports, refusals that name their argument), what NativeClipText
refuses and how it packs, and the CPU rule: native=True on the CPU is the stock tower, bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import clip_ref as R
from clip_stubs import Tokenizer, clip_tower, params_of, run_stock
from paintmind_amd import _lib
from paintmind_amd.modules import clip_native as N
from paintmind_amd.modules.encoder import CLIPTextEmbedder
from text_stubs import StubClipTextTower, stub_clip_tokenize
from util import ROOT

TOWERS = [(128, 2), (192, 4)]
SHAPES = [(2, 77), (3, 24)]


def ids_of(shape, seed=5):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("layer", ["last", "penultimate"])
@pytest.mark.parametrize("quick", [False, True], ids=["erf", "quick"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("width, layers", TOWERS)
def test_float64_restatement_matches_the_stub_tower_in_f32(width, layers, shape, quick, layer):
    tower = clip_tower(width, layers, quick, n_ctx=shape[1])
    ids = ids_of(shape)
    emb = CLIPTextEmbedder(model=tower, tokenizer=Tokenizer(shape[1]), layer=layer)
    with torch.no_grad():
        want = emb.encode_with_transformer(ids).numpy()
    got = R.tower(params_of(tower), ids.numpy(), "quick" if quick else "erf", skip_last=emb.skip_last)
    err = float(np.abs(got - want).max())
    print(f"restatement vs torch f32 W={width} x{layers} {shape} {layer}: max abs {err:.3g}, output RMS {R.rms(want):.3f}")
    assert got.shape == (shape[0], shape[1], width)
    assert err <= 1e-4
    assert np.array_equal(want, run_stock(tower, ids, emb.skip_last).numpy())      # the helper the bf16 comparison uses is that call


def test_restatement_is_causal_and_penultimate_drops_the_last_block():
    tower = clip_tower(128, 3, n_ctx=24)
    P = params_of(tower)
    ids = ids_of((2, 24)).numpy()
    base = R.tower(P, ids, "erf")
    for j in (1, 7, 23):
        other = ids.copy()
        other[:, j:] = (other[:, j:] + 1 + np.arange(24 - j)) % 256
        moved = R.tower(P, other, "erf")
        assert np.array_equal(moved[:, :j], base[:, :j])                           # rows < j never see the tokens >= j
        assert not np.array_equal(moved[:, j:], base[:, j:])
    shorter = {k: v for k, v in P.items() if not k.startswith("transformer.resblocks.2.")}
    assert np.array_equal(R.tower(P, ids, "erf", skip_last=1), R.tower(shorter, ids, "erf"))
    assert not np.array_equal(R.tower(P, ids, "erf", skip_last=1), base)


def test_operator_restatements_agree_with_torch():
    x = torch.linspace(-9, 9, 3001, dtype=torch.float64)
    assert np.allclose(R.gelu_erf(x.numpy()), nn.functional.gelu(x).numpy(), rtol=1e-13, atol=2e-15)
    assert np.allclose(R.gelu_quick(x.numpy()), (x * torch.sigmoid(1.702 * x)).numpy(), rtol=1e-13, atol=2e-15)
    assert -1e-13 < R.gelu_erf(np.array([-8.0]))[0] < 0                             # the erfc form does not cancel to 0 at negative x
    b = R.gelu_bound(np.array([0.0, -1.0, 1.0, -6.0, 40.0, -40.0, 1e30, -1e30]), "erf")
    assert np.all(b > 0) and np.all(np.isfinite(b)) and b[1] < 2e-7 and b[3] < 1e-13
    b = R.gelu_bound(np.array([0.0, -1.0, 1.0, -6.0, 40.0, -40.0, 1e30, -1e30]), "quick")
    assert np.all(b > 0) and np.all(np.isfinite(b)) and b[1] < 2e-7
    torch.manual_seed(0)
    q, k, v = (torch.randn(1, 2, 9, 64, dtype=torch.float64) for _ in range(3))
    want = nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True, scale=1.0).permute(0, 2, 1, 3).reshape(1, 9, 128)
    ref, bound = R.attention_causal(q.numpy(), k.numpy(), v.numpy())
    assert np.allclose(ref, want.numpy(), rtol=0, atol=1e-12) and np.all(bound > 0)
    u = torch.randn(10, 3 * 128 + 8).float().numpy()
    qh, vh, kh = R.split_heads(u, 2, 5, 3, 0.125, (0, 2, 1))
    assert qh.shape == (2, 2, 5, 64) and vh.shape == (2, 2, 64, 5) and kh.shape == (2, 2, 5, 64)
    assert qh[1, 1, 3, 7] == np.float32(u[8, 64 + 7] * np.float32(0.125)) and vh[1, 0, 9, 2] == u[7, 128 + 9] and kh[0, 1, 4, 63] == u[4, 256 + 127]


NEW = ("pmhip_attention_causal", "pmhip_split_heads", "pmhip_gelu")


def test_prototypes_agree_with_the_header_and_the_library_exports_them():
    hdr = open(os.path.join(ROOT, "include", "pmhip.h")).read()
    assert "#define PMHIP_ABI_VERSION 11" in hdr and _lib.ABI_VERSION == 11
    lib = _lib.load()
    assert lib.pmhip_abi_version() == 11
    for name in NEW:
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert decl, f"{name} is not declared in include/pmhip.h"
        params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
        res, argtypes = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(params) == len(argtypes), (name, params)
        for p, ty in zip(params, argtypes):
            pointer = "*" in p or p.startswith("pmhip_stream")
            assert pointer == (ty is C.c_void_p or hasattr(ty, "contents")), (name, p, ty)
            if not pointer:
                assert ty is (C.c_float if p.startswith("float") else C.c_int), (name, p, ty)
        assert hasattr(lib, name)


def test_refusals_name_their_argument():
    """Arguments are validated before anything is launched, so dummy pointers do."""
    lib = _lib.load()
    p = C.c_void_p(256)
    F32, BF16 = _lib.F32, _lib.BF16

    def rejected(rc, *names):
        msg = lib.pmhip_last_error()
        assert rc == _lib.PMHIP_EINVAL and all(n.encode() in msg for n in names), (rc, msg)

    rejected(lib.pmhip_attention_causal(BF16, p, p, p, p, 128, 1, 2, 77, 78, None), "L_pad=78")
    rejected(lib.pmhip_attention_causal(BF16, p, p, p, p, 128, 1, 2, 77, 76, None), "L_pad=76")
    rejected(lib.pmhip_attention_causal(F32, p, p, p, p, 64, 1, 2, 77, 80, None), "ldo=64")
    rejected(lib.pmhip_attention_causal(F32, p, p, p, p, 130, 1, 2, 77, 80, None), "ldo=130")
    rejected(lib.pmhip_attention_causal(2, p, p, p, p, 128, 1, 2, 77, 80, None), "dtype")
    rejected(lib.pmhip_attention_causal(F32, p, None, p, p, 128, 1, 2, 77, 80, None), "null")
    rejected(lib.pmhip_attention_causal(F32, p, p, p, p, 128, 1, 2, 0, 80, None), "L=0")
    rejected(lib.pmhip_attention_causal(F32, p, p, p, p, 128, 1, 2, (1 << 20) + 1, 1 << 21, None), "L=1048577")
    rejected(lib.pmhip_attention_causal(F32, p, C.c_void_p(264), p, p, 128, 1, 2, 77, 80, None), "aligned")
    rejected(lib.pmhip_attention_causal(F32, p, p, p, p, 128, 0, 2, 77, 80, None), "B=0")
    kinds, outs = (C.c_int * 3)(0, 1, 2), (C.c_void_p * 3)(256, 256, 256)
    rejected(lib.pmhip_split_heads(F32, p, 380, 10, 2, 5, 8, 3, kinds, outs, 1.0, None), "ldu=380")
    rejected(lib.pmhip_split_heads(F32, p, 386, 10, 2, 5, 8, 3, kinds, outs, 1.0, None), "ldu=386")
    rejected(lib.pmhip_split_heads(F32, p, 384, 11, 2, 5, 8, 3, kinds, outs, 1.0, None), "M=11")
    rejected(lib.pmhip_split_heads(F32, p, 384, 10, 2, 5, 4, 3, kinds, outs, 1.0, None), "tokens_pad=4")
    rejected(lib.pmhip_split_heads(F32, p, 384, 10, 2, 5, 8, 4, kinds, outs, 1.0, None), "nparts=4")
    rejected(lib.pmhip_split_heads(F32, p, 384, 10, 2, 5, 8, 3, (C.c_int * 3)(0, 1, 3), outs, 1.0, None), "kind 3")
    rejected(lib.pmhip_split_heads(F32, p, 384, 10, 2, 5, 8, 3, kinds, (C.c_void_p * 3)(256, 0, 256), 1.0, None), "part 1")
    rejected(lib.pmhip_split_heads(3, p, 384, 10, 2, 5, 8, 3, kinds, outs, 1.0, None), "dtype")
    rejected(lib.pmhip_split_heads(F32, None, 384, 10, 2, 5, 8, 3, kinds, outs, 1.0, None), "NULL")
    rejected(lib.pmhip_gelu(p, 60, p, 64, F32, 4, 64, 0, None), "ldu=60")
    rejected(lib.pmhip_gelu(p, 64, p, 66, F32, 4, 64, 0, None), "ldo=66")
    rejected(lib.pmhip_gelu(p, 64, p, 64, F32, 4, 62, 0, None), "F=62")
    rejected(lib.pmhip_gelu(p, 64, p, 64, F32, 4, 64, 2, None), "kind 2")
    rejected(lib.pmhip_gelu(p, 64, p, 64, 5, 4, 64, 0, None), "out_dtype")
    rejected(lib.pmhip_gelu(p, 64, None, 64, F32, 4, 64, 0, None), "null")


# ---------------------------------------------------------------------------------------------------------------------------------
# what NativeClipText refuses
# ---------------------------------------------------------------------------------------------------------------------------------
class LayerScale(nn.Module):
    def forward(self, x):
        return 0.5 * x


def _wide_heads(t):
    t.transformer.resblocks[1].attn = nn.MultiheadAttention(128, 4)


def _own_attention(t):
    t.transformer.resblocks[0].attn = nn.Linear(128, 128)


def _separate_projections(t):
    t.transformer.resblocks[0].attn = nn.MultiheadAttention(128, 2, kdim=96, vdim=96)


def _no_in_proj_bias(t):
    t.transformer.resblocks[0].attn = nn.MultiheadAttention(128, 2, bias=False)


def _no_mask(t):
    t.attn_mask = None


def _full_mask(t):
    t.attn_mask = torch.zeros(77, 77)


def _shifted_mask(t):
    t.attn_mask = torch.full((77, 77), float("-inf")).triu_(2)


def _finite_mask(t):
    t.attn_mask = torch.full((77, 77), -1e4).triu_(1)


def _layer_scale(name):
    def edit(t):
        setattr(t.transformer.resblocks[1], name, LayerScale())
    return edit


def _unnamed_mlp(t):
    t.transformer.resblocks[0].mlp = nn.Sequential(nn.Linear(128, 512), nn.GELU(), nn.Linear(512, 128))


def _tanh_gelu(t):
    t.transformer.resblocks[1].mlp.gelu = nn.GELU(approximate="tanh")


def _relu(t):
    t.transformer.resblocks[1].mlp.gelu = nn.ReLU()


def _half(t):
    t.to(torch.bfloat16)


REFUSALS = [(_wide_heads, r"heads=4.*heads \* 64"), (_own_attention, "nn.MultiheadAttention"), (_separate_projections, "in_proj_weight"),
            (_no_in_proj_bias, "in_proj_bias"), (_no_mask, "attn_mask is missing"), (_full_mask, "not the causal matrix"),
            (_shifted_mask, "not the causal matrix"), (_finite_mask, "not the causal matrix"), (_layer_scale("ls_1"), r"ls_1 must be nn.Identity"),
            (_layer_scale("ls_2"), r"ls_2 must be nn.Identity"), (_unnamed_mlp, "c_fc, an activation, c_proj"), (_tanh_gelu, "activation"),
            (_relu, "activation"), (_half, "float32")]


@pytest.mark.parametrize("edit, message", REFUSALS, ids=[e.__name__ if e.__name__ != "edit" else f"layer_scale_{i}" for i, (e, _) in enumerate(REFUSALS)])
def test_a_tower_the_kernels_do_not_serve_is_refused_at_construction(edit, message):
    tower = clip_tower(128, 2)
    edit(tower)
    with pytest.raises(ValueError, match=message):
        N.NativeClipText(tower)
    with pytest.raises(ValueError, match=message):
        CLIPTextEmbedder(model=tower, tokenizer=Tokenizer(), native=True)
    emb = CLIPTextEmbedder(model=tower, tokenizer=Tokenizer())                      # the default serves every tower, as before
    with pytest.raises(ValueError, match=message):
        emb.use_native()
    assert not emb.native


def test_the_width_96_stub_of_the_existing_tests_is_refused_by_design():
    """tests/text_stubs.py's tower: width 96 is no multiple of 64 (and its MLP has ratio 2 and no c_fc / c_proj names)"""
    with pytest.raises(ValueError, match="width=96"):
        N.NativeClipText(StubClipTextTower())
    with pytest.raises(ValueError, match="width=96"):
        CLIPTextEmbedder(model=StubClipTextTower(), tokenizer=stub_clip_tokenize, native=True)
    emb = CLIPTextEmbedder(model=StubClipTextTower(), tokenizer=stub_clip_tokenize)
    assert emb(["a cat"]).shape == (1, 77, 96) and not emb.native
    wide = StubClipTextTower(width=128, heads=2)                                   # a served width: its blocks lack the open_clip names
    with pytest.raises(ValueError, match="ls_1 must be nn.Identity"):
        N.NativeClipText(wide)


def test_packing_shapes_dtypes_and_repacking():
    tower = clip_tower(128, 3, quick=True)
    enc = N.NativeClipText(tower, skip_last=1)
    assert (enc.width, enc.heads, enc.kinds, enc.skip_last) == (128, 2, ["quick"] * 3, 1)
    assert N.NativeClipText(clip_tower(192, 1)).kinds == ["erf"]
    for dtype in (torch.float32, torch.bfloat16):
        pack = enc.packed(dtype)
        assert len(pack["layers"]) == 3 and pack["embed"] is tower.token_embedding.weight and pack["pos"] is tower.positional_embedding
        assert pack["final_w"].dtype == pack["final_b"].dtype == torch.float32 and pack["final_w"].shape == (128,)
        assert pack["final_eps"] == tower.ln_final.eps
        for lw, blk in zip(pack["layers"], tower.transformer.resblocks):
            assert lw["qkv"].shape == (384, 128) and lw["o"].shape == (128, 128) and lw["fc"].shape == (512, 128) and lw["proj"].shape == (128, 512)
            assert all(lw[k].dtype == dtype and lw[k].is_contiguous() for k in ("qkv", "o", "fc", "proj"))
            for k, width in (("qkv_b", 384), ("o_b", 128), ("fc_b", 512), ("proj_b", 128), ("ln1_w", 128), ("ln1_b", 128), ("ln2_w", 128), ("ln2_b", 128)):
                assert lw[k].dtype == torch.float32 and lw[k].shape == (width,), k
            assert torch.equal(lw["qkv"], blk.attn.in_proj_weight.to(dtype)) and torch.equal(lw["qkv_b"], blk.attn.in_proj_bias)
            assert torch.equal(lw["o"], blk.attn.out_proj.weight.to(dtype)) and torch.equal(lw["o_b"], blk.attn.out_proj.bias)
            assert torch.equal(lw["fc"], blk.mlp.c_fc.weight.to(dtype)) and torch.equal(lw["proj_b"], blk.mlp.c_proj.bias)
            assert torch.equal(lw["ln1_w"], blk.ln_1.weight) and torch.equal(lw["ln2_b"], blk.ln_2.bias)
            assert lw["eps1"] == blk.ln_1.eps and lw["eps2"] == blk.ln_2.eps and lw["act"] == "quick"
    assert enc.packed(torch.float32) is enc.packed(torch.float32)                  # cached
    first = enc.packed(torch.float32)
    with torch.no_grad():
        tower.transformer.resblocks[1].attn.in_proj_bias.add_(1.0)                 # an in-place edit re-packs
    again = enc.packed(torch.float32)
    assert again is not first and torch.equal(again["layers"][1]["qkv_b"], tower.transformer.resblocks[1].attn.in_proj_bias)
    assert [k[1] for k in enc._packs] == [torch.float32]                           # the stale bf16 packing went with it
    tower.load_state_dict(clip_tower(128, 3, quick=True, seed=9).state_dict())     # and so does load_state_dict
    assert enc.packed(torch.float32) is not again
    assert torch.equal(enc.packed(torch.float32)["layers"][0]["proj"], tower.transformer.resblocks[0].mlp.c_proj.weight)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        enc(ids_of((1, 77)))


def test_native_on_the_cpu_is_the_stock_tower():
    text = ["a cat on a mat", "dog"]
    for layer in CLIPTextEmbedder.LAYERS:
        a = CLIPTextEmbedder(model=clip_tower(), tokenizer=Tokenizer(), layer=layer)
        b = CLIPTextEmbedder(model=clip_tower(), tokenizer=Tokenizer(), layer=layer, native=True)
        assert b.native and not a.native and b.compute_dtype == torch.float32 and b._native.skip_last == a.skip_last
        assert list(a.state_dict()) == list(b.state_dict()) and all(k.startswith("model.") for k in b.state_dict())
        assert torch.equal(a(text), b(text))
        (ca, la), (cb, lb) = a(text, return_lens=True), b(text, return_lens=True)
        assert torch.equal(ca, cb) and torch.equal(la, lb) and la.tolist() == [16, 5]
        assert b.use_native(False) is b and not b.native and torch.equal(a(text), b(text))
        keys = list(a.state_dict())
        assert a.use_native() is a and a.native and list(a.state_dict()) == keys   # use_native() adds no key
    for call in (lambda: b(text, weighted=True), lambda: b.phrase_rows(text, ["cat", "dog"]), lambda: b.fragment_ids([["a"]])):
        with pytest.raises(NotImplementedError):
            call()


def test_pipeline_round_trip_and_set_compute_dtype():
    import paintmind_amd as pm
    from paintmind_amd.generate import Pipeline
    cfg = pm.Config(dict(pm.ver2cfg["tiny-pipeline"], context_dim=128))
    emb = CLIPTextEmbedder(model=clip_tower(), tokenizer=Tokenizer(), native=True)
    pipe = Pipeline(cfg, stage1_pretrained=False, text_model=emb)
    sd = pipe.state_dict()
    text_keys = [k for k in sd if k.startswith("text_model.")]
    assert text_keys and all(k.startswith("text_model.model.") for k in text_keys)
    plain = Pipeline(cfg, stage1_pretrained=False, text_model=CLIPTextEmbedder(model=clip_tower(seed=3), tokenizer=Tokenizer()))
    assert list(plain.state_dict()) == list(sd)
    plain.load_state_dict(sd)
    assert torch.equal(plain.text_model(["a cat"]), emb(["a cat"]))
    before = emb(["a cat"])
    pipe.set_compute_dtype(torch.bfloat16)
    assert emb.compute_dtype == torch.bfloat16 and emb._pm_dtype == torch.bfloat16
    assert torch.equal(emb(["a cat"]), before)                                     # on the CPU the stock tower runs, in its own dtype
    assert not any(k.endswith("_pm_dtype") for k in pipe.state_dict())
