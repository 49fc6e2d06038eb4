"""The native Flan-T5 tower without a GPU: the bucket table against Hugging Face's own rule, the float64
restatement (tests/t5_ref.py) against the Hugging Face tower, the C ABI of the three new operators (prototypes, exports, refusals
that name their argument), what NativeT5Encoder refuses and how it packs, and the CPU rule: native=True on the CPU is the Hugging
Face tower, bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import t5_ref as R
from paintmind_amd import _lib
from paintmind_amd.modules import t5_native as N
from paintmind_amd.modules.encoder import T5TextEmbedder
from t5_stubs import CharTokenizer as StubTokenizer, gated_t5, params_of
from util import ROOT


@pytest.mark.parametrize("L", [1, 2, 77, 129, 512])
def test_bucket_table_is_hugging_faces_rule(L):
    from transformers.models.t5.modeling_t5 import T5Attention
    pos = torch.arange(L)
    delta = pos[None, :] - pos[:, None]                                            # memory - context = key - query, [q, k]
    want = T5Attention._relative_position_bucket(delta, bidirectional=True, num_buckets=32, max_distance=128)
    line = N.relative_position_bucket(torch.arange(-(L - 1), L), 32, 128)         # one bucket per delta
    assert torch.equal(line[delta + L - 1], want)
    assert np.array_equal(R.bucket(np.arange(-(L - 1), L))[delta.numpy() + L - 1], want.numpy())
    torch.manual_seed(L)
    weight = torch.randn(32, 3)
    table = N.rel_bias_table(weight, L, 32, 128)
    assert table.shape == (3, 2 * L - 1) and table.dtype == torch.float32
    assert torch.equal(table[:, delta + L - 1], weight[want].permute(2, 0, 1))     # HF's position_bias [H, q, k]
    assert np.array_equal(R.bias_table(weight.numpy(), L), table.double().numpy())


@pytest.mark.parametrize("shape", [(3, 77), (3, 24)])
def test_float64_restatement_matches_the_hugging_face_tower(shape):
    model = gated_t5()
    ids = torch.randint(0, 128, shape, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        want = model(input_ids=ids).last_hidden_state.numpy()
    got = R.encoder(params_of(model), ids.numpy(), num_heads=2)
    err = float(np.abs(got - want).max())
    print(f"restatement vs HF f32 {shape}: max abs {err:.3g} on outputs up to {np.abs(want).max():.3g}")
    assert err <= 1e-4
    # with a key count per prompt: Hugging Face's attention_mask
    lens = [shape[1], 5, 1]
    mask = (torch.arange(shape[1])[None, :] < torch.tensor(lens)[:, None]).long()
    with torch.no_grad():
        want = model(input_ids=ids, attention_mask=mask).last_hidden_state.numpy()
    assert float(np.abs(R.encoder(params_of(model), ids.numpy(), num_heads=2, kv_lens=lens) - want).max()) <= 1e-4


NEW = ("pmhip_rmsnorm", "pmhip_geglu", "pmhip_attention_relbias")


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
            assert pointer == (ty is C.c_void_p), (name, p, ty)
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

    rejected(lib.pmhip_attention_relbias(BF16, p, p, p, p, 128, 1, 2, 77, 128, None, None, None), "rel_bias")
    rejected(lib.pmhip_attention_relbias(BF16, p, p, p, p, 128, 1, 2, 77, 76, p, None, None), "L_pad")
    rejected(lib.pmhip_attention_relbias(F32, p, p, p, p, 64, 1, 2, 77, 128, p, None, None), "ldo")
    rejected(lib.pmhip_attention_relbias(2, p, p, p, p, 128, 1, 2, 77, 128, p, None, None), "dtype")
    rejected(lib.pmhip_attention_relbias(F32, p, None, p, p, 128, 1, 2, 77, 128, p, None, None), "null")
    rejected(lib.pmhip_attention_relbias(F32, p, p, p, p, 128, 1, 2, 0, 128, p, None, None), "L=0")
    rejected(lib.pmhip_rmsnorm(p, p, 1e-6, p, F32, 4, 4100, None), "D=4100")
    rejected(lib.pmhip_rmsnorm(p, p, 1e-6, p, F32, 4, 66, None), "D=66")
    rejected(lib.pmhip_rmsnorm(p, p, 1e-6, p, 7, 4, 64, None), "out_dtype")
    rejected(lib.pmhip_rmsnorm(p, None, 1e-6, p, F32, 4, 64, None), "null")
    rejected(lib.pmhip_geglu(p, 120, p, 64, F32, 4, 64, None), "ldu")
    rejected(lib.pmhip_geglu(p, 128, p, 60, F32, 4, 64, None), "ldo")
    rejected(lib.pmhip_geglu(p, 128, p, 64, F32, 4, 62, None), "F=62")


@pytest.mark.parametrize("kw, field", [(dict(d_kv=16), "d_kv"), (dict(feed_forward_proj="relu"), "feed_forward_proj"),
                                       (dict(d_model=96), "d_model"), (dict(d_ff=100), "d_ff")])
def test_a_tower_the_kernels_do_not_serve_is_refused_at_construction(kw, field):
    model = gated_t5(**kw)
    with pytest.raises(ValueError, match=field):
        N.NativeT5Encoder(model)
    with pytest.raises(ValueError, match=field):
        T5TextEmbedder(tokenizer=StubTokenizer(), transformer=model, native=True)
    T5TextEmbedder(tokenizer=StubTokenizer(), transformer=model)                   # the default serves every tower, as before


def test_packing_shapes_and_row_order():
    model = gated_t5(num_layers=3)
    enc = N.NativeT5Encoder(model)
    for dtype in (torch.float32, torch.bfloat16):
        pack = enc.packed(dtype)
        assert len(pack["layers"]) == 3 and pack["embed"] is model.shared.weight
        assert pack["final"].dtype == torch.float32 and pack["final"].shape == (128,)
        for lw, blk in zip(pack["layers"], model.encoder.block):
            sa, ff = blk.layer[0].SelfAttention, blk.layer[1].DenseReluDense
            assert lw["qkv"].shape == (3 * 2 * 64, 128) and lw["o"].shape == (128, 2 * 64)
            assert lw["wi"].shape == (2 * 192, 128) and lw["wo"].shape == (128, 192)
            assert all(lw[k].dtype == dtype and lw[k].is_contiguous() for k in ("qkv", "o", "wi", "wo"))
            assert all(lw[k].dtype == torch.float32 and lw[k].shape == (128,) for k in ("ln1", "ln2"))
            assert torch.equal(lw["qkv"][:128], sa.q.weight.to(dtype)) and torch.equal(lw["qkv"][128:256], sa.k.weight.to(dtype))
            assert torch.equal(lw["qkv"][256:], sa.v.weight.to(dtype)) and torch.equal(lw["o"], sa.o.weight.to(dtype))
            assert torch.equal(lw["wi"][:192], ff.wi_0.weight.to(dtype)) and torch.equal(lw["wi"][192:], ff.wi_1.weight.to(dtype))
            assert torch.equal(lw["wo"], ff.wo.weight.to(dtype))
            assert torch.equal(lw["ln1"], blk.layer[0].layer_norm.weight) and torch.equal(lw["ln2"], blk.layer[1].layer_norm.weight)
    assert enc.packed(torch.float32) is enc.packed(torch.float32)                  # cached
    first = enc.packed(torch.float32)
    with torch.no_grad():
        model.encoder.block[1].layer[0].SelfAttention.k.weight.add_(1.0)           # an in-place edit re-packs
    again = enc.packed(torch.float32)
    assert again is not first
    assert torch.equal(again["layers"][1]["qkv"][128:256], model.encoder.block[1].layer[0].SelfAttention.k.weight)
    model.load_state_dict(gated_t5(seed=9, num_layers=3).state_dict())             # and so does load_state_dict
    assert torch.equal(enc.packed(torch.float32)["layers"][0]["wo"], model.encoder.block[0].layer[1].DenseReluDense.wo.weight)


def test_native_on_the_cpu_is_the_hugging_face_tower():
    a = T5TextEmbedder(tokenizer=StubTokenizer(), transformer=gated_t5())
    b = T5TextEmbedder(tokenizer=StubTokenizer(), transformer=gated_t5(), native=True)
    assert b.native and not a.native and b.compute_dtype == torch.float32
    assert list(a.state_dict()) == list(b.state_dict()) and all(k.startswith("transformer.") for k in b.state_dict())
    text = ["a cat on a mat", "dog"]
    assert torch.equal(a(text), b(text))
    (ca, la), (cb, lb) = a(text, return_lens=True), b(text, return_lens=True)
    assert torch.equal(ca, cb) and torch.equal(la, lb)
    for x, y in zip(a(["a (cat:1.5) on a mat", "dog"], weighted=True), b(["a (cat:1.5) on a mat", "dog"], weighted=True)):
        assert torch.equal(x, y)
    for x, y in zip(a.phrase_rows(text, ["cat", "dog"]), b.phrase_rows(text, ["cat", "dog"])):
        assert torch.equal(x, y)
    fa, fb = a.fragment_ids([["a ", "cat"], ["dog"]]), b.fragment_ids([["a ", "cat"], ["dog"]])
    assert torch.equal(fa[0], fb[0]) and torch.equal(fa[1], fb[1]) and fa[2:] == fb[2:]
    assert b.use_native(False) is b and not b.native and torch.equal(a(text), b(text))
    # the padding mask reaches the Hugging Face tower as attention_mask= and changes a short prompt's context
    m = T5TextEmbedder(tokenizer=StubTokenizer(), transformer=gated_t5(), encoder_padding_mask=True)
    ids = StubTokenizer()(text)["input_ids"]
    lens = (ids != 0).sum(-1)
    keep = (torch.arange(77)[None, :] < lens[:, None]).long()
    with torch.no_grad():
        want = m.transformer(input_ids=ids, attention_mask=keep).last_hidden_state
    assert torch.equal(m(text), want) and not torch.equal(m(text), a(text))


def test_set_compute_dtype_reaches_the_text_model_and_is_inert_without_native():
    import paintmind_amd as pm
    from paintmind_amd.generate import Pipeline
    emb = T5TextEmbedder(tokenizer=StubTokenizer(), transformer=gated_t5())
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False, text_model=emb)
    before = emb(["a cat"])
    pipe.set_compute_dtype(torch.bfloat16)
    assert emb.compute_dtype == torch.bfloat16 and emb._pm_dtype == torch.bfloat16
    assert torch.equal(emb(["a cat"]), before)
    assert not any(k.endswith("_pm_dtype") for k in pipe.state_dict())
