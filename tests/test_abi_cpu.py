"""CPU-side checks of the drop-in boundary: the library loads, exports every declared symbol, and the
host API mirrors the reference's surface.  No compute calls (there is no GPU here)."""
import os
import re

import pytest
import torch

import paintmind_amd as pm
from paintmind_amd import _lib
from util import ROOT, api_facts


def test_header_and_prototypes_agree():
    hdr = open(os.path.join(ROOT, "include", "pmhip.h")).read()
    declared = set(re.findall(r"\b(pmhip_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"pmhip_stream"}
    assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)


def test_library_exports_every_symbol():
    lib = _lib.load()                      # binds every prototype, raises on a missing symbol
    assert lib.pmhip_abi_version() == _lib.ABI_VERSION
    assert lib.pmhip_vq_scratch_bytes(1024, 8192) >= 4 * 1024 * 8


def test_errors_are_reported_not_thrown():
    import ctypes as C
    lib = _lib.load()
    rc = lib.pmhip_gemm(0, None, 64, None, 64, None, None, 0, 0, None, 64, 0, 128, 128, 64, None)
    assert rc == 1 and b"null" in lib.pmhip_last_error()
    rc = lib.pmhip_gemm(0, C.c_void_p(8), 64, C.c_void_p(8), 64, None, None, 0, 0, C.c_void_p(8), 64, 0, 128, 128, 60, None)
    assert rc == 1 and b"multiple of 64" in lib.pmhip_last_error()
    rc = lib.pmhip_timing_get(b"nope", None, None)
    assert rc == 1


def test_undersized_leading_dimensions_are_rejected():
    """A leading dimension smaller than the row it strides over would make rows overlap silently: every entry point that takes one
    answers PMHIP_EINVAL and names the argument.  The checks return before anything is launched, so dummy pointers do."""
    import ctypes as C
    lib = _lib.load()
    p = C.c_void_p(256)
    F32, BF16 = _lib.F32, _lib.BF16

    def rejected(rc, name):
        msg = lib.pmhip_last_error()
        assert rc == _lib.PMHIP_EINVAL and name.encode() in msg and b"smaller" in msg, (rc, msg)

    # check_common: lda / ldw against K, through every entry point that ends there
    rejected(lib.pmhip_gemm(F32, p, 64, p, 128, None, None, 0, 0, p, 128, F32, 128, 128, 128, None), "lda")
    rejected(lib.pmhip_gemm(F32, p, 128, p, 64, None, None, 0, 0, p, 128, F32, 128, 128, 128, None), "ldw")
    rejected(lib.pmhip_gemm_swiglu(BF16, p, 64, p, p, p, 64, 128, 64, 128, None), "lda")
    kinds, outs = (C.c_int * 1)(_lib.PART_Q), (C.c_void_p * 1)(256)
    rejected(lib.pmhip_gemm_heads(BF16, p, 128, p, 64, 128, 128, 2, 128, 128, 1, kinds, outs, 1.0, None), "ldw")
    rejected(lib.pmhip_gemm_hilo(p, 64, p, 128, None, p, p, 128, 0, p, p, 128, 128, 128, 128, None), "lda")
    # the plain GEMM: ldo, and ldr only with a residual
    rejected(lib.pmhip_gemm(F32, p, 128, p, 128, None, None, 0, 0, p, 64, F32, 128, 128, 128, None), "ldo")
    rejected(lib.pmhip_gemm(F32, p, 128, p, 128, None, p, 64, 0, p, 128, F32, 128, 128, 128, None), "ldr")
    rejected(lib.pmhip_gemm_softmax_stats(F32, p, 128, p, 128, None, p, 64, 128, 128, 128, None, p, None), "ldo")
    # the pair producers
    rejected(lib.pmhip_gemm_hilo(p, 128, p, 128, None, p, p, 128, 0, p, p, 64, 128, 128, 128, None), "ldo")
    rejected(lib.pmhip_gemm_hilo(p, 128, p, 128, None, p, p, 64, 0, p, p, 128, 128, 128, 128, None), "ldr")
    rejected(lib.pmhip_gemm_hilo_stats(p, 128, p, 128, None, p, p, 128, 0, p, p, 64, 128, 128, 128, p, None), "ldo")
    rejected(lib.pmhip_gemm_hilo_center(p, 128, p, 128, None, p, p, 64, 0, p, p, 128, 128, 128, 128, None, None, 0.0, None, 0, None),
             "ldr")
    # SwiGLU: ldo against the padded hidden width
    rejected(lib.pmhip_gemm_swiglu(BF16, p, 128, p, p, p, 64, 128, 128, 128, None), "ldo")
    # attention: ldo against heads * dim_head
    rejected(lib.pmhip_attention(BF16, p, p, p, p, 64, 1, 2, 64, 64, 64, 1, None), "ldo")
    rejected(lib.pmhip_attention_dh(BF16, p, p, p, p, 64, 1, 4, 32, 64, 64, 64, 1, None), "ldo")
    rejected(lib.pmhip_attention_dh(BF16, p, p, p, p, 64, 1, 2, 64, 64, 64, 64, 1, None), "ldo")      # forwards to pmhip_attention


def test_hip_operators_have_no_cpu_fallback():
    """The HIP operators never compute on the CPU: a CPU tensor handed to one raises.  (A MODULE that lives on the CPU is a
    different matter: it runs this package's own plain-torch branch, like the reference runs on whatever device the module is
    on -- tests/test_cpu_branch.py.)"""
    from paintmind_amd import ops
    with pytest.raises(_lib.PmhipError):
        ops.layernorm(torch.zeros(4, 64), torch.ones(64), torch.zeros(64))
    with pytest.raises(_lib.PmhipError):
        ops.gemm(torch.zeros(128, 64), torch.zeros(128, 64))
    torch.manual_seed(0)
    m = pm.create_model(arch="vqgan", version="tiny-vqgan", pretrained=False)
    with pytest.raises(_lib.PmhipError):
        m.engine()                                   # the native engine itself is for ROCm devices only


def test_factory_surface():
    with pytest.raises(ValueError) as e:
        pm.create_model(arch="nope", version="vit-s-vqgan", pretrained=False)
    assert str(e.value) == api_facts()["bad_arch_error"]
    cfg = pm.Config(pm.ver2cfg["vit-s-vqgan"])
    assert cfg.enc["dim"] == 512 and cfg.to_dict()["n_embed"] == 8192
    c2 = pm.Config()
    c2.from_dict({"a": 1})
    assert c2.a == 1 and "a" in repr(c2)


def test_seeded_weights_match_reference_checksum():
    """torch.manual_seed(0) + create_model reproduces the reference's random init bit-for-bit (sha256 of the
    state_dict recorded by make_goldens.py from the reference)."""
    import hashlib
    torch.manual_seed(0)
    m = pm.create_model(arch="vqgan", version="vit-s-vqgan", pretrained=False)
    h = hashlib.sha256()
    for k, v in m.state_dict().items():
        h.update(k.encode())
        h.update(v.numpy().tobytes())
    assert h.hexdigest() == api_facts()["full_vqgan_weights_sha256"]
    assert sum(p.numel() for p in m.parameters()) == 52032992


def test_pipeline_wiring_and_schedule():
    from paintmind_amd.generate import Pipeline, num_token_masked, mask_schedule
    torch.manual_seed(0)
    p = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False)
    assert p.num_tokens == 16 and p.mask_token_id == 64 and p.mask_token.shape == (1, 32)
    keys = [k for k in p.state_dict() if not k.startswith("text_model")]
    assert "transformer.layers.layer0.attn2.to_k.weight" in keys and "vqgan.quantize.embedding.weight" in keys
    nm = [num_token_masked(mask_schedule((s + 1) / 8), 1024) for s in range(8)]
    assert nm == api_facts()["mask_counts_T8_N1024"]
    temps, nmask = p._schedule(8, 1.0)
    assert temps[0] == 1.0 and temps[-1] == 0.125 and nmask[-1] == 1
    with pytest.raises(_lib.PmhipError):            # the masked-token objective (forward) is HIP-only: no CPU branch
        p(torch.zeros(1, 3, 32, 32))


def test_packing_roundtrip():
    """interleaved SwiGLU packing: rows [16 x1 | 16 x2] and zero padding to a multiple of 64."""
    from paintmind_amd import packing
    lin = torch.nn.Linear(64, 2 * 88)
    w12p, b12p, hp = packing.pack_w12(lin, torch.float32)
    assert hp == 128 and w12p.shape == (256, 64)
    w = lin.weight.detach()
    assert torch.equal(w12p[0:16], w[0:16]) and torch.equal(w12p[16:32], w[88:104])
    assert torch.equal(w12p[32:48], w[16:32]) and torch.equal(w12p[160 + 16:160 + 24], w[88 + 80:88 + 88])
    assert torch.count_nonzero(w12p[160 + 8:160 + 16]) == 0 and torch.count_nonzero(w12p[192:]) == 0
    assert torch.equal(b12p[16:32], lin.bias.detach()[88:104])


def test_transforms_without_torchvision():
    """stage1/2_transform restated with PIL + torch (reference utils/transform.py:7-34): range, geometry, RNG order"""
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(0)
    img = Image.fromarray(rng.integers(0, 256, (300, 400, 3), dtype=np.uint8))
    x = pm.stage1_transform(is_train=False, scale=0.8)(img)
    assert x.shape == (3, 256, 256) and x.dtype == torch.float32 and -1.0 <= float(x.min()) and float(x.max()) <= 1.0
    # evaluation = bicubic resize to 320 then the central 256 window
    ref = np.asarray(img.resize((320, 320), Image.BICUBIC).crop((32, 32, 288, 288)), dtype=np.float32) / 255
    assert torch.allclose(x, torch.from_numpy(ref).permute(2, 0, 1) * 2 - 1)
    torch.manual_seed(5)
    a = pm.stage1_transform(is_train=True)(img)
    torch.manual_seed(5)
    b = pm.stage1_transform(is_train=True)(img)
    assert torch.equal(a, b)
    torch.manual_seed(5)
    top, left, coin = int(torch.randint(0, 65, (1,))), int(torch.randint(0, 65, (1,))), bool(torch.rand(1) < 0.5)
    crop = img.resize((320, 320), Image.BICUBIC).crop((left, top, left + 256, top + 256))
    if coin:
        crop = crop.transpose(Image.FLIP_LEFT_RIGHT)
    assert torch.allclose(a, torch.from_numpy(np.asarray(crop, dtype=np.float32) / 255).permute(2, 0, 1) * 2 - 1)
    assert pm.stage2_transform(img_size=128, is_train=False)(img).shape == (3, 128, 128)
    from paintmind_amd.reconstruct import restore
    assert restore(x).size == (256, 256)


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under paintmind_amd/ may import, call or link it"""
    import glob
    for path in glob.glob(os.path.join(ROOT, "paintmind_amd", "**", "*"), recursive=True):
        if os.path.isfile(path) and path.endswith((".py", ".hip", ".h", ".sh")):
            text = open(path, errors="ignore").read()
            assert "oracle" not in text.replace("oracle/vq_ref.c", "").replace("the oracle", "").replace("vs the oracle", "") \
                or path.endswith(("vq.hip",)), path
    for path in glob.glob(os.path.join(ROOT, "paintmind_amd", "**", "*.py"), recursive=True):
        src = open(path).read()
        assert "import oracle" not in src and "from oracle" not in src, path


def test_missing_extension_fails_loudly(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", os.path.join(ROOT, "paintmind_amd", "does_not_exist.so"))
    with pytest.raises(_lib.PmhipError) as e:
        _lib.load()
    assert "no CPU fallback" in str(e.value) or "not built" in str(e.value)


def test_product_library_reads_only_the_runtime_switches_the_tests_exercise():
    """Round 6: tuning knobs and the switches of finished A/Bs are compiled into the library as constants (common.h pm_dev_knob;
    the sweep scripts under tools/ use a -DPM_DEV_KNOBS build).  What the shipped library still reads from the environment is this
    list, each of them exercised by a test (PMHIP_HILO / PMHIP_LN_UNFOLD / PMHIP_HILO_CENTER / PMHIP_FOLD_MAX_ROWS:
    tests/test_gpu_model.py and test_gpu_ops.py; AMD_DIRECT_DISPATCH: tests/test_gpu_dist.py) or documented in include/pmhip.h
    (PMHIP_BLOCKING_WAIT, PMHIP_DECODE_OVERLAP_MAX_ROWS)."""
    import re
    import subprocess
    lib = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "paintmind_amd", "libpaintmind_hip.so")
    out = subprocess.run(["strings", "-n", "6", lib], capture_output=True, text=True, timeout=120).stdout
    names = set(re.findall(r"\b(PMHIP_[A-Z0-9_]+|AMD_DIRECT_DISPATCH)\b", out)) - {"PMHIP_H"}
    allowed = {"AMD_DIRECT_DISPATCH", "PMHIP_BLOCKING_WAIT", "PMHIP_DECODE_OVERLAP_MAX_ROWS", "PMHIP_FOLD_MAX_ROWS", "PMHIP_HILO",
               "PMHIP_HILO_CENTER", "PMHIP_LN_UNFOLD"}
    assert names <= allowed, sorted(names - allowed)
