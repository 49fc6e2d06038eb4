"""Per-request guidance in decode sessions, without a GPU: the additive surface of the library (three entries and one 8-byte
record beside pmhip_slot; the ABI version stays 11), and paintmind_amd/serve.py on a CPU pipeline, where a guided request must
equal ``pipe.generate([text], ..., seed=seed, guidance_scale=s)`` at B = 1 whatever shared the session with it."""
import ctypes as C

import numpy as np
import pytest
import torch

import paintmind_amd as pm
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline
from util import load_golden, to_torch_sd


def test_guided_slot_entries_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.pmhip_abi_version() == 11 == _lib.ABI_VERSION
    for name in ("pmhip_guidance_combine_slots", "pmhip_pipeline_step_slots_guided", "pmhip_s2_slots_steps"):
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None
    assert C.sizeof(_lib.SlotGuide) == 8
    assert (_lib.SlotGuide.scale.offset, _lib.SlotGuide.on.offset) == (0, 4)
    assert C.sizeof(_lib.Slot) == 32                                       # the record beside it did not change


def test_pack_slot_guides_layout():
    t = ops.pack_slot_guides([2.5, None])
    assert t.shape == (2, 8) and t.dtype == torch.uint8
    rec = np.frombuffer(t.numpy().tobytes(), dtype=np.dtype([("scale", "<f4"), ("on", "<u4")]))
    assert rec[0].tolist() == (2.5, 1) and rec[1].tolist() == (0.0, 0)
    assert t.numpy().tobytes() == np.float32(2.5).tobytes() + (1).to_bytes(4, "little") + bytes(8)
    # scale 0 is a guided request (it samples from the unconditional logits), not an unguided one
    assert np.frombuffer(ops.pack_slot_guides([0.0]).numpy().tobytes(), dtype="<u4").tolist() == [0, 1]


def test_null_pointers_and_bad_shapes_are_reported_not_thrown():
    lib = _lib.load()
    p = C.c_void_p(64)
    # (cond, uncond, guides, slots, tokens, out, block_stats, M, V, stream)
    for args, word in (((p, p, None, p, 16, p, None, 32, 64, None), b"guides"),
                       ((p, p, p, None, 16, p, None, 32, 64, None), b"slots"),
                       ((p, p, p, p, 16, None, None, 32, 64, None), b"out"),
                       ((None, p, p, p, 16, p, None, 32, 64, None), b"cond")):
        rc = lib.pmhip_guidance_combine_slots(*args)
        msg = lib.pmhip_last_error()
        assert rc == 1 and b"null" in msg and word in msg, msg
    # shapes the kernel does not serve are refused at the host, before anything is launched
    rc = lib.pmhip_guidance_combine_slots(p, p, p, p, 16, p, None, 32, 96, None)
    assert rc == 1 and b"multiple of 64" in lib.pmhip_last_error()
    rc = lib.pmhip_guidance_combine_slots(p, p, p, p, 16, p, None, 40, 64, None)
    assert rc == 1 and b"whole number of images" in lib.pmhip_last_error()
    rc = lib.pmhip_pipeline_step_slots_guided(p, p, None, 0, 2, None, None, 0, None, None, None)
    assert rc == 1 and b"slots" in lib.pmhip_last_error()
    rc = lib.pmhip_s2_slots_steps(None, None, None)
    assert rc == 1 and b"null" in lib.pmhip_last_error()


@pytest.fixture(scope="module")
def tiny_cpu_pipe():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False).eval()
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not [k for k in missing.missing_keys if not k.startswith("text_model")]
    return pipe


# (text, T, temperature, topk, seed, guidance scale)
REQUESTS = [("a", 3, 1.0, 5, 11, None), ("b", 4, 0.7, 3, 22, 2.5), ("c", 3, 1.3, 1, 33, 0.0), ("d", 5, 0.9, 8, 44, 4.0)]


def test_cpu_session_guided_requests_equal_generate_alone(tiny_cpu_pipe):
    pipe = tiny_cpu_pipe
    s = pipe.decode_session(slots=2, conditional=True)
    handles = [s.submit(text=tx, timesteps=T, temperature=temp, topk=k, seed=seed, guidance_scale=g) for tx, T, temp, k, seed, g in REQUESTS]
    assert [h.guidance_scale for h in handles] == [None, 2.5, 0.0, 4.0]
    done = s.drain()
    assert sorted(f.handle.number for f in done) == [0, 1, 2, 3]
    for f in done:
        tx, T, temp, k, seed, g = REQUESTS[f.handle.number]
        imgs, ids = pipe.generate([tx], timesteps=T, temperature=temp, topk=k, save_interval=1, seed=seed, guidance_scale=g, return_ids=True)
        assert len(imgs) == T
        assert torch.equal(f.ids, ids[0]), f.handle
        assert torch.equal(f.image, imgs[-1][0]), f.handle
        if g is not None:                                                  # guidance did something: the unguided twin differs
            imgs_u, ids_u = pipe.generate([tx], timesteps=T, temperature=temp, topk=k, save_interval=1, seed=seed, return_ids=True)
            assert not torch.equal(f.ids, ids_u[0]) and not torch.equal(f.image, imgs_u[-1][0]), f.handle


def test_an_unconditional_session_refuses_guidance(tiny_cpu_pipe):
    u = tiny_cpu_pipe.decode_session(slots=1, conditional=False)
    with pytest.raises(ValueError):
        u.submit(timesteps=3, guidance_scale=2.0)
    assert not u.queue
    with pytest.raises(ValueError):
        tiny_cpu_pipe.decode_session(slots=1, conditional=True).submit(text="a", timesteps=3, guidance_scale=float("nan"))
