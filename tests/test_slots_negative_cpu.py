"""A negative prompt and a guidance schedule per request in decode sessions, without a GPU: the additive surface of the library
(three entries and one flag; the two records and the ABI version stay), submit-time validation, and paintmind_amd/serve.py on a CPU
pipeline, where such a request must equal ``pipe.generate([text], negative_text=..., guidance_scale=[...], seed=seed)`` at B = 1
whatever shared the session with it."""
import ctypes as C

import numpy as np
import pytest
import torch

import paintmind_amd as pm
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline
from util import load_golden, to_torch_sd


def test_negative_slot_entries_are_exported_and_records_and_abi_version_stay():
    lib = _lib.load()
    assert lib.pmhip_abi_version() == 11 == _lib.ABI_VERSION
    for name in ("pmhip_guidance_combine_slots_which", "pmhip_pipeline_step_slots_negative", "pmhip_s2_slots_passes"):
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None
    assert len(_lib.PROTOTYPES["pmhip_pipeline_step_slots_negative"][1]) == 16
    assert len(_lib.PROTOTYPES["pmhip_guidance_combine_slots_which"][1]) == len(_lib.PROTOTYPES["pmhip_guidance_combine_slots"][1]) + 1
    assert C.sizeof(_lib.Slot) == 32 and C.sizeof(_lib.SlotGuide) == 8
    assert (_lib.SlotGuide.scale.offset, _lib.SlotGuide.on.offset) == (0, 4)
    assert (_lib.SLOTS_GRAPH, _lib.SLOTS_KEEP_CONTEXT, _lib.SLOTS_KEEP_NEGATIVE) == (1, 2, 4)
    assert (_lib.GUIDE_OFF, _lib.GUIDE_UNCOND, _lib.GUIDE_NEGATIVE) == (0, 1, 2)


def test_pack_slot_guides_takes_a_kind_per_image():
    t = ops.pack_slot_guides([2.5, None, 0.0, -1.0], kinds=[2, 2, 1, 2])
    rec = np.frombuffer(t.numpy().tobytes(), dtype=np.dtype([("scale", "<f4"), ("on", "<u4")]))
    assert [r.tolist() for r in rec] == [(2.5, 2), (0.0, 0), (0.0, 1), (-1.0, 2)]          # an unguided image stays on = 0
    assert torch.equal(ops.pack_slot_guides([2.5, None]), ops.pack_slot_guides([2.5, None], kinds=[1, 1]))
    with pytest.raises(ValueError):
        ops.pack_slot_guides([2.5, None], kinds=[1])


def test_null_pointers_and_bad_arguments_are_reported_not_thrown():
    lib = _lib.load()
    p = C.c_void_p(64)
    # (cond, other, guides, slots, which, tokens, out, block_stats, M, V, stream)
    for args, word in (((p, p, None, p, 1, 16, p, None, 32, 64, None), b"guides"),
                       ((p, p, p, None, 2, 16, p, None, 32, 64, None), b"slots"),
                       ((p, p, p, p, 1, 16, None, None, 32, 64, None), b"out"),
                       ((None, p, p, p, 2, 16, p, None, 32, 64, None), b"cond")):
        rc = lib.pmhip_guidance_combine_slots_which(*args)
        msg = lib.pmhip_last_error()
        assert rc == 1 and b"null" in msg and word in msg, msg
    for which in (0, 3, -1):
        rc = lib.pmhip_guidance_combine_slots_which(p, p, p, p, which, 16, p, None, 32, 64, None)
        assert rc == 1 and b"which" in lib.pmhip_last_error()
    rc = lib.pmhip_guidance_combine_slots_which(p, p, p, p, 1, 16, p, None, 32, 96, None)
    assert rc == 1 and b"multiple of 64" in lib.pmhip_last_error()
    rc = lib.pmhip_pipeline_step_slots_negative(p, p, None, 0, 2, None, None, None, None, None, 0, None, 0, None, None, None)
    assert rc == 1 and b"slots" in lib.pmhip_last_error()
    rc = lib.pmhip_s2_slots_passes(None, None, None, None)
    assert rc == 1 and b"null" in lib.pmhip_last_error()


@pytest.fixture(scope="module")
def tiny_cpu_pipe():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False).eval()
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not [k for k in missing.missing_keys if not k.startswith("text_model")]
    return pipe


def test_submit_validates_negative_prompts_and_schedules(tiny_cpu_pipe):
    pipe = tiny_cpu_pipe
    s = pipe.decode_session(slots=2, conditional=True, max_negative_len=3)
    D = pipe.text_model(["a"]).shape[2]
    with pytest.raises(ValueError, match="guidance_scale"):                # a negative prompt without a scale
        s.submit(text="a", timesteps=3, negative_text="not a")
    with pytest.raises(ValueError, match="guidance_scale"):
        s.submit(text="a", timesteps=3, negative_context=torch.zeros(2, D))
    with pytest.raises(ValueError, match="3 steps"):                       # a schedule of the wrong length
        s.submit(text="a", timesteps=3, guidance_scale=[1.0, 2.0])
    with pytest.raises(ValueError, match="3 steps"):
        s.submit(text="a", timesteps=3, guidance_scale=torch.tensor([1.0, 2.0, 3.0, 4.0]))
    for bad in (float("nan"), float("inf")):                               # ... or with a value that is not finite
        with pytest.raises(ValueError, match="finite"):
            s.submit(text="a", timesteps=3, guidance_scale=[1.0, bad, 2.0])
    with pytest.raises(ValueError, match="max_negative_len=3"):            # a negative longer than the session's capacity
        s.submit(text="a", timesteps=3, guidance_scale=2.0, negative_context=torch.zeros(4, D))
    with pytest.raises(ValueError):                                        # not [Ln, D]
        s.submit(text="a", timesteps=3, guidance_scale=2.0, negative_context=torch.zeros(1, 2, D))
    with pytest.raises(ValueError, match="width"):
        s.submit(text="a", timesteps=3, guidance_scale=2.0, negative_context=torch.zeros(2, D + 1))
    assert not s.queue                                                     # nothing of it was queued
    h = s.submit(text="a", timesteps=3, guidance_scale=(1.0, 2.0, 3.0), negative_context=torch.zeros(3, D))
    assert h.guidance_scale == (1.0, 2.0, 3.0) and h.scales == [1.0, 2.0, 3.0] and tuple(h.negative.shape) == (3, D)
    with pytest.raises(ValueError):
        pipe.decode_session(slots=1, max_negative_len=0)
    u = pipe.decode_session(slots=1, conditional=False)                    # an unconditional session has nothing to move away from
    for kw in (dict(negative_text="not a", guidance_scale=2.0), dict(negative_context=torch.zeros(2, D)), dict(guidance_scale=[1.0, 2.0, 3.0])):
        with pytest.raises(ValueError):
            u.submit(timesteps=3, **kw)
    assert not u.queue


# (text, T, temperature, topk, seed, guidance scale or schedule, negative text)
REQUESTS = [("a", 3, 1.0, 5, 11, None, None),
            ("b", 4, 0.7, 3, 22, [0.5, 1.5, 2.5, 3.5], "not b"),
            ("c", 3, 1.3, 1, 33, 2.0, "not c at all"),
            ("d", 5, 0.9, 8, 44, [4.0, 0.0, -1.0, 2.0, 2.0], None),
            ("e", 2, 1.0, 4, 55, 3.0, None)]


def test_cpu_session_requests_with_negative_text_and_schedule_equal_generate_alone(tiny_cpu_pipe):
    pipe = tiny_cpu_pipe
    s = pipe.decode_session(slots=2, conditional=True)
    handles = [s.submit(text=tx, timesteps=T, temperature=temp, topk=k, seed=seed, guidance_scale=g, negative_text=neg)
               for tx, T, temp, k, seed, g, neg in REQUESTS]
    assert [h.guidance_scale for h in handles] == [r[5] for r in REQUESTS]           # Request keeps what was passed
    done = s.drain()
    assert sorted(f.handle.number for f in done) == list(range(len(REQUESTS)))
    for f in done:
        tx, T, temp, k, seed, g, neg = REQUESTS[f.handle.number]
        kw = dict(timesteps=T, temperature=temp, topk=k, save_interval=1, seed=seed, return_ids=True)
        imgs, ids = pipe.generate([tx], guidance_scale=g, negative_text=neg, **kw)
        assert len(imgs) == T
        assert torch.equal(f.ids, ids[0]), f.handle
        assert torch.equal(f.image, imgs[-1][0]), f.handle
        if neg is not None:                                                # the negative prompt did something: the twin without it differs
            _, ids_u = pipe.generate([tx], guidance_scale=g, **kw)
            assert not torch.equal(f.ids, ids_u[0]), f.handle


def test_cpu_session_negative_context_with_its_own_length(tiny_cpu_pipe):
    """negative_context [Ln_r, D] instead of a text: the request attends to exactly these rows"""
    pipe = tiny_cpu_pipe
    ctx = pipe.text_model(["a"])
    neg = torch.randn(1, 2, ctx.shape[2], generator=torch.Generator().manual_seed(3))
    s = pipe.decode_session(slots=1, conditional=True, max_negative_len=4)
    h = s.submit(context=ctx[0], timesteps=3, topk=3, seed=7, guidance_scale=2.0, negative_context=neg[0])
    (f,) = s.drain()
    assert f.handle is h
    opts = pipe._options(3, None, 2.0, None, None, ctx, 1, neg, None, 3)   # the CPU loop of generate, on context tensors
    imgs, ids = pipe._generate_cpu(ctx, 1, 3, 1.0, opts, 1, 7, True)
    assert torch.equal(f.ids, ids[0]) and torch.equal(f.image, imgs[-1][0])
    opts = pipe._options(3, None, 2.0, None, None, ctx, 1, None, None, 3)
    assert not torch.equal(f.ids, pipe._generate_cpu(ctx, 1, 3, 1.0, opts, 1, 7, True)[1][0])
