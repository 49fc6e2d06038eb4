"""Decode sessions without a GPU: the ABI-11 surface of the library, and paintmind_amd/serve.py on a CPU pipeline, where a
request must equal ``pipe.generate([text], ..., seed=seed)`` at B = 1 whatever shared the session with it."""
import ctypes as C

import numpy as np
import pytest
import torch

import paintmind_amd as pm
from paintmind_amd import _lib
from paintmind_amd.generate import Pipeline
from util import load_golden, to_torch_sd


def test_abi_11_exports_the_slot_entry_points():
    lib = _lib.load()
    assert lib.pmhip_abi_version() == 11 == _lib.ABI_VERSION
    for name in ("pmhip_sample_rows_slots", "pmhip_remask_slots", "pmhip_pipeline_step_slots"):
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None
    assert C.sizeof(_lib.Slot) == 32
    assert [(_lib.Slot.seed.offset, _lib.Slot.image_index.offset, _lib.Slot.temperature.offset, _lib.Slot.topk.offset,
             _lib.Slot.num_mask.offset, _lib.Slot.step.offset)] == [(0, 8, 16, 20, 24, 28)]


def test_null_slots_are_reported_not_thrown():
    lib = _lib.load()
    p = C.c_void_p(64)
    rc = lib.pmhip_sample_rows_slots(p, 64, None, p, 64, None, 16, p, p, p, 32, 64, None)
    assert rc == 1 and b"null" in lib.pmhip_last_error()
    rc = lib.pmhip_remask_slots(p, p, None, 64, 2, 16, None)
    assert rc == 1 and b"null" in lib.pmhip_last_error()
    rc = lib.pmhip_pipeline_step_slots(p, p, None, 0, 2, None, 0, None, None, None)
    assert rc == 1 and b"slots" in lib.pmhip_last_error()
    # shapes the slots sampler does not serve are refused at the host, before anything is launched
    rc = lib.pmhip_sample_rows_slots(p, 96, None, p, 96, p, 16, p, p, p, 32, 96, None)
    assert rc == 1 and b"multiple of 64" in lib.pmhip_last_error()
    rc = lib.pmhip_sample_rows_slots(p, 64, None, p, 64, p, 16, p, p, p, 40, 64, None)
    assert rc == 1 and b"whole number of images" in lib.pmhip_last_error()


def test_pack_slots_layout():
    from paintmind_amd import ops
    t = ops.pack_slots([(0x1122334455667788, 2 ** 40 + 3, 0.5, 7, 12, 9), None])
    assert t.shape == (2, 32) and t.dtype == torch.uint8
    rec = np.frombuffer(t.numpy().tobytes(), dtype=np.dtype([("seed", "<u8"), ("idx", "<u8"), ("temp", "<f4"), ("topk", "<i4"),
                                                              ("nm", "<i4"), ("step", "<u4")]))
    assert rec[0].tolist() == (0x1122334455667788, 2 ** 40 + 3, 0.5, 7, 12, 9)
    assert rec[1]["step"] == 0x80000000


@pytest.fixture(scope="module")
def tiny_cpu_pipe():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False).eval()
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not [k for k in missing.missing_keys if not k.startswith("text_model")]
    return pipe


# (text, T, temperature, topk, seed): all different
REQUESTS = [("a", 3, 1.0, 5, 11), ("b", 6, 0.7, 3, 22), ("c", 4, 1.3, 1, 33), ("d", 3, 0.9, 8, 44), ("e", 6, 0.0, 2, 55)]


@pytest.fixture(scope="module")
def cpu_session_run(tiny_cpu_pipe):
    s = tiny_cpu_pipe.decode_session(slots=2, conditional=True)
    handles = [s.submit(text=tx, timesteps=T, temperature=temp, topk=k, seed=seed) for tx, T, temp, k, seed in REQUESTS]
    assert len(s.queue) == 5 and s.active == 0
    done = s.drain()
    return s, handles, done


def test_cpu_session_requests_equal_generate_alone(tiny_cpu_pipe, cpu_session_run):
    s, handles, done = cpu_session_run
    assert sorted(f.handle.number for f in done) == [0, 1, 2, 3, 4]
    for f in done:
        tx, T, temp, k, seed = REQUESTS[f.handle.number]
        imgs, ids = tiny_cpu_pipe.generate([tx], timesteps=T, temperature=temp, topk=k, save_interval=1, seed=seed, return_ids=True)
        assert len(imgs) == T
        assert torch.equal(f.ids, ids[0]), f.handle
        assert torch.equal(f.image, imgs[-1][0]), f.handle
        assert f.image.shape == (3, 32, 32)


def test_cpu_session_admission_is_fifo_into_the_lowest_free_slot(cpu_session_run):
    s, handles, done = cpu_session_run
    # two slots; T = 3, 6, 4, 3, 6.  tick 0: #0 -> slot 0, #1 -> slot 1.  #0 retires at tick 2, so #2 enters slot 0 at tick 3 and
    # retires at 6; #1 retires at tick 5, so #3 enters slot 1 at tick 6 and retires at 8; #4 enters slot 0 at tick 7, retires at 12
    assert [(h.slot, h.admitted, h.retired) for h in handles] == [(0, 0, 2), (1, 0, 5), (0, 3, 6), (1, 6, 8), (0, 7, 12)]
    for h in handles:
        assert h.retired == h.admitted + h.timesteps - 1 and h.done == h.timesteps
    assert [f.handle.number for f in done] == [0, 1, 2, 3, 4]
    assert s.tick == 13


def test_cpu_session_schedules_are_the_pipelines(tiny_cpu_pipe, cpu_session_run):
    _, handles, _ = cpu_session_run
    for h, (tx, T, temp, k, seed) in zip(handles, REQUESTS):
        assert (h.temps, h.nmask) == tiny_cpu_pipe._schedule(T, temp)
        assert (h.timesteps, h.temperature, h.topk, h.seed) == (T, temp, k, seed)
    assert [h.image_index for h in handles] == [0, 1, 2, 3, 4]          # image_index=None: a running counter


def test_cpu_session_drain_leaves_every_slot_idle(tiny_cpu_pipe, cpu_session_run):
    s, _, _ = cpu_session_run
    assert s.idle() and s.active == 0 and all(r is None for r in s.occupied) and not s.queue
    assert s.step() == [] and s.drain() == []
    # a request that arrives later is served by the same session, and an unconditional session takes no context
    h = s.submit(text="late", timesteps=2, temperature=1.0, topk=4, seed=9)
    out = s.drain()
    assert [f.handle for f in out] == [h] and h.slot == 0 and s.idle()
    u = tiny_cpu_pipe.decode_session(slots=1, conditional=False)
    with pytest.raises(ValueError):
        u.submit(context=torch.zeros(77, 32))
    with pytest.raises(ValueError):
        tiny_cpu_pipe.decode_session(slots=1, conditional=True).submit(timesteps=3)      # no text, no context


def test_start_ids_are_a_contiguous_copy_and_shape_checked(tiny_cpu_pipe):
    pipe = tiny_cpu_pipe
    N = pipe.num_tokens
    wide = torch.arange(2 * 2 * N, dtype=torch.long).reshape(2, 2 * N) % 65
    view = wide[:, ::2]                                                   # [2, N], strides (2N, 2)
    assert not view.is_contiguous()
    got, want = pipe._start_ids(2, view, "cpu"), pipe._start_ids(2, view.contiguous(), "cpu")
    assert got.is_contiguous() and got.stride() == (N, 1) and torch.equal(got, want) and torch.equal(got, view)
    assert got.data_ptr() != wide.data_ptr()
    assert torch.equal(pipe._start_ids(3, None, "cpu"), torch.full((3, N), pipe.mask_token_id))
    for bad in (torch.zeros(2, N + 1, dtype=torch.long), torch.zeros(1, N, dtype=torch.long), torch.zeros(2 * N, dtype=torch.long)):
        with pytest.raises(ValueError):
            pipe._start_ids(2, bad, "cpu")
        with pytest.raises(ValueError):                                   # checked before any engine is asked for
            pipe.generate_ids(None, 2, 4, 1.0, 3, [False] * 4, 0, ids0=bad)
    # a session hands a request's start ids to the same path: the strided row gives what its contiguous copy gives
    outs = []
    for ids0 in (view[0], view[0].contiguous()):
        s = pipe.decode_session(slots=1, conditional=False)
        s.submit(timesteps=3, temperature=0.8, topk=3, seed=4, ids0=ids0)
        outs.append(s.drain()[0])
    assert torch.equal(outs[0].ids, outs[1].ids) and torch.equal(outs[0].image, outs[1].image)
