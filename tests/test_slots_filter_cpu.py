"""The sampler filters per request in decode sessions, without a GPU: the rule that says which sampling
kernel serves a slot and which launch writes which row, restated in numpy and tried against planted faults; the host validation of
the new native entries; the surface; and a FilterSession on a CPU pipeline, where a request must equal
``pipe.generate([text], ..., topk=, top_p=, seed=)`` whatever shared the session with it."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import paintmind_amd as pm
from paintmind_amd import _lib
from paintmind_amd.generate import Pipeline
from paintmind_amd.serve import DecodeSession, FilterSession
from util import load_golden, to_torch_sd

# ------------------------------------------------------------------------------------------------------------------------------
# the class rule
# ------------------------------------------------------------------------------------------------------------------------------
T, R, W, N = 0, 1, 2, 3                  # block statistics, row, selection, nucleus: the launches, in their order on the stream


def slot_class(topk, top_p, kt_max=8, k_lanes=64, nucleus=lambda p: p < 1.0):
    """common.h pm_sample_class: a function of (top-k, top_p < 1) only"""
    return N if nucleus(top_p) else T if topk <= kt_max else R if topk <= k_lanes else W


def owners(records, idle_launches=(T,), **rule):
    """records: [(topk, top_p) or None (idle)] -> bool [B, 4]: launch c writes the rows of slot b.  A launch serves the active slots
    of its class; the idle rows belong to the T launch"""
    own = np.zeros((len(records), 4), bool)
    for b, rec in enumerate(records):
        if rec is None:
            own[b, list(idle_launches)] = True
        else:
            own[b, slot_class(*rec, **rule)] = True
    return own


def scalar_kernel(topk, top_p):
    """what pm_sample_rows picks for a batch-scalar call at V % 64 == 0 (sample.hip): the table of DESIGN.md section 4s, written
    out as ranges, not through slot_class"""
    if top_p != 1.0:
        return N
    return [c for c, ks in ((T, range(1, 9)), (R, range(9, 65)), (W, range(65, 16385))) if topk in ks][0]


def check_rule(records, own):
    """every row has exactly one owner; an active slot's is the kernel its own scalar run picks, an idle one's the T launch"""
    assert own.shape == (len(records), 4)
    if not (own.sum(1) == 1).all():
        return False
    for b, rec in enumerate(records):
        if own[b].argmax() != (T if rec is None else scalar_kernel(*rec)):
            return False
    return True


def random_records(rng, B, V):
    recs = []
    for _ in range(B):
        if rng.random() < 0.2:
            recs.append(None)
            continue
        topk = int(rng.choice([1, 7, 8, 9, 10, 63, 64, 65, 66, V - 1, V, int(rng.integers(1, V + 1))]))
        top_p = float(rng.choice([1.0, 1.0, 0.5, 0.999, float(np.nextafter(np.float32(1), np.float32(0)))]))
        recs.append((topk, top_p))
    return recs


def test_every_row_has_exactly_one_owner_and_planted_faults_are_rejected():
    rng = np.random.default_rng(0)
    cases = [random_records(rng, 64, V) for V in (256, 1024, 8192, 16384) for _ in range(8)]
    # the boundaries, a nucleus at every top-k class, and idle slots, all in one batch
    cases.append([(1, 1.0), (8, 1.0), (9, 1.0), (64, 1.0), (65, 1.0), (255, 1.0), (256, 1.0), (3, 0.5), (9, 0.5), (256, 0.999), None])
    for recs in cases:
        assert check_rule(recs, owners(recs))
    faults = {
        "8/9 low": dict(kt_max=7), "8/9 high": dict(kt_max=9),
        "64/65 low": dict(k_lanes=63), "64/65 high": dict(k_lanes=65),
        "top_p == 1 as nucleus": dict(nucleus=lambda p: p <= 1.0),
        "idle rows twice": dict(idle_launches=(T, R)),
        "idle rows never": dict(idle_launches=()),
    }
    for name, rule in faults.items():
        assert not all(check_rule(recs, owners(recs, **rule)) for recs in cases), name
        assert not check_rule(cases[-1], owners(cases[-1], **rule)), name      # the boundary batch alone catches each of them


# ------------------------------------------------------------------------------------------------------------------------------
# the surface
# ------------------------------------------------------------------------------------------------------------------------------
NEW = ("pmhip_sample_rows_slots_filter", "pmhip_pipeline_step_slots_filter", "pmhip_s2_slots_filter_steps")


def test_surface():
    lib = _lib.load()
    header = open(_lib._HERE + "/../include/pmhip.h").read()
    for name in NEW:
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None and f"int {name}(" in header
    P = _lib.PROTOTYPES
    # the operator: pmhip_sample_rows_slots with top_p_dev behind the records; the step: the widest entry with top_p_host in front
    # of the flags
    old = P["pmhip_sample_rows_slots"][1]
    assert P["pmhip_sample_rows_slots_filter"][1] == old[:6] + [_lib.vp] + old[6:]
    old = P["pmhip_pipeline_step_slots_negative"][1]
    assert P["pmhip_pipeline_step_slots_filter"][1] == old[:12] + [C.POINTER(_lib.f32)] + old[12:]
    assert C.sizeof(_lib.Slot) == 32 and _lib.ABI_VERSION == 11 == lib.pmhip_abi_version()
    sig = inspect.signature(FilterSession.submit).parameters
    assert sig["top_p"].default is None and "top_p" not in inspect.signature(DecodeSession.submit).parameters
    assert [k for k in sig if k != "top_p"] == list(inspect.signature(DecodeSession.submit).parameters)
    from paintmind_amd import ops
    from paintmind_amd.engine import S2Engine
    assert inspect.signature(S2Engine.step_slots).parameters["top_p"].default is None
    assert inspect.signature(ops.sample_rows_slots).parameters["top_p"].default is None
    assert inspect.signature(ops.sample_rows_slots).parameters["filters"].default is False
    assert inspect.signature(Pipeline.decode_session).parameters["filters"].default is False


# ------------------------------------------------------------------------------------------------------------------------------
# validation before any launch
# ------------------------------------------------------------------------------------------------------------------------------
N_EMBED = 256


@pytest.fixture(scope="module")
def host_handle():
    """a stage-2 handle: creating one touches no device (the weights are only kept), and the slots entries validate their host
    records before they stage or launch anything"""
    lib = _lib.load()
    tower = _lib.TowerCfg(dim=64, depth=1, heads=1, hidden_pad=64, dim_head=64)
    cfg = _lib.S2Cfg(tokens=16, embed_dim=32, n_embed=N_EMBED, context_dim=64, context_dim_pad=64, tower=tower)
    layers = (_lib.LayerWeights * 1)()
    w = _lib.S2Weights(layers=layers)
    h = C.c_void_p()
    assert lib.pmhip_s2_create(C.byref(h), 0, _lib.F32, C.byref(cfg), C.byref(w)) == _lib.PMHIP_OK
    yield h
    lib.pmhip_s2_destroy(h)


def _records(*recs):
    arr = (_lib.Slot * len(recs))()
    for i, r in enumerate(recs):
        if r is None:
            arr[i].step = _lib.SLOT_IDLE
        else:
            arr[i] = _lib.Slot(*r)
    return arr


def test_the_step_validates_topk_and_top_p_on_the_host_and_names_the_slot(host_handle):
    lib = _lib.load()
    p = C.c_void_p(256)                      # a call that got past the checks would fault: every one of these is refused before
    good = (1, 0, 1.0, 3, 4, 0)

    def step(records, top_p=None, handle=host_handle):
        tp = None if top_p is None else (C.c_float * len(top_p))(*top_p)
        return lib.pmhip_pipeline_step_slots_filter(handle, p, None, 0, len(records), None, records, None, None, None, 0, None, tp, 0, None,
                                                    None, None)

    for topk in (0, -1, N_EMBED + 1):
        assert step(_records(good, good, (1, 0, 1.0, topk, 4, 0))) == _lib.PMHIP_EINVAL
        msg = lib.pmhip_last_error().decode()
        assert "pipeline_step_slots_filter" in msg and "slot 2" in msg and f"topk={topk}" in msg and f"n_embed={N_EMBED}" in msg, msg
    for bad in (0.0, 1.5, float("nan"), float("inf"), -0.5):
        assert step(_records(good, (1, 0, 1.0, N_EMBED, 4, 0), good), [1.0, bad, 0.5]) == _lib.PMHIP_EINVAL
        msg = lib.pmhip_last_error().decode()
        assert "pipeline_step_slots_filter" in msg and "slot 1" in msg and "top_p" in msg and "(0, 1]" in msg, msg
    # num_mask stays checked, and the handle and the records are asked for first
    assert step(_records(good, (1, 0, 1.0, 200, 0, 0))) == _lib.PMHIP_EINVAL and b"num_mask" in lib.pmhip_last_error()
    assert step(_records(good), handle=None) == _lib.PMHIP_EINVAL and b"bad arguments" in lib.pmhip_last_error()
    tiles, chain = C.c_int(-1), C.c_int(-1)
    assert lib.pmhip_s2_slots_filter_steps(host_handle, C.byref(tiles), C.byref(chain)) == _lib.PMHIP_OK
    assert (tiles.value, chain.value) == (0, 0)                          # nothing of the refused calls was counted
    assert lib.pmhip_s2_slots_filter_steps(None, None, None) == _lib.PMHIP_EINVAL
    # the entries without filters keep their range on the same handle
    rc = lib.pmhip_pipeline_step_slots(host_handle, p, None, 0, 2, _records(good, (1, 0, 1.0, 9, 4, 0)), 0, None, None, None)
    assert rc == _lib.PMHIP_EINVAL and b"[1, 8]" in lib.pmhip_last_error()


def test_the_operator_entry_keeps_the_shape_rules_of_the_slots_sampler():
    lib = _lib.load()
    p = C.c_void_p(64)
    call = lib.pmhip_sample_rows_slots_filter
    assert call(p, 64, None, p, 64, None, None, 16, p, p, p, 32, 64, None) == 1 and b"null" in lib.pmhip_last_error()
    assert call(p, 96, None, p, 96, p, None, 16, p, p, p, 32, 96, None) == 1 and b"multiple of 64" in lib.pmhip_last_error()
    assert call(p, 64, None, p, 64, p, p, 16, p, p, p, 40, 64, None) == 1 and b"whole number of images" in lib.pmhip_last_error()
    assert call(p, 32, None, p, 64, p, p, 16, p, p, p, 32, 64, None) == 1 and b"bad shape" in lib.pmhip_last_error()
    assert call(p, 16448, None, p, 64, p, p, 16, p, p, p, 32, 16448, None) == 1 and b"at most 16384" in lib.pmhip_last_error()


# ------------------------------------------------------------------------------------------------------------------------------
# a FilterSession on a CPU pipeline
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_cpu_pipe():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False).eval()
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not [k for k in missing.missing_keys if not k.startswith("text_model")]
    return pipe


# (text, T, temperature, topk, top_p, seed): all different; n_embed = 64
REQUESTS = [("a", 3, 1.0, 3, None, 11), ("b", 5, 0.7, None, None, 22), ("c", 4, 1.3, 40, 0.5, 33), ("d", 2, 0.9, None, 0.9, 44)]


def test_cpu_filter_session_requests_equal_generate_alone(tiny_cpu_pipe):
    pipe = tiny_cpu_pipe
    s = pipe.decode_session(slots=2, conditional=True, filters=True)
    assert type(s) is FilterSession
    handles = [s.submit(text=tx, timesteps=Ts, temperature=temp, topk=k, top_p=p, seed=seed) for tx, Ts, temp, k, p, seed in REQUESTS]
    assert [(h.topk, h.top_p) for h in handles] == [(3, 1.0), (64, 1.0), (40, 0.5), (64, 0.9)]
    done = s.drain()
    assert [(h.slot, h.admitted) for h in handles] == [(0, 0), (1, 0), (0, 3), (1, 5)]      # staggered into the two slots
    assert sorted(f.handle.number for f in done) == [0, 1, 2, 3]
    for f in done:
        tx, Ts, temp, k, p, seed = REQUESTS[f.handle.number]
        imgs, ids = pipe.generate([tx], timesteps=Ts, temperature=temp, topk=k, top_p=p, save_interval=1, seed=seed, return_ids=True)
        assert torch.equal(f.ids, ids[0]), f.handle
        assert torch.equal(f.image, imgs[-1][0]), f.handle
    # the filters did something: the nucleus request differs from its twin without one
    tx, Ts, temp, k, p, seed = REQUESTS[2]
    _, twin = pipe.generate([tx], timesteps=Ts, temperature=temp, topk=k, save_interval=1, seed=seed, return_ids=True)
    assert not torch.equal(next(f for f in done if f.handle.number == 2).ids, twin[0])


def test_submit_checks_the_filters_and_the_default_session_is_the_one_it_was(tiny_cpu_pipe):
    pipe = tiny_cpu_pipe
    plain = pipe.decode_session(slots=2, conditional=False)
    assert type(plain) is DecodeSession and type(pipe.decode_session(slots=2, conditional=False, filters=False)) is DecodeSession
    with pytest.raises(TypeError):
        plain.submit(timesteps=2, top_p=0.5)
    s = pipe.decode_session(slots=2, conditional=False, filters=True)
    for bad in (0, -3, 65):
        with pytest.raises(ValueError, match="topk"):
            s.submit(timesteps=2, topk=bad)
    for bad in (0.0, 1.5, float("nan"), float("inf"), -1):
        with pytest.raises(ValueError, match="top_p"):
            s.submit(timesteps=2, top_p=bad)
    assert not s.queue                                                    # nothing of it was queued
    h = s.submit(timesteps=2, topk=None, top_p=1.0, seed=3)
    assert (h.topk, h.top_p) == (64, 1.0)
