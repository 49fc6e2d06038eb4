"""The from-mask flag without a GPU: ``Pipeline.generate_ids`` tells the native loop that it starts from the all-mask state
exactly when no start ids were given (include/pmhip.h, PMHIP_GENERATE_FROM_MASK), on every lane; a pipeline that lives on the
CPU never reaches the native call."""
import contextlib

import pytest
import torch

import paintmind_amd as pm
from paintmind_amd import _lib, engine as engine_mod
from paintmind_amd.generate import Pipeline
from util import load_golden, to_torch_sd


class StubEngine:
    """stands in for S2Engine / the VQGAN engine: records what generate() is asked for"""
    device = torch.device("cpu")

    def __init__(self, log):
        self.log = log

    def clone(self):
        return StubEngine(self.log)

    def generate(self, vq_engine, ids, context, temps, nmask, decode_flags, topk, **kw):
        self.log.append(dict(kw, B=ids.shape[0], ids=ids.clone(), engine=self))
        return ids, None


@pytest.fixture()
def stub_pipe(monkeypatch):
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False).eval()
    pipe.load_state_dict(to_torch_sd(p), strict=False)
    log = []
    eng, vq = StubEngine(log), StubEngine(log)
    monkeypatch.setattr(pipe, "engine", lambda: eng)
    monkeypatch.setattr(pipe.vqgan, "engine", lambda: vq)
    monkeypatch.setattr(Pipeline, "_new_lane_stream", staticmethod(lambda device, lane, n_lanes: object()))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: object())
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "stream", lambda stream: contextlib.nullcontext())
    return pipe, log


def test_library_exports_the_flag_and_the_counter():
    lib = _lib.load()
    assert lib.pmhip_abi_version() == _lib.ABI_VERSION
    assert (_lib.GENERATE_GRAPH, _lib.GENERATE_CONCURRENT_LANES, _lib.GENERATE_FROM_MASK) == (1, 2, 4)
    assert "pmhip_s2_step0_shared" in _lib.PROTOTYPES and lib.pmhip_s2_step0_shared is not None
    assert lib.pmhip_s2_step0_shared(None, None, None) == 1 and b"null" in lib.pmhip_last_error()
    hdr = open(__file__.replace("tests/test_step0_cpu.py", "include/pmhip.h")).read()
    assert "#define PMHIP_GENERATE_FROM_MASK 4" in hdr


def test_flag_is_set_iff_no_start_ids_were_given(stub_pipe):
    pipe, log = stub_pipe
    N, mask = pipe.num_tokens, pipe.mask_token_id
    flags = [True, False, True]
    pipe.generate_ids(None, 3, 3, 1.0, 2, flags, seed=1, streams=1)
    assert len(log) == 1 and log[0]["from_mask"] is True and log[0]["B"] == 3
    assert torch.equal(log[0]["ids"], torch.full((3, N), mask, dtype=torch.long))
    # explicit start ids -- even all-mask ones -- keep the full path: the flag is a statement about what the CALLER passed
    del log[:]
    all_mask = torch.full((3, N), mask, dtype=torch.long)
    pipe.generate_ids(None, 3, 3, 1.0, 2, flags, seed=1, streams=1, ids0=all_mask)
    assert len(log) == 1 and log[0]["from_mask"] is False and torch.equal(log[0]["ids"], all_mask)
    del log[:]
    some = all_mask.clone()
    some[:, ::2] = 5
    pipe.generate_ids(None, 3, 3, 1.0, 2, flags, seed=1, streams=1, ids0=some)
    assert log[0]["from_mask"] is False and torch.equal(log[0]["ids"], some)
    # with a context the flag still travels (the native loop then only fills the ids)
    del log[:]
    ctx = torch.zeros(3, 4, 8)
    pipe.generate_ids(ctx, 3, 3, 1.0, 2, flags, seed=1, streams=1, guidance_scale=2.0)
    assert log[0]["from_mask"] is True and log[0]["guidance_scale"] == 2.0


@pytest.mark.parametrize("streams", [2, 3, (4, 2, 1, 2)])
def test_flag_is_set_on_every_lane(stub_pipe, streams):
    pipe, log = stub_pipe
    B = 9
    parts = pipe.generate_ids(None, B, 2, 1.0, 2, [True, True], seed=4, image_base=10, streams=streams, join=False,
                              wait_current=False)
    n_lanes = len(streams) if isinstance(streams, tuple) else streams
    assert len(parts) == n_lanes == len(log)
    assert all(c["from_mask"] is True and c["concurrent_lanes"] is True for c in log)
    assert sum(c["B"] for c in log) == B
    assert [c["image_base"] for c in log] == [10 + sum(c["B"] for c in log[:i]) for i in range(n_lanes)]
    assert len({id(c["engine"]) for c in log}) == n_lanes            # one handle -- and so one step-0 cache -- per lane
    # lanes never start from given ids
    with pytest.raises(ValueError):
        pipe.generate_ids(None, B, 2, 1.0, 2, [True, True], seed=4, streams=2,
                          ids0=torch.full((B, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long))


def test_engine_generate_ors_the_flag_in(monkeypatch):
    """S2Engine.generate: use_graph | concurrent_lanes | from_mask -> bits 1 | 2 | 4 of the native call's use_graph argument"""
    seen = []

    class Lib:
        @staticmethod
        def pmhip_pipeline_generate(*args):
            seen.append(args[14])
            return 0

    e = object.__new__(engine_mod.S2Engine)
    e.__dict__.update(lib=Lib, handle=None, device=torch.device("cpu"), tokens=16, n_embed=64, context_dim=8)
    monkeypatch.setattr(engine_mod, "stream_ptr", lambda device: None)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    ids = torch.zeros(2, 16, dtype=torch.long)
    for graph, lanes, fm in [(False, False, False), (True, False, False), (False, False, True), (True, True, True), (False, True, True)]:
        e.generate(None, ids, None, [1.0, 0.5], [8, 1], [False, False], 2, use_graph=graph, concurrent_lanes=lanes, from_mask=fm)
        assert seen[-1] == (1 if graph else 0) | (2 if lanes else 0) | (4 if fm else 0)
    e.generate(None, ids, None, [1.0], [1], [False], 2)
    assert seen[-1] == 0                                             # the default does not claim the state
    e.handle = None                                                  # (__del__ has nothing to destroy)


def test_cpu_pipeline_never_reaches_the_native_call(monkeypatch):
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False).eval()
    pipe.load_state_dict(to_torch_sd(p), strict=False)
    calls = []
    monkeypatch.setattr(engine_mod.S2Engine, "generate", lambda self, *a, **k: calls.append("generate"))
    monkeypatch.setattr(engine_mod.S2Engine, "__init__", lambda self, *a, **k: calls.append("engine"))
    monkeypatch.setattr(Pipeline, "generate_ids", lambda self, *a, **k: calls.append("generate_ids"))
    imgs, ids = pipe.generate(["a", "b"], timesteps=3, topk=2, save_interval=1, seed=3, return_ids=True)
    assert calls == [] and len(imgs) == 3 and ids.shape == (2, pipe.num_tokens)
    assert imgs[0].device.type == "cpu" and bool((ids != pipe.mask_token_id).any())
