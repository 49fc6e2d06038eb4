"""The from-mask flag without a GPU: ``Pipeline.generate_ids`` tells the native loop that it starts from the all-mask state
exactly when no start ids were given (include/pmhip.h, PMHIP_GENERATE_FROM_MASK), on every lane; a pipeline that lives on the
CPU never reaches the native call."""
import contextlib
import itertools
import types

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


def stub_engine(lib, monkeypatch):
    """an S2Engine over `lib` instead of the native library: no handle, no device"""
    e = object.__new__(engine_mod.S2Engine)
    e.__dict__.update(lib=lib, handle=None, device=torch.device("cpu"), tokens=16, n_embed=64, context_dim=8)
    monkeypatch.setattr(engine_mod, "stream_ptr", lambda device: None)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    return e


def test_engine_generate_ors_the_flag_in(monkeypatch):
    """S2Engine.generate: use_graph | concurrent_lanes | from_mask -> bits 1 | 2 | 4 of the native call's use_graph argument"""
    seen = []

    class Lib:
        @staticmethod
        def pmhip_pipeline_generate_nucleus(*args):
            seen.append(args[15])                                    # use_graph: one place behind pmhip_pipeline_generate's, after ctx_lens_host
            return 0

    e = stub_engine(Lib, monkeypatch)
    ids = torch.zeros(2, 16, dtype=torch.long)
    for graph, lanes, fm in [(False, False, False), (True, False, False), (False, False, True), (True, True, True), (False, True, True)]:
        e.generate(None, ids, None, [1.0, 0.5], [8, 1], [False, False], 2, use_graph=graph, concurrent_lanes=lanes, from_mask=fm)
        assert seen[-1] == (1 if graph else 0) | (2 if lanes else 0) | (4 if fm else 0)
    e.generate(None, ids, None, [1.0], [1], [False], 2)
    assert seen[-1] == 0                                             # the default does not claim the state
    e.handle = None                                                  # (__del__ has nothing to destroy)


def test_engine_methods_make_one_call_to_the_widest_entry(monkeypatch):
    """S2Engine.sample / generate / step_slots: ONE native call each, to the family's widest entry (include/pmhip.h), whatever
    options came: an absent option arrives as the value with which the header promises the narrower entry's computation (NULL
    lengths, guided = 0, choice 0 with a NULL pointer, top_p = 1, NULL guides), a present one at the header's argument position"""
    calls = []

    class Lib:
        def __getattr__(self, name):
            def entry(*args):
                calls.append((name, args))
                return 0
            return entry

    def only_call(name, n_args):
        assert len(calls) == 1 and calls[0][0] == name and len(calls[0][1]) == n_args, [c[0] for c in calls]
        return calls.pop()[1]

    def null(arg):                                                   # None, or a ctypes NULL pointer
        return getattr(arg, "value", arg) is None

    e = stub_engine(Lib(), monkeypatch)
    B, N, L = 2, 16, 3
    ids, ctx = torch.zeros(B, N, dtype=torch.long), torch.zeros(B, L, 8)
    # step_slots wants ids on the device: what it reads of them, without one
    dev_ids = types.SimpleNamespace(shape=(B, N), is_cuda=True, dtype=torch.int64, is_contiguous=lambda: True, data_ptr=lambda: 4096)
    noise = torch.rand(B, N)
    for lens, scale, choice, top_p in itertools.product((None, [2, 1]), (None, 2.5), (0.0, 4.5), (None, 1.0, 0.5)):
        case = (lens, scale, choice, top_p)
        e.sample(None, ids, ctx, 5, 0.7, 4, seed=9, step=3, image_base=11, want_img=False, guidance_scale=scale, context_lens=lens,
                 choice_temperature=choice, choice_noise=noise, top_p=top_p)
        a = only_call("pmhip_pipeline_sample_nucleus", 23)
        assert (a[4], a[5], a[7], a[9], a[11], a[12], a[13]) == (L, B, 5, 4, 9, 3, 11) and abs(a[8] - 0.7) < 1e-12, case
        assert (null(a[6]) if lens is None else list(a[6]) == lens), case
        assert (a[17], a[18]) == ((0, 0.0) if scale is None else (1, scale)), case
        assert a[19] == choice and (null(a[20]) if choice == 0.0 else a[20].value == noise.data_ptr()), case    # no uniforms without a temperature
        assert a[21] == (0.5 if top_p == 0.5 else 1.0), case

        for ctemps in ([choice, choice / 2, 0.0], None if choice == 0.0 else [0.0, 0.0, choice]):
            e.generate(None, ids, ctx, [1.0, 0.6, 0.3], [8, 4, 1], [False] * 3, 5, seed=9, image_base=11, guidance_scale=scale, context_lens=lens,
                       choice_temps=ctemps, top_p=top_p)
            a = only_call("pmhip_pipeline_generate_nucleus", 24)
            assert (a[4], a[5], a[7], a[11], a[12], a[13], a[15]) == (L, B, 3, 5, 9, 11, 0) and list(a[9]) == [8, 4, 1], case
            assert (null(a[6]) if lens is None else list(a[6]) == lens), case
            assert (a[20], a[21]) == ((0, 0.0) if scale is None else (1, scale)), case
            assert (null(a[22]) if not ctemps or not any(ctemps) else list(a[22]) == ctemps), case                # None and all-zero: NULL
            assert a[23] == (0.5 if top_p == 0.5 else 1.0), case

        if top_p is None:                                            # a slots step has no top_p
            slots = (_lib.Slot * B)()
            guides = None if scale is None else (_lib.SlotGuide * B)(_lib.SlotGuide(scale, 1), _lib.SlotGuide(0.0, 0))
            e.step_slots(dev_ids, ctx, slots, use_graph=True, want_aux=False, guides=guides, context_lens=lens, choice=[choice, 0.0])
            a = only_call("pmhip_pipeline_step_slots_choice", 13)
            assert (a[3], a[4], a[9]) == (L, B, _lib.SLOTS_GRAPH) and a[6] is slots and a[7] is guides, case
            assert (null(a[5]) if lens is None else list(a[5]) == lens), case
            assert (null(a[8]) if choice == 0.0 else list(a[8]) == [choice, 0.0]), case
    e.step_slots(dev_ids, ctx, (_lib.Slot * B)(), want_aux=False)    # choice=None, like all zero
    assert null(only_call("pmhip_pipeline_step_slots_choice", 13)[8])
    # forward: the entry with lengths, NULL without them
    for lens in (None, [2, 1]):
        e.forward(torch.zeros(B, N, 4), ctx, context_lens=lens)
        a = only_call("pmhip_s2_forward_lens", 8)
        assert (a[3], a[4]) == (L, B) and (null(a[5]) if lens is None else list(a[5]) == lens)


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
