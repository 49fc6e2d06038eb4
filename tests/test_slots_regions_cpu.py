"""Regional prompts per request in a decode session, without a GPU: the session option and what it leaves
alone, a regions session on the tiny CPU pipeline against ``Pipeline.generate(regions=)`` request by request, every new ValueError,
the per-slot arrays of the native step against ``region_layout``, and the host-side validation of the two new C entries."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import paintmind_amd as pm
from paintmind_amd import _lib, ops
from paintmind_amd.generate import MAX_REGIONS, Pipeline, region_layout
from paintmind_amd.serve import DecodeSession, FilterSession
from util import load_golden, to_torch_sd

NEW = ("pmhip_attention_pick", "pmhip_pipeline_step_slots_regions", "pmhip_s2_slots_region_steps")
# the parameter lists of both submits as they were before the option existed (regions=None was already the last one of each)
SUBMIT = ["self", "text", "timesteps", "temperature", "topk", "seed", "image_index", "context", "ids0", "guidance_scale",
          "choice_temperature", "negative_text", "negative_context", "keep_given", "image", "mask", "token_mask", "preserve", "regions"]
FILTER_SUBMIT = SUBMIT[:13] + ["top_p"] + SUBMIT[13:]


class _Rows(torch.nn.Module):
    """a text model whose prompts name their rows: "name:count" -> 77 rows of N(0, 1) keyed by the name, loud behind `count`"""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def forward(self, text, return_lens=False):
        rows, counts = [], []
        for prompt in text:
            name, count = prompt.split(":")
            g = torch.Generator().manual_seed(sum(ord(c) * 131 ** i for i, c in enumerate(name)))
            full = torch.randn(77, self.dim, generator=g)
            full[int(count):] = 7.0
            rows.append(full)
            counts.append(int(count))
        ctx = torch.stack(rows)
        return (ctx, torch.tensor(counts, dtype=torch.int32)) if return_lens else ctx


@pytest.fixture(scope="module")
def pipe():
    p, _ = load_golden("tiny_pipeline.npz")
    torch.manual_seed(4)
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False, text_model=_Rows(96)).eval()
    missing = pipe.load_state_dict({k: v for k, v in to_torch_sd(p).items() if not k.startswith("text_model")}, strict=False)
    assert not [k for k in missing.missing_keys if not k.startswith("text_model")]
    return pipe


def _masks(pipe):
    """the left half as a pixel mask, and a token mask that overlaps it"""
    S, g = pipe.image_size, pipe.image_size // pipe.patch_size
    left = torch.zeros(S, S, dtype=torch.uint8)
    left[:, :S // 2] = 1
    tm = torch.zeros(g, g, dtype=torch.bool)
    tm[1:3, 1:3] = True
    return left, tm


def test_new_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.pmhip_abi_version() == 11 == _lib.ABI_VERSION
    header = open(_lib._HERE + "/../include/pmhip.h").read()
    for name in NEW:
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None
        assert f"int {name}(" in header


def test_the_option_is_off_by_default_and_the_signatures_stay(pipe):
    assert inspect.signature(Pipeline.decode_session).parameters["regions"].default is False
    assert list(inspect.signature(DecodeSession.submit).parameters) == SUBMIT
    assert list(inspect.signature(FilterSession.submit).parameters) == FILTER_SUBMIT
    left, _ = _masks(pipe)
    for kw in (dict(), dict(filters=True), dict(regions=False)):
        session = pipe.decode_session(slots=2, conditional=True, **kw)
        assert session.regions is False
        with pytest.raises(ValueError, match="a decode session serves no regional prompts"):
            session.submit(text="a:5", regions=[("b:5", left)])
    assert type(pipe.decode_session(slots=2, regions=True)) is DecodeSession            # an option, not a class of its own ...
    both = pipe.decode_session(slots=2, regions=True, filters=True)
    assert type(both) is FilterSession and both.regions is True                          # ... so it composes with the filters


@torch.no_grad()
def test_a_regions_session_equals_generate_request_by_request(pipe):
    """two regions / one region / none, T = 3, admitted together into a 3-slot session: ids and images are exact"""
    left, tm = _masks(pipe)
    requests = [("a:77", [("d:30", left), ("e:12", tm)], 11), ("b:40", [("f:77", tm)], 12), ("c:10", None, 13)]
    session = pipe.decode_session(slots=3, conditional=True, regions=True)
    handles = [session.submit(text=t, regions=r, timesteps=3, topk=3, seed=s) for t, r, s in requests]
    assert [h.segments is not None for h in handles] == [True, True, False]
    assert handles[0].context.shape[0] == 77 * 3 and handles[1].context.shape[0] == 77 * 2 and handles[2].context.shape[0] == 77
    done = {f.handle.number: f for f in session.drain()}
    assert sorted(done) == [0, 1, 2]
    results = []
    for i, (t, r, s) in enumerate(requests):
        kw = {} if r is None else dict(regions=[r])
        imgs, ids = pipe.generate([t], timesteps=3, topk=3, save_interval=1, seed=s, return_ids=True, **kw)
        assert torch.equal(done[i].ids, ids[0]), i
        assert torch.equal(done[i].image, imgs[-1][0]), i
        results.append(ids[0])
    # the regions matter: the same prompt and seed without them is another result
    assert not torch.equal(pipe.generate(["a:77"], timesteps=3, topk=3, seed=11, return_ids=True)[1][0], results[0])


@torch.no_grad()
def test_regions_compose_with_guidance_a_negative_prompt_and_the_filters(pipe):
    left, tm = _masks(pipe)
    session = pipe.decode_session(slots=2, conditional=True, regions=True, filters=True)
    kw = dict(timesteps=3, topk=None, top_p=0.9, seed=21, guidance_scale=[1.0, 2.0, 3.0], negative_text="n:33", choice_temperature=2.0)
    session.submit(text="a:77", regions=[("d:30", left)], **kw)
    session.submit(text="b:40", timesteps=2, topk=3, seed=5)
    done = {f.handle.number: f for f in session.drain()}
    ids = pipe.generate(["a:77"], regions=[[("d:30", left)]], return_ids=True, **kw)[1]
    assert torch.equal(done[0].ids, ids[0])
    assert torch.equal(done[1].ids, pipe.generate(["b:40"], timesteps=2, topk=3, seed=5, return_ids=True)[1][0])


@torch.no_grad()
def test_context_tensors_instead_of_text(pipe):
    left, tm = _masks(pipe)
    glob, reg = pipe.text_model(["a:77"])[0, :20], pipe.text_model(["d:30"])[0, :30]
    session = pipe.decode_session(slots=1, conditional=True, regions=True)
    r = session.submit(context=glob, regions=[(reg, tm)], timesteps=2, topk=3, seed=3)
    assert torch.equal(r.context, torch.cat([glob, reg])) and r.segments[0].tolist() == [0] * 20 + [1] * 30
    ctx, ks, qm = region_layout([[glob, reg]], [[tm]], pipe.image_size, pipe.patch_size)
    opts = pipe._options(3, None, None, None, None, ctx, 1, timesteps=2)
    ids = pipe._generate_cpu(ctx, 1, 2, 1.0, opts, 1, 3, True, ops.host_keys(1, ctx.shape[1], pipe.num_tokens, None, ks, qm))[1]
    assert torch.equal(session.drain()[0].ids, ids[0])
    with pytest.raises(ValueError, match=r"\(context \[L_r, D\], mask\) pair"):
        session.submit(context=glob, regions=[("d:30", tm)])
    with pytest.raises(ValueError, match=r"\(context \[L_r, D\], mask\) pair"):
        session.submit(context=glob, regions=[(reg[:, :5], tm)])


def test_every_new_value_error(pipe):
    S = pipe.image_size
    left, tm = _masks(pipe)
    session = pipe.decode_session(slots=2, conditional=True, regions=True, max_context_len=100)
    with pytest.raises(ValueError, match=f"{MAX_REGIONS + 1} regions, at most {MAX_REGIONS}"):
        session.submit(text="a:5", regions=[("b:5", left)] * (MAX_REGIONS + 1))
    with pytest.raises(ValueError, match="a mask must be"):
        session.submit(text="a:5", regions=[("b:5", torch.ones(3, 3))])
    with pytest.raises(ValueError, match=r"\(prompt, mask\) pair"):
        session.submit(text="a:5", regions=["b:5"])
    with pytest.raises(ValueError, match="an edit request .* takes no regions"):
        session.submit(text="a:5", regions=[("b:5", left)], ids0=torch.zeros(pipe.num_tokens, dtype=torch.long), keep_given=True)
    with pytest.raises(ValueError, match="an edit request .* takes no regions"):
        session.submit(text="a:5", regions=[("b:5", left)], image=torch.zeros(3, S, S), mask=left)
    with pytest.raises(ValueError, match="154 rows does not fit the session's max_context_len=100"):
        session.submit(text="a:5", regions=[("b:5", left)])                       # 77 + 77: the capacity rules apply to the total
    assert session.submit(text="a:5", timesteps=1).context.shape[0] == 77       # ... and a plain request of 77 rows still fits
    assert not session.queue[-1].edit and session.queue[-1].segments is None
    unconditional = pipe.decode_session(slots=2, conditional=False, regions=True)
    with pytest.raises(ValueError, match="regions need a text condition"):
        unconditional.submit(regions=[("b:5", left)])


def test_the_per_slot_arrays_agree_with_region_layout(pipe):
    """three occupied slots of four (two regions / none / one region) at capacities 231 and 260: a regional slot's rows are
    region_layout's rows of that image with 255 behind its total, the others carry the one-segment layout and flag 0"""
    left, tm = _masks(pipe)
    session = pipe.decode_session(slots=4, conditional=True, regions=True)
    assert session._segment_arrays(10) is None
    plain = session.submit(text="c:10", timesteps=1)
    session._admit()
    assert session._segment_arrays(77) is None                                   # no occupied slot is regional: the step without
    a = session.submit(text="a:77", regions=[("d:30", left), ("e:12", tm)], timesteps=1)
    b = session.submit(text="b:40", regions=[("f:77", tm)], timesteps=1)
    session._admit()
    assert (plain.slot, a.slot, b.slot) == (0, 1, 2)
    _, ks, qm = pipe._region_context(["a:77", "b:40"], [[("d:30", left), ("e:12", tm)], [("f:77", tm)]], False)
    for cap in (231, 260):
        cs, ts, flags = session._segment_arrays(cap)
        assert cs.dtype == np.uint8 and cs.shape == (4, cap) and ts.dtype == np.uint32 and ts.shape == (4, pipe.num_tokens)
        assert flags.dtype == np.uint8 and flags.tolist() == [0, 1, 1, 0]
        for slot, row in ((1, 0), (2, 1)):
            assert np.array_equal(cs[slot, :231], ks[row]) and (cs[slot, 231:] == 255).all()
            assert np.array_equal(ts[slot], qm[row])
        assert (cs[2, 154:] == 255).all() and cs[2, 153] == 1
        assert cs[0].tolist() == [0] * 77 + [255] * (cap - 77) and ts[0].tolist() == [1] * pipe.num_tokens
        assert ts[3].tolist() == [1] * pipe.num_tokens and (cs[3] == 0).all()   # idle: one segment, every token attending to it


def test_native_entries_check_their_arguments_before_anything_runs():
    """A handle made on the host and fake non-null pointers everywhere else: a call that got past the checks would fault, so every
    one of these is refused before anything is staged or launched."""
    lib = _lib.load()
    p = C.c_void_p(64)
    B, L, N = 3, 5, 16
    cfg = _lib.S2Cfg(N, 32, 64, 128, 128, _lib.TowerCfg(128, 0, 2, 256, 64))
    handle = C.c_void_p()
    assert lib.pmhip_s2_create(C.byref(handle), 0, _lib.F32, C.byref(cfg), C.byref(_lib.S2Weights())) == _lib.PMHIP_OK
    slots = (_lib.Slot * B)()
    for b in range(B):
        slots[b].topk, slots[b].num_mask, slots[b].temperature, slots[b].step = 3, 1, 1.0, 0
    slots[1].step = _lib.SLOT_IDLE
    seg = lambda rows: (C.c_ubyte * (B * L))(*[v for r in rows for v in r])
    tok = lambda rows: (C.c_uint32 * (B * N))(*[v for r in rows for v in r])
    flag = lambda *v: (C.c_ubyte * B)(*v)
    good_seg, good_tok = [[0, 1, 1, 255, 255]] * B, [[1] * N] * B

    def call(s, t, f, ctx=p, L=L, lens=None):
        return lib.pmhip_pipeline_step_slots_regions(handle, p, ctx, L, B, lens, slots, None, None, None, 0, None, None, None, s, t, f, 0,
                                                     None, None, None)
    bad_id = [r[:] for r in good_seg]
    bad_id[2][3] = 40
    no_key = [r[:] for r in good_tok]
    no_key[0][9] = 0b100
    idle_bad = [good_seg[0], [77] * L, good_seg[2]]                          # slot 1 is idle: its rows and its flag are not looked at
    try:
        for s, t, f, words in ((seg(good_seg), None, flag(1, 0, 1), ("come together",)), (None, tok(good_tok), None, ("come together",)),
                               (seg(good_seg), tok(good_tok), None, ("come together",)),
                               (seg(good_seg), tok(good_tok), flag(1, 0, 2), ("slot 2", "region_host=2")),
                               (seg(bad_id), tok(good_tok), flag(1, 0, 1), ("slot 2", "context row 3", "segment 40")),
                               (seg(good_seg), tok(no_key), flag(1, 0, 1), ("slot 0", "token 9", "allows no segment"))):
            assert call(s, t, f) == _lib.PMHIP_EINVAL, words
            msg = lib.pmhip_last_error().decode()
            assert "pipeline_step_slots_regions" in msg and all(w in msg for w in words), msg
        assert call(seg(good_seg), tok(good_tok), flag(1, 0, 1), ctx=None, L=0) == _lib.PMHIP_EINVAL
        assert b"without a context" in lib.pmhip_last_error()
        # a plain slot keeps the length check, a regional slot's length is not used
        assert call(seg(good_seg), tok(good_tok), flag(1, 9, 0), lens=(C.c_int * B)(99, 1, 9)) == _lib.PMHIP_EINVAL
        assert b"image 2: context length 9" in lib.pmhip_last_error()
        # rows and flags of idle slots are not looked at: such a call gets past the region checks and is stopped by a later one
        slots[0].topk = 0
        assert call(seg(idle_bad), tok(good_tok), flag(1, 7, 0)) == _lib.PMHIP_EINVAL and b"slot 0: topk=0" in lib.pmhip_last_error()
        slots[0].topk = 3
        steps = C.c_int(-1)
        assert lib.pmhip_s2_slots_region_steps(handle, C.byref(steps)) == _lib.PMHIP_OK and steps.value == 0
        assert lib.pmhip_s2_slots_region_steps(None, C.byref(steps)) == _lib.PMHIP_EINVAL
    finally:
        lib.pmhip_s2_destroy(handle)
    # the operator: pick is required, and exactly one form
    args = lambda lens, ks, qm, pick, want=0: (0, p, p, p, p, 64, 1, 1, 64, 16, 64, 64, 0, lens, ks, qm, pick, want, None)
    for a, word in ((args(p, None, None, None), b"pick is NULL"), (args(None, None, None, p), b"exactly one"),
                    (args(p, p, p, p), b"exactly one"), (args(None, p, None, p), b"go together"), (args(None, None, p, p), b"go together"),
                    (args(p, None, None, p, 256), b"want=256"), (args(p, None, None, p, -1), b"want=-1")):
        assert lib.pmhip_attention_pick(*a) == _lib.PMHIP_EINVAL
        assert word in lib.pmhip_last_error(), lib.pmhip_last_error()
    # ... behind which the family's checks follow, under the entry's name
    assert lib.pmhip_attention_pick(7, p, p, p, p, 64, 1, 1, 64, 16, 64, 64, 0, p, None, None, p, 0, None) == _lib.PMHIP_EINVAL
    assert b"attention_pick: bad dtype 7" in lib.pmhip_last_error()
