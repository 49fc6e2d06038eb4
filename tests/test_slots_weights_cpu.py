"""Prompt weights per request in a decode session, without a GPU: the session option and what it leaves alone,
a weights session on the tiny CPU pipeline against ``Pipeline.generate`` request by request (a prompt with emphasis, one without, a
regional request with a weighted item, an explicit (context, weights) pair), every new ValueError, the per-step arrays of the native
step against ``ops.host_weights`` / ``region_layout``, and the host-side validation of the two new C entries.

The text model is a one-layer T5 over a character tokenizer (as in tests/test_weights_cpu.py): its weighted mode gives every context
row the weight of the fragment its character came from."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import paintmind_amd as pm
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline
from paintmind_amd.modules.encoder import T5TextEmbedder
from paintmind_amd.serve import DecodeSession, FilterSession, weighted
from util import load_golden, to_torch_sd

NEW = ("pmhip_attention_pick_weighted", "pmhip_pipeline_step_slots_weights", "pmhip_s2_slots_weight_steps")
SUBMIT = ["self", "text", "timesteps", "temperature", "topk", "seed", "image_index", "context", "ids0", "guidance_scale",
          "choice_temperature", "negative_text", "negative_context", "keep_given", "image", "mask", "token_mask", "preserve", "regions"]
FILTER_SUBMIT = SUBMIT[:13] + ["top_p"] + SUBMIT[13:]
LMAX = 24                                                    # rows of every prompt's context
EMPH, PLAIN = "a (red:1.4) barn, (blurry:0.5)", "a plain barn"


class CharTokenizer:
    """one id per character (2 + ord % 100), pad 0, end-of-sequence 1; both call forms the embedder uses"""
    pad_token_id, eos_token_id = 0, 1

    @staticmethod
    def ids_of(s):
        return [2 + ord(c) % 100 for c in s]

    def __call__(self, text, max_length=77, add_special_tokens=True, **kw):
        if isinstance(text, str):
            return {"input_ids": self.ids_of(text) + ([1] if add_special_tokens else [])}
        ids = torch.zeros(len(text), max_length, dtype=torch.long)
        for i, s in enumerate(text):
            row = self.ids_of(s)[:max_length - 1] + [1]
            ids[i, :len(row)] = torch.tensor(row)
        return {"input_ids": ids}


@pytest.fixture(scope="module")
def pipe():
    from transformers import T5Config, T5EncoderModel
    p, _ = load_golden("tiny_pipeline.npz")
    torch.manual_seed(3)
    tower = T5EncoderModel(T5Config(vocab_size=128, d_model=96, d_kv=16, d_ff=64, num_layers=1, num_heads=2))
    emb = T5TextEmbedder(tokenizer=CharTokenizer(), transformer=tower, max_length=LMAX)
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False, text_model=emb).eval()
    missing = pipe.load_state_dict({k: v for k, v in to_torch_sd(p).items() if not k.startswith("text_model")}, strict=False)
    assert not [k for k in missing.missing_keys if not k.startswith("text_model")]
    return pipe


def _top(pipe):
    g = pipe.image_size // pipe.patch_size
    top = np.zeros((g, g), bool)
    top[:g // 2] = True
    return top


def test_new_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.pmhip_abi_version() == 11 == _lib.ABI_VERSION
    header = open(_lib._HERE + "/../include/pmhip.h").read()
    for name in NEW:
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None
        assert f"int {name}(" in header


def test_the_rule():
    assert not weighted(None) and not weighted(np.ones(5, np.float32)) and not weighted([1, 1.0])
    assert weighted([1, 1, 0]) and weighted(np.float32([1, 1.0000001])) and weighted(torch.tensor([2.0]).numpy())


def test_the_option_is_off_by_default_and_the_signatures_stay(pipe):
    assert inspect.signature(Pipeline.decode_session).parameters["weights"].default is False
    assert list(inspect.signature(DecodeSession.submit).parameters) == SUBMIT
    assert list(inspect.signature(FilterSession.submit).parameters) == FILTER_SUBMIT
    top = _top(pipe)
    ctx = pipe.text_model([PLAIN])[0]
    for kw in (dict(), dict(filters=True), dict(regions=True), dict(weights=False, regions=True)):
        session = pipe.decode_session(slots=2, conditional=True, **kw)
        assert session.weights is False
        if session.regions:                                                        # the triple item raises as before
            with pytest.raises(ValueError, match="a decode session serves no prompt weights"):
                session.submit(text=PLAIN, regions=[("x", top, 0.5)])
        with pytest.raises((ValueError, AttributeError)):                          # ... and so does the pair
            session.submit(context=(ctx, np.ones(LMAX, np.float32)))
        # emphasis syntax is text like any other: the prompt goes through the unweighted call of the text model
        assert torch.equal(session.submit(text=EMPH, timesteps=1).context, pipe.text_model([EMPH])[0])
        assert session.queue[-1].weights is None
    assert type(pipe.decode_session(slots=2, weights=True)) is DecodeSession        # an option, not a class of its own ...
    every = pipe.decode_session(slots=2, weights=True, regions=True, filters=True)
    assert type(every) is FilterSession and every.weights is True and every.regions is True   # ... so it composes with the other two


@torch.no_grad()
def test_a_weights_session_equals_generate_request_by_request(pipe):
    """four requests of T = 3 admitted together into a 4-slot session; ids and images are exact"""
    top = _top(pipe)
    ctx, _, w = pipe.text_model(["(sky:2) over (sea:0.25)"], weighted=True)
    session = pipe.decode_session(slots=4, conditional=True, weights=True, regions=True)
    kw = dict(timesteps=3, topk=4)
    handles = [session.submit(text=EMPH, seed=11, **kw), session.submit(text=PLAIN, seed=12, **kw),
               session.submit(text="the sky", regions=[("(x:3) y", top, 0.5)], seed=13, **kw),
               session.submit(context=(ctx[0], w[0]), seed=14, **kw)]
    assert [h.weights is not None for h in handles] == [True, False, True, True]
    assert [h.segments is not None for h in handles] == [False, False, True, False]
    assert handles[0].context.shape[0] == LMAX and handles[2].context.shape[0] == 2 * LMAX     # attended to in full
    assert sorted(set(handles[0].weights.tolist())) == pytest.approx([0.5, 1.0, 1.4])
    n0 = LMAX
    assert handles[2].weights[n0:n0 + 4].tolist() == [1.5, 0.5, 0.5, 0.5] and (handles[2].weights[:n0] == 1).all()
    done = {f.handle.number: f for f in session.drain()}
    assert sorted(done) == [0, 1, 2, 3]
    g = dict(timesteps=3, topk=4, save_interval=1, return_ids=True)
    want = [pipe.generate([EMPH], prompt_weights=True, seed=11, **g), pipe.generate([PLAIN], seed=12, **g),
            pipe.generate(["the sky"], prompt_weights=True, regions=[[("(x:3) y", top, 0.5)]], seed=13, **g)]
    opts = pipe._options(4, None, None, None, None, ctx, 1, None, None, 3)
    want.append(pipe._generate_cpu(ctx, 1, 3, 1.0, opts, 1, 14, True, ops.host_keys(1, LMAX, pipe.num_tokens, context_weights=w)))
    for i, (imgs, ids) in enumerate(want):
        assert torch.equal(done[i].ids, ids[0]), i
        assert torch.equal(done[i].image, imgs[-1][0]), i
    # the emphasis matters: the same words and seed without it are another result
    assert not torch.equal(pipe.generate(["a red barn, blurry"], seed=11, **g)[1][0], want[0][1][0])
    # a prompt without emphasis is the plain request of a session without the option
    plain = pipe.decode_session(slots=1, conditional=True)
    plain.submit(text=PLAIN, seed=12, **kw)
    assert torch.equal(plain.drain()[0].ids, done[1].ids)


@torch.no_grad()
def test_weights_compose_with_guidance_a_negative_prompt_and_the_filters(pipe):
    session = pipe.decode_session(slots=2, conditional=True, weights=True, filters=True)
    kw = dict(timesteps=3, topk=None, top_p=0.9, seed=21, guidance_scale=[1.0, 2.0, 3.0], negative_text="(ugly:3)", choice_temperature=2.0)
    session.submit(text=EMPH, **kw)
    session.submit(text=PLAIN, timesteps=2, topk=3, seed=5)
    done = {f.handle.number: f for f in session.drain()}
    ids = pipe.generate([EMPH], prompt_weights=True, return_ids=True, **kw)[1]             # negative_text is not read for emphasis
    assert torch.equal(done[0].ids, ids[0])
    assert torch.equal(done[1].ids, pipe.generate([PLAIN], timesteps=2, topk=3, seed=5, return_ids=True)[1][0])


def test_every_new_value_error(pipe):
    S = pipe.image_size
    top = _top(pipe)
    ctx = pipe.text_model([PLAIN])[0]
    session = pipe.decode_session(slots=2, conditional=True, weights=True, regions=True)
    w = np.ones(LMAX, np.float32)
    w[3] = 2.0
    for bad, words in ((2.0 ** 21, "must be 0 or in"), (-1.0, "must be 0 or in"), (float("nan"), "must be 0 or in"), (2.0 ** -21, "must be 0 or in")):
        v = w.copy()
        v[5] = bad
        with pytest.raises(ValueError, match=words):
            session.submit(context=(ctx, v))
    with pytest.raises(ValueError, match="must be 0 or in"):
        session.submit(text=PLAIN, regions=[("x", top, 2.0 ** 21)])
    with pytest.raises(ValueError, match="allows no context row with a weight above 0"):
        session.submit(context=(ctx, np.zeros(LMAX, np.float32)))
    with pytest.raises(ValueError, match="one per context row"):
        session.submit(context=(ctx, w[:5]))
    with pytest.raises(ValueError, match="a tensor .* or a pair"):
        session.submit(context=(ctx, w, w))
    with pytest.raises(ValueError, match="an edit request .* takes no prompt weights"):
        session.submit(text=EMPH, ids0=torch.zeros(pipe.num_tokens, dtype=torch.long), keep_given=True)
    with pytest.raises(ValueError, match="an edit request .* takes no prompt weights"):
        session.submit(context=(ctx, w), image=torch.zeros(3, S, S), token_mask=torch.from_numpy(top))
    # an edit request without emphasis is served as before
    assert session.submit(text=PLAIN, ids0=torch.full((pipe.num_tokens,), pipe.mask_token_id), keep_given=True, timesteps=1).edit
    with pytest.raises(ValueError, match="position"):
        session.submit(text="(never closed")
    unconditional = pipe.decode_session(slots=2, conditional=False, weights=True)
    with pytest.raises(ValueError, match="prompt weights need a text condition"):
        unconditional.submit(context=(ctx, w))
    assert unconditional.submit(text=EMPH, timesteps=1).weights is None           # (an unconditional session reads no text)


def test_the_per_step_arrays(pipe):
    """four slots: emphasis / plain / regional with a weighted item / idle, at capacities 48 and 60"""
    top = _top(pipe)
    session = pipe.decode_session(slots=4, conditional=True, weights=True, regions=True)
    assert session._segment_arrays(10) is None and session._weight_array(10) is None
    plain = session.submit(text=PLAIN, timesteps=1)
    session._admit()
    assert session._segment_arrays(LMAX) is None and session._weight_array(LMAX) is None   # no such slot: the step without
    a = session.submit(text=EMPH, timesteps=1)
    b = session.submit(text="the sky", regions=[("(x:3) y", top, 0.5)], timesteps=1)
    session._admit()
    assert (plain.slot, a.slot, b.slot) == (0, 1, 2)
    _, ks, qm, wr = pipe._region_context_weighted(["the sky"], [[("(x:3) y", top, 0.5)]], False, True)
    _, _, wa = pipe.text_model([EMPH], weighted=True)
    for cap in (48, 60):
        cs, ts, kinds = session._segment_arrays(cap)
        w = session._weight_array(cap)
        assert kinds.dtype == np.uint8 and kinds.tolist() == [0, 2, 2, 0]
        assert w.dtype == np.float32 and w.shape == (4, cap) and cs.shape == (4, cap) and ts.shape == (4, pipe.num_tokens)
        # the weighted slot without regions: the one-segment layout, its weights, 1 behind its total
        assert cs[1].tolist() == [0] * LMAX + [255] * (cap - LMAX) and ts[1].tolist() == [1] * pipe.num_tokens
        assert np.array_equal(w[1, :LMAX], wa[0].numpy()) and (w[1, LMAX:] == 1).all()
        # ... which is what ops.host_weights makes of them beside the length (its token masks allow every segment)
        hs, _, hw = ops.host_weights(w[1:2], 1, cap, pipe.num_tokens, context_lens=[LMAX])
        assert np.array_equal(hs[0], cs[1]) and np.array_equal(hw[0], w[1])
        # the weighted regional slot: region_layout's rows, 255 behind its total, its weights
        assert np.array_equal(cs[2, :48], ks[0]) and (cs[2, 48:] == 255).all() and np.array_equal(ts[2], qm[0])
        assert np.array_equal(w[2, :48], wr[0]) and (w[2, 48:] == 1).all()
        # plain and idle slots: weights of 1
        assert (w[0] == 1).all() and (w[3] == 1).all() and cs[0].tolist() == [0] * LMAX + [255] * (cap - LMAX)
    # a regional request without emphasis beside them keeps kind 1
    session._retire(plain)
    r = session.submit(text=PLAIN, regions=[("y", top)], timesteps=1)
    session._admit()
    assert r.slot == 0 and r.weights is None and session._segment_arrays(48)[2].tolist() == [1, 2, 2, 0]
    # ... and once the weighted ones are gone no weights array is passed
    session._retire(a)
    session._retire(b)
    assert session._weight_array(48) is None and session._segment_arrays(48)[2].tolist() == [1, 0, 0, 0]


def test_native_entries_check_their_arguments_before_anything_runs():
    """A handle made on the host and fake non-null pointers everywhere else (the ids among them): a call that got past the checks
    would fault, so every one of these is refused before anything is staged or launched, the ids untouched."""
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
    wts = lambda rows: (C.c_float * (B * L))(*[v for r in rows for v in r])
    kind = lambda *v: (C.c_ubyte * B)(*v)
    good_seg, good_tok, good_w = [[0, 1, 1, 255, 255]] * B, [[1] * N] * B, [[1.0, 0.0, 8.0, 0.125, 1.0]] * B
    nan = float("nan")

    def call(s, t, f, w, ctx=p, L=L, lens=None):
        return lib.pmhip_pipeline_step_slots_weights(handle, p, ctx, L, B, lens, slots, None, None, None, 0, None, None, None, s, t, f, w, 0,
                                                     None, None, None)
    S, T, W = seg(good_seg), tok(good_tok), wts(good_w)
    bad_id = [r[:] for r in good_seg]
    bad_id[2][3] = 40
    dead = [r[:] for r in good_tok]
    dead[0][9] = 0b10                                                         # segment 1: rows 1 and 2 ...
    w_dead = [[1.0, 0.0, 0.0, 1.0, 1.0]] + good_w[1:]                         # ... both at weight 0 in slot 0 (rows 3, 4 are padding)
    try:
        cases = [(S, T, kind(2, 0, 3), W, ("slot 2", "region_host=3", "0, 1 or 2")),
                 (S, T, kind(2, 0, 1), None, ("pipeline_step_slots_regions", "slot 0", "region_host=2")),
                 (None, None, None, W, ("ctx_w_host given without",)),
                 (S, None, kind(2, 0, 1), W, ("come together",)),
                 (seg(bad_id), T, kind(1, 0, 2), W, ("slot 2", "context row 3", "segment 40")),
                 (S, tok(dead), kind(2, 0, 1), wts(w_dead), ("slot 0", "token 9", "allows no context row with a weight above 0"))]
        for bad in (2.0 ** 21, 2.0 ** -21, -1.0, nan, float("inf")):
            rows = [r[:] for r in good_w]
            rows[2][1] = bad
            cases.append((S, T, kind(1, 0, 2), wts(rows), ("slot 2", "context row 1", "must be 0 or in [2^-20, 2^20]")))
        for s, t, f, w, words in cases:
            assert call(s, t, f, w) == _lib.PMHIP_EINVAL, words
            msg = lib.pmhip_last_error().decode()
            assert all(x in msg for x in words), msg
            assert "pipeline_step_slots_weights" in msg or w is None, msg
        assert call(S, T, kind(2, 0, 1), W, ctx=None, L=0) == _lib.PMHIP_EINVAL and b"without a context" in lib.pmhip_last_error()
        # a slot of kind 0 keeps the length check; a weighted slot's length is not used
        assert call(S, T, kind(2, 9, 0), W, lens=(C.c_int * B)(99, 1, 9)) == _lib.PMHIP_EINVAL
        assert b"image 2: context length 9" in lib.pmhip_last_error()
        # the weight rows of slots of kind 0 and 1 and of idle slots are not looked at (nor is a token of theirs that would allow no
        # weighted row): such a call gets past the weight checks and is stopped by a later one
        slots[0].topk = 0
        loose = [[nan] * L, [-5.0] * L, good_w[2]]
        assert call(S, tok(dead), kind(1, 7, 2), wts(loose)) == _lib.PMHIP_EINVAL and b"slot 0: topk=0" in lib.pmhip_last_error()
        assert call(S, T, kind(0, 7, 2), wts(loose)) == _lib.PMHIP_EINVAL and b"slot 0: topk=0" in lib.pmhip_last_error()
        slots[0].topk = 3
        steps = C.c_int(-1)
        assert lib.pmhip_s2_slots_weight_steps(handle, C.byref(steps)) == _lib.PMHIP_OK and steps.value == 0
        assert lib.pmhip_s2_slots_region_steps(handle, C.byref(steps)) == _lib.PMHIP_OK and steps.value == 0
        assert lib.pmhip_s2_slots_weight_steps(None, C.byref(steps)) == _lib.PMHIP_EINVAL
    finally:
        lib.pmhip_s2_destroy(handle)
    # the operator: pick and the three arrays are required
    args = lambda ks, qm, bias, pick, want=2: (0, p, p, p, p, 64, 1, 1, 64, 16, 64, 64, 0, ks, qm, bias, pick, want, None)
    for a, word in ((args(p, p, p, None), b"pick is NULL"), (args(None, p, p, p), b"key_bias is NULL"), (args(p, None, p, p), b"key_bias is NULL"),
                    (args(p, p, None, p), b"key_bias is NULL"), (args(p, p, p, p, 256), b"want=256"), (args(p, p, p, p, -1), b"want=-1")):
        assert lib.pmhip_attention_pick_weighted(*a) == _lib.PMHIP_EINVAL
        assert word in lib.pmhip_last_error(), lib.pmhip_last_error()
    # ... behind which the family's checks follow, under the entry's name
    assert lib.pmhip_attention_pick_weighted(7, p, p, p, p, 64, 1, 1, 64, 16, 64, 64, 0, p, p, p, p, 2, None) == _lib.PMHIP_EINVAL
    assert b"attention_pick_weighted: bad dtype 7" in lib.pmhip_last_error()
