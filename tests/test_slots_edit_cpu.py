"""Edit requests in decode sessions, without a GPU: a CPU-session edit request must equal
``pipe.edit(img[None], ...)`` with the same seed whatever shares the session with it, kept ids stay, an empty mask gives
``decode(encode(img))``; the ValueErrors of ``submit``; the surface; and the host validation of the new native entries, which refuse
bad arguments before anything is staged or launched."""
import ctypes as C
import inspect

import pytest
import torch

import paintmind_amd as pm
from paintmind_amd import _lib, ops
from paintmind_amd.engine import S2Engine
from paintmind_amd.generate import Pipeline, edit_schedule
from paintmind_amd.serve import DecodeSession, FilterSession
from util import load_golden, to_torch_sd


@pytest.fixture(scope="module")
def pipe():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False).eval()
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not [k for k in missing.missing_keys if not k.startswith("text_model")]
    return pipe


def _inputs(pipe, n=4):
    """n images and per image a token mask (5 tokens, all, none, one) with the pixel mask of one lit pixel per masked token"""
    g, p = pipe.image_size // pipe.patch_size, pipe.patch_size
    gen = torch.Generator().manual_seed(12)
    img = torch.rand(n, 3, pipe.image_size, pipe.image_size, generator=gen) * 2 - 1
    tm = torch.zeros(n, g * g, dtype=torch.bool)
    tm[0, torch.randperm(g * g, generator=gen)[:5]] = True
    tm[1] = True
    tm[3, 6] = True
    tm = tm.reshape(n, g, g)
    pix = torch.zeros(n, pipe.image_size, pipe.image_size, dtype=torch.uint8)
    for b, r, c in tm.nonzero().tolist():
        pix[b, r * p + (r + c) % p, c * p + (2 * r + c) % p] = 200
    return img, tm, pix


def test_cpu_session_edit_requests_equal_edit_alone(pipe):
    img, tm, pix = _inputs(pipe)
    enc = pipe.to_latent(img)[1].reshape(4, -1)
    s = pipe.decode_session(slots=2, conditional=True, filters=True)
    # (text, T, temperature, topk, top_p, seed, extra): four edits and one generation share two slots
    plan = [("a", 8, 1.0, 5, None, 11, dict(token_mask=tm[0])),
            ("b", 3, 0.7, None, 0.9, 22, dict(mask=pix[1], choice_temperature=4.5)),
            ("c", 2, 1.0, 3, None, 33, dict(token_mask=tm[2])),
            ("d", 4, 1.3, 40, None, 44, dict(mask=pix[3], preserve="pixels", guidance_scale=2.0, negative_text="blurry"))]
    handles = [s.submit(text=tx, timesteps=T, temperature=temp, topk=k, top_p=p, seed=seed, image=img[i], **kw)
               for i, (tx, T, temp, k, p, seed, kw) in enumerate(plan)]
    gen_h = s.submit(text="e", timesteps=3, topk=5, seed=55)
    assert [h.edit for h in handles] == [True] * 4 and not gen_h.edit
    assert handles[0].nmask == [4, 3, 2, 1, 0, 0, 0, 0] == edit_schedule(5, 8) and handles[2].nmask == [0, 0]
    done = {f.handle.number: f for f in s.drain()}
    assert len(done) == 5
    for i, (tx, T, temp, k, p, seed, kw) in enumerate(plan):
        want_img, want_ids = pipe.edit(img[i:i + 1], text=[tx], timesteps=T, temperature=temp, topk=k, top_p=p, seed=seed, return_ids=True,
                                       **kw)
        f = done[i]
        assert torch.equal(f.ids, want_ids[0]) and torch.equal(f.image, want_img[0]), i
        keep = ~tm[i].reshape(-1)
        assert torch.equal(f.ids[keep], enc[i][keep]) and not bool((f.ids == pipe.mask_token_id).any())
    # an empty mask: decode(encode(img)); preserve="pixels": the input outside the pixel mask, bit for bit
    assert torch.equal(done[2].ids, enc[2]) and torch.equal(done[2].image, pipe.vqgan.decode_from_indice(enc[2:3])[0])
    sel = (pix[3] != 0)[None].expand_as(img[3])
    assert torch.equal(done[3].image[~sel], img[3][~sel])
    # the generation beside them is the generation alone
    imgs, ids = pipe.generate(["e"], timesteps=3, topk=5, save_interval=1, seed=55, return_ids=True)
    assert torch.equal(done[4].ids, ids[0]) and torch.equal(done[4].image, imgs[-1][0])


def test_ids0_with_keep_given_is_the_same_edit(pipe):
    img, tm, _ = _inputs(pipe)
    enc = pipe.to_latent(img)[1].reshape(4, -1)
    start = torch.where(tm[0].reshape(-1), torch.full_like(enc[0], pipe.mask_token_id), enc[0])
    s = pipe.decode_session(slots=1, conditional=False)
    a = s.submit(timesteps=4, seed=5, ids0=start, keep_given=True)
    b = s.submit(timesteps=4, seed=5, image=img[0], token_mask=tm[0])
    c = s.submit(timesteps=4, seed=5, ids0=start)                        # without keep_given: the reference's schedule over the image
    assert a.edit and b.edit and not c.edit and a.nmask == b.nmask == edit_schedule(5, 4) and c.nmask != a.nmask
    fa, fb, fc = s.drain()
    want_img, want_ids = pipe.edit(img[:1], token_mask=tm[0], timesteps=4, seed=5, return_ids=True)
    for f in (fa, fb):
        assert torch.equal(f.ids, want_ids[0]) and torch.equal(f.image, want_img[0])
    assert int((fc.ids == pipe.mask_token_id).sum()) == 1                # that loop leaves one mask id behind


def test_submit_refuses_what_does_not_fit_together(pipe, monkeypatch):
    monkeypatch.setattr(Pipeline, "_sample_cpu", lambda *a, **k: pytest.fail("a step ran"))
    img, tm, pix = _inputs(pipe)
    ids0 = torch.zeros(pipe.num_tokens, dtype=torch.long)
    for session in (pipe.decode_session(slots=2, conditional=False), pipe.decode_session(slots=2, conditional=False, filters=True)):
        for kw, match in ((dict(keep_given=True), "keep_given"),
                          (dict(image=img[0], mask=pix[0], ids0=ids0), "not both"),
                          (dict(mask=pix[0]), "needs the image"),
                          (dict(token_mask=tm[0]), "needs the image"),
                          (dict(image=img[0]), "exactly one"),
                          (dict(image=img[0], mask=pix[0], token_mask=tm[0]), "exactly one"),
                          (dict(image=img[0], mask=pix[0], preserve="both"), "preserve"),
                          (dict(preserve="pixels"), "needs the image"),
                          (dict(image=img[:1], mask=pix[0]), r"\[C, H, W\]"),
                          (dict(image=img[0], token_mask=tm[0].float()), "token_mask")):
            with pytest.raises(ValueError, match=match):
                session.submit(timesteps=2, **kw)
        assert not session.queue                                         # nothing of it was queued


NEW = ("pmhip_remask_slots_counts", "pmhip_remask_choice_slots_counts", "pmhip_pipeline_step_slots_edit", "pmhip_s2_slots_edit_steps")


def test_surface():
    lib = _lib.load()
    header = open(_lib._HERE + "/../include/pmhip.h").read()
    for name in NEW:
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None and f"int {name}(" in header
    P = _lib.PROTOTYPES
    # a count array behind the records (and the choice array); the step: the filter entry with counts_host in front of the flags
    old = P["pmhip_remask_slots"][1]
    assert P["pmhip_remask_slots_counts"][1] == old[:3] + [_lib.vp] + old[3:]
    old = P["pmhip_remask_choice_slots"][1]
    assert P["pmhip_remask_choice_slots_counts"][1] == old[:4] + [_lib.vp] + old[4:]
    old = P["pmhip_pipeline_step_slots_filter"][1]
    assert P["pmhip_pipeline_step_slots_edit"][1] == old[:13] + [C.POINTER(_lib.i32)] + old[13:]
    assert C.sizeof(_lib.Slot) == 32 and _lib.ABI_VERSION == 11 == lib.pmhip_abi_version()
    for cls in (DecodeSession, FilterSession):
        sig = inspect.signature(cls.submit).parameters
        assert sig["keep_given"].default is False and sig["preserve"].default == "tokens"
        assert all(sig[k].default is None for k in ("image", "mask", "token_mask"))
    assert inspect.signature(S2Engine.step_slots).parameters["counts"].default is None
    assert list(inspect.signature(ops.remask_slots_counts).parameters) == ["ids", "scores", "slots", "counts", "mask_id", "choice"]


def test_the_operator_entries_refuse_bad_arguments_before_a_launch():
    """fake non-null pointers that are never dereferenced: a call that got past the checks would not return PMHIP_EINVAL"""
    lib = _lib.load()
    p = C.c_void_p(64)
    plain, choice = lib.pmhip_remask_slots_counts, lib.pmhip_remask_choice_slots_counts
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert plain(*args, 64, 2, 16, None) == _lib.PMHIP_EINVAL and b"remask_slots_counts: null pointer" in lib.pmhip_last_error()
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        assert choice(*args, 64, 2, 16, None) == _lib.PMHIP_EINVAL and b"remask_choice_slots_counts: null pointer" in lib.pmhip_last_error()
    for B, N in ((0, 16), (2, 0), (2, 4097), (-1, 16)):
        assert plain(p, p, p, p, 64, B, N, None) == _lib.PMHIP_EINVAL and b"remask_slots_counts: bad shape" in lib.pmhip_last_error()
        assert choice(p, p, p, p, p, 64, B, N, None) == _lib.PMHIP_EINVAL and b"remask_choice_slots_counts: bad shape" in lib.pmhip_last_error()


@pytest.fixture(scope="module")
def host_handle():
    """a stage-2 handle: creating one touches no device (the weights are only kept), and the slots entries validate their host
    records before they stage or launch anything"""
    lib = _lib.load()
    tower = _lib.TowerCfg(dim=64, depth=1, heads=1, hidden_pad=64, dim_head=64)
    cfg = _lib.S2Cfg(tokens=16, embed_dim=32, n_embed=256, context_dim=64, context_dim_pad=64, tower=tower)
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


def test_the_step_validates_every_count_on_the_host_and_names_the_slot(host_handle):
    lib = _lib.load()
    p = C.c_void_p(256)                      # a call that got past the checks would fault: every one of these is refused before
    good = (1, 0, 1.0, 3, 4, 0)

    def step(records, counts, handle=host_handle):
        cn = None if counts is None else (C.c_int * len(counts))(*counts)
        return lib.pmhip_pipeline_step_slots_edit(handle, p, None, 0, len(records), None, records, None, None, None, 0, None, None, cn, 0,
                                                  None, None, None)

    for bad in (-2, 17, 2 ** 31 - 1, -2 ** 31):
        assert step(_records(good, good, good), [-1, 3, bad]) == _lib.PMHIP_EINVAL
        msg = lib.pmhip_last_error().decode()
        assert "pipeline_step_slots_edit" in msg and "slot 2" in msg and f"count {bad}" in msg and "tokens=16" in msg, msg
    # the record's own count stays checked where it is read: at -1, and without counts
    for counts in ([-1, -1], None):
        assert step(_records(good, (1, 0, 1.0, 3, 0, 0)), counts) == _lib.PMHIP_EINVAL and b"num_mask" in lib.pmhip_last_error()
    # ... and the filters keep their checks
    assert step(_records(good, (1, 0, 1.0, 257, 4, 0)), [0, 0]) == _lib.PMHIP_EINVAL and b"topk=257" in lib.pmhip_last_error()
    assert step(_records(good), [0], handle=None) == _lib.PMHIP_EINVAL and b"bad arguments" in lib.pmhip_last_error()
    steps = C.c_int(-1)
    assert lib.pmhip_s2_slots_edit_steps(host_handle, C.byref(steps)) == _lib.PMHIP_OK and steps.value == 0      # nothing was counted
    assert lib.pmhip_s2_slots_edit_steps(None, None) == _lib.PMHIP_EINVAL
