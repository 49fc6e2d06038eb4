"""The region-preserving edit without a GPU: the schedule against its examples and invariants, the plain-torch
branch of ``Pipeline.edit`` on a CPU pipeline, every ``ValueError`` of the call, and the refusals of the five native entries before
anything is launched."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import paintmind_amd as pm
from edit_ref import schedule_np
from paintmind_amd import _lib, engine as engine_mod, ops
from paintmind_amd.generate import Pipeline, edit_schedule
from util import load_golden, to_torch_sd

NEW = ("pmhip_remask_counts", "pmhip_remask_choice_counts", "pmhip_mask_tokens", "pmhip_composite", "pmhip_pipeline_generate_edit")


@pytest.fixture(scope="module")
def pipe():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False).eval()
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not [k for k in missing.missing_keys if not k.startswith("text_model")]
    return pipe


def test_schedule_examples():
    assert edit_schedule(5, 8) == [4, 3, 2, 1, 0, 0, 0, 0]
    assert edit_schedule(37, 8) == [36, 34, 30, 26, 20, 14, 7, 0]
    assert edit_schedule(1024, 8) == [1004, 946, 851, 724, 568, 391, 199, 0]
    for m, T in ((0, 8), (1, 8), (0, 1), (1, 1), (37, 1), (1024, 1)):
        assert edit_schedule(m, T) == [0] * T, (m, T)


@pytest.mark.parametrize("T", [1, 2, 3, 8, 18])
def test_schedule_invariants(T):
    for m in list(range(41)) + [100, 1024]:
        s = edit_schedule(m, T)
        assert s == schedule_np(m, T) and len(s) == T and all(isinstance(v, int) for v in s), (m, T)
        assert s[-1] == 0, (m, T)
        assert s[0] <= max(m - 1, 0), (m, T)
        assert all(b < a for a, b in zip(s, s[1:]) if a > 0), (m, T, s)             # strictly decreasing while > 0
        assert all(b == 0 for a, b in zip(s, s[1:]) if a == 0), (m, T, s)


def _masks(pipe):
    """B = 3 token masks of 0, 5 and 16 tokens on the 4 x 4 grid, and pixel masks that light them: one pixel per token, in a
    different corner of its patch each time"""
    g, p = pipe.image_size // pipe.patch_size, pipe.patch_size
    tm = torch.zeros(3, g, g, dtype=torch.bool)
    tm[1].view(-1)[[0, 3, 6, 9, 15]] = True
    tm[2] = True
    pix = torch.zeros(3, pipe.image_size, pipe.image_size, dtype=torch.uint8)
    corners = [(0, 0), (0, p - 1), (p - 1, 0), (p - 1, p - 1)]
    for b, r, c in tm.nonzero().tolist():
        dy, dx = corners[(r + c) % 4]
        pix[b, r * p + dy, c * p + dx] = 1
    return tm, pix


@torch.no_grad()
def test_cpu_edit_keeps_what_it_was_told_to_keep(pipe):
    tm, pix = _masks(pipe)
    B, T = 3, 3
    img = torch.rand(B, 3, pipe.image_size, pipe.image_size, generator=torch.Generator().manual_seed(3)) * 2 - 1
    enc = pipe.to_latent(img)[1].reshape(B, -1)
    out, ids = pipe.edit(img, token_mask=tm, timesteps=T, topk=5, seed=7, return_ids=True)
    flat = tm.reshape(B, -1)
    assert out.shape == img.shape and ids.shape == enc.shape
    assert torch.equal(ids[~flat], enc[~flat])                                    # outside the mask: the encoded ids
    assert not bool((ids == pipe.mask_token_id).any())                            # no mask id is left
    assert int((ids[flat] != enc[flat]).sum()) > 0                                # ... and inside it something was drawn
    assert torch.equal(out[0], pipe.vqgan.decode_from_indice(enc)[0])             # the empty mask: decode(encode)
    assert torch.equal(out, pipe.vqgan.decode_from_indice(ids))                   # decoded from the final (= last merged) ids
    # the pixel mask lights the same tokens: the same call
    out_p, ids_p = pipe.edit(img, mask=pix, timesteps=T, topk=5, seed=7, return_ids=True)
    assert torch.equal(ids_p, ids) and torch.equal(out_p, out)
    for shaped in (pix[:, None], pix.float(), pix.bool()):
        assert torch.equal(pipe.edit(img, mask=shaped, timesteps=T, topk=5, seed=7), out)
    # preserve="pixels": the input, bit for bit, outside the pixel mask; the decode inside it
    keep = pipe.edit(img, mask=pix, timesteps=T, topk=5, seed=7, preserve="pixels")
    sel = (pix != 0)[:, None].expand_as(img)
    assert torch.equal(keep[~sel], img[~sel]) and torch.equal(keep[sel], out[sel])
    # with a token mask: outside the token mask's pixels
    keep_t = pipe.edit(img, token_mask=tm, timesteps=T, topk=5, seed=7, preserve="pixels")
    p = pipe.patch_size
    sel_t = tm.repeat_interleave(p, 1).repeat_interleave(p, 2)[:, None].expand_as(img)
    assert torch.equal(keep_t[~sel_t], img[~sel_t]) and torch.equal(keep_t[sel_t], out[sel_t])
    # a broadcast [g, g] / [H, W] mask is every image's
    one = pipe.edit(img, token_mask=tm[1], timesteps=T, topk=5, seed=7, return_ids=True)[1]
    assert torch.equal(one[~flat[1:2].expand(B, -1)], enc[~flat[1:2].expand(B, -1)])
    # T = 1: one step, every masked token taken at once; options pass through _options
    ids1 = pipe.edit(img, token_mask=tm, timesteps=1, topk=None, top_p=0.9, choice_temperature=4.5, seed=1, return_ids=True)[1]
    assert torch.equal(ids1[~flat], enc[~flat]) and not bool((ids1 == pipe.mask_token_id).any())
    txt = pipe.edit(img, token_mask=tm, text=["a", "b", "c"], timesteps=T, guidance_scale=[1.0, 2.0, 3.0], negative_text="blurry", seed=7,
                    return_ids=True)[1]
    assert torch.equal(txt[~flat], enc[~flat]) and not bool((txt == pipe.mask_token_id).any())


def test_argument_errors(pipe, monkeypatch):
    monkeypatch.setattr(Pipeline, "_sample_cpu", lambda *a, **k: pytest.fail("a step ran"))
    tm, pix = _masks(pipe)
    img = torch.zeros(3, 3, pipe.image_size, pipe.image_size)
    for kw, word in ((dict(), "exactly one"),
                     (dict(mask=pix, token_mask=tm), "exactly one"),
                     (dict(mask=pix[:2]), "mask must be"),
                     (dict(mask=pix[:, :-1]), "mask must be"),
                     (dict(mask=pix[:, None, None]), "mask must be"),
                     (dict(token_mask=tm[:2]), "token_mask must be"),
                     (dict(token_mask=tm.float()), "token_mask must be"),
                     (dict(token_mask=tm[:, :2]), "token_mask must be"),
                     (dict(mask=pix, preserve="both"), "preserve"),
                     (dict(mask=pix, guidance_scale=2.0), "text condition"),
                     (dict(mask=pix, negative_text="x"), "text condition"),
                     (dict(mask=pix, text=["a", "b", "c"], negative_text="x"), "needs guidance_scale"),
                     (dict(mask=pix, top_p=1.5), "top_p"),
                     (dict(mask=pix, choice_temperature=-1.0), "choice_temperature")):
        with pytest.raises(ValueError, match=word):
            pipe.edit(img, **kw)
    with pytest.raises(ValueError, match="img must be"):
        pipe.edit(img[0], mask=pix[0])
    with pytest.raises(ValueError, match="img must be"):
        pipe.edit(img[..., :16], mask=pix[..., :16])


def test_signature_and_the_reference_shaped_calls_say_what_they_are():
    sig = inspect.signature(Pipeline.edit).parameters
    assert list(sig)[1:] == ["img", "mask", "text", "timesteps", "temperature", "topk", "seed", "image_base", "token_mask", "guidance_scale",
                             "negative_text", "mask_padding", "context_lens", "choice_temperature", "top_p", "preserve", "return_ids"]
    assert (sig["timesteps"].default, sig["temperature"].default, sig["topk"].default, sig["preserve"].default) == (8, 1.0, 5, "tokens")
    for fn in (Pipeline.inpaint, Pipeline.outpaint):
        assert "region-preserving" in fn.__doc__ and "edit" not in inspect.signature(fn).parameters
    assert inspect.signature(engine_mod.S2Engine.generate).parameters["nmask_img"].default is None
    assert callable(ops.remask_counts) and callable(ops.mask_tokens) and callable(ops.composite)


def test_abi_stays_and_the_new_symbols_are_exported():
    lib = _lib.load()
    assert lib.pmhip_abi_version() == 11 == _lib.ABI_VERSION
    assert C.sizeof(_lib.Slot) == 32
    header = open(_lib._HERE + "/../include/pmhip.h").read()
    for name in NEW:
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None and f"int {name}(" in header
    assert "1 <= topk <= 8" in header and "1 <= topk <= V" in header
    P = _lib.PROTOTYPES
    assert P["pmhip_pipeline_generate_edit"][1] == P["pmhip_pipeline_generate_negative"][1]
    assert P["pmhip_remask_choice_counts"][1] == P["pmhip_remask_choice"][1][:2] + [_lib.vp] + P["pmhip_remask_choice"][1][3:]


def test_native_entries_refuse_bad_arguments_before_a_launch():
    """fake non-null pointers that are never dereferenced: a call that got past the checks would not return PMHIP_EINVAL"""
    lib = _lib.load()
    p = C.c_void_p(64)
    E = _lib.PMHIP_EINVAL

    def refused(rc, *words):
        msg = lib.pmhip_last_error().decode()
        assert rc == E and all(w in msg for w in words), (rc, msg)

    refused(lib.pmhip_remask_counts(None, p, p, 64, 2, 16, None), "remask_counts", "null")
    refused(lib.pmhip_remask_counts(p, None, p, 64, 2, 16, None), "remask_counts", "null")
    refused(lib.pmhip_remask_counts(p, p, None, 64, 2, 16, None), "remask_counts", "null")
    refused(lib.pmhip_remask_counts(p, p, p, 64, 0, 16, None), "remask_counts", "bad shape")
    refused(lib.pmhip_remask_counts(p, p, p, 64, 2, 4097, None), "remask_counts", "bad shape")
    refused(lib.pmhip_remask_choice_counts(p, p, None, 64, 2, 16, 1.0, None, 1, 0, 0, None), "remask_choice_counts", "null")
    refused(lib.pmhip_remask_choice_counts(None, p, p, 64, 2, 16, 1.0, None, 1, 0, 0, None), "remask_choice_counts", "null")
    refused(lib.pmhip_remask_choice_counts(p, p, p, 64, 2, 0, 1.0, None, 1, 0, 0, None), "remask_choice_counts", "bad shape")
    for t in (-0.5, float("nan"), float("inf"), 1000.5):
        refused(lib.pmhip_remask_choice_counts(p, p, p, 64, 2, 16, t, None, 1, 0, 0, None), "remask_choice_counts", "choice temperature")
    refused(lib.pmhip_mask_tokens(None, 8, p, 64, p, 2, 32, 32, None), "mask_tokens", "null")
    refused(lib.pmhip_mask_tokens(p, 8, None, 64, p, 2, 32, 32, None), "mask_tokens", "null")
    refused(lib.pmhip_mask_tokens(p, 8, p, 64, None, 2, 32, 32, None), "mask_tokens", "null")
    refused(lib.pmhip_mask_tokens(p, 8, p, 64, p, 2, 30, 32, None), "mask_tokens", "bad shape")
    refused(lib.pmhip_mask_tokens(p, 0, p, 64, p, 2, 32, 32, None), "mask_tokens", "bad shape")
    refused(lib.pmhip_mask_tokens(p, 8, p, 64, p, 0, 32, 32, None), "mask_tokens", "bad shape")
    for bad in range(4):
        args = [p, p, p, p]
        args[bad] = None
        refused(lib.pmhip_composite(*args, 2, 3, 32, 32, None), "composite", "null")
    refused(lib.pmhip_composite(p, p, p, p, 2, 0, 32, 32, None), "composite", "bad shape")
    refused(lib.pmhip_composite(p, p, p, p, 2, 3, 32, -1, None), "composite", "bad shape")
    fl = (C.c_float * 2)(1.0, 0.5)
    tab = (C.c_int * 6)(3, 2, 1, 0, 0, 0)
    dec = (C.c_ubyte * 2)(0, 1)

    def loop(s2, table, guided=0, gs=None):
        return lib.pmhip_pipeline_generate_edit(s2, None, p, None, 0, 3, None, 2, fl, table, dec, 3, 1, 0, None, 0, None, None, 0, None, guided, 2.0,
                                                None, 1.0, None, 0, None, gs)

    refused(loop(None, None), "pipeline_generate_edit", "null count table")
    refused(loop(None, tab), "bad arguments")                                       # no handle: refused before the table is looked at
    refused(loop(None, tab, 0, fl), "pipeline_generate_edit", "needs guidance")     # the negative entry's checks come with it
