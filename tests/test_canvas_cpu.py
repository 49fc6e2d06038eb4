"""Canvases beyond the token grid on the CPU: the layout rule and its refusals, the bound of
tests/canvas_ref.py against the named faults at the inputs tests/test_gpu_canvas.py uses, the plain-torch steps against the
restatements, the whole feature on the tiny pipeline's CPU branch, and the two new entries of the C ABI."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import canvas_ref as R
import paintmind_amd as pm
from paintmind_amd import _lib
from paintmind_amd.canvas import MAX_AXIS_COVER, MAX_COVER, axis_offsets, canvas_layout
from paintmind_amd.generate import Pipeline, edit_schedule
from paintmind_amd.steps import TorchSteps
from util import ROOT, load_golden, to_torch_sd

SMALL = [((gh, gw), 4, s) for gh in (4, 6, 7, 8) for gw in (4, 6, 7, 8) for s in (1, 2, 3, 4)]
FULL = [((gh, gw), 32, 16) for gh in (32, 48, 64) for gw in (32, 48, 64)]


# ---------------------------------------------------------------------------------------------------------------- the layout

def test_axis_offsets_follow_the_rule():
    assert axis_offsets(4, 4, 2) == [0] and axis_offsets(6, 4, 2) == [0, 2] and axis_offsets(7, 4, 2) == [0, 2, 3]
    assert axis_offsets(8, 4, 2) == [0, 2, 4] and axis_offsets(8, 4, 3) == [0, 3, 4] and axis_offsets(8, 4, 4) == [0, 4]
    assert axis_offsets(7, 4, 1) == [0, 1, 2, 3] and axis_offsets(64, 32, 16) == [0, 16, 32] and axis_offsets(48, 32, 16) == [0, 16]


@pytest.mark.parametrize("fuse", ("uniform", "tent"))
def test_layout_properties(fuse):
    for grid, g, stride in SMALL + FULL:
        lay = canvas_layout(grid, g, stride, 8, fuse)
        (Gh, Gw), what = grid, f"{grid} g={g} stride={stride} {fuse}"
        assert lay.windows == tuple(itertools.product(axis_offsets(Gh, g, stride), axis_offsets(Gw, g, stride))), what
        assert all(0 <= a and a + g <= Gh and 0 <= b and b + g <= Gw for a, b in lay.windows), what          # inside the canvas
        on = lay.cover >= 0
        counts = on.sum(1)
        assert lay.cover.shape == (Gh * Gw, lay.K) and counts.min() >= 1 and counts.max() == lay.K <= MAX_COVER, what   # every token
        # the entries come first, in ascending window order, -1 and weight 0 behind them; each names this very token
        assert all(on[t, :c].all() and not on[t, c:].any() for t, c in enumerate(counts)), what
        assert (np.diff(np.where(on, lay.cover, (1 << 30) + np.arange(lay.K)), axis=1) > 0).all() and (lay.weight[~on] == 0).all(), what
        assert (lay.gather.reshape(-1)[lay.cover[on]] == np.nonzero(on)[0]).all(), what
        assert lay.gather.shape == (len(lay.windows), g * g) and sorted(set(lay.gather.reshape(-1).tolist())) == list(range(Gh * Gw)), what
        # the f32 weights of a token sum to 1 within 4 ulp; a single cover weighs exactly 1
        assert np.abs(lay.weight.astype(np.float64).sum(1) - 1).max() <= 4 * 2.0 ** -23, what
        assert (lay.weight[counts == 1, 0] == 1).all(), what
        for (win, w), extent, offs, E in ((lay.token_y, Gh, lay.offsets_y, g), (lay.token_x, Gw, lay.offsets_x, g),
                                         (lay.pixel_y, Gh * 8, lay.pixel_off_y, g * 8), (lay.pixel_x, Gw * 8, lay.pixel_off_x, g * 8)):
            n = (win >= 0).sum(1)
            assert win.shape == (extent, MAX_AXIS_COVER) and n.min() >= 1, what                               # every pixel
            assert np.abs(w.astype(np.float64).sum(1) - 1).max() <= 4 * 2.0 ** -23 and (w[n == 1, 0] == 1).all(), what
            for c in range(extent):                            # exactly the windows whose extent holds the coordinate, ascending
                assert [j for j in win[c] if j >= 0] == [j for j, o in enumerate(offs) if o <= c < o + E], what
        assert lay.size == (Gh * 8, Gw * 8) and not lay.cover.flags.writeable and not lay.weight.flags.writeable


def test_tent_weights_are_the_rule():
    lay = canvas_layout((4, 6), 4, 2, 8, "tent")
    # column 2 is local 2 of window 0 (raw min(3, 2) = 2) and local 0 of window 1 (raw 1); column 3: raw 1 and 2
    assert lay.token_x[1][2].tolist()[:2] == [np.float32(2 / 3), np.float32(1 / 3)]
    assert lay.token_x[1][3].tolist()[:2] == [np.float32(1 / 3), np.float32(2 / 3)]
    t = 1 * 6 + 2
    assert lay.cover[t].tolist() == [0 * 16 + 1 * 4 + 2, 1 * 16 + 1 * 4 + 0] and lay.weight[t, 0] == np.float32(1) * np.float32(2 / 3)
    uni = canvas_layout((4, 6), 4, 2, 8)
    assert uni.weight[t].tolist() == [0.5, 0.5] and uni.pixel_x[1][16].tolist()[:2] == [np.float32(16 / 17), np.float32(1 / 17)]


def test_refusals_name_the_offender():
    for kwargs, word in ((dict(grid=(3, 8), g=4, stride=2), "Gh=3"), (dict(grid=(8, 2), g=4, stride=2), "Gw=2"),
                         (dict(grid=(64, 65), g=32, stride=16), "4160"), (dict(grid=(8, 8), g=4, stride=0), "stride=0"),
                         (dict(grid=(8, 8), g=4, stride=5), "stride=5"), (dict(grid=(32, 64), g=32, stride=2), "too small"),
                         (dict(grid=(64, 64), g=32, stride=4), "too small"), (dict(grid=(8, 8), g=4, stride=2, fuse="cone"), "cone")):
        with pytest.raises(ValueError, match=word):
            canvas_layout(patch=8, **kwargs)
    pipe = tiny()
    with pytest.raises(ValueError, match="multiple of patch"):
        pipe.canvas_layout((32, 50))
    with pytest.raises(ValueError, match="Gh=3"):
        pipe.canvas_layout((24, 64))


def test_half_window_strides_cover_by_one_two_or_four():
    """the exact GPU tests rest on this: it holds for the layout rule as written"""
    for grid, g, stride in [((a, b), 4, 2) for a in (4, 6, 8) for b in (4, 6, 8)] + FULL:
        lay = canvas_layout(grid, g, stride, 8)
        assert set((lay.cover >= 0).sum(1).tolist()) <= {1, 2, 4} and R.power_of_two_layout(lay), grid
    assert all(R.power_of_two_layout(R.layout(*case)) for case in R.EXACT)
    assert not any(R.power_of_two_layout(R.layout(grid, 2, "tent")) for grid in R.GRIDS) and not R.power_of_two_layout(R.layout((7, 7), 2))


# ---------------------------------------------------------------------------------------------------------------- the bound

@pytest.mark.parametrize("V", R.VS)
def test_the_bound_rejects_the_named_faults(V):
    """at the very inputs the GPU test uses: the restatement with a fault injected exceeds the bound on at least one element, and
    the restatement as it is -- one rounding per operation, no fused multiply-add -- stays within twice of it"""
    for case in R.BOUNDED:
        lay = R.layout(*case)
        win = R.random_rows(R.B * lay.window_rows, V, 1)
        ref, bound = R.fuse_bound(win, lay)
        assert R.worst_ratio(R.fuse(win, lay, np.float32), ref, bound) <= 2.0, case
        for fault in R.FAULTS:
            assert R.worst_ratio(R.fuse(win, lay, np.float32, fault), ref, bound) > 1.0, (case, fault)


def test_index_probes_are_exact_and_reject_the_faults():
    for case in R.EXACT:
        lay = R.layout(*case)
        win = R.probe_rows(R.B * lay.window_rows, 64)
        exact = R.fuse(win, lay, np.float64)
        assert np.array_equal(R.fuse(win, lay, np.float32).astype(np.float64), exact), case
        for fault in R.FAULTS:
            assert not np.array_equal(R.fuse(win, lay, np.float32, fault).astype(np.float64), exact), (case, fault)


def test_the_pixel_bound_holds_for_the_chain_and_rejects_a_shift():
    for g, grid, stride in R.PIXEL_CASES[:3]:
        lay = R.layout(grid, stride, "uniform", g)
        imgs = R.window_images(g, grid, stride)
        ref, bound, single = R.blend_bound(imgs, lay)
        assert R.worst_ratio(R.blend(imgs, lay, np.float32), ref, bound) <= 2.0 and single.any() and not single.all()
        assert np.abs(ref).max() <= 1.0
        assert R.worst_ratio(R.blend(np.roll(imgs, 1, axis=3), lay, np.float32), ref, bound) > 1.0       # a window's rows off by one


# ---------------------------------------------------------------------------------------------------------------- the torch steps

def tiny():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False).eval()
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not [k for k in missing.missing_keys if not k.startswith("text_model")]
    return pipe


@pytest.fixture(scope="module")
def pipe():
    return tiny()


def test_torch_steps_are_the_restatements(pipe):
    st = TorchSteps(pipe)
    for case in R.EXACT + R.BOUNDED:
        lay = R.layout(*case)
        win = R.random_rows(R.B * lay.window_rows, 64, 1)
        got = st.window_logits(lay, torch.from_numpy(win.copy()).reshape(-1, 16, 64), None, None).reshape(-1, 64).numpy()
        assert np.array_equal(got, R.fuse(win, lay, np.float32)), case
        un = R.random_rows(R.B * lay.window_rows, 64, 2)
        guided = st.window_logits(lay, torch.from_numpy(win.copy()).reshape(-1, 16, 64), torch.from_numpy(un.copy()).reshape(-1, 16, 64), 3.0)
        combined = st.guide(torch.from_numpy(win.copy()), torch.from_numpy(un.copy()), 3.0).numpy()
        assert np.array_equal(guided.reshape(-1, 64).numpy(), R.fuse(combined, lay, np.float32)), case
    for g, grid, stride in R.PIXEL_CASES[:3]:
        lay = R.layout(grid, stride, "uniform", g)
        imgs = R.window_images(g, grid, stride)
        ref, bound, single = R.blend_bound(imgs, lay)
        got = st.window_pixels(lay, torch.from_numpy(imgs.copy())).numpy()
        assert R.worst_ratio(got, ref, bound) <= 2.0 and np.array_equal(got[..., single], R.single_window_pixels(imgs, lay)[..., single])


# ---------------------------------------------------------------------------------------------------------------- end to end

def context(pipe, B):
    return pipe.text_model(["a wide valley", "a long wall", "a tall tower"][:B])


def test_a_canvas_equal_to_the_grid_is_the_ordinary_loop(pipe):
    """one window of weight 1: the fused logits are the window's, and the loop is ``generate``'s on the CPU branch.  (The CPU branch
    draws a batch's noise from ONE generator, a canvas call gives every canvas its own -- so that canvas j is the call with
    image_base + j -- and the two agree for one image; a batch is compared canvas by canvas.)"""
    ctx = context(pipe, 2)
    lay = pipe.canvas_layout((32, 32))
    assert lay.n_windows == 1 and lay.K == 1
    for kw in (dict(), dict(guidance_scale=2.0), dict(choice_temperature=4.5, top_p=0.9), dict(guidance_scale=[1.0, 2.0, 3.0, 4.0])):
        opts = pipe._options(5, kw.get("top_p"), kw.get("guidance_scale"), None, kw.get("choice_temperature"), ctx[:1], 1, timesteps=4)
        _, want = pipe._generate_cpu(ctx[:1], 1, 4, 1.0, opts, 2, 11, True)
        ids, merged = pipe.canvas_ids(ctx[:1], 1, lay, 4, 1.0, 5, 11, **kw)
        assert torch.equal(ids, want), kw
        assert bool((merged != pipe.mask_token_id).all()) and torch.equal(merged[ids != pipe.mask_token_id], ids[ids != pipe.mask_token_id])
    imgs, want = pipe.generate(["a wide valley"], timesteps=4, seed=11, return_ids=True)
    img, ids = pipe.generate_canvas(["a wide valley"], (32, 32), timesteps=4, seed=11, return_ids=True)
    assert torch.equal(ids, want) and img.shape == imgs[-1].shape


@pytest.mark.parametrize("size,stride", [((32, 48), 2), ((64, 64), 2), ((56, 56), 3)])
def test_canvases_are_deterministic_and_a_batch_is_its_canvases(pipe, size, stride):
    ctx = context(pipe, 3)
    lay = pipe.canvas_layout(size, stride)
    kw = dict(guidance_scale=2.0, choice_temperature=2.0)
    one = pipe.canvas_ids(ctx, 3, lay, 4, 1.0, 5, 7, image_base=2, **kw)
    two = pipe.canvas_ids(ctx, 3, lay, 4, 1.0, 5, 7, image_base=2, **kw)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    other = pipe.canvas_ids(ctx, 3, lay, 4, 1.0, 5, 8, image_base=2, **kw)
    assert not torch.equal(one[1], other[1])
    for j in range(3):
        alone = pipe.canvas_ids(ctx[j:j + 1], 1, lay, 4, 1.0, 5, 7, image_base=2 + j, **kw)
        assert torch.equal(alone[0], one[0][j:j + 1]) and torch.equal(alone[1], one[1][j:j + 1]), j
    chunked = pipe.canvas_ids(ctx, 3, lay, 4, 1.0, 5, 7, image_base=2, window_batch=2, **kw)
    assert chunked[0].shape == one[0].shape and bool((chunked[1] != pipe.mask_token_id).all())
    img = pipe.decode_canvas(one[1], lay)
    assert tuple(img.shape) == (3, 3) + size and bool(torch.isfinite(img).all()) and float(img.min()) >= -1 and float(img.max()) <= 1


def test_given_ids_are_kept_and_nothing_stays_masked(pipe):
    mask = pipe.mask_token_id
    text = ["a wide valley", "a long wall"]
    ids0 = torch.full((2, 4 * 12), mask)
    ids0.reshape(2, 4, 12)[0, :, :4] = torch.arange(16).reshape(4, 4)              # an "encoded image" at the left of a 3-wide canvas
    ids0.reshape(2, 4, 12)[1, :, 5:7] = 3
    for kw in (dict(), dict(guidance_scale=2.0, negative_text="fog", fuse="tent", choice_temperature=4.5)):
        img, ids = pipe.generate_canvas(text, (32, 96), timesteps=5, seed=1, ids0=ids0, return_ids=True, **kw)
        given = ids0 != mask
        assert torch.equal(ids[given], ids0[given]) and not bool((ids == mask).any()), kw
        assert tuple(img.shape) == (2, 3, 32, 96) and bool(torch.isfinite(img).all()) and float(img.abs().max()) <= 1
    assert ids0[0, 0] == 0 and int((ids0 == mask).sum()) == 2 * 48 - 16 - 8                                  # the caller's tensor is left alone
    assert edit_schedule(32, 5)[-1] == 0


def test_refused_calls(pipe):
    text = ["a wide valley"]
    for kw, word in ((dict(regions=[[]]), "regions"), (dict(prompt_weights=True), "prompt_weights"), (dict(context_segments=[[0]]), "context_segments"),
                     (dict(context_weights=[[1.0]]), "context_weights"), (dict(context_lens=[3]), "context_lens"), (dict(ids0=torch.zeros(1, 7, dtype=torch.long)), "ids0"),
                     (dict(ids0=torch.full((1, 24), 65)), "65"), (dict(ids0=torch.full((1, 24), -1)), "-1"),
                     (dict(ids0=torch.zeros(1, 24)), "ids0"), (dict(window_batch=0), "window_batch"), (dict(stride=5), "stride=5"),
                     (dict(fuse="cone"), "cone")):
        with pytest.raises(ValueError, match=word):
            pipe.generate_canvas(text, (32, 48), timesteps=2, **kw)
    with pytest.raises(TypeError, match="timestep"):                  # a misspelt keyword stays a TypeError
        pipe.generate_canvas(text, (32, 48), timestep=2)
    with pytest.raises(ValueError, match="guidance_scale needs a text"):
        pipe.canvas_ids(None, 1, pipe.canvas_layout((32, 48)), 2, 1.0, 5, 0, guidance_scale=2.0)
    with pytest.raises(ValueError, match="not this pipeline's"):
        pipe.canvas_ids(None, 1, canvas_layout((8, 8), 8, 4, 8), 2, 1.0, 5, 0)


# ---------------------------------------------------------------------------------------------------------------- the ABI

def test_the_two_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pmhip.h")).read()
    lib = _lib.load()
    for name, nargs in (("pmhip_window_logits", 14), ("pmhip_window_pixels", 16)):
        decl = re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]) and _lib.PROTOTYPES[name][0] is _lib.i32
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert lib.pmhip_abi_version() == _lib.ABI_VERSION == 11
    # the unserved shapes are an error code in front of any launch (dummy pointers do)
    import ctypes as C
    p, q = C.c_void_p(256), C.c_void_p(264)
    ok = dict(win=p, win_u=None, scale=0.0, ldw=64, cover=p, weight=p, K=2, window_rows=32, out=p, ldo=64, B=1, Nc=24, V=64)
    for change, word in ((dict(V=62), b"V=62"), (dict(ldw=66), b"ldw=66"), (dict(ldo=70), b"ldo=70"), (dict(ldw=60), b"ldw=60"), (dict(win=q), b"aligned"),
                         (dict(out=q), b"aligned"), (dict(win_u=q), b"aligned"), (dict(K=0), b"K=0"), (dict(K=17), b"K=17"), (dict(cover=None), b"NULL"),
                         (dict(win_u=p, scale=float("inf")), b"finite")):
        rc = lib.pmhip_window_logits(*{**ok, **change}.values(), None)
        assert rc == _lib.PMHIP_EINVAL and word in lib.pmhip_last_error(), (change, lib.pmhip_last_error())
    assert lib.pmhip_window_pixels(p, p, p, p, p, p, p, p, 1, 3, 32, 1, 2, 16, 48, None) == _lib.PMHIP_EINVAL
    assert lib.pmhip_window_pixels(p, p, p, None, p, p, p, p, 1, 3, 32, 1, 2, 32, 48, None) == _lib.PMHIP_EINVAL
