"""Canvases beyond the token grid on the GPU.

pmhip_window_logits at V in {64, 1000, 8192} on the 4 x 6, 7 x 7 and 8 x 8-token canvases of the tiny window (g = 4) at strides 2 and 3,
B = 2, row strides V + 8 with NaN in the padding, every buffer inside guard bands (tests/abi_frames.py); pmhip_window_pixels at S = 32 and
S = 256; then ``Pipeline.canvas_ids`` / ``decode_canvas`` / ``generate_canvas`` on the tiny pipeline in both compute dtypes.  Cases,
restatements and the derived bound are those of tests/canvas_ref.py; tests/test_canvas_cpu.py proves on the CPU that the bound rejects
the named faults at exactly these inputs, and that the half-window layouts cover by 1, 2 or 4 -- where every product and partial sum
is exact and the kernel must equal the sequential f32 restatement bit for bit."""
import numpy as np
import pytest
import torch

import canvas_ref as R
import paintmind_amd as pm
from abi_frames import bits, call, framed
from gpu_common import dev, n, t
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline, edit_schedule, loop_schedule
from util import load_golden, to_torch_sd

pytestmark = pytest.mark.gpu
F32, I32 = torch.float32, torch.int32
VS = pytest.mark.parametrize("V", R.VS)
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


def launch(lay, win, un=None, scale=0.0, tables=None, nb=R.B):
    """the C entry on framed buffers -> the canvas logits [nb * Nc, V]; asserts the memory contract: the inputs as they were, nothing
    outside the output's extents written"""
    rows, V = win.shape
    cover, weight = (lay.cover, lay.weight) if tables is None else tables
    Nc, K = cover.shape
    fw = framed(rows, V, ld=V + 8, dtype=F32, payload=t(np.array(win)), fill="nan")
    fu = None if un is None else framed(rows, V, ld=V + 8, dtype=F32, payload=t(np.array(un)), fill="nan")
    fc = framed(Nc, K, ld=K, dtype=I32, payload=t(np.array(cover)))
    fk = framed(Nc, K, ld=K, dtype=F32, payload=t(np.array(weight)), fill="nan")
    out = framed(nb * Nc, V, ld=V + 8, dtype=F32, device=dev())
    call("pmhip_window_logits", fw, fu, float(scale), V + 8, fc, fk, K, lay.window_rows, out, V + 8, nb, Nc, V)
    torch.cuda.synchronize()
    for f, x, name in ((fw, win, "win"), (fu, un, "win_u"), (fc, cover, "cover"), (fk, weight, "weight")):
        if f is not None:
            f.assert_frame_untouched(name)
            assert np.array_equal(n(f.payload()), x, equal_nan=True), f"{name} was written"
    out.assert_frame_untouched("out")
    return n(out.payload())


# ------------------------------------------------------------------------------------------------------------- window logits

@VS
def test_index_probes_are_exact(V):
    """element [r, c] holds 64 r + c % 64: on the power-of-two layouts the result is exact, and a wrong index cannot produce it"""
    for case in R.EXACT + (((8, 8), 4, "uniform"),):
        lay = R.layout(*case)
        win = R.probe_rows(R.B * lay.window_rows, V)
        assert same_bits(launch(lay, win), R.fuse(win, lay, np.float32)), case


@VS
def test_random_rows_exact_layouts_are_the_sequential_sum_bit_for_bit(V):
    for case in R.EXACT:
        lay = R.layout(*case)
        win = R.random_rows(R.B * lay.window_rows, V, 1)
        assert same_bits(launch(lay, win), R.fuse(win, lay, np.float32)), case


@VS
def test_random_rows_hold_the_bound(V):
    worst = 0.0
    for case in R.BOUNDED:
        lay = R.layout(*case)
        win = R.random_rows(R.B * lay.window_rows, V, 1)
        ref, bound = R.fuse_bound(win, lay)
        ratio = R.worst_ratio(launch(lay, win), ref, bound)
        print(f"V={V} {case}: worst err / bound {ratio:.4f}")
        worst = max(worst, ratio)
        assert ratio <= 1.0, case
    print(f"V={V}: the window-logits kernel's worst err / bound {worst:.4f}")


@VS
def test_a_layout_without_overlap_is_an_exact_gather(V):
    lay = R.layout((8, 8), 4, "uniform")
    assert lay.K == 1 and lay.n_windows == 4
    win = R.random_rows(R.B * lay.window_rows, V, 3)
    got = launch(lay, win).reshape(R.B, lay.tokens, V)
    assert same_bits(got, win.reshape(R.B, lay.window_rows, V)[:, lay.cover[:, 0]])


def test_nan_stays_where_the_cover_puts_it():
    lay, V = R.layout((8, 8), 2, "uniform"), 64
    win = np.array(R.random_rows(R.B * lay.window_rows, V, 1))
    r = 1 * lay.window_rows + 4 * 16 + 5                      # canvas 1, window 4, local 5
    win[r] = np.nan
    got = launch(lay, win).reshape(R.B, lay.tokens, V)
    names = (lay.cover == 4 * 16 + 5).any(1)
    assert names.sum() == 1 and np.isnan(got[1, names]).all() and not np.isnan(got[1, ~names]).any() and not np.isnan(got[0]).any()
    # entries outside [0, W g^2) are skipped in front of the load, whatever stands beside them: -1, the first row past the end, far out
    cover, weight = lay.cover.copy(), lay.weight.copy()
    off = cover < 0
    weight[off] = np.nan
    cover[off] = np.resize(np.array([-1, lay.window_rows, 1 << 30, -(1 << 31), -7], np.int32), int(off.sum()))
    clean = np.array(R.random_rows(R.B * lay.window_rows, V, 1))
    assert off.any() and same_bits(launch(lay, clean, tables=(cover, weight)), launch(lay, clean))
    # a canvas row without a valid entry is written as 0
    cover[5], weight[5] = -1, np.nan
    got = launch(lay, clean, tables=(cover, weight)).reshape(R.B, lay.tokens, V)
    assert (got[:, 5] == 0).all() and not np.isnan(got).any()


@VS
def test_the_guided_form_is_the_combine_and_the_plain_form(V):
    for case in (((8, 8), 2, "uniform"), ((7, 7), 3, "tent")):
        lay = R.layout(*case)
        win, un = R.random_rows(R.B * lay.window_rows, V, 1), R.random_rows(R.B * lay.window_rows, V, 2)
        for scale in (3.0, -0.75):
            combined = n(ops.guidance_combine(t(np.array(win)), t(np.array(un)), scale))
            guided = launch(lay, win, un=un, scale=scale)
            assert same_bits(guided, launch(lay, combined)), (case, scale)
            assert same_bits(guided, launch(lay, win, un=un, scale=scale)), "two launches differ"


def test_the_operator_and_its_refusals():
    lay, V = R.layout((7, 7), 2, "tent"), 1000
    win, un = R.random_rows(R.B * lay.window_rows, V, 1), R.random_rows(R.B * lay.window_rows, V, 2)
    tables = ops.canvas_tables(lay, dev())
    assert ops.canvas_tables(lay, dev()) is tables
    got = ops.window_logits(t(np.array(win)), tables.cover, tables.weight, lay.window_rows)
    assert same_bits(n(got), launch(lay, win))
    wide = torch.full((R.B * lay.tokens, V + 24), 7.0, device=dev())
    got = ops.window_logits(t(np.array(win)), tables.cover, tables.weight, lay.window_rows, uncond=t(np.array(un)), scale=2.0, out=wide[:, 8:8 + V])
    assert same_bits(n(got), launch(lay, win, un=un, scale=2.0)) and bool((wide[:, :8] == 7).all()) and bool((wide[:, 8 + V:] == 7).all())
    x = t(np.array(win))
    for bad in (lambda: ops.window_logits(x[:, :998], tables.cover, tables.weight, lay.window_rows),          # V % 4
                lambda: ops.window_logits(x[:, 1:997], tables.cover, tables.weight, lay.window_rows),         # a base off 16 bytes
                lambda: ops.window_logits(x[:-1], tables.cover, tables.weight, lay.window_rows),              # no whole canvas
                lambda: ops.window_logits(x, tables.cover, tables.weight, lay.window_rows, uncond=x),         # uncond without scale
                lambda: ops.window_logits(x, tables.cover.long(), tables.weight, lay.window_rows),
                lambda: ops.window_logits(x.cpu(), tables.cover.cpu(), tables.weight.cpu(), lay.window_rows)):
        with pytest.raises((ValueError, _lib.PmhipError)):
            bad()
    # the entry itself answers the unserved shapes with the error code: V % 4, a row stride % 4, a base off 16 bytes
    rows = R.B * lay.window_rows
    buf, out = torch.zeros(rows + 1, 1008, device=dev()), torch.zeros(R.B * lay.tokens + 1, 1008, device=dev())
    for args in ((buf, None, 0.0, 1008, tables.cover, tables.weight, lay.K, lay.window_rows, out, 1008, R.B, lay.tokens, 998),
                 (buf, None, 0.0, 1006, tables.cover, tables.weight, lay.K, lay.window_rows, out, 1008, R.B, lay.tokens, 1000),
                 (buf, None, 0.0, 1008, tables.cover, tables.weight, lay.K, lay.window_rows, out, 1004 + 2, R.B, lay.tokens, 1000),
                 (buf.reshape(-1)[1:], None, 0.0, 1008, tables.cover, tables.weight, lay.K, lay.window_rows, out, 1008, R.B, lay.tokens, 1000),
                 (buf, buf.reshape(-1)[2:], 1.0, 1008, tables.cover, tables.weight, lay.K, lay.window_rows, out, 1008, R.B, lay.tokens, 1000)):
        with pytest.raises(_lib.PmhipError) as e:
            call("pmhip_window_logits", *args)
        assert e.value.code == _lib.PMHIP_EINVAL
    torch.cuda.synchronize()
    assert not bool(out.any())


def test_full_size_is_the_sequential_sum_bit_for_bit():
    """g = 32, a 32 x 48-token canvas at stride 16, V = 8192, B = 1, uniform: two windows, 2048 rows of window logits"""
    lay = R.layout((32, 48), 16, "uniform", 32)
    assert lay.n_windows == 2 and R.power_of_two_layout(lay)
    win = np.random.default_rng(9).standard_normal((lay.window_rows, 8192), dtype=np.float32) * np.float32(4)
    tables = ops.canvas_tables(lay, dev())
    x = t(win)
    got = ops.window_logits(x, tables.cover, tables.weight, lay.window_rows)
    again = ops.window_logits(x, tables.cover, tables.weight, lay.window_rows)
    assert torch.equal(bits(got), bits(again)) and torch.equal(bits(x), bits(t(win)))
    assert same_bits(n(got), R.fuse(win, lay, np.float32))


# ------------------------------------------------------------------------------------------------------------- window pixels

@pytest.mark.parametrize("g,grid,stride", R.PIXEL_CASES)
def test_window_pixels_hold_the_bound_and_copy_single_covers(g, grid, stride):
    lay = R.layout(grid, stride, "uniform", g)
    imgs = R.window_images(g, grid, stride)
    nwin, C, S, _ = imgs.shape
    (Hc, Wc), tb = lay.size, ops.canvas_tables(lay, dev())
    fi = framed(nwin * C * S, S, ld=S, dtype=F32, payload=t(np.array(imgs)).reshape(-1, S), fill="nan")
    out = framed(C * Hc, Wc, ld=Wc, dtype=F32, device=dev())
    call("pmhip_window_pixels", fi, tb.ywin, tb.yw, tb.xwin, tb.xw, tb.yoff, tb.xoff, out, 1, C, S, len(lay.offsets_y), len(lay.offsets_x), Hc, Wc)
    torch.cuda.synchronize()
    fi.assert_frame_untouched("img")
    out.assert_frame_untouched("out")
    assert np.array_equal(n(fi.payload()).reshape(imgs.shape), imgs)
    got = n(out.payload()).reshape(1, C, Hc, Wc)
    ref, bound, single = R.blend_bound(imgs, lay)
    ratio = R.worst_ratio(got, ref, bound)
    print(f"S={S} canvas {Hc} x {Wc}: worst err / bound {ratio:.4f}")
    assert ratio <= 1.0 and single.any() and not single.all()
    assert same_bits(got[..., single], R.single_window_pixels(imgs, lay)[..., single])
    assert got.min() == -1.0 and got.max() == 1.0                     # inputs at and beyond +-1: clamped, like unpatchify_clamp
    via = ops.window_pixels(t(np.array(imgs)), tb)
    assert same_bits(n(via), got)


# ------------------------------------------------------------------------------------------------------------- the loop

@pytest.fixture(scope="module")
def tiny_pipe():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False)
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("text_model") for k in missing.missing_keys)
    return pipe.eval().to(dev())


class Mode:
    def __init__(self, pipe, dtype):
        self.pipe, self.dtype = pipe, dtype

    def __enter__(self):
        self.pipe.set_compute_dtype(self.dtype)

    def __exit__(self, *exc):
        self.pipe.set_compute_dtype(torch.float32)


def context(pipe, B):
    return pipe.text_model(["a wide valley", "a long wall", "a tall tower"][:B]).to(dev())


@DTYPES
def test_a_canvas_equal_to_the_grid_is_generate_ids(tiny_pipe, dtype):
    pipe, T = tiny_pipe, 4
    ctx = context(pipe, 2)
    lay = pipe.canvas_layout((32, 32))
    with Mode(pipe, dtype):
        for kw in (dict(), dict(guidance_scale=2.0), dict(choice_temperature=4.5, top_p=0.9), dict(guidance_scale=[1.0, 2.0, 3.0, 4.0])):
            want, _ = pipe.generate_ids(ctx, 2, T, 1.0, 5, [False] * T, 11, image_base=3, use_graph=False, streams=1, **kw)
            ids, merged = pipe.canvas_ids(ctx, 2, lay, T, 1.0, 5, 11, image_base=3, **kw)
            assert torch.equal(ids, want), kw
            assert bool((merged != pipe.mask_token_id).all())
        want, _ = pipe.generate_ids(None, 2, T, 1.0, 5, [False] * T, 11, use_graph=False, streams=1)
        assert torch.equal(pipe.canvas_ids(None, 2, lay, T, 1.0, 5, 11)[0], want)


def side_loop(pipe, ctx, B, lay, T, seed, image_base, scale, ids0):
    """the canvas loop written from the public operators, the numpy fusion (bit-exact on the power-of-two layouts) in the kernel's place"""
    mask, Nc, W = pipe.mask_token_id, lay.tokens, lay.n_windows
    temps, nmask, _ = loop_schedule(T, 1.0, Nc)
    gather = t(np.array(lay.gather))
    ids = torch.full((B, Nc), mask, dtype=torch.long, device=dev()) if ids0 is None else ids0.to(dev()).clone()
    counts = None if ids0 is None else [edit_schedule(m, T) for m in (ids0 == mask).sum(1).tolist()]
    ctx_w = ctx.repeat_interleave(W, 0)
    for step in range(T):
        tok = pipe.ids2tokens(ids[:, gather].reshape(B * W, -1))
        logits = pipe.tokens2logits(tok, ctx_w)
        if scale is not None:
            logits = ops.guidance_combine(logits, pipe.tokens2logits(tok, None), scale)
        fused = t(R.fuse(n(logits).reshape(-1, logits.shape[-1]), lay, np.float32))
        _, merged, score = ops.sample_rows(fused, ids.reshape(-1), mask, 5, temps[step], seed=seed, step=step, row_base=image_base * Nc)
        last = merged.reshape(B, Nc).clone()
        if counts is None:
            ids = ops.remask(merged.reshape(B, Nc), score.reshape(B, Nc), nmask[step], mask)
        else:
            ids = ops.remask_counts(merged.reshape(B, Nc), score.reshape(B, Nc), torch.tensor([c[step] for c in counts], dtype=I32, device=dev()), mask)
    return ids, last



def start_ids(pipe, lay):
    """two canvases with given ids: a block at the left of the first, a column in the second"""
    Gh, Gw = lay.grid
    ids0 = torch.full((2, Gh, Gw), pipe.mask_token_id)
    ids0[0, :4, :4] = torch.arange(16).reshape(4, 4)
    ids0[1, :, Gw - 2] = 3
    return ids0.reshape(2, -1)


@DTYPES
@pytest.mark.parametrize("size", [(32, 48), (64, 64)])
def test_the_flow_is_the_loop_of_public_operators(tiny_pipe, dtype, size):
    pipe, T = tiny_pipe, 4
    ctx = context(pipe, 2)
    lay = pipe.canvas_layout(size, 2)
    assert R.power_of_two_layout(lay)
    with Mode(pipe, dtype):
        for scale in (None, 2.5):
            for ids0 in (None, start_ids(pipe, lay)):
                got = pipe.canvas_ids(ctx, 2, lay, T, 1.0, 5, 21, image_base=1, guidance_scale=scale, ids0=ids0)
                want = side_loop(pipe, ctx, 2, lay, T, 21, 1, scale, ids0)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (scale, ids0 is not None)
                assert bool((got[1] != pipe.mask_token_id).all())
                if ids0 is not None:
                    given = (ids0 != pipe.mask_token_id).to(dev())
                    assert torch.equal(got[0][given], ids0.to(dev())[given]) and not bool((got[0] == pipe.mask_token_id).any())


@DTYPES
def test_canvases_are_deterministic_and_a_batch_is_its_canvases(tiny_pipe, dtype):
    pipe = tiny_pipe
    ctx = context(pipe, 3)
    with Mode(pipe, dtype):
        for size, stride, fuse in (((32, 48), 2, "uniform"), ((64, 64), 2, "tent"), ((56, 56), 3, "uniform")):
            lay = pipe.canvas_layout(size, stride, fuse)
            kw = dict(guidance_scale=2.0, choice_temperature=2.0)
            one = pipe.canvas_ids(ctx, 3, lay, 4, 1.0, 5, 7, image_base=2, **kw)
            two = pipe.canvas_ids(ctx, 3, lay, 4, 1.0, 5, 7, image_base=2, **kw)
            assert all(torch.equal(a, b) for a, b in zip(one, two)), size
            for j in range(3):
                alone = pipe.canvas_ids(ctx[j:j + 1], 1, lay, 4, 1.0, 5, 7, image_base=2 + j, **kw)
                assert torch.equal(alone[0], one[0][j:j + 1]) and torch.equal(alone[1], one[1][j:j + 1]), (size, j)
            chunked = pipe.canvas_ids(ctx, 3, lay, 4, 1.0, 5, 7, image_base=2, window_batch=4, **kw)
            assert chunked[0].shape == one[0].shape and bool((chunked[1] != pipe.mask_token_id).all())


@DTYPES
def test_generate_canvas_and_decode_canvas(tiny_pipe, dtype):
    pipe = tiny_pipe
    text = ["a wide valley", "a long wall"]
    with Mode(pipe, dtype):
        lay = pipe.canvas_layout((32, 96))
        ids0 = start_ids(pipe, lay)
        img, ids = pipe.generate_canvas(text, (32, 96), timesteps=5, seed=1, ids0=ids0, return_ids=True, guidance_scale=2.0, negative_text="fog")
        given = (ids0 != pipe.mask_token_id).to(dev())
        assert torch.equal(ids[given], ids0.to(dev())[given]) and not bool((ids == pipe.mask_token_id).any())
        assert tuple(img.shape) == (2, 3, 32, 96) and img.is_cuda and bool(torch.isfinite(img).all()) and float(img.abs().max()) <= 1
        # the decode: every window decoded on its own, blended by the restated rule
        again = pipe.decode_canvas(ids, lay)
        assert torch.equal(bits(again), bits(img))
        wins = pipe.vqgan.decode_from_indice(ids[:, t(np.array(lay.gather))].reshape(2 * lay.n_windows, -1))
        ref, bound, single = R.blend_bound(n(wins), lay)
        ratio = R.worst_ratio(n(img), ref, bound)
        print(f"decode_canvas {dtype}: worst err / bound {ratio:.4f}")
        assert ratio <= 1.0 and same_bits(n(img)[..., single], R.single_window_pixels(n(wins), lay)[..., single])
        img2 = pipe.generate_canvas(text, (64, 64), timesteps=3, seed=2, fuse="tent", mask_padding=True)
        assert tuple(img2.shape) == (2, 3, 64, 64) and bool(torch.isfinite(img2).all()) and float(img2.abs().max()) <= 1
