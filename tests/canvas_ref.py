"""Cases, restatements and bounds of the canvas operators: pmhip_window_logits and pmhip_window_pixels.

Shared by tests/test_canvas_cpu.py -- which proves that the bound rejects the named faults at exactly these inputs -- and
tests/test_gpu_canvas.py.  Not collected.

THE BOUND (derived, not tuned).  A canvas element is out = rn(w_0 x_0), then fma(w_k, x_k, out) for the n entries that cover it: n
roundings, each of a partial sum whose magnitude is at most (1 + u)^n S with S = sum |w_k x_k| and u = 2^-24.  Against the float64
sum of the same products (exact to 2^-53, nothing beside u) the error is at most n u S (1 + n u); the float64 value's own rounding to
the f32 the kernel returns adds u |ref|.  Hence B = n u S (1 + n u) + u |ref| + 2^-149.  The blend of pixels is the same chain over
the products rn(ay ax) p -- the rounded weight product is part of the rule, the restatement uses it too -- and the clamp to [-1, 1]
is 1-Lipschitz: the bound passes through it."""
import functools

import numpy as np

from paintmind_amd.canvas import canvas_layout

U = 2.0 ** -24
G, PATCH, B = 4, 8, 2                                          # the tiny pipeline's window: 4 x 4 tokens of 8 pixels; canvases per launch
VS = (64, 1000, 8192)                                          # 1000 leaves the last vector group ragged
GRIDS = ((4, 6), (7, 7), (8, 8))
STRIDES = (2, 3)
# (grid, stride, fuse) whose cover counts are in {1, 2, 4} with weights 1, 1/2, 1/4: every product and the f32 sums are exact in order
EXACT = tuple((grid, 2, "uniform") for grid in ((4, 6), (8, 8)))
# ... and those held to the bound against float64: stride 3, the 7 x 7 canvas, and every "tent"
BOUNDED = tuple((grid, s, f) for grid in GRIDS for s in STRIDES for f in ("uniform", "tent") if (grid, s, f) not in EXACT)
FAULTS = ("wrong_row", "dropped_last", "neighbour_weight", "transposed_local")


@functools.lru_cache(maxsize=None)
def layout(grid, stride, fuse="uniform", g=G, patch=PATCH):
    return canvas_layout(grid, g, stride, patch, fuse)


def power_of_two_layout(lay):
    """every weight is 1, 1/2 or 1/4 and every cover count 1, 2 or 4"""
    counts = (lay.cover >= 0).sum(1)
    return bool(np.isin(counts, (1, 2, 4)).all() and np.isin(lay.weight[lay.cover >= 0], (1.0, 0.5, 0.25)).all())


@functools.lru_cache(maxsize=None)
def random_rows(rows, V, seed):
    """window logits f32 [rows, V], logit-sized; read-only"""
    x = (np.random.default_rng(seed).standard_normal((rows, V)) * 4.0).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def probe_rows(rows, V):
    """index probes: element [r, c] holds the integer 64 r + c % 64 -- a row and a column cannot be confused with another"""
    x = (64.0 * np.arange(rows)[:, None] + (np.arange(V) % 64)[None, :]).astype(np.float32)
    assert x.max() < 2 ** 22                                   # (weights down to 1/4 and sums of four stay exact)
    x.setflags(write=False)
    return x


def faulty_tables(lay, fault):
    """the cover and weight tables with one of the named faults injected (None: as they are)"""
    cover, weight = lay.cover.copy(), lay.weight.copy()
    g2 = lay.g * lay.g
    counts = (cover >= 0).sum(1)
    if fault == "wrong_row":                                   # one source row of one token is its neighbour in the window
        t = int(np.argmax(counts))
        cover[t, 0] = cover[t, 0] + 1 if cover[t, 0] % g2 != g2 - 1 else cover[t, 0] - 1
    elif fault == "dropped_last":
        for t in np.nonzero(counts > 1)[0]:
            cover[t, counts[t] - 1] = -1
    elif fault == "neighbour_weight":
        weight = np.roll(weight, -1, axis=0)
    elif fault == "transposed_local":
        on = cover >= 0
        w, local = cover // g2, cover % g2
        cover = np.where(on, w * g2 + (local % lay.g) * lay.g + local // lay.g, -1).astype(np.int32)
    elif fault is not None:
        raise ValueError(fault)
    return cover, weight


def fuse(win, lay, dtype, fault=None, tables=None):
    """the restatement of pmhip_window_logits: win [B * Rw, V] -> [B * Nc, V], the products w_k x_k summed sequentially in ascending
    order in `dtype` (np.float32: the kernel's own chain where the products are exact; np.float64: the reference of the bound)"""
    cover, weight = faulty_tables(lay, fault) if tables is None else tables
    Rw, Nc = lay.window_rows, lay.tokens
    nb = win.shape[0] // Rw
    x = win.reshape(nb, Rw, -1).astype(dtype)
    out = np.zeros((nb, Nc, x.shape[2]), dtype)
    started = np.zeros(Nc, bool)
    for k in range(cover.shape[1]):
        on = (cover[:, k] >= 0) & (cover[:, k] < Rw)
        term = weight[:, k].astype(dtype)[None, :, None] * x[:, np.where(on, cover[:, k], 0)]
        out = np.where((on & started)[None, :, None], out + term, np.where((on & ~started)[None, :, None], term, out))
        started |= on
    return out.reshape(nb * Nc, -1)


def fuse_bound(win, lay):
    """-> (float64 reference, element-wise bound) of the fused logits"""
    ref = fuse(win, lay, np.float64)
    S = fuse(np.abs(win), lay, np.float64)
    n = np.tile((lay.cover >= 0).sum(1), win.shape[0] // lay.window_rows)[:, None].astype(np.float64)
    return ref, n * U * S * (1 + n * U) + U * np.abs(ref) + 2.0 ** -149


def worst_ratio(got, ref, bound):
    return float((np.abs(got.astype(np.float64) - ref) / bound).max())


# ---------------------------------------------------------------------------------------------------------------- pixels
# (g, grid in tokens, stride): canvases of 1 x 2 and 2 x 2 windows and one whose last window is flush against the edge
PIXEL_CASES = ((4, (4, 6), 2), (4, (6, 6), 2), (4, (4, 7), 2), (32, (32, 48), 16), (32, (48, 48), 16), (32, (32, 56), 16))


@functools.lru_cache(maxsize=None)
def window_images(g, grid, stride, channels=3, nb=1, seed=5):
    """decoded windows f32 [nb * W, C, S, S] in [-1.5, 1.5], a few exactly at +-1 and beyond (the clamp has work); read-only"""
    lay = layout(grid, stride, "uniform", g)
    S = g * PATCH
    x = np.random.default_rng(seed).uniform(-1.5, 1.5, (nb * lay.n_windows, channels, S, S)).astype(np.float32)
    x[:, :, 0, ::7], x[:, :, 1, ::5] = 1.0, -1.0
    x.setflags(write=False)
    return x


def _axis_dense(table, n):
    """(win [E, 4], w [E, 4]) -> f32 [n, E]: window j's weight at every coordinate, 0 where it does not cover"""
    win, w = table
    out = np.zeros((n, win.shape[0]), np.float32)
    for k in range(win.shape[1]):
        on = win[:, k] >= 0
        out[win[on, k], np.nonzero(on)[0]] = w[on, k]
    return out


def blend(imgs, lay, dtype, clamp=True):
    """the restatement of pmhip_window_pixels: [nb * W, C, S, S] -> [nb, C, Hc, Wc]; the weight product is rounded to f32 first, the
    terms are summed with jy ascending outside and jx ascending inside in `dtype`"""
    (Hc, Wc), S = lay.size, lay.g * lay.patch
    ny, nx = len(lay.offsets_y), len(lay.offsets_x)
    x = imgs.reshape(-1, ny, nx, imgs.shape[1], S, S)
    wy, wx = _axis_dense(lay.pixel_y, ny), _axis_dense(lay.pixel_x, nx)
    out = np.zeros((x.shape[0], x.shape[3], Hc, Wc), dtype)
    for jy, oy in enumerate(lay.pixel_off_y):
        for jx, ox in enumerate(lay.pixel_off_x):
            w = (wy[jy, oy:oy + S, None] * wx[jx, None, ox:ox + S]).astype(np.float32)       # rn(ay ax)
            out[:, :, oy:oy + S, ox:ox + S] += w.astype(dtype) * x[:, jy, jx].astype(dtype)
    return np.clip(out, -1.0, 1.0) if clamp else out


def blend_bound(imgs, lay):
    """-> (float64 reference behind the clamp, element-wise bound, bool [Hc, Wc]: the pixels one window covers)"""
    ref = blend(imgs, lay, np.float64)
    S = blend(np.abs(imgs), lay, np.float64, clamp=False)
    ny, nx = (lay.pixel_y[0] >= 0).sum(1), (lay.pixel_x[0] >= 0).sum(1)
    n = (ny[:, None] * nx[None, :]).astype(np.float64)
    return ref, n * U * S * (1 + n * U) + U * np.abs(ref) + 2.0 ** -149, n == 1


def single_window_pixels(imgs, lay):
    """f32 [nb, C, Hc, Wc]: at the pixels one window covers, that window's pixel clamped (elsewhere unspecified)"""
    return blend(imgs, lay, np.float32)
