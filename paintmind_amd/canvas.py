"""Canvases beyond the token grid: the layout of overlapping model-sized windows over a larger canvas, said
once on the host.  ``canvas_layout`` returns an immutable record; the fusion of window logits (``ops.window_logits``), the blend of
decoded window pixels (``ops.window_pixels``), their plain-torch twins in ``steps.TorchSteps`` and the loop ``Pipeline.canvas_ids``
all read this record and nothing else.

THE RULE, per axis of extent G tokens under windows of g tokens: offsets 0, stride, 2 stride, ... while o + g < G, then G - g if that
is not the last offset already (G == g: [0]).  The windows are the product of the two axes, row-major.

THE WEIGHTS are separable.  On an axis a window's raw weight at local coordinate i of extent E is 1 ("uniform") or min(i + 1, E - i)
("tent"); it is normalised over the windows that cover the coordinate in float64 and rounded once to f32; a coordinate one window
covers has weight exactly 1.  Tokens: E = g on the token grid, `fuse` picks the kind.  Pixels: always "tent", E = g * patch."""
from dataclasses import dataclass
from typing import Tuple

import numpy as np

MAX_COVER = 16             # windows per canvas token (the K of pmhip_window_logits)
MAX_AXIS_COVER = 4         # windows per coordinate of one axis (the table width of pmhip_window_pixels)
MAX_TOKENS = 4096          # tokens per canvas: the re-masking kernel's limit
FUSE_KINDS = ("uniform", "tent")


def axis_offsets(G, g, stride):
    """the window offsets of one axis, by the rule above"""
    out, o = [], 0
    while o + g < G:
        out.append(o)
        o += stride
    if not out or out[-1] != G - g:
        out.append(G - g)
    return out


def axis_cover(extent, E, offsets, kind, width):
    """one axis of `extent` coordinates under windows of extent E at `offsets` -> (window index int32 [extent, width] in ascending
    order, padded with -1; weight f32 [extent, width], 0 beside a -1; the largest cover count)"""
    win = np.full((extent, width), -1, np.int32)
    wgt = np.zeros((extent, width), np.float32)
    most = 0
    for c in range(extent):
        cover = [(j, c - o) for j, o in enumerate(offsets) if o <= c < o + E]
        most = max(most, len(cover))
        if len(cover) > width:
            continue                                          # (the caller refuses the layout by `most`)
        raw = np.array([1.0 if kind == "uniform" else float(min(i + 1, E - i)) for _, i in cover], np.float64)
        w = np.ones(1, np.float32) if len(cover) == 1 else (raw / raw.sum()).astype(np.float32)
        for k, (j, _) in enumerate(cover):
            win[c, k], wgt[c, k] = j, w[k]
    return win, wgt, most


def _frozen(a):
    a.setflags(write=False)
    return a


@dataclass(frozen=True, eq=False)
class CanvasLayout:
    """grid (Gh, Gw) tokens; g tokens a window side; stride tokens; patch pixels a token side; fuse the token weights' kind.
    offsets_y / offsets_x: the axes' window offsets in tokens; windows: (oy, ox) of every window, row-major; K: the largest cover.
    cover int32 [Nc, K]: for canvas token t the rows w * g^2 + local of the windows that cover it, ascending, padded with -1;
    weight f32 [Nc, K]: f32(ay) * f32(ax) rounded to f32 (0 beside a -1).  gather int64 [W, g^2]: the canvas token under every
    window token.  token_y / token_x, pixel_y / pixel_x: the axis tables (window index on that axis int32 [extent, 4], weight f32
    [extent, 4]); pixel_off_y / pixel_off_x int32: the windows' offsets in pixels.  The arrays are read-only."""
    grid: Tuple[int, int]
    g: int
    stride: int
    patch: int
    fuse: str
    offsets_y: Tuple[int, ...]
    offsets_x: Tuple[int, ...]
    windows: Tuple[Tuple[int, int], ...]
    K: int
    cover: np.ndarray
    weight: np.ndarray
    gather: np.ndarray
    token_y: Tuple[np.ndarray, np.ndarray]
    token_x: Tuple[np.ndarray, np.ndarray]
    pixel_y: Tuple[np.ndarray, np.ndarray]
    pixel_x: Tuple[np.ndarray, np.ndarray]
    pixel_off_y: np.ndarray
    pixel_off_x: np.ndarray

    @property
    def tokens(self):
        return self.grid[0] * self.grid[1]

    @property
    def n_windows(self):
        return len(self.windows)

    @property
    def window_rows(self):
        """rows of window logits per canvas: W * g^2"""
        return len(self.windows) * self.g * self.g

    @property
    def size(self):
        """(H, W) of the canvas in pixels"""
        return self.grid[0] * self.patch, self.grid[1] * self.patch


def canvas_layout(grid, g, stride, patch, fuse="uniform"):
    """the layout of a canvas of grid = (Gh, Gw) tokens under g x g-token windows `stride` tokens apart -> ``CanvasLayout``.
    ValueError, naming the offender: an axis below g, more than 4096 tokens, a stride outside 1..g, a token under more than 16
    windows or a coordinate of one axis under more than 4 ("stride too small"), an unknown `fuse`."""
    Gh, Gw = (int(v) for v in grid)
    g, stride, patch = int(g), int(stride), int(patch)
    if g < 1 or patch < 1:
        raise ValueError(f"canvas_layout: g={g} and patch={patch} must be positive")
    if fuse not in FUSE_KINDS:
        raise ValueError(f"canvas_layout: fuse {fuse!r} is neither 'uniform' nor 'tent'")
    for name, G in (("Gh", Gh), ("Gw", Gw)):
        if G < g:
            raise ValueError(f"canvas_layout: {name}={G} tokens is below the model's grid g={g}")
    if Gh * Gw > MAX_TOKENS:
        raise ValueError(f"canvas_layout: Gh * Gw = {Gh * Gw} tokens is above {MAX_TOKENS}, the re-masking kernel's limit")
    if not 1 <= stride <= g:
        raise ValueError(f"canvas_layout: stride={stride} must be in 1..g={g}")
    oy, ox = axis_offsets(Gh, g, stride), axis_offsets(Gw, g, stride)
    ty, tx = axis_cover(Gh, g, oy, fuse, MAX_AXIS_COVER), axis_cover(Gw, g, ox, fuse, MAX_AXIS_COVER)
    if max(ty[2], tx[2]) > MAX_AXIS_COVER or ty[2] * tx[2] > MAX_COVER:
        raise ValueError(f"canvas_layout: stride={stride} too small: a token is covered by {ty[2]} x {tx[2]} windows (at most {MAX_AXIS_COVER} "
                         f"per axis, {MAX_COVER} in all)")
    py = axis_cover(Gh * patch, g * patch, [o * patch for o in oy], "tent", MAX_AXIS_COVER)
    px = axis_cover(Gw * patch, g * patch, [o * patch for o in ox], "tent", MAX_AXIS_COVER)
    K, nx = ty[2] * tx[2], len(ox)
    cover = np.full((Gh * Gw, K), -1, np.int32)
    weight = np.zeros((Gh * Gw, K), np.float32)
    for y in range(Gh):
        for x in range(Gw):
            k = 0
            for a in range(MAX_AXIS_COVER):
                for b in range(MAX_AXIS_COVER):
                    jy, jx = int(ty[0][y, a]), int(tx[0][x, b])
                    if jy < 0 or jx < 0:
                        continue
                    cover[y * Gw + x, k] = (jy * nx + jx) * g * g + (y - oy[jy]) * g + (x - ox[jx])
                    weight[y * Gw + x, k] = np.float32(ty[1][y, a]) * np.float32(tx[1][x, b])
                    k += 1
    windows = tuple((a, b) for a in oy for b in ox)
    local = np.arange(g)
    gather = np.stack([((a + local)[:, None] * Gw + (b + local)[None, :]).reshape(-1) for a, b in windows]).astype(np.int64)
    return CanvasLayout((Gh, Gw), g, stride, patch, fuse, tuple(oy), tuple(ox), windows, K, _frozen(cover), _frozen(weight), _frozen(gather),
                        (_frozen(ty[0]), _frozen(ty[1])), (_frozen(tx[0]), _frozen(tx[1])), (_frozen(py[0]), _frozen(py[1])),
                        (_frozen(px[0]), _frozen(px[1])), _frozen(np.array([o * patch for o in oy], np.int32)),
                        _frozen(np.array([o * patch for o in ox], np.int32)))


def canvas_grid(size, patch):
    """a canvas size (H, W) in pixels -> (Gh, Gw) tokens; ValueError for a size that is no multiple of `patch`"""
    H, W = (int(v) for v in size)
    if H < 1 or W < 1 or H % patch or W % patch:
        raise ValueError(f"canvas size {H} x {W} pixels must be a positive multiple of patch={patch} on both axes")
    return H // patch, W // patch
