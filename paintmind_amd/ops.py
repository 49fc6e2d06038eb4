"""Operator-level host wrappers: torch tensors in, torch tensors out, compute in libpaintmind_hip.so.

PyTorch is plumbing here (device memory from its caching allocator, the current HIP stream).  Every
function asserts its operands live on a ROCm device; nothing falls back to ATen.
"""
import ctypes as C
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import BF16, F32, PART_K, PART_Q, PART_V, check

_TORCH2PM = {torch.float32: F32, torch.bfloat16: BF16}


def pm_dtype(dt):
    try:
        return _TORCH2PM[dt]
    except KeyError:
        raise TypeError(f"paintmind_amd computes in float32 or bfloat16, not {dt}") from None


def _dev(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.PmhipError(
                "paintmind_amd runs only on a ROCm device (got a CPU tensor); there is no CPU fallback")
        if not t.is_contiguous():
            raise ValueError("paintmind_amd ops need contiguous tensors")
        dev = t.device if dev is None else dev
        if t.device != dev:
            raise ValueError("operands live on different devices")
    return dev


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def round_up(v, m):
    return (v + m - 1) // m * m


def host_lens(lens, B, L, what="context_lens"):
    """per-image lengths (a list, a CPU tensor or a device tensor; None passes through) -> a list of B ints on the host, each in
    [1, L]: brought to the host ONCE per call, checked before anything is launched"""
    if lens is None:
        return None
    vals = lens.detach().reshape(-1).tolist() if isinstance(lens, torch.Tensor) else list(lens)
    if len(vals) != B:
        raise ValueError(f"{what}: {len(vals)} lengths for a batch of {B}")
    out = []
    for b, v in enumerate(vals):
        if int(v) != v or not 1 <= int(v) <= L:
            raise ValueError(f"{what}: image {b}: length {v} must be an integer in [1, {L}]")
        out.append(int(v))
    return out


def host_control(row_map, blend, gain, B, L):
    """cross-attention control: row_map [B, L] ints (the source row of every edited row, negative: none), blend
    [B, L] in [0, 1] and gain [B, L] finite and >= 0, as lists, numpy arrays, CPU or device tensors -> contiguous numpy (int32,
    float32, float32) on the host, brought there ONCE per call and checked before anything is launched"""
    to_np = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    rm, bl, gn = to_np(row_map), to_np(blend), to_np(gain)
    if rm.shape != (B, L) or rm.dtype.kind not in "iu":
        raise ValueError(f"row_map must be integers of shape ({B}, {L}), got {rm.dtype} {rm.shape}")
    for name, x in (("blend", bl), ("gain", gn)):
        if x.shape != (B, L) or x.dtype.kind not in "fiu":
            raise ValueError(f"{name} must be numbers of shape ({B}, {L}), got {x.dtype} {x.shape}")
    bl, gn = bl.astype(np.float32), gn.astype(np.float32)
    if rm.size and rm.max() >= L:
        raise ValueError(f"row_map: source row {int(rm.max())} must be below L={L} (negative: none)")
    if not ((bl >= 0) & (bl <= 1)).all():
        raise ValueError("blend must be in [0, 1]")
    if not (np.isfinite(gn) & (gn >= 0)).all():
        raise ValueError("gain must be finite and >= 0")
    return np.ascontiguousarray(np.maximum(rm, -1).astype(np.int32)), np.ascontiguousarray(bl), np.ascontiguousarray(gn)


def host_phrase_weights(score_weights, B, L):
    """the local blend's phrase rows: (w_src, w_edit), each [B, L] numbers, finite and >= 0, as lists, numpy
    arrays, CPU or device tensors -> two contiguous numpy float32 arrays on the host, brought there ONCE per call and checked before
    anything is launched.  (That every pair has a positive weight below its length is the native entry's and the model's check: it
    needs the lengths.)"""
    if not (isinstance(score_weights, (tuple, list)) and len(score_weights) == 2):
        raise ValueError("score_weights must be the pair (w_src, w_edit)")
    out = []
    for name, x in zip(("w_src", "w_edit"), score_weights):
        w = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        if w.shape != (B, L) or w.dtype.kind not in "fiub":
            raise ValueError(f"{name} must be numbers of shape ({B}, {L}), got {w.dtype} {w.shape}")
        w = np.ascontiguousarray(w.astype(np.float32))
        if not (np.isfinite(w) & (w >= 0)).all():
            raise ValueError(f"{name} must be finite and >= 0")
        out.append(w)
    return out[0], out[1]


def check_phrase_rows(w_src, w_edit, lens, B, L):
    """every pair looks at something: a positive weight below its length in at least one half (lens: the 2B checked lengths, the
    source half in front, or None: every row) -- the rule of pmhip_s2_forward_control_scores"""
    for b in range(B):
        ns, nt = (L, L) if lens is None else (lens[b], lens[B + b])
        if not ((w_src[b, :ns] > 0).any() or (w_edit[b, :nt] > 0).any()):
            raise ValueError(f"score_weights: pair {b}: no row of the phrase has a positive weight below its length in either half")


def host_segments(context_segments, token_segments, B, L, N):
    """regional prompts: context_segments [B, L] ints (the segment 0..31 of every context row; -1 or 255 =
    padding) and token_segments [B, N] int bitmasks (bit s = the token attends to segment s), as lists, numpy arrays, CPU or device
    tensors; both None pass through as None.  -> (numpy uint8 [B, L] with 255 for padding, numpy uint32 [B, N]) on the host, brought
    there ONCE per call and checked before anything is launched: ids in range, every token allows a segment present in its image."""
    if context_segments is None and token_segments is None:
        return None
    if context_segments is None or token_segments is None:
        raise ValueError("context_segments and token_segments come together")
    to_np = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    cs, ts = to_np(context_segments), to_np(token_segments)
    if cs.shape != (B, L) or cs.dtype.kind not in "iu":
        raise ValueError(f"context_segments must be integers of shape ({B}, {L}), got {cs.dtype} {cs.shape}")
    if ts.shape != (B, N) or ts.dtype.kind not in "iu":
        raise ValueError(f"token_segments must be integer bitmasks of shape ({B}, {N}), got {ts.dtype} {ts.shape}")
    cs, ts = cs.astype(np.int64), ts.astype(np.int64)
    cs = np.where(cs == -1, 255, cs)
    bad = np.argwhere(((cs < 0) | (cs > 31)) & (cs != 255))
    if len(bad):
        b, k = bad[0]
        raise ValueError(f"context_segments: image {b}: context row {k}: segment {int(cs[b, k])} must be in 0..31, or -1 / 255 for padding")
    bad = np.argwhere((ts < 0) | (ts >= 2 ** 32))
    if len(bad):
        b, t = bad[0]
        raise ValueError(f"token_segments: image {b}: token {t}: mask {int(ts[b, t])} must be a 32-bit mask")
    present = np.zeros(B, np.int64)
    for b in range(B):
        present[b] = np.bitwise_or.reduce(np.int64(1) << cs[b][cs[b] < 32]) if (cs[b] < 32).any() else 0
    bad = np.argwhere((ts & present[:, None]) == 0)
    if len(bad):
        b, t = bad[0]
        raise ValueError(f"token_segments: image {b}: token {t} allows no segment that is present in its context "
                         f"(mask {int(ts[b, t]):#x}, present {int(present[b]):#x})")
    return np.ascontiguousarray(cs.astype(np.uint8)), np.ascontiguousarray(ts.astype(np.uint32))


W_MIN, W_MAX = 2.0 ** -20, 2.0 ** 20      # the range of a non-zero prompt weight (include/pmhip.h, PROMPT WEIGHTS)


def host_weights(context_weights, B, L, N, context_segments=None, token_segments=None, context_lens=None):
    """prompt weights: context_weights [B, L] (the weight >= 0 of every context row; 0 = the row is padding),
    as a list, a numpy array, a CPU or a device tensor; None passes through as None.  Beside it the pair of segment arrays
    (``host_segments``), or per-image lengths (``host_lens``), or nothing: without segment arrays the NEUTRAL ones are built here --
    segment 0 for the rows below the image's length, 255 behind, every token mask all ones.
    -> (numpy uint8 [B, L], numpy uint32 [B, N], numpy float32 [B, L]) on the host, brought there ONCE per call and checked before
    anything is launched: every weight finite and 0 or in [2^-20, 2^20], every token allows a row with a weight above 0."""
    if context_weights is None:
        return None
    w = context_weights.detach().cpu().numpy() if isinstance(context_weights, torch.Tensor) else np.asarray(context_weights)
    if w.shape != (B, L) or w.dtype.kind not in "fiu":
        raise ValueError(f"context_weights must be numbers of shape ({B}, {L}), got {w.dtype} {w.shape}")
    w = np.ascontiguousarray(w.astype(np.float32))
    bad = np.argwhere(~(np.isfinite(w) & ((w == 0) | ((w >= W_MIN) & (w <= W_MAX)))))
    if len(bad):
        b, k = bad[0]
        raise ValueError(f"context_weights: image {b}: context row {k}: weight {float(w[b, k])!r} must be 0 or in [2^-20, 2^20]")
    if context_segments is not None or token_segments is not None:
        if context_lens is not None:
            raise ValueError("context_segments and context_lens exclude each other (mark padding rows with segment 255)")
        cs, ts = host_segments(context_segments, token_segments, B, L, N)
    else:
        lens = host_lens(context_lens, B, L) or [L] * B
        cs = np.where(np.arange(L)[None, :] < np.asarray(lens)[:, None], 0, 255).astype(np.uint8)
        ts = np.full((B, N), 0xFFFFFFFF, np.uint32)
    live = np.where(w > 0, cs, 255).astype(np.uint8)                      # a row of weight 0 is padding
    bad = np.argwhere(~segments_allowed(live, ts).any(-1))
    if len(bad):
        b, t = bad[0]
        raise ValueError(f"context_weights: image {b}: token {t} allows no context row with a weight above 0 (mask {int(ts[b, t]):#x})")
    return cs, ts, w


def host_layers(layers, depth, what, allow_empty=False):
    """a choice of tower layers (any iterable of ints) -> a list of distinct indices in [0, depth), checked; `what` names the
    argument in the message; an empty choice is refused unless allow_empty"""
    chosen = [int(l) for l in layers]
    if (not chosen and not allow_empty) or len(set(chosen)) != len(chosen) or (chosen and (min(chosen) < 0 or max(chosen) >= depth)):
        raise ValueError(f"{what} {chosen!r} must be distinct indices in [0, {depth})")
    return chosen


class Keys(NamedTuple):
    """The KEY SETS of one call, checked (``host_keys``): which context rows a token attends to, and how much
    each counts.  lens: a list of B ints or None; context_segments numpy uint8 [B, L] / token_segments numpy uint32 [B, N] or None;
    weights numpy float32 [B, L] or None; shape: the (B, L, N) it was checked for.  Weights without segment arrays bring the neutral
    segments (segment 0 below an image's length, 255 behind, every token mask all ones) and no lengths; `neutral` says so and
    neutral_lens keeps the lengths they were built from (None: every row), for the native entries that stage them themselves.
    A layer that receives a Keys does not check it again."""
    lens: Optional[list] = None
    context_segments: Optional[np.ndarray] = None
    token_segments: Optional[np.ndarray] = None
    weights: Optional[np.ndarray] = None
    shape: tuple = (0, 0, 0)
    neutral: bool = False
    neutral_lens: Optional[list] = None

    def lane(self, lo, hi):
        """the record of the micro-batch of images [lo, hi): every array sliced"""
        cut = lambda a: None if a is None else a[lo:hi]
        return Keys(cut(self.lens), cut(self.context_segments), cut(self.token_segments), cut(self.weights),
                    (len(range(self.shape[0])[lo:hi]),) + tuple(self.shape[1:]), self.neutral, cut(self.neutral_lens))

    def cpu_args(self):
        """the four arrays in the order ``Layer.forward`` and ``CrossAttention.run`` take them behind the context; ``Layer.forward``
        hands them on beside the record"""
        return self.lens, self.context_segments, self.token_segments, self.weights


def host_keys(B, L, N, context_lens=None, context_segments=None, token_segments=None, context_weights=None, has_context=True, keys=None,
              missing="a context (context None IS the unconditional branch)"):
    """The four ways to say which context rows a token attends to -> the call's ``Keys``, brought to the host and checked ONCE
    (``host_lens``, ``host_segments``, ``host_weights``).  The rules live here and nowhere else: the arrays need a context; segments
    exclude lengths; weights fold the lengths into the neutral segments, after which there are no lengths.  All None: the empty
    record.  keys (instead of the four): a record checked before -- it comes back as it is, no array is looked at; one checked for
    another (B, L, N) is refused.  missing: what a caller without a context lacks, in that caller's words."""
    none = context_lens is None and context_segments is None and token_segments is None and context_weights is None
    if keys is not None:
        if not none:
            raise ValueError("keys stands for context_lens, context_segments, token_segments and context_weights: none of them beside it")
        if keys.shape != (B, L, N):
            raise ValueError(f"keys were checked for (B, L, N) = {keys.shape}, not for {(B, L, N)}")
        return keys
    if none:
        return Keys(shape=(B, L, N))
    if not has_context:
        what = "context_lens needs" if context_lens is not None else "context_weights need" if context_weights is not None else \
            "context_segments / token_segments need"
        raise ValueError(f"{what} {missing}")
    lens = host_lens(context_lens, B, L)
    if context_weights is not None:
        cs, ts, w = host_weights(context_weights, B, L, N, context_segments, token_segments, lens)
        neutral = context_segments is None and token_segments is None
        return Keys(None, cs, ts, w, (B, L, N), neutral, lens if neutral else None)
    if context_segments is None and token_segments is None:
        return Keys(lens, shape=(B, L, N))
    if lens is not None:
        raise ValueError("context_segments and context_lens exclude each other (mark padding rows with segment 255)")
    cs, ts = host_segments(context_segments, token_segments, B, L, N)
    return Keys(None, cs, ts, None, (B, L, N))


def segments_allowed(key_seg, query_mask):
    """numpy uint8 [B, L], uint32 [B, N] -> bool [B, N, L]: row k takes part in token t's softmax (the rule of pmhip_attention_segments)"""
    ks = key_seg.astype(np.int64)[:, None, :]
    return (ks < 32) & (((query_mask.astype(np.int64)[:, :, None] >> np.minimum(ks, 31)) & 1) != 0)


def swiglu_hidden(hidden_features):
    """hidden width rule of SwiGLUFFNFused (reference modules/mlp.py:53)."""
    return (int(hidden_features * 2 / 3) + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------
def gemm(a, w, bias=None, residual=None, res_rows=0, out_dtype=None, out=None):
    """a[M,K] @ w[N,K]^T (+bias) (+residual[m % res_rows]).  out (optional): the contiguous [M,N] tensor to write; it may BE the f32
    residual (res_rows covering all M rows): the stream updated in place, as pmhip_gemm allows."""
    dev = _dev(a, w, bias, residual, out)
    lib = _lib.load()
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out_dtype = out_dtype or a.dtype
        out = torch.empty(M, N, device=dev, dtype=out_dtype)
    else:
        if tuple(out.shape) != (M, N) or (out_dtype is not None and out.dtype != out_dtype):
            raise ValueError(f"gemm: out must be [{M}, {N}] of the requested dtype, got {out.dtype} {tuple(out.shape)}")
        out_dtype = out.dtype
    ldr = residual.shape[-1] if residual is not None else 0
    rr = res_rows or (residual.shape[0] if residual is not None else 0)
    with torch.cuda.device(dev):
        check(lib.pmhip_gemm(pm_dtype(a.dtype), _p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(residual), ldr,
                             rr, _p(out), N, pm_dtype(out_dtype), M, N, K, stream_ptr(dev)), "pmhip_gemm")
    return out


def gemm_swiglu(a, w12p, b12p):
    dev = _dev(a, w12p, b12p)
    lib = _lib.load()
    M, K = a.shape
    Hp = w12p.shape[0] // 2
    out = torch.empty(M, Hp, device=dev, dtype=a.dtype)
    with torch.cuda.device(dev):
        check(lib.pmhip_gemm_swiglu(pm_dtype(a.dtype), _p(a), a.stride(0), _p(w12p), _p(b12p), _p(out), Hp, M, Hp, K,
                                    stream_ptr(dev)), "pmhip_gemm_swiglu")
    return out


def gemm_heads(a, w, heads, tokens, kinds, q_scale=1.0, dim_head=64):
    """Head-split projection; returns one tensor per part (Q [B,H,t,dh], K [B,H,tp,dh], V^T [B,H,dh,tp]).
    dim_head 64 runs the fused epilogue; other values the plain GEMM + split path (pmhip_gemm_heads_dh)."""
    dev = _dev(a, w)
    lib = _lib.load()
    M, K = a.shape
    B = M // tokens
    tp = round_up(tokens, 64)
    dh = int(dim_head)
    outs = []
    for kind in kinds:
        if kind == PART_Q:
            outs.append(torch.empty(B, heads, tokens, dh, device=dev, dtype=a.dtype))
        elif kind == PART_K:
            outs.append(torch.zeros(B, heads, tp, dh, device=dev, dtype=a.dtype))
        else:
            outs.append(torch.zeros(B, heads, dh, tp, device=dev, dtype=a.dtype))
    kinds_c = (C.c_int * len(kinds))(*kinds)
    outs_c = (C.c_void_p * len(kinds))(*[o.data_ptr() for o in outs])
    with torch.cuda.device(dev):
        if dh == 64:
            check(lib.pmhip_gemm_heads(pm_dtype(a.dtype), _p(a), a.stride(0), _p(w), w.stride(0), M, K, heads, tokens, tp,
                                       len(kinds), kinds_c, outs_c, float(q_scale), stream_ptr(dev)), "pmhip_gemm_heads")
        else:
            scratch = torch.empty(M, len(kinds) * heads * dh, device=dev, dtype=torch.float32)
            check(lib.pmhip_gemm_heads_dh(pm_dtype(a.dtype), _p(a), a.stride(0), _p(w), w.stride(0), M, K, heads, dh, tokens, tp,
                                          len(kinds), kinds_c, outs_c, float(q_scale), _p(scratch), stream_ptr(dev)),
                  "pmhip_gemm_heads_dh")
    return outs


# ---- bf16 hi/lo residual stream + LayerNorm folded into the consuming GEMM (include/pmhip.h, pmhip_lnfold) ------------
def split_hilo(x):
    """x f32 [M,D] -> (hi, lo) bf16 planes with x = hi + lo"""
    dev = _dev(x)
    lib = _lib.load()
    M, D = x.shape
    hi = torch.empty(M, D, device=dev, dtype=torch.bfloat16)
    lo = torch.empty(M, D, device=dev, dtype=torch.bfloat16)
    with torch.cuda.device(dev):
        check(lib.pmhip_split_hilo(_p(x), _p(hi), _p(lo), M, D, stream_ptr(dev)), "pmhip_split_hilo")
    return hi, lo


def join_hilo(hi, lo):
    dev = _dev(hi, lo)
    lib = _lib.load()
    M, D = hi.shape
    out = torch.empty(M, D, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(lib.pmhip_join_hilo(_p(hi), _p(lo), _p(out), M, D, stream_ptr(dev)), "pmhip_join_hilo")
    return out


def gemm_hilo(a, w, res_hi, res_lo, bias=None, res_rows=0, stats=False):
    """(hi, lo) = split(a @ w^T + bias + (res_hi + res_lo)[m % res_rows]); bf16 operands.
    stats=True: also the per-row partial statistics [M, N/64, 2] of the new hi plane (for ln_coef_parts)."""
    dev = _dev(a, w, res_hi, res_lo)
    lib = _lib.load()
    M, K = a.shape
    N = w.shape[0]
    hi = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    lo = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    with torch.cuda.device(dev):
        if stats:
            parts = torch.full((M, N // 64, 2), float("nan"), device=dev, dtype=torch.float32)
            check(lib.pmhip_gemm_hilo_stats(_p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(res_hi), _p(res_lo), res_hi.stride(0),
                                            int(res_rows), _p(hi), _p(lo), N, M, N, K, _p(parts), stream_ptr(dev)), "pmhip_gemm_hilo_stats")
            return hi, lo, parts
        check(lib.pmhip_gemm_hilo(_p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(res_hi), _p(res_lo), res_hi.stride(0),
                                  int(res_rows), _p(hi), _p(lo), N, M, N, K, stream_ptr(dev)), "pmhip_gemm_hilo")
    return hi, lo


def gemm_hilo_center(a, w, res_hi, res_lo, bias=None, center_coef=None, shift=None, shift_mode=0, stats=False, center_extra=0.0):
    """gemm_hilo storing the pair of x - c, c = the row mean of the previous hi plane taken from `center_coef` ([M,2], ln_coef /
    ln_coef_parts); `shift` [M] fp32 is updated IN PLACE (shift_mode 1: <- 0, 2: += c).  -> (hi, lo[, parts])"""
    dev = _dev(a, w, res_hi, res_lo, center_coef, shift)
    lib = _lib.load()
    M, K = a.shape
    N = w.shape[0]
    hi = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    lo = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    parts = torch.full((M, N // 64, 2), float("nan"), device=dev, dtype=torch.float32) if stats else None
    with torch.cuda.device(dev):
        check(lib.pmhip_gemm_hilo_center(_p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(res_hi), _p(res_lo), res_hi.stride(0), 0,
                                         _p(hi), _p(lo), N, M, N, K, _p(parts), _p(center_coef), float(center_extra), _p(shift), int(shift_mode),
                                         stream_ptr(dev)), "pmhip_gemm_hilo_center")
    return (hi, lo, parts) if stats else (hi, lo)


def unshift_hilo(hi, lo, shift):
    """in place: (hi, lo) <- split(hi + lo + shift[row])"""
    dev = _dev(hi, lo, shift)
    M, D = hi.shape
    with torch.cuda.device(dev):
        check(_lib.load().pmhip_unshift_hilo(_p(hi), _p(lo), _p(shift), M, D, stream_ptr(dev)), "pmhip_unshift_hilo")
    return hi, lo


def ln_coef_parts(parts, eps=1e-5):
    """per-row (rstd, -rstd * mean) from gemm_hilo(..., stats=True)'s partial statistics -> f32 [M,2]"""
    dev = _dev(parts)
    lib = _lib.load()
    M, nparts, _ = parts.shape
    coef = torch.empty(M, 2, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(lib.pmhip_ln_coef_parts(_p(parts), nparts, float(eps), _p(coef), M, stream_ptr(dev)), "pmhip_ln_coef_parts")
    return coef


def layernorm_hilo(hi, lo, gamma, beta, eps=1e-5, out_dtype=torch.bfloat16):
    dev = _dev(hi, lo, gamma, beta)
    lib = _lib.load()
    M, D = hi.shape
    out = torch.empty(M, D, device=dev, dtype=out_dtype)
    with torch.cuda.device(dev):
        check(lib.pmhip_layernorm_hilo(_p(hi), _p(lo), _p(gamma), _p(beta), float(eps), _p(out), pm_dtype(out_dtype), M, D,
                                       stream_ptr(dev)), "pmhip_layernorm_hilo")
    return out


def layernorm_to_hilo(x, gamma, beta, eps=1e-5):
    dev = _dev(x, gamma, beta)
    lib = _lib.load()
    M, D = x.shape
    hi = torch.empty(M, D, device=dev, dtype=torch.bfloat16)
    lo = torch.empty(M, D, device=dev, dtype=torch.bfloat16)
    with torch.cuda.device(dev):
        check(lib.pmhip_layernorm_to_hilo(_p(x), _p(gamma), _p(beta), float(eps), _p(hi), _p(lo), M, D, stream_ptr(dev)),
              "pmhip_layernorm_to_hilo")
    return hi, lo


def ln_coef(hi, eps=1e-5):
    """per-row (rstd, -rstd * mean) of the hi plane -> f32 [M,2]"""
    dev = _dev(hi)
    lib = _lib.load()
    M, D = hi.shape
    coef = torch.empty(M, 2, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(lib.pmhip_ln_coef(_p(hi), float(eps), _p(coef), M, D, stream_ptr(dev)), "pmhip_ln_coef")
    return coef


def _lnfold(coef, c, d, parts=None, eps=1e-5):
    """coef [M,2] is an input, or -- with `parts` [M, K/64, 2] (the producer's partial statistics) -- an OUTPUT the call fills"""
    ln = _lib.LnFold()
    ln.coef, ln.c, ln.d = coef.data_ptr(), c.data_ptr(), d.data_ptr()
    if parts is not None:
        if parts.dtype != torch.float32 or not parts.is_contiguous() or parts.shape[0] != coef.shape[0] or parts.shape[-1] != 2:
            raise ValueError("fold parts must be a contiguous fp32 [M, K/64, 2] tensor")
        ln.parts, ln.nparts, ln.eps = parts.data_ptr(), parts.shape[1], float(eps)
    ln._keep = (coef, c, d, parts)
    return ln


def lnfold_supported(kind, M, N, K):
    return bool(_lib.load().pmhip_lnfold_supported(BF16, kind, M, N, K))


def gemm_ln(xb, wg, coef, c, d, bias=None, out_dtype=None, parts=None):
    dev = _dev(xb, wg, coef, c, d)
    lib = _lib.load()
    M, K = xb.shape
    N = wg.shape[0]
    out_dtype = out_dtype or xb.dtype
    out = torch.empty(M, N, device=dev, dtype=out_dtype)
    ln = _lnfold(coef, c, d, parts)
    with torch.cuda.device(dev):
        check(lib.pmhip_gemm_ln(pm_dtype(xb.dtype), _p(xb), xb.stride(0), _p(wg), wg.stride(0), _p(bias), _p(out), N,
                                pm_dtype(out_dtype), M, N, K, C.byref(ln), stream_ptr(dev)), "pmhip_gemm_ln")
    return out


def gemm_softmax_stats(x, w, bias=None, fold=None):
    """logits f32 [M,N] = x @ w.T + bias and the softmax statistics of their 64-column blocks, f32 [M, N/64, 2] = (max, sum of exp)
    (pmhip_gemm_softmax_stats; transformer.py:91).  fold = (coef, c, d[, parts]): x is the hi plane and w the gamma-scaled weights
    of a folded LayerNorm (gemm_ln)."""
    dev = _dev(x, w, bias)
    lib = _lib.load()
    M, K = x.shape
    N = w.shape[0]
    if N % 64:
        raise ValueError("gemm_softmax_stats: N must be a multiple of 64")
    out = torch.empty(M, N, device=dev, dtype=torch.float32)
    stats = torch.empty(M, N // 64, 2, device=dev, dtype=torch.float32)
    ln = _lnfold(*fold) if fold is not None else None
    with torch.cuda.device(dev):
        check(lib.pmhip_gemm_softmax_stats(pm_dtype(x.dtype), _p(x), x.stride(0), _p(w), w.stride(0), _p(bias), _p(out), N, M, N, K,
                                           C.byref(ln) if ln is not None else None, _p(stats), stream_ptr(dev)),
              "pmhip_gemm_softmax_stats")
    return out, stats


def gemm_swiglu_ln(xb, w12pg, b12p, coef, c, d, parts=None):
    dev = _dev(xb, w12pg, b12p)
    lib = _lib.load()
    M, K = xb.shape
    Hp = w12pg.shape[0] // 2
    out = torch.empty(M, Hp, device=dev, dtype=xb.dtype)
    ln = _lnfold(coef, c, d, parts)
    with torch.cuda.device(dev):
        check(lib.pmhip_gemm_swiglu_ln(pm_dtype(xb.dtype), _p(xb), xb.stride(0), _p(w12pg), _p(b12p), _p(out), Hp, M, Hp, K,
                                       C.byref(ln), stream_ptr(dev)), "pmhip_gemm_swiglu_ln")
    return out


def gemm_heads_ln(xb, wg, heads, tokens, kinds, q_scale, coef, c, d, parts=None):
    dev = _dev(xb, wg)
    lib = _lib.load()
    M, K = xb.shape
    B = M // tokens
    tp = round_up(tokens, 64)
    outs = []
    for kind in kinds:
        shape = (B, heads, tokens, 64) if kind == PART_Q else ((B, heads, tp, 64) if kind == PART_K else (B, heads, 64, tp))
        outs.append(torch.empty(shape, device=dev, dtype=xb.dtype))
    kinds_c = (C.c_int * len(kinds))(*kinds)
    outs_c = (C.c_void_p * len(kinds))(*[o.data_ptr() for o in outs])
    ln = _lnfold(coef, c, d, parts)
    with torch.cuda.device(dev):
        check(lib.pmhip_gemm_heads_ln(pm_dtype(xb.dtype), _p(xb), xb.stride(0), _p(wg), wg.stride(0), M, K, heads, tokens, tp,
                                      len(kinds), kinds_c, outs_c, float(q_scale), C.byref(ln), stream_ptr(dev)),
              "pmhip_gemm_heads_ln")
    return outs


def attention_fallbacks(reset=False, device=None):
    """Workgroups of the bf16 attention kernel that had to be run again through its exact path since the last reset
    (a probability of the fixed-reference fast path left the f32 range; include/pmhip.h)."""
    lib = _lib.load()
    n = C.c_ulonglong(0)
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        check(lib.pmhip_attention_fallbacks(C.byref(n), int(bool(reset))), "pmhip_attention_fallbacks")
    return int(n.value)


def key_bias(weights, use_exp2):
    """weights f32 on the device, any shape -> the bias of ``attention(key_weights=)`` in the kernel's score unit, same shape
    (pmhip_key_bias): 0 -> -inf, 1 -> exactly 0, otherwise log2(w), times ln 2 when the scores are nats (use_exp2 False).  One
    asynchronous launch on the current stream."""
    dev = _dev(weights)
    if weights.dtype != torch.float32 or weights.numel() == 0:
        raise ValueError(f"weights must be a non-empty float32 tensor, got {weights.dtype} {tuple(weights.shape)}")
    out = torch.empty_like(weights)
    with torch.cuda.device(dev):
        check(_lib.load().pmhip_key_bias(_p(weights), _p(out), weights.numel(), int(bool(use_exp2)), stream_ptr(dev)), "pmhip_key_bias")
    return out


def _key_sets(B, Nq, n_kv, dev, use_exp2, kv_lens, key_segments, query_segments, key_weights, exactly_one=False):
    """The optional arrays of ``attention``, ``attention_pick`` and ``attention_maps`` against (B, Nq, n_kv) -- the one place that
    says which go together.  exactly_one (``attention_pick``): one of kv_lens and the pair of segment arrays must select the form.
    For weights given alone the neutral arrays (every key segment 0, every query all ones) are built here.
    -> (key_segments, query_segments, bias), each None where the form has none"""
    if kv_lens is not None and (kv_lens.dtype != torch.int32 or tuple(kv_lens.shape) != (B,)):
        raise ValueError(f"kv_lens must be an int32 tensor of shape ({B},), got {kv_lens.dtype} {tuple(kv_lens.shape)}")
    if (key_segments is None) != (query_segments is None):
        raise ValueError("key_segments and query_segments come together")
    if key_segments is not None:
        if kv_lens is not None:
            raise ValueError("exactly one of kv_lens and the pair key_segments + query_segments selects the form" if exactly_one else
                             "key_segments / query_segments and kv_lens exclude each other (mark padding keys with segment 255)")
        if key_segments.dtype != torch.uint8 or tuple(key_segments.shape) != (B, n_kv) or not key_segments.is_contiguous():
            raise ValueError(f"key_segments must be a contiguous uint8 tensor of shape ({B}, {n_kv}), got {key_segments.dtype} "
                             f"{tuple(key_segments.shape)}")
        if query_segments.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or tuple(query_segments.shape) != (B, Nq) or \
                not query_segments.is_contiguous():
            raise ValueError(f"query_segments must be a contiguous int32 / uint32 tensor of shape ({B}, {Nq}), got {query_segments.dtype} "
                             f"{tuple(query_segments.shape)}")
    bias = None
    if key_weights is not None:
        if kv_lens is not None:
            raise ValueError("key_weights and kv_lens exclude each other (a weight of 0 makes a key padding)")
        if key_weights.dtype != torch.float32 or tuple(key_weights.shape) != (B, n_kv):
            raise ValueError(f"key_weights must be a float32 tensor of shape ({B}, {n_kv}), got {key_weights.dtype} {tuple(key_weights.shape)}")
        bias = key_bias(key_weights, use_exp2)
        if key_segments is None:
            key_segments = torch.zeros(B, n_kv, dtype=torch.uint8, device=dev)
            query_segments = torch.full((B, Nq), -1, dtype=torch.int32, device=dev)
    if exactly_one and kv_lens is None and key_segments is None:
        raise ValueError("exactly one of kv_lens and the pair key_segments + query_segments selects the form")
    return key_segments, query_segments, bias


def attention(q, k, vt, n_kv, use_exp2=False, kv_lens=None, key_segments=None, query_segments=None, key_weights=None):
    """q [B,H,Nq,dh], k [B,H,Nkp,dh], vt [B,H,dh,Nkp] -> [B*Nq, H*dh]  (dh 64: tuned MFMA kernel; else pmhip_attention_dh).
    kv_lens (None: every image attends to n_kv keys): int32 [B] on the device, image b attends to its first kv_lens[b] keys
    (clamped to [1, n_kv] by the kernel) -- pmhip_attention_lens.
    key_segments uint8 [B, n_kv] + query_segments int32 / uint32 [B, Nq] (bit masks), both on the device and never beside kv_lens:
    key j takes part in query i's softmax iff key_segments[b, j] < 32 and bit key_segments[b, j] of query_segments[b, i] is set; 255
    marks padding, whose K rows and V^T columns never reach a result -- pmhip_attention_segments.  Every query must allow a key.
    key_weights f32 [B, n_kv] on the device, alone or with the pair of segment arrays, never beside kv_lens:
    over the keys a query allows p = w exp(s) / sum w exp(s); weight 0 makes the key padding, weights 0 or in [2^-20, 2^20].  Alone,
    the neutral arrays (every key segment 0, every query all ones) are built here -- pmhip_key_bias, pmhip_attention_weighted."""
    dev = _dev(q, k, vt, kv_lens, key_segments, query_segments, key_weights)
    lib = _lib.load()
    B, H, Nq, dh = q.shape
    nkp = k.shape[2]
    out = torch.empty(B * Nq, H * dh, device=dev, dtype=q.dtype)
    key_segments, query_segments, bias = _key_sets(B, Nq, n_kv, dev, use_exp2, kv_lens, key_segments, query_segments, key_weights)
    with torch.cuda.device(dev):
        if bias is not None:
            check(lib.pmhip_attention_weighted(pm_dtype(q.dtype), _p(q), _p(k), _p(vt), _p(out), H * dh, B, H, dh, Nq, n_kv, nkp,
                                               int(use_exp2), _p(key_segments), _p(query_segments), _p(bias), stream_ptr(dev)),
                  "pmhip_attention_weighted")
        elif key_segments is not None:
            check(lib.pmhip_attention_segments(pm_dtype(q.dtype), _p(q), _p(k), _p(vt), _p(out), H * dh, B, H, dh, Nq, n_kv, nkp,
                                               int(use_exp2), _p(key_segments), _p(query_segments), stream_ptr(dev)),
                  "pmhip_attention_segments")
        elif kv_lens is not None:
            check(lib.pmhip_attention_lens(pm_dtype(q.dtype), _p(q), _p(k), _p(vt), _p(out), H * dh, B, H, dh, Nq, n_kv, nkp,
                                           int(use_exp2), _p(kv_lens), stream_ptr(dev)), "pmhip_attention_lens")
        elif dh == 64:
            check(lib.pmhip_attention(pm_dtype(q.dtype), _p(q), _p(k), _p(vt), _p(out), H * 64, B, H, Nq, n_kv, nkp,
                                      int(use_exp2), stream_ptr(dev)), "pmhip_attention")
        else:
            check(lib.pmhip_attention_dh(pm_dtype(q.dtype), _p(q), _p(k), _p(vt), _p(out), H * dh, B, H, dh, Nq, n_kv, nkp,
                                         int(use_exp2), stream_ptr(dev)), "pmhip_attention_dh")
    return out


def attention_pick(q, k, vt, n_kv, pick, want, out, use_exp2=False, kv_lens=None, key_segments=None, query_segments=None,
                   key_weights=None):
    """``attention`` for SOME images of the batch, into a caller-supplied `out` (pmhip_attention_pick).
    pick uint8 [B] on the device names the kind of every image, `want` the kind this call serves: the rows of an image with
    pick[b] == want become, bit for bit, what ``attention`` with the same kv_lens / key_segments + query_segments writes for it,
    the rows of every other image stay as they are -- so two calls, one per kind, fill one buffer.  Exactly one of kv_lens and the
    pair key_segments + query_segments selects the form.  out: [B*Nq, H*dh] of q's dtype with unit column stride; its row stride is
    the leading dimension (a window of a larger buffer will do).
    key_weights f32 [B, n_kv] on the device, alone or with the pair of segment arrays, never beside kv_lens, as
    in ``attention``: the served images get the rows of ``attention(key_weights=)`` -- pmhip_key_bias, pmhip_attention_pick_weighted.
    The weights of a skipped image are read by pmhip_key_bias only; what it makes of them (NaN included) is read by nothing.  -> out"""
    dev = _dev(q, k, vt, pick, kv_lens, key_segments, query_segments, key_weights)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dim() == 2):
        raise ValueError("out must be a 2-D tensor on the operands' device")
    lib = _lib.load()
    B, H, Nq, dh = q.shape
    nkp = k.shape[2]
    if pick.dtype != torch.uint8 or tuple(pick.shape) != (B,):
        raise ValueError(f"pick must be a uint8 tensor of shape ({B},), got {pick.dtype} {tuple(pick.shape)}")
    if out.dtype != q.dtype or tuple(out.shape) != (B * Nq, H * dh) or out.stride(1) != 1 or out.stride(0) < H * dh:
        raise ValueError(f"out must be a {q.dtype} [{B * Nq}, {H * dh}] tensor with unit column stride, got {out.dtype} {tuple(out.shape)} "
                         f"strides {tuple(out.stride())}")
    key_segments, query_segments, bias = _key_sets(B, Nq, n_kv, dev, use_exp2, kv_lens, key_segments, query_segments, key_weights,
                                                   exactly_one=True)
    if bias is not None:
        with torch.cuda.device(dev):
            check(lib.pmhip_attention_pick_weighted(pm_dtype(q.dtype), _p(q), _p(k), _p(vt), _p(out), out.stride(0), B, H, dh, Nq, n_kv, nkp,
                                                    int(use_exp2), _p(key_segments), _p(query_segments), _p(bias), _p(pick), int(want),
                                                    stream_ptr(dev)), "pmhip_attention_pick_weighted")
        return out
    with torch.cuda.device(dev):
        check(lib.pmhip_attention_pick(pm_dtype(q.dtype), _p(q), _p(k), _p(vt), _p(out), out.stride(0), B, H, dh, Nq, n_kv, nkp, int(use_exp2),
                                       _p(kv_lens), _p(key_segments), _p(query_segments), _p(pick), int(want), stream_ptr(dev)),
              "pmhip_attention_pick")
    return out


def attention_maps(q, k, n_kv, use_exp2=False, kv_lens=None, key_segments=None, query_segments=None, key_weights=None, out=None,
                   scale=1.0, accumulate=False):
    """The head-mean probabilities of the softmax ``attention`` defines on the same arguments (pmhip_attention_maps; DESIGN.md
    section 4y): q [B,H,Nq,dh], k [B,H,Nkp,dh] -> f32 [B, Nq, n_kv] with out[b, q, j] = scale / H * sum_h p_h[q, j], added to what
    `out` holds when `accumulate`.  kv_lens, key_segments + query_segments and key_weights select the form exactly as in
    ``attention`` (same checks, same neutral arrays for weights alone, the weights through ``key_bias``).  A key that takes part in
    no softmax of a query is exactly 0 (left as it is under `accumulate`).  P stays f32 in bf16 mode.  out (None: a new tensor;
    required under `accumulate`): f32 [B, Nq, n_kv] on the operands' device with unit stride in the last dimension, stride(1) >= n_kv
    the leading dimension and stride(0) == Nq * stride(1) (a window of a wider buffer will do).  -> out"""
    dev = _dev(q, k, kv_lens, key_segments, query_segments, key_weights)
    lib = _lib.load()
    B, H, Nq, dh = q.shape
    nkp = k.shape[2]
    if k.dtype != q.dtype or k.shape[0] != B or k.shape[1] != H or k.shape[3] != dh or nkp < n_kv:
        raise ValueError(f"k must be a {q.dtype} [{B}, {H}, >= {n_kv}, {dh}] tensor, got {k.dtype} {tuple(k.shape)}")
    key_segments, query_segments, bias = _key_sets(B, Nq, n_kv, dev, use_exp2, kv_lens, key_segments, query_segments, key_weights)
    if out is None:
        if accumulate:
            raise ValueError("accumulate adds to `out`: pass the tensor to add to")
        out = torch.empty(B, Nq, n_kv, device=dev, dtype=torch.float32)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == torch.float32 and
            tuple(out.shape) == (B, Nq, n_kv) and out.stride(2) == 1 and out.stride(1) >= n_kv and out.stride(0) == Nq * out.stride(1)):
        raise ValueError(f"out must be a float32 [{B}, {Nq}, {n_kv}] tensor on the operands' device with unit stride in the last dimension "
                         f"and stride(0) == {Nq} * stride(1)")
    with torch.cuda.device(dev):
        check(lib.pmhip_attention_maps(pm_dtype(q.dtype), _p(q), _p(k), _p(out), out.stride(1), B, H, dh, Nq, n_kv, nkp, int(bool(use_exp2)),
                                       _p(kv_lens), _p(key_segments), _p(query_segments), _p(bias), float(scale), int(bool(accumulate)),
                                       stream_ptr(dev)), "pmhip_attention_maps")
    return out


def _pair_operands(qs, ks, qt, kt, vt, n_src, n_tgt, row_map, blend, gain, lens_src, lens_tgt, required):
    """The operands of a prompt-to-prompt pair, checked once for ``attention_control`` and ``attention_phrase_score``: qs like qt
    [B,H,Nq,dh], ks [B,H,Lsp,dh], kt [B,H,Ltp,dh] (and vt [B,H,dh,Ltp] unless None) of qt's dtype, n_src / n_tgt within the pads, the
    control arrays row_map int32, blend and gain float32 [B, n_tgt] -- all three (`required`) or all three or none --, and the
    lengths int32 [B] or None.  -> B, H, Nq, dh, Lsp, Ltp"""
    B, H, Nq, dh = qt.shape
    if tuple(qs.shape) != (B, H, Nq, dh) or qs.dtype != qt.dtype:
        raise ValueError(f"qs must be a {qt.dtype} {(B, H, Nq, dh)} tensor like qt, got {qs.dtype} {tuple(qs.shape)}")
    lsp, ltp = ks.shape[2], kt.shape[2]
    for name, x, want in (("ks", ks, (B, H, lsp, dh)), ("kt", kt, (B, H, ltp, dh)), ("vt", vt, (B, H, dh, ltp))):
        if x is not None and (x.dtype != qt.dtype or tuple(x.shape) != want):
            raise ValueError(f"{name} must be a {qt.dtype} {want} tensor, got {x.dtype} {tuple(x.shape)}")
    if lsp < n_src or ltp < n_tgt:
        raise ValueError(f"n_src={n_src} / n_tgt={n_tgt} exceed the padded contexts {lsp} / {ltp}")
    control = (("row_map", row_map, torch.int32), ("blend", blend, torch.float32), ("gain", gain, torch.float32))
    if required or any(x is not None for _, x, _ in control):
        if any(x is None for _, x, _ in control):
            raise ValueError("row_map, blend and gain " + ("are required" if required else "come together (all None: no control)"))
        for name, x, dt in control:
            if x.dtype != dt or tuple(x.shape) != (B, n_tgt):
                raise ValueError(f"{name} must be a {dt} tensor of shape ({B}, {n_tgt}), got {x.dtype} {tuple(x.shape)}")
    for name, x in (("lens_src", lens_src), ("lens_tgt", lens_tgt)):
        if x is not None and (x.dtype != torch.int32 or tuple(x.shape) != (B,)):
            raise ValueError(f"{name} must be an int32 tensor of shape ({B},), got {x.dtype} {tuple(x.shape)}")
    return B, H, Nq, dh, lsp, ltp


def attention_control(qs, ks, qt, kt, vt, n_src, n_tgt, row_map, blend, gain, use_exp2=False, lens_src=None, lens_tgt=None, out=None):
    """The edited pass of a prompt-to-prompt pair (pmhip_attention_control): qs [B,H,Nq,dh], ks [B,H,Lsp,dh] the
    source pass, qt, kt [B,H,Ltp,dh], vt [B,H,dh,Ltp] the edited one -> [B*Nq, H*dh] with
        P[q, j] = gain[b, j] * (has ? (1 - blend[b, j]) * pt[q, j] + blend[b, j] * ps[q, row_map[b, j]] : pt[q, j]),   out = P V
    ps / pt the softmaxes of the two passes over their first lens_src[b] / lens_tgt[b] keys (None: n_src / n_tgt; clamped by the
    kernel as in ``attention``), has = 0 <= row_map[b, j] < the source length and blend[b, j] != 0.  No renormalisation.
    row_map int32, blend and gain float32, all contiguous [B, n_tgt] on the device; the ranges (blend in [0, 1], gain finite and
    >= 0) are the caller's to keep.  out (None: a new tensor): [B*Nq, H*dh] of q's dtype with unit column stride; its row stride is
    the leading dimension.  -> out"""
    dev = _dev(qs, ks, qt, kt, vt, row_map, blend, gain, lens_src, lens_tgt)      # (every one of them on the device and contiguous)
    lib = _lib.load()
    B, H, Nq, dh, lsp, ltp = _pair_operands(qs, ks, qt, kt, vt, n_src, n_tgt, row_map, blend, gain, lens_src, lens_tgt, required=True)
    if out is None:
        out = torch.empty(B * Nq, H * dh, device=dev, dtype=qt.dtype)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == qt.dtype and
            tuple(out.shape) == (B * Nq, H * dh) and out.stride(1) == 1 and out.stride(0) >= H * dh):
        raise ValueError(f"out must be a {qt.dtype} [{B * Nq}, {H * dh}] tensor on the operands' device with unit column stride")
    with torch.cuda.device(dev):
        check(lib.pmhip_attention_control(pm_dtype(qt.dtype), _p(qs), _p(ks), _p(qt), _p(kt), _p(vt), _p(out), out.stride(0), B, H, dh, Nq,
                                          int(n_src), lsp, int(n_tgt), ltp, int(bool(use_exp2)), _p(row_map), _p(blend), _p(gain),
                                          _p(lens_src), _p(lens_tgt), stream_ptr(dev)), "pmhip_attention_control")
    return out


def attention_phrase_score(qs, ks, qt, kt, n_src, n_tgt, w_src, w_tgt, row_map=None, blend=None, gain=None, use_exp2=False, lens_src=None,
                           lens_tgt=None, out=None, scale=1.0, accumulate=False):
    """Where a prompt-to-prompt pair looks at a phrase (pmhip_attention_phrase_score): the operands, lengths
    and control arrays of ``attention_control`` without vt -> (score_src, score_tgt), f32 [B, Nq] each, with
        score_src[b, q] = scale / H * sum_h sum_k w_src[b, k] ps_h[q, k]        score_tgt[b, q] = scale / H * sum_h sum_j w_tgt[b, j] P_h[q, j]
    ps and P those of ``attention_control``; row_map, blend and gain come together or not at all (None: P is the edited pass's own
    softmax).  w_src f32 [B, n_src], w_tgt f32 [B, n_tgt]: the phrase's row weights, finite and >= 0 (the caller's to keep).  P stays
    f32 in bf16 mode.  out (None: two new tensors; required under `accumulate`, which adds to what they hold): the pair
    (score_src, score_tgt), contiguous f32 [B, Nq] on the operands' device.  -> out"""
    dev = _dev(qs, ks, qt, kt, w_src, w_tgt, row_map, blend, gain, lens_src, lens_tgt)
    lib = _lib.load()
    B, H, Nq, dh, lsp, ltp = _pair_operands(qs, ks, qt, kt, None, n_src, n_tgt, row_map, blend, gain, lens_src, lens_tgt, required=False)
    for name, x, n in (("w_src", w_src, n_src), ("w_tgt", w_tgt, n_tgt)):
        if x is None or x.dtype != torch.float32 or tuple(x.shape) != (B, n):
            raise ValueError(f"{name} must be a float32 tensor of shape ({B}, {n})")
    if out is None:
        if accumulate:
            raise ValueError("accumulate adds to `out`: pass the pair of tensors to add to")
        out = (torch.empty(B, Nq, device=dev, dtype=torch.float32), torch.empty(B, Nq, device=dev, dtype=torch.float32))
    if not (isinstance(out, (tuple, list)) and len(out) == 2 and all(
            isinstance(o, torch.Tensor) and o.is_cuda and o.device == dev and o.dtype == torch.float32 and tuple(o.shape) == (B, Nq) and
            o.is_contiguous() for o in out)):
        raise ValueError(f"out must be a pair of contiguous float32 [{B}, {Nq}] tensors on the operands' device")
    with torch.cuda.device(dev):
        check(lib.pmhip_attention_phrase_score(pm_dtype(qt.dtype), _p(qs), _p(ks), _p(qt), _p(kt), B, H, dh, Nq, int(n_src), lsp, int(n_tgt), ltp,
                                               int(bool(use_exp2)), _p(row_map), _p(blend), _p(gain), _p(lens_src), _p(lens_tgt), _p(w_src),
                                               _p(w_tgt), _p(out[0]), _p(out[1]), float(scale), int(bool(accumulate)), stream_ptr(dev)),
              "pmhip_attention_phrase_score")
    return out[0], out[1]


def phrase_region(score_src, score_tgt, g, threshold, grow=0, out=None):
    """The blend region of a pair from its two phrase scores (pmhip_phrase_region): score_src, score_tgt
    contiguous f32 [B, g*g] on the device -> uint8 [B, g*g], 1 where score_x >= threshold * max score_x in either half, dilated
    `grow` times by a 3 x 3 maximum on the g x g grid.  0 < threshold <= 1, grow >= 0, 1 <= g <= 64."""
    dev = _dev(score_src, score_tgt)
    B = score_src.shape[0]
    for name, x in (("score_src", score_src), ("score_tgt", score_tgt)):
        if x.dtype != torch.float32 or tuple(x.shape) != (B, g * g):
            raise ValueError(f"{name} must be a float32 tensor of shape ({B}, {g * g}), got {x.dtype} {tuple(x.shape)}")
    if not (isinstance(threshold, (int, float)) and 0 < threshold <= 1):
        raise ValueError(f"phrase_region: threshold {threshold!r} must be in (0, 1]")
    if not (isinstance(grow, int) and grow >= 0):
        raise ValueError(f"phrase_region: grow {grow!r} must be a non-negative integer")
    if out is None:
        out = torch.empty(B, g * g, device=dev, dtype=torch.uint8)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == torch.uint8 and tuple(out.shape) == (B, g * g) and
            out.is_contiguous()):
        raise ValueError(f"out must be a contiguous uint8 [{B}, {g * g}] tensor on the operands' device")
    with torch.cuda.device(dev):
        check(_lib.load().pmhip_phrase_region(_p(score_src), _p(score_tgt), _p(out), B, int(g), float(threshold), int(grow), stream_ptr(dev)),
              "pmhip_phrase_region")
    return out


def blend_tokens(mask, pred_src, merged_src, score_src, pred_tgt, merged_tgt, score_tgt):
    """The token blend under a region (pmhip_blend_tokens), IN PLACE on the edited half: where mask == 0
    (pred_tgt, merged_tgt, score_tgt) take the source half's values, elsewhere they stay.  mask uint8, pred / merged int64, score f32,
    all contiguous with B * N elements on the device.  The source half is read only.  -> (pred_tgt, merged_tgt, score_tgt)"""
    dev = _dev(mask, pred_src, merged_src, score_src, pred_tgt, merged_tgt, score_tgt)
    n = mask.numel()
    if mask.dtype != torch.uint8 or mask.dim() != 2 or n == 0:
        raise ValueError(f"mask must be a non-empty uint8 tensor [B, N], got {mask.dtype} {tuple(mask.shape)}")
    for name, x, dt in (("pred_src", pred_src, torch.int64), ("merged_src", merged_src, torch.int64), ("score_src", score_src, torch.float32),
                        ("pred_tgt", pred_tgt, torch.int64), ("merged_tgt", merged_tgt, torch.int64), ("score_tgt", score_tgt, torch.float32)):
        if x.dtype != dt or x.numel() != n:
            raise ValueError(f"{name} must be a {dt} tensor of {n} elements, got {x.dtype} {tuple(x.shape)}")
    with torch.cuda.device(dev):
        check(_lib.load().pmhip_blend_tokens(_p(mask), _p(pred_src), _p(merged_src), _p(score_src), _p(pred_tgt), _p(merged_tgt), _p(score_tgt),
                                             mask.shape[0], mask.shape[1], stream_ptr(dev)), "pmhip_blend_tokens")
    return pred_tgt, merged_tgt, score_tgt


def layernorm(x, gamma, beta, eps=1e-5, out_dtype=torch.float32):
    dev = _dev(x, gamma, beta)
    lib = _lib.load()
    M, D = x.shape
    out = torch.empty(M, D, device=dev, dtype=out_dtype)
    with torch.cuda.device(dev):
        check(lib.pmhip_layernorm(_p(x), _p(gamma), _p(beta), float(eps), _p(out), pm_dtype(out_dtype), M, D,
                                  stream_ptr(dev)), "pmhip_layernorm")
    return out


def rmsnorm(x, weight, eps=1e-6, out_dtype=torch.float32):
    """T5LayerNorm (pmhip_rmsnorm): weight * (x * rsqrt(mean(x^2) + eps)); x f32 [M, D], D % 4 == 0, D <= 4096"""
    dev = _dev(x, weight)
    lib = _lib.load()
    M, D = x.shape
    out = torch.empty(M, D, device=dev, dtype=out_dtype)
    with torch.cuda.device(dev):
        check(lib.pmhip_rmsnorm(_p(x), _p(weight), float(eps), _p(out), pm_dtype(out_dtype), M, D, stream_ptr(dev)), "pmhip_rmsnorm")
    return out


def geglu(u, out_dtype=torch.float32):
    """T5's gated GELU (pmhip_geglu): u f32 [M, 2F], the output of one GEMM against [wi_0; wi_1] -> gelu_new(u[:, :F]) * u[:, F:] as
    `out_dtype` [M, F]"""
    dev = _dev(u)
    lib = _lib.load()
    M, F2 = u.shape
    F = F2 // 2
    if F2 != 2 * F or u.dtype != torch.float32:
        raise ValueError(f"geglu: u must be float32 [M, 2F], got {u.dtype} {tuple(u.shape)}")
    out = torch.empty(M, F, device=dev, dtype=out_dtype)
    with torch.cuda.device(dev):
        check(lib.pmhip_geglu(_p(u), 2 * F, _p(out), F, pm_dtype(out_dtype), M, F, stream_ptr(dev)), "pmhip_geglu")
    return out


def attention_relbias(q, k, vt, rel_bias, kv_lens=None, out=None):
    """Self-attention with T5's relative-position bias (pmhip_attention_relbias): q [B,H,L,64] UNSCALED, k [B,H,Lp,64], vt [B,H,64,Lp]
    as gemm_heads writes them; rel_bias f32 [H, 2L-1] on the device, entry (k - q) + L - 1 is added to the score of query q and key k;
    kv_lens int32 [B] on the device or None -> [B*L, H*64].  `out` may be a column slice of a wider matrix."""
    dev = _dev(q, k, vt, rel_bias, kv_lens)
    lib = _lib.load()
    B, H, L, dh = q.shape
    if dh != 64:
        raise ValueError(f"attention_relbias: dim_head={dh} not served (64 only)")
    if tuple(rel_bias.shape) != (H, 2 * L - 1) or rel_bias.dtype != torch.float32:
        raise ValueError(f"attention_relbias: rel_bias must be float32 [{H}, {2 * L - 1}], got {rel_bias.dtype} {tuple(rel_bias.shape)}")
    if kv_lens is not None and (kv_lens.dtype != torch.int32 or kv_lens.numel() != B):
        raise ValueError(f"attention_relbias: kv_lens must be int32 [{B}]")
    if out is None:
        out = torch.empty(B * L, H * 64, device=dev, dtype=q.dtype)
    if not out.is_cuda or out.dtype != q.dtype or tuple(out.shape) != (B * L, H * 64) or out.stride(1) != 1:
        raise ValueError(f"attention_relbias: out must be {q.dtype} [{B * L}, {H * 64}] with unit column stride")
    with torch.cuda.device(dev):
        check(lib.pmhip_attention_relbias(pm_dtype(q.dtype), _p(q), _p(k), _p(vt), _p(out), out.stride(0), B, H, L, k.shape[2], _p(rel_bias),
                                          _p(kv_lens), stream_ptr(dev)), "pmhip_attention_relbias")
    return out


def attention_causal(q, k, vt, out=None):
    """Causal self-attention (pmhip_attention_causal): q [B,H,L,64] ALREADY SCALED, k [B,H,Lp,64], vt [B,H,64,Lp] as gemm_heads /
    split_heads write them; query q attends to the keys [0, q] -> [B*L, H*64].  `out` may be a column slice of a wider matrix."""
    dev = _dev(q, k, vt)
    lib = _lib.load()
    B, H, L, dh = q.shape
    if dh != 64:
        raise ValueError(f"attention_causal: dim_head={dh} not served (64 only)")
    if k.dtype != q.dtype or vt.dtype != q.dtype or tuple(k.shape) != (B, H, k.shape[2], 64) or tuple(vt.shape) != (B, H, 64, k.shape[2]):
        raise ValueError(f"attention_causal: k / vt must be {q.dtype} [{B}, {H}, Lp, 64] / [{B}, {H}, 64, Lp], got {k.dtype} "
                         f"{tuple(k.shape)} / {vt.dtype} {tuple(vt.shape)}")
    if out is None:
        out = torch.empty(B * L, H * 64, device=dev, dtype=q.dtype)
    if not out.is_cuda or out.dtype != q.dtype or tuple(out.shape) != (B * L, H * 64) or out.stride(1) != 1:
        raise ValueError(f"attention_causal: out must be {q.dtype} [{B * L}, {H * 64}] with unit column stride")
    with torch.cuda.device(dev):
        check(lib.pmhip_attention_causal(pm_dtype(q.dtype), _p(q), _p(k), _p(vt), _p(out), out.stride(0), B, H, L, k.shape[2],
                                         stream_ptr(dev)), "pmhip_attention_causal")
    return out


def split_heads(u, heads, tokens, kinds, q_scale=1.0, dtype=torch.float32):
    """Head split of a projection that already carries its bias (pmhip_split_heads): u f32 [M, len(kinds)*heads*64], the output of
    one gemm(bias=) -> one `dtype` tensor per part, as gemm_heads returns them (Q [B,H,t,64] * q_scale, K [B,H,tp,64], V^T
    [B,H,64,tp], tp = tokens rounded up to 64, the padding zero)."""
    dev = _dev(u)
    lib = _lib.load()
    M, N = u.shape
    if u.dtype != torch.float32 or N != len(kinds) * heads * 64 or M % tokens:
        raise ValueError(f"split_heads: u must be float32 [B*{tokens}, {len(kinds)}*{heads}*64], got {u.dtype} {tuple(u.shape)}")
    B = M // tokens
    tp = round_up(tokens, 64)
    outs = []
    for kind in kinds:
        if kind == PART_Q:
            outs.append(torch.empty(B, heads, tokens, 64, device=dev, dtype=dtype))
        elif kind == PART_K:
            outs.append(torch.zeros(B, heads, tp, 64, device=dev, dtype=dtype))
        else:
            outs.append(torch.zeros(B, heads, 64, tp, device=dev, dtype=dtype))
    kinds_c = (C.c_int * len(kinds))(*kinds)
    outs_c = (C.c_void_p * len(kinds))(*[o.data_ptr() for o in outs])
    with torch.cuda.device(dev):
        check(lib.pmhip_split_heads(pm_dtype(dtype), _p(u), N, M, heads, tokens, tp, len(kinds), kinds_c, outs_c, float(q_scale),
                                    stream_ptr(dev)), "pmhip_split_heads")
    return outs


GELU_KINDS = {"erf": 0, "quick": 1}


def gelu(u, out_dtype=torch.float32, kind="erf"):
    """pmhip_gelu on the f32 output of a GEMM that added its bias: kind "erf" is nn.GELU() (0.5 x erfc(-x / sqrt 2)), "quick" is
    open_clip's QuickGELU (x / (1 + exp(-1.702 x))); u f32 [M, F], F % 4 == 0 -> `out_dtype` [M, F]"""
    dev = _dev(u)
    lib = _lib.load()
    if kind not in GELU_KINDS:
        raise ValueError(f"gelu: kind must be one of {sorted(GELU_KINDS)}, got {kind!r}")
    if u.dim() != 2 or u.dtype != torch.float32:
        raise ValueError(f"gelu: u must be float32 [M, F], got {u.dtype} {tuple(u.shape)}")
    M, F = u.shape
    out = torch.empty(M, F, device=dev, dtype=out_dtype)
    with torch.cuda.device(dev):
        check(lib.pmhip_gelu(_p(u), F, _p(out), F, pm_dtype(out_dtype), M, F, GELU_KINDS[kind], stream_ptr(dev)), "pmhip_gelu")
    return out


def patchify(img, patch, out_dtype=torch.float32):
    dev = _dev(img)
    lib = _lib.load()
    B, Cc, H, W = img.shape
    out = torch.empty(B * (H // patch) * (W // patch), Cc * patch * patch, device=dev, dtype=out_dtype)
    with torch.cuda.device(dev):
        check(lib.pmhip_patchify(_p(img), _p(out), pm_dtype(out_dtype), B, Cc, H, W, patch, stream_ptr(dev)),
              "pmhip_patchify")
    return out


def unpatchify_clamp(y, B, channels, size, patch, lo=-1.0, hi=1.0):
    dev = _dev(y)
    lib = _lib.load()
    img = torch.empty(B, channels, size, size, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(lib.pmhip_unpatchify_clamp(_p(y), _p(img), B, channels, size, size, patch, float(lo), float(hi),
                                         stream_ptr(dev)), "pmhip_unpatchify_clamp")
    return img


def convert_pad(x, kpad, out_dtype):
    dev = _dev(x)
    lib = _lib.load()
    M, K = x.shape
    out = torch.empty(M, kpad, device=dev, dtype=out_dtype)
    with torch.cuda.device(dev):
        check(lib.pmhip_convert_pad(_p(x), K, _p(out), pm_dtype(out_dtype), kpad, M, stream_ptr(dev)),
              "pmhip_convert_pad")
    return out


def add_rows(x, table):
    dev = _dev(x, table)
    lib = _lib.load()
    M, D = x.shape
    out = torch.empty_like(x)
    with torch.cuda.device(dev):
        check(lib.pmhip_add_rows(_p(x), _p(table), table.shape[0], _p(out), M, D, stream_ptr(dev)), "pmhip_add_rows")
    return out


def guidance_combine(cond, uncond, scale, out=None, with_stats=False):
    """uncond + scale * (cond - uncond), fp32, same shape; `out` may be one of the inputs.
    with_stats: returns (out, block_stats [..., V/64, 2]) -- the softmax statistics sample_rows(block_stats=) takes."""
    dev = _dev(cond, uncond)
    if cond.shape != uncond.shape or cond.dtype != torch.float32 or uncond.dtype != torch.float32:
        raise ValueError("guidance_combine needs two fp32 tensors of one shape")
    out = torch.empty(cond.shape, device=dev, dtype=torch.float32) if out is None else out
    if out.shape != cond.shape or out.dtype != torch.float32 or out.device != cond.device:
        raise ValueError("guidance_combine: `out` must be an fp32 tensor of the inputs' shape on their device")
    if not (cond.is_contiguous() and uncond.is_contiguous() and out.is_contiguous()):
        raise ValueError("guidance_combine needs contiguous tensors (the kernel walks them as flat arrays)")
    if cond.numel() % 4:
        raise ValueError("guidance_combine: the element count must be a multiple of 4")
    if with_stats:
        if cond.shape[-1] % 64:
            raise ValueError("guidance_combine(with_stats=True): rows must be a multiple of 64 long")
        stats = torch.empty(cond.shape[:-1] + (cond.shape[-1] // 64, 2), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            check(_lib.load().pmhip_guidance_combine_stats(_p(cond), _p(uncond), float(scale), _p(out), cond.numel(), _p(stats),
                                                           stream_ptr(dev)), "pmhip_guidance_combine_stats")
        return out, stats
    with torch.cuda.device(dev):
        check(_lib.load().pmhip_guidance_combine(_p(cond), _p(uncond), float(scale), _p(out), cond.numel(), stream_ptr(dev)),
              "pmhip_guidance_combine")
    return out


def guidance_combine_dev(cond, uncond, scale_dev, out=None, with_stats=False):
    """guidance_combine with the scale read by the kernel from `scale_dev`, an fp32 tensor of one element on the operands' device
    (pmhip_guidance_combine_dev): for the same value the same bits as guidance_combine, logits and statistics.  The value is not
    checked: whoever wrote it checked it."""
    dev = _dev(cond, uncond, scale_dev)
    if cond.shape != uncond.shape or cond.dtype != torch.float32 or uncond.dtype != torch.float32:
        raise ValueError("guidance_combine_dev needs two fp32 tensors of one shape")
    if scale_dev.dtype != torch.float32 or scale_dev.numel() != 1:
        raise ValueError("guidance_combine_dev: scale_dev must be an fp32 tensor of one element on the operands' device")
    out = torch.empty(cond.shape, device=dev, dtype=torch.float32) if out is None else out
    if out.shape != cond.shape or out.dtype != torch.float32 or out.device != cond.device:
        raise ValueError("guidance_combine_dev: `out` must be an fp32 tensor of the inputs' shape on their device")
    if not (cond.is_contiguous() and uncond.is_contiguous() and out.is_contiguous()):
        raise ValueError("guidance_combine_dev needs contiguous tensors (the kernel walks them as flat arrays)")
    if cond.numel() % 4:
        raise ValueError("guidance_combine_dev: the element count must be a multiple of 4")
    stats = None
    if with_stats:
        if cond.shape[-1] % 64:
            raise ValueError("guidance_combine_dev(with_stats=True): rows must be a multiple of 64 long")
        stats = torch.empty(cond.shape[:-1] + (cond.shape[-1] // 64, 2), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(_lib.load().pmhip_guidance_combine_dev(_p(cond), _p(uncond), _p(scale_dev), _p(out), cond.numel(), _p(stats),
                                                     stream_ptr(dev)), "pmhip_guidance_combine_dev")
    return (out, stats) if with_stats else out


def guidance_scales(value, timesteps, what="guidance_scale"):
    """a guidance schedule (a sequence of `timesteps` numbers, one per step) -> a list of floats, checked as the native entry checks
    it: every scale finite"""
    vals = value.detach().reshape(-1).tolist() if isinstance(value, torch.Tensor) else list(value)
    if len(vals) != timesteps:
        raise ValueError(f"{what}: {len(vals)} scales for {timesteps} steps")
    out = [float(v) for v in vals]
    for i, v in enumerate(out):
        if not math.isfinite(v):
            raise ValueError(f"{what}: step {i}: the scale {v} must be finite")
    return out


def guidance_parts(guidance_scale, timesteps):
    """the ``guidance_scale`` keyword -> (scalar or None, schedule or None): a sequence is a loop's schedule, one scale per step
    (``guidance_scales``), which a single step -- timesteps None -- refuses; anything else, a 0-d array or tensor included, is one scale, as it came"""
    if isinstance(guidance_scale, (list, tuple, np.ndarray, torch.Tensor)) and np.ndim(guidance_scale) > 0:
        if timesteps is None:
            raise ValueError("guidance_scale: one step takes one scale (a sequence is a loop's schedule)")
        return None, guidance_scales(guidance_scale, timesteps)
    return guidance_scale, None


def embed_rows(table, ids, kpad, out_dtype):
    dev = _dev(table, ids)
    lib = _lib.load()
    V, E = table.shape
    M = ids.numel()
    out = torch.empty(M, kpad, device=dev, dtype=out_dtype)
    with torch.cuda.device(dev):
        check(lib.pmhip_embed_rows(_p(table), _p(ids), _p(out), pm_dtype(out_dtype), kpad, M, V, E, stream_ptr(dev)),
              "pmhip_embed_rows")
    return out


def vq_prepare(codebook):
    dev = _dev(codebook)
    lib = _lib.load()
    V, E = codebook.shape
    en = torch.empty_like(codebook)
    sq = torch.empty(V, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(lib.pmhip_vq_prepare(_p(codebook), _p(en), _p(sq), V, E, stream_ptr(dev)), "pmhip_vq_prepare")
    return en, sq


def vq_quantize(z, en, sq, beta=0.25):
    """z fp32 [M,E] -> (z_out [M,E], idx int64 [M], loss [1])."""
    dev = _dev(z, en, sq)
    lib = _lib.load()
    M, E = z.shape
    V = en.shape[0]
    z_out = torch.empty_like(z)
    idx = torch.empty(M, device=dev, dtype=torch.int64)
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    scratch = torch.empty(lib.pmhip_vq_scratch_bytes(M, V), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        check(lib.pmhip_vq_quantize(_p(z), _p(en), _p(sq), float(beta), _p(z_out), _p(idx), _p(loss), _p(scratch), M, V,
                                    E, stream_ptr(dev)), "pmhip_vq_quantize")
    return z_out, idx, loss


def nucleus_p(value, what="top_p"):
    """a nucleus mass (None = 1 = no filter) -> a float, checked as the native entries check it: finite, 0 < top_p <= 1"""
    p = 1.0 if value is None else float(value)
    if not (math.isfinite(p) and 0.0 < p <= 1.0):
        raise ValueError(f"{what}: {value} must be finite and in (0, 1]")
    return p


def sample_rows(logits, ids, mask_id, topk, temperature, noise=None, seed=0, step=0, row_base=0, block_stats=None, top_p=None):
    """logits fp32 [M,V], ids int64 [M] -> (pred [M], merged ids [M], score [M]).
    top_p: None or 1.0 = no nucleus filter (the kernels below, as without the keyword); 0 < top_p < 1, finite (else ValueError):
    of the top-k elements only those whose mass strictly above them is below top_p of the top-k's mass are drawn from -- the
    nucleus kernel for every topk (pmhip_sample_rows_nucleus), block_stats ignored.
    topk: 1..V.  Which kernel serves it depends on (V, topk) only: up to 8 (V % 64 == 0) the block-statistics kernel, up to 64 the
    row kernel with one candidate per lane, above 64 the selection kernel; block_stats are ignored above 8.
    block_stats fp32 [M, V/64, 2] (gemm_softmax_stats / guidance_combine(with_stats=True)): the kernel reads them and the top-k
    blocks of a row instead of the row; same bits as without."""
    nucleus = nucleus_p(top_p)
    dev = _dev(logits, ids, noise)
    lib = _lib.load()
    M, V = logits.shape
    pred = torch.empty(M, device=dev, dtype=torch.int64)
    ids_out = torch.empty(M, device=dev, dtype=torch.int64)
    score = torch.empty(M, device=dev, dtype=torch.float32)
    if nucleus < 1.0:
        with torch.cuda.device(dev):
            check(lib.pmhip_sample_rows_nucleus(_p(logits), logits.stride(0), _p(ids), int(mask_id), int(topk), nucleus, float(temperature),
                                                _p(noise), int(seed), int(step), int(row_base), _p(pred), _p(ids_out), _p(score),
                                                M, V, stream_ptr(dev)), "pmhip_sample_rows_nucleus")
        return pred, ids_out, score
    if block_stats is not None:
        if (block_stats.dtype != torch.float32 or not block_stats.is_contiguous() or block_stats.device != logits.device
                or tuple(block_stats.shape) != (M, V // 64, 2) or V % 64):
            raise ValueError("sample_rows: block_stats must be a contiguous fp32 [M, V/64, 2] tensor on the logits' device")
        with torch.cuda.device(dev):
            check(lib.pmhip_sample_rows_stats(_p(logits), logits.stride(0), _p(block_stats), _p(ids), int(mask_id), int(topk),
                                              float(temperature), _p(noise), int(seed), int(step), int(row_base), _p(pred),
                                              _p(ids_out), _p(score), M, V, stream_ptr(dev)), "pmhip_sample_rows_stats")
        return pred, ids_out, score
    with torch.cuda.device(dev):
        check(lib.pmhip_sample_rows(_p(logits), logits.stride(0), _p(ids), int(mask_id), int(topk), float(temperature),
                                    _p(noise), int(seed), int(step), int(row_base), _p(pred), _p(ids_out), _p(score),
                                    M, V, stream_ptr(dev)), "pmhip_sample_rows")
    return pred, ids_out, score


def sample_rows_forced(logits, ids, target, mask_id, ids_out=None):
    """The forced step (pmhip_sample_rows_forced): logits fp32 [M,V], ids int64 [M], target int64 [M] ->
    (pred [M], merged ids [M], score [M]) with pred = target, merged = target where ids == mask_id, score = 1 - softmax(logits)[target]
    there and -1e5 where the id was given: what ``sample_rows`` leaves for a row whose draw came out as `target`, bit for bit where
    that draw ran on the row, selection or nucleus kernel.  A target outside [0, V) leaves its row undrawn (pred = merged = ids,
    score = -1e5); the kernel tests the range in front of its load.  ids_out (None: a new tensor): where the merged ids go, `ids`
    itself for the step in place."""
    dev = _dev(logits, ids, target, ids_out)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError(f"sample_rows_forced: logits must be fp32 [M, V], got {logits.dtype} {tuple(logits.shape)}")
    M, V = logits.shape
    for name, x in (("ids", ids), ("target", target), ("ids_out", ids_out)):
        if x is not None and (x.dtype != torch.int64 or tuple(x.shape) != (M,)):
            raise ValueError(f"sample_rows_forced: {name} must be int64 [{M}], got {x.dtype} {tuple(x.shape)}")
    lib = _lib.load()
    pred = torch.empty(M, device=dev, dtype=torch.int64)
    if ids_out is None:
        ids_out = torch.empty(M, device=dev, dtype=torch.int64)
    score = torch.empty(M, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(lib.pmhip_sample_rows_forced(_p(logits), logits.stride(0), _p(ids), _p(target), int(mask_id), _p(pred), _p(ids_out), _p(score),
                                           M, V, stream_ptr(dev)), "pmhip_sample_rows_forced")
    return pred, ids_out, score


DIVERGENCE_KINDS = {"tv": 0, "jeffreys": 1}


def logit_divergence(a, b, ids=None, mask_id=None, kind="tv", out=None, accumulate=False):
    """The divergence between two rows of logits (pmhip_logit_divergence): a, b fp32 [M, V] on the device, unit
    column stride and one common row stride (a multiple of 4 elements; two halves of one tensor are served as they are, and a may be
    b) -> (acc f32 [M], count int32 [M]).  Row r is scored iff ids is None or ids[r] == mask_id (ids int64 [M], contiguous; mask_id
    comes with it).  kind "tv": 1/2 sum |p - q| in [0, 1]; "jeffreys": sum (p - q)(log p - log q) = KL(p||q) + KL(q||p); p, q the two
    rows' softmax.  A scored row: acc = d, count = 1; an unscored one: 0 and 0, its logits never loaded.  Under `accumulate` a scored
    row adds d and 1 to what `out` holds and an unscored row is left alone.  out (None: two new tensors; required under `accumulate`):
    the pair (acc, count), contiguous f32 [M] and int32 [M] on the operands' device.  a == b gives exactly 0; swapping a and b gives
    the same bits; two calls give the same bits.  Every argument fault is a ValueError in front of the launch.  -> out"""
    for name, x in (("a", a), ("b", b)):
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32:
            raise ValueError(f"logit_divergence: {name} must be an fp32 [M, V] tensor, got "
                             f"{(x.dtype, tuple(x.shape)) if isinstance(x, torch.Tensor) else type(x).__name__}")
    dev = a.device
    M, V = a.shape
    if tuple(b.shape) != (M, V) or b.device != dev:
        raise ValueError(f"logit_divergence: b must be an fp32 [{M}, {V}] tensor on a's device, got {tuple(b.shape)} on {b.device}")
    if M == 0 or V == 0 or V % 4 or V > 16384:
        raise ValueError(f"logit_divergence: M={M} must be positive and V={V} a multiple of 4 in (0, 16384]")
    ldl = a.stride(0) if M > 1 else V
    for name, x in (("a", a), ("b", b)):
        if x.stride(1) != 1 or (M > 1 and x.stride(0) != ldl) or ldl < V or ldl % 4 or x.data_ptr() % 16:
            raise ValueError(f"logit_divergence: {name} must have unit column stride, the common row stride (a multiple of 4, at least V={V}) and "
                             f"16-byte alignment, got strides {tuple(x.stride())}")
    if kind not in DIVERGENCE_KINDS:
        raise ValueError(f"logit_divergence: kind {kind!r} is neither 'tv' nor 'jeffreys'")
    if (ids is None) != (mask_id is None):
        raise ValueError("logit_divergence: ids and mask_id come together (ids=None scores every row)")
    if ids is not None:
        if not (isinstance(ids, torch.Tensor) and ids.dtype == torch.int64 and tuple(ids.shape) == (M,) and ids.is_contiguous() and ids.device == dev):
            raise ValueError(f"logit_divergence: ids must be a contiguous int64 [{M}] tensor on the operands' device")
        if isinstance(mask_id, bool) or not isinstance(mask_id, int):
            raise ValueError(f"logit_divergence: mask_id {mask_id!r} must be an integer")
    if out is None and accumulate:
        raise ValueError("accumulate adds to `out`: pass the pair of tensors to add to")
    if not a.is_cuda:                                          # (behind the argument checks: those hold without a device)
        raise _lib.PmhipError("paintmind_amd runs only on a ROCm device (got a CPU tensor); there is no CPU fallback")
    if out is None:
        out = (torch.empty(M, device=dev, dtype=torch.float32), torch.empty(M, device=dev, dtype=torch.int32))
    if not (isinstance(out, (tuple, list)) and len(out) == 2 and all(
            isinstance(o, torch.Tensor) and o.is_cuda and o.device == dev and o.dtype == dt and tuple(o.shape) == (M,) and o.is_contiguous()
            for o, dt in zip(out, (torch.float32, torch.int32)))):
        raise ValueError(f"out must be a pair of contiguous tensors (float32 [{M}], int32 [{M}]) on the operands' device")
    with torch.cuda.device(dev):
        check(_lib.load().pmhip_logit_divergence(_p(a), _p(b), int(ldl), _p(ids), int(mask_id or 0), DIVERGENCE_KINDS[kind], _p(out[0]), _p(out[1]),
                                                 int(bool(accumulate)), M, V, stream_ptr(dev)), "pmhip_logit_divergence")
    return out[0], out[1]


def token_logprob(logits, target, uncond=None, scale=None, ids=None, mask_id=None, out=None, accumulate=False, entropy=True, rank=True):
    """The model's likelihood of given tokens (pmhip_token_logprob): logits fp32 [M, V] on the device, unit
    column stride and a row stride that is a multiple of 4 elements; target int64 [M] -> (logp f32 [M], entropy f32 [M] or None,
    rank int32 [M] or None, count int32 [M]).  Row r is scored iff (ids is None or ids[r] == mask_id) and 0 <= target[r] < V (ids
    int64 [M], contiguous; mask_id comes with it); the kernel tests the range in front of its load.  uncond (fp32 [M, V], logits' row
    stride) with scale (a finite number; the two come together): the scored row is uncond + scale * (logits - uncond), formed at load
    by ``guidance_combine``'s expression, bit for bit.  A scored row: logp = log softmax(x)[target] <= 0, entropy = that of softmax(x)
    >= 0, rank = the target's place in the samplers' order (value descending, column ascending; rank < k iff topk = k keeps it),
    count = 1; an unscored one: 0 everywhere, its logits never loaded.  Under `accumulate` a scored row adds to what `out` holds
    and an unscored row is left alone.  entropy / rank False: that output is not computed into anything and comes back as None.
    out (None: new tensors; required under `accumulate`): the 4-tuple in the order of the result, None where entropy / rank is off,
    contiguous [M] tensors on the operands' device.  Two calls give the same bits.  Every argument fault is a ValueError in front of
    the launch.  -> out"""
    for name, x in (("logits", logits), ("uncond", uncond)):
        if x is not None and (not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32):
            raise ValueError(f"token_logprob: {name} must be an fp32 [M, V] tensor, got "
                             f"{(x.dtype, tuple(x.shape)) if isinstance(x, torch.Tensor) else type(x).__name__}")
    if logits is None:
        raise ValueError("token_logprob: logits must be an fp32 [M, V] tensor, got None")
    dev = logits.device
    M, V = logits.shape
    if M == 0 or V == 0 or V % 4 or V > 16384:
        raise ValueError(f"token_logprob: M={M} must be positive and V={V} a multiple of 4 in (0, 16384]")
    if (uncond is None) != (scale is None):
        raise ValueError("token_logprob: uncond and scale come together (neither: the plain logits are scored)")
    if uncond is not None:
        if tuple(uncond.shape) != (M, V) or uncond.device != dev:
            raise ValueError(f"token_logprob: uncond must be an fp32 [{M}, {V}] tensor on the logits' device, got {tuple(uncond.shape)} on {uncond.device}")
        if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale):
            raise ValueError(f"token_logprob: scale {scale!r} must be a finite number")
    ldl = logits.stride(0) if M > 1 else V
    for name, x in (("logits", logits), ("uncond", uncond)):
        if x is not None and (x.stride(1) != 1 or (M > 1 and x.stride(0) != ldl) or ldl < V or ldl % 4 or x.data_ptr() % 16):
            raise ValueError(f"token_logprob: {name} must have unit column stride, the common row stride (a multiple of 4, at least V={V}) and "
                             f"16-byte alignment, got strides {tuple(x.stride())}")
    if not (isinstance(target, torch.Tensor) and target.dtype == torch.int64 and tuple(target.shape) == (M,) and target.is_contiguous()
            and target.device == dev):
        raise ValueError(f"token_logprob: target must be a contiguous int64 [{M}] tensor on the logits' device")
    if (ids is None) != (mask_id is None):
        raise ValueError("token_logprob: ids and mask_id come together (ids=None scores every row with a target in range)")
    if ids is not None:
        if not (isinstance(ids, torch.Tensor) and ids.dtype == torch.int64 and tuple(ids.shape) == (M,) and ids.is_contiguous() and ids.device == dev):
            raise ValueError(f"token_logprob: ids must be a contiguous int64 [{M}] tensor on the logits' device")
        if isinstance(mask_id, bool) or not isinstance(mask_id, int):
            raise ValueError(f"token_logprob: mask_id {mask_id!r} must be an integer")
    if out is None and accumulate:
        raise ValueError("accumulate adds to `out`: pass the tensors to add to")
    if not logits.is_cuda:                                     # (behind the argument checks: those hold without a device)
        raise _lib.PmhipError("paintmind_amd runs only on a ROCm device (got a CPU tensor); there is no CPU fallback")
    want = (torch.float32, torch.float32 if entropy else None, torch.int32 if rank else None, torch.int32)
    if out is None:
        out = tuple(None if dt is None else torch.empty(M, device=dev, dtype=dt) for dt in want)
    if not (isinstance(out, (tuple, list)) and len(out) == 4 and all(
            (o is None) if dt is None else (isinstance(o, torch.Tensor) and o.is_cuda and o.device == dev and o.dtype == dt
                                            and tuple(o.shape) == (M,) and o.is_contiguous()) for o, dt in zip(out, want))):
        raise ValueError(f"out must be (float32 [{M}], float32 [{M}] or None without entropy, int32 [{M}] or None without rank, int32 [{M}]): "
                         f"contiguous tensors on the operands' device")
    with torch.cuda.device(dev):
        check(_lib.load().pmhip_token_logprob(_p(logits), _p(uncond), float(scale or 0.0), int(ldl), _p(ids), int(mask_id or 0), _p(target),
                                              _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), int(bool(accumulate)), M, V, stream_ptr(dev)),
              "pmhip_token_logprob")
    return tuple(out)


class CanvasTables(NamedTuple):
    """the tables of a ``canvas.CanvasLayout`` on one device, as the two canvas operators take them"""
    cover: torch.Tensor        # int32 [Nc, K]
    weight: torch.Tensor       # f32 [Nc, K]
    gather: torch.Tensor       # int64 [W, g^2]
    ywin: torch.Tensor         # int32 [Hc, 4]
    yw: torch.Tensor           # f32 [Hc, 4]
    xwin: torch.Tensor         # int32 [Wc, 4]
    xw: torch.Tensor           # f32 [Wc, 4]
    yoff: torch.Tensor         # int32 [ny]
    xoff: torch.Tensor         # int32 [nx]


_canvas_tables = {}


def canvas_tables(layout, device):
    """``CanvasTables`` of `layout` on `device`: copied once per (layout, device) and kept as long as the layout lives"""
    import weakref
    key = (id(layout), str(device))
    hit = _canvas_tables.get(key)
    if hit is None or hit[0]() is not layout:
        arrays = (layout.cover, layout.weight, layout.gather, *layout.pixel_y, *layout.pixel_x, layout.pixel_off_y, layout.pixel_off_x)
        tables = CanvasTables(*(torch.from_numpy(np.array(a)).to(device).contiguous() for a in arrays))
        _canvas_tables[key] = hit = (weakref.ref(layout, lambda _, k=key: _canvas_tables.pop(k, None)), tables)
    return hit[1]


def window_logits(win, cover, weight, window_rows, uncond=None, scale=None, out=None):
    """The canvas logits from the window logits (pmhip_window_logits).  win fp32 [B * window_rows, V] on the
    device, unit column stride, a row stride that is a multiple of 4 elements: canvas b's window rows are [b * window_rows, (b + 1) *
    window_rows).  cover int32 [Nc, K] / weight fp32 [Nc, K] (1 <= K <= 16; ``canvas_tables``): the window rows that cover canvas
    token t, ascending, padded with -1.  uncond (fp32, win's shape and strides) with scale (a finite number; the two come together):
    the element used is uncond + scale * (win - uncond), formed at load by ``guidance_combine``'s expression, bit for bit.
    -> out fp32 [B * Nc, V] (None: a new contiguous tensor; else unit column stride and a row stride that is a multiple of 4):
    out[b * Nc + t] = w_0 x_0, then fma(w_k, x_k, .) over the entries in [0, window_rows), ascending.  An entry outside that range is
    skipped in front of its load.  Deterministic: two calls give the same bits.  Every argument fault is a ValueError in front of the
    launch."""
    for name, x in (("win", win), ("uncond", uncond)):
        if x is not None and (not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32):
            raise ValueError(f"window_logits: {name} must be an fp32 [rows, V] tensor, got "
                             f"{(x.dtype, tuple(x.shape)) if isinstance(x, torch.Tensor) else type(x).__name__}")
    if win is None:
        raise ValueError("window_logits: win must be an fp32 [rows, V] tensor, got None")
    dev = win.device
    M, V = win.shape
    window_rows = int(window_rows)
    if window_rows < 1 or M == 0 or M % window_rows:
        raise ValueError(f"window_logits: the {M} rows of win must be a positive multiple of window_rows={window_rows}")
    B = M // window_rows
    if V == 0 or V % 4:
        raise ValueError(f"window_logits: V={V} must be a positive multiple of 4")
    if (uncond is None) != (scale is None):
        raise ValueError("window_logits: uncond and scale come together (neither: the plain window logits are fused)")
    if uncond is not None:
        if tuple(uncond.shape) != (M, V) or uncond.device != dev:
            raise ValueError(f"window_logits: uncond must be an fp32 [{M}, {V}] tensor on win's device, got {tuple(uncond.shape)} on {uncond.device}")
        if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale):
            raise ValueError(f"window_logits: scale {scale!r} must be a finite number")
    ldw = win.stride(0) if M > 1 else V
    for name, x in (("win", win), ("uncond", uncond)):
        if x is not None and (x.stride(1) != 1 or (M > 1 and x.stride(0) != ldw) or ldw < V or ldw % 4 or x.data_ptr() % 16):
            raise ValueError(f"window_logits: {name} must have unit column stride, the common row stride (a multiple of 4, at least V={V}) and "
                             f"16-byte alignment, got strides {tuple(x.stride())}")
    if not (isinstance(cover, torch.Tensor) and cover.dtype == torch.int32 and cover.dim() == 2 and cover.is_contiguous() and cover.device == dev
            and 1 <= cover.shape[1] <= 16 and cover.shape[0] > 0):
        raise ValueError("window_logits: cover must be a contiguous int32 [Nc, K] tensor on win's device, 1 <= K <= 16")
    Nc, K = cover.shape
    if not (isinstance(weight, torch.Tensor) and weight.dtype == torch.float32 and tuple(weight.shape) == (Nc, K) and weight.is_contiguous()
            and weight.device == dev):
        raise ValueError(f"window_logits: weight must be a contiguous fp32 [{Nc}, {K}] tensor on win's device")
    if not win.is_cuda:                                        # (behind the argument checks: those hold without a device)
        raise _lib.PmhipError("paintmind_amd runs only on a ROCm device (got a CPU tensor); there is no CPU fallback")
    rows = B * Nc
    if out is None:
        out = torch.empty(rows, V, device=dev, dtype=torch.float32)
    if not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == (rows, V) and out.device == dev
            and out.stride(1) == 1 and (rows == 1 or (out.stride(0) >= V and out.stride(0) % 4 == 0)) and out.data_ptr() % 16 == 0):
        raise ValueError(f"window_logits: out must be an fp32 [{rows}, {V}] tensor on win's device with unit column stride, a row stride that is a "
                         f"multiple of 4 and 16-byte alignment")
    ldo = out.stride(0) if rows > 1 else V
    with torch.cuda.device(dev):
        check(_lib.load().pmhip_window_logits(_p(win), _p(uncond), float(scale or 0.0), int(ldw), _p(cover), _p(weight), K, window_rows, _p(out),
                                              int(ldo), B, Nc, V, stream_ptr(dev)), "pmhip_window_logits")
    return out


def window_pixels(img, tables, out=None):
    """The canvas image from the decoded window images (pmhip_window_pixels).  img fp32 [B * W, C, S, S] on the
    device, canvas b's W = ny * nx windows row-major in front of canvas b + 1's; tables: the layout's ``CanvasTables`` on that device
    (``canvas_tables``).  -> out fp32 [B, C, Hc, Wc]: per pixel the sum over the windows that cover it of rn(ay ax) * pixel, rows
    ascending outside and columns ascending inside, fused multiply-adds behind the first product, clamped to [-1, 1] like
    ``unpatchify_clamp``.  A pixel one window covers is that window's pixel, bit for bit."""
    if not isinstance(img, torch.Tensor) or img.dim() != 4 or img.dtype != torch.float32 or img.shape[2] != img.shape[3]:
        raise ValueError(f"window_pixels: img must be an fp32 [B * W, C, S, S] tensor, got "
                         f"{(img.dtype, tuple(img.shape)) if isinstance(img, torch.Tensor) else type(img).__name__}")
    if not isinstance(tables, CanvasTables):
        raise ValueError(f"window_pixels: tables must be the layout's CanvasTables (canvas_tables), got {type(tables).__name__}")
    ny, nx, Hc, Wc = tables.yoff.shape[0], tables.xoff.shape[0], tables.ywin.shape[0], tables.xwin.shape[0]
    for name, x, dt, shape in (("ywin", tables.ywin, torch.int32, (Hc, 4)), ("yw", tables.yw, torch.float32, (Hc, 4)),
                               ("xwin", tables.xwin, torch.int32, (Wc, 4)), ("xw", tables.xw, torch.float32, (Wc, 4)),
                               ("yoff", tables.yoff, torch.int32, (ny,)), ("xoff", tables.xoff, torch.int32, (nx,))):
        if x.dtype != dt or tuple(x.shape) != shape or not x.is_contiguous() or x.device != img.device:
            raise ValueError(f"window_pixels: tables.{name} must be a contiguous {dt} {list(shape)} tensor on img's device, got {x.dtype} "
                             f"{tuple(x.shape)} on {x.device}")
    n, Cc, S, _ = img.shape
    if n == 0 or ny == 0 or nx == 0 or n % (ny * nx):
        raise ValueError(f"window_pixels: {n} window images are no positive multiple of the layout's {ny} x {nx} windows")
    B = n // (ny * nx)
    if Hc < S or Wc < S:
        raise ValueError(f"window_pixels: the canvas {Hc} x {Wc} is smaller than a window image ({S} x {S})")
    if not img.is_contiguous():
        raise ValueError("window_pixels: img must be contiguous")
    if out is not None and not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == (B, Cc, Hc, Wc)
                                and out.is_contiguous() and out.device == img.device):
        raise ValueError(f"window_pixels: out must be a contiguous fp32 [{B}, {Cc}, {Hc}, {Wc}] tensor on img's device")
    dev = _dev(img)
    if out is None:
        out = torch.empty(B, Cc, Hc, Wc, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(_lib.load().pmhip_window_pixels(_p(img), _p(tables.ywin), _p(tables.yw), _p(tables.xwin), _p(tables.xw), _p(tables.yoff),
                                              _p(tables.xoff), _p(out), B, Cc, S, ny, nx, Hc, Wc, stream_ptr(dev)), "pmhip_window_pixels")
    return out


def choice_t(value, what="choice_temperature"):
    """a step's choice temperature (None = 0) -> a float, checked as the native entries check it: finite, 0 <= t <= CHOICE_T_MAX"""
    t = 0.0 if value is None else float(value)
    if not (math.isfinite(t) and 0.0 <= t <= _lib.CHOICE_T_MAX):
        raise ValueError(f"{what}: {value} must be finite and in [0, {_lib.CHOICE_T_MAX:g}]")
    return t


def remask(ids, scores, num_mask, mask_id, choice_temperature=0.0, noise=None, seed=0, step=0, row_base=0):
    """in place on ids int64 [B,N].
    choice_temperature (this step's value; 0 = the plain re-masking): MaskGIT's perturbed confidence -- a taken position sorts by
    -(log(max(1 - score, 2^-24)) + t * gumbel(u)), a given one (score < 0) by its score (pmhip_remask_choice).  u: `noise` fp32
    [B,N] uniform(0,1), or Philox under (seed, step, row_base + b*N + i) at the column word 0xFFFFFFFF."""
    dev = _dev(ids, scores, noise)
    lib = _lib.load()
    B, N = ids.shape
    t = choice_t(choice_temperature)
    if noise is not None and (noise.dtype != torch.float32 or tuple(noise.shape) != (B, N)):
        raise ValueError(f"remask: noise must be a contiguous fp32 [{B}, {N}] tensor on the operands' device")
    with torch.cuda.device(dev):
        if t == 0.0 and noise is None:
            check(lib.pmhip_remask(_p(ids), _p(scores), int(num_mask), int(mask_id), B, N, stream_ptr(dev)), "pmhip_remask")
        else:
            check(lib.pmhip_remask_choice(_p(ids), _p(scores), int(num_mask), int(mask_id), B, N, t, _p(noise), int(seed), int(step),
                                          int(row_base), stream_ptr(dev)), "pmhip_remask_choice")
    return ids


def remask_counts(ids, scores, counts, mask_id, choice_temperature=0.0, noise=None, seed=0, step=0, row_base=0):
    """remask with a count PER IMAGE, in place on ids int64 [B,N]: counts int32 [B] on the device; row b equals remask on that
    row alone with num_mask = counts[b] (noise at row_base + b * N), and a count of 0 leaves the row untouched
    (pmhip_remask_counts / pmhip_remask_choice_counts).  The other keywords: as in ``remask``."""
    dev = _dev(ids, scores, counts, noise)
    lib = _lib.load()
    B, N = ids.shape
    t = choice_t(choice_temperature)
    if counts.dtype != torch.int32 or tuple(counts.shape) != (B,) or not counts.is_contiguous():
        raise ValueError(f"remask_counts: counts must be a contiguous int32 [{B}] tensor on the operands' device")
    if noise is not None and (noise.dtype != torch.float32 or tuple(noise.shape) != (B, N)):
        raise ValueError(f"remask_counts: noise must be a contiguous fp32 [{B}, {N}] tensor on the operands' device")
    with torch.cuda.device(dev):
        if t == 0.0 and noise is None:
            check(lib.pmhip_remask_counts(_p(ids), _p(scores), _p(counts), int(mask_id), B, N, stream_ptr(dev)), "pmhip_remask_counts")
        else:
            check(lib.pmhip_remask_choice_counts(_p(ids), _p(scores), _p(counts), int(mask_id), B, N, t, _p(noise), int(seed), int(step),
                                                 int(row_base), stream_ptr(dev)), "pmhip_remask_choice_counts")
    return ids


def mask_tokens(pixel_mask, patch, ids, mask_id):
    """pixel mask -> token mask, in place on ids int64 [B, (H/patch) * (W/patch)]: pixel_mask uint8 [B,H,W]; a token whose patch
    holds ANY non-zero pixel gets mask_id.  -> (ids, counts int32 [B]: how many tokens of each image did)."""
    dev = _dev(pixel_mask, ids)
    if pixel_mask.dtype != torch.uint8 or pixel_mask.dim() != 3 or not pixel_mask.is_contiguous():
        raise ValueError("mask_tokens: pixel_mask must be a contiguous uint8 [B, H, W] tensor")
    B, H, W = pixel_mask.shape
    if patch <= 0 or H % patch or W % patch:
        raise ValueError(f"mask_tokens: H={H} and W={W} must be multiples of patch={patch}")
    if ids.dtype != torch.int64 or tuple(ids.shape) != (B, (H // patch) * (W // patch)) or not ids.is_contiguous():
        raise ValueError(f"mask_tokens: ids must be a contiguous int64 [{B}, {(H // patch) * (W // patch)}] tensor")
    counts = torch.empty(B, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        check(_lib.load().pmhip_mask_tokens(_p(pixel_mask), int(patch), _p(ids), int(mask_id), _p(counts), B, H, W, stream_ptr(dev)),
              "pmhip_mask_tokens")
    return ids, counts


def composite(gen, orig, pixel_mask, out=None):
    """where(pixel_mask != 0, gen, orig): gen, orig fp32 [B,C,H,W], pixel_mask uint8 [B,H,W] broadcast over C; `out` (default: a
    new tensor) may be gen."""
    dev = _dev(gen, orig, pixel_mask)
    if gen.dim() != 4 or gen.shape != orig.shape or gen.dtype != torch.float32 or orig.dtype != torch.float32:
        raise ValueError("composite needs two fp32 [B, C, H, W] tensors of one shape")
    B, Cn, H, W = gen.shape
    if pixel_mask.dtype != torch.uint8 or tuple(pixel_mask.shape) != (B, H, W):
        raise ValueError(f"composite: pixel_mask must be a uint8 [{B}, {H}, {W}] tensor")
    out = torch.empty_like(gen) if out is None else out
    if out.shape != gen.shape or out.dtype != torch.float32 or out.device != gen.device:
        raise ValueError("composite: `out` must be an fp32 tensor of the inputs' shape on their device")
    if not (gen.is_contiguous() and orig.is_contiguous() and pixel_mask.is_contiguous() and out.is_contiguous()):
        raise ValueError("composite needs contiguous tensors (the kernel walks them as flat arrays)")
    with torch.cuda.device(dev):
        check(_lib.load().pmhip_composite(_p(gen), _p(orig), _p(pixel_mask), _p(out), B, Cn, H, W, stream_ptr(dev)), "pmhip_composite")
    return out


def pack_slots(records, device=None):
    """[(seed, image_index, temperature, topk, num_mask, step) or None (idle), ...] -> the pmhip_slot array as a uint8 tensor
    [B, 32] (on `device` when given): what sample_rows_slots / remask_slots read."""
    arr = (_lib.Slot * len(records))()
    for i, r in enumerate(records):
        if r is None:
            arr[i].step = _lib.SLOT_IDLE
            continue
        seed, image_index, temperature, topk, num_mask, step = r
        arr[i] = _lib.Slot(int(seed) & (2 ** 64 - 1), int(image_index) & (2 ** 64 - 1), float(temperature), int(topk), int(num_mask), int(step))
    t = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).reshape(len(records), C.sizeof(_lib.Slot))
    return t if device is None else t.to(device)


def _check_slots(slots, B, dev):
    if (slots.dtype != torch.uint8 or not slots.is_contiguous() or slots.device != dev
            or tuple(slots.shape) != (B, C.sizeof(_lib.Slot))):
        raise ValueError(f"slots must be a contiguous uint8 [{B}, {C.sizeof(_lib.Slot)}] tensor (pack_slots) on the operands' device")


def sample_rows_slots(logits, ids, mask_id, slots, tokens, block_stats=None, top_p=None, filters=False):
    """sample_rows with the scalars of row r taken from slots[r // tokens] (pack_slots): logits fp32 [B*tokens, V], ids int64
    [B*tokens] -> (pred, merged ids, score).  Image b equals sample_rows on its rows alone with its slot's values and
    row_base = image_index * tokens, bit for bit; an idle slot keeps its ids (pred = ids, score = -1e5).  V % 64 == 0, topk <= 8.
    filters=True (pmhip_sample_rows_slots_filter): a slot's topk may be anywhere in 1..V and `top_p`, fp32 [B]
    on the device (None: every slot 1), gives every slot its nucleus mass -- image b then equals sample_rows(..., topk, top_p=) on
    its rows, on the kernel that call picks (block_stats are read for the slots at topk <= 8 without a nucleus only)."""
    dev = _dev(logits, ids, slots, block_stats, top_p)
    lib = _lib.load()
    M, V = logits.shape
    if tokens <= 0 or M % tokens:
        raise ValueError(f"sample_rows_slots: {M} rows are not a whole number of images of {tokens} tokens")
    _check_slots(slots, M // tokens, dev)
    if block_stats is not None and (block_stats.dtype != torch.float32 or tuple(block_stats.shape) != (M, V // 64, 2) or V % 64):
        raise ValueError("sample_rows_slots: block_stats must be a contiguous fp32 [M, V/64, 2] tensor on the logits' device")
    if top_p is not None:
        if not filters:
            raise ValueError("sample_rows_slots: top_p needs filters=True (the entry without filters has no nucleus)")
        if top_p.dtype != torch.float32 or tuple(top_p.shape) != (M // tokens,) or not top_p.is_contiguous():
            raise ValueError(f"sample_rows_slots: top_p must be a contiguous fp32 [{M // tokens}] tensor on the operands' device")
    pred = torch.empty(M, device=dev, dtype=torch.int64)
    ids_out = torch.empty(M, device=dev, dtype=torch.int64)
    score = torch.empty(M, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        if filters:
            check(lib.pmhip_sample_rows_slots_filter(_p(logits), logits.stride(0), _p(block_stats), _p(ids), int(mask_id), _p(slots), _p(top_p),
                                                     int(tokens), _p(pred), _p(ids_out), _p(score), M, V, stream_ptr(dev)),
                  "pmhip_sample_rows_slots_filter")
        else:
            check(lib.pmhip_sample_rows_slots(_p(logits), logits.stride(0), _p(block_stats), _p(ids), int(mask_id), _p(slots), int(tokens),
                                              _p(pred), _p(ids_out), _p(score), M, V, stream_ptr(dev)), "pmhip_sample_rows_slots")
    return pred, ids_out, score


def remask_slots(ids, scores, slots, mask_id, choice=None):
    """remask with num_mask = slot b's, in place on ids int64 [B,N]; the row of an idle slot is left untouched.
    choice (None = the plain re-masking): fp32 [B] on the device, image b's choice temperature of this step (0: the plain key);
    seed, step and image index of the Philox stream come from the slot (pmhip_remask_choice_slots)."""
    dev = _dev(ids, scores, slots, choice)
    lib = _lib.load()
    B, N = ids.shape
    _check_slots(slots, B, dev)
    with torch.cuda.device(dev):
        if choice is None:
            check(lib.pmhip_remask_slots(_p(ids), _p(scores), _p(slots), int(mask_id), B, N, stream_ptr(dev)), "pmhip_remask_slots")
        else:
            if choice.dtype != torch.float32 or tuple(choice.shape) != (B,):
                raise ValueError(f"remask_slots: choice must be a contiguous fp32 [{B}] tensor on the operands' device")
            check(lib.pmhip_remask_choice_slots(_p(ids), _p(scores), _p(slots), _p(choice), int(mask_id), B, N, stream_ptr(dev)),
                  "pmhip_remask_choice_slots")
    return ids


def remask_slots_counts(ids, scores, slots, counts, mask_id, choice=None):
    """remask_slots with a count PER SLOT, in place on ids int64 [B,N]: counts int32 [B] on the device.  counts[b] < 0: slot b's
    num_mask, as remask_slots does it; 0: the row untouched; > 0: exactly that many positions, as remask_counts does it on that row
    alone with the slot's seed, step and row_base = image_index * N; the row of an idle slot is left untouched whatever its count.
    choice: as in ``remask_slots`` (pmhip_remask_slots_counts / pmhip_remask_choice_slots_counts)."""
    dev = _dev(ids, scores, slots, counts, choice)
    lib = _lib.load()
    B, N = ids.shape
    _check_slots(slots, B, dev)
    if counts.dtype != torch.int32 or tuple(counts.shape) != (B,) or not counts.is_contiguous():
        raise ValueError(f"remask_slots_counts: counts must be a contiguous int32 [{B}] tensor on the operands' device")
    with torch.cuda.device(dev):
        if choice is None:
            check(lib.pmhip_remask_slots_counts(_p(ids), _p(scores), _p(slots), _p(counts), int(mask_id), B, N, stream_ptr(dev)),
                  "pmhip_remask_slots_counts")
        else:
            if choice.dtype != torch.float32 or tuple(choice.shape) != (B,):
                raise ValueError(f"remask_slots_counts: choice must be a contiguous fp32 [{B}] tensor on the operands' device")
            check(lib.pmhip_remask_choice_slots_counts(_p(ids), _p(scores), _p(slots), _p(choice), _p(counts), int(mask_id), B, N,
                                                       stream_ptr(dev)), "pmhip_remask_choice_slots_counts")
    return ids


def pack_slot_guides(scales, device=None, kinds=None):
    """[guidance scale or None (not guided), ...] -> the pmhip_slot_guide array as a uint8 tensor [B, 8] (on `device` when given):
    what guidance_combine_slots reads, one record beside every pack_slots record.  kinds (None: 1 for every guided image): the
    record's `on` per guided image -- 1 guided against the pass without a context, 2 against the negative context."""
    arr = (_lib.SlotGuide * len(scales))()
    if kinds is not None and len(kinds) != len(scales):
        raise ValueError(f"pack_slot_guides: {len(kinds)} kinds for {len(scales)} scales")
    for i, sc in enumerate(scales):
        if sc is not None:
            arr[i] = _lib.SlotGuide(float(sc), 1 if kinds is None else int(kinds[i]))
    t = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).reshape(len(scales), C.sizeof(_lib.SlotGuide))
    return t if device is None else t.to(device)


def guidance_combine_slots(cond, uncond, guides, slots, tokens, out=None, block_stats=None, which=None):
    """guidance_combine with the scale of row r taken from guides[r // tokens] (pack_slot_guides): cond, uncond fp32
    [B*tokens, V] -> `out` (default: a new tensor; may be cond), and `block_stats` fp32 [B*tokens, V/64, 2] when given.  The rows
    of an image that is guided and whose slot (pack_slots) is active equal guidance_combine(with_stats=True) on that image alone,
    bit for bit; the rows of every other image are neither read nor written: `out` and `block_stats` keep what they held.
    V % 64 == 0.
    which (None: every active image whose record has a non-zero `on`): 1 or 2 -- only the active images whose `on` EQUALS it are
    combined (pmhip_guidance_combine_slots_which), `uncond` then being the plane of that kind: the pass without a context for 1,
    the pass against the negative context for 2."""
    dev = _dev(cond, uncond, guides, slots, out, block_stats)
    if which is not None and which not in (1, 2):
        raise ValueError(f"guidance_combine_slots: which={which!r} must be None, 1 or 2")
    lib = _lib.load()
    if cond.dim() != 2 or cond.shape != uncond.shape or cond.dtype != torch.float32 or uncond.dtype != torch.float32:
        raise ValueError("guidance_combine_slots needs two fp32 [M, V] tensors of one shape")
    M, V = cond.shape
    if tokens <= 0 or M % tokens:
        raise ValueError(f"guidance_combine_slots: {M} rows are not a whole number of images of {tokens} tokens")
    B = M // tokens
    _check_slots(slots, B, dev)
    if (guides.dtype != torch.uint8 or not guides.is_contiguous() or guides.device != dev
            or tuple(guides.shape) != (B, C.sizeof(_lib.SlotGuide))):
        raise ValueError(f"guides must be a contiguous uint8 [{B}, {C.sizeof(_lib.SlotGuide)}] tensor (pack_slot_guides) on the operands' device")
    out = torch.empty_like(cond) if out is None else out
    if out.shape != cond.shape or out.dtype != torch.float32 or out.device != cond.device:
        raise ValueError("guidance_combine_slots: `out` must be an fp32 tensor of the inputs' shape on their device")
    if not (cond.is_contiguous() and uncond.is_contiguous() and out.is_contiguous()):
        raise ValueError("guidance_combine_slots needs contiguous tensors (rows of V consecutive elements)")
    if block_stats is not None and (block_stats.dtype != torch.float32 or not block_stats.is_contiguous()
                                    or tuple(block_stats.shape) != (M, V // 64, 2) or V % 64):
        raise ValueError("guidance_combine_slots: block_stats must be a contiguous fp32 [M, V/64, 2] tensor on the inputs' device")
    with torch.cuda.device(dev):
        if which is None:
            check(lib.pmhip_guidance_combine_slots(_p(cond), _p(uncond), _p(guides), _p(slots), int(tokens), _p(out), _p(block_stats), M, V,
                                                   stream_ptr(dev)), "pmhip_guidance_combine_slots")
        else:
            check(lib.pmhip_guidance_combine_slots_which(_p(cond), _p(uncond), _p(guides), _p(slots), int(which), int(tokens), _p(out),
                                                         _p(block_stats), M, V, stream_ptr(dev)), "pmhip_guidance_combine_slots_which")
    return out if block_stats is None else (out, block_stats)


def random_mask(z, noise, mask_token, len_keep):
    """z fp32 [B,N,E], noise fp32 [B,N], mask_token fp32 [E] -> (x [B,N,E], mask [B,N] with 1 = masked)."""
    dev = _dev(z, noise, mask_token)
    lib = _lib.load()
    B, N, E = z.shape
    x = torch.empty_like(z)
    mask = torch.empty(B, N, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(lib.pmhip_random_mask(_p(z), _p(noise), _p(mask_token), int(len_keep), _p(x), _p(mask), B, N, E,
                                    stream_ptr(dev)), "pmhip_random_mask")
    return x, mask


def masked_ce(logits, labels, mask, label_smoothing=0.1):
    """logits fp32 [M,V], labels int64 [M], mask fp32 [M] -> (loss [1], row_loss [M])."""
    dev = _dev(logits, labels, mask)
    lib = _lib.load()
    M, V = logits.shape
    row_loss = torch.empty(M, device=dev, dtype=torch.float32)
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(lib.pmhip_masked_ce(_p(logits), logits.stride(0), _p(labels), _p(mask), float(label_smoothing), _p(row_loss),
                                  _p(loss), M, V, stream_ptr(dev)), "pmhip_masked_ce")
    return loss, row_loss


# ------------------------------------------------------------------------------------------------
def timing_enable(on=True):
    check(_lib.load().pmhip_timing_enable(int(on)))


def timing_reset():
    check(_lib.load().pmhip_timing_reset())


def timing_get(family):
    n = C.c_int(0)
    ms = C.c_double(0.0)
    check(_lib.load().pmhip_timing_get(family.encode(), C.byref(n), C.byref(ms)), "pmhip_timing_get")
    return n.value, ms.value


def device_info(device=0):
    cu = C.c_int(0)
    lds = C.c_int(0)
    arch = C.create_string_buffer(64)
    check(_lib.load().pmhip_device_info(int(device), C.byref(cu), C.byref(lds), arch, 64), "pmhip_device_info")
    return {"cu_count": cu.value, "lds_bytes": lds.value, "arch": arch.value.decode()}


LOG2E = math.log2(math.e)
__all__ = [n for n in dir() if not n.startswith("_")]
