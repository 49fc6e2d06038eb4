"""Attention operator for the reference's plug-point.

The reference selects its attention class through ``Layer.ATTENTION_MODES`` (reference
stage1/layers.py:41-48, stage2/transformer.py:29-36) with two interchangeable entries,
``CrossAttention`` and ``MemoryEfficientCrossAttention`` (modules/attention.py:25-108).  This
class is the third implementation of the same contract: same constructor signature, same
``forward(x, context=None)``, same state_dict keys (to_q/to_k/to_v/to_out.0), with the arithmetic
done by libpaintmind_hip.so: fused q|k|v projection with head-split epilogue, flash-style
softmax(QK^T)V that never materialises the score matrix, and an out-projection with fused bias
(+ residual when called from a Layer).
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import ops, packing

XFORMERS_IS_AVAILBLE = False   # name kept for source compatibility (reference attention.py:7-12)


class CrossAttention(nn.Module):
    def __init__(self, query_dim, context_dim=None, heads=8, dim_head=64, dropout=0.):
        super().__init__()
        if dim_head % 16 or not 16 <= dim_head <= 128 or (dim_head * heads) % 64:
            raise ValueError(f"dim_head={dim_head}, heads={heads}: the HIP operators serve dim_head = 16, 32, ..., 128 with "
                             f"heads*dim_head a multiple of 64 (64 runs the tuned MFMA kernels, the rest a plain path)")
        inner_dim = dim_head * heads
        context_dim = query_dim if context_dim is None else context_dim
        self.scale = dim_head ** -0.5
        self.heads = heads
        self.dim_head = dim_head
        self.query_dim = query_dim
        self.context_dim = context_dim
        # creation order == the reference's, so a seeded construction draws identical weights
        self.to_q = nn.Linear(query_dim, inner_dim, bias=False)
        self.to_k = nn.Linear(context_dim, inner_dim, bias=False)
        self.to_v = nn.Linear(context_dim, inner_dim, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner_dim, query_dim), nn.Dropout(dropout))
        self._pack = None

    # -- packed weights, rebuilt whenever a parameter changes ---------------------------------------
    def packed(self, dtype):
        stamp = (packing.params_fingerprint(self), dtype)
        if self._pack is None or self._pack[0] != stamp:
            qd, cd = round_up64(self.query_dim), round_up64(self.context_dim)
            pk = {
                "wq": packing.pad_cols(self.to_q.weight, qd, dtype),
                "wkv": torch.cat([packing.pad_cols(self.to_k.weight, cd, dtype),
                                  packing.pad_cols(self.to_v.weight, cd, dtype)], dim=0),
                "wo": packing.cast(self.to_out[0].weight, dtype),
                "bo": packing.cast(self.to_out[0].bias, torch.float32),
            }
            if qd == cd:
                pk["wqkv"] = torch.cat([pk["wq"], pk["wkv"]], dim=0)
            self._pack = (stamp, pk)
        return self._pack[1]

    def forward(self, x, context=None, context_lens=None, context_segments=None, token_segments=None, context_weights=None):
        return self.run(x, context, residual=None, context_lens=context_lens, context_segments=context_segments,
                        token_segments=token_segments, context_weights=context_weights)

    def run(self, x, context=None, residual=None, context_lens=None, context_segments=None, token_segments=None, context_weights=None,
            want_maps=False, control=None, inject_self=False, keys=None, score=None):
        """x [B,N,query_dim]; returns to_out(attn) (+ residual) as fp32/bf16 like x.
        want_maps (extension, attention maps): -> (that, maps) with maps f32 [B, N, L], the mean over the heads
        of this call's softmax probabilities -- exactly 0 where a row takes no part; it needs a context.
        context_lens (extension; None = the reference's behaviour, no mask): one length per image -- image b attends to rows
        [0, context_lens[b]) of its context only; the rows beyond never reach the result, NaN included.
        context_segments [B, L] + token_segments [B, N] (extension, regional prompts; never beside context_lens): row k of image
        b's context belongs to segment context_segments[b, k] (0..31; -1 or 255 = padding, which never reaches the result), and
        token t attends to the rows whose segment is a set bit of token_segments[b, t].  Every token must allow a present segment.
        context_weights [B, L] (extension, prompt weights; beside the segment arrays, beside context_lens, or alone): over the rows
        a token attends to, p = w exp(s) / sum w exp(s).  A weight of 0 makes the row padding; otherwise 2^-20 <= w <= 2^20.
        control (extension, prompt-to-prompt): (row_map, blend, gain), each [B / 2, L] -- the batch is B / 2 pairs,
        the source images in front; the edited half attends with P = gain (has ? (1 - blend) pt + blend ps[row_map] : pt), ps the source
        half's probabilities (``ops.attention_control``).  It needs a context and stands beside context_lens only.
        inject_self (the same extension, a self-attention): the edited half attends with the source half's Q and K and its own V.
        score (extension, the local blend): (w_src, w_edit, scale, into) -- the phrase's row weights [B / 2, L]
        of the two halves of a batch of pairs, checked (``ops.host_phrase_weights``), a scale, and None or the pair of f32 [B / 2, N]
        tensors to add to -> (that, (score_src, score_edit)): scale times the head-mean of the phrase rows' probabilities, the source
        half's own and the edited half's as it attends -- under `control` where given (``ops.attention_phrase_score``).  It needs a
        context and stands beside context_lens only.
        keys: the call's checked ``ops.Keys``, which is not checked again; the four arrays beside it are then its own (what
        ``Layer.forward`` hands over) and are not looked at.  Without it the four arrays are checked here, whatever their types."""
        shape = (x.shape[0], 0 if context is None else context.shape[1], x.shape[1])
        if keys is not None:
            keys = ops.host_keys(*shape, keys=keys)
        else:
            keys = ops.host_keys(*shape, context_lens, context_segments, token_segments, context_weights, has_context=context is not None,
                                 missing="a context (self-attention takes no mask and no weights)")
        context_lens, weights = keys.lens, keys.weights
        segments = None if keys.context_segments is None else (keys.context_segments, keys.token_segments)
        if control is not None:
            if context is None or segments is not None or want_maps:
                raise ValueError("control needs a context and stands beside context_lens only")
            if x.shape[0] % 2:
                raise ValueError(f"control: {x.shape[0]} images are no pairs")
            control = ops.host_control(*control, x.shape[0] // 2, context.shape[1])
        if inject_self and (context is not None or x.shape[0] % 2):
            raise ValueError("inject_self is for the self-attention of a batch of pairs")
        if score is not None and (context is None or segments is not None or want_maps or x.shape[0] % 2):
            raise ValueError("score needs a context and a batch of pairs, and stands beside context_lens only")
        if self.training and self.to_out[1].p > 0:
            raise RuntimeError("paintmind_amd attention is inference-only (dropout>0 in training mode)")
        if want_maps and context is None:
            raise ValueError("want_maps: the maps are those of a cross-attention: a context is required")
        if not x.is_cuda:
            if control is not None or inject_self or score is not None:
                return self._run_cpu(x, context, residual, context_lens, control=control, inject_self=inject_self, score=score)
            if want_maps:
                return self._run_cpu(x, context, residual, context_lens, segments, weights, want_maps=True)
            return self._run_cpu(x, context, residual, context_lens, segments, weights)
        B, N, D = x.shape
        dtype = x.dtype
        pk = self.packed(dtype)
        fast = dtype == torch.bfloat16
        q_scale = self.scale * (ops.LOG2E if fast else 1.0)
        a = _rows(x.reshape(B * N, D), dtype)
        if context is None:
            if "wqkv" not in pk:
                raise ValueError("self-attention needs context_dim == query_dim")
            q, k, vt = ops.gemm_heads(a, pk["wqkv"], self.heads, N, [ops.PART_Q, ops.PART_K, ops.PART_V], q_scale, self.dim_head)
            n_kv = N
        else:
            L = context.shape[1]
            c = _rows(context.reshape(B * L, context.shape[2]), dtype)
            (q,) = ops.gemm_heads(a, pk["wq"], self.heads, N, [ops.PART_Q], q_scale, self.dim_head)
            k, vt = ops.gemm_heads(c, pk["wkv"], self.heads, L, [ops.PART_K, ops.PART_V], 1.0, self.dim_head)
            n_kv = L
        kv_lens = None if context_lens is None else torch.tensor(context_lens, dtype=torch.int32, device=x.device)
        if segments is not None:
            form = dict(key_segments=torch.from_numpy(segments[0]).to(x.device),
                        query_segments=torch.from_numpy(segments[1].view(np.int32)).to(x.device),
                        key_weights=None if weights is None else torch.from_numpy(weights).to(x.device))
        else:
            form = dict(kv_lens=kv_lens)
        if control is not None or inject_self:
            # a batch of pairs: the source half as ever, on its own; the edited half under control / on the source half's Q and K
            h2 = B // 2
            o = torch.empty(B * N, self.heads * self.dim_head, device=x.device, dtype=dtype)
            o[:h2 * N] = ops.attention(q[:h2], k[:h2], vt[:h2], n_kv, use_exp2=fast, kv_lens=None if kv_lens is None else kv_lens[:h2])
            if inject_self:
                o[h2 * N:] = ops.attention(q[:h2], k[:h2], vt[h2:], n_kv, use_exp2=fast)
            else:
                rm, bl, gn = (torch.from_numpy(c).to(x.device) for c in control)
                ops.attention_control(q[:h2], k[:h2], q[h2:], k[h2:], vt[h2:], n_kv, n_kv, rm, bl, gn, use_exp2=fast,
                                      lens_src=None if kv_lens is None else kv_lens[:h2].contiguous(),
                                      lens_tgt=None if kv_lens is None else kv_lens[h2:].contiguous(), out=o[h2 * N:])
        else:
            o = ops.attention(q, k, vt, n_kv, use_exp2=fast, **form)
        res = residual.reshape(B * N, D) if residual is not None else None
        out_dtype = torch.float32 if residual is not None else dtype
        out = ops.gemm(o, pk["wo"], bias=pk["bo"], residual=res, out_dtype=out_dtype)
        if want_maps:
            return out.reshape(B, N, D), ops.attention_maps(q, k, n_kv, use_exp2=fast, **form)
        if score is not None:
            h2 = B // 2
            w_src, w_edit, scale, into = score
            ctl = (None, None, None) if control is None else tuple(torch.from_numpy(c).to(x.device) for c in control)
            got = ops.attention_phrase_score(q[:h2], k[:h2], q[h2:], k[h2:], n_kv, n_kv, torch.from_numpy(w_src).to(x.device),
                                             torch.from_numpy(w_edit).to(x.device), *ctl, use_exp2=fast,
                                             lens_src=None if kv_lens is None else kv_lens[:h2].contiguous(),
                                             lens_tgt=None if kv_lens is None else kv_lens[h2:].contiguous(), out=into, scale=scale,
                                             accumulate=into is not None)
            return out.reshape(B, N, D), got
        return out.reshape(B, N, D)


    def _run_cpu(self, x, context, residual, context_lens=None, segments=None, weights=None, want_maps=False, control=None,
                 inject_self=False, score=None):
        """Parameters on the CPU: the same operator in plain torch (reference modules/attention.py:43-59; BASELINE config 1
        runs the model there).  q is scaled BEFORE the product (:52), no mask, softmax over the keys, head split 'b n (h d)'.
        context_lens (a checked list, or None): scores of the keys at or beyond an image's length become -inf (whatever they
        were, NaN included) and the V rows there are ZEROED -- a probability of 0 alone would not do, 0 * NaN is NaN in P @ V.
        segments (checked numpy arrays (uint8 [B, L], uint32 [B, N]), or None): the same per QUERY -- scores of the rows a token
        does not attend to become -inf, and the V rows of padding (segment 255) are zeroed.
        weights (checked numpy float32 [B, L] beside segments, or None): log w is added to the scores of the rows with w > 0; a row
        with w == 0 is padding.
        want_maps: -> (the result, p.mean(heads) f32 [B, N, L]): the probabilities of this very softmax, 0 where a row takes no part.
        control (checked numpy (int32, float32, float32) [B / 2, L], or None): the edited half's probabilities become
        gain (has ? (1 - blend) pt + blend ps[row_map] : pt), ps the source half's, has = 0 <= row_map < the source length and
        blend != 0; no renormalisation.  inject_self: the edited half's q and k are the source half's.
        score ((w_src, w_edit, scale, into), checked, or None): -> (the result, (score_src, score_edit)), f32 [B / 2, N] each: scale
        times the mean over the heads of sum_k w[k] p[q, k], p the source half's probabilities and the edited half's as it attends
        (behind `control`), added to `into` when given."""
        B, N, _ = x.shape
        c = x if context is None else context
        L = c.shape[1]
        if context_lens is not None and len(set(context_lens)) == 1 and control is None and score is None:
            c, context_lens = c[:, :context_lens[0]], None       # one length for the batch (B = 1 always): cut the padding off
        h, d = self.heads, self.dim_head
        q = (F.linear(x, self.to_q.weight) * self.scale).reshape(B, N, h, d).permute(0, 2, 1, 3)
        k = F.linear(c, self.to_k.weight).reshape(B, c.shape[1], h, d).permute(0, 2, 1, 3)
        v = F.linear(c, self.to_v.weight).reshape(B, c.shape[1], h, d).permute(0, 2, 1, 3)
        if inject_self:
            q, k = torch.cat([q[:B // 2]] * 2), torch.cat([k[:B // 2]] * 2)
        s = q @ k.transpose(-1, -2)
        if context_lens is not None:
            pad = torch.arange(c.shape[1])[None, :] >= torch.tensor(context_lens)[:, None]           # [B, L]
            s = s.masked_fill(pad[:, None, None, :], float("-inf"))
            v = v.masked_fill(pad[:, None, :, None], 0.0)
        if segments is not None:
            allowed = torch.from_numpy(ops.segments_allowed(*segments))                               # [B, N, L]
            s = s.masked_fill(~allowed[:, None], float("-inf"))
            v = v.masked_fill(torch.from_numpy(segments[0] == 255)[:, None, :, None], 0.0)
        if weights is not None:
            w = torch.from_numpy(weights)
            off = (w == 0)
            s = s + torch.log(torch.where(off, torch.ones_like(w), w))[:, None, None, :].to(s.dtype)
            s = s.masked_fill(off[:, None, None, :], float("-inf"))
            v = v.masked_fill(off[:, None, :, None], 0.0)
        p = torch.softmax(s, dim=-1)
        if control is not None:
            h2 = B // 2
            rm, bl, gn = (torch.from_numpy(c) for c in control)
            ns = torch.tensor(context_lens[:h2] if context_lens is not None else [L] * h2)
            has = (rm >= 0) & (rm < ns[:, None]) & (bl != 0)                                            # [B / 2, L]
            ps = torch.gather(p[:h2], -1, torch.where(has, rm, 0).long()[:, None, None, :].expand_as(p[h2:]))
            bl, gn = bl.to(p.dtype)[:, None, None, :], gn.to(p.dtype)[:, None, None, :]
            p = torch.cat([p[:h2], gn * torch.where(has[:, None, None, :], (1 - bl) * p[h2:] + bl * ps, p[h2:])])
        o = (p @ v).permute(0, 2, 1, 3).reshape(B, N, h * d)
        out = F.linear(o, self.to_out[0].weight, self.to_out[0].bias)
        out = out if residual is None else out + residual
        if score is not None:
            h2 = B // 2
            w_src, w_edit, scale, into = score
            part = lambda ph, w: ((ph * torch.from_numpy(w).to(ph.dtype)[:, None, None, :]).sum(-1).mean(1) * scale).float()
            got = part(p[:h2], w_src), part(p[h2:], w_edit)
            return out, (got if into is None else (into[0] + got[0], into[1] + got[1]))
        if want_maps:
            return out, F.pad(p.mean(1).float(), (0, L - p.shape[-1]))       # (a context cut to one common length: zeros behind it)
        return out


def round_up64(v):
    return ops.round_up(v, 64)


def _rows(x2d, dtype):
    """contiguous [M,K] in `dtype` with K padded to a multiple of 64 (device-side pad-convert kernel)."""
    k = x2d.shape[1]
    if x2d.dtype == dtype and k % 64 == 0:
        return x2d.contiguous()
    if x2d.dtype != torch.float32:
        raise TypeError("only float32 inputs can be pad-converted")
    return ops.convert_pad(x2d.contiguous(), round_up64(k), dtype)


# both reference names resolve to the HIP operator
MemoryEfficientCrossAttention = CrossAttention
ATTENTION_MODES = {"vanilla": CrossAttention, "xformer": CrossAttention, "hip": CrossAttention}
