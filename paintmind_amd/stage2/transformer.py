"""Stage-2 bidirectional conditional transformer holder (reference stage2/transformer.py:28-93)."""
import torch
from torch import nn

from .. import ops, packing
from ..modules.attention import ATTENTION_MODES, _rows
from ..modules.mlp import SwiGLUFFNFused
from ..stage1.layers import _norm, _xavier_like_reference, compute_dtype_of


class Layer(nn.Module):
    ATTENTION_MODES = ATTENTION_MODES

    def __init__(self, dim, dim_head, mlp_dim, num_head=8, dropout=0.0, dim_context=None):
        super().__init__()
        attn_cls = self.ATTENTION_MODES["hip"]
        self.norm1 = nn.LayerNorm(dim)
        self.attn1 = attn_cls(query_dim=dim, heads=num_head, dim_head=dim_head, dropout=dropout)
        self.norm2 = nn.LayerNorm(dim)
        self.attn2 = attn_cls(query_dim=dim, context_dim=dim_context, heads=num_head, dim_head=dim_head, dropout=dropout)
        self.norm3 = nn.LayerNorm(dim)
        self.ffnet = SwiGLUFFNFused(in_features=dim, hidden_features=mlp_dim)

    def forward(self, x, context=None, context_lens=None, context_segments=None, token_segments=None, context_weights=None, want_maps=False,
                control=None, inject_self=False, keys=None, score=None):
        """self-attn, cross-attn (a 2nd self-attn when context is None), SwiGLU (transformer.py:44-49).
        want_maps: -> (x, maps), maps f32 [B, N, L] the head-mean probabilities of the cross-attention (modules/attention.py).
        context_lens: per-image context lengths for the cross-attention only (modules/attention.py).
        context_segments / token_segments: regional prompts, for the cross-attention only (modules/attention.py).
        context_weights: prompt weights, for the cross-attention only (modules/attention.py).
        control / inject_self: prompt-to-prompt on a batch of pairs, the cross-attention's control and the injection into the first
        self-attention (modules/attention.py).
        score: the local blend's phrase score of the cross-attention (modules/attention.py): -> (x, (score_src, score_edit)).
        keys (instead of the four arrays): the call's checked ``ops.Keys``; the cross-attention gets the record and, as keywords, the
        record's own arrays."""
        if keys is not None:
            context_lens, context_segments, token_segments, context_weights = keys.cpu_args()
        B, N, D = x.shape
        T = compute_dtype_of(self)
        x = x.contiguous()
        x = self.attn1.run(_norm(x.reshape(B * N, D), self.norm1, T).reshape(B, N, D), None, residual=x,
                           **(dict(inject_self=True) if inject_self else {}))
        kw = dict(want_maps=True) if want_maps else {}
        if control is not None:
            kw["control"] = control
        if score is not None:
            kw["score"] = score
        x = self.attn2.run(_norm(x.reshape(B * N, D), self.norm2, T).reshape(B, N, D), context, residual=x,
                           context_lens=context_lens if context is not None else None,
                           context_segments=context_segments if context is not None else None,
                           token_segments=token_segments if context is not None else None,
                           context_weights=context_weights if context is not None else None,
                           keys=keys if context is not None else None, **kw)
        maps = None
        if want_maps or score is not None:
            x, maps = x
        x = self.ffnet.run(_norm(x.reshape(B * N, D), self.norm3, T).reshape(B, N, D), residual=x)
        return (x, maps) if want_maps or score is not None else x


class CondTransformer(nn.Module):
    def __init__(self, in_dim, dim, len_seq, dim_head, mlp_dim, num_head=8, depth=6, dropout=0.1, context_dim=None,
                 num_classes=8192):
        super().__init__()
        self.token_proj = nn.Linear(in_dim, dim)
        self.position_embedding = nn.Parameter(torch.randn(1, len_seq, dim) * dim ** -0.5)
        self.context_proj = nn.Linear(context_dim, dim, bias=False) if context_dim != dim else nn.Identity()
        self.layers = nn.Sequential()
        for i in range(depth):
            self.layers.add_module("layer" + str(i), Layer(dim, dim_head, mlp_dim, num_head, dropout, dim))
        self.norm = nn.LayerNorm(dim)
        self.to_logits = nn.Linear(dim, num_classes)
        _xavier_like_reference(self)

    def _layers(self, h, maps_layers, context, keys, control=None, score=None):
        """the tower over the projected context and the call's checked ``ops.Keys``; maps_layers (None, or the checked layer
        indices): -> (h, the mean of those layers' cross-attention maps);
        control (None, or per controlled layer its keywords): prompt-to-prompt, never beside maps_layers;
        score (None, or (the tapped layers, w_src, w_edit, the pair to add to or None)): beside control -> (h, (score_src, score_edit)),
        the first tapped layer writing unless there is a pair to add to, the later ones accumulating, each with scale 1 / n"""
        if control is not None:
            running = None if score is None else score[3]
            for i, layer in enumerate(self.layers):
                if score is not None and i in score[0]:
                    h, running = layer(h, context, keys=keys, score=(score[1], score[2], 1.0 / len(score[0]), running), **control.get(i, {}))
                else:
                    h = layer(h, context, keys=keys, **control.get(i, {}))
            return h if score is None else (h, running)
        if maps_layers is None:
            for layer in self.layers:
                h = layer(h, context, keys=keys)
            return h
        maps = None
        for i, layer in enumerate(self.layers):
            if i in maps_layers:
                h, m = layer(h, context, keys=keys, want_maps=True)
                maps = m if maps is None else maps + m
            else:
                h = layer(h, context, keys=keys)
        return h, maps / len(maps_layers)

    def forward(self, x, context=None, context_lens=None, context_segments=None, token_segments=None, context_weights=None,
                maps_layers=None, control=None, keys=None):
        """operator-level composition of transformer.py:80-93 (Pipeline uses the native engine instead).
        maps_layers (extension, attention maps; None = the call as without it): distinct layer indices ->
        (logits, maps), the logits as without it and maps f32 [B, N, L], the mean over those layers of the head-mean probabilities
        of each layer's cross-attention.  It needs a context.
        context_lens (extension; None = the reference's behaviour): image b's cross-attention sees rows [0, context_lens[b]) of
        its context only.  The context projection still covers every row: it is row-local, so padding stays in the padding.
        context_segments [B, L] / token_segments [B, N] (extension, regional prompts): see ``CrossAttention.run``.
        context_weights [B, L] (extension, prompt weights; beside the segments, beside context_lens, or alone): likewise.
        control (extension, prompt-to-prompt; None = the call as without it): a dict with row_map, blend, gain
        ([B / 2, L]; required iff cross_layers), cross_layers and self_layers (distinct layer indices) over a batch of B / 2 pairs, the
        source images in front -- ``S2Engine.forward_control`` as a composition of operators.  Beside context_lens only.
        With score_layers (distinct layer indices) and score_weights = (w_src, w_edit) ([B / 2, L], finite and >= 0, every pair with a
        positive weight below its length in one half) in the dict (extension, the local blend) -> (logits,
        scores), scores f32 [B, N] with the source half in front: the mean over those layers of ``ops.attention_phrase_score``, added
        to the dict's `scores` when given.  cross_layers and self_layers may then both be empty.
        keys (instead of the four arrays): the call's checked ``ops.Keys``; it is not checked again."""
        keys = ops.host_keys(x.shape[0], 0 if context is None else context.shape[1], x.shape[1], context_lens, context_segments,
                             token_segments, context_weights, has_context=context is not None, keys=keys)
        if control is not None:
            if context is None or keys.context_segments is not None or maps_layers is not None or x.shape[0] % 2:
                raise ValueError("control needs a context and an even batch, and stands beside context_lens only")
            cl, sl = (ops.host_layers(control.get(k, ()), len(self.layers), "control: layers", allow_empty=True)
                      for k in ("cross_layers", "self_layers"))
            arrays = [control.get(k) for k in ("row_map", "blend", "gain")]
            scl = ops.host_layers(control.get("score_layers", ()), len(self.layers), "control: score_layers", allow_empty=True)
            if not (cl or sl or scl) or any(a is None for a in arrays) != (not cl) or any(a is None for a in arrays) != all(a is None for a in arrays):
                raise ValueError("control: a layer must be chosen; row_map, blend and gain are required with cross_layers and refused without")
            if not scl and (control.get("score_weights") is not None or control.get("scores") is not None):
                raise ValueError("control: score_weights and scores stand beside score_layers only")
            score = None
            if scl:
                h2, into = x.shape[0] // 2, control.get("scores")
                scores_in = into
                w_src, w_edit = ops.host_phrase_weights(control.get("score_weights"), h2, context.shape[1])
                ops.check_phrase_rows(w_src, w_edit, keys.lens, h2, context.shape[1])
                if into is not None and not (isinstance(into, torch.Tensor) and into.dtype == torch.float32 and into.device == x.device and
                                             tuple(into.shape) == (x.shape[0], x.shape[1]) and into.is_contiguous()):
                    raise ValueError(f"control: scores must be a contiguous float32 [{x.shape[0]}, {x.shape[1]}] tensor on the tokens' device")
                score = (scl, w_src, w_edit, None if into is None else (into[:h2], into[h2:]))
            ctl = ops.host_control(*arrays, x.shape[0] // 2, context.shape[1]) if cl else None
            control = {l: (dict(control=ctl) if l in cl else {}) | (dict(inject_self=True) if l in sl else {}) for l in set(cl) | set(sl)}
        if maps_layers is not None:
            if context is None:
                raise ValueError("maps_layers: the maps are those of the cross-attention: a context is required")
            maps_layers = ops.host_layers(maps_layers, len(self.layers), "maps_layers")
        T = compute_dtype_of(self)
        B, N, E = x.shape
        dim = self.token_proj.out_features
        if not x.is_cuda:
            # parameters on the CPU (reference stage2/transformer.py:80-93 in plain torch): the context is projected once
            # per forward, a missing context makes attn2 a second self-attention
            h = self.token_proj(x.float()) + self.position_embedding
            if context is not None:
                context = self.context_proj(context.float())
            h = self._layers(h, maps_layers, context, keys, control=control, score=score if control is not None else None)
            if maps_layers is not None:
                return self.to_logits(self.norm(h[0])), h[1]
            if control is not None and score is not None:
                return self.to_logits(self.norm(h[0])), torch.cat(h[1])
            return self.to_logits(self.norm(h))
        a = ops.convert_pad(x.contiguous().float().reshape(B * N, E), 64, T)
        pos = self.position_embedding.detach()[0].contiguous()
        h = ops.gemm(a, packing.pad_cols(self.token_proj.weight, 64, T), bias=self.token_proj.bias.detach().float(),
                     residual=pos, res_rows=N, out_dtype=torch.float32).reshape(B, N, dim)
        if context is not None:
            L = context.shape[1]
            c = _rows(context.contiguous().float().reshape(B * L, -1), T)
            if isinstance(self.context_proj, nn.Linear):
                c = ops.gemm(c, packing.pad_cols(self.context_proj.weight, c.shape[1], T))
            context = c.reshape(B, L, dim)
        h = self._layers(h, maps_layers, context, keys, control=control, score=score if control is not None else None)
        maps = None
        if control is not None and score is not None:
            h, halves = h
            halves = torch.cat(halves) if score[3] is None else scores_in    # (the operator added to the caller's buffer in place)
        if maps_layers is not None:
            h, maps = h
        y = _norm(h.reshape(B * N, dim), self.norm, T)
        logits = ops.gemm(y, packing.cast(self.to_logits.weight, T), bias=self.to_logits.bias.detach().float(),
                          out_dtype=torch.float32)
        if control is not None and score is not None:
            return logits.reshape(B, N, -1), halves
        return (logits.reshape(B, N, -1), maps) if maps_layers is not None else logits.reshape(B, N, -1)
