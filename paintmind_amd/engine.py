"""Host side of the model-level C ABI: pack a module tree's weights, build the pointer tables
(pmhip_vqgan_weights / pmhip_s2_weights) and own the native handles.

Engines are cached per (parameter fingerprint, compute dtype, device): loading a checkpoint, moving
the module or editing a weight in place transparently rebuilds the packed copy.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, ops, packing
from ._lib import LayerWeights, S2Cfg, S2Weights, TowerCfg, VqganCfg, VqganWeights, check
from .ops import _p, pm_dtype, round_up, stream_ptr


def _f32(t):
    return t.detach().float().contiguous()


def _c_ints(vals):
    """a host list of ints (or None) -> a ctypes int32 array (or None: NULL)"""
    return None if vals is None else (C.c_int * len(vals))(*vals)


def _key_args(keys, native_lens=True):
    """a checked ``ops.Keys`` -> the ctypes arguments (ctx_lens_host int32 [B], ctx_seg_host uint8 [B * L], tok_seg_host uint32
    [B * tokens], ctx_w_host float32 [B * L]), None where the entry takes NULL.  The neutral segments of weights without segment
    arrays are not handed over: the native entry stages them itself from the lengths -- except one that takes no lengths
    (native_lens False), which gets them from here when there are lengths."""
    lens, cs, ts = keys.lens, keys.context_segments, keys.token_segments
    if cs is None:
        return _c_ints(lens), None, None, None
    flat = lambda a: None if a is None else np.ctypeslib.as_ctypes(np.ascontiguousarray(a).reshape(-1))
    if keys.neutral:
        lens = keys.neutral_lens if native_lens else None
        if native_lens or keys.neutral_lens is None:
            cs = ts = None
    return _c_ints(lens), flat(cs), flat(ts), flat(keys.weights)


class _Keep:
    """keeps packed tensors alive for as long as the native handle points at them"""

    def __init__(self):
        self.tensors = []

    def __call__(self, t):
        self.tensors.append(t)
        return C.c_void_p(t.data_ptr())


def _pack_layer(layer, dtype, keep, stage2):
    lw = LayerWeights()
    a1 = layer.attn1
    lw.ln1_g, lw.ln1_b = keep(_f32(layer.norm1.weight)), keep(_f32(layer.norm1.bias))
    lw.wqkv = keep(packing.pack_qkv(a1.to_q, a1.to_k, a1.to_v, dtype))
    lw.wo, lw.bo = keep(packing.cast(a1.to_out[0].weight, dtype)), keep(_f32(a1.to_out[0].bias))
    if stage2:
        a2 = layer.attn2
        lw.lnx_g, lw.lnx_b = keep(_f32(layer.norm2.weight)), keep(_f32(layer.norm2.bias))
        lw.wqkv2 = keep(packing.pack_qkv(a2.to_q, a2.to_k, a2.to_v, dtype))
        lw.wo2, lw.bo2 = keep(packing.cast(a2.to_out[0].weight, dtype)), keep(_f32(a2.to_out[0].bias))
        ffn_norm = layer.norm3
    else:
        ffn_norm = layer.norm2
    lw.ln2_g, lw.ln2_b = keep(_f32(ffn_norm.weight)), keep(_f32(ffn_norm.bias))
    w12p, b12p, hp = packing.pack_w12(layer.ffnet.w12, dtype)
    lw.w12p, lw.b12p = keep(w12p), keep(b12p)
    lw.w3p, lw.b3 = keep(packing.pack_w3(layer.ffnet.w3, hp, dtype)), keep(_f32(layer.ffnet.w3.bias))
    # what each residual producer adds to every row's mean (centred hi plane, include/pmhip.h)
    lw.bo_mean = float(a1.to_out[0].bias.detach().float().mean())
    lw.b3_mean = float(layer.ffnet.w3.bias.detach().float().mean())
    if stage2:
        lw.bo2_mean = float(layer.attn2.to_out[0].bias.detach().float().mean())
    if dtype == torch.bfloat16:
        # LayerNorm fold (include/pmhip.h, pmhip_lnfold): gamma-scaled copies of the weights that consume a LayerNorm
        def fold(w32, norm):
            wg, c, d = packing.ln_fold(w32, norm.weight, norm.bias, dtype)
            return keep(wg), keep(c), keep(d)
        lw.wqkv_f, lw.qkv_c, lw.qkv_d = fold(packing.pack_qkv(a1.to_q, a1.to_k, a1.to_v, torch.float32), layer.norm1)
        if stage2:
            a2 = layer.attn2
            if a2.to_k.in_features == a2.to_q.in_features:      # always true in the reference (context is pre-projected)
                lw.wqkv2_f, lw.qkv2_c, lw.qkv2_d = fold(packing.pack_qkv(a2.to_q, a2.to_k, a2.to_v, torch.float32), layer.norm2)
        lw.w12p_f, lw.w12_c, lw.w12_d = fold(packing.pack_w12(layer.ffnet.w12, torch.float32)[0], ffn_norm)
    return lw, hp


def _pack_tower(layers, dtype, keep, stage2):
    arr = (LayerWeights * len(layers))()
    hp = 0
    for i, layer in enumerate(layers):
        arr[i], hp = _pack_layer(layer, dtype, keep, stage2)
    return arr, hp


def _switch_dict(bits):
    return {"ln_fold": bool(bits & 1), "hilo": bool(bits & 2), "ln_stats": bool(bits & 4), "hilo_center": bool(bits & 8),
            "blocking_wait": bool(bits & 16), "graph_replay_off": bool(bits & 32)}


class VqganEngine:
    """native VQModel handle (pmhip_vqgan) for one (weights, dtype, device)."""

    @property
    def switches(self):
        """the PMHIP_* switches this handle latched when it was created (they are not re-read: include/pmhip.h)"""
        return _switch_dict(self.lib.pmhip_vqgan_switches(self.handle))

    def __init__(self, model, dtype):
        self.lib = _lib.load()
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise _lib.PmhipError("paintmind_amd needs the model on a ROCm device (model.to('cuda')); no CPU fallback")
        self.device, self.dtype = dev, dtype
        keep = self.keep = _Keep()
        enc, dec, vq = model.encoder, model.decoder, model.quantize
        conv = enc.to_patch_embedding[0]
        P = enc.patch_size
        self.channels = conv.in_channels
        self.image_size = enc.image_size
        self.tokens = (enc.image_size // P) ** 2
        self.embed_dim = vq.e_dim
        with torch.cuda.device(dev):
            enc_layers, enc_hp = _pack_tower(list(enc.transformer.layers), dtype, keep, False)
            dec_layers, dec_hp = _pack_tower(list(dec.transformer.layers), dtype, keep, False)
            self._layer_arrays = (enc_layers, dec_layers)
            en, sq = vq.prepared()
            w = VqganWeights()
            w.patch_w = keep(packing.cast(conv.weight.reshape(conv.out_channels, -1), dtype))
            w.enc_pos = keep(_f32(enc.position_embedding[0]))
            w.pre_g, w.pre_b = keep(_f32(enc.norm_pre.weight)), keep(_f32(enc.norm_pre.bias))
            w.enc_layers = enc_layers
            w.prevq_w, w.prevq_b = keep(packing.cast(model.prev_quant.weight, dtype)), keep(_f32(model.prev_quant.bias))
            w.codebook_n, w.codebook_sq = keep(en), keep(sq)
            w.postq_w, w.postq_b = keep(packing.pad_cols(model.post_quant.weight, 64, dtype)), keep(_f32(model.post_quant.bias))
            w.dec_pos = keep(_f32(dec.position_embedding[0]))
            w.dec_layers = dec_layers
            w.dn_g, w.dn_b = keep(_f32(dec.norm.weight)), keep(_f32(dec.norm.bias))
            w.proj_w, w.proj_b = keep(packing.cast(dec.proj.weight, dtype)), keep(_f32(dec.proj.bias))
            torch.cuda.synchronize(dev)
        cfg = VqganCfg()
        cfg.image_size, cfg.patch_size, cfg.channels = enc.image_size, P, conv.in_channels
        cfg.n_embed, cfg.embed_dim, cfg.beta = vq.n_e, vq.e_dim, float(vq.beta)
        a_enc = enc.transformer.layers[0].attn1
        a_dec = dec.transformer.layers[0].attn1
        cfg.enc = TowerCfg(conv.out_channels, len(enc.transformer.layers), a_enc.heads, enc_hp, a_enc.dim_head)
        cfg.dec = TowerCfg(dec.proj.in_features, len(dec.transformer.layers), a_dec.heads, dec_hp, a_dec.dim_head)
        self.cfg, self.weights = cfg, w
        self.handle = C.c_void_p()
        check(self.lib.pmhip_vqgan_create(C.byref(self.handle), dev.index or 0, pm_dtype(dtype), C.byref(cfg), C.byref(w)),
              "pmhip_vqgan_create")

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.pmhip_vqgan_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def clone(self):
        """a second native handle (own workspace, own graphs) over the SAME packed weights: one per concurrent stream"""
        other = object.__new__(VqganEngine)
        other.__dict__.update({k: v for k, v in self.__dict__.items() if k != "handle"})
        other.handle = C.c_void_p()
        check(self.lib.pmhip_vqgan_create(C.byref(other.handle), self.device.index or 0, pm_dtype(self.dtype), C.byref(self.cfg),
                                          C.byref(self.weights)), "pmhip_vqgan_create")
        return other

    # -- entry points -------------------------------------------------------------------------------
    def _img(self, img):
        if not img.is_cuda:
            raise _lib.PmhipError("input image is on the CPU; paintmind_amd has no CPU fallback")
        return img.to(self.device, torch.float32).contiguous()

    def encode(self, img):
        img = self._img(img)
        B = img.shape[0]
        z = torch.empty(B, self.tokens, self.embed_dim, device=self.device, dtype=torch.float32)
        idx = torch.empty(B, self.tokens, device=self.device, dtype=torch.int64)
        loss = torch.empty(1, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            check(self.lib.pmhip_vqgan_encode(self.handle, _p(img), B, _p(z), _p(idx), _p(loss), stream_ptr(self.device)),
                  "pmhip_vqgan_encode")
        return z, loss.reshape(()), idx

    def encoder_forward(self, img):
        img = self._img(img)
        B = img.shape[0]
        x = torch.empty(B, self.tokens, self.cfg.enc.dim, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            check(self.lib.pmhip_vqgan_encoder_forward(self.handle, _p(img), B, _p(x), stream_ptr(self.device)),
                  "pmhip_vqgan_encoder_forward")
        return x

    def _new_img(self, B):
        return torch.empty(B, self.channels, self.image_size, self.image_size, device=self.device, dtype=torch.float32)

    def decode(self, z):
        z = z.to(self.device, torch.float32).contiguous()
        B = z.shape[0]
        img = self._new_img(B)
        with torch.cuda.device(self.device):
            check(self.lib.pmhip_vqgan_decode(self.handle, _p(z), B, _p(img), stream_ptr(self.device)), "pmhip_vqgan_decode")
        return img

    def decode_indices(self, idx):
        idx = idx.to(self.device, torch.int64).contiguous()
        B = idx.shape[0]
        img = self._new_img(B)
        with torch.cuda.device(self.device):
            check(self.lib.pmhip_vqgan_decode_indices(self.handle, _p(idx), B, _p(img), stream_ptr(self.device)),
                  "pmhip_vqgan_decode_indices")
        return img

    def decoder_forward(self, x):
        x = x.to(self.device, torch.float32).contiguous()
        B = x.shape[0]
        img = self._new_img(B)
        with torch.cuda.device(self.device):
            check(self.lib.pmhip_vqgan_decoder_forward(self.handle, _p(x), B, _p(img), stream_ptr(self.device)),
                  "pmhip_vqgan_decoder_forward")
        return img


class S2Engine:
    """native CondTransformer handle (pmhip_s2) + the MaskGIT loop entry points."""

    @property
    def switches(self):
        """the PMHIP_* switches this handle latched when it was created (they are not re-read: include/pmhip.h)"""
        return _switch_dict(self.lib.pmhip_s2_switches(self.handle))

    def graph_count(self):
        """(entries, captured) of this handle's graph cache (pmhip_s2_graph_count): the keys it holds, and how many of them hold
        captured graphs"""
        entries, captured = C.c_int(0), C.c_int(0)
        check(self.lib.pmhip_s2_graph_count(self.handle, C.byref(entries), C.byref(captured)), "pmhip_s2_graph_count")
        return entries.value, captured.value

    def step0_shared(self):
        """(fills, hits) of this handle's shared step-0 logits (pmhip_s2_step0_shared): computed 0 or 1 times, sampled from by
        `hits` later unconditional loops that ran no step-0 tower"""
        fills, hits = C.c_int(0), C.c_int(0)
        check(self.lib.pmhip_s2_step0_shared(self.handle, C.byref(fills), C.byref(hits)), "pmhip_s2_step0_shared")
        return fills.value, hits.value

    def __init__(self, transformer, codebook, mask_token, dtype):
        self.lib = _lib.load()
        dev = next(transformer.parameters()).device
        if dev.type != "cuda":
            raise _lib.PmhipError("paintmind_amd needs the model on a ROCm device (model.to('cuda')); no CPU fallback")
        self.device, self.dtype = dev, dtype
        keep = self.keep = _Keep()
        tr = transformer
        layers = list(tr.layers)
        with torch.cuda.device(dev):
            arr, hp = _pack_tower(layers, dtype, keep, True)
            self._layer_array = arr
            w = S2Weights()
            # RAW codebook rows then the mask token (reference generate.py:148-157)
            w.tok_table = keep(torch.cat([_f32(codebook), _f32(mask_token)], dim=0).contiguous())
            w.tokproj_w, w.tokproj_b = keep(packing.pad_cols(tr.token_proj.weight, 64, dtype)), keep(_f32(tr.token_proj.bias))
            w.pos = keep(_f32(tr.position_embedding[0]))
            dim = tr.token_proj.out_features
            if isinstance(tr.context_proj, torch.nn.Linear):
                ctx_dim = tr.context_proj.in_features
                ctx_pad = round_up(ctx_dim, 64)
                w.ctxproj_w = keep(packing.pad_cols(tr.context_proj.weight, ctx_pad, dtype))
            else:
                ctx_dim = ctx_pad = dim
                w.ctxproj_w = C.c_void_p(0)
            w.layers = arr
            w.norm_g, w.norm_b = keep(_f32(tr.norm.weight)), keep(_f32(tr.norm.bias))
            w.logits_w, w.logits_b = keep(packing.cast(tr.to_logits.weight, dtype)), keep(_f32(tr.to_logits.bias))
            if dtype == torch.bfloat16:
                wg, c, d = packing.ln_fold(tr.to_logits.weight, tr.norm.weight, tr.norm.bias, dtype)
                w.logits_wf, w.logits_c, w.logits_d = keep(wg), keep(c), keep(d)
            torch.cuda.synchronize(dev)
        cfg = S2Cfg()
        cfg.tokens = tr.position_embedding.shape[1]
        cfg.embed_dim = tr.token_proj.in_features
        cfg.n_embed = tr.to_logits.out_features
        cfg.context_dim, cfg.context_dim_pad = ctx_dim, ctx_pad
        cfg.tower = TowerCfg(dim, len(layers), layers[0].attn1.heads, hp, layers[0].attn1.dim_head)
        self.cfg, self.weights = cfg, w
        self.tokens, self.n_embed, self.embed_dim, self.context_dim = cfg.tokens, cfg.n_embed, cfg.embed_dim, ctx_dim
        self.handle = C.c_void_p()
        check(self.lib.pmhip_s2_create(C.byref(self.handle), dev.index or 0, pm_dtype(dtype), C.byref(cfg), C.byref(w)),
              "pmhip_s2_create")

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.pmhip_s2_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def clone(self):
        """a second native handle (own workspace, own graphs) over the SAME packed weights: one per concurrent stream"""
        other = object.__new__(S2Engine)
        other.__dict__.update({k: v for k, v in self.__dict__.items() if k != "handle"})
        other.handle = C.c_void_p()
        check(self.lib.pmhip_s2_create(C.byref(other.handle), self.device.index or 0, pm_dtype(self.dtype), C.byref(self.cfg),
                                       C.byref(self.weights)), "pmhip_s2_create")
        return other

    def _ctx(self, context):
        if context is None:
            return None, 0
        context = context.to(self.device, torch.float32).contiguous()
        if context.shape[-1] != self.context_dim:
            raise ValueError(f"context width {context.shape[-1]} != context_dim {self.context_dim}")
        return context, context.shape[1]

    def _keys(self, B, L, context_lens=None, context_segments=None, token_segments=None, context_weights=None, keys=None):
        """the four keywords of an entry point, or the record that stands for them -> the call's ``ops.Keys``: checked here, at the
        door, unless it comes checked (and once more by the native entry).  L == 0: there is no context."""
        return ops.host_keys(B, L, self.tokens, context_lens, context_segments, token_segments, context_weights, has_context=L > 0, keys=keys)

    def _call(self, table, head, tail=()):
        """the native call of an entry family: `table` is ordered (condition, entry name, trailing arguments); the first row whose
        condition holds is called with head + its trailing arguments + tail -- an entry gets what it declares, no wider one stands in"""
        for cond, name, extra in table:
            if cond:
                return check(getattr(self.lib, name)(*head, *extra, *tail), name)

    def forward(self, tokens, context=None, context_lens=None, context_segments=None, token_segments=None, context_weights=None, keys=None,
                out=None):
        """context_segments / token_segments (None = the call as without them): regional prompts (pmhip_s2_forward_segments).
        context_weights (None = the call as without them): prompt weights (pmhip_s2_forward_weights).  keys (instead of the four
        keywords): the call's checked ``ops.Keys``.  out (None: a new tensor): where the logits go, a contiguous fp32 [B, tokens,
        n_embed] tensor on the engine's device -- a slice of a larger buffer that several calls fill."""
        tokens = tokens.to(self.device, torch.float32).contiguous()
        B = tokens.shape[0]
        context, L = self._ctx(context)
        keys = self._keys(B, L, context_lens, context_segments, token_segments, context_weights, keys)
        lens, cs, ts, w = _key_args(keys, native_lens=False)
        logits = torch.empty(B, self.tokens, self.n_embed, device=self.device, dtype=torch.float32) if out is None else out
        if (logits.dtype != torch.float32 or tuple(logits.shape) != (B, self.tokens, self.n_embed) or logits.device != tokens.device
                or not logits.is_contiguous()):
            raise ValueError(f"forward: out must be a contiguous fp32 [{B}, {self.tokens}, {self.n_embed}] tensor on {self.device}")
        with torch.cuda.device(self.device):
            self._call(((w is not None, "pmhip_s2_forward_weights", (cs, ts, w)),
                        (cs is not None, "pmhip_s2_forward_segments", (cs, ts)),
                        (True, "pmhip_s2_forward_lens", (lens,))),
                       (self.handle, _p(tokens), _p(context), L, B), (_p(logits), stream_ptr(self.device)))
        return logits

    def forward_maps(self, tokens, context, layers, context_lens=None, context_segments=None, token_segments=None, context_weights=None,
                     keys=None):
        """``forward`` with the cross-attention maps of the chosen layers beside the logits (pmhip_s2_forward_maps; DESIGN.md section
        4y).  layers: the layer indices (an iterable of distinct ints in [0, depth)).  -> (logits, maps): the logits ``forward`` returns
        on the same arguments, bit for bit, and maps f32 [B, tokens, L], the mean over the chosen layers of the head-mean
        probabilities of each layer's cross-attention; context rows that take part in no softmax are exactly 0.  Always eager."""
        if context is None:
            raise ValueError("forward_maps: the maps are those of the cross-attention: a context is required")
        bits = sum(1 << l for l in ops.host_layers(layers, self.cfg.tower.depth, "forward_maps: layers"))
        tokens = tokens.to(self.device, torch.float32).contiguous()
        B = tokens.shape[0]
        context, L = self._ctx(context)
        lens, cs, ts, w = _key_args(self._keys(B, L, context_lens, context_segments, token_segments, context_weights, keys))
        logits = torch.empty(B, self.tokens, self.n_embed, device=self.device, dtype=torch.float32)
        maps = torch.empty(B, self.tokens, L, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            check(self.lib.pmhip_s2_forward_maps(self.handle, _p(tokens), _p(context), L, B, lens, cs, ts, w, bits, _p(logits), _p(maps),
                                                 stream_ptr(self.device)),
                  "pmhip_s2_forward_maps")
        return logits, maps

    def forward_control(self, tokens, context, row_map=None, blend=None, gain=None, cross_layers=(), self_layers=(), context_lens=None,
                        score_layers=(), score_weights=None, scores=None):
        """One eager forward over B pairs (pmhip_s2_forward_control): tokens [2B, tokens, E] and context
        [2B, L, D] with the source images in front, the edited ones behind.  In the layers of cross_layers the edited half's
        cross-attention blends the source half's probabilities into its own under row_map / blend / gain ([B, L] each, one row per
        pair: ``ops.host_control``); in the layers of self_layers its first self-attention takes the source half's Q and K.
        -> logits [2B, tokens, n_embed]; the source half's are those of ``forward`` on the source half alone, bit for bit.

        score_layers (default (): the call as without the three keywords): the layers whose cross-attention is tapped for the PHRASE
        SCORE (pmhip_s2_forward_control_scores) under score_weights = (w_src, w_edit), the phrase's row weights
        [B, L] of the two prompts, finite and >= 0.  scores (None: a new buffer, written): f32 [2B, tokens] on the device, the source
        half in front, which the call ACCUMULATES into -- mean over the tapped layers of ``ops.attention_phrase_score``, under the
        control where the layer is controlled.  cross_layers and self_layers may then both be empty: the logits are ``forward``'s.
        -> (logits, scores)"""
        if context is None:
            raise ValueError("forward_control: the control is that of the cross-attention: a context is required")
        depth = self.cfg.tower.depth
        bits = []
        for name, layers in (("cross_layers", cross_layers), ("self_layers", self_layers)):
            bits.append(sum(1 << l for l in ops.host_layers(layers, depth, f"forward_control: {name}", allow_empty=True)))
        score_bits = sum(1 << l for l in ops.host_layers(score_layers, depth, "forward_control: score_layers", allow_empty=True))
        if not (bits[0] | bits[1] | score_bits):
            raise ValueError("forward_control: cross_layers and self_layers select no layer")
        if (score_weights is not None or scores is not None) and not score_bits:
            raise ValueError("forward_control: score_weights and scores stand beside score_layers only")
        tokens = tokens.to(self.device, torch.float32).contiguous()
        if tokens.shape[0] % 2:
            raise ValueError(f"forward_control: {tokens.shape[0]} images are no pairs")
        B = tokens.shape[0] // 2
        context, L = self._ctx(context)
        lens = _c_ints(self._keys(2 * B, L, context_lens).lens)
        given = [x is not None for x in (row_map, blend, gain)]
        if any(given) != bool(bits[0]) or any(given) != all(given):
            raise ValueError("forward_control: row_map, blend and gain are required with cross_layers and refused without")
        ctl = (None, None, None)
        if bits[0]:
            rm, bl, gn = ops.host_control(row_map, blend, gain, B, L)
            ctl = tuple(np.ctypeslib.as_ctypes(x.reshape(-1)) for x in (rm, bl, gn))
        logits = torch.empty(2 * B, self.tokens, self.n_embed, device=self.device, dtype=torch.float32)
        if score_bits:
            w_src, w_edit = ops.host_phrase_weights(score_weights, B, L)
            accumulate = scores is not None
            if scores is None:
                scores = torch.empty(2 * B, self.tokens, device=self.device, dtype=torch.float32)
            if not (isinstance(scores, torch.Tensor) and scores.device == self.device and scores.dtype == torch.float32 and
                    tuple(scores.shape) == (2 * B, self.tokens) and scores.is_contiguous()):
                raise ValueError(f"forward_control: scores must be a contiguous float32 [{2 * B}, {self.tokens}] tensor on {self.device}")
            with torch.cuda.device(self.device):
                check(self.lib.pmhip_s2_forward_control_scores(self.handle, _p(tokens), _p(context), L, B, lens, bits[0], bits[1], ctl[0], ctl[1],
                                                               ctl[2], score_bits, np.ctypeslib.as_ctypes(w_src.reshape(-1)),
                                                               np.ctypeslib.as_ctypes(w_edit.reshape(-1)), _p(logits), _p(scores),
                                                               int(accumulate), stream_ptr(self.device)), "pmhip_s2_forward_control_scores")
            return logits, scores
        with torch.cuda.device(self.device):
            check(self.lib.pmhip_s2_forward_control(self.handle, _p(tokens), _p(context), L, B, lens, bits[0], bits[1], ctl[0], ctl[1], ctl[2],
                                                    _p(logits), stream_ptr(self.device)), "pmhip_s2_forward_control")
        return logits

    def sample(self, vq_engine, ids, context, topk, temperature, num_mask, noise=None, seed=0, step=0, image_base=0,
               want_img=True, want_aux=False, guidance_scale=None, context_lens=None, choice_temperature=None, choice_noise=None,
               top_p=None, negative_context=None, negative_lens=None, context_segments=None, token_segments=None, context_weights=None,
               keys=None):
        """one MaskGIT step; ids int64 [B,N] is updated IN PLACE (pass a clone to keep the input).
        context_weights (None = the calls below): prompt weights; only the pass with the context sees them
        (pmhip_pipeline_sample_weights).
        context_segments / token_segments (None = the calls below): regional prompts; only the pass with the context sees them
        (pmhip_pipeline_sample_segments).  keys (instead of these and context_lens): the call's checked ``ops.Keys``.
        negative_context fp32 [B, Ln, context_dim] (None = the calls below, as without the keyword): the second tower of the guided
        step attends to it instead of running without a context (pmhip_pipeline_sample_negative); negative_lens: its per-image
        lengths, like context_lens.  Needs guidance_scale.
        topk: an integer in 1..n_embed (Pipeline resolves its topk=None to n_embed before it gets here).
        guidance_scale (None = the reference's step): sample from uncond + scale * (cond - uncond), two tower passes.
        context_lens (None = every image attends to its whole context): image b's cross-attention sees context rows
        [0, context_lens[b]) only (pmhip_pipeline_sample_lens).
        choice_temperature (None or 0 = the reference's step): THIS step's choice temperature -- the re-masking sorts by MaskGIT's
        perturbed confidence (pmhip_pipeline_sample_choice); choice_noise fp32 [B,N]: its uniforms (default: Philox).
        top_p (None or 1 = no nucleus filter: the calls above): the token draw's nucleus mass, 0 < top_p <= 1
        (pmhip_pipeline_sample_nucleus)."""
        B = ids.shape[0]
        ct = ops.choice_t(choice_temperature)
        nucleus = ops.nucleus_p(top_p)
        context, L = self._ctx(context)
        lens, cs, ts, w = _key_args(self._keys(B, L, context_lens, context_segments, token_segments, context_weights, keys))
        img = vq_engine._new_img(B) if want_img else None
        pred = torch.empty(B, self.tokens, device=self.device, dtype=torch.int64) if want_aux else None
        score = torch.empty(B, self.tokens, device=self.device, dtype=torch.float32) if want_aux else None
        if noise is not None:
            noise = noise.to(self.device, torch.float32).contiguous()
        if choice_noise is not None:
            choice_noise = choice_noise.to(self.device, torch.float32).contiguous()
            if tuple(choice_noise.shape) != (B, self.tokens):
                raise ValueError(f"choice_noise must be [B, {self.tokens}]")
        neg_ctx, Ln, neg_lens = self._negative(negative_context, negative_lens, B)
        neg = (_p(neg_ctx), Ln, neg_lens)                 # (neg_ctx lives until the native call has returned)
        # the widest argument list of the entries before there was a negative context: an absent option travels as the value with which
        # the header promises the narrower entry's computation (NULL lengths, guided = 0, choice_t = 0, top_p = 1)
        args = (self.handle, vq_engine.handle if vq_engine is not None else C.c_void_p(0), _p(ids), _p(context), L, B, lens,
                int(topk), float(temperature), int(num_mask), _p(noise), int(seed), int(step), int(image_base), _p(img), _p(pred),
                _p(score), int(guidance_scale is not None), float(guidance_scale or 0.0), ct, _p(choice_noise if ct else None), nucleus)
        with torch.cuda.device(self.device):      # without a negative context the native call is the one made before there was one
            self._call(((w is not None, "pmhip_pipeline_sample_weights", neg + (cs, ts, w)),
                        (cs is not None, "pmhip_pipeline_sample_segments", neg + (cs, ts)),
                        (negative_context is not None, "pmhip_pipeline_sample_negative", neg),
                        (True, "pmhip_pipeline_sample_nucleus", ())), args, (stream_ptr(self.device),))
        return ids, img, pred, score

    def _negative(self, negative_context, negative_lens, B, keep=False):
        """(negative_context, negative_lens) -> (the context on the device or None, Ln, a ctypes int32 [B] or None); the caller
        holds the tensor while the native call reads it.  keep (``step_slots(keep_negative=)``): the negative K/V are kept, the
        context only says how long it is -- None, Ln."""
        if negative_context is None:
            if keep:
                raise ValueError("step_slots: keep_negative needs the negative context it keeps (for its length)")
            if negative_lens is not None:
                raise ValueError("negative_lens needs a negative context")
            return None, 0, None
        if keep:
            if negative_context.dim() != 3 or negative_context.shape[0] != B:
                raise ValueError(f"step_slots: negative context {tuple(negative_context.shape)}, batch of {B}")
            neg, Ln = None, negative_context.shape[1]
        else:
            neg, Ln = self._ctx(negative_context)
            if neg.shape[0] != B:
                raise ValueError(f"negative context for {neg.shape[0]} images, batch of {B}")
        return neg, Ln, _c_ints(ops.host_lens(negative_lens, B, Ln, "negative_lens"))

    def slots_steps(self):
        """(one_pass, two_pass): the slots steps this handle ran, by tower passes (pmhip_s2_slots_steps) -- two passes exactly when
        an active slot of the step was guided"""
        one, two = C.c_int(0), C.c_int(0)
        check(self.lib.pmhip_s2_slots_steps(self.handle, C.byref(one), C.byref(two)), "pmhip_s2_slots_steps")
        return one.value, two.value

    def slots_passes(self):
        """(one_pass, two_pass, three_pass): the slots steps this handle ran, by tower passes (pmhip_s2_slots_passes) -- the
        conditional pass, plus one without a context when an active slot had on == 1, plus one against the negative context when
        one had on == 2"""
        one, two, three = C.c_int(0), C.c_int(0), C.c_int(0)
        check(self.lib.pmhip_s2_slots_passes(self.handle, C.byref(one), C.byref(two), C.byref(three)), "pmhip_s2_slots_passes")
        return one.value, two.value, three.value

    def slots_filter_steps(self):
        """(tiles_only, chain): the steps pmhip_pipeline_step_slots_filter ran on this handle, by the form of their sampling tail --
        the one block-statistics launch (every active slot at topk <= 8 without a nucleus) or the launch per class"""
        tiles, chain = C.c_int(0), C.c_int(0)
        check(self.lib.pmhip_s2_slots_filter_steps(self.handle, C.byref(tiles), C.byref(chain)), "pmhip_s2_slots_filter_steps")
        return tiles.value, chain.value

    def slots_region_steps(self):
        """the steps pmhip_pipeline_step_slots_regions ran on this handle with the two-launch cross-attention (an active slot was
        regional)"""
        steps = C.c_int(0)
        check(self.lib.pmhip_s2_slots_region_steps(self.handle, C.byref(steps)), "pmhip_s2_slots_region_steps")
        return steps.value

    def slots_weight_steps(self):
        """the steps pmhip_pipeline_step_slots_weights ran on this handle with the three-launch cross-attention (an active slot was
        weighted); they are not counted by ``slots_region_steps``"""
        steps = C.c_int(0)
        check(self.lib.pmhip_s2_slots_weight_steps(self.handle, C.byref(steps)), "pmhip_s2_slots_weight_steps")
        return steps.value

    def slots_edit_steps(self):
        """the steps pmhip_pipeline_step_slots_edit ran on this handle with the re-masking form that takes a count per slot"""
        steps = C.c_int(0)
        check(self.lib.pmhip_s2_slots_edit_steps(self.handle, C.byref(steps)), "pmhip_s2_slots_edit_steps")
        return steps.value

    def step_slots(self, ids, context, slots, use_graph=False, keep_context=False, want_aux=True, guides=None, context_lens=None,
                   choice=None, negative_context=None, negative_lens=None, keep_negative=False, top_p=None, counts=None,
                   segments=None, weights=None):
        """one MaskGIT step in which image b runs with slots[b] (a ctypes array of _lib.Slot, HOST records: seed, image_index,
        temperature, topk <= 8, num_mask, step; bit 31 of step = idle); ids int64 [B,N] is updated IN PLACE.  No image: the
        caller decodes the rows it wants.  keep_context: `context` only says whether there is one (None / not None) and its
        length; the cross K/V the previous step_slots call prepared are reused.  guides: a ctypes array of _lib.SlotGuide beside
        `slots` (HOST records: scale, on) -- an active slot with on != 0 samples from uncond + scale * (cond - uncond), and a step
        with such a slot runs the tower twice (pmhip_pipeline_step_slots_guided).  context_lens: per-slot context lengths of THIS
        step (pmhip_pipeline_step_slots_lens; also with keep_context, which keeps the cross K/V only).  choice: one choice
        temperature per slot for THIS step (a list of B floats, 0 = the plain re-masking; pmhip_pipeline_step_slots_choice); None
        or all zero is the step without.
        negative_context fp32 [B, Ln, context_dim]: a slot whose guide record has on == 2 is guided against ITS rows of it instead of
        the pass without a context (on == 1); negative_lens: per-slot lengths of it for THIS step, like context_lens.
        keep_negative: like keep_context for the negative K/V -- `negative_context` only says how long it is.  A step without an
        active on == 2 slot runs what it ran before there was a negative context (pmhip_pipeline_step_slots_negative).
        top_p (None: the routing and the limits above): one nucleus mass per slot for THIS step (a sequence of B values, finite and
        in (0, 1], None = 1), which routes the step to pmhip_pipeline_step_slots_filter -- also when every value is 1: an active
        slot may then carry topk in 1..n_embed, and a step whose active slots all have topk <= 8 and top_p == 1 runs the launches
        and the graph of the entries above.
        counts (None: the steps above): one re-masking count per slot for THIS step (a sequence of B integers in -1..tokens), which
        routes the step to pmhip_pipeline_step_slots_edit with the limits of the `top_p` route: -1 = the record's num_mask, c >= 0 =
        exactly c positions, 0 leaving the row as the sampler merged it (an edit request: DESIGN.md section 4t).  A step in which
        every active slot is at -1 runs the launches and the graph of the `top_p` route.
        segments (None: the steps above): ``(ctx_seg uint8 [B, L], tok_seg uint32 [B, tokens], flags uint8 [B])``, host arrays, which
        route the step to pmhip_pipeline_step_slots_regions with the limits of the `top_p` route: an active
        slot with flags[b] == 1 runs the cross-attention of the pass with the context under its key sets -- ctx_seg[b, k] the
        segment 0..31 of context row k or 255 for padding, tok_seg[b, t] the segments token t attends to --, every other slot under
        its context length; the native entry validates them (a context is required).  A step in which no active slot is flagged
        runs the launches and the graph of the `counts` route.
        weights (None: the steps above; needs `segments`): f32 [B, L], a host array, which routes the step to
        pmhip_pipeline_step_slots_weights: flags[b] is then a KIND -- 0 under the length, 1 under the key sets,
        2 under the key sets and weights[b] (0 or in [2^-20, 2^20]; a weighted slot without regions brings the one-segment layout) --
        and a step with an active slot of kind 2 runs three picked cross-attention launches per layer.  A step without such a slot
        runs the launches and the graph of the `segments` route.
        -> (ids, pred [B,N], score [B,N])"""
        B = ids.shape[0]
        if len(slots) != B:
            raise ValueError(f"step_slots: {len(slots)} slot records for a batch of {B}")
        if guides is not None and len(guides) != B:
            raise ValueError(f"step_slots: {len(guides)} guide records for a batch of {B}")
        if not (ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous() and ids.shape[1] == self.tokens):
            raise ValueError(f"step_slots: ids must be a contiguous int64 [B, {self.tokens}] tensor on the device")
        if keep_context:
            L = 0 if context is None else context.shape[1]
            context = None
        else:
            context, L = self._ctx(context)
        lens = _c_ints(self._keys(B, L, context_lens).lens)
        pred = torch.empty(B, self.tokens, device=self.device, dtype=torch.int64) if want_aux else None
        score = torch.empty(B, self.tokens, device=self.device, dtype=torch.float32) if want_aux else None
        flags = ((_lib.SLOTS_GRAPH if use_graph else 0) | (_lib.SLOTS_KEEP_CONTEXT if keep_context else 0) |
                 (_lib.SLOTS_KEEP_NEGATIVE if keep_negative else 0))
        neg_ctx, Ln, neg_lens = self._negative(negative_context, negative_lens, B, keep=keep_negative)
        neg = (_p(neg_ctx), Ln, neg_lens)                 # (neg_ctx lives until the native call has returned)
        if choice is not None:
            if len(choice) != B:
                raise ValueError(f"step_slots: {len(choice)} choice temperatures for a batch of {B}")
            vals = [ops.choice_t(v, f"step_slots: slot {b}: choice temperature") for b, v in enumerate(choice)]
            choice = (C.c_float * B)(*vals) if any(vals) else None
        # the widest entry of the family as it was before a slot could carry a negative prompt (NULL lengths, guides or choice: the
        # step without them) -- unless this step has something only the entry with a negative context reads: that context, kept or
        # given, or a guide record whose `on` names a kind beyond 1 (which that entry validates)
        kinds = guides is not None and any(g.on > _lib.GUIDE_UNCOND for g in guides)
        if top_p is not None:
            if len(top_p) != B:
                raise ValueError(f"step_slots: {len(top_p)} nucleus masses for a batch of {B}")
            # checked like ops.sample_rows checks its top_p; an idle slot's value is not looked at (it travels as 1)
            top_p = (C.c_float * B)(*[1.0 if slots[b].step & _lib.SLOT_IDLE else ops.nucleus_p(v, f"step_slots: slot {b}: top_p")
                                      for b, v in enumerate(top_p)])
        if counts is not None:
            if len(counts) != B:
                raise ValueError(f"step_slots: {len(counts)} re-masking counts for a batch of {B}")
            vals = [0 if slots[b].step & _lib.SLOT_IDLE else int(v) for b, v in enumerate(counts)]
            for b, v in enumerate(vals):
                if not -1 <= v <= self.tokens:
                    raise ValueError(f"step_slots: slot {b}: count {v} must be in -1..{self.tokens}")
            counts = (C.c_int * B)(*vals)
        if segments is not None:
            cs, ts, fl = (np.ascontiguousarray(a, dtype=t) for a, t in zip(segments, (np.uint8, np.uint32, np.uint8)))
            if cs.shape != (B, L) or ts.shape != (B, self.tokens) or fl.shape != (B,):
                raise ValueError(f"step_slots: segments {cs.shape}, {ts.shape}, {fl.shape}: expected ({B}, {L}), ({B}, {self.tokens}), ({B},)")
            segments = tuple(a.ctypes.data_as(C.POINTER(t)) for a, t in ((cs, C.c_ubyte), (ts, C.c_uint32), (fl, C.c_ubyte)))
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != (B, L):
                raise ValueError(f"step_slots: weights {w.shape}: expected ({B}, {L})")
            weights = w.ctypes.data_as(C.POINTER(C.c_float))
        none = (None, None, None)
        with torch.cuda.device(self.device):
            self._call(((weights is not None, "pmhip_pipeline_step_slots_weights", neg + (top_p, counts) + (segments or none) + (weights,)),
                        (segments is not None, "pmhip_pipeline_step_slots_regions", neg + (top_p, counts) + (segments or none)),
                        (counts is not None, "pmhip_pipeline_step_slots_edit", neg + (top_p, counts)),
                        (top_p is not None, "pmhip_pipeline_step_slots_filter", neg + (top_p,)),
                        (negative_context is not None or kinds, "pmhip_pipeline_step_slots_negative", neg),
                        (True, "pmhip_pipeline_step_slots_choice", ())),
                       (self.handle, _p(ids), _p(context), L, B, lens, slots, guides, choice),
                       (flags, _p(pred), _p(score), stream_ptr(self.device)))
        return ids, pred, score

    def generate(self, vq_engine, ids, context, temps, nmask, decode_flags, topk, seed=0, image_base=0, use_graph=False,
                 host=None, want_device_imgs=True, guidance_scale=None, concurrent_lanes=False, from_mask=False, context_lens=None,
                 choice_temps=None, top_p=None, negative_context=None, negative_lens=None, guidance_scales=None, nmask_img=None,
                 context_segments=None, token_segments=None, context_weights=None, keys=None):
        """T MaskGIT steps in one native call; returns imgs [n_decoded, B, C, H, W] (device) or None.

        context_weights (None = the loops below): prompt weights (pmhip_pipeline_generate_weights); the captured loop reads their
        bias array from device memory: one graph serves every set of weights.

        context_segments / token_segments (None = the loops below): regional prompts (pmhip_pipeline_generate_segments); the captured
        loop reads them from device memory: one graph serves every layout.

        keys (instead of these three and context_lens): the call's checked ``ops.Keys``.

        nmask_img (None = the loops below): the EDIT loop (pmhip_pipeline_generate_edit) -- T rows of B integers, step t re-masking
        nmask_img[t][b] positions of image b (0: none) instead of nmask[t] of every image; a decoded step then decodes the merged
        ids, not the predictions at all positions, and the loop starts from `ids` (from_mask is refused).  `nmask` is ignored.
        The captured loop reads the table from device memory: one graph serves every set of masks.

        negative_context / negative_lens: as in ``sample``.  guidance_scales: one finite scale per step (a list of T floats) instead of
        the one guidance_scale, which is then ignored -- the captured loop reads them from device memory: one graph serves every
        schedule.  Without any of the three the native call is the one made before they existed; with any of them it is ONE call to
        pmhip_pipeline_generate_negative, absent ones at their neutral values (NULL).

        topk: an integer in 1..n_embed, the same for every step; part of the key of a captured graph.

        host = (pinned float32 tensor [n_decoded, B_total, C, H, W], first row of this batch, copy stream): every decoded
        image is copied into its rows on the copy stream as soon as it is complete (the reference's `img.cpu()`,
        generate.py:195-196); the caller synchronises that stream.
        concurrent_lanes: other micro-batches run beside this call on other streams (PMHIP_GENERATE_CONCURRENT_LANES: the loop
        then does not put a small batch's decode on a side stream of its own).
        from_mask: the loop starts from the all-mask state (PMHIP_GENERATE_FROM_MASK): the native call writes that state itself --
        what `ids` holds on entry is ignored -- and an unconditional loop samples its step 0 from the handle's shared logits.
        context_lens: per-image context lengths (pmhip_pipeline_generate_lens); the captured graphs read them from device memory.
        choice_temps: one choice temperature per step (pmhip_pipeline_generate_choice); None or all zero is the loop without.
        top_p (None or 1 = no nucleus filter: the calls above): every step's nucleus mass, 0 < top_p <= 1
        (pmhip_pipeline_generate_nucleus); below 1 part of the key of a captured graph, like topk."""
        B = ids.shape[0]
        T = len(temps)
        nucleus = ops.nucleus_p(top_p)
        if choice_temps is not None:
            if len(choice_temps) != T:
                raise ValueError(f"generate: {len(choice_temps)} choice temperatures for {T} steps")
            vals = [ops.choice_t(v, f"generate: step {i}: choice temperature") for i, v in enumerate(choice_temps)]
            choice_temps = (C.c_float * T)(*vals) if any(vals) else None
        context, L = self._ctx(context)
        lens, cs, ts, w = _key_args(self._keys(B, L, context_lens, context_segments, token_segments, context_weights, keys))
        if w is not None and nmask_img is not None:
            raise ValueError("generate: the edit loop takes no prompt weights")
        if cs is not None and nmask_img is not None:
            raise ValueError("generate: the edit loop takes no regional prompts")
        n_dec = int(sum(1 for f in decode_flags if f))
        imgs = None
        if n_dec and (want_device_imgs or host is None):
            imgs = torch.empty(n_dec, B, vq_engine.channels, vq_engine.image_size, vq_engine.image_size, device=self.device,
                               dtype=torch.float32)
        host_ptr, host_stride, copy_stream = C.c_void_p(0), 0, C.c_void_p(0)
        if host is not None and n_dec:
            buf, row0, cstream = host
            if not (buf.is_pinned() and buf.dtype == torch.float32 and buf.is_contiguous() and buf.shape[0] == n_dec):
                raise ValueError("host image buffer must be a pinned contiguous float32 tensor [n_decoded, B_total, C, H, W]")
            per_img = buf[0, 0].numel()
            host_ptr = C.c_void_p(buf.data_ptr() + row0 * per_img * 4)
            host_stride = buf.shape[1] * per_img
            copy_stream = C.c_void_p(cstream.cuda_stream)
        temps_c = (C.c_float * T)(*[float(t) for t in temps])
        if nmask_img is not None:
            rows = [[int(n) for n in row] for row in nmask_img]
            if len(rows) != T or any(len(row) != B for row in rows):
                raise ValueError(f"generate: nmask_img must hold {T} rows of {B} counts")
            if from_mask:
                raise ValueError("generate: an edit loop starts from its ids (from_mask)")
            nmask_c = (C.c_int * (T * B))(*[n for row in rows for n in row])
        else:
            nmask_c = (C.c_int * T)(*[int(n) for n in nmask])
        dec_c = (C.c_ubyte * T)(*[1 if f else 0 for f in decode_flags])
        flags = ((_lib.GENERATE_GRAPH if use_graph else 0) | (_lib.GENERATE_CONCURRENT_LANES if concurrent_lanes else 0) |
                 (_lib.GENERATE_FROM_MASK if from_mask else 0))
        neg_ctx, Ln, neg_lens = self._negative(negative_context, negative_lens, B)
        neg = (_p(neg_ctx), Ln, neg_lens)                 # (neg_ctx lives until the native call has returned)
        gscales = None
        if guidance_scales is not None:
            gscales = (C.c_float * T)(*ops.guidance_scales(guidance_scales, T, "generate: guidance_scales"))
        guided = guidance_scale is not None or gscales is not None
        # the widest argument list of the loops before there was a negative context, absent options as the header's neutral values
        # (see sample); behind it what only the later entries read -- without any of it the call is the one made before they existed
        args = (self.handle, vq_engine.handle if vq_engine is not None else C.c_void_p(0), _p(ids), _p(context), L, B, lens, T,
                temps_c, nmask_c, dec_c, int(topk), int(seed), int(image_base), _p(imgs), flags, stream_ptr(self.device), host_ptr,
                host_stride, copy_stream, int(guided), float(guidance_scale or 0.0), choice_temps, nucleus)
        with torch.cuda.device(self.device):
            self._call(((w is not None, "pmhip_pipeline_generate_weights", neg + (gscales, cs, ts, w)),
                        (cs is not None, "pmhip_pipeline_generate_segments", neg + (gscales, cs, ts)),
                        (nmask_img is not None, "pmhip_pipeline_generate_edit", neg + (gscales,)),
                        (negative_context is not None or gscales is not None, "pmhip_pipeline_generate_negative", neg + (gscales,)),
                        (True, "pmhip_pipeline_generate_nucleus", ())), args)
        return ids, imgs
