"""The Flan-T5 encoder on the HIP path: Hugging Face's ``T5EncoderModel`` keeps the parameters -- so a state_dict
keeps its ``text_model.transformer.*`` keys, the checkpoint contract -- and ``NativeT5Encoder`` runs its arithmetic on the library's
kernels: the generic GEMMs, ``gemm_heads`` and ``embed_rows`` that already serve these shapes, and the three operators a T5 adds
(``ops.rmsnorm``, ``ops.geglu``, ``ops.attention_relbias``).

The residual stream is float32 in both compute dtypes; in bfloat16 the GEMM and attention operands are bfloat16 with float32
accumulation, and every operator rounds its output once.  Nothing here falls back to ATen: a config the kernels do not serve is
refused at construction, naming the field.
"""
import math

import torch

from .. import ops, packing
from .._lib import PART_K, PART_Q, PART_V


def relative_position_bucket(delta, num_buckets=32, max_distance=128):
    """The bucket of the relative position delta = key - query in a BIDIRECTIONAL T5 stack: a restatement of Hugging Face's
    ``T5Attention._relative_position_bucket(bidirectional=True)`` for int64 deltas.  Half of the buckets serve delta > 0; in each half
    the first half is exact (|delta| < num_buckets / 4), the rest logarithmic up to max_distance, beyond which the last bucket."""
    delta = torch.as_tensor(delta, dtype=torch.long)
    half = num_buckets // 2
    bucket = (delta > 0).to(torch.long) * half
    dist = delta.abs()
    max_exact = half // 2
    large = max_exact + (torch.log(dist.float() / max_exact) / math.log(max_distance / max_exact) * (half - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, half - 1))
    return bucket + torch.where(dist < max_exact, dist, large)


def rel_bias_table(weight, L, num_buckets=32, max_distance=128):
    """weight [num_buckets, H] (block 0's ``relative_attention_bias``; every layer shares it, as in HF) -> float32 [H, 2L-1] on weight's
    device: entry (k - q) + L - 1 of row h is the bias head h adds to the score of query q and key k.  The bucket depends on k - q
    alone, so the table is all of HF's [1, H, L, L] ``position_bias``.  ``NativeT5Encoder`` keeps one per L beside its packed weights
    (a table lives exactly as long as the packing it was gathered from)."""
    buckets = relative_position_bucket(torch.arange(-(L - 1), L), num_buckets, max_distance).to(weight.device)
    return weight.detach().float()[buckets].t().contiguous()              # [2L-1, H] -> [H, 2L-1]


def check_config(cfg):
    """what the kernels serve; anything else is a ValueError naming the config field"""
    if cfg.d_kv != 64:
        raise ValueError(f"NativeT5Encoder: d_kv={cfg.d_kv} is not served (the attention kernel is built for d_kv == 64)")
    if not getattr(cfg, "is_gated_act", False) or cfg.dense_act_fn != "gelu_new":
        raise ValueError(f"NativeT5Encoder: feed_forward_proj={cfg.feed_forward_proj!r} (is_gated_act={getattr(cfg, 'is_gated_act', False)}, "
                         f"dense_act_fn={cfg.dense_act_fn!r}) is not served: only the gated GELU (is_gated_act with dense_act_fn 'gelu_new')")
    if cfg.d_model % 64 or cfg.d_model > 4096:
        raise ValueError(f"NativeT5Encoder: d_model={cfg.d_model} is not served (a multiple of 64, at most 4096)")
    if cfg.d_ff % 64:
        raise ValueError(f"NativeT5Encoder: d_ff={cfg.d_ff} is not served (a multiple of 64)")


class NativeT5Encoder:
    """Runs ``model`` (a Hugging Face ``T5EncoderModel``) on the HIP kernels.  Owns no parameter: it packs the module's weights per
    (device, compute dtype), lazily at the first call, and re-packs when ``packing.params_fingerprint`` changes (``.to()``,
    ``load_state_dict``, in-place edits)."""

    def __init__(self, model):
        check_config(model.config)
        self.model = model
        self._packs = {}

    def packed(self, dtype):
        """-> dict: per layer ``qkv`` [3*H*64, D], ``o`` [D, H*64], ``wi`` [2F, D] (wi_0 above wi_1), ``wo`` [D, F] in `dtype`, ``ln1`` /
        ``ln2`` f32 [D]; ``final`` f32 [D]; ``embed`` = the module's own f32 table (no copy); ``bias`` = block 0's bucket weights,
        ``tables`` = the [H, 2L-1] bias tables gathered from them so far, by L"""
        enc = self.model.encoder
        dev = enc.final_layer_norm.weight.device
        stamp = packing.params_fingerprint(self.model)
        hit = self._packs.get((dev, dtype))
        if hit is not None and hit[0] == stamp:
            return hit[1]
        self._packs = {k: v for k, v in self._packs.items() if v[0] == stamp}       # stale packings of other dtypes go too

        def w(*mods):
            return torch.cat([m.weight.detach().float() for m in mods], 0).to(dtype).contiguous()

        layers = []
        for blk in enc.block:
            att, ff = blk.layer[0], blk.layer[1]
            sa, dense = att.SelfAttention, ff.DenseReluDense
            layers.append(dict(ln1=att.layer_norm.weight.detach().float().contiguous(), qkv=w(sa.q, sa.k, sa.v), o=w(sa.o),
                               ln2=ff.layer_norm.weight.detach().float().contiguous(), wi=w(dense.wi_0, dense.wi_1), wo=w(dense.wo)))
        table = self.model.shared.weight
        if table.dtype != torch.float32:
            raise TypeError(f"NativeT5Encoder: the embedding table is {table.dtype}; the tower's parameters must be float32 (the compute "
                            "dtype is chosen per call, the checkpoint stays fp32 as the reference loads it)")
        pack = dict(layers=layers, final=enc.final_layer_norm.weight.detach().float().contiguous(), embed=table,
                    bias=enc.block[0].layer[0].SelfAttention.relative_attention_bias.weight, tables={})
        self._packs[(dev, dtype)] = (stamp, pack)
        return pack

    @torch.no_grad()
    def __call__(self, input_ids, kv_lens=None, dtype=torch.float32):
        """input_ids int64 [B, L] on the tower's GPU; kv_lens None or int32 [B] (device or host): prompt b attends to its first
        kv_lens[b] keys -> last_hidden_state float32 [B, L, d_model].  Eager, on the caller's current stream."""
        cfg = self.model.config
        if not input_ids.is_cuda:
            raise RuntimeError("NativeT5Encoder runs on a ROCm device only (the CPU gets the Hugging Face tower)")
        pack = self.packed(dtype)
        B, L = input_ids.shape
        D, H, F, eps = cfg.d_model, cfg.num_heads, cfg.d_ff, float(cfg.layer_norm_epsilon)
        bias = pack["tables"].get(L)
        if bias is None:
            bias = pack["tables"][L] = rel_bias_table(pack["bias"], L, cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance)
        if kv_lens is not None:
            kv_lens = torch.as_tensor(kv_lens).to(device=input_ids.device, dtype=torch.int32).contiguous()
        x = ops.embed_rows(pack["embed"], input_ids.reshape(-1).contiguous(), D, torch.float32)      # the f32 residual stream [B*L, D]
        for lw in pack["layers"]:
            h = ops.rmsnorm(x, lw["ln1"], eps, dtype)
            q, k, vt = ops.gemm_heads(h, lw["qkv"], H, L, [PART_Q, PART_K, PART_V], q_scale=1.0)
            a = ops.attention_relbias(q, k, vt, bias, kv_lens)
            ops.gemm(a, lw["o"], residual=x, out=x)
            h = ops.rmsnorm(x, lw["ln2"], eps, dtype)
            u = ops.gemm(h, lw["wi"], out_dtype=torch.float32)
            g = ops.geglu(u, dtype)
            ops.gemm(g, lw["wo"], residual=x, out=x)
        return ops.rmsnorm(x, pack["final"], eps, torch.float32).view(B, L, D)
