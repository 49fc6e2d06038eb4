"""The OpenCLIP text tower on the HIP path: the open_clip-interface module keeps the parameters -- so a
state_dict keeps its ``text_model.model.*`` keys, the checkpoint contract -- and ``NativeClipText`` runs its arithmetic on the library's
kernels: the generic GEMMs (bias and in-place f32 residual), ``layernorm``, ``embed_rows`` and ``add_rows`` that already serve these
shapes, and the three operators a CLIP text tower adds (``ops.split_heads``, ``ops.attention_causal``, ``ops.gelu``).

The residual stream is float32 in both compute dtypes; in bfloat16 the GEMM and attention operands are bfloat16 with float32
accumulation, and every operator rounds its output once.  Nothing here falls back to ATen: a tower the kernels do not serve is
refused at construction, naming what is wrong.  Written against the open_clip interface (``token_embedding``, ``positional_embedding``,
``transformer.resblocks`` of ``ln_1, attn, ls_1, ln_2, mlp(c_fc, gelu, c_proj), ls_2``, ``attn_mask``, ``ln_final``).
"""
import torch
import torch.nn as nn

from .. import ops, packing
from .._lib import PART_K, PART_Q, PART_V

WHO = "NativeClipText"


def gelu_kind(act):
    """the ``ops.gelu`` kind of an MLP's activation module, or None"""
    if isinstance(act, nn.GELU):
        return "erf" if getattr(act, "approximate", "none") == "none" else None
    return "quick" if type(act).__name__ == "QuickGELU" else None


def check_tower(model):
    """what the kernels serve; anything else is a ValueError naming what is wrong -> (width, heads, one gelu kind per block)"""
    width = int(model.positional_embedding.shape[1])
    blocks = list(model.transformer.resblocks)
    if not blocks:
        raise ValueError(f"{WHO}: transformer.resblocks is empty")
    if width % 64:
        raise ValueError(f"{WHO}: width={width} is not served (a multiple of 64: the attention kernel is built for dim_head 64)")
    for p in model.parameters():
        if p.dtype != torch.float32:
            raise ValueError(f"{WHO}: the tower's parameters must be float32, found {p.dtype} (the compute dtype is chosen per call, the "
                             "checkpoint stays fp32 as the reference loads it)")
    mask = getattr(model, "attn_mask", None)
    n_ctx = int(model.positional_embedding.shape[0])
    if mask is None:
        raise ValueError(f"{WHO}: attn_mask is missing (the kernel is causal; a tower without a mask is not served)")
    causal = torch.full((n_ctx, n_ctx), float("-inf")).triu_(1)
    if tuple(mask.shape) != (n_ctx, n_ctx) or not torch.equal(mask.detach().float().cpu(), causal):
        raise ValueError(f"{WHO}: attn_mask is not the causal matrix (-inf strictly above the diagonal, 0 elsewhere, "
                         f"[{n_ctx}, {n_ctx}]); only that mask is served")
    heads, kinds = None, []
    for i, blk in enumerate(blocks):
        attn = getattr(blk, "attn", None)
        if not isinstance(attn, nn.MultiheadAttention) or attn.in_proj_weight is None or attn.in_proj_bias is None:
            raise ValueError(f"{WHO}: resblocks[{i}].attn must be an nn.MultiheadAttention with in_proj_weight and in_proj_bias, got "
                             f"{type(attn).__name__}")
        if attn.embed_dim != width or attn.num_heads * 64 != width or (heads is not None and attn.num_heads != heads):
            raise ValueError(f"{WHO}: resblocks[{i}].attn has heads={attn.num_heads} at width {attn.embed_dim}: heads * 64 must equal the "
                             f"width {width} (dim_head 64 only)")
        heads = attn.num_heads
        for name in ("ls_1", "ls_2"):
            if not isinstance(getattr(blk, name, None), nn.Identity):
                raise ValueError(f"{WHO}: resblocks[{i}].{name} must be nn.Identity (a layer scale is not served), got "
                                 f"{type(getattr(blk, name, None)).__name__}")
        mlp = getattr(blk, "mlp", None)
        parts = list(mlp.named_children()) if isinstance(mlp, nn.Module) else []
        if [k for k, _ in parts][0::2] != ["c_fc", "c_proj"] or len(parts) != 3 or not all(isinstance(parts[j][1], nn.Linear) for j in (0, 2)):
            raise ValueError(f"{WHO}: resblocks[{i}].mlp must be c_fc, an activation, c_proj (two nn.Linear around a GELU), got "
                             f"{[k for k, _ in parts]}")
        kind = gelu_kind(parts[1][1])
        if kind is None:
            raise ValueError(f"{WHO}: resblocks[{i}].mlp activation {parts[1][1]!r} is not served: nn.GELU(approximate='none') or a module "
                             "whose class is named QuickGELU")
        if mlp.c_fc.bias is None or mlp.c_proj.bias is None or attn.out_proj.bias is None or mlp.c_fc.out_features % 4:
            raise ValueError(f"{WHO}: resblocks[{i}] needs biases on out_proj, c_fc and c_proj and an MLP width that is a multiple of 4")
        kinds.append(kind)
    return width, heads, kinds


class NativeClipText:
    """Runs ``model`` (the open_clip text-tower interface) on the HIP kernels; ``skip_last`` blocks at the end are left out (the
    embedder's ``layer="penultimate"`` is 1).  Owns no parameter: it packs the module's weights per (device, compute dtype), lazily at
    the first call, and re-packs when ``packing.params_fingerprint`` changes (``.to()``, ``load_state_dict``, in-place edits)."""

    def __init__(self, model, skip_last=0):
        self.width, self.heads, self.kinds = check_tower(model)
        self.model = model
        self.skip_last = int(skip_last)
        self._packs = {}

    def packed(self, dtype):
        """-> dict: per block ``qkv`` [3W, W] (in_proj_weight), ``o`` [W, W], ``fc`` [F, W], ``proj`` [W, F] in `dtype`; ``qkv_b``, ``o_b``,
        ``fc_b``, ``proj_b``, ``ln1_w/b``, ``ln2_w/b`` f32, ``eps1``, ``eps2``, ``act``; ``final_w/b`` f32 and ``final_eps``; ``embed`` and
        ``pos`` = the module's own f32 parameters (no copy)"""
        m = self.model
        dev = m.ln_final.weight.device
        stamp = packing.params_fingerprint(m)
        hit = self._packs.get((dev, dtype))
        if hit is not None and hit[0] == stamp:
            return hit[1]
        self._packs = {k: v for k, v in self._packs.items() if v[0] == stamp}       # stale packings of other dtypes go too

        def w(t):
            return t.detach().to(dtype).contiguous()

        def f(t):
            return t.detach().float().contiguous()

        layers = []
        for blk, act in zip(m.transformer.resblocks, self.kinds):
            a, mlp = blk.attn, blk.mlp
            layers.append(dict(qkv=w(a.in_proj_weight), qkv_b=f(a.in_proj_bias), o=w(a.out_proj.weight), o_b=f(a.out_proj.bias),
                               fc=w(mlp.c_fc.weight), fc_b=f(mlp.c_fc.bias), proj=w(mlp.c_proj.weight), proj_b=f(mlp.c_proj.bias),
                               ln1_w=f(blk.ln_1.weight), ln1_b=f(blk.ln_1.bias), eps1=float(blk.ln_1.eps),
                               ln2_w=f(blk.ln_2.weight), ln2_b=f(blk.ln_2.bias), eps2=float(blk.ln_2.eps), act=act))
        pack = dict(layers=layers, final_w=f(m.ln_final.weight), final_b=f(m.ln_final.bias), final_eps=float(m.ln_final.eps),
                    embed=m.token_embedding.weight, pos=m.positional_embedding)
        self._packs[(dev, dtype)] = (stamp, pack)
        return pack

    @torch.no_grad()
    def __call__(self, tokens, dtype=torch.float32):
        """tokens int64 [B, n_ctx] on the tower's GPU -> ln_final of the last served block, float32 [B, n_ctx, width].  Eager, on the
        caller's current stream."""
        if not tokens.is_cuda:
            raise RuntimeError(f"{WHO} runs on a ROCm device only (the CPU gets the stock tower)")
        pack = self.packed(dtype)
        B, L = tokens.shape
        W, H = self.width, self.heads
        if L != pack["pos"].shape[0]:
            raise ValueError(f"{WHO}: {L} tokens per prompt, but positional_embedding has {pack['pos'].shape[0]} rows (a prompt is "
                             "exactly n_ctx tokens)")
        layers = pack["layers"]
        x = ops.embed_rows(pack["embed"], tokens.reshape(-1).contiguous(), W, torch.float32)
        x = ops.add_rows(x, pack["pos"])                                             # the f32 residual stream [B*L, W]
        for lw in layers[:len(layers) - self.skip_last]:
            h = ops.layernorm(x, lw["ln1_w"], lw["ln1_b"], lw["eps1"], dtype)
            u = ops.gemm(h, lw["qkv"], bias=lw["qkv_b"], out_dtype=torch.float32)
            q, k, vt = ops.split_heads(u, H, L, [PART_Q, PART_K, PART_V], q_scale=64 ** -0.5, dtype=dtype)
            a = ops.attention_causal(q, k, vt)
            ops.gemm(a, lw["o"], bias=lw["o_b"], residual=x, out=x)
            h = ops.layernorm(x, lw["ln2_w"], lw["ln2_b"], lw["eps2"], dtype)
            u = ops.gemm(h, lw["fc"], bias=lw["fc_b"], out_dtype=torch.float32)
            g = ops.gelu(u, dtype, lw["act"])
            ops.gemm(g, lw["proj"], bias=lw["proj_b"], residual=x, out=x)
        return ops.layernorm(x, pack["final_w"], pack["final_b"], pack["final_eps"], torch.float32).view(B, L, W)
