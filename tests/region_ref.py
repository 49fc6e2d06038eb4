"""The float64 restatement of REGIONAL PROMPTS (include/pmhip.h, pmhip_attention_segments), shared by
tests/test_regions_cpu.py, tests/test_gpu_attention_segments.py and tests/test_gpu_regions.py.

The contract.  Image b's context is a list of rows, each with a segment: 0..31, or 255 for padding.  Every query (token) carries a
32-bit mask.  Key k takes part in query q's softmax iff ``seg[b, k] < 32 and (mask[b, q] >> seg[b, k]) & 1``; every other key has
weight exactly 0 for that query, and a padding row reaches no result whatever it holds, NaN included.

Everything here is written for clarity, not speed, and shares no code with the package: loops over images, float64 torch, a softmax
per query over the allowed keys only.
"""
import numpy as np
import torch

LN2 = float(np.log(2.0))
PAD = 255


def allowed(key_seg, query_mask):
    """key_seg [B, Nkv] ints (255 / -1 = padding), query_mask [B, Nq] ints -> bool numpy [B, Nq, Nkv]"""
    ks = np.asarray(key_seg).astype(np.int64)
    qm = np.asarray(query_mask).astype(np.int64) & 0xFFFFFFFF
    B, Nkv = ks.shape
    out = np.zeros((B, qm.shape[1], Nkv), bool)
    for b in range(B):
        for k in range(Nkv):
            s = int(ks[b, k])
            if 0 <= s < 32:
                out[b, :, k] = ((qm[b] >> s) & 1) == 1
    return out


def attention(q, k, v, key_seg, query_mask, exp2):
    """q [B, H, Nq, dh], k / v [B, H, Nkv, dh] (what the kernel sees: q scaled and rounded), the two arrays of one launch ->
    float64 numpy (ref [B, H, Nq, dh], A = sum_j p_ij |v_je|, s [B, H, Nq, Nkv] in the kernel's unit with -inf where denied): the
    triple of attention_probes.reference under the mask.  Padding rows of k / v are never read."""
    ok = torch.from_numpy(allowed(key_seg, query_mask))[:, None]                     # [B, 1, Nq, Nkv]
    pad = torch.from_numpy((np.asarray(key_seg).astype(np.int64) & 0xFF) == PAD)     # -1 & 0xFF = 255
    q, k, v = (torch.as_tensor(np.asarray(x, np.float64)) for x in (q, k, v))
    k = torch.where(pad[:, None, :, None], torch.zeros_like(k), k)
    v = torch.where(pad[:, None, :, None], torch.zeros_like(v), v)
    s = q @ k.transpose(-1, -2)
    s = torch.where(ok, s, torch.full_like(s, float("-inf")))
    assert bool(ok.any(-1).all()), "every query must allow at least one key"
    p = torch.softmax(s * LN2 if exp2 else s, dim=-1)
    return (p @ v).numpy(), (p @ v.abs()).numpy(), s.numpy()


def averaged_keys(key_seg, query_mask):
    """-> per (b, q) the sorted list of key indices that take part (for the selector probes)"""
    ok = allowed(key_seg, query_mask)
    return [[np.flatnonzero(ok[b, i]).tolist() for i in range(ok.shape[1])] for b in range(ok.shape[0])]


def token_mask_of(mask, image_size, patch):
    """a region's mask -> bool numpy [g * g]: a bool [g, g] token mask as it is; of a pixel mask [H, W] a token is part iff any
    pixel of its patch is non-zero"""
    m = np.asarray(mask)
    g = image_size // patch
    if m.shape == (g, g) and m.dtype == bool:
        return m.reshape(-1).copy()
    assert m.shape == (image_size, image_size), m.shape
    out = np.zeros((g, g), bool)
    for i in range(g):
        for j in range(g):
            out[i, j] = bool((m[i * patch:(i + 1) * patch, j * patch:(j + 1) * patch] != 0).any())
    return out.reshape(-1)


def layout(global_rows, regions, image_size, patch):
    """global_rows: per image a [L0, D] tensor (the global prompt's rows); regions: per image a list of (rows [L_r, D], mask).
    -> (context float32 [B, Lmax, D] zero-filled behind an image's rows, key_seg uint8 [B, Lmax] with 255 there,
    query_mask uint32 [B, g * g]: bit 0, plus bit r for every region r = 1.. the token is part of)"""
    B = len(global_rows)
    g = image_size // patch
    parts = [[global_rows[b]] + [rows for rows, _ in regions[b]] for b in range(B)]
    Lmax = max(sum(int(p.shape[0]) for p in ps) for ps in parts)
    D = int(global_rows[0].shape[1])
    context = torch.zeros(B, Lmax, D, dtype=torch.float32)
    key_seg = np.full((B, Lmax), PAD, np.uint8)
    query_mask = np.zeros((B, g * g), np.uint32)
    for b in range(B):
        at = 0
        for r, rows in enumerate(parts[b]):
            n = int(rows.shape[0])
            context[b, at:at + n] = rows.float()
            key_seg[b, at:at + n] = r
            at += n
        for t in range(g * g):
            bits = 1
            for r, (_, mask) in enumerate(regions[b], start=1):
                if token_mask_of(mask, image_size, patch)[t]:
                    bits |= 1 << r
            query_mask[b, t] = bits
    return context, key_seg, query_mask


def cross_attention(attn, x, context, key_seg, query_mask):
    """``CrossAttention`` (weights read from the module, nothing else) on x [B, N, D] and context [B, L, Dc] in float64 under the
    mask -> float64 tensor [B, N, D] (to_out included, no residual).  Padding rows of the context are never read."""
    f = lambda t: t.detach().double()
    B, N, _ = x.shape
    h, d = attn.heads, attn.dim_head
    pad = torch.from_numpy((np.asarray(key_seg).astype(np.int64) & 0xFF) == PAD)
    c = torch.where(pad[:, :, None], torch.zeros_like(f(context)), f(context))
    split = lambda t, n: t.reshape(B, n, h, d).permute(0, 2, 1, 3)
    q = split(f(x) @ f(attn.to_q.weight).T * (d ** -0.5), N)
    k = split(c @ f(attn.to_k.weight).T, c.shape[1])
    v = split(c @ f(attn.to_v.weight).T, c.shape[1])
    ref, _, _ = attention(q.numpy(), k.numpy(), v.numpy(), key_seg, query_mask, exp2=False)
    o = torch.from_numpy(ref).permute(0, 2, 1, 3).reshape(B, N, h * d)
    return o @ f(attn.to_out[0].weight).T + f(attn.to_out[0].bias)
