"""References for the negative-prompt tests (not a conftest, not collected): the step composed from the operator-level entries,
the oracle's step with a second conditioned forward, and a text model whose prompts have rows and lengths of their own."""
import hashlib

import numpy as np
import torch

from oracle import paintmind_oracle as O
from paintmind_amd import ops


def composed_step(pipe, ids, nm, ctx, ctx_lens, neg, neg_lens, topk, temperature, noise, seed, step, image_base, scale):
    """Pipeline._sample_guided_composed with the second forward taking the negative context and its lengths: two
    pmhip_s2_forward_lens + pmhip_guidance_combine + pmhip_sample_rows + decode + pmhip_remask -- the kernels of
    pmhip_pipeline_sample_negative, in its order"""
    eng = pipe.engine()
    ids = ids.to(eng.device, torch.int64).clone().contiguous()
    B, N = ids.shape
    tok = pipe.ids2tokens(ids)
    cond = eng.forward(tok, ctx, context_lens=ctx_lens)
    negl = eng.forward(tok, neg, context_lens=neg_lens)
    logits = ops.guidance_combine(cond, negl, scale, out=cond)
    if noise is not None:
        noise = noise.to(eng.device, torch.float32).reshape(B * N, -1).contiguous()
    pred, merged, score = ops.sample_rows(logits.reshape(B * N, -1), ids.reshape(-1), pipe.mask_token_id, topk, temperature, noise=noise,
                                          seed=seed, step=step, row_base=image_base * N)
    img = pipe.vqgan.decode_from_indice(pred.reshape(B, N))
    return ops.remask(merged.reshape(B, N), score.reshape(B, N), nm, pipe.mask_token_id), img


def oracle_negative_step(ids, mask_ratio, context, negative, topk, temperature, noise, p, cfg, s2cfg, scale):
    """oracle.sample_step with guidance against a negative context: O.cond_transformer twice, the oracle's one fused multiply-add
    per element in float32, then the oracle's existing tail (sample_rows, decode, remask) -> (ids', img)"""
    B, N = ids.shape
    tok = O.ids2tokens(ids, p)
    cond, neg = O.cond_transformer(tok, context, p, s2cfg), O.cond_transformer(tok, negative, p, s2cfg)
    diff = (cond - neg).astype(np.float32)
    logits = (np.float64(np.float32(scale)) * diff.astype(np.float64) + neg.astype(np.float64)).astype(np.float32)
    V = logits.shape[-1]
    pred, merged, score = O.sample_rows(logits.reshape(B * N, V), ids.reshape(-1), cfg["n_embed"], topk, temperature, noise.reshape(B * N, V))
    vq_p = {k[len("vqgan."):]: v for k, v in p.items() if k.startswith("vqgan.")}
    img = O.vqgan_decode_indices(pred.reshape(B, N), vq_p, cfg)
    return O.remask(merged.reshape(B, N), score.reshape(B, N), O.num_token_masked(mask_ratio, N), cfg["n_embed"]), img


class PromptRows(torch.nn.Module):
    """a text model for tests: the rows of a prompt are N(0,1) features keyed by the prompt's own characters; a prompt that starts
    with "not " has `neg_rows` rows, every other one `rows`; return_lens gives every prompt a length of its own in [1, rows]"""

    def __init__(self, context_dim, rows=7, neg_rows=3):
        super().__init__()
        self.context_dim, self.rows, self.neg_rows = context_dim, rows, neg_rows
        self.register_buffer("_anchor", torch.zeros(1), persistent=False)

    @staticmethod
    def _key(prompt):
        return int.from_bytes(hashlib.sha256(prompt.encode()).digest()[:4], "little")

    def forward(self, text, return_lens=False):
        out, lens = [], []
        for prompt in text:
            L = self.neg_rows if prompt.startswith("not ") else self.rows
            out.append(torch.randn(L, self.context_dim, generator=torch.Generator().manual_seed(self._key(prompt))))
            lens.append(1 + self._key(prompt) % L)
        ctx = torch.stack(out).to(self._anchor.device)
        return (ctx, torch.tensor(lens, dtype=torch.int32)) if return_lens else ctx
