"""The step vocabulary of the eager decode flows: what ``Pipeline.control_ids``, ``forced_ids``, ``diff_mask``,
``token_scores`` and ``surprise_mask`` do per step, said once, with two implementations of one set of signatures -- ``TorchSteps`` for
a pipeline on the CPU (the plain-torch primitives ``Pipeline._*_cpu``, reached through the pipeline instance at call time) and
``HipSteps`` for a pipeline with an engine (``S2Engine`` and ``ops.*``).  ``Pipeline._steps`` picks one; a flow is written once
against either.  What differs between the two stays in here: the generator against Philox (``Draw.rng``), a bool region against a
uint8 one, a blend that returns against one in place, float accumulators against kernel-side ``accumulate=True``."""
import functools
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops


class Draw(NamedTuple):
    """what a token draw leaves before any re-masking: [B, N] each on the torch side, B * N elements on the HIP side"""
    pred: torch.Tensor
    merged: torch.Tensor
    score: torch.Tensor
    rng: Optional[torch.Generator]     # the generator the draw used, which the re-masking draws from next; None: no seed, or Philox


@functools.lru_cache(maxsize=8)
def _torch_tables(layout):
    """a ``canvas.CanvasLayout``'s tables as CPU tensors, built once per layout (it hashes by identity): cover int64 [Nc, K], weight
    f32 [Nc, K], and per pixel axis the dense f32 [windows, extent] weight of every window, 0 where it does not cover"""
    def dense(table, n):
        win, w = (torch.from_numpy(np.array(a)) for a in table)
        return torch.stack([(w * (win == j)).sum(1) for j in range(n)])
    return (torch.from_numpy(np.array(layout.cover)).long(), torch.from_numpy(np.array(layout.weight)),
            dense(layout.pixel_y, len(layout.offsets_y)), dense(layout.pixel_x, len(layout.offsets_x)))


class TorchSteps:
    """the steps of a pipeline that lives on the CPU"""

    def __init__(self, pipe):
        self.pipe, self.device = pipe, pipe.mask_token.device

    def ids(self, x):
        return x.to(self.device)

    def context(self, x):
        return None if x is None else x.to(self.device)

    def drawn_region(self, x):
        """a region that was drawn, bool [B, N], as ``blend`` takes it"""
        return x.to(self.device)

    def forward(self, tok, context, keys):
        return self.pipe.transformer(tok, context, keys=keys)   # plain-torch operators of this package (no HIP engine on the CPU)

    def forward_control(self, tok, context, keys, cross, inject, ctl, tap):
        """the forward over pairs under control and / or the phrase tap -> (logits, the accumulated scores or None)"""
        out = self.pipe.transformer(tok, context, keys=keys, control=dict(cross_layers=cross, self_layers=inject, **ctl, **tap))
        return out if tap else (out, None)

    def guide(self, cond, uncond, scale):
        return torch.addcmul(uncond, cond - uncond, torch.tensor(float(scale)))

    def draw(self, ids, logits, opts, temperature, noise, seed, step, image_base):
        return Draw(*self.pipe._draw_cpu(ids, logits, opts.topk, temperature, noise, None if seed is None else seed + step, opts.top_p))

    def forced(self, ids, logits, target, noise, seed, step):
        return Draw(*self.pipe._forced_cpu(ids, logits, target, noise, None if seed is None else seed + step))

    def region(self, score_src, score_edit, g, threshold, grow):
        return self.pipe._region_cpu(score_src, score_edit, g, threshold, grow)

    def blend(self, region, src, edit):
        """-> the edited half's draw, the source's where not region; it keeps its own generator"""
        return Draw(*self.pipe._blend_cpu(region, src[:3], edit[:3]), edit.rng)

    def remask(self, draw, nm, choice_t, seed, step, image_base):
        return self.pipe._remask_cpu(draw.merged, draw.score, nm, draw.rng, choice_t, None, [nm] * draw.merged.shape[0])

    def divergence_start(self, B, N):
        return torch.zeros(B, N), torch.zeros(B, N)

    def divergence_add(self, acc, logits, m, masked, kind):
        """one draw: the logits of 2 B images, the source contexts in front; m bool [B, N] is where `masked` holds the mask id"""
        B = m.shape[0]
        acc[0].add_(torch.where(m, self.pipe._divergence_cpu(logits[:B], logits[B:], kind), torch.zeros(m.shape)))
        acc[1].add_(m)

    def divergence_finish(self, acc):
        return acc[0] / acc[1]

    def logprob_start(self, ids):
        known = ids != self.pipe.mask_token_id                 # (a position that holds the mask id has no true id: never scored)
        return [torch.zeros(ids.shape) for _ in range(4)], known, torch.where(known, ids, torch.zeros_like(ids))

    def logprob_add(self, acc, logits, uncond, scale, m, masked):
        """one draw; with uncond the row that is scored is the guided one"""
        sums, known, target = acc
        if uncond is not None:
            logits = self.guide(logits, uncond, scale)
        for a, v in zip(sums, self.pipe._token_logprob_cpu(logits, target)):
            a += torch.where(m & known, v.float(), torch.zeros(m.shape))
        sums[3] += m & known

    def logprob_finish(self, acc):
        return tuple(a / acc[0][3] for a in acc[0][:3])

    # -- canvases beyond the token grid ---------------------------------------------------------------------
    def forward_chunks(self, tok, context, keys, chunk):
        """``forward`` over the windows of a canvas call, at most `chunk` windows at a time (None: all at once) -> one logits tensor"""
        n = tok.shape[0]
        if not chunk or chunk >= n:
            return self.forward(tok, context, keys)
        return torch.cat([self.forward(tok[lo:lo + chunk], None if context is None else context[lo:lo + chunk],
                                       None if keys is None else keys.lane(lo, min(n, lo + chunk))) for lo in range(0, n, chunk)])

    def window_logits(self, layout, cond, uncond, scale):
        """``ops.window_logits`` in plain torch, the same order of operations: the window logits [B * W, g^2, V] (with uncond and scale:
        guided at load) -> the canvas logits [B, Nc, V]; w_0 x_0, then + w_k x_k over the windows that cover a token, ascending"""
        x = cond if uncond is None else self.guide(cond, uncond, scale)
        x = x.reshape(-1, layout.window_rows, x.shape[-1])
        cover, weight = _torch_tables(layout)[:2]
        acc = weight[:, 0, None] * x[:, cover[:, 0]]
        for k in range(1, layout.K):
            on = cover[:, k] >= 0
            acc = torch.where(on[None, :, None], acc + weight[:, k, None] * x[:, cover[:, k].clamp(min=0)], acc)
        return acc

    def window_pixels(self, layout, imgs):
        """``ops.window_pixels`` in plain torch, the same order of operations: the decoded windows [B * W, C, S, S] -> [B, C, Hc, Wc]"""
        (Hc, Wc), S = layout.size, layout.g * layout.patch
        ny, nx = len(layout.offsets_y), len(layout.offsets_x)
        imgs = imgs.reshape(-1, ny, nx, imgs.shape[1], S, S)
        out = torch.zeros(imgs.shape[0], imgs.shape[3], Hc, Wc)
        seen = torch.zeros(Hc, Wc, dtype=torch.bool)
        wy, wx = _torch_tables(layout)[2:]
        for jy, oy in enumerate(layout.pixel_off_y.tolist()):
            for jx, ox in enumerate(layout.pixel_off_x.tolist()):
                w = wy[jy, oy:oy + S, None] * wx[jx, None, ox:ox + S]
                term, at = w * imgs[:, jy, jx], (slice(None), slice(None), slice(oy, oy + S), slice(ox, ox + S))
                out[at] = torch.where(seen[oy:oy + S, ox:ox + S], out[at] + term, term)
                seen[oy:oy + S, ox:ox + S] = True
        return out.clamp(-1.0, 1.0)

    def canvas_draw(self, ids, logits, opts, temperature, seed, step, image_base):
        """one draw over the canvases [B, Nc].  Every canvas draws from a generator of its own, seeded seed + step + 2^32 (image_base
        + j): canvas j of a batch is the call with image_base + j alone, and canvas 0 at image_base 0 draws what ``draw`` draws"""
        if seed is None:
            return self.draw(ids, logits, opts, temperature, None, None, step, image_base)
        parts = [self.pipe._draw_cpu(ids[j:j + 1], logits[j:j + 1], opts.topk, temperature, None, seed + step + ((image_base + j) << 32), opts.top_p)
                 for j in range(ids.shape[0])]
        return Draw(*(torch.cat([p[i] for p in parts]) for i in range(3)), [p[3] for p in parts])

    def canvas_remask(self, draw, shape, nm, counts, choice_t, seed, step, image_base):
        """one re-masking over the canvases, shape = (B, Nc): nm positions each, or counts[b] (a list of B ints) where given"""
        B = shape[0]
        counts = [nm] * B if counts is None else counts
        if not isinstance(draw.rng, list):
            return self.pipe._remask_cpu(draw.merged, draw.score, nm, draw.rng, choice_t, None, counts)
        return torch.cat([self.pipe._remask_cpu(draw.merged[j:j + 1], draw.score[j:j + 1], nm, draw.rng[j], choice_t, None, counts[j:j + 1])
                          for j in range(B)])


class HipSteps:
    """the steps of a pipeline with an engine: every method is the launch the flows' docstrings name"""

    def __init__(self, pipe):
        self.pipe, self.eng = pipe, pipe.engine()
        self.device = self.eng.device

    def ids(self, x):
        return x.to(self.device, torch.long).contiguous()

    def context(self, x):
        return None if x is None else x.to(self.device).contiguous()

    def drawn_region(self, x):
        """a region that was drawn, bool [B, N], as ``blend`` takes it"""
        return x.to(self.device, torch.uint8).contiguous()

    def forward(self, tok, context, keys):
        return self.eng.forward(tok, context, keys=keys)

    def forward_control(self, tok, context, keys, cross, inject, ctl, tap):
        """the forward over pairs under control and / or the phrase tap -> (logits, the accumulated scores or None)"""
        out = self.eng.forward_control(tok, context, cross_layers=cross, self_layers=inject, context_lens=keys.lens, **ctl, **tap)
        return out if tap else (out, None)

    def guide(self, cond, uncond, scale):
        return ops.guidance_combine(cond, uncond, scale, out=cond)

    def draw(self, ids, logits, opts, temperature, noise, seed, step, image_base):
        if noise is not None:                                  # (the caller's uniforms [B, N, n_embed], wherever they are)
            noise = noise.to(self.device, torch.float32).reshape(ids.numel(), -1).contiguous()
        return Draw(*ops.sample_rows(logits.reshape(ids.numel(), -1), ids.reshape(-1), self.pipe.mask_token_id, opts.topk, temperature, seed=seed,
                                     step=step, row_base=image_base * ids.shape[1], top_p=opts.top_p, noise=noise), None)

    def forced(self, ids, logits, target, noise, seed, step):
        return Draw(*ops.sample_rows_forced(logits.reshape(ids.numel(), -1), ids.reshape(-1), target.reshape(-1), self.pipe.mask_token_id), None)

    def region(self, score_src, score_edit, g, threshold, grow):
        return ops.phrase_region(score_src, score_edit, g, threshold, grow)

    def blend(self, region, src, edit):
        """-> the edited half's draw, the source's where not region; it keeps its own generator"""
        ops.blend_tokens(region, *src[:3], *edit[:3])
        return edit

    def remask(self, draw, nm, choice_t, seed, step, image_base):
        N = self.pipe.num_tokens
        return ops.remask(draw.merged.reshape(-1, N), draw.score.reshape(-1, N), nm, self.pipe.mask_token_id, choice_temperature=choice_t,
                          seed=seed, step=step, row_base=image_base * N)

    def divergence_start(self, B, N):
        return torch.zeros(B * N, device=self.device, dtype=torch.float32), torch.zeros(B * N, device=self.device, dtype=torch.int32)

    def divergence_add(self, acc, logits, m, masked, kind):
        """one draw: the logits of 2 B images, the source contexts in front; m bool [B, N] is where `masked` holds the mask id"""
        rows = masked.numel()
        logits = logits.reshape(2 * rows, -1)
        ops.logit_divergence(logits[:rows], logits[rows:], ids=masked.reshape(-1), mask_id=self.pipe.mask_token_id, kind=kind, out=acc,
                             accumulate=True)

    def divergence_finish(self, acc):
        return (acc[0] / acc[1]).reshape(-1, self.pipe.num_tokens)

    def logprob_start(self, ids):
        n = ids.numel()
        return (torch.zeros(n, device=self.device), torch.zeros(n, device=self.device), torch.zeros(n, device=self.device, dtype=torch.int32),
                torch.zeros(n, device=self.device, dtype=torch.int32)), ids

    def logprob_add(self, acc, logits, uncond, scale, m, masked):
        """one draw; with uncond the row that is scored is the guided one"""
        out, ids = acc
        n = ids.numel()
        ops.token_logprob(logits.reshape(n, -1), ids.reshape(-1), uncond=None if uncond is None else uncond.reshape(n, -1), scale=scale,
                          ids=masked.reshape(-1), mask_id=self.pipe.mask_token_id, out=out, accumulate=True)

    def logprob_finish(self, acc):
        count = acc[0][3].float()
        return tuple((a.float() / count).reshape(acc[1].shape) for a in acc[0][:3])

    # -- canvases beyond the token grid ---------------------------------------------------------------------
    def forward_chunks(self, tok, context, keys, chunk):
        """``forward`` over the windows of a canvas call, at most `chunk` windows at a time (None: all at once) into ONE logits buffer"""
        n = tok.shape[0]
        if not chunk or chunk >= n:
            return self.forward(tok, context, keys)
        out = torch.empty(n, self.eng.tokens, self.eng.n_embed, device=self.device, dtype=torch.float32)
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            self.eng.forward(tok[lo:hi], None if context is None else context[lo:hi], keys=None if keys is None else keys.lane(lo, hi),
                             out=out[lo:hi])
        return out

    def window_logits(self, layout, cond, uncond, scale):
        """the window logits [B * W, g^2, V] (with uncond and scale: guided at load, no combined window logits are written) -> the
        canvas logits [B * Nc, V]"""
        tables = ops.canvas_tables(layout, self.device)
        V = cond.shape[-1]
        return ops.window_logits(cond.reshape(-1, V), tables.cover, tables.weight, layout.window_rows,
                                 uncond=None if uncond is None else uncond.reshape(-1, V), scale=None if uncond is None else float(scale))

    def window_pixels(self, layout, imgs):
        return ops.window_pixels(imgs.contiguous(), ops.canvas_tables(layout, self.device))

    def canvas_draw(self, ids, logits, opts, temperature, seed, step, image_base):
        """one draw over the B * Nc rows of the canvases [B, Nc]: Philox under row_base = image_base * Nc"""
        return self.draw(ids, logits, opts, temperature, None, seed, step, image_base)

    def canvas_remask(self, draw, shape, nm, counts, choice_t, seed, step, image_base):
        """one re-masking over the canvases, shape = (B, Nc): nm positions each, or counts[b] (a list of B ints) where given"""
        B, N = shape
        merged, score = draw.merged.reshape(B, N), draw.score.reshape(B, N)
        if counts is None:
            return ops.remask(merged, score, nm, self.pipe.mask_token_id, choice_temperature=choice_t, seed=seed, step=step, row_base=image_base * N)
        return ops.remask_counts(merged, score, torch.tensor(counts, dtype=torch.int32, device=self.device), self.pipe.mask_token_id,
                                 choice_temperature=choice_t, seed=seed, step=step, row_base=image_base * N)
