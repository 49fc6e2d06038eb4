"""References for the edit tests (not a conftest, not collected): the numpy restatement of the re-masking
order with a count per image, of the two pixel-side operators and of the schedule, the inputs the operator tests share, and the
edit loop composed from already pinned operators."""
import math

import numpy as np
import torch

from paintmind_amd import ops
from paintmind_amd.generate import edit_schedule, loop_schedule

GIVEN = np.float32(-1e5)
MASK_ID = 8192


def schedule_np(m, T):
    """edit_schedule restated from the issue's formula"""
    out, c = [], m
    for s in range(T - 1):
        n = max(0, min(max(int(math.cos(math.pi / 2 * (s + 1) / T) * m), 1), c - 1))
        out.append(n)
        c = n
    return out + [0]


def scores_with_ties(B, N, seed):
    """scores 1 - p in [0, 1) drawn from 40 distinct values (so: many exact ties), every 7th position given (-1e5), image 2 given at
    EVERY position; ids below the mask id"""
    rng = np.random.default_rng(seed)
    levels = (1.0 - 10.0 ** rng.uniform(-6.0, 0.0, 40)).astype(np.float32)
    scores = levels[rng.integers(0, 40, (B, N))]
    scores[:, ::7] = GIVEN
    if B > 2:
        scores[2] = GIVEN
    ids = rng.integers(0, 50, (B, N)).astype(np.int64)
    return ids, scores


def remask_counts_np(ids, keys, counts, mask_id):
    """per image: order (key descending, index ascending), the first counts[b] positions get the mask id; 0 leaves the row"""
    out = ids.copy()
    for b, c in enumerate(counts):
        c = min(int(c), ids.shape[1])
        if c <= 0:
            continue
        order = np.argsort(-keys[b].astype(np.float64), kind="stable")     # stable: equal keys stay in index order
        out[b, order[:c]] = mask_id
    return out


def mask_tokens_np(pixel_mask, patch, ids, mask_id):
    B, H, W = pixel_mask.shape
    lit = pixel_mask.reshape(B, H // patch, patch, W // patch, patch).max(axis=(2, 4)) != 0
    lit = lit.reshape(B, -1)
    return np.where(lit, mask_id, ids), lit.sum(1).astype(np.int32)


def composite_np(gen, orig, pixel_mask):
    return np.where(pixel_mask[:, None] != 0, gen, orig)


def composed_edit(pipe, ids0, counts, context, T, temperature, opts, seed, image_base=0):
    """the edit loop from pinned operators: per step the native step's logits / draw / score (S2Engine.sample with want_aux: the
    operator chain of Pipeline.sample), the merge where(ids == mask, pred, ids), then ops.remask on every row ALONE with the
    table's count (none for a count of 0) and the noise of the image's own rows; the image is the decode of the last step's merged
    ids.  -> (final ids, image)"""
    eng = pipe.engine()
    B, N = ids0.shape
    temps, _, ctemps = loop_schedule(T, temperature, N, opts.choice_temperature)
    per_image = [edit_schedule(m, T) for m in counts]
    ids = ids0.to(eng.device, torch.int64).clone().contiguous()
    merged = ids
    for step in range(T):
        _, _, pred, score = eng.sample(None, ids.clone(), context, opts.topk, temps[step], 1, seed=seed, step=step, image_base=image_base,
                                       want_img=False, want_aux=True, guidance_scale=opts.step_scale(step), context_lens=opts.lens,
                                       top_p=opts.top_p, negative_context=opts.negative, negative_lens=opts.negative_lens)
        merged = torch.where(ids == pipe.mask_token_id, pred, ids)
        ids = merged.clone()
        for b in range(B):
            if per_image[b][step] > 0:
                row = ids[b:b + 1].clone()
                ops.remask(row, score[b:b + 1].clone(), per_image[b][step], pipe.mask_token_id,
                           choice_temperature=ctemps[step] if ctemps else 0.0, seed=seed, step=step, row_base=(image_base + b) * N)
                ids[b] = row[0]
    return ids, pipe.vqgan.decode_from_indice(merged)
