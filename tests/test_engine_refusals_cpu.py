"""What the native decode entries refuse, and in which words: the sample, generate and slots families and
the eager forward validate their host arguments before the first HIP call, so every row of the table below runs without a device
(a stage-2 or VQGAN handle only keeps its weights; see the host_handle fixture of test_slots_filter_cpu.py).

A row is (entry, the arguments that differ from DEFAULTS, return code, the complete message).  The messages were recorded from the
library of the commit before the entries were rebuilt on call records, and the rows ran unchanged against it; the table pins

  * every refusal site a call can reach without a device, one fault per row,
  * the name a message carries: per entry with no wider feature present, and per arm of the rule "the widest feature present names
    the call" (pmhip_pipeline_generate and _guided have no reachable message that carries their name: their only `who`-less checks
    say pipeline_generate / pipeline_generate_guided),
  * the order of the checks: for neighbouring checks that one call can violate together, the first one's message,
  * and, behind the slots rows, that a refused step counted nothing and cached nothing.

The dummy pointer P is never dereferenced: a row that got past the checks would fail in the first HIP call, not fault.

Not reachable without a device, and so not here: "pipeline_sample: img_out requested without a vqgan handle" (behind the tower),
"... the shared step-0 logits are missing during a graph capture", the workspace and HIP errors, the two keep-refusals "the prepared
context / negative context has another B or L / Ln" (a slots call has to have prepared one), and the two slots checks behind the
preparation, "... but the kept context was prepared without one" (a kept context of length 0 is refused by the checks in front)."""
import ctypes as C
import re

import pytest

from paintmind_amd import _lib

P = C.c_void_p(256)
NAN, INF = float("nan"), float("inf")
GOOD = (1, 0, 1.0, 3, 4, 0)                   # seed, image_index, temperature, topk, num_mask, step
IDLE = None
TOKENS, N_EMBED = 16, 256
ALL = [0xFFFFFFFF] * TOKENS                   # a token mask row that allows every segment
EINVAL, ESTATE = _lib.PMHIP_EINVAL, _lib.PMHIP_ESTATE

DEFAULTS = dict(
    h="s2", s2="s2", vq=None, ids=P, tokens=P, logits_out=P, maps_out=P, context=None, L=0, B=2, stream=None,
    ctx_lens_host=None, ctx_seg_host=None, tok_seg_host=None, ctx_w_host=None, layer_bits=1,
    topk=4, temperature=1.0, num_mask=1, noise=None, seed=0, step=0, image_base=0, img_out=None, pred_out=None, score_out=None,
    guided=0, guidance_scale=0.0, choice_t=0.0, choice_noise=None, top_p=1.0, neg_context=None, Ln=0, neg_lens_host=None,
    T=2, temps_host=[1.0, 1.0], nmask_host=[1, 1], nmask_img_host=[1, 1, 1, 1], decode_host=None, imgs_out=None, use_graph=0,
    imgs_host=None, host_stride=0, copy_stream=None, ctemps_host=None, gscales_host=None,
    slots_host=[GOOD, GOOD], guides_host=None, choice_host=None, flags=0, top_p_host=None, counts_host=None, region_host=None,
)

def A(*parts, **more):
    """the arguments of a row: shared parts first, what the row sets itself last"""
    out = {}
    for part in parts:
        out.update(part)
    out.update(more)
    return out


S, G, SL, F = "pmhip_pipeline_sample", "pmhip_pipeline_generate", "pmhip_pipeline_step_slots", "pmhip_s2_forward"
CTX = A(context=P, L=4)                    # a context of four rows
SEG = A(ctx_seg_host=[0, 0, 1, 255] * 2, tok_seg_host=ALL * 2)
W1 = [1.0, 1.0, 1.0, 1.0] * 2
NEG = A(CTX, guided=1, neg_context=P, Ln=2)
REG = A(CTX, SEG, region_host=[1, 1])
KEEP_CTX, KEEP_NEG, FROM_MASK = _lib.SLOTS_KEEP_CONTEXT, _lib.SLOTS_KEEP_NEGATIVE, _lib.GENERATE_FROM_MASK
T129 = A(T=129, temps_host=[1.0] * 129, nmask_host=[1] * 129)

ROWS = [
    # ---- the eager forward: every site, one fault per row
    (F, A(tokens=None), EINVAL, "s2_forward: bad arguments"),
    (F, A(B=0), EINVAL, "s2_forward: bad arguments"),
    (F, A(context=P, L=0), EINVAL, "s2: context given with L=0"),
    (F + "_lens", A(ctx_lens_host=[1, 1]), EINVAL, "s2_forward_lens: ctx_lens_host given without a context"),
    (F + "_lens", A(CTX, ctx_lens_host=[4, 5]), EINVAL, "s2_forward_lens: image 1: context length 5 must be in [1, L=4]"),
    (F + "_lens", A(CTX, ctx_lens_host=[0, 4]), EINVAL, "s2_forward_lens: image 0: context length 0 must be in [1, L=4]"),
    (F + "_segments", A(CTX, ctx_seg_host=SEG["ctx_seg_host"]), EINVAL, "s2_forward_segments: ctx_seg_host and tok_seg_host come together (one of them is NULL)"),
    (F + "_segments", A(SEG, L=4), EINVAL, "s2_forward_segments: segments given without a context"),
    (F + "_segments", A(CTX, SEG, ctx_seg_host=[0, 0, 1, 255, 0, 32, 1, 255]), EINVAL, "s2_forward_segments: image 1: context row 1: segment 32 must be in 0..31, or 255 for padding"),
    (F + "_segments", A(CTX, SEG, tok_seg_host=ALL + [1] * 15 + [4]), EINVAL, "s2_forward_segments: image 1: token 15 allows no segment that is present in its context (mask 0x00000004, present 0x00000003)"),
    (F + "_weights", A(ctx_w_host=W1, L=4), EINVAL, "s2_forward_weights: weights given without a context"),
    (F + "_weights", A(CTX, ctx_w_host=[1.0, 1.0, 1.0, 1.0, 1.0, 1e-7, 1.0, 1.0]), EINVAL, "s2_forward_weights: image 1: context row 1: weight 1e-07 must be 0 or in [2^-20, 2^20]"),
    (F + "_weights", A(CTX, ctx_w_host=[1.0, 1.0, 1.0, 1.0, 1.0, NAN, 1.0, 1.0]), EINVAL, "s2_forward_weights: image 1: context row 1: weight nan must be 0 or in [2^-20, 2^20]"),
    (F + "_weights", A(CTX, SEG, ctx_w_host=[1.0, 1.0, 0.0, 1.0] * 2, tok_seg_host=ALL + [3] * 15 + [2]), EINVAL, "s2_forward_weights: image 1: token 15 allows no context row with a weight above 0 (mask 0x00000002, segments with such a row 0x00000001)"),
    (F + "_weights", A(CTX, ctx_w_host=[1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0]), EINVAL, "s2_forward_weights: image 1: token 0 allows no context row with a weight above 0 (mask 0xffffffff, segments with such a row 0x00000000)"),
    (F + "_maps", A(CTX, maps_out=None), EINVAL, "s2_forward_maps: maps_out is NULL (pmhip_s2_forward_weights is the entry without maps)"),
    (F + "_maps", A(), EINVAL, "s2_forward_maps: the maps are those of the cross-attention: a context is required"),
    (F + "_maps", A(CTX, layer_bits=0), EINVAL, "s2_forward_maps: layer_bits selects no layer"),
    (F + "_maps", A(CTX, layer_bits=2), EINVAL, "s2_forward_maps: layer_bits 0x2 selects a layer at or above depth=1"),
    (F + "_maps", A(CTX, SEG, ctx_lens_host=[4, 4]), EINVAL, "s2_forward_maps: segments and ctx_lens_host exclude each other (mark padding rows with segment 255)"),
    # the name: per entry, and per arm of the rule (the maps entry keeps its own whatever came)
    (F + "_lens", A(tokens=None), EINVAL, "s2_forward_lens: bad arguments"),
    (F + "_segments", A(tokens=None), EINVAL, "s2_forward: bad arguments"),
    (F + "_weights", A(tokens=None), EINVAL, "s2_forward: bad arguments"),
    (F + "_maps", A(tokens=None), EINVAL, "s2_forward_maps: bad arguments"),
    (F + "_segments", A(SEG, tokens=None), EINVAL, "s2_forward_segments: bad arguments"),
    (F + "_segments", A(tok_seg_host=ALL * 2, tokens=None), EINVAL, "s2_forward_segments: bad arguments"),
    (F + "_weights", A(SEG, tokens=None), EINVAL, "s2_forward_segments: bad arguments"),
    (F + "_weights", A(SEG, ctx_w_host=W1, tokens=None), EINVAL, "s2_forward_weights: bad arguments"),
    (F + "_maps", A(SEG, ctx_w_host=W1, tokens=None), EINVAL, "s2_forward_maps: bad arguments"),
    # the order: two faults, the first check's message
    (F + "_maps", A(tokens=None, layer_bits=0), EINVAL, "s2_forward_maps: bad arguments"),
    (F + "_maps", A(layer_bits=0), EINVAL, "s2_forward_maps: the maps are those of the cross-attention: a context is required"),
    (F + "_maps", A(CTX, layer_bits=2, ctx_lens_host=[4, 5]), EINVAL, "s2_forward_maps: layer_bits 0x2 selects a layer at or above depth=1"),
    (F + "_lens", A(tokens=None, ctx_lens_host=[1, 1]), EINVAL, "s2_forward_lens: bad arguments"),
    (F + "_maps", A(CTX, ctx_lens_host=[4, 5], ctx_seg_host=SEG["ctx_seg_host"]), EINVAL, "s2_forward_maps: image 1: context length 5 must be in [1, L=4]"),
    (F + "_maps", A(CTX, SEG, ctx_lens_host=[4, 4], ctx_seg_host=[40, 0, 1, 255] * 2), EINVAL, "s2_forward_maps: segments and ctx_lens_host exclude each other (mark padding rows with segment 255)"),
    (F + "_segments", A(CTX, ctx_seg_host=[40, 0, 1, 255] * 2, tok_seg_host=[0] * 32), EINVAL, "s2_forward_segments: image 0: context row 0: segment 40 must be in 0..31, or 255 for padding"),
    (F + "_weights", A(CTX, SEG, tok_seg_host=[4] * 32, ctx_w_host=[INF] * 8), EINVAL, "s2_forward_weights: image 0: token 0 allows no segment that is present in its context (mask 0x00000004, present 0x00000003)"),
    (F + "_weights", A(CTX, ctx_w_host=[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0]), EINVAL, "s2_forward_weights: image 1: context row 3: weight -1 must be 0 or in [2^-20, 2^20]"),

    # ---- the sample family: every site
    (S + "_nucleus", A(top_p=0.0), EINVAL, "pipeline_sample_nucleus: top_p=0 must be finite and in (0, 1]"),
    (S + "_nucleus", A(top_p=NAN), EINVAL, "pipeline_sample_nucleus: top_p=nan must be finite and in (0, 1]"),
    (S + "_choice", A(choice_t=-1.0), EINVAL, "pipeline_sample_choice: the choice temperature -1 must be finite and in [0, 1000]"),
    (S + "_nucleus", A(choice_t=1001.0, top_p=0.5), EINVAL, "pipeline_sample_nucleus: the choice temperature 1001 must be finite and in [0, 1000]"),
    (S + "_negative", A(neg_lens_host=[1, 1]), EINVAL, "pipeline_sample_negative: neg_lens_host given without a negative context"),
    (S + "_negative", A(CTX, neg_context=P, Ln=2), EINVAL, "pipeline_sample_negative: a negative context or a guidance schedule needs guidance (guided != 0) and a context"),
    (S + "_negative", A(guided=1, neg_context=P, Ln=2), EINVAL, "pipeline_sample_negative: a negative context or a guidance schedule needs guidance (guided != 0) and a context"),
    (S + "_negative", A(NEG, Ln=0), EINVAL, "pipeline_sample_negative: negative context given with Ln=0"),
    (S + "_negative", A(NEG, neg_lens_host=[2, 3]), EINVAL, "pipeline_sample_negative: image 1: negative context length 3 must be in [1, Ln=2]"),
    (S, A(s2=None), EINVAL, "pipeline_sample: bad arguments"),
    (S, A(B=0), EINVAL, "pipeline_sample: bad arguments"),
    (S + "_guided", A(guidance_scale=2.0), EINVAL, "pipeline_sample_guided: guidance needs a context (context NULL IS the unconditional branch)"),
    (S + "_lens", A(CTX, L=0, context=None, guided=1), EINVAL, "pipeline_sample_lens: guidance needs a context (context NULL IS the unconditional branch)"),
    (S + "_lens", A(ctx_lens_host=[1, 1]), EINVAL, "pipeline_sample_lens: ctx_lens_host given without a context"),
    (S + "_lens", A(CTX, ctx_lens_host=[5, 1]), EINVAL, "pipeline_sample_lens: image 0: context length 5 must be in [1, L=4]"),
    (S + "_segments", A(CTX, tok_seg_host=ALL * 2), EINVAL, "pipeline_sample_segments: ctx_seg_host and tok_seg_host come together (one of them is NULL)"),
    (S + "_segments", A(SEG), EINVAL, "pipeline_sample_segments: segments given without a context"),
    (S + "_segments", A(CTX, SEG, ctx_lens_host=[4, 4]), EINVAL, "pipeline_sample_segments: segments and ctx_lens_host exclude each other (mark padding rows with segment 255)"),
    (S + "_segments", A(CTX, SEG, ctx_seg_host=[254, 0, 1, 255] * 2), EINVAL, "pipeline_sample_segments: image 0: context row 0: segment 254 must be in 0..31, or 255 for padding"),
    (S + "_segments", A(CTX, SEG, tok_seg_host=[8] + [1] * 31), EINVAL, "pipeline_sample_segments: image 0: token 0 allows no segment that is present in its context (mask 0x00000008, present 0x00000003)"),
    (S + "_weights", A(ctx_w_host=W1), EINVAL, "pipeline_sample_weights: weights given without a context"),
    (S + "_weights", A(CTX, ctx_w_host=[2.0 ** 21] + [1.0] * 7), EINVAL, "pipeline_sample_weights: image 0: context row 0: weight 2.09715e+06 must be 0 or in [2^-20, 2^20]"),
    (S + "_weights", A(CTX, ctx_lens_host=[4, 2], ctx_w_host=[1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0]), EINVAL, "pipeline_sample_weights: image 1: token 0 allows no context row with a weight above 0 (mask 0xffffffff, segments with such a row 0x00000000)"),
    (S, A(context=P, L=0), EINVAL, "s2: context given with L=0"),
    # the name: per entry, then per arm
    (S, A(ids=None), EINVAL, "pipeline_sample: bad arguments"),
    (S + "_guided", A(ids=None), EINVAL, "pipeline_sample_guided: bad arguments"),
    (S + "_lens", A(ids=None), EINVAL, "pipeline_sample_lens: bad arguments"),
    (S + "_choice", A(ids=None), EINVAL, "pipeline_sample_lens: bad arguments"),
    (S + "_nucleus", A(ids=None), EINVAL, "pipeline_sample_lens: bad arguments"),
    (S + "_negative", A(ids=None), EINVAL, "pipeline_sample_lens: bad arguments"),
    (S + "_segments", A(ids=None), EINVAL, "pipeline_sample_lens: bad arguments"),
    (S + "_weights", A(ids=None), EINVAL, "pipeline_sample_lens: bad arguments"),
    (S + "_choice", A(ids=None, choice_t=1.0), EINVAL, "pipeline_sample_choice: bad arguments"),
    (S + "_nucleus", A(ids=None, choice_t=1.0), EINVAL, "pipeline_sample_choice: bad arguments"),
    (S + "_nucleus", A(ids=None, top_p=0.5), EINVAL, "pipeline_sample_nucleus: bad arguments"),
    (S + "_nucleus", A(ids=None, top_p=0.5, choice_t=1.0), EINVAL, "pipeline_sample_nucleus: bad arguments"),
    (S + "_negative", A(NEG, ids=None, top_p=0.5), EINVAL, "pipeline_sample_negative: bad arguments"),
    (S + "_segments", A(NEG, ids=None, ctx_seg_host=SEG["ctx_seg_host"]), EINVAL, "pipeline_sample_segments: bad arguments"),
    (S + "_segments", A(ids=None, tok_seg_host=ALL * 2), EINVAL, "pipeline_sample_segments: bad arguments"),
    (S + "_weights", A(NEG, SEG, ids=None, ctx_w_host=W1), EINVAL, "pipeline_sample_weights: bad arguments"),
    (S + "_weights", A(SEG, ids=None), EINVAL, "pipeline_sample_segments: bad arguments"),
    # the order
    (S + "_nucleus", A(top_p=2.0, choice_t=-1.0), EINVAL, "pipeline_sample_nucleus: top_p=2 must be finite and in (0, 1]"),
    (S + "_negative", A(choice_t=-1.0, neg_lens_host=[1, 1]), EINVAL, "pipeline_sample_choice: the choice temperature -1 must be finite and in [0, 1000]"),
    (S + "_negative", A(CTX, neg_context=P, Ln=0), EINVAL, "pipeline_sample_negative: a negative context or a guidance schedule needs guidance (guided != 0) and a context"),
    (S + "_negative", A(NEG, Ln=0, neg_lens_host=[1, 1]), EINVAL, "pipeline_sample_negative: negative context given with Ln=0"),
    (S + "_negative", A(NEG, neg_lens_host=[0, 1], ids=None), EINVAL, "pipeline_sample_negative: image 0: negative context length 0 must be in [1, Ln=2]"),
    (S + "_lens", A(ids=None, guided=1), EINVAL, "pipeline_sample_lens: bad arguments"),
    (S + "_lens", A(guided=1, ctx_lens_host=[1, 1]), EINVAL, "pipeline_sample_lens: guidance needs a context (context NULL IS the unconditional branch)"),
    (S + "_segments", A(CTX, ctx_lens_host=[9, 1], ctx_seg_host=SEG["ctx_seg_host"]), EINVAL, "pipeline_sample_segments: image 0: context length 9 must be in [1, L=4]"),
    (S + "_segments", A(CTX, SEG, ctx_lens_host=[4, 4], ctx_seg_host=[40, 0, 1, 255] * 2), EINVAL, "pipeline_sample_segments: segments and ctx_lens_host exclude each other (mark padding rows with segment 255)"),
    (S + "_segments", A(CTX, ctx_seg_host=[40, 0, 1, 255] * 2, tok_seg_host=[0] * 32), EINVAL, "pipeline_sample_segments: image 0: context row 0: segment 40 must be in 0..31, or 255 for padding"),
    (S + "_weights", A(CTX, SEG, tok_seg_host=[4] * 32, ctx_w_host=[INF] * 8), EINVAL, "pipeline_sample_weights: image 0: token 0 allows no segment that is present in its context (mask 0x00000004, present 0x00000003)"),
    (S + "_weights", A(CTX, ctx_w_host=[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0]), EINVAL, "pipeline_sample_weights: image 1: context row 3: weight -1 must be 0 or in [2^-20, 2^20]"),

    # ---- the generate family: every site
    (G + "_nucleus", A(top_p=1.5), EINVAL, "pipeline_generate_nucleus: top_p=1.5 must be finite and in (0, 1]"),
    (G + "_negative", A(neg_lens_host=[1, 1]), EINVAL, "pipeline_generate_negative: neg_lens_host given without a negative context"),
    (G + "_negative", A(CTX, neg_context=P, Ln=2), EINVAL, "pipeline_generate_negative: a negative context or a guidance schedule needs guidance (guided != 0) and a context"),
    (G + "_negative", A(CTX, gscales_host=[1.0, 1.0]), EINVAL, "pipeline_generate_negative: a negative context or a guidance schedule needs guidance (guided != 0) and a context"),
    (G + "_negative", A(guided=1, gscales_host=[1.0, 1.0]), EINVAL, "pipeline_generate_negative: a negative context or a guidance schedule needs guidance (guided != 0) and a context"),
    (G + "_negative", A(NEG, Ln=-1), EINVAL, "pipeline_generate_negative: negative context given with Ln=-1"),
    (G + "_negative", A(NEG, neg_lens_host=[1, 0]), EINVAL, "pipeline_generate_negative: image 1: negative context length 0 must be in [1, Ln=2]"),
    (G + "_negative", A(CTX, T129, guided=1, gscales_host=[1.0] * 129), EINVAL, "pipeline_generate_negative: a guidance schedule serves at most 128 steps, T=129"),
    (G + "_negative", A(CTX, guided=1, gscales_host=[1.0, INF]), EINVAL, "pipeline_generate_negative: step 1: the guidance scale must be finite"),
    (G + "_edit", A(CTX, guided=1, neg_context=P, Ln=0), EINVAL, "pipeline_generate_edit: negative context given with Ln=0"),
    (G + "_edit", A(CTX, guided=1, gscales_host=[NAN, 1.0]), EINVAL, "pipeline_generate_edit: step 0: the guidance scale must be finite"),
    (G, A(ids=None), EINVAL, "pipeline_generate: bad arguments"),
    (G, A(T=0), EINVAL, "pipeline_generate: bad arguments"),
    (G, A(nmask_host=None), EINVAL, "pipeline_generate: bad arguments"),
    (G + "_edit", A(nmask_img_host=None), EINVAL, "pipeline_generate_edit: null count table"),
    (G + "_edit", A(use_graph=FROM_MASK), EINVAL, "pipeline_generate_edit: an edit starts from the caller's ids, the from-mask flag is refused"),
    (G + "_edit", A(nmask_img_host=[1, 1, 17, 1]), EINVAL, "pipeline_generate_edit: step 1, image 0: the re-masking count 17 must be in [0, 16]"),
    (G + "_edit", A(nmask_img_host=[1, -1, 1, 1]), EINVAL, "pipeline_generate_edit: step 0, image 1: the re-masking count -1 must be in [0, 16]"),
    (G + "_guided", A(guidance_scale=2.0), EINVAL, "pipeline_generate_guided: guidance needs a context (context NULL IS the unconditional branch)"),
    (G + "_lens", A(guided=1, L=4), EINVAL, "pipeline_generate_guided: guidance needs a context (context NULL IS the unconditional branch)"),
    (G + "_lens", A(ctx_lens_host=[1, 1]), EINVAL, "pipeline_generate_lens: ctx_lens_host given without a context"),
    (G + "_lens", A(CTX, ctx_lens_host=[1, 5]), EINVAL, "pipeline_generate_lens: image 1: context length 5 must be in [1, L=4]"),
    (G + "_segments", A(CTX, ctx_seg_host=SEG["ctx_seg_host"]), EINVAL, "pipeline_generate_segments: ctx_seg_host and tok_seg_host come together (one of them is NULL)"),
    (G + "_segments", A(SEG), EINVAL, "pipeline_generate_segments: segments given without a context"),
    (G + "_segments", A(CTX, SEG, ctx_lens_host=[4, 4]), EINVAL, "pipeline_generate_segments: segments and ctx_lens_host exclude each other (mark padding rows with segment 255)"),
    (G + "_segments", A(CTX, SEG, ctx_seg_host=[0, 0, 1, 255, 0, 0, 1, 33]), EINVAL, "pipeline_generate_segments: image 1: context row 3: segment 33 must be in 0..31, or 255 for padding"),
    (G + "_segments", A(CTX, SEG, tok_seg_host=ALL + [1] * 15 + [0]), EINVAL, "pipeline_generate_segments: image 1: token 15 allows no segment that is present in its context (mask 0x00000000, present 0x00000003)"),
    (G + "_weights", A(ctx_w_host=W1), EINVAL, "pipeline_generate_weights: weights given without a context"),
    (G + "_weights", A(CTX, ctx_w_host=[1.0] * 7 + [-1.0]), EINVAL, "pipeline_generate_weights: image 1: context row 3: weight -1 must be 0 or in [2^-20, 2^20]"),
    (G + "_weights", A(CTX, SEG, ctx_w_host=[0.0, 0.0, 1.0, 1.0] * 2, tok_seg_host=[1] * 32), EINVAL, "pipeline_generate_weights: image 0: token 0 allows no context row with a weight above 0 (mask 0x00000001, segments with such a row 0x00000002)"),
    (G + "_choice", A(ctemps_host=[1.0, 1000.5]), EINVAL, "pipeline_generate_choice: the choice temperature 1000.5 must be finite and in [0, 1000]"),
    (G, A(context=P, L=-3), EINVAL, "s2: context given with L=-3"),
    (G, A(decode_host=[0, 1]), EINVAL, "pipeline_generate: decode requested without vqgan / an image destination"),
    (G, A(vq="vq", decode_host=[0, 1]), EINVAL, "pipeline_generate: decode requested without vqgan / an image destination"),
    (G, A(vq="vq", imgs_host=P, host_stride=2047), EINVAL, "pipeline_generate: host_stride smaller than one image batch"),
    # the name: per entry with lengths, then per arm
    (G + "_lens", A(ctx_lens_host=[1, 1]), EINVAL, "pipeline_generate_lens: ctx_lens_host given without a context"),
    (G + "_choice", A(ctx_lens_host=[1, 1]), EINVAL, "pipeline_generate_lens: ctx_lens_host given without a context"),
    (G + "_nucleus", A(ctx_lens_host=[1, 1]), EINVAL, "pipeline_generate_lens: ctx_lens_host given without a context"),
    (G + "_negative", A(ctx_lens_host=[1, 1]), EINVAL, "pipeline_generate_lens: ctx_lens_host given without a context"),
    (G + "_segments", A(ctx_lens_host=[1, 1]), EINVAL, "pipeline_generate_lens: ctx_lens_host given without a context"),
    (G + "_weights", A(ctx_lens_host=[1, 1]), EINVAL, "pipeline_generate_lens: ctx_lens_host given without a context"),
    (G + "_edit", A(ctx_lens_host=[1, 1]), EINVAL, "pipeline_generate_edit: ctx_lens_host given without a context"),
    (G + "_choice", A(ctx_lens_host=[1, 1], ctemps_host=[0.0, 0.0]), EINVAL, "pipeline_generate_choice: ctx_lens_host given without a context"),
    (G + "_nucleus", A(ctx_lens_host=[1, 1], ctemps_host=[0.0, 0.0], top_p=0.5), EINVAL, "pipeline_generate_nucleus: ctx_lens_host given without a context"),
    (G + "_negative", A(NEG, ctx_lens_host=[0, 1], top_p=0.5), EINVAL, "pipeline_generate_negative: image 0: context length 0 must be in [1, L=4]"),
    (G + "_negative", A(CTX, guided=1, gscales_host=[1.0, 1.0], ctx_lens_host=[0, 1]), EINVAL, "pipeline_generate_negative: image 0: context length 0 must be in [1, L=4]"),
    (G + "_edit", A(NEG, ctx_lens_host=[0, 1], top_p=0.5), EINVAL, "pipeline_generate_edit: image 0: context length 0 must be in [1, L=4]"),
    (G + "_segments", A(NEG, ctx_lens_host=[0, 1], tok_seg_host=ALL * 2), EINVAL, "pipeline_generate_segments: image 0: context length 0 must be in [1, L=4]"),
    (G + "_weights", A(NEG, SEG, ctx_lens_host=[0, 1]), EINVAL, "pipeline_generate_segments: image 0: context length 0 must be in [1, L=4]"),
    (G + "_weights", A(NEG, SEG, ctx_lens_host=[0, 1], ctx_w_host=W1), EINVAL, "pipeline_generate_weights: image 0: context length 0 must be in [1, L=4]"),
    # the order
    (G + "_negative", A(top_p=0.0, neg_lens_host=[1, 1]), EINVAL, "pipeline_generate_nucleus: top_p=0 must be finite and in (0, 1]"),
    (G + "_negative", A(neg_lens_host=[1, 1], gscales_host=[1.0, 1.0]), EINVAL, "pipeline_generate_negative: neg_lens_host given without a negative context"),
    (G + "_negative", A(CTX, neg_context=P, Ln=0), EINVAL, "pipeline_generate_negative: a negative context or a guidance schedule needs guidance (guided != 0) and a context"),
    (G + "_negative", A(NEG, Ln=0, neg_lens_host=[1, 1]), EINVAL, "pipeline_generate_negative: negative context given with Ln=0"),
    (G + "_negative", A(NEG, T129, neg_lens_host=[3, 1], gscales_host=[1.0] * 129), EINVAL, "pipeline_generate_negative: image 0: negative context length 3 must be in [1, Ln=2]"),
    (G + "_negative", A(CTX, T129, guided=1, gscales_host=[NAN] * 129), EINVAL, "pipeline_generate_negative: a guidance schedule serves at most 128 steps, T=129"),
    (G + "_negative", A(CTX, guided=1, gscales_host=[1.0, NAN], ids=None), EINVAL, "pipeline_generate_negative: step 1: the guidance scale must be finite"),
    (G + "_edit", A(ids=None, use_graph=FROM_MASK), EINVAL, "pipeline_generate: bad arguments"),
    (G + "_edit", A(use_graph=FROM_MASK, nmask_img_host=[99, 1, 1, 1]), EINVAL, "pipeline_generate_edit: an edit starts from the caller's ids, the from-mask flag is refused"),
    (G + "_edit", A(nmask_img_host=[99, 1, 1, 1], guided=1), EINVAL, "pipeline_generate_edit: step 0, image 0: the re-masking count 99 must be in [0, 16]"),
    (G + "_lens", A(guided=1, ctx_lens_host=[1, 1]), EINVAL, "pipeline_generate_guided: guidance needs a context (context NULL IS the unconditional branch)"),
    (G + "_segments", A(CTX, ctx_lens_host=[9, 1], ctx_seg_host=SEG["ctx_seg_host"]), EINVAL, "pipeline_generate_segments: image 0: context length 9 must be in [1, L=4]"),
    (G + "_segments", A(CTX, SEG, ctx_lens_host=[4, 4], ctx_seg_host=[40, 0, 1, 255] * 2), EINVAL, "pipeline_generate_segments: segments and ctx_lens_host exclude each other (mark padding rows with segment 255)"),
    (G + "_segments", A(CTX, ctx_seg_host=[40, 0, 1, 255] * 2, tok_seg_host=[0] * 32), EINVAL, "pipeline_generate_segments: image 0: context row 0: segment 40 must be in 0..31, or 255 for padding"),
    (G + "_weights", A(CTX, SEG, tok_seg_host=[4] * 32, ctx_w_host=[INF] * 8), EINVAL, "pipeline_generate_weights: image 0: token 0 allows no segment that is present in its context (mask 0x00000004, present 0x00000003)"),
    (G + "_weights", A(CTX, ctx_w_host=[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0]), EINVAL, "pipeline_generate_weights: image 1: context row 3: weight -1 must be 0 or in [2^-20, 2^20]"),
    (G + "_weights", A(CTX, ctx_w_host=[0.0] * 8, ctemps_host=[-1.0, 0.0]), EINVAL, "pipeline_generate_weights: image 0: token 0 allows no context row with a weight above 0 (mask 0xffffffff, segments with such a row 0x00000000)"),
    (G + "_choice", A(context=P, L=0, ctemps_host=[-1.0, 0.0]), EINVAL, "pipeline_generate_choice: the choice temperature -1 must be finite and in [0, 1000]"),
    (G, A(context=P, L=0, decode_host=[1, 1]), EINVAL, "s2: context given with L=0"),

    # ---- the slots family: every site
    (SL, A(ids=None), EINVAL, "pipeline_step_slots: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL, A(slots_host=None), EINVAL, "pipeline_step_slots: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL, A(B=-1), EINVAL, "pipeline_step_slots: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_regions", A(CTX, SEG, region_host=None), EINVAL, "pipeline_step_slots_regions: ctx_seg_host, tok_seg_host and region_host come together (one of them is NULL)"),
    (SL + "_regions", A(REG, tok_seg_host=None), EINVAL, "pipeline_step_slots_regions: ctx_seg_host, tok_seg_host and region_host come together (one of them is NULL)"),
    (SL + "_regions", A(REG, region_host=[1, 2]), EINVAL, "pipeline_step_slots_regions: slot 1: region_host=2 must be 0 or 1 (2 needs ctx_w_host)"),
    (SL + "_weights", A(REG, ctx_w_host=W1, region_host=[3, 0]), EINVAL, "pipeline_step_slots_weights: slot 0: region_host=3 must be 0, 1 or 2"),
    (SL + "_weights", A(CTX, ctx_w_host=W1), EINVAL, "pipeline_step_slots_weights: ctx_w_host given without ctx_seg_host, tok_seg_host and region_host"),
    (SL + "_lens", A(ctx_lens_host=[1, 1]), EINVAL, "pipeline_step_slots_lens: ctx_lens_host given without a context"),
    (SL + "_lens", A(CTX, ctx_lens_host=[1, 7]), EINVAL, "pipeline_step_slots_lens: image 1: context length 7 must be in [1, L=4]"),
    (SL + "_regions", A(REG, context=None), EINVAL, "pipeline_step_slots_regions: regional slots given without a context"),
    (SL + "_regions", A(REG, ctx_seg_host=[0, 0, 1, 255, 0, 100, 1, 255]), EINVAL, "pipeline_step_slots_regions: slot 1: context row 1: segment 100 must be in 0..31, or 255 for padding"),
    (SL + "_regions", A(REG, tok_seg_host=[4] + [1] * 31), EINVAL, "pipeline_step_slots_regions: slot 0: token 0 allows no segment that is present in its context (mask 0x00000004, present 0x00000003)"),
    (SL + "_weights", A(REG, region_host=[1, 2], ctx_w_host=[1.0] * 6 + [3e-7, 1.0]), EINVAL, "pipeline_step_slots_weights: slot 1: context row 2: weight 3e-07 must be 0 or in [2^-20, 2^20]"),
    (SL + "_weights", A(REG, region_host=[2, 1], ctx_w_host=[0.0, 0.0, 1.0, 1.0] * 2, tok_seg_host=[1] * 32), EINVAL, "pipeline_step_slots_weights: slot 0: token 0 allows no context row with a weight above 0 (mask 0x00000001, segments with such a row 0x00000002)"),
    (SL + "_regions", A(REG, region_host=[1, 0], ctx_lens_host=[4, 0]), EINVAL, "pipeline_step_slots_regions: image 1: context length 0 must be in [1, L=4]"),
    (SL, A(s2="s2 n_embed=100"), EINVAL, "pipeline_step_slots: n_embed=100 must be a multiple of 64"),
    (SL + "_negative", A(neg_lens_host=[1, 1]), EINVAL, "pipeline_step_slots_negative: neg_lens_host given without a negative context"),
    (SL + "_negative", A(neg_context=P, Ln=0), EINVAL, "pipeline_step_slots_negative: negative context given with Ln=0"),
    (SL + "_negative", A(flags=KEEP_NEG, Ln=0), EINVAL, "pipeline_step_slots_negative: negative context given with Ln=0"),
    (SL + "_negative", A(neg_context=P, Ln=2, neg_lens_host=[2, 3]), EINVAL, "pipeline_step_slots_negative: slot 1: negative context length 3 must be in [1, Ln=2]"),
    (SL + "_choice", A(choice_host=[1.0, INF]), EINVAL, "pipeline_step_slots_choice: the choice temperature inf must be finite and in [0, 1000]"),
    (SL + "_filter", A(slots_host=[GOOD, (1, 0, 1.0, 257, 4, 0)]), EINVAL, "pipeline_step_slots_filter: slot 1: topk=257 must be in [1, n_embed=256]"),
    (SL + "_filter", A(top_p_host=[1.0, 0.0]), EINVAL, "pipeline_step_slots_filter: slot 1: top_p=0 must be finite and in (0, 1]"),
    (SL, A(slots_host=[GOOD, (1, 0, 1.0, 9, 4, 0)]), EINVAL, "pipeline_step_slots: slot 1: topk=9 must be in [1, 8]"),
    (SL + "_negative", A(slots_host=[(1, 0, 1.0, 0, 4, 0), GOOD]), EINVAL, "pipeline_step_slots_lens: slot 0: topk=0 must be in [1, 8]"),
    (SL + "_edit", A(counts_host=[-1, 17]), EINVAL, "pipeline_step_slots_edit: slot 1: count 17 must be in [-1, tokens=16]"),
    (SL + "_edit", A(counts_host=[-2, 1]), EINVAL, "pipeline_step_slots_edit: slot 0: count -2 must be in [-1, tokens=16]"),
    (SL, A(slots_host=[GOOD, (1, 0, 1.0, 3, 0, 0)]), EINVAL, "pipeline_step_slots: slot 1: num_mask=0 must be >= 1"),
    (SL + "_edit", A(slots_host=[GOOD, (1, 0, 1.0, 3, 0, 0)], counts_host=[0, -1]), EINVAL, "pipeline_step_slots_edit: slot 1: num_mask=0 must be >= 1"),
    (SL + "_negative", A(CTX, guides_host=[(1.0, 0), (1.0, 3)]), EINVAL, "pipeline_step_slots_lens: slot 1: on=3 must be 0, 1 or 2"),
    (SL + "_guided", A(CTX, guides_host=[(NAN, 1), (1.0, 0)]), EINVAL, "pipeline_step_slots_guided: slot 0: the guidance scale must be finite"),
    (SL + "_guided", A(guides_host=[(1.0, 0), (1.0, 1)]), EINVAL, "pipeline_step_slots_guided: slot 1: guidance needs a context (context NULL IS the unconditional branch)"),
    (SL + "_guided", A(L=4, guides_host=[(1.0, 7), (1.0, 0)]), EINVAL, "pipeline_step_slots_guided: slot 0: guidance needs a context (context NULL IS the unconditional branch)"),
    (SL + "_negative", A(CTX, guides_host=[(1.0, 1), (1.0, 2)]), EINVAL, "pipeline_step_slots_lens: slot 1: on=2 needs a negative context, given or kept"),
    (SL + "_negative", A(s2="s2 fresh", flags=KEEP_NEG, Ln=2), ESTATE, "pipeline_step_slots_negative: keep-negative asked for B=2 Ln=2, but no slots call has prepared a negative context on this handle (or another entry point replaced it)"),
    (SL, A(s2="s2 fresh", flags=KEEP_CTX, L=4), ESTATE, "pipeline_step_slots: keep-context asked for B=2 L=4, but no slots call has prepared a context on this handle (or another entry point replaced it)"),
    (SL + "_lens", A(s2="s2 fresh", flags=KEEP_CTX), ESTATE, "pipeline_step_slots_lens: keep-context asked for B=2 L=0, but no slots call has prepared a context on this handle (or another entry point replaced it)"),
    (SL, A(context=P, L=0), EINVAL, "s2: context given with L=0"),
    # an idle slot is not looked at
    (SL + "_filter", A(slots_host=[IDLE, (1, 0, 1.0, 0, 4, 0)], top_p_host=[7.0, 1.0]), EINVAL, "pipeline_step_slots_filter: slot 1: topk=0 must be in [1, n_embed=256]"),
    # the name: per entry, then per arm
    (SL + "_guided", A(ids=None), EINVAL, "pipeline_step_slots_guided: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_lens", A(ids=None), EINVAL, "pipeline_step_slots_lens: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_choice", A(ids=None), EINVAL, "pipeline_step_slots_lens: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_negative", A(ids=None), EINVAL, "pipeline_step_slots_lens: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_filter", A(ids=None), EINVAL, "pipeline_step_slots_filter: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_edit", A(ids=None), EINVAL, "pipeline_step_slots_filter: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_regions", A(ids=None), EINVAL, "pipeline_step_slots_filter: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_weights", A(ids=None), EINVAL, "pipeline_step_slots_filter: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_choice", A(ids=None, choice_host=[0.0, 0.0]), EINVAL, "pipeline_step_slots_choice: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_negative", A(ids=None, choice_host=[0.0, 0.0], neg_context=P), EINVAL, "pipeline_step_slots_negative: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_negative", A(ids=None, flags=KEEP_NEG), EINVAL, "pipeline_step_slots_negative: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_negative", A(ids=None, neg_lens_host=[1, 1]), EINVAL, "pipeline_step_slots_negative: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_choice", A(ids=None, flags=KEEP_NEG), EINVAL, "pipeline_step_slots_lens: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_edit", A(ids=None, neg_context=P, top_p_host=[1.0, 1.0]), EINVAL, "pipeline_step_slots_filter: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_edit", A(ids=None, neg_context=P, counts_host=[-1, -1]), EINVAL, "pipeline_step_slots_edit: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_regions", A(ids=None, counts_host=[-1, -1], region_host=[0, 0]), EINVAL, "pipeline_step_slots_regions: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_regions", A(ids=None, tok_seg_host=ALL * 2), EINVAL, "pipeline_step_slots_regions: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_weights", A(REG, ids=None), EINVAL, "pipeline_step_slots_regions: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_weights", A(REG, ids=None, ctx_w_host=W1), EINVAL, "pipeline_step_slots_weights: bad arguments (null handle, ids or slots, or B <= 0)"),
    # the order
    (SL + "_regions", A(ids=None, ctx_seg_host=SEG["ctx_seg_host"]), EINVAL, "pipeline_step_slots_regions: bad arguments (null handle, ids or slots, or B <= 0)"),
    (SL + "_regions", A(CTX, region_host=[3, 3]), EINVAL, "pipeline_step_slots_regions: ctx_seg_host, tok_seg_host and region_host come together (one of them is NULL)"),
    (SL + "_weights", A(CTX, ctx_w_host=W1, ctx_seg_host=SEG["ctx_seg_host"]), EINVAL, "pipeline_step_slots_weights: ctx_seg_host, tok_seg_host and region_host come together (one of them is NULL)"),
    (SL + "_weights", A(ctx_w_host=W1, ctx_lens_host=[1, 1]), EINVAL, "pipeline_step_slots_weights: ctx_w_host given without ctx_seg_host, tok_seg_host and region_host"),
    (SL + "_lens", A(CTX, s2="s2 n_embed=100", ctx_lens_host=[5, 1]), EINVAL, "pipeline_step_slots_lens: image 0: context length 5 must be in [1, L=4]"),
    (SL + "_regions", A(REG, context=None, region_host=[1, 3]), EINVAL, "pipeline_step_slots_regions: slot 1: region_host=3 must be 0 or 1 (2 needs ctx_w_host)"),
    (SL + "_regions", A(REG, context=None, ctx_seg_host=[40, 0, 1, 255] * 2), EINVAL, "pipeline_step_slots_regions: regional slots given without a context"),
    (SL + "_regions", A(REG, ctx_seg_host=[40, 0, 1, 255] * 2, tok_seg_host=[0] * 32), EINVAL, "pipeline_step_slots_regions: slot 0: context row 0: segment 40 must be in 0..31, or 255 for padding"),
    (SL + "_weights", A(REG, region_host=[2, 2], tok_seg_host=[4] * 32, ctx_w_host=[INF] * 8), EINVAL, "pipeline_step_slots_weights: slot 0: token 0 allows no segment that is present in its context (mask 0x00000004, present 0x00000003)"),
    (SL + "_weights", A(REG, region_host=[2, 2], ctx_w_host=[-1.0] + [0.0] * 7), EINVAL, "pipeline_step_slots_weights: slot 0: context row 0: weight -1 must be 0 or in [2^-20, 2^20]"),
    (SL + "_weights", A(REG, region_host=[2, 0], ctx_w_host=[0.0] * 8, ctx_lens_host=[4, 9]), EINVAL, "pipeline_step_slots_weights: slot 0: token 0 allows no context row with a weight above 0 (mask 0xffffffff, segments with such a row 0x00000000)"),
    (SL + "_regions", A(REG, s2="s2 n_embed=100", region_host=[1, 0], ctx_lens_host=[4, 9]), EINVAL, "pipeline_step_slots_regions: image 1: context length 9 must be in [1, L=4]"),
    (SL + "_negative", A(s2="s2 n_embed=100", neg_lens_host=[1, 1]), EINVAL, "pipeline_step_slots_negative: n_embed=100 must be a multiple of 64"),
    (SL + "_negative", A(neg_context=P, Ln=0, neg_lens_host=[1, 1]), EINVAL, "pipeline_step_slots_negative: negative context given with Ln=0"),
    (SL + "_negative", A(neg_context=P, Ln=2, neg_lens_host=[3, 1], choice_host=[-1.0, 0.0]), EINVAL, "pipeline_step_slots_negative: slot 0: negative context length 3 must be in [1, Ln=2]"),
    (SL + "_filter", A(choice_host=[-1.0, 0.0], slots_host=[(1, 0, 1.0, 0, 4, 0), GOOD]), EINVAL, "pipeline_step_slots_filter: the choice temperature -1 must be finite and in [0, 1000]"),
    (SL + "_filter", A(slots_host=[(1, 0, 1.0, 0, 4, 0), GOOD], top_p_host=[2.0, 1.0]), EINVAL, "pipeline_step_slots_filter: slot 0: topk=0 must be in [1, n_embed=256]"),
    (SL + "_choice", A(choice_host=[-1.0, 0.0], slots_host=[(1, 0, 1.0, 9, 4, 0), GOOD]), EINVAL, "pipeline_step_slots_choice: the choice temperature -1 must be finite and in [0, 1000]"),
    (SL + "_edit", A(top_p_host=[2.0, 1.0], counts_host=[99, 1]), EINVAL, "pipeline_step_slots_edit: slot 0: top_p=2 must be finite and in (0, 1]"),
    (SL + "_edit", A(counts_host=[-2, 1], slots_host=[(1, 0, 1.0, 3, 0, 0), GOOD]), EINVAL, "pipeline_step_slots_edit: slot 0: count -2 must be in [-1, tokens=16]"),
    (SL + "_negative", A(CTX, slots_host=[(1, 0, 1.0, 3, 0, 0), GOOD], guides_host=[(1.0, 3), (1.0, 0)]), EINVAL, "pipeline_step_slots_lens: slot 0: num_mask=0 must be >= 1"),
    (SL + "_negative", A(CTX, guides_host=[(NAN, 3), (1.0, 0)]), EINVAL, "pipeline_step_slots_lens: slot 0: on=3 must be 0, 1 or 2"),
    (SL + "_guided", A(guides_host=[(NAN, 1), (1.0, 0)]), EINVAL, "pipeline_step_slots_guided: slot 0: the guidance scale must be finite"),
    (SL + "_negative", A(guides_host=[(1.0, 2), (1.0, 0)]), EINVAL, "pipeline_step_slots_lens: slot 0: guidance needs a context (context NULL IS the unconditional branch)"),
    (SL + "_negative", A(s2="s2 fresh", L=4, flags=KEEP_CTX, guides_host=[(1.0, 2), (1.0, 0)]), EINVAL, "pipeline_step_slots_lens: slot 0: on=2 needs a negative context, given or kept"),
    (SL + "_negative", A(s2="s2 fresh", flags=KEEP_CTX | KEEP_NEG, L=4, Ln=2), ESTATE, "pipeline_step_slots_negative: keep-negative asked for B=2 Ln=2, but no slots call has prepared a negative context on this handle (or another entry point replaced it)"),
    (SL + "_negative", A(s2="s2 fresh", flags=KEEP_NEG, Ln=2, context=P, L=0), ESTATE, "pipeline_step_slots_negative: keep-negative asked for B=2 Ln=2, but no slots call has prepared a negative context on this handle (or another entry point replaced it)"),
]


def _signatures():
    """entry -> its parameter names, from include/pmhip.h (the header's types are checked against PROTOTYPES by test_abi_cpu.py)"""
    text = re.sub(r"/\*.*?\*/", "", open(_lib._HERE + "/../include/pmhip.h").read(), flags=re.S)
    sigs = {}
    for name, params in re.findall(r"\bint (pmhip_\w+)\(([^)]*)\)", text):
        sigs[name] = [re.findall(r"\w+", p)[-1] for p in params.split(",") if p.strip() and p.strip() != "void"]
    return sigs


SIGNATURES = _signatures()


def _s2_handle(lib, n_embed=N_EMBED):
    tower = _lib.TowerCfg(dim=64, depth=1, heads=1, hidden_pad=64, dim_head=64)
    cfg = _lib.S2Cfg(tokens=TOKENS, embed_dim=32, n_embed=n_embed, context_dim=64, context_dim_pad=64, tower=tower)
    w = _lib.S2Weights(layers=(_lib.LayerWeights * 1)())
    h = C.c_void_p()
    assert lib.pmhip_s2_create(C.byref(h), 0, _lib.F32, C.byref(cfg), C.byref(w)) == _lib.PMHIP_OK
    return h


@pytest.fixture(scope="module")
def handles():
    """handles that only keep their weights: creating one touches no device.  "s2": shared by the rows (a refused call leaves it as
    it was); "vq": a VQGAN of 2 x 1 x 32 x 32 = 2048 floats per image batch; "s2 fresh" and "s2 n_embed=100" are made per row"""
    lib = _lib.load()
    tower = _lib.TowerCfg(dim=64, depth=1, heads=1, hidden_pad=64, dim_head=64)
    cfg = _lib.VqganCfg(image_size=32, patch_size=8, channels=1, n_embed=N_EMBED, embed_dim=32, beta=0.25, enc=tower, dec=tower)
    w = _lib.VqganWeights(enc_layers=(_lib.LayerWeights * 1)(), dec_layers=(_lib.LayerWeights * 1)())
    vq = C.c_void_p()
    assert lib.pmhip_vqgan_create(C.byref(vq), 0, _lib.F32, C.byref(cfg), C.byref(w)) == _lib.PMHIP_OK
    made = {"s2": _s2_handle(lib), "vq": vq}
    yield made
    lib.pmhip_vqgan_destroy(made.pop("vq"))
    for h in made.values():
        lib.pmhip_s2_destroy(h)


def _convert(argtype, value):
    if value is None or isinstance(value, C.c_void_p) or not isinstance(value, list):
        return value
    elem = argtype._type_
    if elem in (_lib.Slot, _lib.SlotGuide):
        arr = (elem * len(value))()
        for i, rec in enumerate(value):
            if rec is IDLE:
                arr[i].step = _lib.SLOT_IDLE
            else:
                arr[i] = elem(*rec)
        return arr
    return (elem * len(value))(*value)


def _call(lib, handles, entry, args):
    values = dict(DEFAULTS, **args)
    names = SIGNATURES[entry]
    assert not set(args) - set(names), (entry, set(args) - set(names))
    fresh, call_args = [], []
    for name, argtype in zip(names, _lib.PROTOTYPES[entry][1]):
        v = values[name]
        if isinstance(v, str):                                # a handle, by name
            if v in handles:
                v = handles[v]
            else:
                v = _s2_handle(lib, **({"n_embed": 100} if v == "s2 n_embed=100" else {}))
                fresh.append(v)
        call_args.append(_convert(argtype, v))
    rc = getattr(lib, entry)(*call_args)
    msg = lib.pmhip_last_error().decode()
    for h in fresh:
        lib.pmhip_s2_destroy(h)
    return rc, msg


@pytest.mark.parametrize("number", range(len(ROWS)))
def test_refusal(handles, number):
    entry, args, rc, message = ROWS[number]
    assert _call(_lib.load(), handles, entry, args) == (rc, message), (entry, args)


def test_the_refused_slots_steps_counted_nothing_and_cached_nothing(handles):
    """behind the slots rows, on the handle they shared"""
    lib, h = _lib.load(), handles["s2"]
    n = [C.c_int(-1) for _ in range(11)]
    r = [C.byref(x) for x in n]
    assert lib.pmhip_s2_slots_passes(h, r[0], r[1], r[2]) == _lib.PMHIP_OK
    assert lib.pmhip_s2_slots_filter_steps(h, r[3], r[4]) == _lib.PMHIP_OK
    assert lib.pmhip_s2_slots_edit_steps(h, r[5]) == _lib.PMHIP_OK
    assert lib.pmhip_s2_slots_region_steps(h, r[6]) == _lib.PMHIP_OK
    assert lib.pmhip_s2_slots_weight_steps(h, r[7]) == _lib.PMHIP_OK
    assert lib.pmhip_s2_graph_count(h, r[8], r[9]) == _lib.PMHIP_OK
    assert [x.value for x in n[:10]] == [0] * 10
