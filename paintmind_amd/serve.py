"""Decode sessions: a fixed number of SLOTS decode together, every slot with its own MaskGIT schedule, temperature, top-k, seed
and global image index, and new requests are admitted into free slots between steps.

The native step behind it is pmhip_pipeline_step_slots (include/pmhip.h): the tower, the attention and the sampler never mix
rows, and the sampling tail reads every per-image value from a device record, so a request computes what it would compute alone
whatever shares the batch with it.  The contract ("Decode sessions"): a request (T, temperature, topk, seed, image
index k, context c) that sits in slot j of an S-slot session produces, bit for bit, the per-step predictions, scores and final
ids of row j of ``Pipeline.generate_ids(context with c in row j, B=S, T, temperature, topk, ..., seed, image_base=k - j,
streams=1, guidance_scale=s)``; its image is ``vqgan.decode_from_indice`` of the last step's predictions.

Contexts of different lengths share a session: a request's ``context`` is ``[L_r, D]`` with its own ``L_r``.  The session keeps its
contexts in one ``[S, capacity, D]`` tensor -- ``max_context_len`` rows, or, when that is None, as many as the longest context
admitted so far (growing re-prepares the cross K/V) -- and hands the native step one length per slot
(pmhip_pipeline_step_slots_lens), so a request never attends to the rows behind its own.  The contract above then reads
``generate_ids(context padded to the capacity, context_lens with L_r in row j, ...)`` (a step taken at capacity C is the scalar
step at capacity C: a request that lives through a growth follows the capacity step by step).  A step in which every occupied slot fills
the capacity passes no lengths, which IS the step without them: the same result, on the kernels every earlier version ran.

Guidance is per request (``submit(guidance_scale=s)``, conditional sessions only): the native step
(pmhip_pipeline_step_slots_guided) reads a scale per slot from a second device record, runs the tower twice in a step in which
at least one active slot is guided, and combines the two towers' logits on the rows of the guided slots only, so requests with
different scales, and unguided ones, share a batch and each computes what it would compute alone.

Limits: a session is all-conditional or all-unconditional (``context=None`` selects attn2's inputs for the whole batch), every
context of a session has the same width D, top-k <= 8 (the block-statistics sampling kernel: ``Pipeline.generate`` takes any
top-k up to n_embed, and ``None`` for no filter, DESIGN.md section 4n, but this session does not -- a batch that mixes requests at
and above 8 needs further sampling launches chosen step by step: ``decode_session(filters=True)``, the FilterSession below), and
idle slots still run through the tower (no compaction).  For the same reason an unguided slot beside a guided one still pays the
second tower pass: the unconditional pass runs at the session's batch size.

A negative prompt and a guidance schedule are per request as well (``submit(negative_text=..., guidance_scale=[s_0, ..., s_T-1])``,
what ``Pipeline.generate`` takes for a whole batch).  A request's negative context is ``[Ln_r, D]`` with its own length; the session
keeps them in a second ``[S, capacity_n, D]`` tensor with the rules of the contexts (``max_negative_len``, or growing with the
longest one admitted; growth or admission re-prepares the negative K/V; a step in which every occupied slot with a negative
prompt fills the capacity passes no lengths).  The guide record of a slot says what it is guided against -- nothing, the pass
without a context, or the negative context -- and the native step (pmhip_pipeline_step_slots_negative) runs, beside the
conditional pass, the pass without a context iff an occupied slot needs it and the pass against the negative K/V iff one needs
that: up to three tower passes, each combine touching only the slots of its kind.  A schedule is written into the slot's guide
record step by step.  The contract reads ``generate_ids(..., guidance_scale=s or the schedule, negative_context=[S, capacity_n, D]
with the request's rows in row j, negative_lens with Ln_r in row j)``.  A session without such a request runs the steps it ran
before there were any.

A choice temperature is per request too (``submit(choice_temperature=c)``): the request keeps MaskGIT's annealed value of each of
its steps beside its temperatures and mask counts, the native step (pmhip_pipeline_step_slots_choice) reads one value per slot
from a device array, and the contract reads ``generate_ids(..., choice_temperature=c)``.  A step in which no occupied slot has a
non-zero value passes none, which IS the step without: the same kernels and graph as before.  The guided loop's step-0 cache ("Not built") stays
not built.

The sampler filters are per request in a FilterSession (``pipe.decode_session(..., filters=True)``):
``submit(topk=k, top_p=p)`` with k anywhere in 1..n_embed (``None``: no filter) and a nucleus mass p in (0, 1] (``None``: none),
what ``Pipeline.generate`` takes for a whole batch.  Which sampling kernel serves a row depends on its request's (topk, top_p < 1)
alone, so the native step (pmhip_pipeline_step_slots_filter) issues one sampling launch per kernel class, each serving the rows of
its class, and a step in which every occupied slot has top-k <= 8 and no nucleus runs the launches and the graph of the session
above.  The contract sentence extends unchanged: a request (T, temperature, topk, top_p, seed, k, ...) in slot j of an S-slot
session produces, bit for bit, the per-step predictions, scores and final ids of row j of ``generate_ids(..., B=S, topk=topk,
top_p=top_p, ..., image_base=k - j, streams=1)``.

Edit requests: ``submit(ids0=x, keep_given=True)`` regenerates the m positions of x that hold the mask id
and KEEPS the rest -- ``Pipeline.edit`` for one request -- and ``submit(image=[C,H,W], mask=[H,W] | token_mask=[g,g],
preserve="tokens" | "pixels")`` builds x from an image at submit (``to_latent`` at B = 1 and the mask operator of ``Pipeline.edit``).
The request's re-masking counts are ``edit_schedule(m, T)`` instead of ``loop_schedule``'s, m counted once at submit, so a given id
is never re-masked and no mask id is left at the end; its temperatures and choice temperatures are unchanged.  The native step
(pmhip_pipeline_step_slots_edit) takes one count per slot beside the records -- the request's own for an edit, -1 (the record's)
for a generation, 0 leaving the row as the sampler merged it -- and ``Finished.image`` of an edit is decoded from its merged ids,
in the one decode call of the step (``preserve="pixels"`` then composites the original pixels back outside the pixel mask).  The
contract reads: an edit request in slot j produces, bit for bit, the per-step predictions and scores and the final ids of row j of
``Pipeline.edit_ids(ids with x in row j, counts with m in row j, ..., B=S, image_base=k - j, use_graph=False)``, whatever shares the
batch with it; every other keyword of a request composes unchanged, and a step in which no occupied slot is an edit request passes
no counts, which IS the step without: the same kernels and graph as before.

Regional prompts are per request in a session opened with ``pipe.decode_session(..., regions=True)`` (it is an
option of the session, not a class of its own, so it composes with ``filters=True``; without it ``regions=`` is refused as
before).  ``submit(text=..., regions=[(prompt, mask), ...])`` takes ONE image's list of what ``Pipeline.generate(regions=)`` takes
per image: ``prompt`` a string (or a ``[L_r, D]`` tensor when ``context=`` is given instead of ``text=``), ``mask`` a pixel mask
``[H, W]`` or a bool token mask ``[g, g]``, at most ``MAX_REGIONS`` regions.  The request's context is the concatenation [global |
region 1 | ...], built at submit by the code of ``generate`` at B = 1; its length is the total, and the capacity rules above
(``max_context_len``, growth, re-preparing the K/V) apply to the total.  The native step (pmhip_pipeline_step_slots_regions) takes,
beside everything above, a segment row and a token-mask row per slot and a flag per slot: every layer's cross-attention of the
pass with the context is then two launches into one buffer, the per-image-length kernel serving the plain slots and the
per-query kernel serving the regional ones, each returning at once on the other kind's images.  The contract: a regional request
in slot j of an S-slot session produces, bit for bit, the per-step predictions, the scores and the final ids of row j of
``generate_ids(context [S, capacity, D] with its rows in row j, context_segments / token_segments with its layout in row j and a
one-segment layout in the other rows, B=S, ..., image_base=k - j, streams=1)``; a request WITHOUT regions in the same session still
equals row j of ``generate_ids(..., context_lens=...)``, as in the default session; both hold whatever shares the batch.  A step
passes the arrays only while an occupied slot is regional: a session without such a request runs the steps it ran before.
Guidance or a schedule, a negative prompt, a choice temperature, the filters and the seed compose unchanged (the pass without a
context and the negative prompt's pass never see regions).  An edit request (``keep_given``, ``image=``) with ``regions=`` is
refused -- there is no scalar edit with regions to be identical to -- and so is ``regions=`` in an unconditional session.

Prompt weights are per request in a session opened with ``pipe.decode_session(..., weights=True)`` (an option
like ``regions=``, composing with it and with ``filters=True``; without it the session is the one above, refusals included).
``submit(text=...)`` is then read as ``Pipeline.generate(prompt_weights=True)`` reads it -- the session calls ``text_model([text],
weighted=True)`` and, as a session always does, attends to the context in full; ``submit(context=(ctx [L, D], w [L]))`` takes the
weights explicitly (a plain tensor stays what it was); with ``regions=True`` an item of ``regions=`` may be ``(prompt, mask, weight)``
and beside ``text=`` the region prompts are read for emphasis too (``_region_context_weighted`` at B = 1).  ``negative_text`` is not
read for emphasis.  A request is WEIGHTED iff any weight of its context is not exactly 1 (``weighted`` below states the rule; its
``Request.weights`` is then the array, otherwise None): it runs as kind 2 of the native step (pmhip_pipeline_step_slots_weights: a
kind per slot -- 0 under its length, 1 under its key sets, 2 under its key sets and its weights), under its own segments if it is
regional and the one-segment layout otherwise; every other request keeps the kind and the cost it has today.  Every layer's
cross-attention of the pass with the context is then three picked launches into one buffer, the third being the picked weighted
form.  The contract: a weighted request in slot j of an S-slot session produces, bit for bit, the per-step predictions, the scores
and the final ids of row j of ``generate_ids(context [S, capacity, D] with its rows in row j, context_segments / token_segments with
its layout (or the one-segment layout: segment 0 below its total, 255 behind, token masks of 1) in row j, context_weights with its
weights in row j, neutral rows -- one segment, weights of 1 -- elsewhere, B=S, ..., image_base=k - j, streams=1)``; the plain and the
regional requests beside it still equal their ``context_lens=`` / segment rows.  A step passes the weights only while an occupied
slot is weighted: a session without such a request runs the steps, launches and graphs it ran before.  An edit request with
weights (the edit loop takes none), weights in an unconditional session and a weight outside 0 / [2^-20, 2^20] raise ValueError.

On a CPU pipeline the session steps every occupied slot alone through the plain-torch step (B = 1, seed + step, like
``Pipeline.generate`` on the CPU): a request then equals ``pipe.generate([text], ..., seed=seed, guidance_scale=s,
negative_text=n)`` -- in a FilterSession with ``topk=, top_p=`` as well -- and an edit request equals ``pipe.edit(img[None], ...,
seed=seed)``; a regional request equals ``pipe.generate([text], regions=[regions], ..., seed=seed)``; in a weights session a request with
emphasis equals ``pipe.generate([text], prompt_weights=True, ..., seed=seed)``, ids and image exact.
"""
import collections
import math
import os

import numpy as np
import torch

from . import _lib, ops

Finished = collections.namedtuple("Finished", ["handle", "image", "ids"])


def weighted(weights):
    """THE rule of a weights session: a request is weighted iff any weight of its context is not exactly 1.
    Every other request is the request it would be in a session without the option, at the cost it has there."""
    return weights is not None and bool((np.asarray(weights, np.float32) != 1).any())


def _no_regions(regions):
    if regions is not None:
        raise ValueError("a decode session serves no regional prompts (regions=): Pipeline.generate(regions=) does")


class _SlotContexts:
    """the contexts of a session's slots in one tensor [S, capacity, D] fp32, on the GPU: `capacity` rows when it is fixed, else as
    many as the longest context admitted so far; a slot's rows behind its length are 0.  dirty: a slot's rows changed since the
    cross K/V were prepared from the tensor."""

    def __init__(self, slots, capacity=None):
        self.slots, self.capacity = slots, capacity
        self.tensor = None
        self.dirty = True
        self.lens = [1] * slots             # rows of every slot (a slot that holds none keeps a valid value)

    def admit(self, slot, rows):
        """slot `slot` holds `rows` [L_r, D] (on the device) from now on: grow to L_r rows if need be, fill, zero the tail"""
        Lr, D = rows.shape
        if self.tensor is None:
            self.tensor = torch.zeros(self.slots, self.capacity or Lr, D, device=rows.device, dtype=torch.float32)
        if D != self.tensor.shape[2]:
            raise ValueError(f"every context of a session has the same width: {D} != {self.tensor.shape[2]}")
        if Lr > self.tensor.shape[1]:               # no fixed capacity (submit checked the other case): it grows
            grown = torch.zeros(self.slots, Lr, D, device=rows.device, dtype=torch.float32)
            grown[:, :self.tensor.shape[1]] = self.tensor
            self.tensor = grown
        self.tensor[slot, :Lr] = rows
        self.tensor[slot, Lr:] = 0
        self.lens[slot] = Lr
        self.dirty = True

    def step_lens(self, uses):
        """this step's length per slot -- or None when every slot of `uses` (one bool per slot) fills the capacity, which IS the step
        without lengths"""
        cap = self.tensor.shape[1]
        if not any(u and n != cap for u, n in zip(uses, self.lens)):
            return None
        return [min(n, cap) for n in self.lens]


class Request:
    """what submit() returns: the request's parameters, its schedule and where / when it ran"""

    def __init__(self, number, text, context, timesteps, temperature, topk, seed, image_index, temps, nmask, ids0, guidance_scale=None,
                 ctemps=None, negative=None, scales=None, top_p=1.0, edit=False, orig=None, pixel_mask=None, segments=None, weights=None):
        # a weighted request (``weighted`` above): numpy float32 [L_r], the weight of every row of its context; None: a plain one
        self.weights = weights
        # a regional request: (numpy uint8 [L_r], the segment of every row of its context; numpy uint32 [N], the segments of every token)
        self.segments = segments
        self.edit = edit                            # an edit request: nmask is edit_schedule's over its masked start ids, given ids stay
        self.orig, self.pixel_mask = orig, pixel_mask   # preserve="pixels": the image [C,H,W] and the pixel mask uint8 [H,W] to composite by
        self.top_p = top_p                          # the nucleus mass (1: none; a FilterSession's requests may carry another)
        self.number, self.text, self.context = number, text, context
        self.negative = negative                    # None: no negative prompt; else its context [Ln_r, D]
        self.scales = scales                        # None: one scale (guidance_scale); else the scale of every step
        self.ctemps = ctemps                        # None: no choice temperature; else the annealed value of every step
        self.guidance_scale = guidance_scale        # None: not guided
        self.timesteps, self.temperature, self.topk, self.seed, self.image_index = timesteps, temperature, topk, seed, image_index
        self.temps, self.nmask = temps, nmask
        self.ids0 = ids0
        self.slot = None            # the slot it was admitted into
        self.admitted = None        # tick of the step() that admitted it; it retires at tick admitted + timesteps - 1
        self.retired = None
        self.done = 0               # steps taken
        self.trace = []             # record_steps: (pred [N], score [N]) of every step, on the device

    def __repr__(self):
        return (f"Request(#{self.number}, T={self.timesteps}, temperature={self.temperature}, topk={self.topk}, seed={self.seed}, "
                f"image_index={self.image_index}, guidance_scale={self.guidance_scale}, slot={self.slot}, admitted={self.admitted}, retired={self.retired})")


class DecodeSession:
    """``pipe.decode_session(slots=64, conditional=True, use_graph=True)``; see the module docstring.
    use_graph=None follows PMHIP_GENERATE_GRAPH like ``Pipeline.generate``."""

    def __init__(self, pipe, slots=64, conditional=True, use_graph=None, record_steps=False, decode=True, max_context_len=None,
                 max_negative_len=None, regions=False, weights=False):
        self.weights = bool(weights)        # prompt weights are served; False: refused, as before there was the option
        self.regions = bool(regions)        # submit(regions=) is served; False: refused, as before there was the option
        if slots < 1:
            raise ValueError("a decode session needs at least one slot")
        if max_negative_len is not None and int(max_negative_len) < 1:
            raise ValueError("max_negative_len must be >= 1 (or None: the capacity grows with the negative contexts admitted)")
        self.max_negative_len = None if max_negative_len is None else int(max_negative_len)
        if max_context_len is not None and int(max_context_len) < 1:
            raise ValueError("max_context_len must be >= 1 (or None: the capacity grows with the contexts admitted)")
        self.max_context_len = None if max_context_len is None else int(max_context_len)
        self.pipe, self.size, self.conditional = pipe, int(slots), bool(conditional)
        if use_graph is None:
            use_graph = os.environ.get("PMHIP_GENERATE_GRAPH", "1") != "0"
        self.use_graph = bool(use_graph)
        self.record_steps = record_steps    # keep every step's (pred, score) rows in Request.trace (tests, inspection)
        self.decode = decode                # False: Finished.image is None (the caller only wants the ids)
        self.queue = collections.deque()
        self.occupied = [None] * self.size  # slot -> Request
        self.tick = 0                       # step() calls so far
        self._submitted = 0
        self._next_index = 0
        self._cpu = pipe._on_cpu()
        self._ids = None                    # GPU: [S, N] int64, one row per slot; CPU: one [1, N] tensor per slot
        self._rows = [None] * self.size
        self._contexts = _SlotContexts(self.size, self.max_context_len)     # GPU, conditional: the contexts
        self._negatives = _SlotContexts(self.size, self.max_negative_len)    # GPU: the negative contexts, once a request brought one
        self._records = (_lib.Slot * self.size)()
        self._guides = (_lib.SlotGuide * self.size)() if self.conditional else None

    # the context tensor and its flag, as the session's own attributes (tests and tools poison padding rows through them)
    _ctx = property(lambda self: self._contexts.tensor)
    _ctx_dirty = property(lambda self: self._contexts.dirty, lambda self, dirty: setattr(self._contexts, "dirty", dirty))

    # -- requests -----------------------------------------------------------------------------------
    def submit(self, text=None, timesteps=18, temperature=1.0, topk=5, seed=None, image_index=None, context=None, ids0=None,
               guidance_scale=None, choice_temperature=None, negative_text=None, negative_context=None, keep_given=False, image=None,
               mask=None, token_mask=None, preserve="tokens", regions=None):
        """queue one request (any time, also between steps) -> its Request.  `context` [L_r, D] may be given instead of `text`
        (a conditional session runs the pipeline's text model on `text` otherwise), with its OWN length L_r: the request attends
        to exactly these rows; `ids0` [N]: start ids instead of all-mask;
        `guidance_scale` (None = not guided): this request samples from uncond + scale * (cond - uncond), like
        ``Pipeline.generate(guidance_scale=)``; `choice_temperature` (None or 0 = the deterministic re-masking): MaskGIT's base
        choice temperature, annealed over this request's own steps like ``Pipeline.generate(choice_temperature=)``.
        `guidance_scale` may also be a sequence of `timesteps` finite numbers, one per step of THIS request (a guidance schedule).
        `negative_text` / `negative_context` [Ln_r, D] (needs guidance_scale): a negative prompt -- the request samples from
        neg + scale * (cond - neg), like ``Pipeline.generate(negative_text=)``; the text goes through the pipeline's text model like
        `text`, the context has its own length like `context`.
        `keep_given` (with `ids0`): an EDIT request over the m positions of `ids0` that hold the mask id -- its re-masking counts are
        ``edit_schedule(m, timesteps)``, so a given id is never re-masked, no mask id is left at the end, and the image is decoded
        from the merged ids (``Pipeline.edit`` for one request).
        `image` [C,H,W] with exactly one of `mask` [H,W] (pixels, non-zero = regenerate) / `token_mask` bool [g,g]: the same edit
        from an image -- it is encoded and masked here, at submit -- and `preserve` ("tokens" | "pixels"): "pixels" puts the original
        pixels back outside the pixel mask, as in ``Pipeline.edit``.
        `regions`: refused -- unless the session was opened with ``regions=True``: then ONE image's list ``[(prompt, mask), ...]`` of
        ``Pipeline.generate(regions=)``, `text` (or `context`) staying the global prompt (the module docstring has the rules).
        In a session opened with ``weights=True`` `text` (and the prompts of `regions`) may carry emphasis, ``a (red:1.4) barn``,
        `context` may be a pair ``(context [L_r, D], weights [L_r])``, and an item of `regions` may be ``(prompt, mask, weight)``."""
        if not self.regions:
            _no_regions(regions)
        return self._submit(text, timesteps, temperature, topk, None, seed, image_index, context, ids0, guidance_scale, choice_temperature,
                            negative_text, negative_context, keep_given, image, mask, token_mask, preserve, regions)

    def _filters(self, topk, top_p):
        """a request's sampler filters as this session serves them -> (topk, top_p): top-k in 1..8 where the native slots step runs
        (the block-statistics kernel), no nucleus"""
        topk = int(topk)
        if not self._cpu and not 1 <= topk <= 8:
            raise ValueError(f"a decode session serves topk in 1..8, got {topk}")
        return topk, 1.0

    def _region_request(self, text, context, regions, weights=None):
        """submit(regions=) -> (the request's context [L_total, D]: global | region 1 | ..., (its segment row uint8 [L_total], its
        token masks uint32 [N]), its weights float32 [L_total] or None), by the code of ``Pipeline.generate(regions=)`` at B = 1.
        In a weights session the prompts are read for emphasis (``generate(prompt_weights=True)``), `weights` are those of a
        ``context=`` pair (the global prompt's rows), and a region's third element multiplies its rows' weights."""
        from .generate import MAX_REGIONS, region_layout
        pipe = self.pipe
        regions = list(regions)
        if len(regions) > MAX_REGIONS:
            raise ValueError(f"regions: {len(regions)} regions, at most {MAX_REGIONS} per request")
        if context is None:
            if text is None:
                raise ValueError("a conditional session needs a text (or a context) for every request")
            ctx, cs, ts, weights = pipe._region_context_weighted([text], [regions], False, self.weights)
            if weights is not None and not self.weights:
                raise ValueError("regions: a decode session serves no prompt weights ((prompt, mask, weight)): Pipeline.generate(regions=) does")
            weights = None if weights is None else weights[0]
        else:
            sizes = (2, 3) if self.weights else (2,)
            for item in regions:
                if not (isinstance(item, (tuple, list)) and len(item) in sizes and isinstance(item[0], torch.Tensor) and item[0].dim() == 2
                        and item[0].shape[0] >= 1 and item[0].shape[1] == context.shape[-1]):
                    raise ValueError("regions: beside context= every region is a (context [L_r, D], mask) pair of the context's width")
                if len(item) == 3 and (isinstance(item[2], bool) or not isinstance(item[2], (int, float))):
                    raise ValueError("regions: beside context= every region is a (context [L_r, D], mask) pair of the context's width")
            if context.dim() != 2 or context.shape[0] < 1:
                raise ValueError(f"a request's context is [L, D] with L >= 1, got {tuple(context.shape)}")
            ctx, cs, ts = region_layout([[context] + [item[0] for item in regions]], [[item[1] for item in regions]], pipe.image_size,
                                        pipe.patch_size)
            if self.weights:                            # the pair's weights on the global rows, a region's number on its rows
                parts = [np.ones(context.shape[0], np.float32) if weights is None else np.asarray(weights, np.float32).reshape(-1)]
                parts += [np.full(item[0].shape[0], item[2] if len(item) == 3 else 1.0, np.float32) for item in regions]
                weights = np.concatenate(parts)
        return ctx[0], (cs[0], ts[0]), weights

    def _request_weights(self, weights, context, segments):
        """a weights session's request: its weights as they came (the text model's, a ``context=`` pair's, the regions') -> numpy
        float32 [L_r] checked by ``ops.host_weights`` at B = 1 under the request's own layout, or None when the request is not
        weighted (``weighted``): it is then a plain request"""
        if weights is None:
            return None
        w = weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else np.asarray(weights)
        L = context.shape[0]
        if w.shape != (L,) or w.dtype.kind not in "fiu":
            raise ValueError(f"a request's weights are numbers of shape ({L},), one per context row, got {w.dtype} {w.shape}")
        cs, ts = (None, None) if segments is None else (segments[0][None], segments[1][None])
        w = ops.host_weights(w[None], 1, L, self.pipe.num_tokens, cs, ts)[2][0]
        return w if weighted(w) else None

    def _segment_arrays(self, capacity):
        """this step's (ctx_seg uint8 [S, capacity], tok_seg uint32 [S, N], flags uint8 [S]) for the native step, or None when no
        occupied slot is regional or weighted (the step without).  The flag is the slot's kind: 0 plain, 1 regional, 2 weighted
        (DESIGN.md section 4x).  A regional slot's rows are its layout, 255 behind its total; every other
        slot's rows are the one-segment layout (the native step does not look at them)."""
        if not any(r is not None and (r.segments is not None or r.weights is not None) for r in self.occupied):
            return None
        cs = np.zeros((self.size, capacity), np.uint8)
        ts = np.ones((self.size, self.pipe.num_tokens), np.uint32)
        flags = np.zeros(self.size, np.uint8)
        for j, r in enumerate(self.occupied):
            if r is None:
                continue
            cs[j, r.context.shape[0]:] = 255
            if r.segments is not None:
                cs[j, :r.context.shape[0]] = r.segments[0]
                ts[j] = r.segments[1]
                flags[j] = 1
            if r.weights is not None:                   # under its own segments if it is regional, the one-segment layout otherwise
                flags[j] = 2
        return cs, ts, flags

    def _weight_array(self, capacity):
        """this step's weights float32 [S, capacity] for the native step, or None when no occupied slot is weighted (the step
        without).  A weighted slot's row is its weights, 1 behind its total; every other slot's row is 1 (not looked at)."""
        if not any(r is not None and r.weights is not None for r in self.occupied):
            return None
        w = np.ones((self.size, capacity), np.float32)
        for j, r in enumerate(self.occupied):
            if r is not None and r.weights is not None:
                w[j, :r.weights.shape[0]] = r.weights
        return w

    def _edit_start(self, ids0, keep_given, image, mask, token_mask, preserve):
        """the edit keywords of submit(), checked -> (ids0, edit, orig, pixel mask): an image is encoded (B = 1) and masked here, by
        the operators and the checks of ``Pipeline.edit``; orig / pixel mask only where preserve asks for the pixels"""
        pipe = self.pipe
        if preserve not in ("tokens", "pixels"):
            raise ValueError(f"preserve must be 'tokens' or 'pixels', got {preserve!r}")
        if image is None:
            if mask is not None or token_mask is not None:
                raise ValueError("a mask needs the image it is about (image=)")
            if preserve == "pixels":
                raise ValueError("preserve='pixels' needs the image whose pixels are kept (image=)")
            if keep_given and ids0 is None:
                raise ValueError("keep_given needs the start ids whose given positions are kept (ids0=)")
            return ids0, bool(keep_given), None, None
        if ids0 is not None:
            raise ValueError("give the start of an edit as image= (with a mask) or as ids0=, not both")
        if image.dim() != 3:
            raise ValueError(f"a request's image is [C, H, W], got {tuple(image.shape)}")
        device = "cpu" if self._cpu else pipe.engine().device
        img = image[None].to(device)
        tm, pm = pipe._edit_masks(img, mask, token_mask)
        with torch.no_grad():
            ids = pipe.to_latent(img)[1].reshape(1, pipe.num_tokens)
        if not self._cpu:
            ids = ids.to(device, torch.long).clone(memory_format=torch.contiguous_format)
        ids, _ = pipe._masked_ids(ids, tm, pm)
        if preserve == "pixels":
            return ids[0], True, img[0], pm[0]
        return ids[0], True, None, None

    def _submit(self, text, timesteps, temperature, topk, top_p, seed, image_index, context, ids0, guidance_scale, choice_temperature,
                negative_text, negative_context, keep_given=False, image=None, mask=None, token_mask=None, preserve="tokens", regions=None):
        """submit() behind its keywords; (topk, top_p) go through _filters, the session's own range of them"""
        topk, top_p = self._filters(topk, top_p)
        segments, weights = None, None
        if isinstance(context, (tuple, list)):          # the pair (context [L_r, D], weights [L_r]) of a weights session
            if not self.weights:
                raise ValueError("a decode session serves no prompt weights (context=(context, weights)): open it with weights=True")
            if not self.conditional:
                raise ValueError("prompt weights need a text condition (an unconditional session IS the unconditional branch)")
            if len(context) != 2 or not isinstance(context[0], torch.Tensor):
                raise ValueError("context= is a tensor [L, D] or a pair (context [L, D], weights [L])")
            context, weights = context
        if regions is not None:
            if not self.conditional:
                raise ValueError("regions need a text condition (an unconditional session IS the unconditional branch)")
            if keep_given or image is not None:
                raise ValueError("an edit request (keep_given, image=) takes no regions: Pipeline.edit has none to be identical to")
            context, segments, weights = self._region_request(text, context, regions, weights)
        elif self.weights and self.conditional and context is None and text is not None:
            # the text is read as generate(prompt_weights=True) reads it; the context is attended to in full, as a session always does
            context, _, weights = self.pipe.text_model([text], weighted=True)
            if context is None:
                raise ValueError("the pipeline's text model gives no context: open the session with conditional=False")
            context, weights = context[0], weights[0]
        if weights is not None:
            if context.dim() != 2 or context.shape[0] < 1:
                raise ValueError(f"a request's context is [L, D] with L >= 1, got {tuple(context.shape)}")
            weights = self._request_weights(weights, context, segments)
            if weights is not None and (keep_given or image is not None):
                raise ValueError("an edit request (keep_given, image=) takes no prompt weights: Pipeline.edit has none to be identical to")
        ids0, edit, orig, pixel_mask = self._edit_start(ids0, keep_given, image, mask, token_mask, preserve)
        timesteps = int(timesteps)
        if timesteps < 1:
            raise ValueError("timesteps must be >= 1")
        scales = None
        if guidance_scale is not None:
            if not self.conditional:
                raise ValueError("guidance_scale needs a text condition (an unconditional session IS the unconditional branch)")
            scalar, scales = ops.guidance_parts(guidance_scale, timesteps)
            if scales is None:
                guidance_scale = float(scalar)
                if not math.isfinite(guidance_scale):
                    raise ValueError("guidance_scale must be finite")
        negative = None
        if negative_text is not None or negative_context is not None:
            if not self.conditional:
                raise ValueError("a negative prompt needs a text condition (an unconditional session IS the unconditional branch)")
            if guidance_scale is None:
                raise ValueError("a negative prompt needs guidance_scale (the step moves away from it by that much)")
            if negative_context is None:
                negative_context = self.pipe._negative_context(negative_text, 1, False)[0]
                if negative_context is None:
                    raise ValueError("the pipeline's text model gives no context for the negative prompt")
                negative_context = negative_context[0]
            negative = negative_context.detach().to(torch.float32)
            if negative.dim() != 2 or negative.shape[0] < 1:
                raise ValueError(f"a request's negative context is [Ln, D] with Ln >= 1, got {tuple(negative.shape)}")
            if self.max_negative_len is not None and negative.shape[0] > self.max_negative_len:
                raise ValueError(f"a negative context of {negative.shape[0]} rows does not fit the session's max_negative_len={self.max_negative_len}")
        if self.conditional:
            if context is None:
                if text is None:
                    raise ValueError("a conditional session needs a text (or a context) for every request")
                context = self.pipe.text_model([text])
                if context is None:
                    raise ValueError("the pipeline's text model gives no context: open the session with conditional=False")
                context = context[0]
            context = context.detach().to(torch.float32)
            if context.dim() != 2 or context.shape[0] < 1:
                raise ValueError(f"a request's context is [L, D] with L >= 1, got {tuple(context.shape)}")
            if self.max_context_len is not None and context.shape[0] > self.max_context_len:
                raise ValueError(f"a context of {context.shape[0]} rows does not fit the session's max_context_len={self.max_context_len}")
            if negative is not None and negative.shape[1] != context.shape[1]:
                raise ValueError(f"a negative context has the context's width: {negative.shape[1]} != {context.shape[1]}")
        elif context is not None:
            raise ValueError("an unconditional session takes no context")
        if seed is None:
            from .generate import _draw_seed
            seed = _draw_seed()
        if image_index is None:
            image_index = self._next_index
            self._next_index += 1
        if ids0 is not None:
            ids0 = self.pipe._start_ids(1, ids0.reshape(1, -1), ids0.device)
        from .generate import edit_schedule, loop_schedule
        temps, nmask, ctemps = loop_schedule(timesteps, temperature, self.pipe.num_tokens, choice_temperature)
        if edit:                                    # m is counted once, here: the schedule over the region instead of the image
            nmask = edit_schedule(int((ids0 == self.pipe.mask_token_id).sum()), timesteps)
        r = Request(self._submitted, text, context, timesteps, temperature, topk, int(seed), int(image_index), temps, nmask, ids0, guidance_scale,
                    ctemps, negative, scales, top_p, edit, orig, pixel_mask, segments, weights)
        self._submitted += 1
        self.queue.append(r)
        return r

    @property
    def active(self):
        return sum(1 for r in self.occupied if r is not None)

    def idle(self):
        return not self.queue and self.active == 0

    # -- stepping -----------------------------------------------------------------------------------
    def _admit(self):
        admitted = []
        for j in range(self.size):
            if not self.queue:
                break
            if self.occupied[j] is None:                 # FIFO into the lowest free slot
                r = self.queue.popleft()
                r.slot, r.admitted = j, self.tick
                self.occupied[j] = r
                admitted.append(r)
        return admitted

    @torch.no_grad()
    def step(self):
        """admit queued requests, run ONE MaskGIT step for every occupied slot, retire the slots that took their last step
        -> [Finished(handle, image [C,H,W], ids [N]), ...] in slot order"""
        admitted = self._admit()
        out = self._step_cpu(admitted) if self._cpu else self._step_gpu(admitted)
        self.tick += 1
        return out

    def drain(self):
        """step until the queue and all slots are empty -> everything that finished on the way"""
        out = []
        while not self.idle():
            out += self.step()
        return out

    def _retire(self, r):
        r.retired = self.tick
        self.occupied[r.slot] = None

    def _step_filters(self):
        """what this step's native call takes beyond DecodeSession's: nothing"""
        return {}

    def _step_cpu(self, admitted):
        pipe = self.pipe
        for r in admitted:
            self._rows[r.slot] = pipe._start_ids(1, r.ids0, "cpu")
        out = []
        for j, r in enumerate(self.occupied):
            if r is None:
                continue
            t = r.done
            ctx = None if r.context is None else r.context[None]
            neg = None if r.negative is None else r.negative[None]
            # an edit request: the step with a count per image, as Pipeline.edit's CPU branch takes it
            cs, ts = (None, None) if r.segments is None else (r.segments[0][None], r.segments[1][None])
            keys = ops.host_keys(1, 0 if ctx is None else ctx.shape[1], pipe.num_tokens, None, cs, ts,
                                 None if r.weights is None else r.weights[None], has_context=ctx is not None)
            ids, img = pipe._sample_cpu(self._rows[j], 0 if r.edit else r.nmask[t], ctx, r.topk, r.temps[t], None, r.seed + t,
                                        r.scales[t] if r.scales else r.guidance_scale, keys, r.ctemps[t] if r.ctemps else 0.0,
                                        top_p=r.top_p, negative=neg, negative_lens=None, **({"counts": [r.nmask[t]]} if r.edit else {}))
            self._rows[j] = ids
            r.done = t + 1
            if r.done == r.timesteps:
                if r.edit and self.decode:          # from the merged ids; the original pixels back outside the mask
                    img = pipe.vqgan.decode_from_indice(ids)
                    if r.orig is not None:
                        img = torch.where(r.pixel_mask[None, None] != 0, img, r.orig[None].to(img.dtype))
                out.append(Finished(r, img[0] if self.decode else None, ids[0].clone()))
                self._rows[j] = None
                self._retire(r)
        return out

    def _step_gpu(self, admitted):
        pipe = self.pipe
        eng = pipe.engine()
        N, mask_id = pipe.num_tokens, pipe.mask_token_id
        if self._ids is None or self._ids.device != eng.device:
            self._ids = pipe._start_ids(self.size, None, eng.device)
            self._contexts.tensor, self._contexts.dirty = None, True
            self._negatives.tensor, self._negatives.dirty = None, True
        for r in admitted:
            self._ids[r.slot] = mask_id if r.ids0 is None else r.ids0[0].to(eng.device)
            if self.conditional:
                self._contexts.admit(r.slot, r.context.to(eng.device))
            if r.negative is not None:
                self._negatives.admit(r.slot, r.negative.to(eng.device))
        if self.active == 0:
            return []
        retiring = []
        # this step's choice temperature of every slot; None when no occupied slot has a non-zero one: the step without
        choice = [r.ctemps[r.done] if r is not None and r.ctemps else 0.0 for r in self.occupied]
        choice = choice if any(choice) else None
        for j, r in enumerate(self.occupied):
            rec = self._records[j]
            if self._guides is not None:
                # what the slot is guided against (nothing / no context / its negative context) and THIS step's scale
                on = r is not None and r.guidance_scale is not None
                kind = _lib.GUIDE_OFF if not on else _lib.GUIDE_UNCOND if r.negative is None else _lib.GUIDE_NEGATIVE
                scale = 0.0 if not on else r.scales[r.done] if r.scales else r.guidance_scale
                self._guides[j].scale, self._guides[j].on = scale, kind
            if r is None:
                rec.step = _lib.SLOT_IDLE
                continue
            t = r.done
            rec.seed, rec.image_index = r.seed & (2 ** 64 - 1), r.image_index & (2 ** 64 - 1)
            rec.temperature, rec.topk, rec.num_mask, rec.step = r.temps[t], r.topk, max(r.nmask[t], 1), t
            if t + 1 == r.timesteps:
                retiring.append(r)
        # this step's re-masking count of every slot: an edit request's own, -1 (the record's) otherwise; None when no occupied slot
        # is an edit request: the step without
        counts = None
        if any(r is not None and r.edit for r in self.occupied):
            counts = [r.nmask[r.done] if r is not None and r.edit else -1 for r in self.occupied]
        want_aux = (any(not r.edit for r in retiring) and self.decode) or self.record_steps
        ctx = self._contexts.tensor if self.conditional else None
        keep = not self._contexts.dirty
        # one length per slot -- unless every occupied slot fills the capacity, which IS the step without lengths
        lens = self._contexts.step_lens([r is not None for r in self.occupied]) if self.conditional else None

        # the negative contexts: once a request brought one, every step hands the tensor over (or keeps its K/V), so that the set
        # outlives the steps in which no occupied slot uses it; lengths like the contexts', over the slots that have a negative prompt
        neg = self._negatives.tensor
        keep_neg = neg is not None and not self._negatives.dirty
        neg_lens = None if neg is None else self._negatives.step_lens([r is not None and r.negative is not None for r in self.occupied])

        # the regional and the weighted slots' arrays -- None when no occupied slot is regional / weighted: the step without
        segments = self._segment_arrays(ctx.shape[1]) if (self.regions or self.weights) and self.conditional else None
        wts = self._weight_array(ctx.shape[1]) if self.weights and self.conditional else None

        def run(keep_context, keep_negative):
            return eng.step_slots(self._ids, ctx, self._records, use_graph=self.use_graph, keep_context=keep_context, want_aux=want_aux,
                                  guides=self._guides, context_lens=lens, choice=choice, negative_context=neg, negative_lens=neg_lens,
                                  keep_negative=keep_negative, counts=counts, segments=segments, weights=wts, **self._step_filters())
        try:
            _, pred, score = run(keep, keep_neg)
        except _lib.PmhipError as e:
            # another call on this handle (pipe.generate, a rebuilt engine ...) replaced the prepared contexts: prepare them again
            if not ((keep or keep_neg) and getattr(e, "code", None) == _lib.PMHIP_ESTATE):
                raise
            _, pred, score = run(False, False)
        self._contexts.dirty = self._negatives.dirty = False
        for r in self.occupied:
            if r is not None:
                r.done += 1
                if self.record_steps:
                    r.trace.append((pred[r.slot].clone(), score[r.slot].clone()))
        if not retiring:
            return []
        # ONE decode call for the rows that finished: the image comes from the predictions at ALL positions of the last step -- for
        # an edit request from its merged ids (its last count is 0: no mask id is left in them)
        rows = torch.tensor([r.slot for r in retiring], device=eng.device)
        ids = self._ids.index_select(0, rows)
        imgs = None
        if self.decode:
            edits = [r.edit for r in retiring]
            src = ids if all(edits) else pred.index_select(0, rows)
            if any(edits) and not all(edits):
                src = torch.where(torch.tensor(edits, device=eng.device)[:, None], ids, src)
            imgs = pipe.vqgan.engine().decode_indices(src)
        out = []
        for i, r in enumerate(retiring):
            img = imgs[i] if self.decode else None
            if img is not None and r.orig is not None:
                img = ops.composite(img[None].contiguous(), r.orig[None].to(eng.device, torch.float32).contiguous(),
                                    r.pixel_mask[None].to(eng.device).contiguous())[0]
            out.append(Finished(r, img, ids[i]))
            self._retire(r)
        return out


class FilterSession(DecodeSession):
    """``pipe.decode_session(..., filters=True)``: a DecodeSession whose requests carry the sampler filters of ``Pipeline.generate``
    -- top-k anywhere in 1..n_embed (None: no filter) and a nucleus mass top_p -- see the module docstring.  Everything else a
    request can carry works as in DecodeSession, through the same code."""

    def submit(self, text=None, timesteps=18, temperature=1.0, topk=5, seed=None, image_index=None, context=None, ids0=None,
               guidance_scale=None, choice_temperature=None, negative_text=None, negative_context=None, top_p=None, keep_given=False,
               image=None, mask=None, token_mask=None, preserve="tokens", regions=None):
        """DecodeSession.submit with `topk` in 1..n_embed, or None for no filter (stored as n_embed), and `top_p` (None or 1 = no
        nucleus filter; else finite, 0 < top_p < 1): of the request's top-k classes only those whose mass strictly above them is
        below top_p of the top-k's mass are drawn from, like ``Pipeline.generate(top_p=)``.  Out of range: ValueError, here."""
        if not self.regions:
            _no_regions(regions)
        return self._submit(text, timesteps, temperature, topk, top_p, seed, image_index, context, ids0, guidance_scale, choice_temperature,
                            negative_text, negative_context, keep_given, image, mask, token_mask, preserve, regions)

    def _filters(self, topk, top_p):
        V = self.pipe.mask_token_id                 # n_embed
        topk = V if topk is None else int(topk)
        if not 1 <= topk <= V:
            raise ValueError(f"topk must be in 1..n_embed={V} (or None: no filter), got {topk}")
        return topk, ops.nucleus_p(top_p)

    def _step_filters(self):
        # one nucleus mass per slot, also when every one is 1: the step that takes top-k up to n_embed
        return {"top_p": [1.0 if r is None else r.top_p for r in self.occupied]}
