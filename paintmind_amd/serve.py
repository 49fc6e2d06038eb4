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
top-k up to n_embed, and ``None`` for no filter, DESIGN.md section 4n, but a session does not -- a batch that mixes requests at
and above 8 needs a second sampling launch chosen step by step, which is not built), and idle slots still run through
the tower (no compaction).  For the same reason an unguided slot beside a guided one still pays the second tower pass: the
unconditional pass runs at the session's batch size.  Requests carry no negative prompt and no guidance schedule (``Pipeline.generate`` has both).

A choice temperature is per request too (``submit(choice_temperature=c)``): the request keeps MaskGIT's annealed value of each of
its steps beside its temperatures and mask counts, the native step (pmhip_pipeline_step_slots_choice) reads one value per slot
from a device array, and the contract reads ``generate_ids(..., choice_temperature=c)``.  A step in which no occupied slot has a
non-zero value passes none, which IS the step without: the same kernels and graph as before.  The guided loop's step-0 cache ("Not built") stays
not built.

On a CPU pipeline the session steps every occupied slot alone through the plain-torch step (B = 1, seed + step, like
``Pipeline.generate`` on the CPU): a request then equals ``pipe.generate([text], ..., seed=seed, guidance_scale=s)``.
"""
import collections
import math
import os

import torch

from . import _lib

Finished = collections.namedtuple("Finished", ["handle", "image", "ids"])


class Request:
    """what submit() returns: the request's parameters, its schedule and where / when it ran"""

    def __init__(self, number, text, context, timesteps, temperature, topk, seed, image_index, temps, nmask, ids0, guidance_scale=None,
                 ctemps=None):
        self.number, self.text, self.context = number, text, context
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

    def __init__(self, pipe, slots=64, conditional=True, use_graph=None, record_steps=False, decode=True, max_context_len=None):
        if slots < 1:
            raise ValueError("a decode session needs at least one slot")
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
        self._ctx = None                    # GPU, conditional: [S, capacity, context_dim] fp32, a slot's rows behind its length are 0
        self._ctx_dirty = True              # a slot's context changed since the cross K/V were prepared
        self._lens = [1] * self.size        # GPU, conditional: context rows of every slot (an idle slot keeps a valid value)
        self._records = (_lib.Slot * self.size)()
        self._guides = (_lib.SlotGuide * self.size)() if self.conditional else None

    # -- requests -----------------------------------------------------------------------------------
    def submit(self, text=None, timesteps=18, temperature=1.0, topk=5, seed=None, image_index=None, context=None, ids0=None,
               guidance_scale=None, choice_temperature=None):
        """queue one request (any time, also between steps) -> its Request.  `context` [L_r, D] may be given instead of `text`
        (a conditional session runs the pipeline's text model on `text` otherwise), with its OWN length L_r: the request attends
        to exactly these rows; `ids0` [N]: start ids instead of all-mask;
        `guidance_scale` (None = not guided): this request samples from uncond + scale * (cond - uncond), like
        ``Pipeline.generate(guidance_scale=)``; `choice_temperature` (None or 0 = the deterministic re-masking): MaskGIT's base
        choice temperature, annealed over this request's own steps like ``Pipeline.generate(choice_temperature=)``."""
        timesteps, topk = int(timesteps), int(topk)
        if guidance_scale is not None:
            if not self.conditional:
                raise ValueError("guidance_scale needs a text condition (an unconditional session IS the unconditional branch)")
            guidance_scale = float(guidance_scale)
            if not math.isfinite(guidance_scale):
                raise ValueError("guidance_scale must be finite")
        if timesteps < 1:
            raise ValueError("timesteps must be >= 1")
        if not self._cpu and not 1 <= topk <= 8:
            raise ValueError(f"a decode session serves topk in 1..8, got {topk}")
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
        from .generate import loop_schedule
        temps, nmask, ctemps = loop_schedule(timesteps, temperature, self.pipe.num_tokens, choice_temperature)
        r = Request(self._submitted, text, context, timesteps, temperature, topk, int(seed), int(image_index), temps, nmask, ids0, guidance_scale,
                    ctemps)
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
            ids, img = pipe._sample_cpu(self._rows[j], r.nmask[t], ctx, r.topk, r.temps[t], None, r.seed + t, r.guidance_scale,
                                        None, r.ctemps[t] if r.ctemps else 0.0)
            self._rows[j] = ids
            r.done = t + 1
            if r.done == r.timesteps:
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
            self._ctx, self._ctx_dirty = None, True
        for r in admitted:
            self._ids[r.slot] = mask_id if r.ids0 is None else r.ids0[0].to(eng.device)
            if self.conditional:
                c = r.context.to(eng.device)
                Lr = c.shape[0]
                if self._ctx is None:
                    self._ctx = torch.zeros(self.size, self.max_context_len or Lr, c.shape[1], device=eng.device, dtype=torch.float32)
                if c.shape[1] != self._ctx.shape[2]:
                    raise ValueError(f"every context of a session has the same width: {c.shape[1]} != {self._ctx.shape[2]}")
                if Lr > self._ctx.shape[1]:              # max_context_len None (submit checked the other case): the capacity grows
                    grown = torch.zeros(self.size, Lr, c.shape[1], device=eng.device, dtype=torch.float32)
                    grown[:, :self._ctx.shape[1]] = self._ctx
                    self._ctx = grown
                self._ctx[r.slot, :Lr] = c
                self._ctx[r.slot, Lr:] = 0
                self._lens[r.slot] = Lr
                self._ctx_dirty = True
        if self.active == 0:
            return []
        retiring = []
        # this step's choice temperature of every slot; None when no occupied slot has a non-zero one: the step without
        choice = [r.ctemps[r.done] if r is not None and r.ctemps else 0.0 for r in self.occupied]
        choice = choice if any(choice) else None
        for j, r in enumerate(self.occupied):
            rec = self._records[j]
            if self._guides is not None:
                on = r is not None and r.guidance_scale is not None
                self._guides[j].scale, self._guides[j].on = (r.guidance_scale if on else 0.0), int(on)
            if r is None:
                rec.step = _lib.SLOT_IDLE
                continue
            t = r.done
            rec.seed, rec.image_index = r.seed & (2 ** 64 - 1), r.image_index & (2 ** 64 - 1)
            rec.temperature, rec.topk, rec.num_mask, rec.step = r.temps[t], r.topk, r.nmask[t], t
            if t + 1 == r.timesteps:
                retiring.append(r)
        want_aux = (bool(retiring) and self.decode) or self.record_steps
        ctx = self._ctx if self.conditional else None
        keep = not self._ctx_dirty
        # one length per slot -- unless every occupied slot fills the capacity, which IS the step without lengths
        lens = None
        if self.conditional and any(r is not None and self._lens[j] != ctx.shape[1] for j, r in enumerate(self.occupied)):
            lens = [min(n, ctx.shape[1]) for n in self._lens]

        def run(keep_context):
            return eng.step_slots(self._ids, ctx, self._records, use_graph=self.use_graph, keep_context=keep_context, want_aux=want_aux,
                                  guides=self._guides, context_lens=lens, choice=choice)
        try:
            _, pred, score = run(keep)
        except _lib.PmhipError as e:
            # another call on this handle (pipe.generate, a rebuilt engine ...) replaced the prepared context: prepare it again
            if not (keep and getattr(e, "code", None) == _lib.PMHIP_ESTATE):
                raise
            _, pred, score = run(False)
        self._ctx_dirty = False
        for r in self.occupied:
            if r is not None:
                r.done += 1
                if self.record_steps:
                    r.trace.append((pred[r.slot].clone(), score[r.slot].clone()))
        if not retiring:
            return []
        # ONE decode call for the rows that finished: the image comes from the predictions at ALL positions of the last step
        rows = torch.tensor([r.slot for r in retiring], device=eng.device)
        imgs = pipe.vqgan.engine().decode_indices(pred.index_select(0, rows)) if self.decode else None
        ids = self._ids.index_select(0, rows)
        out = []
        for i, r in enumerate(retiring):
            out.append(Finished(r, imgs[i] if self.decode else None, ids[i]))
            self._retire(r)
        return out
