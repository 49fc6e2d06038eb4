"""Pipeline: frozen VQGAN + text tower + CondTransformer and the MaskGIT decode loop
(reference paintmind/generate.py:49-236), driven through the native engine.

Kept 1:1 with the reference: constructor wiring and parameter names, ``to_latent`` /
``tokens2logits`` / ``ids2tokens`` / ``sample`` / ``generate`` / ``inpaint`` / ``outpaint`` signatures,
return structures and the quirks listed in SURVEY.md section 8(a) (image decoded from the predictions at
ALL positions, confidence from the unfiltered softmax, >= 1 token re-masked on the last step,
``generate`` returning only the steps with ``step % save_interval == 0`` as CPU tensors).
The masked-token objective (forward / loss / random_masking, generate.py:78-146) is built forward-only: no backward.
"""
import math
import concurrent.futures
import os
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from . import ops, packing
from .canvas import canvas_grid, canvas_layout
from .config import ver2cfg
from .engine import S2Engine
from .stage2 import CondTransformer
from .steps import HipSteps, TorchSteps


def exists(x):
    return x is not None


def _draw_seed():
    """a Philox seed from the torch CPU generator: governed by torch.manual_seed like the reference's noise"""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def mask_schedule(ratio):
    """cosine schedule, evaluated in float64 like the reference (generate.py:25-26)."""
    return np.cos(math.pi / 2. * ratio)


def num_token_masked(mask_ratio, num_tokens):
    """generate.py:175 -- max(int(mask_ratio * num_tokens), 1); accepts numpy scalars, tensors, floats."""
    r = mask_ratio * num_tokens
    r = r.item() if hasattr(r, "item") else r
    return max(int(r), 1)


def edit_schedule(m, timesteps):
    """the re-masking counts of an EDIT of m tokens over T steps (``Pipeline.edit``) -> a list of T ints.
    MaskGIT's rule, counted over the region: with c_0 = m, step s < T - 1 re-masks
    n_s = max(0, min(max(int(cosine((s + 1) / T) * m), 1), c_s - 1)) and c_{s+1} = n_s; the last step re-masks 0.  At least one
    token is committed per step, nothing is left at the end, and -- n_s being below the c_s positions step s took -- a given id is
    never re-masked.  The cosine is ``mask_schedule``'s, float64."""
    out, c = [], int(m)
    for step in range(timesteps - 1):
        n = max(0, min(max(int(mask_schedule((step + 1) / timesteps) * m), 1), c - 1))
        out.append(n)
        c = n
    return out + [0]


def choice_schedule(timesteps, choice_temperature):
    """MaskGIT's annealed choice temperature: step s of T re-masks with t_s = choice_temperature * (1 - (s + 1) / T), evaluated in
    double precision and rounded to fp32 once (what the kernels take); the last step's value is exactly 0.  None or 0 -> None (the
    reference's deterministic re-masking).  The base value obeys the bound of every step's: finite, in [0, 1000]."""
    base = ops.choice_t(choice_temperature)
    if base == 0.0:
        return None
    return [float(np.float32(base * (1.0 - (step + 1) / timesteps))) for step in range(timesteps)]


def linear_guidance(timesteps, scale):
    """a guidance schedule that rises linearly to `scale`: step s of T guides with scale * (s + 1) / T -- low early for diversity,
    high late for fidelity, as Muse describes it (without naming endpoints: any list of T finite floats is a schedule for
    ``Pipeline.generate(guidance_scale=[...])``, this is one choice)"""
    return [scale * (step + 1) / timesteps for step in range(timesteps)]


def loop_schedule(timesteps, temperature, num_tokens, choice_temperature=None):
    """the per-step values of a decode loop (generate.py:187-190) -> (temps [T], nmask [T], ctemps [T] or None), evaluated in
    float64 like the reference: step s samples at temperature * (1 - s / T), re-masks num_token_masked(cosine((s + 1) / T)) tokens
    and does so with choice_schedule's value.  Every loop of this package -- native, CPU, region, session -- reads its steps here."""
    temps = [temperature * (1 - step / timesteps) for step in range(timesteps)]
    nmask = [num_token_masked(mask_schedule((step + 1) / timesteps), num_tokens) for step in range(timesteps)]
    return temps, nmask, choice_schedule(timesteps, choice_temperature)


def region_token_mask(mask, image_size, patch_size):
    """one region's mask -> bool [g * g] over the token grid (g = image_size // patch_size): a bool [g, g] token mask as it is, or
    a pixel mask [H, W] (non-zero = inside), of which a token is part iff ANY pixel of its patch is -- the rule of ``Pipeline.edit``"""
    m = torch.as_tensor(mask).cpu()
    g = image_size // patch_size
    if tuple(m.shape) == (g, g) and (m.dtype == torch.bool or g == image_size):
        return (m != 0).reshape(-1)
    if tuple(m.shape) != (image_size, image_size):
        raise ValueError(f"regions: a mask must be a bool [{g}, {g}] token mask or a [{image_size}, {image_size}] pixel mask, got "
                         f"{m.dtype} {tuple(m.shape)}")
    return ((m != 0).reshape(g, patch_size, g, patch_size).to(torch.uint8).amax(dim=(1, 3)) != 0).reshape(-1)


def diff_draws(B, N, mask_ratio, draws, seed):
    """the masks of ``Pipeline.diff_mask``'s draws -> bool [draws, B, N] on the CPU.  Every image gets ONE
    permutation, rank = argsort(argsort(torch.rand(B, N, generator=torch.Generator().manual_seed(seed)))), and with
    k = ceil(mask_ratio * N) draw j masks the positions with (rank - (j * N) // draws) mod N < k: a window of k ranks that starts
    where draw j's share of the permutation does.  0 < mask_ratio < 1, draws >= 1 and k >= ceil(N / draws) -- consecutive windows
    start at most ceil(N / draws) apart, so under the last condition every position is masked in at least one draw -- else ValueError.
    The CPU generator draws them: the CPU branch and the GPU see the same masks."""
    if isinstance(draws, bool) or not isinstance(draws, int) or draws < 1:
        raise ValueError(f"diff_draws: draws {draws!r} must be an integer >= 1")
    if isinstance(mask_ratio, bool) or not isinstance(mask_ratio, (int, float)) or not 0 < mask_ratio < 1:
        raise ValueError(f"diff_draws: mask_ratio {mask_ratio!r} must satisfy 0 < mask_ratio < 1")
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"diff_draws: seed {seed!r} must be an integer")
    if B < 1 or N < 1:
        raise ValueError(f"diff_draws: B={B} and N={N} must be positive")
    k = math.ceil(mask_ratio * N)
    if k < math.ceil(N / draws):
        raise ValueError(f"diff_draws: k = ceil(mask_ratio * N) = {k} must satisfy k >= ceil(N / draws) = {math.ceil(N / draws)}: with fewer "
                         f"some position is masked in no draw (raise mask_ratio or draws)")
    rank = torch.argsort(torch.argsort(torch.rand(B, N, generator=torch.Generator().manual_seed(seed)), dim=1), dim=1)
    starts = torch.tensor([(j * N) // draws for j in range(draws)], dtype=rank.dtype)
    return (rank[None] - starts[:, None, None]) % N < k


# ``generate``'s keywords that ``generate_canvas`` refuses by name (a ValueError; any other unknown keyword is a TypeError)
CANVAS_UNSERVED = ("regions", "prompt_weights", "context_weights", "context_segments", "token_segments", "context_lens", "negative_context_lens")

MAX_REGIONS = 31           # segments 1..31 beside the global prompt's segment 0: one bit each of a token's 32-bit mask


def region_layout(contexts, masks, image_size, patch_size):
    """The concatenated context of regional prompts and its two arrays.  contexts: per image a list of [L_r, D] tensors, the global
    prompt's rows first, then every region's; masks: per image the regions' masks (one fewer than contexts).
    -> (context fp32 [B, Lmax, D], zero-filled behind an image's rows; numpy uint8 [B, Lmax], the segment of every row, 255 = padding;
    numpy uint32 [B, N], bit 0 | bit r for every region r the token is part of)"""
    B = len(contexts)
    g = image_size // patch_size
    totals = [sum(c.shape[0] for c in cs) for cs in contexts]
    Lmax, D = max(totals), contexts[0][0].shape[1]
    context = torch.zeros(B, Lmax, D, dtype=torch.float32)
    ctx_seg = np.full((B, Lmax), 255, np.uint8)
    tok_seg = np.ones((B, g * g), np.uint32)
    for b in range(B):
        if len(masks[b]) != len(contexts[b]) - 1:
            raise ValueError(f"regions: image {b}: {len(masks[b])} masks for {len(contexts[b]) - 1} region prompts")
        if len(masks[b]) > MAX_REGIONS:
            raise ValueError(f"regions: image {b}: {len(masks[b])} regions, at most {MAX_REGIONS} per image")
        at = 0
        for r, c in enumerate(contexts[b]):
            context[b, at:at + c.shape[0]] = c.detach().to("cpu", torch.float32)
            ctx_seg[b, at:at + c.shape[0]] = r
            at += c.shape[0]
        for r, m in enumerate(masks[b], start=1):
            tok_seg[b] |= region_token_mask(m, image_size, patch_size).numpy().astype(np.uint32) << np.uint32(r)
    return context, ctx_seg, tok_seg


class _Options(NamedTuple):
    """the sampler options of one public call, checked once (Pipeline._options): topk an integer (None resolved to n_embed), top_p a
    float (1.0 = no nucleus filter), guidance_scale a number or None, lens the per-image context lengths as the caller gave them
    (a host list or None; ``Pipeline._keys`` is their one reader: behind it the call's ``ops.Keys`` says what is attended to),
    choice_temperature the base value as a float (0.0 = the deterministic re-masking), negative the negative context [B, Ln, D] or
    None with negative_lens its per-image lengths as a host list or None, guidance_scales the loop's per-step scales as a list of
    floats or None (then guidance_scale is every step's)"""
    topk: int
    top_p: float
    guidance_scale: Optional[float]
    lens: Optional[list]
    choice_temperature: float
    negative: Optional[torch.Tensor] = None
    negative_lens: Optional[list] = None
    guidance_scales: Optional[list] = None

    def lane(self, lo, hi):
        """the options of the micro-batch of images [lo, hi): everything is per batch except the negative context (the call's
        ``ops.Keys`` has a ``lane`` of its own)"""
        if self.negative is None:
            return self
        return self._replace(negative=self.negative[lo:hi].contiguous(),
                             negative_lens=None if self.negative_lens is None else self.negative_lens[lo:hi])

    def step_scale(self, step):
        """the guidance scale of step `step` of a loop (None: no guidance)"""
        return self.guidance_scale if self.guidance_scales is None else self.guidance_scales[step]


def choice_keys(scores, t, u):
    """the re-masking keys of the plain-torch branch, fp32: a given position (score < 0) keeps its score, a taken one gets
    -(log(max(1 - score, 2^-24)) + t * gumbel(u)) -- DESIGN.md section 4m; the largest keys are re-masked"""
    conf = torch.log((1.0 - scores).clamp(min=2.0 ** -24))
    gumbel = -torch.log((-torch.log(u.clamp(min=1e-20))).clamp(min=1e-20))
    return torch.where(scores < 0, scores, -(conf + torch.tensor(t, dtype=scores.dtype) * gumbel))


def nucleus_keep(val, top_p):
    """the nucleus rule of the plain-torch branch on the top-k VALUES val [..., k], sorted descending as
    torch.topk returns them -> bool [..., k]: with w = exp(val - max), Z = sum w and P = top_p * Z an element is kept iff the
    mass of the elements whose weight is strictly above its own is below P -- a plateau of equal weights whole or not at all, the
    maximum always, a weight of 0 never.  float64: the kernels' fp32 sums decide elements within 1e-4 Z of P on their own."""
    w = torch.exp((val - val[..., :1]).double())
    c = w.cumsum(-1)
    before = c - w                                          # the mass in front of every element
    start = torch.ones_like(w, dtype=torch.bool)
    start[..., 1:] = w[..., 1:] != w[..., :-1]
    above = torch.where(start, before, torch.zeros_like(before)).cummax(-1).values     # ... in front of its plateau
    return (above < top_p * c[..., -1:]) & (w > 0)


class _PinnedPool:
    """Pinned host buffers for the images generate() returns.  Page-locking a fresh 400 MB allocation costs ~35 ms (more
    than the copies themselves), so buffers are kept and handed out again -- but only once nothing the caller received
    still aliases them: every returned tensor (and any view / numpy alias of it) holds a reference to the buffer's
    storage, so a use count of 2 (the pool's tensor + the probe) means the earlier results are gone.  Results a caller
    keeps stay valid for ever; their buffer simply leaves the pool."""
    MAX_KEPT = 4

    def __init__(self):
        self.bufs = []

    @staticmethod
    def _free(t):
        # private torch API; without it a buffer is never handed out twice (every call page-locks a fresh one: slower, safe)
        use_count = getattr(torch._C, "_storage_Use_Count", None)
        if use_count is None:
            return False
        try:
            return use_count(t.untyped_storage()._cdata) <= 2
        except Exception:
            return False

    def discard(self, t):
        """forget a buffer whose contents may still be written by copies in flight (a lane failed): it is never reused"""
        self.bufs = [b for b in self.bufs if b.untyped_storage().data_ptr() != t.untyped_storage().data_ptr()]

    def get(self, shape):
        n = 1
        for d in shape:
            n *= int(d)
        for t in self.bufs:
            if t.numel() == n and self._free(t):
                return t.view(shape)
        t = torch.empty(n, dtype=torch.float32, pin_memory=True)
        self.bufs = [b for b in self.bufs if not (self._free(b) and b.numel() != n)][-(self.MAX_KEPT - 1):] + [t]
        return t.view(shape)


_pinned_pool = _PinnedPool()
_lane_threads = None


def _lane_thread_pool(n):
    """process-wide worker threads that drive concurrent micro-batch lanes (kept out of the Module: it stays copyable)"""
    global _lane_threads
    if _lane_threads is None or _lane_threads._max_workers < n:
        from concurrent.futures import ThreadPoolExecutor
        _lane_threads = ThreadPoolExecutor(max_workers=max(n, 2), thread_name_prefix="pm-lane")
    return _lane_threads


T5_VERSION = {'t5-l': 'google/flan-t5-large', 't5-xl': 'google/flan-t5-xl', 't5-xxl': 'google/flan-t5-xxl'}
T5_TXT_DIM = {'t5-l': 1024, 't5-xl': 2048}      # no 't5-xxl' entry, as in the reference (generate.py:53)


# generate(): smallest B * tokens * width that runs as two concurrent micro-batch lanes by default (bf16).  Below it ONE lane, whose
# per-step decode is deferred beside the next step's tower, is faster; measured crossovers (tools/small_batch_lanes_ab.py,
# profiles/r05_g_*): d512 between 32 and 36 images, d768 between 20 and 22, d1024 between 16 and 20 -- 16-19 M in this unit.
LANES_MIN_WORK = 17_000_000


class TokenScores(NamedTuple):
    """``Pipeline.token_scores``: three f32 [B, g, g] maps of an image's tokens under a caption"""
    logp: torch.Tensor        # mean over the draws that masked the token of log p(true id | the unmasked rest, text): <= 0
    entropy: torch.Tensor     # ... of the entropy of the model's distribution at the token: >= 0
    rank: torch.Tensor        # ... of the true id's place in the samplers' order: < k iff topk = k would have kept it


def best_index(scores):
    """the winner of ``Pipeline.best_of`` per prompt: scores f32 [B, n] -> int64 [B], the arg-max with ties to the lowest j; a NaN
    never beats a number (a row of NaN only: 0)"""
    s = torch.where(torch.isnan(scores), torch.full_like(scores, float("-inf")), scores)
    cols = torch.arange(s.shape[1], device=s.device).expand_as(s)
    return torch.where(s == s.amax(dim=1, keepdim=True), cols, torch.full_like(cols, s.shape[1])).amin(dim=1)


def _check_region(who, threshold, grow, bools=False, prefix=""):
    """the two numbers of a region rule for caller `who`: a threshold in (0, 1] and a non-negative dilation count.  bools: True and
    False pass as the numbers 1 and 0 (``phrase_mask`` and ``control_ids`` have always let them; the later callers refuse them)"""
    if not (isinstance(threshold, (int, float)) and (bools or not isinstance(threshold, bool)) and 0 < threshold <= 1):
        raise ValueError(f"{who}: {prefix}threshold {threshold!r} must be in (0, 1]")
    if not (isinstance(grow, int) and (bools or not isinstance(grow, bool)) and grow >= 0):
        raise ValueError(f"{who}: {prefix}grow {grow!r} must be a non-negative integer")


def _no_schedule(who, guidance_scale):
    """the eager pair and forced loops guide every step alike: anything with a dimension is refused"""
    if guidance_scale is not None and np.ndim(guidance_scale) > 0:
        raise ValueError(f"{who}: guidance_scale is one number (a schedule is not served)")


def _finite_number(who, name, x, why=""):
    """the scale of a scoring pass: None, or one finite int or float (no bool)"""
    if x is not None and (isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x)):
        raise ValueError(f"{who}: {name} {x!r} must be one finite number{why}")


class Pipeline(nn.Module):
    def __init__(self, config, stage1_pretrained=True, stage1_checkpoint_path=None, text_model=None):
        super().__init__()
        from .factory import create_model
        self.vqgan = create_model(arch='vqgan', version=config.stage1, pretrained=stage1_pretrained,
                                  checkpoint_path=stage1_checkpoint_path)
        self.vqgan.freeze()

        context_dim = getattr(config, "context_dim", None) or T5_TXT_DIM[config.t5]
        if text_model is not None:
            self.text_model = text_model
        elif getattr(config, "text_model", "t5") == "none":
            from .modules.encoder import SyntheticTextEmbedder
            self.text_model = SyntheticTextEmbedder(context_dim)
        else:
            from .modules.encoder import T5TextEmbedder
            self.text_model = T5TextEmbedder(version=T5_VERSION[config.t5], freeze=True)

        vq_cfg = ver2cfg[config.stage1]
        self.image_size = vq_cfg['enc']['image_size']
        self.patch_size = vq_cfg['enc']['patch_size']
        self.num_tokens = (self.image_size // self.patch_size) ** 2
        self._width = config.dim

        self.transformer = CondTransformer(
            vq_cfg['embed_dim'], config.dim, self.num_tokens, config.dim_head, config.mlp_dim,
            config.num_head, config.depth, config.dropout, context_dim, vq_cfg['n_embed'],
        )
        self.mask_token = nn.Parameter(torch.zeros(1, vq_cfg['embed_dim']))
        self.mask_token_id = vq_cfg['n_embed']
        nn.init.normal_(self.mask_token, std=.02)
        self._pm_dtype = torch.float32
        self._engine = None

    @property
    def image_shape(self):
        """(C, H, W) of the images this pipeline returns (used by dist.generate_sharded for ranks with an empty shard)"""
        return (self.vqgan.encoder.to_patch_embedding[0].in_channels, self.image_size, self.image_size)

    # -- precision / engines ------------------------------------------------------------------------
    def set_compute_dtype(self, dtype):
        self.vqgan.set_compute_dtype(dtype)
        for m in self.transformer.modules():
            m._pm_dtype = dtype
        self.text_model._pm_dtype = dtype           # read by T5TextEmbedder / CLIPTextEmbedder(native=True) only: inert otherwise
        self._pm_dtype = dtype
        return self

    @property
    def compute_dtype(self):
        if torch.is_autocast_enabled('cuda') and torch.get_autocast_dtype('cuda') == torch.bfloat16:
            return torch.bfloat16
        return self._pm_dtype

    def engine(self):
        """native stage-2 handle for the current compute dtype; one cached per dtype, rebuilt when a parameter's
        (data_ptr, version) changes.  After edits through `p.data` call invalidate_engines()."""
        dtype = self.compute_dtype
        cb = self.vqgan.quantize.embedding.weight
        stamp = (packing.params_fingerprint(self.transformer), cb.data_ptr(), cb._version, self.mask_token.data_ptr(),
                 self.mask_token._version)
        cache = self._engine if isinstance(self._engine, dict) else {}
        hit = cache.get(dtype)
        if hit is None or hit[0] != stamp:
            cache[dtype] = hit = (stamp, S2Engine(self.transformer, cb, self.mask_token, dtype))
            self._engine = cache
        return hit[1]

    def invalidate_engines(self):
        """drop every packed weight copy / captured graph of this pipeline and its VQGAN"""
        self._engine = None
        self._lane_cache = None
        self._copy_streams = None
        self.vqgan.invalidate_engines()

    def from_pretrained(self, path):
        return self.load_state_dict(torch.load(path, map_location="cpu"))

    # -- masked-token objective, forward only (generate.py:78-146) ---------------------------------
    # The HIP path has no backward: these return tensors without a grad_fn, for validation loss and
    # for checking a training run's forward numerics.  Optimisation stays with the reference trainer.
    @torch.no_grad()
    def random_masking(self, x, mask_ratio, noise=None):
        """(x [B,L,D], ratio) -> (x with masked positions replaced by mask_token, mask [B,L], 1 = masked)
        (generate.py:78-110).  `noise` [B,L]: the uniforms the reference draws at :89 (default: torch.rand)."""
        B, L, _ = x.shape
        len_keep = L - max(int(L * mask_ratio), 1)
        if noise is None:
            noise = torch.rand(B, L, device=x.device)
        return ops.random_mask(x.float().contiguous(), noise.float().contiguous(),
                               self.mask_token.data.float().reshape(-1).contiguous(), len_keep)

    @torch.no_grad()
    def loss(self, logit, label, masks):
        """label-smoothed (0.1) cross entropy averaged over the masked positions (generate.py:112-125)"""
        V = logit.shape[-1]
        out, _ = ops.masked_ce(logit.float().reshape(-1, V).contiguous(), label.reshape(-1).contiguous(),
                               masks.float().reshape(-1).contiguous(), 0.1)
        return out.reshape(())

    @torch.no_grad()
    def forward(self, img, text=None, mask_ratio=0.75, noise=None):
        """generate.py:136-146: encode -> random masking -> stage-2 logits -> masked cross entropy"""
        x, ids, text = self.to_latent(img, text)
        x, mask = self.random_masking(x, mask_ratio, noise)
        return self.loss(self.tokens2logits(x, text), ids, mask)

    # -- inference API ------------------------------------------------------------------------------
    @torch.no_grad()
    def to_latent(self, img, text=None):
        x, _, indices = self.vqgan.encode(img)
        if exists(text):
            text = self.text_model(text)
        return x, indices, text

    def _on_cpu(self):
        return self.mask_token.device.type == "cpu"

    def _steps(self):
        """the step vocabulary of the eager flows (paintmind_amd/steps.py) for where this pipeline lives: their one device test"""
        return TorchSteps(self) if self._on_cpu() else HipSteps(self)

    def _check_img(self, who, img, B=None):
        """an image batch [B, C, size, size] of this pipeline, for caller `who`; B: one image per prompt"""
        size = self.image_size
        if not isinstance(img, torch.Tensor) or img.dim() != 4 or B not in (None, img.shape[0]) or img.shape[2] != size or img.shape[3] != size:
            raise ValueError(f"{who}: img must be [{'B' if B is None else B}, C, {size}, {size}]{'' if B is None else ' (one image per prompt)'}, got "
                             f"{tuple(img.shape) if isinstance(img, torch.Tensor) else type(img).__name__}")

    @staticmethod
    def _score_mask(st, s, g, threshold, grow):
        """a mask from ONE score f32 [B, g*g]: the region rule on it (``ops.phrase_region`` / ``_region_cpu`` through the vocabulary's
        ``region``) -> bool [B, g*g]; an image whose maximum is exactly 0 gets an EMPTY mask (>= 0 would select everything)"""
        return (st.region(s, s, g, threshold, grow) != 0) & (s.amax(dim=1, keepdim=True) > 0)

    def _topk(self, topk):
        """topk=None is 'no filter' (the plain MaskGIT / Muse sampler): every class is kept, topk = n_embed -- on the CPU and
        on the GPU branch alike.  An integer passes through unchecked: the step itself refuses what is out of 1..n_embed."""
        return self.mask_token_id if topk is None else topk

    def _options(self, topk, top_p, guidance_scale, context_lens, choice_temperature, context, B, negative=None, negative_lens=None,
                 timesteps=None):
        """the keywords of a public call -> its _Options, every value checked here and nowhere behind: the choice temperature and
        the nucleus mass (their ranges), guidance and context lengths (both need the context [B, L, D] they are about), the
        negative context [B, Ln, D] (needs guidance) and its lengths (need it).  guidance_scale: a number, or -- in a loop, which
        says so by its `timesteps` -- a sequence of that many finite numbers, one per step.  A caller that holds the record
        already passes it as `topk` and leaves the other keywords at None: it comes back as it is."""
        if isinstance(topk, _Options):
            return topk
        base = ops.choice_t(choice_temperature)
        top_p = ops.nucleus_p(top_p)
        if guidance_scale is not None and context is None:
            raise ValueError("guidance_scale needs a text condition (text=None IS the unconditional branch)")
        guidance_scale, scales = ops.guidance_parts(guidance_scale, timesteps)
        if negative_lens is not None and negative is None:
            raise ValueError("negative_context_lens needs a negative text")
        if negative is not None:
            if context is None:
                raise ValueError("negative_text needs a text condition (text=None IS the unconditional branch)")
            if guidance_scale is None and scales is None:
                raise ValueError("negative_text needs guidance_scale (the step moves away from it by that much)")
            if negative.dim() != 3 or negative.shape[0] != B or negative.shape[2] != context.shape[2]:
                raise ValueError(f"negative_text must be a context tensor [{B}, Ln, {context.shape[2]}], got {tuple(negative.shape)}")
            negative_lens = ops.host_lens(negative_lens, B, negative.shape[1], "negative_context_lens")
        lens = self._host_keys(context, B, context_lens).lens
        return _Options(self._topk(topk), top_p, guidance_scale, lens, base, negative, negative_lens, scales)

    def _host_keys(self, context, B, context_lens=None, context_segments=None, token_segments=None, context_weights=None, keys=None):
        """``ops.host_keys`` (which has the rules) for a context [B, L, D] or None of this pipeline, in the words of its callers"""
        return ops.host_keys(B, 0 if context is None else context.shape[1], self.num_tokens, context_lens, context_segments,
                             token_segments, context_weights, has_context=context is not None, keys=keys,
                             missing="a text condition (text=None IS the unconditional branch)")

    def _keys(self, context, B, opts, context_segments=None, token_segments=None, context_weights=None):
        """the ``ops.Keys`` of a call that has its ``_Options``: opts.lens -- read here and nowhere else -- with the segment and weight
        arrays of the call beside them, brought to the host and checked ONCE per public call, here"""
        return self._host_keys(context, B, opts.lens, context_segments, token_segments, context_weights)

    def tokens2logits(self, token, text=None, context_lens=None, context_segments=None, token_segments=None, context_weights=None):
        """context_lens (extension; None = the reference's behaviour, every row of the context is attended to): one length per
        image -- rows [len_b, L) of image b's context never reach its logits, NaN included.

        context_segments [B, L] ints + token_segments [B, N] int bitmasks (extension, REGIONAL PROMPTS; never
        beside context_lens): row k of image b's context belongs to segment context_segments[b, k] in 0..31 (-1 or 255: padding,
        which never reaches the logits, NaN included), and token t attends to exactly the rows whose segment is a set bit of
        token_segments[b, t].  Every token must allow a segment that is present in its image.  ``generate(regions=)`` builds both
        from prompts and masks.

        context_weights [B, L] (extension, PROMPT WEIGHTS; beside the two segment arrays, beside context_lens,
        or alone): how much a context row counts -- over the rows a token attends to, p = w exp(s) / sum w exp(s).  1 is the row as
        without weights, an integer n the row repeated n times, 0 a padding row; otherwise 2^-20 <= w <= 2^20.  Every token must
        allow a row with a weight above 0.  ``generate(prompt_weights=True)`` reads them from ``(words:1.3)`` in the prompts."""
        return self._logits(token, text, self._host_keys(text, token.shape[0], context_lens, context_segments, token_segments, context_weights))

    def _logits(self, token, text, keys=None):
        """``tokens2logits`` behind its checks; keys None: every row of the context is attended to"""
        if self._on_cpu():
            return self.transformer(token, text, keys=keys)   # plain-torch operators of this package (no HIP engine on the CPU)
        return self.engine().forward(token, text, keys=keys)

    @torch.no_grad()
    def attention_maps(self, ids=None, text=None, layers=None, context_lens=None, mask_padding=False, context_segments=None,
                       token_segments=None, context_weights=None, return_logits=False, img=None):
        """CROSS-ATTENTION MAPS (extension): which tokens of the picture look at which rows of the prompt.

        ``ids``: int64 [B, N] token ids, the mask id allowed (what a decode loop holds at some step); or ``img=`` [B, C, H, W]
        instead, which is encoded first, as ``to_latent`` does.  ``text``: a list of prompts or a context tensor [B, L, D].
        ``layers``: the layer indices to average over (None: all).  ``context_lens`` / ``mask_padding``, ``context_segments`` +
        ``token_segments`` and ``context_weights``: as in ``tokens2logits`` / ``generate`` -- the maps are those of the very
        softmax these select, and a context row that takes no part (padding, a denied segment, weight 0) is exactly 0.

        -> f32 [B, L, g, g] on the pipeline's device: map [b, r] is where row r of image b's context is looked at -- the mean over
        the chosen layers and over the heads of the cross-attention probabilities, so over r a token's values sum to 1.  With
        ``return_logits`` (maps, logits [B, N, n_embed]), the logits being ``tokens2logits``' on the same arguments, bit for bit.
        One eager forward: nothing is captured, and a later call of anything runs what it ran before."""
        if (ids is None) == (img is None):
            raise ValueError("attention_maps: give exactly one of ids and img")
        if text is None:
            raise ValueError("attention_maps: the maps are those of the cross-attention: a text condition is required")
        if img is not None:
            _, ids, _ = self.to_latent(img)
        B = ids.shape[0]
        ids = ids.reshape(B, self.num_tokens)
        if isinstance(text, torch.Tensor):
            context = text
        elif mask_padding and context_lens is None:
            context, context_lens = self.text_model(list(text), return_lens=True)
        else:
            context = self.text_model(list(text))
        depth = len(self.transformer.layers)
        chosen = ops.host_layers(range(depth) if layers is None else layers, depth, "attention_maps: layers")
        keys = self._host_keys(context, B, context_lens, context_segments, token_segments, context_weights)
        g = self.image_size // self.patch_size
        if self._on_cpu():
            logits, maps = self.transformer(self.ids2tokens(ids), context, maps_layers=chosen, keys=keys)
        else:
            eng = self.engine()
            token = self.ids2tokens(ids.to(eng.device))
            logits, maps = eng.forward_maps(token, context.to(eng.device), chosen, keys=keys)
        maps = maps.transpose(1, 2).reshape(B, context.shape[1], g, g).contiguous()
        return (maps, logits) if return_logits else maps

    @torch.no_grad()
    def phrase_mask(self, img, text, phrase, threshold=0.5, layers=None, grow=0):
        """An edit mask from a PHRASE of the prompt (extension): the tokens of ``img`` that look at the phrase.

        ``text``: the prompts, ``phrase``: one phrase for all or one per prompt, each occurring exactly once in its prompt
        (``T5TextEmbedder.phrase_rows``; other text towers raise NotImplementedError).  The rule, which is the contract:
            score[b, t] = the sum over the phrase's context rows of ``attention_maps(img=img, ...)``, run under the non-pad lengths
                          as ``mask_padding=True`` does
            mask        = score >= threshold * max_t score[b],   0 < threshold <= 1
        then dilated ``grow`` times by a 3 x 3 maximum.  The default threshold 0.5 is a default, not a measured optimum: look at
        the maps and choose.  -> bool [B, g, g] on the pipeline's device: what ``edit(token_mask=)`` takes."""
        _check_region("phrase_mask", threshold, grow, bools=True)
        if not hasattr(self.text_model, "phrase_rows"):
            raise NotImplementedError(f"{type(self.text_model).__name__} serves no phrase rows (phrase_rows): T5TextEmbedder does")
        prompts = [text] * img.shape[0] if isinstance(text, str) else list(text)
        if len(prompts) != img.shape[0]:
            raise ValueError(f"phrase_mask: {len(prompts)} prompts for a batch of {img.shape[0]}")
        context, lens, rows = self.text_model.phrase_rows(prompts, phrase)
        maps = self.attention_maps(img=img, text=context, layers=layers, context_lens=lens)      # [B, L, g, g]
        score = (maps * rows.to(maps.device)[:, :, None, None].to(maps.dtype)).sum(1)             # [B, g, g]
        mask = score >= threshold * score.amax(dim=(1, 2), keepdim=True)
        for _ in range(grow):
            mask = torch.nn.functional.max_pool2d(mask[:, None].float(), 3, stride=1, padding=1)[:, 0] > 0
        return mask

    @staticmethod
    def _divergence_cpu(la, lb, kind):
        """``ops.logit_divergence`` on every row in plain torch, float32 with log_softmax: logits [..., V] twice -> f32 [...]"""
        lp, lq = torch.log_softmax(la.float(), dim=-1), torch.log_softmax(lb.float(), dim=-1)
        dp = lp.exp() - lq.exp()
        if kind == "tv":
            return 0.5 * dp.abs().sum(-1)
        gone_p, gone_q = lp == float("-inf"), lq == float("-inf")
        t = torch.where(gone_p & gone_q, torch.zeros_like(dp), dp * (lp - lq))         # -inf in both: nothing; in one: +inf
        return torch.where(gone_p != gone_q, torch.full_like(dp, float("inf")), t).sum(-1)

    def _diff_context(self, text, B, mask_padding, lens, who, caller="diff_mask"):
        """one side of ``diff_mask`` (or the caption of `caller`): a list of B prompts, one prompt for every image, or a context tensor
        [B, L, D] -> (context, lens)"""
        if isinstance(text, torch.Tensor):
            if text.dim() != 3 or text.shape[0] != B:
                raise ValueError(f"{caller}: {who} must be a context tensor [{B}, L, D], got {tuple(text.shape)}")
            if mask_padding:
                raise ValueError(f"{caller}: mask_padding takes the lengths from the text model: {who} is a tensor, pass its lengths")
            return text, lens
        if getattr(self, "text_model", None) is None:
            raise ValueError(f"{caller} needs a text condition (an unconditional pipeline has no prompt to disagree about)")
        if isinstance(text, str):
            prompts = [text] * B
        elif isinstance(text, (list, tuple)) and all(isinstance(p, str) for p in text):
            prompts = list(text)
        else:
            raise ValueError(f"{caller}: {who} must be a prompt, a list of {B} prompts or a context tensor, got {type(text).__name__}")
        if len(prompts) != B:
            raise ValueError(f"{caller}: {who} has {len(prompts)} prompts for a batch of {B}")
        if mask_padding and lens is None:
            return self.text_model(prompts, return_lens=True)
        return self.text_model(prompts), lens

    @torch.no_grad()
    def diff_mask(self, img, text, edit_text, mask_ratio=0.5, draws=4, seed=0, kind="tv", threshold=0.5, grow=1, mask_padding=False,
                  context_lens=None, edit_context_lens=None, return_score=False, **refused):
        """An edit mask from where TWO PROMPTS DISAGREE about ``img`` (extension; DiffEdit's idea on a
        masked-token model): no phrase, no drawn mask.  ``text`` is the image's caption, ``edit_text`` what it should become: each a
        list of B prompts, one prompt for every image, or a context tensor [B, L, D]; the two contexts must have one shape.  With
        ``mask_padding`` the non-pad lengths come from the text model; ``context_lens`` / ``edit_context_lens`` give them per side.

        The rule, which is the contract:
            1. ids = to_latent(img)
            2. for draw j of ``draws``: m = diff_draws(B, N, mask_ratio, draws, seed)[j]; the ids with the mask id where m is set go
               through ONE forward of 2 B images -- the same masked ids twice, under the contexts cat[text, edit_text] -- and every
               masked position t of image b adds  d(softmax(logits_text[b, t]), softmax(logits_edit[b, t]))  to acc[b, t] and 1 to
               count[b, t]; d is ``kind``: "tv" = 1/2 sum |p - q| in [0, 1], "jeffreys" = KL(p||q) + KL(q||p)
            3. score = acc / count                  (count >= 1 everywhere: ``diff_draws`` guarantees it)
            4. mask  = score >= threshold * max_t score[b],   0 < threshold <= 1,   dilated ``grow`` times by a 3 x 3 maximum;
               an image whose maximum score is exactly 0 -- the two prompts are the same text -- gets an EMPTY mask
        On the GPU step 2's divergence is one HBM-bound kernel over the two halves of the logits (``ops.logit_divergence``) and step 4
        the region kernel of the local blend (``ops.phrase_region``); on the CPU the same rule in plain torch.  The logits of a draw
        take 2 B * N * n_embed * 4 bytes (B = 32 on the 8192-code tower: 2 GiB); a larger batch is the caller's to split.

        The defaults 0.5 / 4 / 0.5 / 1 follow DiffEdit's spirit (half the image corrupted, a few draws, half the maximum, one
        dilation); they are not optima measured on this tower, whose image quality is unmeasured.  Not served (ValueError):
        guidance or a negative prompt in the divergence passes, the segment arrays, prompt weights.

        -> bool [B, g, g] on the pipeline's device: what ``edit(token_mask=)`` and ``prompt_to_prompt(blend_mask=)`` take; with
        ``return_score`` (mask, score f32 [B, g, g]).  Nothing is captured: a later call of anything runs what it ran before."""
        if refused:
            raise ValueError(f"diff_mask does not serve {sorted(refused)} (guidance, negative prompts, the segment arrays and prompt weights "
                             f"take no part in the divergence passes)")
        _check_region("diff_mask", threshold, grow)
        if kind not in ops.DIVERGENCE_KINDS:
            raise ValueError(f"diff_mask: kind {kind!r} is neither 'tv' nor 'jeffreys'")
        self._check_img("diff_mask", img)
        if text is None or edit_text is None:
            raise ValueError("diff_mask needs a text condition on both sides (the caption and what it should become)")
        B, N, V = img.shape[0], self.num_tokens, self.mask_token_id
        g = self.image_size // self.patch_size
        masks = diff_draws(B, N, mask_ratio, draws, seed)
        ctx_src, lens_src = self._diff_context(text, B, mask_padding, context_lens, "text")
        ctx_edit, lens_edit = self._diff_context(edit_text, B, mask_padding, edit_context_lens, "edit_text")
        if ctx_src.shape != ctx_edit.shape:
            raise ValueError(f"diff_mask: the two contexts must have one shape, got {tuple(ctx_src.shape)} and {tuple(ctx_edit.shape)}")
        L = ctx_src.shape[1]
        lens = None
        if lens_src is not None or lens_edit is not None:
            lens = (ops.host_lens([L] * B if lens_src is None else lens_src, B, L, "context_lens") +
                    ops.host_lens([L] * B if lens_edit is None else lens_edit, B, L, "edit_context_lens"))
        st = self._steps()
        ids = st.ids(self.to_latent(img)[1].reshape(B, N))
        context = st.context(torch.cat((ctx_src.to(st.device), ctx_edit.to(st.device))).float())
        keys = self._host_keys(context, 2 * B, lens)
        acc = st.divergence_start(B, N)
        for m in masks:
            m = m.to(st.device)
            masked = torch.where(m, torch.full_like(ids, V), ids)
            st.divergence_add(acc, st.forward(self.ids2tokens(torch.cat((masked, masked))), context, keys), m, masked, kind)
        score = st.divergence_finish(acc)
        mask = self._score_mask(st, score, g, threshold, grow).reshape(B, g, g)
        return (mask, score.reshape(B, g, g)) if return_score else mask

    # ------------------------------------------------------------------------------------------------ model likelihood (section 4zg)
    @staticmethod
    def _token_logprob_cpu(x, target):
        """``ops.token_logprob`` on every row in plain torch, float32, by the kernel's expressions (torch's own sums, exp and log):
        logits [..., V], target int64 [...] -> (logp, entropy f32, rank int64)"""
        x = x.float()
        t = target[..., None]
        d = x - x.amax(dim=-1, keepdim=True)
        e = d.exp()
        s = e.sum(-1)
        L = s.log()
        ent = L + torch.where(e == 0, torch.zeros_like(e), e * -d).sum(-1) / s           # (a -inf column: 0 * inf through a select)
        xt = x.gather(-1, t)
        cols = torch.arange(x.shape[-1], device=x.device)
        rank = ((x > xt) | ((x == xt) & (cols < t))).sum(-1)
        return d.gather(-1, t)[..., 0] - L, ent, rank

    def _score_args(self, who, img, ids, text, mask_padding, context_lens, guidance_scale, refused):
        """what ``token_scores`` / ``score`` check: -> (ids int64 [B, N], context or None, lens or None, the scale or None)"""
        if refused:
            raise ValueError(f"{who} does not serve {sorted(refused)} (the segment arrays, prompt weights, negative prompts and a guidance "
                             f"schedule take no part in the scoring passes)")
        if (ids is None) == (img is None):
            raise ValueError(f"{who}: give exactly one of img and ids")
        N = self.num_tokens
        if img is not None:
            self._check_img(who, img)
            ids = self.to_latent(img)[1].reshape(img.shape[0], N)
        else:
            if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.dim() < 2 or ids[0].numel() != N:
                raise ValueError(f"{who}: ids must be an int64 tensor [B, {N}] or [B, g, g], got "
                                 f"{(ids.dtype, tuple(ids.shape)) if isinstance(ids, torch.Tensor) else type(ids).__name__}")
            ids = ids.reshape(ids.shape[0], N)
            bad = ((ids < 0) | (ids > self.mask_token_id)).nonzero()
            if len(bad):
                b, i = bad[0].tolist()
                raise ValueError(f"{who}: ids: image {b}, token {i}: {int(ids[b, i])} is neither a code nor the mask id {self.mask_token_id}")
        B = ids.shape[0]
        if guidance_scale is not None:
            _finite_number(who, "guidance_scale", guidance_scale, " (a schedule belongs to a decode loop)")
            if text is None:
                raise ValueError(f"{who}: guidance_scale needs a text condition (text=None IS the unconditional branch)")
        if text is None:
            if mask_padding or context_lens is not None:
                raise ValueError(f"{who}: mask_padding and context_lens need a text condition")
            return ids, None, None, None
        context, lens = self._diff_context(text, B, mask_padding, context_lens, "text", who)
        return ids, context, lens, None if guidance_scale is None else float(guidance_scale)

    def _token_scores(self, ids, context, lens, masks, scale):
        """the rule of ``token_scores`` behind its checks: ids int64 [B, N], masks bool [draws, B, N] (CPU) -> (logp, entropy, rank) f32
        [B, N] on the pipeline's device, each acc / count (NaN = 0 / 0 where the id is the mask id: such a position is never scored)"""
        B, V = ids.shape[0], self.mask_token_id
        st = self._steps()
        ids, context = st.ids(ids), st.context(None if context is None else context.float())
        keys, nokeys = self._host_keys(context, B, lens), self._host_keys(None, B)
        acc = st.logprob_start(ids)
        for m in masks:
            m = m.to(st.device)
            masked = torch.where(m, torch.full_like(ids, V), ids)
            tok = self.ids2tokens(masked)
            x = st.forward(tok, context, keys)
            st.logprob_add(acc, x, None if scale is None else st.forward(tok, None, nokeys), scale, m, masked)
        return st.logprob_finish(acc)

    @torch.no_grad()
    def token_scores(self, img=None, text=None, *, ids=None, mask_ratio=0.5, draws=4, seed=0, guidance_scale=None, mask_padding=False,
                     context_lens=None, **refused):
        """HOW LIKELY the model finds every token of a picture under a caption (extension).  ``img`` [B, C, H, W]
        is encoded as ``to_latent`` does, or ``ids=`` int64 [B, N] gives the codes; a position that holds the mask id (a decode loop
        leaves some) has no true id: it stays masked in every draw, is never scored, and its map entries are NaN (0 / 0).  ``text``: a list of B
        prompts, one prompt for every image, a context tensor [B, L, D], or None -- the unconditional branch.  With ``mask_padding``
        the non-pad lengths come from the text model; ``context_lens`` gives them.

        The rule, which is the contract:
            1. ids are given, or ids = to_latent(img)
            2. masks = diff_draws(B, N, mask_ratio, draws, seed): every position is masked in at least one draw
            3. draw j: the ids with the mask id where masks[j] is set go through ONE forward under ``text``
            4. with ``guidance_scale`` (one finite number; needs text) a second forward of the same ids runs without text, and the row
               that is scored is uncond + guidance_scale * (cond - uncond): the logits a guided step samples from
            5. every masked position t of image b, with its TRUE id i, adds  log softmax(x)[i],  the entropy of softmax(x)  and the
               place of i in the samplers' order (value descending, column ascending)  to three accumulators, and 1 to count[b, t]
            6. each map = acc / count (the rank as a float mean)
        On the GPU step 5 is one HBM-bound kernel (``ops.token_logprob``) that forms step 4's row at load; on the CPU the same rule in
        plain torch.  Not served (ValueError): the segment arrays, prompt weights, negative prompts, a guidance schedule.

        -> TokenScores(logp, entropy, rank), f32 [B, g, g] on the pipeline's device.  Nothing is captured: a later call of anything
        runs what it ran before."""
        ids, context, lens, scale = self._score_args("token_scores", img, ids, text, mask_padding, context_lens, guidance_scale, refused)
        B, g = ids.shape[0], self.image_size // self.patch_size
        masks = diff_draws(B, self.num_tokens, mask_ratio, draws, seed)
        return TokenScores(*(x.reshape(B, g, g) for x in self._token_scores(ids, context, lens, masks, scale)))

    @torch.no_grad()
    def score(self, img=None, text=None, *, ids=None, relative=False, mask_ratio=0.5, draws=4, seed=0, guidance_scale=None,
              mask_padding=False, context_lens=None, **refused):
        """The model's LIKELIHOOD of a picture under a caption (extension): the mean over the tokens of
        ``token_scores(...).logp`` that hold a code (mask ids among ``ids=`` take no part) -> f32 [B], <= 0, higher = more plausible.  ``relative=True`` subtracts the same call with
        ``text=None`` and the same masks: log p(tokens | text) - log p(tokens | no text), a text-to-image alignment score (it needs
        text and refuses ``guidance_scale``, which mixes the two branches it compares).  Arguments as in ``token_scores``."""
        ids, context, lens, scale = self._score_args("score", img, ids, text, mask_padding, context_lens, guidance_scale, refused)
        if relative and (context is None or scale is not None):
            raise ValueError("score: relative=True compares the text branch with the unconditional one: it needs text and takes no guidance_scale")
        B = ids.shape[0]
        masks = diff_draws(B, self.num_tokens, mask_ratio, draws, seed)
        known = (ids != self.mask_token_id).to(self.mask_token.device)

        def mean(logp):                                        # over the positions that hold a code (0 / 0 = NaN for an image with none)
            return torch.where(known, logp, torch.zeros_like(logp)).sum(dim=1) / known.sum(dim=1)
        value = mean(self._token_scores(ids, context, lens, masks, scale)[0])
        if relative:
            value = value - mean(self._token_scores(ids, None, None, masks, None)[0])
        return value

    @torch.no_grad()
    def surprise_mask(self, img, text, threshold=0.5, grow=1, return_score=False, **token_scores_keywords):
        """An edit mask from WHAT DOES NOT FIT THE CAPTION (extension): no phrase, no second prompt.
            s    = -token_scores(img, text, ...).logp           the surprise of every token's true id under the caption
            mask = s >= threshold * max_t s[b],  0 < threshold <= 1,  dilated ``grow`` times by a 3 x 3 maximum (``ops.phrase_region``);
                   an image whose maximum is exactly 0 gets an EMPTY mask
        -> bool [B, g, g] on the pipeline's device: what ``edit(token_mask=)`` and ``prompt_to_prompt(blend_mask=)`` take; with
        ``return_score`` (mask, s f32 [B, g, g]).  The repair of what does not fit is the composition
        ``edit(img, token_mask=surprise_mask(img, text), text=text)``.  The defaults are defaults, not optima measured on this tower."""
        _check_region("surprise_mask", threshold, grow)
        if "ids" in token_scores_keywords:
            raise ValueError("surprise_mask: the mask is one of an image: pass img")
        s = -self.token_scores(img, text, **token_scores_keywords).logp
        B, g = s.shape[0], s.shape[1]
        s = s.reshape(B, g * g).contiguous()
        mask = self._score_mask(self._steps(), s, g, threshold, grow).reshape(B, g, g)
        return (mask, s.reshape(B, g, g)) if return_score else mask

    @torch.no_grad()
    def best_of(self, text, n, *, score_guidance=None, score_mask_ratio=0.5, score_draws=4, score_seed=0, return_all=False, timesteps=18,
                temperature=1.0, topk=5, top_p=None, guidance_scale=None, choice_temperature=None, mask_padding=False, seed=None,
                image_base=0, **refused):
        """BEST OF n (extension): n candidates per prompt, the one the model itself finds most plausible is
        kept.  ``text``: a list of B prompts.  Candidate j of prompt b is the image with the global index image_base + j * B + b: its ids
        are, bit for bit, row b of the ``generate`` / ``generate_ids`` run with ``image_base = image_base + j * B`` and the same
        ``seed`` (None: one seed is drawn for the call) -- that loop runs n times.  Then
            scores[:, j] = score(ids=candidate ids, text=the prompts' context, guidance_scale=score_guidance,
                                 mask_ratio=score_mask_ratio, draws=score_draws, seed=score_seed)
        and the winner is the arg-max over j, ties to the lowest j; a NaN score never beats a number (``best_index``).  The ids a
        loop returns still hold the mask id at the positions its last step re-masked (at least one): they take no part in the score,
        and no image can be decoded from them -- ``generate``'s image is decoded from the last step's predictions at ALL positions.
        So every candidate's LAST step is decoded inside its loop (one decode per candidate, none for the other steps) and the
        winners' images are picked; they stay on the device.  ``timesteps, temperature, topk, top_p, guidance_scale,
        choice_temperature, mask_padding, seed, image_base`` are ``generate``'s; regions, prompt weights, negative prompts and edits
        are refused in this version.
        (A pipeline on the CPU runs the same rule; its loop does not key the noise by the image index, so under a fixed seed its
        candidates coincide.)

        -> (imgs [B, C, H, W] on the pipeline's device, index int64 [B], scores f32 [B, n]); with ``return_all`` the candidates' ids
        int64 [B, n, N] as a fourth."""
        if refused:
            raise ValueError(f"best_of does not serve {sorted(refused)} (regions, prompt weights, negative prompts and edits are refused "
                             f"in this version)")
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"best_of: n {n!r} must be an integer >= 1")
        if isinstance(text, str) or not isinstance(text, (list, tuple)) or not all(isinstance(p, str) for p in text) or not text:
            raise ValueError("best_of: text must be a list of prompts")
        if isinstance(image_base, bool) or not isinstance(image_base, int) or image_base < 0:
            raise ValueError(f"best_of: image_base {image_base!r} must be a non-negative integer")
        B = len(text)
        diff_draws(B, self.num_tokens, score_mask_ratio, score_draws, score_seed)       # the scoring keywords, checked before any loop runs
        _finite_number("best_of", "score_guidance", score_guidance)
        if mask_padding:
            context, lens = self.text_model(list(text), return_lens=True)
        else:
            context, lens = self.text_model(list(text)), None
        if context is None:
            raise ValueError("best_of needs a text condition (the score is that of the picture under its prompt)")
        opts = self._options(topk, top_p, guidance_scale, lens, choice_temperature, context, B, timesteps=timesteps)
        keys = self._keys(context, B, opts)
        if seed is None:
            seed = _draw_seed()
        cpu = self._on_cpu()
        if not cpu:
            context = context.to(self.engine().device)
            use_graph = os.environ.get("PMHIP_GENERATE_GRAPH", "1") != "0"
        cands, scores, last = [], [], []
        flags = [False] * (timesteps - 1) + [True]
        for j in range(n):
            if cpu:
                imgs, ids = self._generate_cpu(context, B, timesteps, temperature, opts, 1, seed, True, keys)
            else:
                ids, imgs = self.generate_ids(context, B, timesteps, temperature, opts, flags, seed, image_base=image_base + j * B,
                                              use_graph=use_graph, streams=1, keys=keys)
            cands.append(ids)
            last.append(imgs[-1])
            scores.append(self.score(ids=ids, text=context, guidance_scale=score_guidance, mask_ratio=score_mask_ratio, draws=score_draws,
                                     seed=score_seed, context_lens=lens))
        scores = torch.stack(scores, dim=1)
        cands = torch.stack(cands, dim=1)
        index = best_index(scores)
        last = torch.stack(last, dim=1)
        imgs = last[torch.arange(B, device=last.device), index.to(last.device)]
        return (imgs, index, scores, cands) if return_all else (imgs, index, scores)

    @torch.no_grad()
    def ids2tokens(self, ids):
        """lookup in cat(RAW codebook, mask_token) (generate.py:148-157)."""
        table = torch.cat((self.vqgan.quantize.embedding.weight.data.float(), self.mask_token.data.float())).contiguous()
        if self._on_cpu():
            return table[ids]
        rows = ops.embed_rows(table, ids.contiguous().reshape(-1), table.shape[1], torch.float32)
        return rows.reshape(ids.shape + (table.shape[1],))

    @torch.no_grad()
    def sample(self, ids, mask_ratio, text=None, topk=1, temperature=1, noise=None, seed=None, step=0, image_base=0,
               guidance_scale=None, context_lens=None, choice_temperature=None, choice_noise=None, top_p=None, negative_text=None,
               negative_context_lens=None, context_segments=None, token_segments=None, context_weights=None):
        """One MaskGIT step (generate.py:159-181) -> (ids', img).

        ``context_weights`` (extension; None = the step as without them): prompt weights, see ``tokens2logits``.  Like the segments,
        only the forward with ``text`` sees them.

        ``context_segments`` / ``token_segments`` (extension; None = the step as without them): regional prompts, see
        ``tokens2logits``.  Only the forward with ``text`` sees them: the second forward of a guided step -- without a context or with
        the negative one -- never does.

        ``negative_text`` (extension; None = the step as without the keyword): a NEGATIVE prompt -- like ``text`` a context tensor
        (B, Ln, D) here; Ln need not equal L.  The second forward of the guided step then sees this context instead of none, and
        the step's logits are ``neg + guidance_scale * (cond - neg)``: the image moves away from it (Muse's negative prompting).
        Needs ``guidance_scale`` and ``text``.  ``negative_context_lens``: one length per image for it, like ``context_lens``.

        ``top_p`` (extension; None or 1.0 = no nucleus filter, the step as without the keyword): 0 < top_p <= 1.  Behind the
        top-k, only the elements whose probability mass strictly above them is below ``top_p`` of the top-k's mass are drawn
        from.  Like ``topk`` it reads the raw logits: the temperature acts in the draw only.

        ``topk``: 1..n_embed like the reference's ``top_k(logits, k)``, on the GPU as on the CPU (above
        64 the selection kernel); ``None`` = no filter, i.e. n_embed.

        ``noise``: optional uniform(0,1) tensor shaped like the logits (B,N,V) -- the parity hook for the
        reference's ``torch.zeros_like(t).uniform_(0,1)``; without it a counter-based Philox stream keyed
        by (seed, step, image_base + image index, position, class) is used.  ``seed=None`` draws a fresh
        seed from the torch generator on every call, like the reference's fresh global-RNG noise
        (generate.py:40-46), so a caller looping over sample() never reuses uniforms.

        ``guidance_scale`` (extension; None = the reference's behaviour): the step's logits become
        ``uncond + guidance_scale * (cond - uncond)`` with ``uncond = transformer(tokens, None)``, the path the reference
        trains by dropping the text 10 % of the time (utils/trainer.py:379,387-388) but never uses when sampling.  Both
        forwards share the step's token lookup; everything after the logits is the reference's step unchanged.

        ``context_lens`` (extension; None = the reference's behaviour): one context length per image, see ``tokens2logits``.
        The unconditional forward of a guided step takes no context and so no lengths.

        ``choice_temperature`` (extension; None or 0 = the reference's behaviour): THIS step's choice temperature, like
        ``temperature`` the step's own value.  The re-masking then picks the ``num_mask`` positions by MaskGIT's perturbed
        confidence ``log p + choice_temperature * gumbel`` instead of by ``1 - p`` alone; a position whose id was given is
        never preferred to one the step took.  ``choice_noise``: optional uniform(0,1) tensor (B,N), the parity hook for
        that gumbel noise; without it the Philox stream of the step, at a counter word no class column uses.
        """
        nm = num_token_masked(mask_ratio, self.num_tokens)
        opts = self._options(topk, top_p, guidance_scale, context_lens, choice_temperature, text, ids.shape[0], negative_text,
                             negative_context_lens)
        keys = self._keys(text, ids.shape[0], opts, context_segments, token_segments, context_weights)
        return self._step(ids, nm, text, opts, temperature, opts.choice_temperature, noise, seed, step, image_base, choice_noise, keys)

    @torch.no_grad()
    def _step(self, ids, nm, text, opts, temperature, choice_t, noise=None, seed=None, step=0, image_base=0, choice_noise=None,
              keys=None):
        """``sample`` behind its checks: one step that re-masks nm tokens, with the step's own temperature and choice temperature;
        keys: the call's ``ops.Keys`` (None: those of opts alone)"""
        if keys is None:
            keys = self._keys(text, ids.shape[0], opts)
        if self._on_cpu():
            return self._sample_cpu(ids, nm, text, opts.topk, temperature, noise, seed, opts.guidance_scale, keys, choice_t,
                                    choice_noise, opts.top_p, opts.negative, opts.negative_lens)
        if seed is None:
            seed = _draw_seed()
        eng = self.engine()
        ids = ids.to(eng.device, torch.int64).clone().contiguous()
        ids, img, _, _ = eng.sample(self.vqgan.engine(), ids, text, opts.topk, temperature, nm, noise=noise, seed=seed, step=step,
                                    image_base=image_base, want_img=True, guidance_scale=opts.guidance_scale, choice_temperature=choice_t,
                                    choice_noise=choice_noise, top_p=opts.top_p, negative_context=opts.negative,
                                    negative_lens=opts.negative_lens, keys=keys)
        return ids, img

    def _sample_guided_composed(self, ids, nm, text, topk, temperature, noise, seed, step, image_base, scale, context_lens=None):
        """the guided step composed from the operator-level C ABI (two pmhip_s2_forward + pmhip_guidance_combine +
        pmhip_sample_rows + decode + pmhip_remask): the same kernels, in the same order, as pmhip_pipeline_sample_guided.
        Not on any product path: the bit-identity reference of tests/test_gpu_model.py for the native guided step / loop."""
        eng = self.engine()
        ids = ids.to(eng.device, torch.int64).clone().contiguous()
        B, N = ids.shape
        tok = self.ids2tokens(ids)
        cond = eng.forward(tok, text, context_lens=context_lens)
        uncond = eng.forward(tok, None)
        logits = ops.guidance_combine(cond, uncond, scale, out=cond)
        if noise is not None:
            noise = noise.to(eng.device, torch.float32).reshape(B * N, -1).contiguous()
        pred, merged, score = ops.sample_rows(logits.reshape(B * N, -1), ids.reshape(-1), self.mask_token_id, topk, temperature,
                                              noise=noise, seed=seed, step=step, row_base=image_base * N)
        img = self.vqgan.decode_from_indice(pred.reshape(B, N))   # decoded from the predictions at ALL positions (:165)
        ids = ops.remask(merged.reshape(B, N), score.reshape(B, N), nm, self.mask_token_id)
        return ids, img

    def _sample_cpu(self, ids, nm, text, topk, temperature, noise, seed, guidance_scale=None, keys=None, choice_t=0.0,
                    choice_noise=None, top_p=1.0, negative=None, negative_lens=None, counts=None):
        """generate.py:159-181 in plain torch for a pipeline that lives on the CPU.  The noise is drawn from the torch CPU
        generator like the reference's (`seed` re-seeds a private generator; `noise` overrides it); ties in top-k / argmax
        follow torch.  keys: the checked ``ops.Keys`` of the forward with `text` (None: every row is attended to).
        choice_t != 0: the re-masking sorts by choice_keys; its uniforms are `choice_noise`, or drawn behind the
        token noise from the same generator.  top_p < 1: of the top-k values only those nucleus_keep keeps.  negative: the second
        forward of a guided step takes this context (with negative_lens) instead of none.  counts (a list of B ints; None = the
        reference's step): the EDIT step -- image b re-masks counts[b] positions (0: none) instead of nm, and no image is decoded
        (``edit`` decodes the merged ids of its last step itself)."""
        tok = self.ids2tokens(ids)
        logits = self._logits(tok, text, keys)
        if guidance_scale is not None:
            uncond = self.tokens2logits(tok, negative, negative_lens)
            logits = torch.addcmul(uncond, logits - uncond, torch.tensor(float(guidance_scale)))
        return self._tail_cpu(ids, logits, nm, topk, temperature, noise, seed, choice_t, choice_noise, top_p, counts)

    def _tail_cpu(self, ids, logits, nm, topk, temperature, noise, seed, choice_t=0.0, choice_noise=None, top_p=1.0, counts=None):
        """the sampling tail of ``_sample_cpu`` behind the logits: the token draw, the decode, the merge and the re-masking"""
        pred, merged, scores, g = self._draw_cpu(ids, logits, topk, temperature, noise, seed, top_p)
        img = None if counts is not None else self.vqgan.decode_from_indice(pred)   # decoded from the predictions at ALL positions (:165)
        return self._remask_cpu(merged, scores, nm, g, choice_t, choice_noise, counts), img

    def _draw_cpu(self, ids, logits, topk, temperature, noise, seed, top_p=1.0):
        """the first half of ``_tail_cpu``: the token draw and the merge -> (pred, merged, score, the generator the draw used): what
        ``ops.sample_rows`` leaves, before any re-masking (the local blend works on these)"""
        val, ind = logits.topk(topk, dim=-1)
        if top_p < 1.0:
            val = val.masked_fill(~nucleus_keep(val, top_p), float("-inf"))
        filtered = torch.full_like(logits, float("-inf")).scatter_(2, ind, val)
        g = None if seed is None else torch.Generator().manual_seed(int(seed) & (2 ** 63 - 1))
        if noise is None:
            noise = torch.rand(logits.shape, generator=g)
        gumbel = -torch.log((-torch.log(noise.clamp(min=1e-20))).clamp(min=1e-20))
        pred = (filtered / max(temperature, 1e-10) + gumbel).argmax(dim=-1)
        is_mask = ids == self.mask_token_id
        merged = torch.where(is_mask, pred, ids)
        scores = 1 - logits.softmax(dim=-1).gather(2, pred[..., None])[..., 0]
        return pred, merged, scores.masked_fill(~is_mask, -1e5), g

    def _forced_cpu(self, ids, logits, target, noise, seed):
        """``ops.sample_rows_forced`` in plain torch: what ``_draw_cpu`` returns, with pred = target and score =
        1 - softmax(logits)[target] (-1e5 at given ids).  It builds the generator ``_draw_cpu`` builds and, with noise None, draws and
        DISCARDS the token draw's uniforms: the choice-temperature noise drawn behind them (``_remask_cpu``) is then the noise the
        other half of a pair sees."""
        g = None if seed is None else torch.Generator().manual_seed(int(seed) & (2 ** 63 - 1))
        if noise is None:
            torch.rand(logits.shape, generator=g)
        pred = target.to(ids.device, torch.long)
        is_mask = ids == self.mask_token_id
        merged = torch.where(is_mask, pred, ids)
        scores = 1 - logits.softmax(dim=-1).gather(2, pred[..., None])[..., 0]
        return pred, merged, scores.masked_fill(~is_mask, -1e5), g

    def _source_ids(self, source_ids, B, who):
        """the tokens of a real image, checked on the host once: int64 [B, N], every value a code of the codebook (no mask id)"""
        if not isinstance(source_ids, torch.Tensor) or source_ids.dtype != torch.int64 or tuple(source_ids.shape) != (B, self.num_tokens):
            got = f"{source_ids.dtype} {tuple(source_ids.shape)}" if isinstance(source_ids, torch.Tensor) else type(source_ids).__name__
            raise ValueError(f"{who}: source ids must be an int64 tensor [{B}, {self.num_tokens}], got {got}")
        bad = ((source_ids < 0) | (source_ids >= self.mask_token_id)).nonzero()
        if len(bad):
            b, i = bad[0].tolist()
            raise ValueError(f"{who}: source ids: image {b}, token {i}: {int(source_ids[b, i])} is no code in [0, {self.mask_token_id})")
        return source_ids

    @torch.no_grad()
    def forced_ids(self, target_ids, context, B, timesteps, seed, image_base=0, choice_temperature=None, guidance_scale=None,
                   context_lens=None, return_steps=False):
        """The teacher-forced loop of ONE image batch: the eager MaskGIT loop from the all-mask state in which
        every step's token draw is replaced by the KNOWN token, target_ids int64 [B, N] (``vqgan.encode``'s ids of a real image; every
        value in [0, n_embed), else ValueError naming the first offender -- checked on the host, once).  Every step runs the tower on
        the partially revealed image (a scalar guidance_scale adds the pass without a context), scores each revealed token by the
        model's own confidence in it -- 1 - softmax(logits)[target] -- and re-masks by the usual schedule (``loop_schedule``; the
        choice temperature's noise under `seed`, `image_base` as in ``generate_ids``): the image is revealed in the order the model
        finds it plausible.  Nothing is drawn, so there is no temperature, top-k or top_p.
        -> ids [B, N]: target_ids except at the nmask[T-1] positions per image still masked.  return_steps: (ids, revealed_at), int64
        [B, N], the first step after which the position is unmasked (T: still masked at the end)."""
        T, N = int(timesteps), self.num_tokens
        st = self._steps()
        target = st.ids(self._source_ids(target_ids, B, "forced_ids"))
        _no_schedule("forced_ids", guidance_scale)
        opts = self._options(1, None, guidance_scale, context_lens, choice_temperature, context, B)
        keys = self._keys(context, B, opts)
        _, nmask, ctemps = loop_schedule(T, 1.0, N, opts.choice_temperature)
        context = st.context(context)
        ids = torch.full((B, N), self.mask_token_id, dtype=torch.long, device=st.device)
        revealed_at = torch.full((B, N), T, dtype=torch.long, device=st.device)
        for step in range(T):
            tok = self.ids2tokens(ids)
            logits = st.forward(tok, context, keys)
            if opts.guidance_scale is not None:
                logits = st.guide(logits, st.forward(tok, None, None), opts.guidance_scale)
            draw = st.forced(ids, logits, target, None, seed, step)
            ids = st.remask(draw, nmask[step], ctemps[step] if ctemps else 0.0, seed, step, image_base)
            if return_steps:
                revealed_at = torch.where((ids != self.mask_token_id) & (revealed_at == T), torch.full_like(revealed_at, step), revealed_at)
        return (ids, revealed_at) if return_steps else ids

    # -- canvases beyond the token grid ---------------------------------------------------------------------
    def canvas_layout(self, size, stride=None, fuse="uniform"):
        """the ``canvas.CanvasLayout`` of a canvas of size = (H, W) pixels under this pipeline's windows; stride in tokens (None:
        half a window)"""
        g = self.image_size // self.patch_size
        return canvas_layout(canvas_grid(size, self.patch_size), g, g // 2 if stride is None else stride, self.patch_size, fuse)

    def _canvas_ids0(self, ids0, B, Nc):
        """the start ids of a canvas call, checked on the host once: an integer tensor [B, Nc], every value a code or the mask id"""
        if not isinstance(ids0, torch.Tensor) or ids0.dtype not in (torch.int64, torch.int32) or tuple(ids0.shape) != (B, Nc):
            got = f"{ids0.dtype} {tuple(ids0.shape)}" if isinstance(ids0, torch.Tensor) else type(ids0).__name__
            raise ValueError(f"canvas: ids0 must be an integer tensor [{B}, {Nc}], got {got}")
        bad = ((ids0 < 0) | (ids0 > self.mask_token_id)).nonzero()
        if len(bad):
            b, i = bad[0].tolist()
            raise ValueError(f"canvas: ids0: canvas {b}, token {i}: {int(ids0[b, i])} is outside [0, {self.mask_token_id}] (codes and the mask id)")
        return ids0.to(torch.long)

    @torch.no_grad()
    def canvas_ids(self, context, B, layout, timesteps, temperature, topk, seed, image_base=0, guidance_scale=None, context_lens=None,
                   choice_temperature=None, top_p=None, negative_context=None, negative_lens=None, ids0=None, window_batch=None):
        """The decode loop of B CANVASES larger than the token grid on an explicit context -> (ids, merged),
        int64 [B, Nc] each: the ids behind the last re-masking, and the last step's merged ids, every position filled.

        layout (``canvas_layout``) lays overlapping model-sized windows over the canvas.  Every step gathers the windows' ids from
        the canvas ids, runs the tower on the B * W windows -- every window of a canvas under that canvas's context, lengths and
        negative context --, fuses the windows' logits into ONE row of logits per canvas token (``ops.window_logits``; a guided step
        hands over both passes and the step's scale, so no combined window logits are written), and then takes one draw over the
        B * Nc rows (the noise under row_base = image_base * Nc) and one re-masking over [B, Nc] with ``loop_schedule(T, temperature,
        Nc, choice_temperature)``.  Overlapping windows therefore see the same token at every shared position at every step.

        ids0 (None: all masked): int [B, Nc], a code or the mask id per position.  Positions that hold a code are kept: canvas b then
        re-masks by ``edit_schedule`` over its own masked count, as ``edit`` does -- a given token is never re-masked and nothing
        is left masked.  window_batch = n: the forward runs in chunks of at most n windows into one logits buffer; the engine may pick
        another GEMM route per batch size, so results for different window_batch values are NOT promised to be bit-identical.
        The other keywords: as in ``generate_ids``.  Eager; not served: the captured-graph loop, lanes, sessions, regions, weights."""
        T, Nc, W = int(timesteps), layout.tokens, layout.n_windows
        if layout.g * layout.g != self.num_tokens or layout.patch != self.patch_size:
            raise ValueError(f"canvas_ids: the layout's windows ({layout.g} x {layout.g} tokens of {layout.patch} pixels) are not this pipeline's")
        if window_batch is not None and (isinstance(window_batch, bool) or not isinstance(window_batch, int) or window_batch < 1):
            raise ValueError(f"canvas_ids: window_batch {window_batch!r} must be a positive integer or None")
        st = self._steps()
        opts = self._options(topk, top_p, guidance_scale, context_lens, choice_temperature, context, B, negative_context, negative_lens, T)
        per_window = lambda lens: None if lens is None else [n for n in lens for _ in range(W)]
        context_w = st.context(None if context is None else context.repeat_interleave(W, 0))
        negative_w = st.context(None if opts.negative is None else opts.negative.repeat_interleave(W, 0))
        keys = self._host_keys(context_w, B * W, per_window(opts.lens))
        negative_keys = None if negative_w is None else self._host_keys(negative_w, B * W, per_window(opts.negative_lens))
        temps, nmask, ctemps = loop_schedule(T, temperature, Nc, opts.choice_temperature)
        if ids0 is None:
            ids, per_canvas = torch.full((B, Nc), self.mask_token_id, dtype=torch.long, device=st.device), None
        else:
            ids0 = self._canvas_ids0(ids0, B, Nc)
            per_canvas = [edit_schedule(m, T) for m in (ids0 == self.mask_token_id).sum(1).tolist()]
            ids = st.ids(ids0.clone())
        if seed is None and not self._on_cpu():
            seed = _draw_seed()
        gather = st.ids(torch.from_numpy(np.array(layout.gather)))
        merged = ids
        for step in range(T):
            tok = self.ids2tokens(ids[:, gather].reshape(B * W, self.num_tokens))
            cond = st.forward_chunks(tok, context_w, keys, window_batch)
            scale = opts.step_scale(step)
            uncond = None if scale is None else st.forward_chunks(tok, negative_w, negative_keys, window_batch)
            logits = st.window_logits(layout, cond, uncond, scale)
            draw = st.canvas_draw(ids, logits, opts, temps[step], seed, step, image_base)
            if step == T - 1:
                merged = draw.merged.reshape(B, Nc).clone()    # (the re-masking works in place on the draw's merged ids)
            ids = st.canvas_remask(draw, (B, Nc), nmask[step], None if per_canvas is None else [s[step] for s in per_canvas],
                                   ctemps[step] if ctemps else 0.0, seed, step, image_base).reshape(B, Nc)
        return ids, merged

    @torch.no_grad()
    def decode_canvas(self, ids, layout):
        """canvas ids int64 [B, Nc] without a mask id -> the canvas image f32 [B, C, H, W]: the ids are gathered per window, every
        window is decoded like an image of its own, and the windows' pixels are blended under the layout's separable tent weights
        (``ops.window_pixels``): a pixel one window covers is that window's pixel"""
        B, W = ids.shape[0], layout.n_windows
        if tuple(ids.shape) != (B, layout.tokens):
            raise ValueError(f"decode_canvas: ids must be [B, {layout.tokens}], got {tuple(ids.shape)}")
        st = self._steps()
        gather = st.ids(torch.from_numpy(np.array(layout.gather)))
        imgs = self.vqgan.decode_from_indice(st.ids(ids)[:, gather].reshape(B * W, self.num_tokens))
        return st.window_pixels(layout, imgs)

    @torch.no_grad()
    def generate_canvas(self, text, size, stride=None, timesteps=18, temperature=1.0, topk=5, seed=None, image_base=0, fuse="uniform",
                        guidance_scale=None, negative_text=None, mask_padding=False, top_p=None, choice_temperature=None, ids0=None,
                        window_batch=None, return_ids=False, **unserved):
        """A picture LARGER than the model's square (extension): size = (H, W) pixels, multiples of the patch
        size and at least the model's image on both axes, at most 4096 tokens -- a panorama, a 512 x 512, an image extended to three
        times its width.  Overlapping model-sized windows, `stride` tokens apart (None: half a window), are laid over the canvas; the
        tower runs on every window and the windows' LOGITS are fused per canvas token -- ``fuse`` "uniform": the mean over the windows
        that cover it, "tent": weighted towards a window's centre --, so one draw and one re-masking are taken over the whole canvas
        (``canvas_ids`` has the step).  The image is decoded per window from the last step's merged ids and the windows' pixels are
        blended (``decode_canvas``).  -> img f32 [B, 3, H, W] on the pipeline's device; with return_ids (img, final ids [B, Gh * Gw]).

        ids0 (None: everything is generated): int [B, Gh * Gw] with the mask id where a token is to be generated; the other
        positions are kept as they are.  A 256-pixel image's ``vqgan.encode`` ids placed into a wide all-mask canvas are extended.
        text, guidance_scale (a number or one per step), negative_text, mask_padding, topk, top_p, choice_temperature, temperature,
        seed, image_base: as in ``generate``; canvas j of a batch is the call with image_base + j alone.  window_batch = n: at most n
        windows per forward (memory); results for different values are not promised to be bit-identical (the engine may pick another
        GEMM route per batch size).  Not served, a ValueError: regions, prompt weights, segment arrays, context lengths by hand."""
        for name in sorted(unserved):
            if name not in CANVAS_UNSERVED:                    # (a misspelt keyword is what it is anywhere else)
                raise TypeError(f"generate_canvas() got an unexpected keyword argument {name!r}")
            raise ValueError(f"generate_canvas: {name} is not served on a canvas (regions, prompt weights, segment arrays and context lengths "
                             f"by hand are not parameters of generate_canvas)")
        layout = self.canvas_layout(size, stride, fuse)
        B = len(text)
        context, context_lens = self.text_model(text, return_lens=True) if mask_padding else (self.text_model(text), None)
        if negative_text is not None and context is None:
            raise ValueError("negative_text needs a text condition (an unconditional pipeline has none)")
        negative, negative_lens = self._negative_context(negative_text, B, mask_padding)
        ids, merged = self.canvas_ids(context, B, layout, timesteps, temperature, topk, seed, image_base, guidance_scale, context_lens,
                                      choice_temperature, top_p, negative, negative_lens, ids0, window_batch)
        img = self.decode_canvas(merged, layout)
        return (img, ids) if return_ids else img

    def _remask_cpu(self, ids, scores, nm, g, choice_t=0.0, choice_noise=None, counts=None):
        """the second half of ``_tail_cpu``: the re-masking of the merged ids under their scores -> ids"""
        if choice_t:
            if choice_noise is None:
                choice_noise = torch.rand(scores.shape, generator=g)
            scores = choice_keys(scores, choice_t, choice_noise.to(scores.dtype))
        if counts is not None:
            for b, n in enumerate(counts):
                if n > 0:
                    ids[b, scores[b].topk(n).indices] = self.mask_token_id
            return ids
        return ids.scatter(1, scores.topk(nm, dim=-1).indices, self.mask_token_id)

    @staticmethod
    def _region_cpu(score_src, score_edit, g, threshold, grow):
        """``ops.phrase_region`` in plain torch: f32 [B, g*g] twice -> bool [B, g*g], the rule of ``phrase_mask`` on both halves, joined,
        dilated `grow` times by a 3 x 3 maximum"""
        B = score_src.shape[0]
        mask = (score_src >= threshold * score_src.amax(dim=1, keepdim=True)) | (score_edit >= threshold * score_edit.amax(dim=1, keepdim=True))
        mask = mask.reshape(B, g, g)
        for _ in range(grow):
            mask = torch.nn.functional.max_pool2d(mask[:, None].float(), 3, stride=1, padding=1)[:, 0] > 0
        return mask.reshape(B, g * g)

    @staticmethod
    def _blend_cpu(mask, src, edit):
        """``ops.blend_tokens`` in plain torch: (pred, merged, score) of the two halves -> the edited half's, the source's where not mask"""
        return tuple(torch.where(mask, e, s_) for s_, e in zip(src, edit))

    @torch.no_grad()
    def _generate_cpu(self, context, B, timesteps, temperature, opts, save_interval, seed, return_ids, keys=None):
        """generate.py:183-198, with plain or guided steps (see `sample`), for a pipeline that lives on the CPU.  (On the GPU the
        loop is the native one, graph-captured and lane-able.)  keys: the call's ``ops.Keys`` (None: those of opts alone)."""
        if keys is None:
            keys = self._keys(context, B, opts)
        temps, nmask, ctemps = loop_schedule(timesteps, temperature, self.num_tokens, opts.choice_temperature)
        ids = torch.full((B, self.num_tokens), self.mask_token_id, dtype=torch.long)
        imgs = []
        for step in range(timesteps):
            ids, img = self._sample_cpu(ids, nmask[step], context, opts.topk, temps[step], None, None if seed is None else seed + step,
                                        opts.step_scale(step), keys, ctemps[step] if ctemps else 0.0, None, opts.top_p, opts.negative,
                                        opts.negative_lens)
            if step % save_interval == 0:
                imgs.append(img)
        return (imgs, ids) if return_ids else imgs

    def _schedule(self, timesteps, temperature):
        return loop_schedule(timesteps, temperature, self.num_tokens)[:2]

    @torch.no_grad()
    def _lanes(self, k):
        """k (engine pair, stream) lanes for concurrent micro-batches; lane 0 is the primary engines"""
        eng, vq = self.engine(), self.vqgan.engine()
        cache = getattr(self, "_lane_cache", None)
        if cache is None or cache[0] is not eng or cache[1] is not vq:
            cache = (eng, vq, [(eng, vq, self._new_lane_stream(eng.device, 0, k))])
            self._lane_cache = cache
        lanes = cache[2]
        while len(lanes) < k:
            lanes.append((eng.clone(), vq.clone(), self._new_lane_stream(eng.device, len(lanes), k)))
        return lanes[:k]

    @staticmethod
    def _new_lane_stream(device, lane, n_lanes):
        """the HIP stream of one lane (a hook: tools/cu_mask_lanes.py replaces it with CU-masked streams for an experiment)"""
        return torch.cuda.Stream(device=device)

    def _start_ids(self, B, ids0, device):
        """the ids a decode loop starts from: all-mask, or a CONTIGUOUS int64 copy of ids0 [B, N] on `device` (the native calls
        read B * N consecutive ids; clone() alone would keep a view's strides)"""
        if ids0 is None:
            return torch.full((B, self.num_tokens), self.mask_token_id, dtype=torch.long, device=device)
        if tuple(ids0.shape) != (B, self.num_tokens):
            raise ValueError(f"start ids have shape {tuple(ids0.shape)}, expected {(B, self.num_tokens)}")
        return ids0.to(device, torch.long).clone(memory_format=torch.contiguous_format)

    def decode_session(self, slots=64, conditional=True, use_graph=None, record_steps=False, decode=True, max_context_len=None,
                       max_negative_len=None, filters=False, regions=False, weights=False):
        """a DecodeSession over this pipeline (paintmind_amd/serve.py): `slots` images decode together, each with its own
        timesteps / temperature / top-k / seed / context length / guidance scale or schedule / negative prompt, and new requests
        are admitted into free slots between steps.  max_negative_len: the capacity of the negative contexts, like max_context_len
        (None: it grows with the longest one admitted).  filters=True: a FilterSession -- a request's top-k may be anywhere in
        1..n_embed (None: no filter) and it may carry a nucleus mass top_p, like ``generate``; False: the session and the limits
        (top-k <= 8, no top_p) of before.  regions=True (an option of either session): ``submit(regions=[(prompt,
        mask), ...])`` gives a request regional prompts, like ``generate(regions=)`` for one image; False: the session refuses them,
        as before.  weights=True (an option of either session, beside the other two): a request carries prompt
        weights -- ``submit(text="a (red:1.4) barn")`` is read like ``generate(prompt_weights=True)``, ``submit(context=(ctx, w))``
        takes them explicitly, a region may be ``(prompt, mask, weight)``; False: the session refuses them, as before"""
        from .serve import DecodeSession, FilterSession
        return (FilterSession if filters else DecodeSession)(self, slots=slots, conditional=conditional, use_graph=use_graph,
                                                             record_steps=record_steps, decode=decode, max_context_len=max_context_len,
                                                             max_negative_len=max_negative_len, regions=bool(regions),
                                                             weights=bool(weights))

    def generate_ids(self, context, B, timesteps, temperature, topk, decode_flags, seed, image_base=0, use_graph=False, streams=1,
                     join=True, wait_current=True, host=None, guidance_scale=None, ids0=None, context_lens=None, choice_temperature=None,
                     top_p=None, negative_context=None, negative_lens=None, context_segments=None, token_segments=None,
                     context_weights=None, keys=None):
        """The decode loop on device tensors: returns (ids [B,N], imgs [n_decoded,B,C,H,W] or None).

        keys (a caller that holds the call's ``_Options`` -- passed as `topk` -- holds its ``ops.Keys`` too, and passes it instead of
        the lengths, segments and weights): nothing is checked again.

        context_weights [B, L] (None: the loop as without them): prompt weights, see ``tokens2logits``.  Every lane takes the rows of
        its micro-batch; the captured loop reads their bias array from device memory, so one graph serves every set of weights.

        context_segments [B, L] / token_segments [B, N] (None: the loop as without them): regional prompts, see ``tokens2logits``.  Every
        lane takes the rows of its micro-batch; the captured loop reads them from device memory, so one graph serves every layout.
        guidance_scale: a number, or a sequence of `timesteps` finite numbers, one per step (``generate`` has the meaning); the captured
        loop reads a schedule from device memory, so one graph serves every schedule.
        negative_context [B, Ln, D] (None: the second pass of a guided step runs without a context) with negative_lens, its per-image
        lengths: the negative prompt of ``generate``.  Every lane takes the rows of its micro-batch.

        streams > 1 (or a tuple of micro-batch sizes): the batch is cut into contiguous micro-batches that run CONCURRENTLY on separate HIP
        streams (own native handle + workspace each, same weights): memory-bound kernels of one micro-batch overlap
        the MFMA-bound kernels of another.  The sampling RNG is keyed by the global image index, so the result is
        identical to streams=1.
        join=False returns the per-lane results [(ids, imgs, stream), ...] without making the current stream wait (the
        caller joins); wait_current=False does not make the lanes wait for work already queued on the current stream
        (only valid when `context` is None or was produced before the lanes last synchronised with it).
        host = (pinned [n_decoded, B, C, H, W] float32 tensor, [copy stream per lane]): the decoded images go straight to
        the host buffer (every lane fills its rows, each image as soon as it is complete, on its own copy stream); no
        device image tensor is returned.
        ids0 (streams = 1 only): start from these ids [B, N] int64 instead of the all-mask state (the region loops of inpaint / outpaint).
        Without ids0 the native loop is told that it starts from the all-mask state (from_mask): an unconditional loop then samples
        its step 0 from logits the handle computed once (include/pmhip.h, PMHIP_GENERATE_FROM_MASK) -- same result, bit for bit,
        as passing an explicit all-mask ids0, which keeps the full path.
        context_lens (None: every image attends to all L rows of its context): one context length per image; image b's cross-attention
        sees rows [0, context_lens[b]) only.  Every lane takes the slice of its micro-batch.
        choice_temperature (None or 0: the reference's deterministic re-masking): MaskGIT's base choice temperature, annealed over the
        loop (choice_schedule); the noise is keyed by the global image index like the token draw's, so lanes change nothing.
        topk: 1..n_embed, or None = no filter (n_embed); part of the key of a captured graph.
        top_p (None or 1.0: no nucleus filter): every step's nucleus mass, 0 < top_p <= 1 (see ``sample``); one value for the batch,
        so every lane takes it as it is; below 1 part of the key of a captured graph."""
        opts = self._options(topk, top_p, guidance_scale, context_lens, choice_temperature, context, B, negative_context, negative_lens,
                             timesteps)
        if keys is None:
            keys = self._keys(context, B, opts, context_segments, token_segments, context_weights)
        else:                                            # (refused beside any of the arrays it stands for, or for another shape)
            keys = self._host_keys(context, B, context_lens, context_segments, token_segments, context_weights, keys)
        if ids0 is not None and tuple(ids0.shape) != (B, self.num_tokens):
            raise ValueError(f"generate_ids: ids0 has shape {tuple(ids0.shape)}, expected {(B, self.num_tokens)}")
        eng = self.engine()
        temps, nmask, ctemps = loop_schedule(timesteps, temperature, self.num_tokens, opts.choice_temperature)

        def run(e, v, ids, c, o, k, **kw):  # the native loop of one engine pair: the whole batch, or one lane's images with their o and k
            if o.negative is not None or o.guidance_scales is not None:
                kw.update(negative_context=o.negative, negative_lens=o.negative_lens, guidance_scales=o.guidance_scales)
            return e.generate(v, ids, c, temps, nmask, decode_flags, o.topk, seed=seed, use_graph=use_graph, want_device_imgs=host is None,
                              guidance_scale=o.guidance_scale, choice_temps=ctemps, top_p=o.top_p, keys=k, **kw)

        if isinstance(streams, (list, tuple)):           # explicit micro-batch sizes, e.g. (32, 16, 16)
            sizes = [int(x) for x in streams]
            if sum(sizes) != B or min(sizes) < 1:
                raise ValueError(f"micro-batch sizes {sizes} must be positive and sum to the batch size {B}")
            bounds = [(sum(sizes[:i]), sum(sizes[:i + 1])) for i in range(len(sizes))]
            streams = len(sizes)
        else:
            streams = max(1, min(int(streams), B))
            bounds = None
            if streams == 2 and B >= 8:
                # two lanes of EQUAL size run the same kernel sequence in lockstep and meet in the same (MFMA- or HBM-bound)
                # kernel all the time; one image of difference lets them drift apart (round 3: 445-447 -> 450-453 images/s).
                # Re-measured with the round-5 kernels (profiles/r05_g_*): equal lanes are within +-1 % of this end to end on
                # every workload and box tried (and the per-launch attention time in the bench's brackets is the same): kept.
                bounds = [(0, B // 2 + 1), (B // 2 + 1, B)]
        if ids0 is not None and streams != 1:
            raise ValueError("generate_ids: ids0 needs streams=1")
        if streams == 1:
            ids = self._start_ids(B, ids0, eng.device)
            return run(eng, self.vqgan.engine(), ids, context, opts, keys, image_base=image_base, from_mask=ids0 is None,
                       host=None if host is None else (host[0], 0, host[1][0]))
        from .dist import shard_range
        cur = torch.cuda.current_stream(eng.device)
        if wait_current:
            ready = torch.cuda.Event()
            ready.record(cur)

        def run_lane(i, e, v, st):
            lo, hi = bounds[i] if bounds is not None else shard_range(B, i, streams)
            if wait_current:
                st.wait_event(ready)
            with torch.cuda.device(eng.device), torch.cuda.stream(st):
                ids = torch.full((hi - lo, self.num_tokens), self.mask_token_id, dtype=torch.long, device=eng.device)
                c = None if context is None else context[lo:hi].contiguous()
                ids, imgs = run(e, v, ids, c, opts.lane(lo, hi), keys.lane(lo, hi), image_base=image_base + lo, concurrent_lanes=True,
                                from_mask=True,                  # lanes exist for ids0 None only (checked above)
                                host=None if host is None else (host[0], lo, host[1][i]))
            return ids, imgs, st

        lanes = self._lanes(streams)
        if host is None:
            parts = [run_lane(i, e, v, st) for i, (e, v, st) in enumerate(lanes)]
        else:
            # with a host destination the native call paces its lane from the host (it blocks between segments, see
            # pmhip_pipeline_generate), so every lane is driven by its own thread; ctypes drops the GIL during the call
            pool = _lane_thread_pool(streams)
            futs = [pool.submit(run_lane, i, e, v, st) for i, (e, v, st) in enumerate(lanes)]
            # wait for EVERY lane before a failure is reported: the other lanes keep copying into the caller's host buffer
            # until their native call returns.  That includes an exception delivered to THIS thread while it waits (a
            # KeyboardInterrupt): the lane threads are inside the native call and cannot be cancelled, so the caller's
            # cleanup (which retires the host buffer) may only run once they have all returned.
            try:
                done = [(f.exception(), f) for f in futs]
            finally:
                concurrent.futures.wait(futs)
            for err, _ in done:
                if err is not None:
                    raise err
            parts = [f.result() for _, f in done]
        if not join:
            return parts
        return self.join_lanes(parts)

    @torch.no_grad()
    def control_ids(self, context_src, context_edit, lens_src, lens_edit, row_map, blend, gain, B, timesteps, temperature, topk, seed,
                    image_base=0, top_p=None, choice_temperature=None, guidance_scale=None, cross_steps=0.8, self_steps=0.0, layers=None,
                    want_imgs=False, noise=None, blend_rows=None, blend_mask=None, blend_threshold=0.3, blend_grow=1, blend_start=0.2,
                    return_mask=False, source_ids=None):
        """Prompt-to-prompt (Hertz et al.): the eager decode loop over B PAIRS of images -- one from
        context_src [B, L, D], one from context_edit [B, L, D], both from the all-mask state under the same seed -- in which the
        edited image's cross-attention takes the source image's probabilities for the context rows row_map pairs.
        -> (ids_src, ids_edit), each [B, N]; with want_imgs (ids_src, ids_edit, img_src, img_edit), the images decoded from the last
        step's predictions at ALL positions, as ``generate`` decodes its images.
        noise (None: drawn under `seed`): the token draw's uniforms, fp32 [T, B, N, n_embed], step t's for BOTH halves -- the same on the
        CPU branch and on the GPU, which draw their own differently.

        row_map, blend, gain [B, L]: per pair, the source row of every edited row (negative: none), how much of the source's
        probability it takes (0..1) and a factor on the result (``prompt.align_rows`` builds the first two; ``ops.attention_control``
        has the formula).  lens_src / lens_edit (None: every row): the per-image context lengths.
        cross_steps / self_steps: the fractions of the loop under control -- steps s < ceil(cross_steps * T) run
        ``S2Engine.forward_control`` with the cross-attention of `layers` (None: every layer) controlled, steps s < ceil(self_steps * T)
        also with the self-attention of those layers injected; later steps run the plain forward on the 2B images.
        The sampling tail runs once per half with the SAME seed, step and image_base: a pair shares its noise.  A scalar
        guidance_scale adds the pass without a context over the 2B images; that pass is never controlled.
        ids_src is ``generate_ids(context_src, ..., use_graph=False, streams=1)`` bit for bit; with cross_steps = self_steps = 0
        ids_edit is that of context_edit.  Whether the edited image keeps the source's layout on a MaskGIT tower is unmeasured.

        LOCAL BLEND (the paper's third control; without the keywords the call is the one above, bit for bit):
        outside a region the edited image takes the source's TOKENS.  The region is either drawn -- blend_mask, bool [B, g, g], and
        no scores are collected -- or follows from where the pair looks at a phrase: blend_rows = (w_src, w_edit), the phrase's row
        weights [B, L] in the two prompts (finite, >= 0, typically 0 / 1; every pair with a positive weight below its length in one
        half).  With blend_rows every step runs ``S2Engine.forward_control(score_layers=layers, ...)`` -- past cross_steps with no
        layer controlled --, from the conditional pass only (guidance's second pass is never tapped), and the scores accumulate into
        one [2B, N] buffer over layers and steps, in the stream's order.  A step s >= ceil(blend_start * T) then, between the token draw
        of both halves and their re-masking: the region ``ops.phrase_region(scores so far, blend_threshold, blend_grow)``, and
        ``ops.blend_tokens``.  Re-masking proceeds per half as ever; both halves share their noise, so outside the region they re-mask
        the same way unless the region's own scores interfere.  The last step's image is decoded from the blended predictions.
        return_mask appends the last region, bool [B, g, g].  blend_threshold 0.3, blend_grow 1 and blend_start 0.2 are the paper's
        values, not optima measured on this tower.  Invariants:
          - the source half never reads the edited half: ids_src stays ``generate_ids`` on the source alone, bit for bit
          - at every blended step, before re-masking, the edited half's (pred, merged, score) equal the source half's at every token
            outside the region, bit for bit
          - blend_mask all true gives the ids of the call without a blend, bit for bit; all false makes ids_edit == ids_src
          - the final IMAGE is not promised to be pixel-equal outside the region: the decoder mixes tokens.

        A REAL IMAGE AS THE SOURCE (source_ids None: the call above, launch for launch): source_ids int64
        [B, N], the image's tokens (every value in [0, n_embed), checked on the host, once).  The source half's token draw at every step
        is then the forced step on them -- ``ops.sample_rows_forced`` on the half's rows of the logits, ``_forced_cpu`` on the CPU --
        and everything else is the loop as it stands: ids_src is ``forced_ids(source_ids, context_src, ...)`` bit for bit, whatever the
        edited half does, and with want_imgs the source image is decoded from source_ids at all positions.  The pair then no longer
        shares its TOKEN draw -- the edited half still draws under its noise; only the attention control and the blend tie the halves
        together (the re-masking noise stays shared)."""
        if context_src is None or context_edit is None or tuple(context_src.shape) != tuple(context_edit.shape) or context_src.dim() != 3 \
                or context_src.shape[0] != B:
            raise ValueError(f"control_ids: context_src and context_edit must be two context tensors [{B}, L, D] of one shape")
        _no_schedule("control_ids", guidance_scale)
        if (lens_src is None) != (lens_edit is None):
            raise ValueError("control_ids: lens_src and lens_edit come together")
        L, T = context_src.shape[1], int(timesteps)
        context = torch.cat([context_src, context_edit])
        lengths = None if lens_src is None else ops.host_lens(lens_src, B, L, "lens_src") + ops.host_lens(lens_edit, B, L, "lens_edit")
        opts = self._options(topk, top_p, guidance_scale, lengths, choice_temperature, context, 2 * B)
        keys = self._keys(context, 2 * B, opts)
        rm, bl, gn = ops.host_control(row_map, blend, gain, B, L)
        depth = len(self.transformer.layers)
        layers = ops.host_layers(range(depth) if layers is None else layers, depth, "control_ids: layers")
        for name, f in (("cross_steps", cross_steps), ("self_steps", self_steps)):
            if not 0.0 <= float(f) <= 1.0:
                raise ValueError(f"control_ids: {name}={f} must be a fraction in [0, 1]")
        n_cross, n_self = math.ceil(float(cross_steps) * T), math.ceil(float(self_steps) * T)
        temps, nmask, ctemps = loop_schedule(T, temperature, self.num_tokens, opts.choice_temperature)
        st = self._steps()
        N = self.num_tokens
        g = self.image_size // self.patch_size
        if blend_rows is not None and blend_mask is not None:
            raise ValueError("control_ids: blend_rows and blend_mask exclude each other (the region follows from a phrase or is drawn)")
        blending = blend_rows is not None or blend_mask is not None
        if return_mask and not blending:
            raise ValueError("control_ids: return_mask needs blend_rows or blend_mask")
        region, scores, blend_from = None, None, T
        if blending:
            _check_region("control_ids", blend_threshold, blend_grow, bools=True, prefix="blend_")
            if not 0.0 <= float(blend_start) < 1.0:
                raise ValueError(f"control_ids: blend_start={blend_start} must be a fraction in [0, 1) (the last step always blends)")
            if g * g != N or g > 64:
                raise ValueError(f"control_ids: the local blend needs a square token grid of at most 64 x 64, got {N} tokens")
            blend_from = math.ceil(float(blend_start) * T)
        if blend_rows is not None:
            blend_rows = ops.host_phrase_weights(blend_rows, B, L)
            ops.check_phrase_rows(*blend_rows, lengths, B, L)
        if blend_mask is not None:
            region = torch.as_tensor(blend_mask)
            if region.dtype != torch.bool or tuple(region.shape) != (B, g, g):
                raise ValueError(f"control_ids: blend_mask must be a bool tensor [{B}, {g}, {g}], got {region.dtype} {tuple(region.shape)}")
            region = st.drawn_region(region.reshape(B, N))
        context = st.context(context)
        ids = torch.full((2 * B, N), self.mask_token_id, dtype=torch.long, device=st.device)
        imgs = [None, None]
        if noise is not None and tuple(noise.shape) != (T, B, N, self.mask_token_id):
            raise ValueError(f"control_ids: noise must be a tensor [{T}, {B}, {N}, {self.mask_token_id}], got {tuple(noise.shape)}")
        if source_ids is not None:
            source_ids = st.ids(self._source_ids(source_ids, B, "control_ids"))
        for step in range(T):
            cross = layers if step < n_cross else []
            inject = layers if step < n_self else []
            ctl = dict(row_map=rm, blend=bl, gain=gn) if cross else {}
            tap = {} if blend_rows is None else dict(score_layers=layers, score_weights=blend_rows, scores=scores)
            tok = self.ids2tokens(ids)
            if cross or inject or tap:
                logits, scores = st.forward_control(tok, context, keys, cross, inject, ctl, tap)
            else:
                logits = st.forward(tok, context, keys)
            if opts.guidance_scale is not None:
                logits = st.guide(logits, st.forward(tok, None, None), opts.guidance_scale)        # (that pass is never controlled or tapped)
            u = None if noise is None else noise[step]
            draws = [st.draw(ids[h * B:(h + 1) * B], logits[h * B:(h + 1) * B], opts, temps[step], u, seed, step, image_base)
                     if h or source_ids is None else st.forced(ids[:B], logits[:B], source_ids, u, seed, step) for h in range(2)]
            if blending and step >= blend_from:
                if blend_rows is not None:
                    region = st.region(scores[:B], scores[B:], g, blend_threshold, blend_grow)
                draws[1] = st.blend(region, draws[0], draws[1])
            for h, d in enumerate(draws):                    # per half: the re-masking, then on the last step the image from ALL predictions
                ids[h * B:(h + 1) * B] = st.remask(d, nmask[step], ctemps[step] if ctemps else 0.0, seed, step, image_base)
                if want_imgs and step == T - 1:
                    imgs[h] = self.vqgan.decode_from_indice(d.pred.reshape(B, N))
        out = (ids[:B].clone(), ids[B:].clone()) + ((imgs[0], imgs[1]) if want_imgs else ())
        return out + ((region != 0).reshape(B, g, g),) if return_mask else out

    @torch.no_grad()
    def prompt_to_prompt(self, text, edit_text, mode="refine", reweight=None, timesteps=18, temperature=1.0, topk=5, seed=None, image_base=0,
                         top_p=None, choice_temperature=None, guidance_scale=None, cross_steps=0.8, self_steps=0.0, layers=None,
                         return_ids=False, local_blend=None, blend_threshold=0.3, blend_grow=1, blend_start=0.2, blend_mask=None,
                         return_mask=False, img=None, source_ids=None, **refused):
        """Change the prompt, keep the picture (Hertz et al., Prompt-to-Prompt): -> (img_src, img_edit), the
        image of `text` and the image of `edit_text` from one seed, the second attending with the first's cross-attention for the
        words the prompts share; ids with return_ids.  text / edit_text: a prompt each, or two lists of as many.

        mode 'refine' (words added or removed) or 'replace' (a word swapped): ``prompt.align_rows``.  reweight {phrase: gain}: the
        rows of that phrase of `edit_text` -- found as ``phrase_rows`` finds them, in every edited prompt that has it (once) -- are
        scaled by gain (>= 0); edit_text == text
        with a reweight is the paper's pure re-weighting.  Always under the non-pad lengths, as ``phrase_mask``.  The other
        keywords are those of ``control_ids``.  Not served (ValueError): negative_text, regions, prompt_weights / context_weights,
        the segment arrays, a guidance schedule, an unconditional pipeline.  Image quality on this tower is unmeasured.

        local_blend (the paper's third control; None = the call as without it): outside the region that looks
        at a phrase the edited image keeps the source's tokens (``control_ids`` has the rule and its invariants).  "dog": the phrase,
        in whichever prompt of a pair has it; ("cat", "dog"): the source prompt's phrase and the edited prompt's; or a list of B such
        items.  Each phrase occurs once in its prompt; a phrase in neither prompt, or with no token below max_length, is a
        ValueError.  blend_threshold / blend_grow / blend_start: the paper's 0.3 / 1 / 0.2, not optima measured on this tower.
        blend_mask (bool [B, g, g], instead of local_blend): the region, drawn.  return_mask appends the last region, bool [B, g, g].

        img ([B, C, H, W] in [-1, 1], encoded as ``edit`` encodes its image) or source_ids (int64 [B, N], its tokens; not both): a
        REAL image as the source.  `text` is then its caption, the source half is teacher-forced on its tokens
        (``control_ids(source_ids=)``) and img_src is the VQGAN reconstruction of the input.  With local_blend on top the edited
        image keeps the input's tokens outside the region; blend_start=0 is the natural setting for a real image (the default stays
        the paper's).  The pair no longer shares its token draw: only the attention and the blend tie the halves together."""
        if refused:
            raise ValueError(f"prompt_to_prompt does not serve {sorted(refused)} (negative prompts, regions, prompt weights and the segment "
                             f"arrays stand beside no attention control)")
        _no_schedule("prompt_to_prompt", guidance_scale)
        if getattr(self, "text_model", None) is None or text is None or edit_text is None:
            raise ValueError("prompt_to_prompt needs a text condition (an unconditional pipeline has no cross-attention to control)")
        if not hasattr(self.text_model, "fragment_ids"):
            raise NotImplementedError(f"{type(self.text_model).__name__} serves no token ids (fragment_ids): T5TextEmbedder does")
        from .prompt import align_rows
        src = [text] if isinstance(text, str) else list(text)
        tgt = [edit_text] if isinstance(edit_text, str) else list(edit_text)
        if len(src) != len(tgt) or not src:
            raise ValueError(f"prompt_to_prompt: {len(src)} prompts and {len(tgt)} edited prompts")
        reweight = dict(reweight or {})
        for phrase, g in reweight.items():
            if not isinstance(phrase, str) or not phrase.strip() or not (math.isfinite(float(g)) and float(g) >= 0):
                raise ValueError(f"prompt_to_prompt: reweight {phrase!r}: {g!r} must be a phrase and a finite gain >= 0")

        def cut(prompt, strict, look=None):
            """the prompt cut at the single occurrence of every phrase -> (fragments, the gain of each or None, whether each is the
            local blend's phrase `look`)"""
            found = {}
            for phrase, g in reweight.items():
                if prompt.count(phrase) == 0:
                    continue                                     # (a phrase of another prompt of the batch)
                if prompt.count(phrase) != 1:
                    if strict:
                        raise ValueError(f"prompt_to_prompt: the phrase {phrase!r} occurs {prompt.count(phrase)} times in {prompt!r}, not once")
                    found = {}
                    break
                found[phrase] = (prompt.index(phrase), phrase, float(g))
            if look is not None:
                if prompt.count(look) != 1:
                    raise ValueError(f"prompt_to_prompt: the phrase {look!r} of local_blend occurs {prompt.count(look)} times in {prompt!r}, not once")
                found.setdefault(look, (prompt.index(look), look, None))
            frags, gains, looks, at = [], [], [], 0
            for pos, phrase, g in sorted(found.values()):
                if pos < at:
                    raise ValueError(f"prompt_to_prompt: the phrases of reweight and local_blend overlap in {prompt!r}")
                frags += [prompt[at:pos], phrase]
                gains += [None, g]
                looks += [False, phrase == look]
                at = pos + len(phrase)
            return frags + [prompt[at:]], gains + [None], looks + [False]

        B = len(src)
        if img is not None and source_ids is not None:
            raise ValueError("prompt_to_prompt: img and source_ids exclude each other (the image, or its tokens)")
        if img is not None:
            self._check_img("prompt_to_prompt", img, B)
            source_ids = self.to_latent(img)[1].reshape(B, self.num_tokens).to(torch.long)
        elif source_ids is not None:
            if not isinstance(source_ids, torch.Tensor) or source_ids.dim() != 2 or source_ids.shape[0] != B:
                raise ValueError(f"prompt_to_prompt: source_ids must be int64 [{B}, {self.num_tokens}] (one image per prompt), got "
                                 f"{tuple(source_ids.shape) if isinstance(source_ids, torch.Tensor) else type(source_ids).__name__}")
        looks = [(None, None)] * B
        if local_blend is not None:
            if blend_mask is not None:
                raise ValueError("prompt_to_prompt: local_blend and blend_mask exclude each other (the region follows from a phrase or is drawn)")
            if not isinstance(local_blend, (str, tuple, list)):
                raise ValueError(f"prompt_to_prompt: local_blend {local_blend!r} must be a phrase, a pair of phrases or a list of {B} such items")
            items = [local_blend] * B if isinstance(local_blend, (str, tuple)) else list(local_blend)
            if len(items) != B:
                raise ValueError(f"prompt_to_prompt: local_blend has {len(items)} items for {B} pairs")
            looks = []
            for b, item in enumerate(items):
                if isinstance(item, str) and item.strip():
                    pair = (item if item in src[b] else None, item if item in tgt[b] else None)
                elif isinstance(item, tuple) and len(item) == 2 and all(isinstance(x, str) and x.strip() for x in item):
                    pair = item
                else:
                    raise ValueError(f"prompt_to_prompt: local_blend {item!r} must be a phrase or a pair (source phrase, edited phrase)")
                if pair == (None, None) or (pair[0] is not None and pair[0] not in src[b]) or (pair[1] is not None and pair[1] not in tgt[b]):
                    raise ValueError(f"prompt_to_prompt: the phrase {item!r} of local_blend does not occur in {src[b]!r} / {tgt[b]!r}")
                looks.append(pair)
        for phrase in reweight:
            if not any(phrase in p for p in tgt):
                raise ValueError(f"prompt_to_prompt: the phrase {phrase!r} of reweight occurs in no edited prompt")
        cuts = [cut(p, False, looks[b][0]) for b, p in enumerate(src)] + [cut(p, True, looks[b][1]) for b, p in enumerate(tgt)]
        context, lens, ids, spans = self.text_model.fragment_ids([c[0] for c in cuts])
        L = context.shape[1]
        lens = [int(n) for n in lens]
        rm, bl, gn = np.full((B, L), -1, np.int32), np.zeros((B, L), np.float32), np.ones((B, L), np.float32)
        for b in range(B):
            m, w = align_rows(ids[b], ids[B + b], mode)
            rm[b, :len(m)], bl[b, :len(w)] = m, w
            for (lo, hi), g in zip(spans[B + b], cuts[B + b][1]):
                if g is not None:
                    if hi <= lo:
                        raise ValueError(f"prompt_to_prompt: a phrase of reweight has no tokens below max_length in {tgt[b]!r}")
                    gn[b, lo:hi] = g
        blend = {}
        if local_blend is not None:
            rows = np.zeros((2, B, L), np.float32)
            for half, prompts in enumerate((src, tgt)):
                for b in range(B):
                    for (lo, hi), look in zip(spans[half * B + b], cuts[half * B + b][2]):
                        if look:
                            if hi <= lo:
                                raise ValueError(f"prompt_to_prompt: the phrase of local_blend has no tokens below max_length in {prompts[b]!r}")
                            rows[half, b, lo:hi] = 1.0
            blend = dict(blend_rows=(rows[0], rows[1]))
        if blend_mask is not None:
            blend = dict(blend_mask=blend_mask)
        if blend:
            blend.update(blend_threshold=blend_threshold, blend_grow=blend_grow, blend_start=blend_start, return_mask=return_mask)
        elif return_mask:
            raise ValueError("prompt_to_prompt: return_mask needs local_blend or blend_mask")
        context = context.to(self.mask_token.device, torch.float32)
        out = self.control_ids(context[:B], context[B:], lens[:B], lens[B:], rm, bl, gn, B, timesteps, temperature, topk,
                               _draw_seed() if seed is None else seed, image_base, top_p, choice_temperature, guidance_scale, cross_steps,
                               self_steps, layers, want_imgs=not return_ids, **blend, **({} if source_ids is None else dict(source_ids=source_ids)))
        return out if return_ids else out[2:]

    def join_lanes(self, parts):
        """make the current stream wait for the lanes and concatenate their results"""
        cur = torch.cuda.current_stream(parts[0][0].device)
        for ids, imgs, st in parts:
            cur.wait_stream(st)
            ids.record_stream(cur)                    # allocated on the lane's stream, consumed on the current one
            if imgs is not None:
                imgs.record_stream(cur)
        ids = torch.cat([p[0] for p in parts], dim=0)
        imgs = None if parts[0][1] is None else torch.cat([p[1] for p in parts], dim=1)
        return ids, imgs

    def generate(self, text, timesteps=18, temperature=1.0, topk=5, save_interval=2, seed=None, image_base=0,
                 return_ids=False, keep_on_device=False, use_graph=None, streams=None, guidance_scale=None, mask_padding=False,
                 context_lens=None, choice_temperature=None, top_p=None, negative_text=None, negative_context_lens=None, regions=None,
                 context_segments=None, token_segments=None, context_weights=None, prompt_weights=False):
        """Full decode loop (generate.py:183-198): list of (B,3,H,W) CPU tensors for steps % save_interval == 0.

        PROMPT WEIGHTS (extension).  prompt_weights=True: the prompts -- ``text`` and the prompts of
        ``regions`` -- carry emphasis syntax, ``a (red:1.4) barn, (blurry:0.5)`` (``paintmind_amd.prompt.parse_weighted``), and the
        text model is called with ``weighted=True``: every context row gets the weight of the words it came from, and the
        cross-attention counts it that much (``tokens2logits`` has the rule).  With ``mask_padding=True`` the padding rows are
        masked as without weights; otherwise they are attended to as before, at weight 1.  context_weights [B, L] gives the weights
        explicitly instead, for a ``text`` that is already a context; not beside ``regions`` or ``prompt_weights``.  An item of
        ``regions`` may be ``(prompt, mask, weight)``: the number multiplies the weight of that region's rows ("this region's
        prompt, but weaker").  The pass without the text and a negative prompt's pass never see weights.

        regions (extension; None = the loop as without it): REGIONAL PROMPTS, different text for different parts of the picture -- a
        list of B lists of ``(prompt, mask)``.  ``mask`` is a pixel mask [H, W] (non-zero = inside) or a bool token mask [g, g]; a
        token belongs to a region iff any pixel of its patch is set (the rule of ``edit``); regions may overlap, and a token in no
        region sees the global prompt only.  ``text`` stays the GLOBAL prompt, which every token attends to.  Image b's context is
        the concatenation [global | region 1 | region 2 | ...] (with ``mask_padding=True`` every prompt contributes its non-pad rows
        only), zero-padded to the longest image's total; its cross-attention lets a token see the global rows and the rows of the
        regions it is part of, nothing else.  At most 31 regions per image.  Guidance, ``negative_text``, ``topk``, ``top_p`` and
        ``choice_temperature`` compose unchanged: the pass without the text and the negative prompt's pass carry no regions.
        context_segments / token_segments give the two arrays explicitly instead (``tokens2logits``), for a ``text`` that is already
        the concatenation; neither goes with context_lens.

        guidance_scale (extension; None = the reference's loop): a number -- every step samples from ``uncond + guidance_scale *
        (cond - uncond)`` (see ``sample``) -- or a sequence of ``timesteps`` finite numbers, step s guiding with its own: Muse
        raises the scale over the steps, low early for diversity and high late for fidelity (``linear_guidance(timesteps, scale)``
        is one such list).  One captured graph serves every schedule; a scalar keeps its path and its graph per value.

        negative_text (extension; needs guidance_scale): a NEGATIVE prompt, one string for every image or a list of B strings, run
        through the text model like ``text``.  The second pass of every step sees it instead of no text, so the images move away
        from it.  With ``mask_padding=True`` its lengths come from the text model too; negative_context_lens gives them explicitly.

        The call is the fast path by default: the loop replays captured hipGraphs (first call eager, second call captures),
        in bf16 mode a batch of at least LANES_MIN_WORK (B * tokens * width: 33 images for d512, 22 for d768, 17 for d1024) runs
        as two concurrent micro-batch lanes (a smaller one as one lane whose per-step decode overlaps the next step), and every saved image starts its copy into a
        pinned host buffer on a copy stream as soon as its step is done (the reference's blocking `img.cpu()` per saved
        step, generate.py:195-196), so only the last image's copy is exposed.  use_graph / streams override the defaults;
        results are bit-identical for every setting (tests/test_gpu_model.py).

        Resource profile of the defaults (differs from a plain eager loop): the second lane owns a clone of both native
        handles -- its own workspace (sized for its share of the batch, so the total stays about the single-stream
        workspace: 6 GiB at B = 64 with vit-s + 12L/d512), its own captured graphs and its own handle-owned image buffer;
        the lanes are driven by a process-wide thread pool (one thread per lane, blocked in the native call between
        segments).  Opt out per call with streams=1 / use_graph=False, or process-wide with the environment variables
        PMHIP_GENERATE_STREAMS=1 and PMHIP_GENERATE_GRAPH=0 (read at every call).

        The returned tensors are views of ONE pinned host buffer [n_saved, B, C, H, W] that the package reuses once no
        tensor (or numpy alias) of an earlier call is alive: keeping one image keeps the whole buffer page-locked, and an
        asynchronous `.to('cuda', non_blocking=True)` of a returned image must be synchronised before the LAST reference to
        the list is dropped.  `.clone()` a result to own ordinary pageable memory, as the reference's `img.cpu()` returns.

        mask_padding (extension; False = the reference's behaviour: every row of the padded context is attended to, padding
        included): the text model is asked for the prompts' token counts (``text_model(text, return_lens=True)``) and every image's
        cross-attention sees its own tokens only.  context_lens gives the lengths explicitly instead (one per prompt).

        topk: any value in 1..n_embed, as in the reference, on the GPU as on the CPU; None = no top-k filter at all (the sampler of
        the MaskGIT / Muse papers), i.e. n_embed.

        choice_temperature (extension; None or 0 = the reference's behaviour: the least confident tokens are re-masked, a
        deterministic choice): MaskGIT's choice temperature (its default is 4.5).  Step s of T re-masks by ``log p +
        choice_temperature * (1 - (s + 1) / T) * gumbel``; the last step's noise is exactly zero.

        top_p (extension; None or 1.0 = no nucleus filter): 0 < top_p <= 1, the same for every step -- behind the top-k, the
        tokens are drawn from the smallest set of classes that holds ``top_p`` of the top-k's probability mass (``sample`` has
        the exact rule).  A mass cut follows the model from its flat early steps to its peaked late ones, which no fixed
        ``topk`` can; with ``topk=None`` it is the only filter."""
        B = len(text)
        if prompt_weights and context_weights is not None:
            raise ValueError("prompt_weights=True reads the weights from the prompts: no context_weights beside it")
        if regions is not None:
            if context_lens is not None or context_segments is not None or token_segments is not None:
                raise ValueError("regions builds the context's segments itself: no context_lens, context_segments or token_segments beside it")
            if context_weights is not None:
                raise ValueError("regions builds the context itself: no context_weights beside it (give a region a weight as its third element)")
            context, context_segments, token_segments, context_weights = self._region_context_weighted(text, regions, mask_padding, prompt_weights)
        elif prompt_weights:
            context, lens, context_weights = self.text_model(list(text), weighted=True)
            if context is None:
                raise ValueError("prompt_weights needs a text model (this pipeline is unconditional)")
            if mask_padding and context_lens is None and context_segments is None:
                context_lens = lens
        elif mask_padding and context_lens is None and context_segments is None:
            context, context_lens = self.text_model(text, return_lens=True)
        else:
            context = self.text_model(text)
        negative, negative_context_lens = self._negative_context(negative_text, B, mask_padding, negative_context_lens)
        opts = self._options(topk, top_p, guidance_scale, context_lens, choice_temperature, context, B, negative, negative_context_lens,
                             timesteps)
        keys = self._keys(context, B, opts, context_segments, token_segments, context_weights)
        if self._on_cpu():
            return self._generate_cpu(context, B, timesteps, temperature, opts, save_interval, seed, return_ids, keys)
        eng = self.engine()
        if seed is None:
            seed = _draw_seed()
        if use_graph is None:
            use_graph = os.environ.get("PMHIP_GENERATE_GRAPH", "1") != "0"
        if streams is None:
            # two lanes once one lane alone fills the chip (LANES_MIN_WORK above): at B = 8..20 ONE lane -- whose decode then overlaps
            # the next step's tower -- is 4-15 % faster than two; two lanes win from 33 (d512) / 22 (d768) / 17 (d1024) images
            streams = 2 if (self.compute_dtype == torch.bfloat16 and B * self.num_tokens * self._width >= LANES_MIN_WORK) else 1
            env_streams = os.environ.get("PMHIP_GENERATE_STREAMS")
            if env_streams:
                try:
                    streams = max(1, min(int(env_streams), B))   # never more lanes than images
                except ValueError:
                    pass                                          # not a number: keep the default
        flags = [step % save_interval == 0 for step in range(timesteps)]
        if context is not None:
            context = context.to(eng.device)
        if opts.negative is not None:
            opts = opts._replace(negative=opts.negative.to(eng.device))
        n_dec = sum(flags)
        if keep_on_device or n_dec == 0:
            ids, imgs = self.generate_ids(context, B, timesteps, temperature, opts, flags, seed, image_base=image_base,
                                          use_graph=use_graph, streams=streams, keys=keys)
            out = [] if imgs is None else list(imgs)
            return (out, ids) if return_ids else out
        vq = self.vqgan.engine()
        host = _pinned_pool.get((n_dec, B, vq.channels, vq.image_size, vq.image_size))

        n_lanes = len(streams) if isinstance(streams, (list, tuple)) else max(1, min(int(streams), B))
        cs = getattr(self, "_copy_streams", None)
        if cs is None or cs[0].device != eng.device:
            cs = self._copy_streams = []
        while len(cs) < n_lanes:
            cs.append(torch.cuda.Stream(device=eng.device))
        try:
            ids, _ = self.generate_ids(context, B, timesteps, temperature, opts, flags, seed, image_base=image_base,
                                       use_graph=use_graph, streams=streams, host=(host, cs), keys=keys)
        except BaseException:
            # a lane failed: whatever the other lanes queued may still be writing into `host`; drain it, and never hand
            # this buffer out again
            _pinned_pool.discard(host)
            try:
                torch.cuda.synchronize(eng.device)
            except Exception:
                pass
            raise
        finally:
            for c in cs[:n_lanes]:
                try:
                    c.synchronize()                          # every image has landed in the host buffer
                except Exception:
                    pass
        out = list(host)                                     # views of one pinned buffer; it is reused once all of them are gone
        return (out, ids) if return_ids else out

    def _negative_context(self, negative_text, B, mask_padding, negative_context_lens=None):
        """a negative prompt -- one string for every image or a list of B -- through the text model -> (its context [B, Ln, D], its
        lengths): with mask_padding the text model's own, unless the caller gave them; None: (None, the lengths as given)"""
        if negative_text is None:
            return None, negative_context_lens
        prompts = [negative_text] * B if isinstance(negative_text, str) else list(negative_text)
        if len(prompts) != B:
            raise ValueError(f"negative_text: {len(prompts)} prompts for a batch of {B}")
        if mask_padding and negative_context_lens is None:
            return self.text_model(prompts, return_lens=True)
        return self.text_model(prompts), negative_context_lens

    def _region_context(self, text, regions, mask_padding):
        """``generate(text, regions=)`` without prompt weights -> (context [B, Lmax, D], context_segments, token_segments); see
        ``_region_context_weighted``, whose first three results these are"""
        return self._region_context_weighted(text, regions, mask_padding)[:3]

    def _region_context_weighted(self, text, regions, mask_padding, prompt_weights=False):
        """``generate(text, regions=)`` -> (context [B, Lmax, D], context_segments, token_segments, context_weights): every prompt of
        every image goes through the text model in ONE call; with mask_padding a prompt contributes its non-pad rows only
        (``region_layout``).  context_weights (numpy float32 [B, Lmax]) is None unless a region carries a weight -- ``(prompt, mask,
        weight)`` -- or prompt_weights asks the text model for the weights of the words; a region's number multiplies its rows'."""
        B = len(text)
        if len(regions) != B:
            raise ValueError(f"regions: {len(regions)} lists for a batch of {B}")
        regions = [list(r) for r in regions]
        for b, r in enumerate(regions):
            if len(r) > MAX_REGIONS:
                raise ValueError(f"regions: image {b}: {len(r)} regions, at most {MAX_REGIONS} per image")
            for item in r:
                if not (isinstance(item, (tuple, list)) and len(item) in (2, 3) and isinstance(item[0], str)):
                    raise ValueError(f"regions: image {b}: every region is a (prompt, mask) pair")
                if len(item) == 3 and (isinstance(item[2], bool) or not isinstance(item[2], (int, float))):
                    raise ValueError(f"regions: image {b}: every region is a (prompt, mask) pair")
        prompts = [p for b in range(B) for p in [text[b]] + [item[0] for item in regions[b]]]
        weighted = prompt_weights or any(len(item) == 3 for r in regions for item in r)
        rows_w = None
        if prompt_weights:
            ctx, lens, rows_w = self.text_model(prompts, weighted=True)
            lens = ops.host_lens(lens, len(prompts), ctx.shape[1], "regions: prompt lengths") if mask_padding and ctx is not None else \
                ([ctx.shape[1]] * len(prompts) if ctx is not None else None)
        elif mask_padding:
            ctx, lens = self.text_model(prompts, return_lens=True)
            lens = ops.host_lens(lens, len(prompts), ctx.shape[1], "regions: prompt lengths")
        else:
            ctx = self.text_model(prompts)
            lens = [ctx.shape[1]] * len(prompts)
        if ctx is None:
            raise ValueError("regions needs a text model (this pipeline is unconditional)")
        contexts, at = [], 0
        for b in range(B):
            n = 1 + len(regions[b])
            contexts.append([ctx[at + i, :lens[at + i]] for i in range(n)])
            at += n
        context, ctx_seg, tok_seg = region_layout(contexts, [[item[1] for item in r] for r in regions], self.image_size, self.patch_size)
        if not weighted:
            return context, ctx_seg, tok_seg, None
        ctx_w = np.ones(ctx_seg.shape, np.float32)                # (rows behind an image's last prompt are padding: any weight will do)
        at = 0
        for b in range(B):
            col = 0
            for i in range(1 + len(regions[b])):
                n = lens[at + i]
                w = np.ones(n, np.float32) if rows_w is None else np.asarray(rows_w[at + i, :n], np.float32)
                if i > 0 and len(regions[b][i - 1]) == 3:
                    w = w * np.float32(regions[b][i - 1][2])
                ctx_w[b, col:col + n] = w
                col += n
            at += 1 + len(regions[b])
        return context, ctx_seg, tok_seg, ctx_w

    def _region_loop(self, img, coord, text, timesteps, topk, temperature, keep_inside, seed=None, return_ids=False,
                     choice_temperature=None, top_p=None):
        # the values are checked before anything runs (a region loop has neither guidance nor context lengths: no context needed)
        opts = self._options(topk, top_p, None, None, choice_temperature, None, 0)
        if seed is None:
            seed = _draw_seed()                 # one stream per call; the step index separates the steps
        z, ids, text = self.to_latent(img, text)
        s = self.patch_size
        x, y, h, w = coord[0] // s, coord[1] // s, coord[2] // s, coord[3] // s
        g = self.image_size // s
        keep = torch.zeros(g, g, dtype=torch.bool, device=ids.device) if keep_inside else \
            torch.ones(g, g, dtype=torch.bool, device=ids.device)
        keep[y:y + h, x:x + w] = keep_inside
        keep = keep.reshape(1, -1)
        # the reference builds this with float arithmetic (ids*mask + id*(1-mask), generate.py:210,229),
        # which yields a float tensor that nn.Embedding rejects; the intended integer result is used here
        ids = torch.where(keep, ids, torch.full_like(ids, self.mask_token_id))
        if timesteps >= 2 and not self._on_cpu():
            # more than the reference's default single step: the native decode loop (graph replay by default, like generate()) from
            # these start ids, decoding only the last step -- bit-identical to the per-step composition below (tests/test_gpu_model.py)
            use_graph = os.environ.get("PMHIP_GENERATE_GRAPH", "1") != "0"
            ids, imgs = self.generate_ids(text, ids.shape[0], timesteps, temperature, opts, [False] * (timesteps - 1) + [True], seed,
                                          use_graph=use_graph, streams=1, ids0=ids)
            return (imgs[0], ids) if return_ids else imgs[0]
        return self._region_steps(ids, text, timesteps, opts, temperature, seed, return_ids)

    def _region_steps(self, ids, text, timesteps, topk, temperature, seed, return_ids=False, choice_temperature=None, top_p=None):
        """the region loop as the reference writes it: one step of ``sample`` per step (generate.py:211-216,230-235)"""
        out = None
        opts = self._options(topk, top_p, None, None, choice_temperature, text, ids.shape[0])
        temps, nmask, ctemps = loop_schedule(timesteps, temperature, self.num_tokens, opts.choice_temperature)
        for step in range(timesteps):
            ids, out = self._step(ids, nmask[step], text, opts, temps[step], ctemps[step] if ctemps else 0.0, seed=seed, step=step)
        return (out, ids) if return_ids else out

    def _edit_masks(self, img, mask, token_mask):
        """the masks of an ``edit`` call, checked -> (token mask bool [B, g, g] or None, pixel mask uint8 [B, H, W]); with a token
        mask the pixel mask is that of its patches"""
        if (mask is None) == (token_mask is None):
            raise ValueError("edit: give exactly one of mask (pixels) and token_mask (tokens)")
        if img.dim() != 4:
            raise ValueError(f"edit: img must be [B, C, H, W], got {tuple(img.shape)}")
        B, _, H, W = img.shape
        if H != self.image_size or W != self.image_size:
            raise ValueError(f"edit: img must be {self.image_size} x {self.image_size}, got {H} x {W}")
        p = self.patch_size
        g = self.image_size // p
        if token_mask is not None:
            tm = torch.as_tensor(token_mask)
            if tm.dtype != torch.bool or tuple(tm.shape) not in ((B, g, g), (g, g)):
                raise ValueError(f"edit: token_mask must be a bool [{B}, {g}, {g}] or [{g}, {g}] tensor, got {tm.dtype} {tuple(tm.shape)}")
            tm = tm.to(img.device).expand(B, g, g)
            return tm, tm.repeat_interleave(p, 1).repeat_interleave(p, 2).to(torch.uint8).contiguous()
        pm = torch.as_tensor(mask)
        if tuple(pm.shape) == (B, 1, H, W):
            pm = pm[:, 0]
        if tuple(pm.shape) not in ((B, H, W), (H, W)):
            raise ValueError(f"edit: mask must be [{B}, {H}, {W}], [{B}, 1, {H}, {W}] or [{H}, {W}], got {tuple(pm.shape)}")
        return None, (pm.to(img.device) != 0).expand(B, H, W).to(torch.uint8).contiguous()

    def _masked_ids(self, ids, token_mask, pixel_mask):
        """ids [B, N] and the masks of ``_edit_masks`` -> (ids with the mask id where a token is regenerated, counts [B]: how many per
        image, on the device of the mask that counted them).  A pixel mask without a token mask marks a token iff any pixel of its patch is set: the mask operator
        on the GPU, its rule in plain torch on the CPU."""
        B = ids.shape[0]
        if token_mask is None and not self._on_cpu():
            return ops.mask_tokens(pixel_mask.to(ids.device), self.patch_size, ids, self.mask_token_id)
        if token_mask is None:
            p = self.patch_size
            token_mask = pixel_mask.reshape(B, pixel_mask.shape[1] // p, p, pixel_mask.shape[2] // p, p).amax(dim=(2, 4)) != 0
        tm = token_mask.reshape(B, -1)
        return torch.where(tm.to(ids.device), torch.full_like(ids, self.mask_token_id), ids), tm.sum(1)       # (counted where the mask is)

    def edit_ids(self, ids, counts, context, timesteps, temperature, opts, seed, image_base=0, use_graph=False, keys=None):
        """the EDIT loop on device tensors (pmhip_pipeline_generate_edit): ids int64 [B, N] with the mask id where a token is
        regenerated, counts = how many per image (a list of B ints), opts the call's ``_Options``.  Step t re-masks
        ``edit_schedule(counts[b], timesteps)[t]`` positions of image b; the last step is decoded, from the merged ids.
        -> (final ids [B, N], image [B, C, H, W]); ``ids`` is left as it is.  keys: the call's ``ops.Keys`` (None: those of opts alone)."""
        eng = self.engine()
        B = ids.shape[0]
        if keys is None:
            keys = self._keys(context, B, opts)
        temps, _, ctemps = loop_schedule(timesteps, temperature, self.num_tokens, opts.choice_temperature)
        per_image = [edit_schedule(m, timesteps) for m in counts]
        table = [[per_image[b][t] for b in range(B)] for t in range(timesteps)]
        kw = {}
        if opts.negative is not None or opts.guidance_scales is not None:
            kw.update(negative_context=opts.negative, negative_lens=opts.negative_lens, guidance_scales=opts.guidance_scales)
        ids = self._start_ids(B, ids, eng.device)
        ids, imgs = eng.generate(self.vqgan.engine(), ids, context, temps, None, [False] * (timesteps - 1) + [True], opts.topk, seed=seed,
                                 image_base=image_base, use_graph=use_graph, guidance_scale=opts.guidance_scale, choice_temps=ctemps,
                                 top_p=opts.top_p, nmask_img=table, keys=keys, **kw)
        return ids, imgs[0]

    @torch.no_grad()
    def edit(self, img, mask=None, text=None, timesteps=8, temperature=1.0, topk=5, seed=None, image_base=0, token_mask=None,
             guidance_scale=None, negative_text=None, mask_padding=False, context_lens=None, choice_temperature=None, top_p=None,
             preserve="tokens", return_ids=False):
        """Regenerate a free-form region of ``img`` [B, C, H, W] in [-1, 1] and KEEP the rest: the region-preserving call beside the
        reference-shaped ``inpaint`` / ``outpaint``.

        ``mask``: a bool / uint8 / float tensor [B, H, W], [B, 1, H, W] or [H, W] (every image), non-zero = regenerate; a token is
        regenerated iff ANY pixel of its patch is.  ``token_mask``: a bool [B, g, g] or [g, g] tensor over the token grid instead.
        Exactly one of the two.  Every image has its own mask, area and schedule: step s of image b re-masks
        ``edit_schedule(m_b, timesteps)[s]`` of ITS m_b tokens, so a kept token is never re-masked, the last step leaves no mask
        id behind, and the image is decoded from the merged ids -- a kept token decodes from its own id.  An image whose mask is
        empty comes back as ``decode(encode(img))``.

        ``text``: the prompts (what ``inpaint`` takes).  ``guidance_scale`` (a number or one per step), ``negative_text``,
        ``mask_padding`` / ``context_lens``, ``topk`` (None included), ``top_p``, ``choice_temperature``, ``temperature``, ``seed``,
        ``image_base``: as in ``generate``.

        ``preserve``: "tokens" returns the decode as it is (a kept token's pixels are the decoder's reconstruction of them);
        "pixels" puts the ORIGINAL pixels back outside the pixel mask (with ``token_mask``: outside its patches).

        -> the image batch on the pipeline's device, like ``inpaint``; with ``return_ids`` (image, final ids)."""
        if preserve not in ("tokens", "pixels"):
            raise ValueError(f"edit: preserve must be 'tokens' or 'pixels', got {preserve!r}")
        tm, pm = self._edit_masks(img, mask, token_mask)
        B = img.shape[0]
        if exists(text):
            if mask_padding and context_lens is None:
                context, context_lens = self.text_model(text, return_lens=True)
            else:
                context = self.text_model(text)
        elif negative_text is not None:
            raise ValueError("negative_text needs a text condition (text=None IS the unconditional branch)")
        else:
            context = None
        negative, negative_lens = self._negative_context(negative_text, B, mask_padding)
        opts = self._options(topk, top_p, guidance_scale, context_lens, choice_temperature, context, B, negative, negative_lens, timesteps)
        _, ids, _ = self.to_latent(img)
        ids = ids.reshape(B, self.num_tokens)
        keys = self._keys(context, B, opts)
        if self._on_cpu():
            ids, counts = self._masked_ids(ids, tm, pm)
            counts = counts.tolist()
            temps, _, ctemps = loop_schedule(timesteps, temperature, self.num_tokens, opts.choice_temperature)
            per_image = [edit_schedule(m, timesteps) for m in counts]
            for step in range(timesteps):
                ids, _ = self._sample_cpu(ids, 0, context, opts.topk, temps[step], None, None if seed is None else seed + step,
                                          opts.step_scale(step), keys, ctemps[step] if ctemps else 0.0, None, opts.top_p,
                                          opts.negative, opts.negative_lens, counts=[sched[step] for sched in per_image])
            out = self.vqgan.decode_from_indice(ids)
            if preserve == "pixels":
                out = torch.where(pm[:, None] != 0, out, img.to(out.dtype))
            return (out, ids) if return_ids else out
        eng = self.engine()
        if seed is None:
            seed = _draw_seed()
        ids = ids.to(eng.device, torch.long).clone(memory_format=torch.contiguous_format)
        ids, counts = self._masked_ids(ids, tm, pm)
        counts = counts.tolist()                               # the one device-to-host copy of the call: B counts
        if context is not None:
            context = context.to(eng.device)
        if opts.negative is not None:
            opts = opts._replace(negative=opts.negative.to(eng.device))
        use_graph = os.environ.get("PMHIP_GENERATE_GRAPH", "1") != "0"
        ids, out = self.edit_ids(ids, counts, context, timesteps, temperature, opts, seed, image_base=image_base, use_graph=use_graph, keys=keys)
        if preserve == "pixels":
            out = ops.composite(out, img.to(eng.device, torch.float32).contiguous(), pm.to(eng.device), out=out)
        return (out, ids) if return_ids else out

    @torch.no_grad()
    def diff_edit(self, img, text, edit_text, *, mask_ratio=0.5, draws=4, diff_seed=0, kind="tv", threshold=0.5, grow=1, return_mask=False,
                  **edit_kwargs):
        """MASK-FREE EDITING (extension): ``img`` with the caption ``text`` becomes ``edit_text`` where the two
        prompts disagree about it, and stays as it is elsewhere.  The body is
            mask = diff_mask(img, text, edit_text, mask_ratio, draws, diff_seed, kind, threshold, grow, mask_padding)
            edit(img, token_mask=mask, text=edit_text, **edit_kwargs)
        and the result is bit-identical to those two calls made by hand (``mask_padding``, if among ``edit_kwargs``, goes to both).
        ``edit_kwargs``: ``edit``'s keywords (timesteps, seed, guidance_scale, ...; not mask / token_mask).  An image whose
        mask is empty -- the prompts agree -- comes back as ``edit`` returns it: ``decode(encode(img))``.  -> what ``edit`` returns;
        with ``return_mask`` that and the mask, bool [B, g, g].

        The same mask serves the pair loop: ``prompt_to_prompt(text, edit_text, img=photo, blend_mask=pipe.diff_mask(photo, text,
        edit_text))`` is prompt-to-prompt on a photograph with no phrase to point at."""
        for k in ("mask", "token_mask"):
            if k in edit_kwargs:
                raise ValueError(f"diff_edit: {k} is not a keyword here (the mask follows from the prompts)")
        mask = self.diff_mask(img, text, edit_text, mask_ratio=mask_ratio, draws=draws, seed=diff_seed, kind=kind, threshold=threshold,
                              grow=grow, mask_padding=edit_kwargs.get("mask_padding", False))
        out = self.edit(img, token_mask=mask, text=edit_text, **edit_kwargs)
        return (out, mask) if return_mask else out

    @torch.no_grad()
    def inpaint(self, img, coord, text=None, timesteps=1, topk=1, temperature=0, seed=None, return_ids=False, choice_temperature=None,
                top_p=None):
        """re-generate the rectangle coord=(x,y,h,w) in pixels (generate.py:200-217).  choice_temperature: as in ``generate`` (the
        kept region's ids are given: the noise never prefers one of them to a position the loop took).  topk: 1..n_embed, or
        None = no filter, as in ``generate``.  top_p: the nucleus mass, as in ``generate``.
        This reproduces the reference's loop, which re-masks and re-predicts the kept region; ``edit`` is the region-preserving call."""
        return self._region_loop(img, coord, text, timesteps, topk, temperature, keep_inside=False, seed=seed,
                                 return_ids=return_ids, choice_temperature=choice_temperature, top_p=top_p)

    @torch.no_grad()
    def outpaint(self, img, coord, text=None, timesteps=1, topk=1, temperature=0, seed=None, return_ids=False, choice_temperature=None,
                 top_p=None):
        """keep the rectangle, re-generate everything else (generate.py:219-236).  choice_temperature, topk, top_p: as in ``inpaint``.
        This reproduces the reference's loop, which re-masks and re-predicts the kept region; ``edit`` is the region-preserving call."""
        return self._region_loop(img, coord, text, timesteps, topk, temperature, keep_inside=True, seed=seed,
                                 return_ids=return_ids, choice_temperature=choice_temperature, top_p=top_p)
