"""Text-conditioning producers (reference modules/encoder.py:18-104): the frozen towers are third-party
pretrained models that stay on stock PyTorch-ROCm; the hot path only consumes their (B,77,ctx) output.  The one exception is opt-in:
``T5TextEmbedder(native=True)`` runs the Flan-T5 encoder's arithmetic on the HIP kernels (``modules/t5_native.py``), and
``CLIPTextEmbedder(native=True)`` the OpenCLIP text tower's (``modules/clip_native.py``).

Both wrappers keep the reference's attribute names (`transformer` for the T5 encoder, `model` for the CLIP tower),
because those names are the checkpoint-key contract: a Pipeline state_dict carries `text_model.transformer.*`
(T5) or `text_model.model.*` (CLIP).  Unlike the reference, the device follows the module (`.to()`), there is no
hard-coded "cuda" (reference encoder.py:19,36,57,80), and a pre-built tower / tokenizer can be injected, which is how
the tests run them with randomly initialised weights (there is no network here).
"""
import torch
import torch.nn as nn

CLIP_ARCH = 'ViT-L-14'                  # reference encoder.py:14-15
CLIP_VERSION = 'laion2b_s32b_b82k'


def _module_device(module):
    return next(module.parameters()).device


def _pad_id(tokenizer):
    pad = getattr(tokenizer, "pad_token_id", None)
    return 0 if pad is None else int(pad)                  # T5's pad token is id 0


def _count_tokens(mask):
    """[B, L] non-pad mask -> int32 [B] on the host: the non-pad token count of every prompt, at least 1 (an empty prompt still
    attends to one row: a softmax over nothing has no value)"""
    return mask.to(torch.int64).sum(-1).clamp_(min=1).to(torch.int32).cpu()


class T5TextEmbedder(nn.Module):
    """Flan-T5 encoder (reference encoder.py:18-42): tokens padded / truncated to max_length -> last_hidden_state."""

    def __init__(self, version="google/flan-t5-xl", device=None, max_length=77, freeze=True, tokenizer=None, transformer=None,
                 native=False, encoder_padding_mask=False):
        """native: run the tower's arithmetic on the HIP kernels (``modules/t5_native.py``) when it lives on a
        GPU -- on the CPU the Hugging Face tower runs, as everywhere in this package.  A tower the kernels do not serve is refused
        here (ValueError naming the config field).  Off (the default): the Hugging Face tower, as before.
        encoder_padding_mask: the tower is given the prompts' non-pad token counts, what Hugging Face users normally do
        (``attention_mask=``).  Off (the default): the reference's behaviour -- padding attends and is attended to."""
        super().__init__()
        if tokenizer is None or transformer is None:
            from transformers import T5EncoderModel, T5Tokenizer   # needs local weights: there is no network here
            tokenizer = tokenizer or T5Tokenizer.from_pretrained(version)
            transformer = transformer or T5EncoderModel.from_pretrained(version)
        self.tokenizer = tokenizer
        self.transformer = transformer
        self.max_length = max_length
        self.encoder_padding_mask = bool(encoder_padding_mask)
        self._pm_dtype = torch.float32
        self._native = None
        if native:
            self.use_native(True)
        if device is not None:
            self.to(device)
        if freeze:
            self.freeze()

    def use_native(self, on=True):
        """switch the HIP tower on or off; -> self"""
        if on and self._native is None:
            from .t5_native import NativeT5Encoder
            self._native = NativeT5Encoder(self.transformer)       # refuses what the kernels do not serve
        elif not on:
            self._native = None
        return self

    @property
    def native(self):
        return self._native is not None

    @property
    def compute_dtype(self):
        """of the native tower (the Hugging Face tower computes in its parameters' dtype): ``_pm_dtype`` (``Pipeline.set_compute_dtype``),
        or bfloat16 inside ``torch.autocast('cuda', bfloat16)``"""
        if torch.is_autocast_enabled('cuda') and torch.get_autocast_dtype('cuda') == torch.bfloat16:
            return torch.bfloat16
        return self._pm_dtype

    def _tower(self, tokens, lens):
        """THE tower call of forward, _forward_weighted, phrase_rows and fragment_ids: tokens int64 [B, max_length] on the tower's
        device, lens int32 [B] on the host (read only with encoder_padding_mask) -> last_hidden_state [B, max_length, d_model]"""
        lens = lens if self.encoder_padding_mask else None
        if self._native is not None and tokens.is_cuda:
            if self._native.model is not self.transformer:          # the tower was replaced after use_native()
                self._native = None
                self.use_native(True)
            return self._native(tokens, kv_lens=lens, dtype=self.compute_dtype)
        if lens is None:
            return self.transformer(input_ids=tokens).last_hidden_state
        keep = torch.arange(tokens.shape[1])[None, :] < torch.as_tensor(lens).to(torch.long)[:, None]
        return self.transformer(input_ids=tokens, attention_mask=keep.to(device=tokens.device, dtype=torch.long)).last_hidden_state

    def freeze(self):
        self.transformer = self.transformer.eval()
        for param in self.parameters():
            param.requires_grad = False

    @torch.no_grad()
    def forward(self, text, return_lens=False, weighted=False):
        """-> context (B, max_length, d_model), every position as in the reference (no mask is passed to the encoder).
        return_lens: -> (context, lens), lens[b] = the number of non-pad tokens of prompt b (the end-of-sequence token counts;
        at least 1), for ``Pipeline.generate(mask_padding=True)`` / ``context_lens=``.
        weighted: the prompts carry emphasis syntax (``paintmind_amd.prompt``) -> (context, lens, weights), weights float32
        [B, max_length] on the host, one per context row: see ``_forward_weighted``."""
        if weighted:
            return self._forward_weighted(text)
        enc = self.tokenizer(text, truncation=True, max_length=self.max_length, return_length=True,
                             return_overflowing_tokens=False, padding="max_length", return_tensors="pt")
        ids = enc["input_ids"]
        tokens = ids.to(_module_device(self.transformer))
        mask = enc["attention_mask"] if "attention_mask" in enc else ids != _pad_id(self.tokenizer)
        lens = _count_tokens(torch.as_tensor(mask))
        context = self._tower(tokens, lens)
        return (context, lens) if return_lens else context

    def _forward_weighted(self, text):
        """Every prompt is parsed (``prompt.parse_weighted``), its fragments are tokenised one by one WITHOUT special tokens, the ids
        are concatenated, closed with the end-of-sequence id and truncated (the end-of-sequence id stays last) or padded to
        max_length; the context is ONE tower call on those ids -- the words see each other as in an unweighted prompt, only the
        syntax is gone.  Row j of prompt b carries the weight of the fragment its token came from; the end-of-sequence row and the
        padding rows carry 1."""
        from ..prompt import parse_weighted
        eos = getattr(self.tokenizer, "eos_token_id", None)
        eos = 1 if eos is None else int(eos)                   # T5's end-of-sequence token is id 1
        pad = _pad_id(self.tokenizer)
        B, L = len(text), self.max_length
        ids = torch.full((B, L), pad, dtype=torch.long)
        weights = torch.ones(B, L, dtype=torch.float32)
        lens = torch.zeros(B, dtype=torch.int32)
        for b, prompt in enumerate(text):
            row, wrow = [], []
            for frag, w in parse_weighted(prompt):
                piece = self.tokenizer(frag, add_special_tokens=False)["input_ids"]
                piece = [int(t) for t in (piece.reshape(-1).tolist() if hasattr(piece, "reshape") else piece)]
                row += piece
                wrow += [float(w)] * len(piece)
            row, wrow = row[:L - 1] + [eos], wrow[:L - 1] + [1.0]
            ids[b, :len(row)] = torch.tensor(row, dtype=torch.long)
            weights[b, :len(row)] = torch.tensor(wrow, dtype=torch.float32)
            lens[b] = len(row)
        context = self._tower(ids.to(_module_device(self.transformer)), lens)
        return context, lens, weights

    @torch.no_grad()
    def phrase_rows(self, text, phrases):
        """Which context rows are a phrase's tokens (``Pipeline.phrase_mask``).  Prompt b is split at the SINGLE
        occurrence of phrases[b] into [before, phrase, after]; the three fragments are tokenised one by one WITHOUT special tokens,
        exactly as ``_forward_weighted`` tokenises its fragments, the ids are concatenated, closed with the end-of-sequence id and
        truncated or padded to max_length, and the context is ONE tower call on them.
        -> (context (B, max_length, d_model), lens int32 [B] on the host, rows bool [B, max_length] on the host: the phrase's tokens).
        A phrase that is empty, absent, occurs twice or is cut off by max_length raises ValueError naming the prompt."""
        text = [text] if isinstance(text, str) else list(text)
        phrases = [phrases] * len(text) if isinstance(phrases, str) else list(phrases)
        if len(phrases) != len(text):
            raise ValueError(f"phrase_rows: {len(phrases)} phrases for {len(text)} prompts")
        eos = getattr(self.tokenizer, "eos_token_id", None)
        eos = 1 if eos is None else int(eos)
        pad = _pad_id(self.tokenizer)
        B, L = len(text), self.max_length
        ids = torch.full((B, L), pad, dtype=torch.long)
        rows = torch.zeros(B, L, dtype=torch.bool)
        lens = torch.zeros(B, dtype=torch.int32)

        def pieces(frag):
            if not frag:
                return []
            piece = self.tokenizer(frag, add_special_tokens=False)["input_ids"]
            return [int(t) for t in (piece.reshape(-1).tolist() if hasattr(piece, "reshape") else piece)]

        for b, (prompt, phrase) in enumerate(zip(text, phrases)):
            if not isinstance(phrase, str) or not phrase.strip():
                raise ValueError(f"phrase_rows: prompt {b} ({prompt!r}): the phrase is empty")
            count = prompt.count(phrase)
            if count == 0:
                raise ValueError(f"phrase_rows: prompt {b} ({prompt!r}): the phrase {phrase!r} does not occur in it")
            if count > 1:
                raise ValueError(f"phrase_rows: prompt {b} ({prompt!r}): the phrase {phrase!r} occurs {count} times, not once")
            before, after = prompt.split(phrase)
            head, mid, tail = pieces(before), pieces(phrase), pieces(after)
            if not mid:
                raise ValueError(f"phrase_rows: prompt {b} ({prompt!r}): the phrase {phrase!r} has no tokens")
            if len(head) + len(mid) > L - 1:
                raise ValueError(f"phrase_rows: prompt {b} ({prompt!r}): the phrase {phrase!r} is cut off by max_length={L} "
                                 f"(its tokens end at row {len(head) + len(mid)}, the last row is the end-of-sequence token's)")
            row = (head + mid + tail)[:L - 1] + [eos]
            ids[b, :len(row)] = torch.tensor(row, dtype=torch.long)
            rows[b, len(head):len(head) + len(mid)] = True
            lens[b] = len(row)
        context = self._tower(ids.to(_module_device(self.transformer)), lens)
        return context, lens, rows

    @torch.no_grad()
    def fragment_ids(self, fragments):
        """Token ids without a second tower call (``Pipeline.prompt_to_prompt``).  fragments[b]: the strings
        prompt b is cut into (their concatenation is the prompt).  They are tokenised one by one WITHOUT special tokens, exactly as
        ``phrase_rows`` and ``_forward_weighted`` tokenise theirs, the ids are concatenated, closed with the end-of-sequence id and
        truncated or padded to max_length, and the context is ONE tower call on them -- so a fragment that is a phrase sits in the rows
        ``phrase_rows`` finds for it.
        -> (context (B, max_length, d_model), lens int32 [B] on the host, ids: per prompt the list of its lens[b] token ids, spans: per
        prompt the (first row, row behind the last) of every fragment, cut off at the end-of-sequence row)"""
        eos = getattr(self.tokenizer, "eos_token_id", None)
        eos = 1 if eos is None else int(eos)
        pad = _pad_id(self.tokenizer)
        B, L = len(fragments), self.max_length
        ids = torch.full((B, L), pad, dtype=torch.long)
        lens = torch.zeros(B, dtype=torch.int32)
        rows, spans = [], []
        for b, frags in enumerate(fragments):
            row, span = [], []
            for frag in frags:
                piece = self.tokenizer(frag, add_special_tokens=False)["input_ids"] if frag else []
                piece = [int(t) for t in (piece.reshape(-1).tolist() if hasattr(piece, "reshape") else piece)]
                span.append((min(len(row), L - 1), min(len(row) + len(piece), L - 1)))
                row += piece
            row = row[:L - 1] + [eos]
            ids[b, :len(row)] = torch.tensor(row, dtype=torch.long)
            lens[b] = len(row)
            rows.append(row)
            spans.append(span)
        context = self._tower(ids.to(_module_device(self.transformer)), lens)
        return context, lens, rows, spans

    def encode(self, text):
        return self(text)


class CLIPTextEmbedder(nn.Module):
    """OpenCLIP text tower (reference encoder.py:45-104).  layer="last": every residual block, then ln_final;
    layer="penultimate": the last block is skipped (ln_final still applied).  Output (B, 77, width), all positions.

    Written against the open_clip model interface: `token_embedding`, `positional_embedding`, `transformer.resblocks`
    (each block called as block(x, attn_mask=...) on sequence-first tensors), `attn_mask`, `ln_final`."""
    LAYERS = ("last", "penultimate")

    def __init__(self, arch=CLIP_ARCH, version=CLIP_VERSION, device=None, max_length=77, layer="last", precision='fp32',
                 freeze=True, model=None, tokenizer=None, native=False):
        """native: run the tower's arithmetic on the HIP kernels (``modules/clip_native.py``) when it lives on
        a GPU -- on the CPU the stock tower runs, as everywhere in this package.  A tower the kernels do not serve is refused here
        (ValueError naming what is wrong).  Off (the default): the stock tower, as before."""
        super().__init__()
        if layer not in self.LAYERS:
            raise ValueError(f"layer must be one of {self.LAYERS}, got {layer!r}")
        if model is None or tokenizer is None:
            try:
                import open_clip
            except ImportError as e:                    # the tower is optional: only this class needs the package
                raise ImportError("CLIPTextEmbedder needs the open_clip package (or pass model= and tokenizer=)") from e
            if model is None:
                model = open_clip.create_model(arch, pretrained=version, precision=precision)
                if hasattr(model, "visual"):
                    del model.visual                    # the image tower is never used here
            tokenizer = tokenizer or open_clip.tokenize
        self.model = model
        self.tokenize = tokenizer
        self.max_length = max_length
        self.layer = layer
        self.skip_last = {"last": 0, "penultimate": 1}[layer]
        self._pm_dtype = torch.float32
        self._native = None
        if native:
            self.use_native(True)
        if device is not None:
            self.to(device)
        if freeze:
            self.freeze()

    def use_native(self, on=True):
        """switch the HIP tower on or off; -> self"""
        if on and self._native is None:
            from .clip_native import NativeClipText
            self._native = NativeClipText(self.model, self.skip_last)       # refuses what the kernels do not serve
        elif not on:
            self._native = None
        return self

    @property
    def native(self):
        return self._native is not None

    @property
    def compute_dtype(self):
        """of the native tower (the stock tower computes in its parameters' dtype): ``_pm_dtype`` (``Pipeline.set_compute_dtype``), or
        bfloat16 inside ``torch.autocast('cuda', bfloat16)``"""
        if torch.is_autocast_enabled('cuda') and torch.get_autocast_dtype('cuda') == torch.bfloat16:
            return torch.bfloat16
        return self._pm_dtype

    def freeze(self):
        self.model = self.model.eval()
        for param in self.parameters():
            param.requires_grad = False

    @torch.no_grad()
    def forward(self, text, return_lens=False, weighted=False):
        """return_lens: -> (context, lens), lens[b] = the number of non-pad tokens of prompt b (open_clip pads with 0; the
        start and end tokens count), for ``Pipeline.generate(mask_padding=True)`` / ``context_lens=``.
        weighted: not served -- the byte-pair tokenizer of this tower is not written for fragments."""
        if weighted:
            raise NotImplementedError("CLIPTextEmbedder serves no prompt weights (weighted=True): T5TextEmbedder does")
        tokens = self.tokenize(text)
        context = self.encode_with_transformer(tokens.to(_module_device(self.model)))
        return (context, _count_tokens(tokens != 0)) if return_lens else context

    def phrase_rows(self, text, phrases):
        raise NotImplementedError("CLIPTextEmbedder serves no phrase rows (phrase_rows): T5TextEmbedder does")

    def fragment_ids(self, fragments):
        raise NotImplementedError("CLIPTextEmbedder serves no token ids (fragment_ids): T5TextEmbedder does")

    def encode_with_transformer(self, tokens):
        """THE tower call: tokens int64 [B, n_ctx] on the tower's device -> [B, n_ctx, width]"""
        if self._native is not None and tokens.is_cuda:
            if self._native.model is not self.model:                # the tower was replaced after use_native()
                self._native = None
                self.use_native(True)
            return self._native(tokens, dtype=self.compute_dtype)
        m = self.model
        x = m.token_embedding(tokens) + m.positional_embedding          # (B, n_ctx, width)
        blocks = list(m.transformer.resblocks)
        blocks = blocks[:len(blocks) - self.skip_last]
        mask = getattr(m, "attn_mask", None)
        seq_first = not getattr(m.transformer, "batch_first", False)   # older open_clip blocks are sequence-first
        if seq_first:
            x = x.permute(1, 0, 2)
        for blk in blocks:
            x = blk(x, attn_mask=mask)
        if seq_first:
            x = x.permute(1, 0, 2)
        return m.ln_final(x)

    def encode(self, text):
        return self(text)


class NullTextEmbedder(nn.Module):
    """Unconditional generation through the drop-in API: the context is None, so attn2 runs as a second self-attention
    (reference modules/attention.py:47).  BASELINE.json configs[2] is this path."""

    def forward(self, text, return_lens=False, weighted=False):
        if weighted:
            return None, None, None
        return (None, None) if return_lens else None


class SyntheticTextEmbedder(nn.Module):
    """Deterministic stand-in used by the benches and tests: N(0,1) features keyed by (seed, prompt index).

    Row i of the output depends only on (seed, base_index + i), so sharding a prompt list over ranks
    yields the same features as a single process.
    """

    def __init__(self, context_dim, max_length=77, seed=1234):
        super().__init__()
        self.context_dim, self.max_length, self.seed = context_dim, max_length, seed
        self.base_index = 0
        self.register_buffer("_anchor", torch.zeros(1), persistent=False)

    def forward(self, text, return_lens=False, weighted=False):
        """return_lens: every row is a feature (there is no tokenizer and no padding): lens = max_length for every prompt.
        weighted: the emphasis syntax is parsed (so a malformed prompt is refused) and dropped; -> (context, lens, weights of 1)"""
        if weighted:
            from ..prompt import strip_weights
            context, lens = self.forward([strip_weights(t) for t in text], return_lens=True)
            return context, lens, torch.ones(len(text), self.max_length, dtype=torch.float32)
        if return_lens:
            return self.forward(text), torch.full((len(text),), self.max_length, dtype=torch.int32)
        rows = []
        for i in range(len(text)):
            g = torch.Generator().manual_seed(self.seed * 1000003 + self.base_index + i)
            rows.append(torch.randn(self.max_length, self.context_dim, generator=g))
        return torch.stack(rows).to(self._anchor.device)

    def phrase_rows(self, text, phrases):
        raise NotImplementedError("SyntheticTextEmbedder has no tokenizer and serves no phrase rows (phrase_rows): T5TextEmbedder does")

    def fragment_ids(self, fragments):
        raise NotImplementedError("SyntheticTextEmbedder has no tokenizer and serves no token ids (fragment_ids): T5TextEmbedder does")
