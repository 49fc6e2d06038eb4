"""A randomly initialised stand-in for an OpenCLIP text tower in a shape the HIP path serves (heads * 64 == width, MLP ratio 4), with
the open_clip text contract: ``token_embedding``, ``positional_embedding``, ``transformer.resblocks`` (sequence-first blocks of ``ln_1,
attn, ls_1, ln_2, mlp(c_fc, gelu, c_proj), ls_2``), ``attn_mask`` (causal), ``ln_final``.  No network, no pretrained weights; not a
conftest, not collected."""
from collections import OrderedDict

import torch
import torch.nn as nn


class QuickGELU(nn.Module):
    """open_clip's: x * sigmoid(1.702 x)"""

    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class Block(nn.Module):
    def __init__(self, width, quick):
        super().__init__()
        self.ln_1 = nn.LayerNorm(width)
        self.attn = nn.MultiheadAttention(width, width // 64)
        self.ls_1 = nn.Identity()
        self.ln_2 = nn.LayerNorm(width)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(width, 4 * width)), ("gelu", QuickGELU() if quick else nn.GELU()),
                                              ("c_proj", nn.Linear(4 * width, width))]))
        self.ls_2 = nn.Identity()

    def forward(self, x, attn_mask=None):                      # sequence-first, like open_clip's ResidualAttentionBlock
        h = self.ln_1(x)
        x = x + self.ls_1(self.attn(h, h, h, need_weights=False, attn_mask=attn_mask)[0])
        return x + self.ls_2(self.mlp(self.ln_2(x)))


class Transformer(nn.Module):
    def __init__(self, width, layers, quick):
        super().__init__()
        self.resblocks = nn.ModuleList([Block(width, quick) for _ in range(layers)])
        self.grad_checkpointing = False


class ClipTextTower(nn.Module):
    def __init__(self, width=128, layers=2, quick=False, n_ctx=77, vocab=256, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.token_embedding = nn.Embedding(vocab, width)
        self.positional_embedding = nn.Parameter(0.01 * torch.randn(n_ctx, width))
        self.transformer = Transformer(width, layers, quick)
        self.ln_final = nn.LayerNorm(width)
        self.register_buffer("attn_mask", torch.full((n_ctx, n_ctx), float("-inf")).triu_(1), persistent=False)
        with torch.no_grad():                                  # non-trivial biases and LayerNorm parameters
            for p in self.parameters():
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn(p.shape))


def clip_tower(width=128, layers=2, quick=False, n_ctx=77, seed=0):
    return ClipTextTower(width, layers, quick, n_ctx, seed=seed).eval()


class Tokenizer:
    """open_clip.tokenize's contract: a list of strings -> int64 [B, n_ctx], 0 is padding, start and end tokens count"""

    def __init__(self, n_ctx=77, vocab=256):
        self.n_ctx, self.vocab = n_ctx, vocab

    def __call__(self, text):
        ids = torch.zeros(len(text), self.n_ctx, dtype=torch.long)
        for i, s in enumerate(text):
            codes = [2] + [3 + (ord(c) % (self.vocab - 4)) for c in s][:self.n_ctx - 2] + [1]
            ids[i, :len(codes)] = torch.tensor(codes)
        return ids


def params_of(tower):
    """the tower's state_dict as float64-ready numpy arrays"""
    return {k: v.detach().cpu().numpy() for k, v in tower.state_dict().items()}


def run_stock(tower, tokens, skip_last=0):
    """the stock tower as CLIPTextEmbedder.encode_with_transformer runs it (sequence-first blocks), on the tower's device and dtype"""
    with torch.no_grad():
        x = (tower.token_embedding(tokens) + tower.positional_embedding).permute(1, 0, 2)
        blocks = list(tower.transformer.resblocks)
        for blk in blocks[:len(blocks) - skip_last]:
            x = blk(x, attn_mask=tower.attn_mask)
        return tower.ln_final(x.permute(1, 0, 2))
