"""Stand-ins for the native Flan-T5 tower's tests: randomly initialised gated-GELU T5 encoders of the shapes the kernels serve
(d_kv 64) and a tokenizer with both call forms T5TextEmbedder uses.  Not a conftest, not collected."""
import torch


class CharTokenizer:
    """one id per character (2 + ord % 100), pad 0, end-of-sequence 1; a string gives a list of ids, a list of strings a padded
    [B, max_length] tensor"""
    pad_token_id, eos_token_id = 0, 1

    @staticmethod
    def ids_of(s):
        return [2 + ord(c) % 100 for c in s]

    def __call__(self, text, max_length=77, add_special_tokens=True, **kw):
        if isinstance(text, str):
            return {"input_ids": self.ids_of(text) + ([1] if add_special_tokens else [])}
        ids = torch.zeros(len(text), max_length, dtype=torch.long)
        for i, s in enumerate(text):
            row = self.ids_of(s)[:max_length - 1] + [1]
            ids[i, :len(row)] = torch.tensor(row)
        return {"input_ids": ids}


def gated_t5(seed=0, **kw):
    """T5Config(vocab_size=128, d_model=128, d_kv=64, d_ff=192, num_layers=2, num_heads=2, feed_forward_proj="gated-gelu") unless
    overridden, randomly initialised from `seed`, in eval mode"""
    from transformers import T5Config, T5EncoderModel
    cfg = dict(vocab_size=128, d_model=128, d_kv=64, d_ff=192, num_layers=2, num_heads=2, feed_forward_proj="gated-gelu")
    cfg.update(kw)
    torch.manual_seed(seed)
    return T5EncoderModel(T5Config(**cfg)).eval()


def params_of(model):
    """the state_dict as float64 numpy arrays (tests/t5_ref.py encoder)"""
    return {k: v.detach().double().cpu().numpy() for k, v in model.state_dict().items()}
