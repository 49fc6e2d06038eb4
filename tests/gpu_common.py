"""helpers for the GPU parity tests"""
import numpy as np
import torch


def dev():
    return torch.device("cuda:0")


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return x.to(dtype) if dtype is not None else x


def n(x):
    return x.detach().float().cpu().numpy() if x.dtype == torch.bfloat16 else x.detach().cpu().numpy()


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


def scaled_chain_pipeline():
    """The model of tests/golden/full_stage2_chain.npz on the GPU: bench-uncond-12L-d512 from torch.manual_seed(0) with
    to_logits.weight times the fixture's logit_scale (16: exact in fp32 and bf16), scaled on the CPU before the model is moved and
    before any engine packs a weight.  -> (pipeline, fixture arrays).  Callers keep it in a module-scoped fixture of their own."""
    import paintmind_amd as pm
    from paintmind_amd.generate import Pipeline
    from util import load_golden
    _, d = load_golden("full_stage2_chain.npz")
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(pm.ver2cfg["bench-uncond-12L-d512"]), stage1_pretrained=False).eval()
    pipe.transformer.to_logits.weight.data.mul_(int(d["logit_scale"]))
    pipe = pipe.to(dev())
    pipe.invalidate_engines()                 # an edit through .data is invisible to the engine cache's fingerprint
    return pipe, d
