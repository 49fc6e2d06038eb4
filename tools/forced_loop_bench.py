"""Cost of a forced source half in the prompt-to-prompt loop, the shapes of tools/control_bench.py: the
12L/d512 model in bf16, 32 pairs = 64 images, L = 77, T = 8 steps, every layer's cross-attention controlled for cross_steps = 0.8.
``control_ids`` with and without source_ids, timed alternately in one process: a host clock around the call, which ends in a device
synchronise.  The forced half replaces one sample_rows launch per step with one forced launch and adds the host check of the
source ids (one device-to-host sync per call); ``forced_ids`` alone (one half, no control) is timed beside them."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import paintmind_amd as pm
from paintmind_amd.generate import Pipeline

dev = torch.device("cuda:0")


def clock(fn, iters=3, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3            # ms


def main():
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(pm.ver2cfg["bench-uncond-12L-d512"]), stage1_pretrained=False).eval().to(dev)
    pipe.set_compute_dtype(torch.bfloat16)
    eng = pipe.engine()
    B, L, T = 32, 77, 8
    src = torch.randn(B, L, eng.context_dim, device=dev)
    edit = torch.randn(B, L, eng.context_dim, device=dev)
    ctl = (np.tile(np.arange(L, dtype=np.int32), (B, 1)), np.ones((B, L), np.float32), np.ones((B, L), np.float32))
    s = torch.randint(0, pipe.mask_token_id, (B, pipe.num_tokens), device=dev)
    args = (src, edit, None, None, *ctl, B, T, 1.0, 5, 7)
    arms = {"control_ids": lambda: pipe.control_ids(*args, cross_steps=0.8),
            "control_ids(source_ids=)": lambda: pipe.control_ids(*args, cross_steps=0.8, source_ids=s),
            "forced_ids": lambda: pipe.forced_ids(s, src, B, T, 7)}
    runs = {name: [] for name in arms}
    for _ in range(3):                                         # alternating: every arm sees the same box in every round
        for name, fn in arms.items():
            runs[name].append(clock(fn))
    a = pipe.control_ids(*args, cross_steps=0.8, source_ids=s)[0]
    print(f"12L/d512 bf16, {B} pairs = {2 * B} images, L={L}, T={T}, N={pipe.num_tokens}, V={pipe.mask_token_id}; "
          f"source half == forced_ids alone: {bool(torch.equal(a, pipe.forced_ids(s, src, B, T, 7)))}")
    for name, v in runs.items():
        print(f"{name}: {min(v):.2f} ms per call (rounds {[round(x, 2) for x in v]}; spread {(max(v) - min(v)) / min(v) * 100:.1f} %)")
    d = min(runs["control_ids(source_ids=)"]) - min(runs["control_ids"])
    print(f"with source_ids - without = {d:+.3f} ms per call = {d / T * 1e3:+.1f} us per step")


if __name__ == "__main__":
    main()
