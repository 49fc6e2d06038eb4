"""Cost of the cross-attention control, HIP events on the current device, 50 launches behind a warm-up, one process:
  the operator alone, bf16, at (B 64, heads 8, Nq 1024, L 77) and (64, 12, 1024, 231) -- every row mapped, half of them, none -- beside the
  ordinary cross-attention under lengths (pmhip_attention_lens) on the same edited pass, timed alternately in the same run;
  forward_control with every layer controlled (cross, and cross + self) on the 12L/d512 model, 32 pairs = 64 images, L = 77, against
  forward on the same 64 images, timed alternately."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import paintmind_amd as pm
from paintmind_amd import ops
from paintmind_amd.generate import Pipeline

dev = torch.device("cuda:0")


def timeit(fn, iters=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3       # us


def operator():
    for B, H, N, L in ((64, 8, 1024, 77), (64, 12, 1024, 231)):
        pad = ops.round_up(L, 64)
        q = lambda: (torch.randn(B, H, N, 64, device=dev) * 0.5).to(torch.bfloat16)
        k = lambda: torch.randn(B, H, pad, 64, device=dev).to(torch.bfloat16)
        qs, ks, qt, kt, vt = q(), k(), q(), k(), torch.randn(B, H, 64, pad, device=dev).to(torch.bfloat16)
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        out = torch.empty(B * N, H * 64, device=dev, dtype=torch.bfloat16)
        j = torch.arange(L, dtype=torch.int32, device=dev)
        ones = torch.ones(B, L, device=dev)
        maps = {"every row mapped": j.repeat(B, 1), "every second row": torch.where(j % 2 == 0, j, -1).repeat(B, 1).contiguous(),
                "no row mapped": torch.full((B, L), -1, dtype=torch.int32, device=dev)}
        plain, ctl = [], {name: [] for name in maps}
        for _ in range(3):                                     # alternating: the yardstick is the lengths form in the same run
            plain.append(timeit(lambda: ops.attention(qt, kt, vt, L, use_exp2=True, kv_lens=lens)))
            for name, rm in maps.items():
                ctl[name].append(timeit(lambda: ops.attention_control(qs, ks, qt, kt, vt, L, L, rm, ones, ones, use_exp2=True, lens_src=lens,
                                                                      lens_tgt=lens, out=out)))
        print(f"bf16 B={B} H={H} Nq={N} L={L}: attention under lengths {min(plain):.1f} us (runs {[round(x, 1) for x in plain]}); "
              + "; ".join(f"control, {name} {min(v):.1f} us = {min(v) / min(plain):.2f} x (runs {[round(x, 1) for x in v]})" for name, v in ctl.items()))


def model():
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(pm.ver2cfg["bench-uncond-12L-d512"]), stage1_pretrained=False).eval().to(dev)
    pipe.set_compute_dtype(torch.bfloat16)
    eng = pipe.engine()
    B, L = 32, 77
    depth = len(pipe.transformer.layers)
    tok = torch.randn(2 * B, eng.tokens, eng.embed_dim, device=dev)
    ctx = torch.randn(2 * B, L, eng.context_dim, device=dev)
    ctl = dict(row_map=np.tile(np.arange(L, dtype=np.int32), (B, 1)), blend=np.ones((B, L), np.float32), gain=np.ones((B, L), np.float32))
    plain, cross, both = [], [], []
    for _ in range(3):                                         # alternating: the yardstick is forward in the same run
        plain.append(timeit(lambda: eng.forward(tok, ctx), iters=10, warm=2))
        cross.append(timeit(lambda: eng.forward_control(tok, ctx, cross_layers=range(depth), **ctl), iters=10, warm=2))
        both.append(timeit(lambda: eng.forward_control(tok, ctx, cross_layers=range(depth), self_layers=range(depth), **ctl), iters=10, warm=2))
    a, b = eng.forward(tok[:B], ctx[:B]), eng.forward_control(tok, ctx, cross_layers=range(depth), **ctl)[:B]
    ms = lambda v: f"{min(v) / 1e3:.3f} ms (runs {[round(x / 1e3, 3) for x in v]})"
    print(f"12L/d512 bf16 {B} pairs = {2 * B} images L={L}: forward {ms(plain)}, forward_control over all {depth} layers, cross {ms(cross)} = "
          f"+{(min(cross) / min(plain) - 1) * 100:.1f} %, {(min(cross) - min(plain)) / depth:.1f} us per controlled layer; cross + self {ms(both)} = "
          f"+{(min(both) / min(plain) - 1) * 100:.1f} %; source-half logits equal: {bool(torch.equal(a, b))}")


if __name__ == "__main__":
    operator()
    model()
