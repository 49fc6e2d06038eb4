"""Cost of the cross-attention maps, HIP events on the current device:
  the operator alone, bf16, at (B 64, heads 8, Nq 1024, Nkv 77) and (64, 12, 1024, 231), writing and accumulating, against its own
  traffic floor -- Q read once plus the map written (and read under accumulate), over the achievable HBM rate DESIGN.md quotes;
  forward_maps over all layers of the 12L/d512 model at B = 64, L = 77 against forward, timed alternately in the same run."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import paintmind_amd as pm
from paintmind_amd import ops
from paintmind_amd.generate import Pipeline

dev = torch.device("cuda:0")
HBM = 6.3e12                    # bytes / s: the achievable HBM rate (the LayerNorm stream)


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
    for B, H, N, nkv in ((64, 8, 1024, 77), (64, 12, 1024, 231)):
        pad = ops.round_up(nkv, 64)
        q = (torch.randn(B, H, N, 64, device=dev) * 0.5).to(torch.bfloat16)
        k = torch.randn(B, H, pad, 64, device=dev).to(torch.bfloat16)
        out = torch.zeros(B, N, nkv, device=dev)
        lens = torch.full((B,), nkv, dtype=torch.int32, device=dev)
        w = torch.ones(B, nkv, device=dev)
        qb, mb = q.numel() * 2, out.numel() * 4
        for name, kw, traffic in (("write", dict(), qb + mb), ("accumulate", dict(accumulate=True, scale=0.5), qb + 2 * mb),
                                  ("write, lengths", dict(kv_lens=lens), qb + mb), ("write, weights", dict(key_weights=w), qb + mb)):
            us = timeit(lambda: ops.attention_maps(q, k, nkv, use_exp2=True, out=out, **kw))
            floor = traffic / HBM * 1e6
            print(f"attention_maps bf16 B={B} H={H} Nq={N} Nkv={nkv} {name}: {us:.1f} us; Q {qb / 1e6:.0f} MB + map {mb / 1e6:.0f} MB"
                  f"{' (read and written)' if 'accumulate' in name else ''} -> floor {floor:.1f} us at {HBM / 1e12:.1f} TB/s = "
                  f"{floor / us:.2f} of the time, {traffic / us / 1e6:.2f} TB/s of its own traffic")


def model():
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(pm.ver2cfg["bench-uncond-12L-d512"]), stage1_pretrained=False).eval().to(dev)
    pipe.set_compute_dtype(torch.bfloat16)
    eng = pipe.engine()
    B, L = 64, 77
    depth = len(pipe.transformer.layers)
    tok = torch.randn(B, eng.tokens, eng.embed_dim, device=dev)
    ctx = torch.randn(B, L, eng.context_dim, device=dev)
    plain, tapped = [], []
    for _ in range(3):                                         # alternating: the yardstick is forward in the same run
        plain.append(timeit(lambda: eng.forward(tok, ctx), iters=10, warm=2))
        tapped.append(timeit(lambda: eng.forward_maps(tok, ctx, range(depth)), iters=10, warm=2))
    one = timeit(lambda: eng.forward_maps(tok, ctx, [depth - 1]), iters=10, warm=2)
    a, b = eng.forward(tok, ctx), eng.forward_maps(tok, ctx, range(depth))[0]
    print(f"12L/d512 bf16 B={B} L={L}: forward {min(plain) / 1e3:.3f} ms (runs {[round(x / 1e3, 3) for x in plain]}), forward_maps over all "
          f"{depth} layers {min(tapped) / 1e3:.3f} ms (runs {[round(x / 1e3, 3) for x in tapped]}) = +{(min(tapped) / min(plain) - 1) * 100:.1f} %, "
          f"{(min(tapped) - min(plain)) / depth:.1f} us per tapped layer; one layer {one / 1e3:.3f} ms; logits equal: {bool(torch.equal(a, b))}")


if __name__ == "__main__":
    operator()
    model()
