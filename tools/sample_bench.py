"""Time of the sampling kernel alone (sample.hip) at the bench shape, (65 536, 8192) fp32 logits, over top-k: 5 (the
block-statistics kernel), 64 (the row kernel, one candidate per lane), 65, 1024 and 8192 (the selection kernel, DESIGN.md section
4n) -- with Philox noise and with given noise; --top-p adds, for every top-k, the nucleus kernel at those masses (DESIGN.md
section 4o).  Device events around back-to-back launches after a warm-up; the variants are
interleaved over several rounds and the median and the minimum of the rounds are printed, with the rate at which the logits are
read (one read of M x V x 4 bytes is the least any of them can do; 8 bytes per 64-column block + k blocks for top-k <= 8).

    python tools/sample_bench.py [--topk 5 64 65 1024 8192] [--top-p 0.5 0.9] [--rounds 5] [--launches 10] [--rows 65536] [--classes 8192]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from paintmind_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--topk", type=int, nargs="+", default=[5, 64, 65, 1024, 8192])
ap.add_argument("--top-p", type=float, nargs="*", default=[], help="nucleus masses: every top-k is also timed with each of them")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--launches", type=int, default=10)
ap.add_argument("--rows", type=int, default=65536)
ap.add_argument("--classes", type=int, default=8192)
ap.add_argument("--no-given-noise", action="store_true", help="Philox only (the given-noise tensor is as large as the logits)")
args = ap.parse_args()

assert torch.cuda.is_available(), "sample_bench needs a ROCm device"
dev = torch.device("cuda:0")
M, V = args.rows, args.classes
g = torch.Generator(device=dev).manual_seed(0)
logits = torch.randn(M, V, device=dev, generator=g) * 3            # random data: trained-like spread, no ties
ids = torch.full((M,), V, dtype=torch.long, device=dev)
noise = None if args.no_given_noise else torch.rand(M, V, device=dev, generator=g)

variants = [(k, p, mode) for k in args.topk for p in [None] + args.top_p for mode in (("philox", "given") if noise is not None else ("philox",))]


def launch(k, p, mode):
    kw = {} if p is None else {"top_p": p}                            # (without --top-p the calls a parent checkout takes)
    if mode == "philox":
        return ops.sample_rows(logits, ids, V, k, 1.0, seed=7, step=3, row_base=0, **kw)
    return ops.sample_rows(logits, ids, V, k, 1.0, noise=noise, **kw)


times = {v: [] for v in variants}
for v in variants:                                                  # every variant's code object and allocator state, warm
    for _ in range(2):
        launch(*v)
torch.cuda.synchronize()
for _ in range(args.rounds):
    for v in variants:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            launch(*v)
        e1.record()
        torch.cuda.synchronize()
        times[v].append(e0.elapsed_time(e1) / args.launches)

print(f"sample_rows at ({M}, {V}) fp32, {args.rounds} rounds of {args.launches} launches, ms per launch (median / min); "
      f"logits = {M * V * 4 / 2 ** 30:.2f} GiB")
for (k, p, mode), ts in times.items():
    med, lo = statistics.median(ts), min(ts)
    print(f"topk={k:5d} top_p={'none' if p is None else format(p, '.3g'):5s} {mode:6s}: {med:8.3f} / {lo:8.3f} ms   {M * V * 4 / med / 1e6:7.0f} GB/s of logits")
