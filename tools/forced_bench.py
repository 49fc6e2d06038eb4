"""Cost of the forced step: HIP events on the current device, one process, one box.
  The operator at (M, V) = (65 536, 8192) fp32 -- 2 GiB of logits, read once -- beside ops.sample_rows(topk=9) (the row kernel: the same
  loads, and nine rounds of a wave arg-max behind them) and ops.masked_ce (the other one-read row kernel) on the SAME logits, timed
  alternately: ROUNDS rounds of each, 20 launches behind a warm-up per round.  Per arm: the fastest round, every round, and the
  run-to-run spread (max - min) / min; against the single-read floor 2 GiB / 8 TB/s (spec) and / 6.3 TB/s (what a float4 copy reaches).
  The triples of the forced launch and of the draw it follows are compared bit for bit in the same run."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from paintmind_amd import ops

dev = torch.device("cuda:0")
M, V, ROUNDS = 65536, 8192, 5


def timeit(fn, iters=20, warm=3):
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


def main():
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn(M, V, device=dev, generator=g)
    logits[torch.arange(M, device=dev), torch.randint(0, V, (M,), device=dev, generator=g)] += 6.0     # trained-like: one dominant class
    ids = torch.where(torch.rand(M, device=dev, generator=g) < 0.5, torch.randint(0, V, (M,), device=dev, generator=g),
                      torch.full((M,), V, device=dev))
    drawn = ops.sample_rows(logits, ids, V, 9, 1.0, seed=1, step=0)
    target = drawn[0].clone()
    forced = ops.sample_rows_forced(logits, ids, target, V)
    same = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(forced, drawn))
    mask = torch.ones(M, device=dev)
    arms = {"sample_rows_forced": lambda: ops.sample_rows_forced(logits, ids, target, V),
            "sample_rows(topk=9)": lambda: ops.sample_rows(logits, ids, V, 9, 1.0, seed=1, step=0),
            "masked_ce": lambda: ops.masked_ce(logits, target, mask)}
    runs = {name: [] for name in arms}
    for _ in range(ROUNDS):                                    # alternating: every arm sees the same box in every round
        for name, fn in arms.items():
            runs[name].append(timeit(fn))
    nbytes = M * V * 4
    print(f"(M, V) = ({M}, {V}) fp32, {nbytes / 2 ** 30:.0f} GiB of logits read once; floor {nbytes / 8.0e12 * 1e6:.0f} us at 8 TB/s (spec), "
          f"{nbytes / 6.3e12 * 1e6:.0f} us at 6.3 TB/s (float4 copy); forced triple == the draw's triple bit for bit: {same}")
    for name, v in runs.items():
        best = min(v)
        print(f"{name}: {best:.1f} us = {nbytes / best / 1e6:.2f} TB/s = {nbytes / 8.0e12 * 1e6 / best * 100:.0f} % of the 8 TB/s floor; "
              f"rounds {[round(x, 1) for x in v]}; spread (max - min) / min {(max(v) - best) / best * 100:.1f} %")
    f, r = min(runs["sample_rows_forced"]), min(runs["sample_rows(topk=9)"])
    spread = max((max(v) - min(v)) / min(v) for v in (runs["sample_rows_forced"], runs["sample_rows(topk=9)"]))
    print(f"forced / sample_rows(topk=9) = {f / r:.3f} (the larger of the two spreads: {spread * 100:.1f} %)")


if __name__ == "__main__":
    main()
