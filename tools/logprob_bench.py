"""Cost of the token likelihood: HIP events on the current device, one process, one box.  Writes
profiles/token_logprob_bench.txt.
  The operator at (M, V) = (65 536, 8192) fp32 -- tensors of 2 GiB -- in three forms: every row scored, every second row scored, and
  the guided form (two tensors read, combined at load), the last set against ops.guidance_combine into a third tensor followed by the
  plain form.  ops.masked_ce on the same tensor (the same traffic floor: one read of each scored row) and ops.logit_divergence (tv) on
  the same pair run in the same process as yardsticks.  The arms alternate: ROUNDS rounds, each a warm-up and ITERS launches timed
  one by one; per arm the median over all of them, the fastest, and the spread of the round medians.  TB/s counts the bytes the arm
  has to move: the scored rows once per operand read, plus what the composed arm writes and reads again."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from paintmind_amd import ops

dev = torch.device("cuda:0")
M, V, ROUNDS, ITERS = 65536, 8192, 3, 10
SCALE = 3.0
OUT = os.path.join(ROOT, "profiles", "token_logprob_bench.txt")
YARD = "masked_ce (yardstick)"
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def times(fn, iters=ITERS, warm=3):
    """-> the time of each of `iters` calls in us, every call between an event pair of its own"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in pairs]


def operator():
    g = torch.Generator(device=dev).manual_seed(0)
    a = torch.randn(M, V, device=dev, generator=g)
    a[torch.arange(M, device=dev), torch.randint(0, V, (M,), device=dev, generator=g)] += 6.0      # trained-like: one dominant class
    b = 0.8 * a + 0.6 * torch.randn(M, V, device=dev, generator=g)
    combined = torch.empty_like(a)
    all_ids = torch.full((M,), V, dtype=torch.int64, device=dev)
    half_ids = torch.where(torch.arange(M, device=dev) % 2 == 0, all_ids, torch.zeros_like(all_ids))
    target = torch.randint(0, V, (M,), device=dev, generator=g)
    mask = torch.ones(M, device=dev)
    out = (torch.zeros(M, device=dev), torch.zeros(M, device=dev), torch.zeros(M, dtype=torch.int32, device=dev), torch.zeros(M, dtype=torch.int32, device=dev))
    div_out = (torch.zeros(M, device=dev), torch.zeros(M, dtype=torch.int32, device=dev))
    row = V * 4

    def composed():
        ops.guidance_combine(a, b, SCALE, out=combined)
        ops.token_logprob(combined, target, ids=all_ids, mask_id=V, out=out)
    arms = {
        "plain, every row scored": (lambda: ops.token_logprob(a, target, ids=all_ids, mask_id=V, out=out), M * row),
        "plain, every second row scored": (lambda: ops.token_logprob(a, target, ids=half_ids, mask_id=V, out=out), M * row // 2),
        "guided (combined at load)": (lambda: ops.token_logprob(a, target, uncond=b, scale=SCALE, ids=all_ids, mask_id=V, out=out), 2 * M * row),
        "guidance_combine + plain": (composed, 4 * M * row),
        YARD: (lambda: ops.masked_ce(a, target, mask, 0.1), M * row),
        "logit_divergence tv (yardstick)": (lambda: ops.logit_divergence(a, b, ids=all_ids, mask_id=V, kind="tv", out=div_out), 2 * M * row),
    }
    runs = {name: [] for name in arms}
    for _ in range(ROUNDS):                                    # alternating: every arm sees the same box in every round
        for name, (fn, _) in arms.items():
            runs[name].append(times(fn))
    say(f"(M, V) = ({M}, {V}) fp32: tensors of {M * row / 2 ** 30:.0f} GiB; {ROUNDS} rounds x {ITERS} launches per arm, each launch between its own events")
    rate, med = {}, {}
    for name, (_, nbytes) in arms.items():
        flat = [x for r in runs[name] for x in r]
        med[name], best = statistics.median(flat), min(flat)
        meds = [statistics.median(r) for r in runs[name]]
        rate[name] = nbytes / med[name] / 1e6
        say(f"{name}: median {med[name]:.1f} us = {rate[name]:.2f} TB/s of {nbytes / 2 ** 30:.0f} GiB moved; fastest {best:.1f} us = {nbytes / best / 1e6:.2f} TB/s; "
            f"round medians {[round(x, 1) for x in meds]}, spread (max - min) / min {(max(meds) - min(meds)) / min(meds) * 100:.1f} %")
    for name in ("plain, every row scored", "plain, every second row scored", "guided (combined at load)"):
        say(f"{name}: {rate[name]:.2f} TB/s / masked_ce {rate[YARD]:.2f} TB/s = {rate[name] / rate[YARD]:.3f} per byte")
    say(f"guided (combined at load) {med['guided (combined at load)']:.1f} us against guidance_combine + plain {med['guidance_combine + plain']:.1f} us: "
        f"{med['guidance_combine + plain'] / med['guided (combined at load)']:.2f} x")


if __name__ == "__main__":
    say(f"device: {torch.cuda.get_device_name(0)}")
    operator()
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
