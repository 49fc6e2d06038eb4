"""Cost of the logit divergence: HIP events on the current device, one process, one box.  Writes
profiles/logit_divergence_bench.txt.
  The operator at (M, V) = (65 536, 8192) fp32 -- two tensors of 2 GiB -- with every row scored and with every second row scored, both
  kinds, beside ops.masked_ce on one of the two tensors (tools/loss_bench.py's call: the same residency, one row where this reads two)
  as the same-box yardstick.  The arms alternate: ROUNDS rounds, each a warm-up and ITERS launches timed one by one; per arm the
  median over all of them, the fastest, and the spread of the round medians.  TB/s counts the SCORED rows' bytes.
  Then one ``Pipeline.diff_mask`` call (B = 16, draws = 4) on the 12-layer d512 pipeline beside 4 plain forwards of 32 images and
  beside its 4 divergence launches alone, so the divergence's share is visible."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import paintmind_amd as pm
from paintmind_amd import ops
from paintmind_amd.generate import Pipeline, diff_draws

dev = torch.device("cuda:0")
M, V, ROUNDS, ITERS = 65536, 8192, 3, 10
OUT = os.path.join(ROOT, "profiles", "logit_divergence_bench.txt")
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
    all_ids = torch.full((M,), V, dtype=torch.int64, device=dev)
    half_ids = torch.where(torch.arange(M, device=dev) % 2 == 0, all_ids, torch.zeros_like(all_ids))
    labels = torch.randint(0, V, (M,), device=dev, generator=g)
    mask = torch.ones(M, device=dev)
    out = (torch.zeros(M, device=dev), torch.zeros(M, dtype=torch.int32, device=dev))
    row = V * 4
    arms = {}
    for kind in ("tv", "jeffreys"):
        arms[f"{kind}, every row scored"] = (lambda k=kind: ops.logit_divergence(a, b, ids=all_ids, mask_id=V, kind=k, out=out), 2 * M * row)
        arms[f"{kind}, every second row scored"] = (lambda k=kind: ops.logit_divergence(a, b, ids=half_ids, mask_id=V, kind=k, out=out), M * row)
    arms["masked_ce (yardstick)"] = (lambda: ops.masked_ce(a, labels, mask, 0.1), M * row)
    runs = {name: [] for name in arms}
    for _ in range(ROUNDS):                                    # alternating: every arm sees the same box in every round
        for name, (fn, _) in arms.items():
            runs[name].append(times(fn))
    say(f"(M, V) = ({M}, {V}) fp32: two tensors of {M * row / 2 ** 30:.0f} GiB; {ROUNDS} rounds x {ITERS} launches per arm, each launch between its own events")
    rate = {}
    for name, (_, nbytes) in arms.items():
        flat = [x for r in runs[name] for x in r]
        med, best = statistics.median(flat), min(flat)
        meds = [statistics.median(r) for r in runs[name]]
        rate[name] = nbytes / med / 1e6
        say(f"{name}: median {med:.1f} us = {rate[name]:.2f} TB/s of {nbytes / 2 ** 30:.0f} GiB scored; fastest {best:.1f} us = {nbytes / best / 1e6:.2f} TB/s; "
            f"round medians {[round(x, 1) for x in meds]}, spread (max - min) / min {(max(meds) - min(meds)) / min(meds) * 100:.1f} %")
    yard = rate["masked_ce (yardstick)"]
    for name in arms:
        if name != "masked_ce (yardstick)":
            say(f"{name}: {rate[name]:.2f} TB/s / masked_ce {yard:.2f} TB/s = {rate[name] / yard:.3f}")


def pipeline():
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(pm.ver2cfg["bench-uncond-12L-d512"]), stage1_pretrained=False).eval().to(dev)
    pipe.set_compute_dtype(torch.bfloat16)
    B, N, S, draws = 16, pipe.num_tokens, pipe.image_size, 4
    g = torch.Generator().manual_seed(1)
    img = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    ctx = torch.randn(2 * B, 77, pipe.text_model.context_dim, generator=g).to(dev)
    eng = pipe.engine()
    ids = pipe.to_latent(img)[1].reshape(B, N).to(dev, torch.long)
    masks = diff_draws(B, N, 0.5, draws, 0).to(dev)
    masked = [torch.where(m, torch.full_like(ids, pipe.mask_token_id), ids).contiguous() for m in masks]
    tokens = [pipe.ids2tokens(torch.cat((m, m))) for m in masked]
    logits = eng.forward(tokens[0], ctx).reshape(2 * B * N, -1).clone()
    out = (torch.zeros(B * N, device=dev), torch.zeros(B * N, dtype=torch.int32, device=dev))

    def forwards():
        for tok in tokens:
            eng.forward(tok, ctx)

    def divergences():
        for m in masked:
            ops.logit_divergence(logits[:B * N], logits[B * N:], ids=m.reshape(-1), mask_id=pipe.mask_token_id, out=out, accumulate=True)
    arms = {"diff_mask(B = 16, draws = 4)": lambda: pipe.diff_mask(img, ctx[:B], ctx[B:], draws=draws),
            "4 plain forwards of 32 images": forwards, "its 4 divergence launches alone": divergences}
    say(f"12-layer d512 pipeline, bf16, N = {N}, n_embed = {logits.shape[1]}: the logits of a draw take {logits.numel() * 4 / 2 ** 30:.2f} GiB")
    med = {}
    for name, fn in arms.items():
        v = times(fn, iters=5, warm=2)
        med[name] = statistics.median(v)
        say(f"{name}: median {med[name] / 1e3:.2f} ms of 5 (fastest {min(v) / 1e3:.2f} ms)")
    say(f"the divergence launches are {med['its 4 divergence launches alone'] / med['diff_mask(B = 16, draws = 4)'] * 100:.1f} % of the diff_mask call; "
        f"the call is {med['diff_mask(B = 16, draws = 4)'] / med['4 plain forwards of 32 images']:.2f} x its four forwards")


if __name__ == "__main__":
    say(f"device: {torch.cuda.get_device_name(0)}")
    operator()
    torch.cuda.empty_cache()
    pipeline()
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
