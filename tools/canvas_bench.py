"""Cost of the canvas operators: HIP events on the current device, one process, one box.  Writes
profiles/canvas_bench.txt.
  ops.window_logits at (g, V) = (32, 8192) on canvases of 32 x 96 and 64 x 64 tokens at stride 16, B = 8, plain and guided, as bytes moved
  per second (every window row read once, twice when guided, every canvas row written once) beside ops.logit_divergence on the same
  window logits in the same process on the same box: that kernel is the yardstick.  The arms alternate: ROUNDS rounds, each a warm-up and
  ITERS launches timed one by one; per arm the median over all of them, the fastest, and the spread of the round medians.
  Then ops.window_pixels alone (S = 256, the 64 x 64-token canvas, B = 8), and ``Pipeline.canvas_ids`` on the 12-layer d512 pipeline
  (a 64 x 64-token canvas, B = 2, 8 steps) beside its own B * W forwards per step, so the share of everything that is not the tower
  is visible.
  --parent PATH (a built checkout of the parent commit): last, the default ``bench.py --gpus 1 --steps 5 --warmup 2`` line of this tree
  and of that one, two runs each, the trees alternating, every run a process of its own -- the default path launches none of this
  code and should be unchanged."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import paintmind_amd as pm
from paintmind_amd import ops
from paintmind_amd.canvas import canvas_layout
from paintmind_amd.generate import Pipeline

dev = torch.device("cuda:0")
G, V, B, ROUNDS, ITERS = 32, 8192, 8, 3, 10
OUT = os.path.join(ROOT, "profiles", "canvas_bench.txt")
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


def report(arms, yardstick):
    runs = {name: [] for name in arms}
    for _ in range(ROUNDS):                                    # alternating: every arm sees the same box in every round
        for name, (fn, _) in arms.items():
            runs[name].append(times(fn))
    rate = {}
    for name, (_, nbytes) in arms.items():
        flat = [x for r in runs[name] for x in r]
        med, best = statistics.median(flat), min(flat)
        meds = [statistics.median(r) for r in runs[name]]
        rate[name] = nbytes / med / 1e6
        say(f"{name}: median {med:.1f} us = {rate[name]:.2f} TB/s of {nbytes / 2 ** 30:.2f} GiB moved; fastest {best:.1f} us = "
            f"{nbytes / best / 1e6:.2f} TB/s; round medians {[round(x, 1) for x in meds]}, spread (max - min) / min "
            f"{(max(meds) - min(meds)) / min(meds) * 100:.1f} %")
    for name in arms:
        if name != yardstick:
            say(f"{name}: {rate[name]:.2f} TB/s / {yardstick} {rate[yardstick]:.2f} TB/s = {rate[name] / rate[yardstick]:.3f}")


def logits(grid):
    lay = canvas_layout(grid, G, 16, 8)
    tb = ops.canvas_tables(lay, dev)
    M = B * lay.window_rows
    g = torch.Generator(device=dev).manual_seed(0)
    a = torch.randn(M, V, device=dev, generator=g)
    b = 0.8 * a + 0.6 * torch.randn(M, V, device=dev, generator=g)
    out = torch.empty(B * lay.tokens, V, device=dev)
    div = (torch.zeros(M, device=dev), torch.zeros(M, dtype=torch.int32, device=dev))
    row = V * 4
    say(f"canvas {grid[0]} x {grid[1]} tokens, g = {G}, stride 16, B = {B}, V = {V}: {lay.n_windows} windows a canvas, K = {lay.K}; window logits "
        f"{M * row / 2 ** 30:.2f} GiB, canvas logits {B * lay.tokens * row / 2 ** 30:.2f} GiB; {ROUNDS} rounds x {ITERS} launches per arm")
    arms = {"window_logits plain": (lambda: ops.window_logits(a, tb.cover, tb.weight, lay.window_rows, out=out), (M + B * lay.tokens) * row),
            "window_logits guided": (lambda: ops.window_logits(a, tb.cover, tb.weight, lay.window_rows, uncond=b, scale=3.0, out=out),
                                     (2 * M + B * lay.tokens) * row),
            "logit_divergence (yardstick)": (lambda: ops.logit_divergence(a, b, out=div), 2 * M * row)}
    report(arms, "logit_divergence (yardstick)")


def pixels():
    lay = canvas_layout((64, 64), G, 16, 8)
    tb = ops.canvas_tables(lay, dev)
    S = G * 8
    img = torch.rand(B * lay.n_windows, 3, S, S, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2 - 1
    out = torch.empty(B, 3, *lay.size, device=dev)
    v = times(lambda: ops.window_pixels(img, tb, out=out))
    nbytes = (img.numel() + out.numel()) * 4
    say(f"window_pixels, {lay.n_windows} windows of {S} x {S} -> {lay.size[0]} x {lay.size[1]}, B = {B}: median {statistics.median(v):.1f} us of {ITERS} "
        f"(fastest {min(v):.1f} us), {nbytes / 2 ** 20:.0f} MiB moved = {nbytes / statistics.median(v) / 1e6:.2f} TB/s")


def loop():
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(pm.ver2cfg["bench-uncond-12L-d512"]), stage1_pretrained=False).eval().to(dev)
    pipe.set_compute_dtype(torch.bfloat16)
    nb, T = 2, 8
    lay = pipe.canvas_layout((512, 512))
    eng = pipe.engine()
    tok = pipe.ids2tokens(torch.full((nb * lay.n_windows, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long, device=dev))

    def forwards():
        for _ in range(T):
            eng.forward(tok, None)
    arms = {f"canvas_ids(512 x 512 px, B = {nb}, T = {T})": lambda: pipe.canvas_ids(None, nb, lay, T, 1.0, 5, 0),
            f"its {T} forwards of {nb * lay.n_windows} windows alone": forwards,
            "decode_canvas": lambda: pipe.decode_canvas(torch.zeros(nb, lay.tokens, dtype=torch.long, device=dev), lay)}
    say(f"12-layer d512 pipeline, bf16, {lay.n_windows} windows a canvas, {lay.tokens} canvas tokens, n_embed = {eng.n_embed}")
    med = {}
    for name, fn in arms.items():
        v = times(fn, iters=5, warm=2)
        med[name] = statistics.median(v)
        say(f"{name}: median {med[name] / 1e3:.2f} ms of 5 (fastest {min(v) / 1e3:.2f} ms)")
    names = list(arms)
    say(f"the loop is {med[names[0]] / med[names[1]]:.2f} x its forwards")


def bench_lines(parent):
    say("bench.py --gpus 1 --steps 5 --warmup 2, the trees alternating, one process a run:")
    for _ in range(2):
        for name, root in (("branch", ROOT), ("parent", os.path.abspath(parent))):
            run = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"], cwd=root, capture_output=True,
                                 text=True, timeout=600, check=True)
            r = json.loads(run.stdout.strip().splitlines()[-1])
            say(f"{name}: {r['value']:.1f} images/s, {r['ms_per_step']:.2f} ms per step")


if __name__ == "__main__":
    say(f"device: {torch.cuda.get_device_name(0)}")
    for grid in ((32, 96), (64, 64)):
        logits(grid)
        torch.cuda.empty_cache()
    pixels()
    loop()
    if "--parent" in sys.argv:
        torch.cuda.empty_cache()
        bench_lines(sys.argv[sys.argv.index("--parent") + 1])
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
