"""The OpenCLIP text tower on the HIP path against stock PyTorch: HIP events on the current device, one process,
one box.  Writes profiles/clip_native_bench.txt (``--out`` another file).
  The towers: random weights in the ViT-L-14 (12 layers, width 768, 12 heads) and ViT-H-14 (24 layers, width 1024, 16 heads) text
  shapes with a 256-word vocabulary (tests/clip_stubs.py: the open_clip text interface, nn.GELU), B = 64 prompts of L = 77 rows.  Four
  arms -- stock f32 (how the reference loads it), stock bf16 (tower.to(bfloat16)), native f32, native bf16 -- alternate: ROUNDS rounds,
  each a warm-up and ITERS calls timed one by one; per arm the median over all of them, the fastest, and the spread of the round
  medians.  TFLOP/s counts the multiply-adds of the GEMMs and of the FULL Q K^T and P V (2 flops each), from the shapes: the causal
  half that is never computed is counted for both sides alike.
  The three new operators alone at those shapes, with the bytes they have to move (and, for the attention, its flops).
  Then ``Pipeline.generate(text)`` on the 12-layer d512 pipeline (bf16, 8 steps, 64 prompts) with the ViT-H-shaped tower as its text
  model, native off (the stock f32 tower) and on (the native tower in the pipeline's compute dtype)."""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import paintmind_amd as pm
from clip_stubs import Tokenizer, clip_tower, run_stock
from paintmind_amd import ops
from paintmind_amd._lib import PART_K, PART_Q, PART_V
from paintmind_amd.generate import Pipeline
from paintmind_amd.modules.clip_native import NativeClipText
from paintmind_amd.modules.encoder import CLIPTextEmbedder

dev = torch.device("cuda:0")
B, L, ROUNDS, ITERS = 64, 77, 3, 5
SHAPES = {"ViT-L-14": (12, 768), "ViT-H-14": (24, 1024)}
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def times(fn, iters=ITERS, warm=2):
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


def alternate(arms, rounds=ROUNDS, iters=ITERS):
    """every arm sees the same box in every round -> {name: (median, fastest, round medians)} in us"""
    runs = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            runs[name].append(times(fn, iters))
    out = {}
    for name, rs in runs.items():
        flat = [x for r in rs for x in r]
        out[name] = (statistics.median(flat), min(flat), [statistics.median(r) for r in rs])
    return out


def make_tower(layers, width):
    with torch.device(dev):
        return clip_tower(width, layers, quick=False)


def tower_flops(b, layers, width):
    gemm = 2 * b * L * 12 * width * width                       # in_proj 3 W^2, out_proj W^2, c_fc and c_proj 4 W^2 each
    attn = 2 * b * (width // 64) * 2 * L * L * 64               # Q K^T and P V, the full square
    return layers * (gemm + attn)


def tower(name, model):
    layers, width = SHAPES[name]
    ids = torch.randint(2, 256, (B, L), generator=torch.Generator().manual_seed(1)).to(dev)
    low = copy.deepcopy(model).to(torch.bfloat16)
    native = NativeClipText(model)
    ref = run_stock(model, ids)
    for what, got in (("stock bf16", run_stock(low, ids).float()), ("native f32", native(ids, dtype=torch.float32)),
                      ("native bf16", native(ids, dtype=torch.bfloat16))):
        d = (got - ref).double()
        say(f"{name} {what} against stock f32 (not an error measurement: both sides round): RMS {float(d.pow(2).mean().sqrt()):.3g}, "
            f"max abs {float(d.abs().max()):.3g}")
    arms = {"stock f32": lambda: run_stock(model, ids), "stock bf16": lambda: run_stock(low, ids),
            "native f32": lambda: native(ids, dtype=torch.float32), "native bf16": lambda: native(ids, dtype=torch.bfloat16)}
    flops = tower_flops(B, layers, width)
    say(f"{name} text tower: {layers} layers, width {width}, {width // 64} heads of 64, MLP {4 * width}; B = {B}, L = {L}: "
        f"{flops / 1e12:.2f} TFLOP per call ({tower_flops(1, layers, width) / 1e9:.1f} GFLOP per prompt); {ROUNDS} rounds x {ITERS} calls "
        "per arm, each call between its own events")
    res = alternate(arms)
    for arm, (med, best, meds) in res.items():
        say(f"{name} {arm}: median {med / 1e3:.2f} ms = {flops / med / 1e6:.0f} TFLOP/s; fastest {best / 1e3:.2f} ms; round medians "
            f"{[round(x / 1e3, 2) for x in meds]} ms, spread (max - min) / min {(max(meds) - min(meds)) / min(meds) * 100:.1f} %")
    for a, b_ in (("native f32", "stock f32"), ("native bf16", "stock bf16"), ("native bf16", "stock f32")):
        say(f"{name} {a} / {b_}: {res[a][0] / res[b_][0]:.3f} of its time")
    del low


def operators(name):
    layers, width = SHAPES[name]
    M, H, F = B * L, width // 64, 4 * width
    g = torch.Generator(device=dev).manual_seed(2)
    u3 = torch.randn(M, 3 * width, device=dev, generator=g)
    uf = torch.randn(M, F, device=dev, generator=g)
    arms, cost = {}, {}
    for dt, size in ((torch.float32, 4), (torch.bfloat16, 2)):
        tag = "f32" if dt == torch.float32 else "bf16"
        key = f"{name} split_heads [{M}, {3 * width}] -> {tag} Q, K, V^T"
        arms[key] = lambda dt=dt: ops.split_heads(u3, H, L, [PART_Q, PART_K, PART_V], q_scale=0.125, dtype=dt)
        cost[key] = (M * 3 * width * (4 + size), 0)
        for kind in ("erf", "quick"):
            key = f"{name} gelu {kind} [{M}, {F}] -> {tag}"
            arms[key] = lambda dt=dt, kind=kind: ops.gelu(uf, dt, kind)
            cost[key] = (M * F * (4 + size), 0)
        q, k, vt = ops.split_heads(u3, H, L, [PART_Q, PART_K, PART_V], q_scale=0.125, dtype=dt)
        out = torch.empty(M, H * 64, device=dev, dtype=dt)
        key = f"{name} attention_causal {tag} B {B}, H {H}, L {L}"
        arms[key] = lambda q=q, k=k, vt=vt, out=out: ops.attention_causal(q, k, vt, out=out)
        cost[key] = (4 * B * H * L * 64 * size, 2 * B * H * L * (L + 1) * 64)         # Q, K, V^T read, out written; the causal half of Q K^T, P V
    say(f"{name}: the new operators alone (split_heads includes the allocation and zeroing of its outputs), {ROUNDS} rounds x 10 launches "
        "per arm, each launch between its own events")
    for key, (med, best, meds) in alternate(arms, iters=10).items():
        nbytes, flops = cost[key]
        extra = f", {flops / med / 1e6:.1f} TFLOP/s (causal half)" if flops else ""
        say(f"{key}: median {med:.1f} us = {nbytes / med / 1e6:.2f} TB/s of {nbytes / 2 ** 20:.1f} MiB{extra}; fastest {best:.1f} us; "
            f"spread of the round medians {(max(meds) - min(meds)) / min(meds) * 100:.1f} %")


def pipeline(model, width):
    emb = CLIPTextEmbedder(model=model, tokenizer=Tokenizer())
    torch.manual_seed(0)
    cfg = dict(pm.ver2cfg["bench-uncond-12L-d512"], context_dim=width)
    pipe = Pipeline(pm.Config(cfg), stage1_pretrained=False, text_model=emb).eval().to(dev)
    pipe.set_compute_dtype(torch.bfloat16)
    text = [f"prompt number {i} of the batch" for i in range(B)]

    def gen():
        pipe.generate(text, timesteps=8, topk=5, seed=1)
    say(f"Pipeline.generate(text) on the 12-layer d512 pipeline, bf16, 8 steps, {B} prompts, the ViT-H-shaped tower as text model")
    res = {}
    for _ in range(2):                                               # alternating
        for name, on in (("native off (stock f32 tower)", False), ("native on (native bf16 tower)", True)):
            emb.use_native(on)
            res.setdefault(name, []).extend(times(gen, iters=3, warm=1))
    for name, v in res.items():
        say(f"{name}: median {statistics.median(v) / 1e3:.1f} ms of {len(v)} (fastest {min(v) / 1e3:.1f} ms) = "
            f"{B / statistics.median(v) * 1e6:.0f} images/s")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_native_bench.txt"))
    args = ap.parse_args()
    say(f"device: {torch.cuda.get_device_name(0)}")
    for name, (layers, width) in SHAPES.items():
        model = make_tower(layers, width)
        tower(name, model)
        torch.cuda.empty_cache()
        operators(name)
        torch.cuda.empty_cache()
    pipeline(model, SHAPES["ViT-H-14"][1])
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
