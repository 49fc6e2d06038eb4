"""A/B of the edit loop against the pinned decode loop on the same start ids.

Both arms run in ONE process on one device, alternating, ROUNDS rounds of ITERS graph replays each:
  pinned  S2Engine.generate(nmask=[n_0 .. n_{T-1}])            -- what generate_ids(ids0=<half-masked ids>, streams=1, use_graph=True) runs
  edit    S2Engine.generate(nmask_img=[[n_t] * B ...], last 0) -- the counts form of the re-masking launch + the merged-ids copy
12L/d512 + vit-s, bf16, B = 8, T = 8, decode of the last step only.  What the edit arm adds per call: the table staging, the
table index in T re-masking launches, one B * N * 8-byte copy on the decoded step.  Prints one line per round and arm (ms per
call) and the spread of each arm over its rounds."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import paintmind_amd as pm  # noqa: E402
from paintmind_amd.generate import Pipeline, loop_schedule  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=8)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(pm.ver2cfg["bench-uncond-12L-d512"]), stage1_pretrained=False).eval().to(dev)
    pipe.set_compute_dtype(torch.bfloat16)
    eng, vq = pipe.engine(), pipe.vqgan.engine()
    B, T, N = args.batch, args.steps, pipe.num_tokens
    temps, nmask, _ = loop_schedule(T, 1.0, N)
    table = [[nmask[t] if t < T - 1 else 0] * B for t in range(T)]
    g = torch.Generator().manual_seed(1)
    ids0 = torch.randint(0, pipe.mask_token_id, (B, N), generator=g)
    ids0[torch.rand(B, N, generator=g) < 0.5] = pipe.mask_token_id
    ids0 = ids0.to(dev)
    flags = [False] * (T - 1) + [True]
    arms = {"pinned": dict(nmask=nmask), "edit": dict(nmask=None, nmask_img=table)}

    def call(kw):
        return eng.generate(vq, ids0.clone(), None, temps, kw["nmask"], flags, 5, seed=3, use_graph=True, nmask_img=kw.get("nmask_img"))

    for kw in arms.values():                          # eager pass, capture, one replay
        for _ in range(3):
            call(kw)
    torch.cuda.synchronize(dev)
    results = {name: [] for name in arms}
    for r in range(args.rounds):
        for name, kw in arms.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.iters):
                call(kw)
            torch.cuda.synchronize(dev)
            ms = (time.perf_counter() - t0) * 1e3 / args.iters
            results[name].append(ms)
            print(f"round {r} {name:6s} {ms:8.3f} ms per call (B={B} T={T}, {args.iters} replays)", flush=True)
    for name, v in results.items():
        print(f"{name:6s} mean {sum(v) / len(v):8.3f} ms  spread {max(v) - min(v):6.3f} ms  rounds {[round(x, 3) for x in v]}")
    d = sum(results["edit"]) / len(results["edit"]) - sum(results["pinned"]) / len(results["pinned"])
    print(f"edit - pinned = {d:+.3f} ms per call; pinned spread {max(results['pinned']) - min(results['pinned']):.3f} ms")


if __name__ == "__main__":
    main()
