"""Decode sessions against the batch decode loop ("Decode sessions"; results under profiles/).

  uniform  S identical requests (T steps each) admitted together: the session (graph replay of the slots step) against
           generate_ids(use_graph=True, streams=1) on the same commit -- what per-image decode state costs when nothing differs.
  mixed    R requests with T drawn from a set in equal shares, all queued at time 0: the session against the best the scalar
           loop can do (sort by T, one generate_ids per homogeneous group of at most S).  Images/s and the mean request latency
           in decode steps (session: the tick a request retires at + 1; sorted groups: the steps run up to the end of its group).

The arms alternate inside one process, --rounds times; nothing is decoded (ids only).  --arms generate runs on a commit that has
no sessions: point --root at such a checkout to time the scalar loop of another commit on the same box.
"""
import argparse
import json
import os
import random
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose paintmind_amd is timed")
    ap.add_argument("--mode", default="uniform", choices=["uniform", "mixed"])
    ap.add_argument("--arms", default="session,generate")
    ap.add_argument("--workload", default="bench-uncond-12L-d512")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--timesteps", type=int, default=8)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--mix", default="8,12,18")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=6, help="uniform: batches per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import torch
    import paintmind_amd as pm
    from paintmind_amd.generate import Pipeline

    assert torch.cuda.is_available(), "slots_bench needs a ROCm device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(pm.ver2cfg[a.workload]), stage1_pretrained=False).to(dev).eval()
    pipe.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    S, arms = a.slots, a.arms.split(",")
    sync = lambda: torch.cuda.synchronize(dev)

    def run_generate(groups, seed):
        """groups: [(B, T), ...] run one after the other -> mean latency in steps over the requests"""
        steps, lat = 0, 0
        for B, T in groups:
            pipe.generate_ids(None, B, T, 1.0, 5, [False] * T, seed, use_graph=True, streams=1)
            steps += T
            lat += B * steps
        return lat / sum(B for B, _ in groups)

    def run_session(ts, seed):
        s = pipe.decode_session(slots=S, conditional=False, use_graph=True, decode=False)
        hs = [s.submit(timesteps=T, temperature=1.0, topk=5, seed=seed + i) for i, T in enumerate(ts)]
        done = s.drain()
        assert len(done) == len(ts)
        return sum(h.retired + 1 for h in hs) / len(hs), s.tick

    if a.mode == "uniform":
        ts = [a.timesteps] * S
        groups = [(S, a.timesteps)]
        reps = a.reps
    else:
        mix = [int(x) for x in a.mix.split(",")]
        ts = [mix[i % len(mix)] for i in range(a.requests)]
        random.Random(0).shuffle(ts)
        groups = []
        for T in sorted(mix):
            left = ts.count(T)
            while left > 0:
                groups.append((min(S, left), T))
                left -= min(S, left)
        reps = 1
    work = {"session": lambda sd: run_session(ts, sd), "generate": lambda sd: (run_generate(groups, sd), sum(T for _, T in groups))}
    for arm in arms:                                   # eager pass, capture pass, replay: every shape the timed window uses
        for w in range(3):
            work[arm](w)
    sync()
    res = {arm: [] for arm in arms}
    info = {}
    for rnd in range(a.rounds):
        for arm in arms:
            sync()
            t0 = time.perf_counter()
            for rep in range(reps):
                info[arm] = work[arm](100 * rnd + rep)
            sync()
            dt = time.perf_counter() - t0
            res[arm].append(len(ts) * reps / dt)
    out = {"mode": a.mode, "root": os.path.abspath(a.root), "workload": a.workload, "dtype": a.dtype, "slots": S,
           "requests": len(ts), "reps": reps, "groups": groups if a.mode == "mixed" else None,
           "images_per_s": res,
           "mean_latency_steps": {arm: info[arm][0] for arm in arms}, "steps_run": {arm: info[arm][1] for arm in arms}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
