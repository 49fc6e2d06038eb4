"""What the sampler filters per request cost a decode session (results under profiles/).

Milliseconds per session step on the 12L/d512 model, S unconditional requests of T steps admitted together, graph replay:

  a  the default session, every slot topk = 5
  b  filters=True, every slot topk = 5 (class T only: the step with the one sampling launch -- asserted from the handle's counter)
  c  filters=True, S - 1 slots topk = 5 and ONE slot topk = 200 (class W): the four launches, nearly all of their waves returning
  d  filters=True, the slots split evenly over T (topk 5), R (32), W (200) and N (no top-k, top_p 0.9)

The arms alternate inside one process, --rounds times; nothing is decoded (ids only).  A checkout without the feature runs arm a
only: point --root at it (with --arms a) to time the parent commit on the same box.
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose paintmind_amd is timed")
    ap.add_argument("--arms", default="a,b,c,d")
    ap.add_argument("--workload", default="bench-uncond-12L-d512")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--timesteps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4, help="sessions per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import torch
    import paintmind_amd as pm
    from paintmind_amd.generate import Pipeline

    assert torch.cuda.is_available(), "slots_filter_bench needs a ROCm device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(pm.ver2cfg[a.workload]), stage1_pretrained=False).to(dev).eval()
    pipe.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    S, T, arms = a.slots, a.timesteps, a.arms.split(",")
    t5, r32, w200, n09 = (5, None), (32, None), (200, None), (None, 0.9)
    filters = {"a": [t5] * S, "b": [t5] * S, "c": [t5] * (S - 1) + [w200], "d": [(t5, r32, w200, n09)[j * 4 // S] for j in range(S)]}

    def run(arm, seed):
        kw = {} if arm == "a" else {"filters": True}
        s = pipe.decode_session(slots=S, conditional=False, use_graph=True, decode=False, **kw)
        for j, (topk, top_p) in enumerate(filters[arm]):
            s.submit(timesteps=T, temperature=1.0, topk=topk, seed=seed + j, **({} if arm == "a" else {"top_p": top_p}))
        assert len(s.drain()) == S and s.tick == T

    forms = {}
    for arm in arms:                                   # eager pass, capture pass, replay
        before = pipe.engine().slots_filter_steps() if arm != "a" else None
        for w in range(3):
            run(arm, w)
        if before is not None:
            forms[arm] = [x - y for x, y in zip(pipe.engine().slots_filter_steps(), before)]
    assert forms.get("b", [3 * T, 0]) == [3 * T, 0] and forms.get("c", [0, 3 * T]) == [0, 3 * T], forms
    torch.cuda.synchronize(dev)
    ms = {arm: [] for arm in arms}
    for rnd in range(a.rounds):
        for arm in arms:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for rep in range(a.reps):
                run(arm, 100 * rnd + rep)
            torch.cuda.synchronize(dev)
            ms[arm].append(1e3 * (time.perf_counter() - t0) / (a.reps * T))
    out = {"root": os.path.abspath(a.root), "workload": a.workload, "dtype": a.dtype, "slots": S, "timesteps": T, "reps": a.reps,
           "ms_per_step": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "median_ms_per_step": {k: round(sorted(v)[len(v) // 2], 4) for k, v in ms.items()},
           "filter_steps_of_the_warm_up": forms}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
