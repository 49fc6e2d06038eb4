"""What edit requests cost a decode session (results under profiles/).

Milliseconds per session step on the 12L/d512 model, S unconditional requests of T steps admitted together, graph replay:

  a  the default session, every slot a generation (the step without counts -- asserted from the handle's counter where there is one)
  b  the same session with every second slot an edit request over a half-masked start (the count array and the re-masking form
     with a count per slot, every step -- asserted from the counter)

The arms alternate inside one process, --rounds times; nothing is decoded (ids only).  A window's time is also split into the
submissions (an edit request counts its masked positions once, one device-to-host read each) and the steps, with a device
synchronise between the two.  A checkout without the feature runs arm a only: point --root at it (with --arms a) to time the
parent commit on the same box.
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose paintmind_amd is timed")
    ap.add_argument("--arms", default="a,b")
    ap.add_argument("--workload", default="bench-uncond-12L-d512")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--timesteps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=4, help="sessions per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import torch
    import paintmind_amd as pm
    from paintmind_amd.generate import Pipeline

    assert torch.cuda.is_available(), "slots_edit_bench needs a ROCm device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    pipe = Pipeline(pm.Config(pm.ver2cfg[a.workload]), stage1_pretrained=False).to(dev).eval()
    pipe.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    S, T, arms, N = a.slots, a.timesteps, a.arms.split(","), pipe.num_tokens
    # the edit requests' start: codes below the mask id with every second position masked (the same ids for every request)
    start = torch.randint(0, pipe.mask_token_id, (N,), generator=torch.Generator().manual_seed(1)).to(dev)
    start[::2] = pipe.mask_token_id
    counter = getattr(pipe.engine(), "slots_edit_steps", None)

    def run(arm, seed):
        t0 = time.perf_counter()
        s = pipe.decode_session(slots=S, conditional=False, use_graph=True, decode=False)
        for j in range(S):
            edit = arm == "b" and j % 2 == 1
            s.submit(timesteps=T, temperature=1.0, topk=5, seed=seed + j, **(dict(ids0=start, keep_given=True) if edit else {}))
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        assert len(s.drain()) == S and s.tick == T
        torch.cuda.synchronize(dev)
        return t1 - t0, time.perf_counter() - t1

    forms = {}
    for arm in arms:                                   # eager pass, capture pass, replay
        before = counter() if counter else 0
        for w in range(3):
            run(arm, w)
        forms[arm] = (counter() if counter else 0) - before
    assert forms.get("a", 0) == 0 and forms.get("b", 3 * T) == 3 * T, forms
    torch.cuda.synchronize(dev)
    ms = {arm: [] for arm in arms}
    parts = {arm: [] for arm in arms}                  # (submissions, steps) of the same windows, ms per step
    for rnd in range(a.rounds):
        for arm in arms:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            split = [run(arm, 100 * rnd + rep) for rep in range(a.reps)]
            torch.cuda.synchronize(dev)
            ms[arm].append(1e3 * (time.perf_counter() - t0) / (a.reps * T))
            parts[arm].append([round(1e3 * sum(x[i] for x in split) / (a.reps * T), 4) for i in (0, 1)])
    out = {"root": os.path.abspath(a.root), "workload": a.workload, "dtype": a.dtype, "slots": S, "timesteps": T, "reps": a.reps,
           "ms_per_step": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "median_ms_per_step": {k: round(sorted(v)[len(v) // 2], 4) for k, v in ms.items()},
           "submit_and_step_ms_per_step": parts, "edit_steps_of_the_warm_up": forms}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
