"""Decode sessions against the batch decode loop ("Decode sessions"; results under profiles/).

  uniform  S identical requests (T steps each) admitted together: the session (graph replay of the slots step) against
           generate_ids(use_graph=True, streams=1) on the same commit -- what per-image decode state costs when nothing differs.
  mixed    R requests with T drawn from a set in equal shares, all queued at time 0: the session against the best the scalar
           loop can do (sort by T, one generate_ids per homogeneous group of at most S).  Images/s and the mean request latency
           in decode steps (session: the tick a request retires at + 1; sorted groups: the steps run up to the end of its group).

  guided   per-request guidance, --part kernel | session | all:
           kernel   guidance_slots_kernel<true> (every image guided, then every second one) against guidance_kernel<true> on the
                    same planes (--rows x --classes, in place at scale 1 so that the values stay put), alternating, --launches
                    each, timed with events; run it under ``rocprofv3 --kernel-trace --stats --`` for the per-kernel figures.
           session  S conditional requests (T steps, scale --scale) admitted together: the guided session against
                    generate_ids(guidance_scale=, use_graph=True, streams=1); then the same with every second request unguided
                    against one generate_ids per homogeneous group (S/2 guided, S/2 unguided).

  negative a negative prompt per request: milliseconds per session step by tower passes -- S conditional
           requests (T steps, a [77, D] context each) admitted together, all unguided (one pass), all guided without a negative
           prompt (two), all guided against a --neg-rows negative context (two, the second against the negative K/V), half and
           half (three).  --arms picks among one,two_uncond,two_negative,three: a commit without the feature runs the first two.

  regions  regional prompts per request: milliseconds per session step, hipEvents around every step of a
           session of S conditional requests (T steps, a [77, D] global context each) admitted together behind two warm-up sessions
           (eager, capture), the admission step left out -- none regional (the steps of a session without the option), every second
           one, all of them (two region prompts of 77 rows each over halves of the grid: a total of 231 rows, the capacity).
           --arms picks among none,half,all; a commit without the feature runs ``--arms none`` (point --root at it).

  weights  prompt weights per request: milliseconds per session step, measured like ``regions`` -- S conditional
           requests (T steps, a [77, D] context each, the capacity) admitted together, none weighted (a weights session's steps without
           such a request: the steps of a session without the option), every second one, all of them (weights cycling through 1/8,
           1, 8 and 1.3 over the rows).  --arms picks among none,half,all; a commit without the feature runs ``--arms none`` (point
           --root at it: the option is then left out).

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
    ap.add_argument("--mode", default="uniform", choices=["uniform", "mixed", "guided", "negative", "regions", "weights"])
    ap.add_argument("--arms", default="session,generate")
    ap.add_argument("--workload", default=None, help="default: bench-uncond-12L-d512; guided: bench-text-24L-d768")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--timesteps", type=int, default=None, help="default: 8; guided: 12")
    ap.add_argument("--part", default="all", choices=["kernel", "session", "all"], help="guided: which half to run")
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--neg-rows", type=int, default=77, help="negative: rows of every request's negative context")
    ap.add_argument("--rows", type=int, default=65536, help="guided kernel: rows of the planes (a multiple of --tokens)")
    ap.add_argument("--classes", type=int, default=8192)
    ap.add_argument("--tokens", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=6)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--mix", default="8,12,18")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=6, help="uniform: batches per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.workload = a.workload or ("bench-text-24L-d768" if a.mode == "guided" else "bench-uncond-12L-d512")
    a.timesteps = a.timesteps or (12 if a.mode == "guided" else 8)
    if a.mode == "negative" and a.arms == "session,generate":
        a.arms = "one,two_uncond,two_negative,three"
    sys.path.insert(0, a.root)
    import torch
    import paintmind_amd as pm
    from paintmind_amd.generate import Pipeline

    assert torch.cuda.is_available(), "slots_bench needs a ROCm device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if a.mode == "guided":
        out = {"mode": "guided", "root": os.path.abspath(a.root), "dtype": a.dtype}
        if a.part in ("kernel", "all"):
            out["kernel"] = guided_kernel(a, dev)
        if a.part in ("session", "all"):
            out["session"] = guided_session(a, dev)
        emit(out, a.out)
        return
    if a.mode == "negative":
        emit(negative_session(a, dev), a.out)
        return
    if a.mode == "regions":
        if a.arms == "session,generate":
            a.arms = "none,half,all"
        emit(regions_session(a, dev), a.out)
        return
    if a.mode == "weights":
        if a.arms == "session,generate":
            a.arms = "none,half,all"
        emit(weights_session(a, dev), a.out)
        return
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
    emit(out, a.out)


def emit(out, path):
    line = json.dumps(out)
    print(line)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def guided_kernel(a, dev):
    """ms per launch: the flat combination, the per-image one with every image guided, with every second image guided"""
    import torch
    from paintmind_amd import ops
    M, V, N = a.rows, a.classes, a.tokens
    B = M // N
    g = torch.Generator(device=dev).manual_seed(1)
    cond = torch.randn(M, V, device=dev, generator=g)
    unc = torch.randn(M, V, device=dev, generator=g)
    stats = torch.empty(M, V // 64, 2, device=dev)
    slots = ops.pack_slots([(1, b, 1.0, 5, 1, 0) for b in range(B)], dev)
    every = ops.pack_slot_guides([1.0] * B, dev)
    half = ops.pack_slot_guides([1.0 if b % 2 == 0 else None for b in range(B)], dev)
    arms = {"guidance_kernel": lambda: ops.guidance_combine(cond, unc, 1.0, out=cond, with_stats=True),
            "guidance_slots_kernel": lambda: ops.guidance_combine_slots(cond, unc, every, slots, N, out=cond, block_stats=stats),
            "guidance_slots_kernel_half": lambda: ops.guidance_combine_slots(cond, unc, half, slots, N, out=cond, block_stats=stats)}
    for f in arms.values():
        f()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in arms}
    for _ in range(a.launches):
        for k, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {"rows": M, "classes": V, "tokens": N, "images": B, "guided_row_bytes": 3 * V * 4, "ms": ms}


def guided_session(a, dev):
    import torch
    import paintmind_amd as pm
    from paintmind_amd.generate import Pipeline
    pipe = Pipeline(pm.Config(pm.ver2cfg[a.workload]), stage1_pretrained=False).to(dev).eval()
    pipe.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    S, T, scale = a.slots, a.timesteps, a.scale
    ctx = torch.randn(S, 77, pipe.engine().context_dim, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    sync = lambda: torch.cuda.synchronize(dev)

    def run_generate(groups, seed):
        at = 0
        for B, sc in groups:
            pipe.generate_ids(ctx[at:at + B].contiguous(), B, T, 1.0, 5, [False] * T, seed, use_graph=True, streams=1, guidance_scale=sc)
            at += B

    def run_session(scales, seed):
        s = pipe.decode_session(slots=S, conditional=True, use_graph=True, decode=False)
        for i, sc in enumerate(scales):
            s.submit(context=ctx[i], timesteps=T, temperature=1.0, topk=5, seed=seed + i, guidance_scale=sc)
        assert len(s.drain()) == S and s.tick == T

    mixed = [scale] * (S // 2) + [None] * (S - S // 2)
    work = {"session_guided": lambda sd: run_session([scale] * S, sd),
            "generate_guided": lambda sd: run_generate([(S, scale)], sd),
            "session_half_guided": lambda sd: run_session(mixed, sd),
            "generate_two_groups": lambda sd: run_generate([(S // 2, scale), (S - S // 2, None)], sd)}
    for f in work.values():                            # eager pass, capture pass, replay
        for w in range(3):
            f(w)
    sync()
    res = {arm: [] for arm in work}
    for rnd in range(a.rounds):
        for arm, f in work.items():
            sync()
            t0 = time.perf_counter()
            for rep in range(a.reps):
                f(100 * rnd + rep)
            sync()
            res[arm].append(S * a.reps / (time.perf_counter() - t0))
    one, two = pipe.engine().slots_steps()
    return {"workload": a.workload, "slots": S, "timesteps": T, "scale": scale, "reps": a.reps, "images_per_s": res,
            "slots_steps": {"one_pass": one, "two_pass": two}}


def negative_session(a, dev):
    """ms per session step (graph replay, nothing decoded) by the tower passes the step runs"""
    import torch
    import paintmind_amd as pm
    from paintmind_amd.generate import Pipeline
    pipe = Pipeline(pm.Config(pm.ver2cfg[a.workload]), stage1_pretrained=False).to(dev).eval()
    pipe.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    S, T, scale = a.slots, a.timesteps, a.scale
    D = pipe.engine().context_dim
    g = torch.Generator(device=dev).manual_seed(2)
    ctx = torch.randn(S, 77, D, device=dev, generator=g)
    neg = torch.randn(S, a.neg_rows, D, device=dev, generator=g)
    # per arm: (guided, with a negative prompt) of request i
    kinds = {"one": lambda i: (False, False), "two_uncond": lambda i: (True, False), "two_negative": lambda i: (True, True),
             "three": lambda i: (True, i % 2 == 1)}
    arms = a.arms.split(",")

    def run(arm, seed):
        s = pipe.decode_session(slots=S, conditional=True, use_graph=True, decode=False)
        for i in range(S):
            guided, negative = kinds[arm](i)
            kw = dict(negative_context=neg[i]) if negative else {}
            s.submit(context=ctx[i], timesteps=T, temperature=1.0, topk=5, seed=seed + i, guidance_scale=scale if guided else None, **kw)
        assert len(s.drain()) == S and s.tick == T

    for arm in arms:                                   # eager pass, capture pass, replay
        for w in range(3):
            run(arm, w)
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
    out = {"mode": "negative", "root": os.path.abspath(a.root), "workload": a.workload, "dtype": a.dtype, "slots": S, "timesteps": T,
           "context_rows": 77, "negative_rows": a.neg_rows, "scale": scale, "reps": a.reps, "ms_per_step": ms}
    eng = pipe.engine()
    if hasattr(eng, "slots_passes"):
        out["slots_passes"] = dict(zip(("one", "two", "three"), eng.slots_passes()))
    return out


def regions_session(a, dev):
    """ms per session step (graph replay, nothing decoded), by how many of the S requests carry regional prompts"""
    import torch
    import paintmind_amd as pm
    from paintmind_amd.generate import Pipeline
    pipe = Pipeline(pm.Config(pm.ver2cfg[a.workload]), stage1_pretrained=False).to(dev).eval()
    pipe.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    S, T = a.slots, max(a.timesteps, 21)
    D, g = pipe.engine().context_dim, pipe.image_size // pipe.patch_size
    gen = torch.Generator().manual_seed(2)
    ctx = torch.randn(S, 3, 77, D, generator=gen)
    left = torch.zeros(g, g, dtype=torch.bool)
    left[:, :g // 2] = True
    share = {"none": lambda i: False, "half": lambda i: i % 2 == 1, "all": lambda i: True}
    arms = a.arms.split(",")

    def run(arm, seed, timed):
        kw = dict(regions=True) if arm != "none" else {}
        s = pipe.decode_session(slots=S, conditional=True, use_graph=True, decode=False, max_context_len=231, **kw)
        for i in range(S):
            rk = dict(regions=[(ctx[i, 1], left), (ctx[i, 2], ~left)]) if share[arm](i) else {}
            s.submit(context=ctx[i, 0], timesteps=T, temperature=1.0, topk=5, seed=seed + i, **rk)
        ms = []
        for step in range(T):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s.step()
            e1.record()
            if timed and step > 0:
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        assert s.idle()
        return ms

    for arm in arms:                                   # eager pass, capture pass
        for w in range(2):
            run(arm, w, False)
    torch.cuda.synchronize(dev)
    ms = {arm: [] for arm in arms}
    for rnd in range(a.rounds):
        for arm in arms:
            ms[arm] += run(arm, 100 * rnd, True)
    stat = lambda v: {"steps": len(v), "median": sorted(v)[len(v) // 2], "mean": sum(v) / len(v), "min": min(v)}
    out = {"mode": "regions", "root": os.path.abspath(a.root), "workload": a.workload, "dtype": a.dtype, "slots": S, "timesteps": T,
           "global_rows": 77, "region_rows": [77, 77], "capacity": 231, "ms_per_step": {arm: stat(v) for arm, v in ms.items()}}
    eng = pipe.engine()
    if hasattr(eng, "slots_region_steps"):
        out["slots_region_steps"] = eng.slots_region_steps()
    return out


def weights_session(a, dev):
    """ms per session step (graph replay, nothing decoded), by how many of the S requests carry prompt weights"""
    import inspect
    import torch
    import paintmind_amd as pm
    from paintmind_amd.generate import Pipeline
    pipe = Pipeline(pm.Config(pm.ver2cfg[a.workload]), stage1_pretrained=False).to(dev).eval()
    pipe.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    S, T = a.slots, max(a.timesteps, 21)
    D = pipe.engine().context_dim
    ctx = torch.randn(S, 77, D, generator=torch.Generator().manual_seed(2))
    w = torch.tensor([0.125, 1.0, 8.0, 1.3])[torch.arange(77) % 4].numpy()
    share = {"none": lambda i: False, "half": lambda i: i % 2 == 1, "all": lambda i: True}
    arms = a.arms.split(",")
    has_option = "weights" in inspect.signature(Pipeline.decode_session).parameters

    def run(arm, seed, timed):
        kw = dict(weights=True) if has_option else {}
        s = pipe.decode_session(slots=S, conditional=True, use_graph=True, decode=False, max_context_len=77, **kw)
        for i in range(S):
            s.submit(context=(ctx[i], w) if share[arm](i) else ctx[i], timesteps=T, temperature=1.0, topk=5, seed=seed + i)
        ms = []
        for step in range(T):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s.step()
            e1.record()
            if timed and step > 0:
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        assert s.idle()
        return ms

    for arm in arms:                                   # eager pass, capture pass
        for k in range(2):
            run(arm, k, False)
    torch.cuda.synchronize(dev)
    ms = {arm: [] for arm in arms}
    for rnd in range(a.rounds):
        for arm in arms:
            ms[arm] += run(arm, 100 * rnd, True)
    stat = lambda v: {"steps": len(v), "median": sorted(v)[len(v) // 2], "mean": sum(v) / len(v), "min": min(v)}
    out = {"mode": "weights", "root": os.path.abspath(a.root), "workload": a.workload, "dtype": a.dtype, "slots": S, "timesteps": T,
           "context_rows": 77, "option": has_option, "ms_per_step": {arm: stat(v) for arm, v in ms.items()}}
    eng = pipe.engine()
    if hasattr(eng, "slots_weight_steps"):
        out["slots_weight_steps"] = eng.slots_weight_steps()
    out["graphs"] = list(eng.graph_count())
    return out


if __name__ == "__main__":
    main()
