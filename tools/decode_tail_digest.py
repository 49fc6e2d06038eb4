"""Bit digest of the decode tail: sampling, re-masking, guidance combination and the tiny pipeline's decode loops.

  python tools/decode_tail_digest.py --root <built checkout> [--out file.jsonl]

One JSON line per case with a sha256 of every output tensor; inputs come from fixed numpy seeds.  The tests compare scores with a
tolerance; this is for "bit for bit what another commit computes": run it on two built checkouts on one box and diff the files
(profiles/decode_tail_digest_*.jsonl).  Only the public Python surface (ops, Pipeline) is used, so any commit that has the
nucleus filter (and so wide top-k, choice temperatures, context lengths and per-request guidance) can be the other side.
The last section -- regional prompts, prompt weights, a negative prompt under a schedule, edit, the attention maps and a session
that mixes the request kinds -- needs a commit that has prompt weights in sessions and the maps
(profiles/host_keys_digest_*.jsonl).  Behind every session and every dtype section one more line gives (entries, captured) of
the tiny pipeline's stage-2 graph cache (profiles/engine_records_digest_parent.jsonl).
"""
import argparse
import hashlib
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose paintmind_amd is run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    sys.path.insert(0, os.path.join(a.root, "tests"))
    import numpy as np
    import torch
    import paintmind_amd as pm
    from paintmind_amd import ops
    from paintmind_amd.generate import Pipeline
    from util import load_golden, to_torch_sd

    assert torch.cuda.is_available(), "decode_tail_digest needs a ROCm device"
    print("library under test:", pm.__file__, file=sys.stderr)
    dev = torch.device("cuda:0")
    out = open(a.out, "w") if a.out else None

    def sha(x):
        return hashlib.sha256(np.ascontiguousarray(x.detach().cpu().numpy()).tobytes()).hexdigest()

    def emit(case, **tensors):
        line = json.dumps({"case": case, **{k: sha(v) for k, v in tensors.items()}})
        print(line)
        if out:
            out.write(line + "\n")

    def emit_graphs(case):
        """(entries, captured) of the tiny pipeline's stage-2 graph cache: a changed graph key shows as a changed count even where
        the ids agree"""
        line = json.dumps({"case": case, "graph_count": list(pipe.engine().graph_count())})
        print(line)
        if out:
            out.write(line + "\n")

    def t(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def logits_of(rng, M, V, quantised):
        x = (rng.standard_normal((M, V)) * 2.0).astype(np.float32)
        return np.round(x * 2) / 2 if quantised else x             # half-integers: many ties

    def ids_of(rng, M, V):
        ids = rng.integers(0, V, M).astype(np.int64)
        ids[rng.random(M) < 0.6] = V
        return ids

    def stats_of(x):
        return ops.guidance_combine(x, x, 1.0, with_stats=True)[1]

    # ---- sample_rows: M = 37 (a partly empty last workgroup), one block / ragged V / the NB2 = 1, 2, 4 boundaries
    M, seed, base, number = 37, 0xFEDCBA9876543210, 2 ** 40 + 12345, 0
    for V in (64, 1000, 4160, 8192, 8256):
        rng = np.random.default_rng(V)
        planes = [t(logits_of(rng, M, V, q)) for q in (False, True)]
        stats = [stats_of(x) if V % 64 == 0 else None for x in planes]
        ids, noise = t(ids_of(rng, M, V)), t(rng.random((M, V)).astype(np.float32))
        for topk in (1, 5, 8, 9, min(64, V)):
            for temp in (0.0, 0.7):
                q = number % 2
                number += 1
                x = planes[q]
                for name, st in (("dense", None), ("stats", stats[q])):
                    if name == "stats" and st is None:
                        continue
                    pred, merged, score = ops.sample_rows(x, ids, V, topk, temp, seed=seed, step=5, row_base=base, block_stats=st)
                    emit(f"sample_rows V={V} k={topk} T={temp} ties={q} philox {name}", pred=pred, ids=merged, score=score)
                    if temp:
                        pred, merged, score = ops.sample_rows(x, ids, V, topk, temp, noise=noise, block_stats=st)
                        emit(f"sample_rows V={V} k={topk} T={temp} ties={q} noise {name}", pred=pred, ids=merged, score=score)

    # ---- sample_rows above 64 (the selection kernel, up to the whole row) and behind the nucleus filter (with topk = 5 and topk = V)
    for V in (1000, 8192):
        rng = np.random.default_rng(3 * V)
        planes = [t(logits_of(rng, M, V, q)) for q in (False, True)]
        ids, noise = t(ids_of(rng, M, V)), t(rng.random((M, V)).astype(np.float32))
        for q, x in enumerate(planes):
            for temp in (0.0, 0.7):
                for topk, top_p in ((65, None), (V, None), (5, 0.5), (5, 0.9), (V, 0.5), (V, 0.9)):
                    pred, merged, score = ops.sample_rows(x, ids, V, topk, temp, seed=seed, step=5, row_base=base, top_p=top_p)
                    emit(f"sample_rows V={V} k={topk} p={top_p} T={temp} ties={q} philox", pred=pred, ids=merged, score=score)
                    if temp:
                        pred, merged, score = ops.sample_rows(x, ids, V, topk, temp, noise=noise, top_p=top_p)
                        emit(f"sample_rows V={V} k={topk} p={top_p} T={temp} ties={q} noise", pred=pred, ids=merged, score=score)

    # ---- the slots forms: the record set of tests/test_gpu_slots.py::_operator_slots at N = 16
    N = 16
    recs = [(0x0123456789ABCDEF, 7, 0.0, 1, 1, 0), (77, 2 ** 33 + 5, 0.8, 8, N, 3), None,
            (0xFEDCBA9876543210, 4096, 1.3, 5, max(N // 2, 1), 17), (5, 1, 0.5, 3, 3, 1)]
    for V in (64, 8192):
        rng = np.random.default_rng(1000 * V + N)
        x, ids = t(logits_of(rng, 5 * N, V, False)), t(ids_of(rng, 5 * N, V))
        slots = ops.pack_slots(recs, dev)
        for name, st in (("dense", None), ("stats", stats_of(x))):
            pred, merged, score = ops.sample_rows_slots(x, ids, V, slots, N, block_stats=st)
            emit(f"sample_rows_slots V={V} {name}", pred=pred, ids=merged, score=score)
        emit(f"remask_slots V={V}", ids=ops.remask_slots(merged.reshape(5, N).clone(), score.reshape(5, N), slots, V))
        choice = t(np.array([4.5, 0.0, 2.0, 1.5, 0.25], dtype=np.float32))
        emit(f"remask_slots V={V} choice", ids=ops.remask_slots(merged.reshape(5, N).clone(), score.reshape(5, N), slots, V, choice=choice))

    # ---- remask: every elements-per-thread class, tied scores
    for N in (16, 100, 300, 1024, 2048, 4096):
        rng = np.random.default_rng(N)
        scores = t((rng.integers(0, 8, (3, N)) / 8.0).astype(np.float32))
        ids = t(rng.integers(0, 64, (3, N)).astype(np.int64))
        for nm in (1, N // 2, N):
            emit(f"remask N={N} num_mask={nm}", ids=ops.remask(ids.clone(), scores, nm, 64))
            emit(f"remask N={N} num_mask={nm} choice philox",
                 ids=ops.remask(ids.clone(), scores, nm, 64, choice_temperature=4.5, seed=seed, step=2, row_base=base))
        emit(f"remask N={N} num_mask={N // 2} choice noise",
             ids=ops.remask(ids.clone(), scores, N // 2, 64, choice_temperature=4.5, noise=t(rng.random((3, N)).astype(np.float32))))

    # ---- guidance: flat (with and without statistics, in place and not) and per image (guided, unguided, idle)
    rng = np.random.default_rng(7)
    tokens, V = 16, 192
    cond, unc = t(rng.standard_normal((3 * tokens, V)).astype(np.float32)), t(rng.standard_normal((3 * tokens, V)).astype(np.float32))
    emit("guidance_combine", out=ops.guidance_combine(cond, unc, 2.5))
    c2 = cond.clone()
    emit("guidance_combine into cond", out=ops.guidance_combine(c2, unc, 2.5, out=c2))
    o, st = ops.guidance_combine(cond, unc, 2.5, with_stats=True)
    emit("guidance_combine stats", out=o, stats=st)
    c2 = cond.clone()
    o, st = ops.guidance_combine(c2, unc, 2.5, out=c2, with_stats=True)
    emit("guidance_combine stats into cond", out=o, stats=st)
    slots = ops.pack_slots([(1, 0, 1.0, 5, 1, 0), (2, 1, 1.0, 5, 1, 0), None], dev)
    guides = ops.pack_slot_guides([1.75, None, 3.0], dev)
    emit("guidance_combine_slots", out=ops.guidance_combine_slots(cond, unc, guides, slots, tokens, out=torch.zeros_like(cond)))
    c2, st = cond.clone(), torch.zeros(3 * tokens, V // 64, 2, device=dev)
    o, st = ops.guidance_combine_slots(c2, unc, guides, slots, tokens, out=c2, block_stats=st)
    emit("guidance_combine_slots stats into cond", out=o, stats=st)

    # ---- the tiny pipeline of tests/test_gpu_step0.py::make_tiny: final ids and images of its loops
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False)
    pipe.load_state_dict(to_torch_sd(p), strict=False)
    pipe = pipe.to(dev).eval()
    B, T, flags = 3, 4, [False, True, False, True]
    rng = np.random.default_rng(11)
    Nt, mask = pipe.num_tokens, pipe.mask_token_id
    ctx = t(rng.standard_normal((4, 5, pipe.engine().context_dim)).astype(np.float32))
    start = rng.integers(0, mask, (B, Nt)).astype(np.int64)
    start[rng.random((B, Nt)) < 0.7] = mask
    for dtype in (torch.float32, torch.bfloat16):
        pipe.set_compute_dtype(dtype)
        pipe.invalidate_engines()
        tag = "fp32" if dtype == torch.float32 else "bf16"
        for topk in (3, 16):
            for src, ids0 in (("mask", None), ("ids", t(start))):
                for guided, kw in (("", {}), (" guided", {"guidance_scale": 2.0})):
                    context = ctx[:B].contiguous() if guided else None
                    for graph, calls in ((False, 1), (True, 3)):            # graph: the eager warm pass, the capture, one replay
                        for call in range(calls):
                            ids, imgs = pipe.generate_ids(context, B, T, 0.9, topk, flags, seed=1234, image_base=2 ** 33, use_graph=graph,
                                                          streams=1, ids0=None if ids0 is None else ids0.clone(), **kw)
                            emit(f"generate_ids {tag} k={topk} from={src}{guided} graph={int(graph)} call={call}", ids=ids, imgs=imgs)
        # the sampler options that came after the loops above: no top-k filter (topk = V), the nucleus filter behind topk = 5 and behind
        # none, the choice temperature, context lengths under guidance, and all of them in one call, also cut into two lanes
        full, lens = ctx[:B].contiguous(), [5, 2, 1]
        option_cases = [("k=V", dict(topk=None))]
        option_cases += [(f"k={k} p={p}", dict(topk=k, top_p=p)) for p in (0.5, 0.9) for k in (5, None)]
        option_cases += [("choice", dict(topk=5, choice_temperature=4.5)),
                         ("lens guided", dict(topk=5, context_lens=lens, guidance_scale=2.0)),
                         ("all", dict(topk=None, top_p=0.9, choice_temperature=4.5, context_lens=lens, guidance_scale=2.0))]
        for name, kw in option_cases:
            topk = kw.pop("topk")
            for graph, calls in ((False, 1), (True, 3)):
                for call in range(calls):
                    ids, imgs = pipe.generate_ids(full, B, T, 0.9, topk, flags, seed=1234, image_base=2 ** 33, use_graph=graph, streams=1, **kw)
                    emit(f"generate_ids {tag} {name} graph={int(graph)} call={call}", ids=ids, imgs=imgs)
            ids, imgs = pipe.generate_ids(full, B, T, 0.9, topk, flags, seed=1234, image_base=2 ** 33, use_graph=False, streams=2, **kw)
            emit(f"generate_ids {tag} {name} lanes=2", ids=ids, imgs=imgs)
            ids, img = pipe.sample(t(start), 0.5, text=full, topk=topk, temperature=0.8, seed=77, step=1, image_base=2 ** 33, **kw)
            emit(f"sample {tag} {name}", ids=ids, img=img)
        # the public loops: generate() through its host buffer and lanes, inpaint with three steps (the native loop from given ids)
        prompts = ["a", "b", "c"]
        imgs, ids = pipe.generate(prompts, timesteps=T, temperature=0.9, topk=None, save_interval=2, seed=5, image_base=2 ** 33, return_ids=True,
                                  streams=2, guidance_scale=2.0, context_lens=[70, 8, 1], choice_temperature=4.5, top_p=0.9)
        emit(f"generate {tag} all lanes=2", ids=ids, **{f"img{i}": im for i, im in enumerate(imgs)})
        picture = t((np.random.default_rng(13).random((2, 3, pipe.image_size, pipe.image_size)) * 2 - 1).astype(np.float32))
        half = pipe.image_size // 2
        for name, kw in (("choice", dict(choice_temperature=4.5)), ("choice p=0.9 k=V", dict(choice_temperature=4.5, top_p=0.9, topk=None))):
            img, ids = pipe.inpaint(picture, (0, 0, half, half), text=prompts[:2], timesteps=3, temperature=0.9, seed=9, return_ids=True,
                                    **dict(dict(topk=5), **kw))
            emit(f"inpaint {tag} T=3 {name}", ids=ids, img=img)
        # a decode session of three requests, each with its own choice temperature
        for graph in (False, True):
            s = pipe.decode_session(slots=3, conditional=True, use_graph=graph)
            for i, (steps, temp, topk, scale, choice) in enumerate([(3, 1.0, 5, None, 4.5), (4, 0.7, 3, 1.5, 1.0), (2, 1.3, 8, None, 0.25)]):
                s.submit(context=ctx[i, :5 - i], timesteps=steps, temperature=temp, topk=topk, seed=200 + i, image_index=2 ** 33 + i,
                         guidance_scale=scale, choice_temperature=choice)
            for f in sorted(s.drain(), key=lambda f: f.handle.number):
                emit(f"session choice {tag} graph={int(graph)} request={f.handle.number}", ids=f.ids, image=f.image)
            emit_graphs(f"session choice {tag} graph={int(graph)} graphs")
        # a decode session of four requests, two of them guided
        for graph in (False, True):
            s = pipe.decode_session(slots=4, conditional=True, use_graph=graph)
            for i, (steps, temp, topk, scale) in enumerate([(3, 1.0, 5, 2.0), (4, 0.7, 3, None), (2, 1.3, 8, 1.5), (4, 0.0, 1, None)]):
                s.submit(context=ctx[i], timesteps=steps, temperature=temp, topk=topk, seed=100 + i, image_index=2 ** 33 + i, guidance_scale=scale)
            for f in sorted(s.drain(), key=lambda f: f.handle.number):
                emit(f"session {tag} graph={int(graph)} request={f.handle.number}", ids=f.ids, image=f.image)
            emit_graphs(f"session {tag} graph={int(graph)} graphs")
        # the host request path: what says which context rows a token attends to (regional prompts, prompt weights alone and beside
        # lengths), a negative prompt under a guidance schedule, edit, the attention maps, and a session that mixes the request kinds
        krng = np.random.default_rng(17)
        ks = np.array([[0, 0, 1, 1, 255], [0, 1, 2, 255, 255], [0, 0, 0, 0, 1]], np.uint8)
        qm = (1 | (krng.integers(0, 4, (B, Nt)) << 1)).astype(np.uint32)
        w = np.array([[1, 1.4, 0.5, 2, 1], [1, 1, 0.25, 1, 1], [3, 1, 1, 1, 0]], np.float32)
        neg = ctx[1:4, :3].contiguous()
        key_cases = [("segments", dict(context_segments=ks, token_segments=qm)), ("weights", dict(context_weights=w)),
                     ("weights lens", dict(context_weights=w, context_lens=lens)),
                     ("negative schedule", dict(negative_context=neg, negative_lens=[3, 1, 2], guidance_scale=[0.5, 1.0, 2.0, 3.0]))]
        for name, kw in key_cases:
            for graph, calls in ((False, 1), (True, 3)):
                for call in range(calls):
                    ids, imgs = pipe.generate_ids(full, B, T, 0.9, 5, flags, seed=1234, image_base=2 ** 33, use_graph=graph, streams=1, **kw)
                    emit(f"generate_ids {tag} {name} graph={int(graph)} call={call}", ids=ids, imgs=imgs)
            ids, imgs = pipe.generate_ids(full, B, T, 0.9, 5, flags, seed=1234, image_base=2 ** 33, use_graph=False, streams=2, **kw)
            emit(f"generate_ids {tag} {name} lanes=2", ids=ids, imgs=imgs)
        for name, kw in key_cases[:3] + [("lens", dict(context_lens=lens))]:
            maps, logits = pipe.attention_maps(ids=t(start), text=full, return_logits=True, **kw)
            emit(f"attention_maps {tag} {name}", maps=maps, logits=logits)
        pixels = t((krng.random((2, pipe.image_size, pipe.image_size)) < 0.02).astype(np.uint8))
        env = os.environ.get("PMHIP_GENERATE_GRAPH")
        for graph, calls in ((False, 1), (True, 3)):
            os.environ["PMHIP_GENERATE_GRAPH"] = str(int(graph))
            for call in range(calls):
                img, ids = pipe.edit(picture, mask=pixels, text=prompts[:2], timesteps=3, temperature=0.9, topk=5, seed=9, preserve="pixels",
                                     guidance_scale=2.0, negative_text="d", mask_padding=True, return_ids=True)
                emit(f"edit {tag} pixels graph={int(graph)} call={call}", ids=ids, img=img)
        if env is None:
            del os.environ["PMHIP_GENERATE_GRAPH"]
        else:
            os.environ["PMHIP_GENERATE_GRAPH"] = env
        g = pipe.image_size // pipe.patch_size
        corner = torch.zeros(g, g, dtype=torch.bool)
        corner[:g // 2, :g // 2] = True
        for graph in (False, True):
            s = pipe.decode_session(slots=4, conditional=True, use_graph=graph, regions=True, weights=True)
            s.submit(context=ctx[0], timesteps=3, temperature=1.0, topk=5, seed=300, image_index=2 ** 33)
            s.submit(context=ctx[1, :3], regions=[(ctx[2, :2], corner)], timesteps=4, temperature=0.7, topk=3, seed=301, image_index=2 ** 33 + 1)
            s.submit(context=(ctx[2, :4], w[0, :4]), timesteps=2, temperature=1.3, topk=8, seed=302, image_index=2 ** 33 + 2)
            s.submit(context=ctx[3], negative_context=ctx[0, :2], guidance_scale=[2.0, 1.0, 0.5], timesteps=3, temperature=0.9, topk=5, seed=303,
                     image_index=2 ** 33 + 3)
            for f in sorted(s.drain(), key=lambda f: f.handle.number):
                emit(f"session mixed {tag} graph={int(graph)} request={f.handle.number}", ids=f.ids, image=f.image)
            emit_graphs(f"session mixed {tag} graph={int(graph)} graphs")
        emit_graphs(f"section {tag} graphs")
    pipe.set_compute_dtype(torch.float32)

    # ---- the sampler forms nothing above reaches (profiles/sampler_forms_digest_parent.jsonl): a count per image and per slot in
    # every elements-per-thread class of the re-masking kernel (E = 1, 2, 4, 8, 16), and the forced step in every row class
    for N in (16, 300, 1024, 2048, 4096):
        rng = np.random.default_rng(5000 + N)
        sc = (rng.integers(0, 8, (4, N)) / 8.0).astype(np.float32)
        sc[rng.random((4, N)) < 0.3] = -1e5                       # given ids: never drawn for, last in the order
        scores, ids = t(sc), t(rng.integers(0, 64, (4, N)).astype(np.int64))
        noise = t(rng.random((4, N)).astype(np.float32))
        counts = t(np.array([0, 1, N, N + 5], dtype=np.int32))
        emit(f"remask_counts N={N}", ids=ops.remask_counts(ids.clone(), scores, counts, 64))
        emit(f"remask_counts N={N} choice philox",
             ids=ops.remask_counts(ids.clone(), scores, counts, 64, choice_temperature=4.5, seed=seed, step=2, row_base=base))
        emit(f"remask_counts N={N} choice noise", ids=ops.remask_counts(ids.clone(), scores, counts, 64, choice_temperature=4.5, noise=noise))
        slots = ops.pack_slots([(0x0123456789ABCDEF, 7, 0.0, 1, 0, 0), (77, 2 ** 33 + 5, 0.8, 8, N, 3),
                                (0xFEDCBA9876543210, 4096, 1.3, 5, max(N // 2, 1), 17), None], dev)
        counts = t(np.array([-1, 0, max(N // 3, 1), 3], dtype=np.int32))    # the record's (clamped to 1), none, its own, idle with a count
        emit(f"remask_slots_counts N={N}", ids=ops.remask_slots_counts(ids.clone(), scores, slots, counts, 64))
        choice = t(np.array([4.5, 2.0, 0.25, 1.5], dtype=np.float32))
        emit(f"remask_slots_counts N={N} choice", ids=ops.remask_slots_counts(ids.clone(), scores, slots, counts, 64, choice=choice))
    for V in (64, 1000, 8192, 16384):
        rng = np.random.default_rng(7000 + V)
        x, ids = t(logits_of(rng, 9, V, False)), t(ids_of(rng, 9, V))
        target = rng.integers(0, V, 9).astype(np.int64)
        target[4] = V                                             # outside [0, V): the row stays undrawn
        pred, merged, score = ops.sample_rows_forced(x, ids, t(target), V)
        emit(f"sample_rows_forced V={V}", pred=pred, ids=merged, score=score)
    if out:
        out.close()


if __name__ == "__main__":
    main()
