"""Bit digest of the eager decode flows: prompt-to-prompt's ``control_ids`` with and without blend, forced
source and guidance, ``forced_ids``, ``diff_mask``, ``token_scores`` / ``score`` / ``surprise_mask`` on the tiny pipeline, 2 pairs.

  python tools/eager_flows_digest.py --root <built checkout> [--device cpu|cuda] [--dtype fp32|bf16] [--out file.jsonl]

One JSON line per case with a sha256 over the raw bytes of every output tensor; the inputs come from fixed seeds.  Only public
methods of ``Pipeline`` are called, so any commit that has ``token_scores`` can be the other side: run it on two built checkouts on
one box and diff the files (profiles/eager_steps_refactor.txt).  On the CPU the compute dtype plays no part."""
import argparse
import hashlib
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose paintmind_amd is run")
    ap.add_argument("--device", default="cuda", choices=("cpu", "cuda"))
    ap.add_argument("--dtype", default="fp32", choices=("fp32", "bf16"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    sys.path.insert(0, os.path.join(a.root, "tests"))
    import numpy as np
    import torch
    import paintmind_amd as pm
    from paintmind_amd.generate import Pipeline
    from util import load_golden, to_torch_sd

    print("library under test:", pm.__file__, file=sys.stderr)
    dev = torch.device("cuda:0" if a.device == "cuda" else "cpu")
    out = open(a.out, "w") if a.out else None

    def sha(x):
        return hashlib.sha256(np.ascontiguousarray(x.detach().cpu().numpy()).tobytes()).hexdigest()

    def emit(case, *tensors):
        line = json.dumps({"case": f"{a.device} {a.dtype} {case}", **{f"out{i}": sha(v) for i, v in enumerate(tensors)}})
        print(line)
        if out:
            out.write(line + "\n")

    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False)
    pipe.load_state_dict(to_torch_sd(p), strict=False)
    pipe = pipe.to(dev).eval()
    if a.device == "cuda":
        pipe.set_compute_dtype(torch.float32 if a.dtype == "fp32" else torch.bfloat16)
    B, T, N, V, S = 2, 3, pipe.num_tokens, pipe.mask_token_id, pipe.image_size
    g = S // pipe.patch_size
    gen = torch.Generator().manual_seed(21)
    rows = pipe.text_model(["a", "b", "c", "d"]).detach().cpu().float()
    L = rows.shape[1]
    lens_src, lens_edit = [L, L - 27], [L - 17, L - 44]
    src, edit = rows[:B].contiguous().to(dev), rows[B:].contiguous().to(dev)
    rm = np.tile(np.arange(L, dtype=np.int32), (B, 1))
    rm[:, ::5] = -1
    bl, gn = np.full((B, L), 0.5, np.float32), np.ones((B, L), np.float32)
    gn[:, 3:6] = 1.7
    w_src, w_edit = np.zeros((B, L), np.float32), np.zeros((B, L), np.float32)
    w_src[:, 3:7], w_edit[:, 5:8] = 1.0, 1.0
    source = torch.randint(0, V, (B, N), generator=gen)
    block = torch.zeros(B, g, g, dtype=torch.bool)
    block[:, 1:3, 1:3] = True
    img = (torch.rand(B, 3, S, S, generator=gen) * 2 - 1).to(dev)

    # ---- control_ids: the call of tests/test_steps_cpu.py, then the keywords one by one
    args = (src, edit, lens_src, lens_edit, rm, bl, gn, B, T, 1.0, 3, 7)
    cases = [("all", dict(guidance_scale=2.0, blend_rows=(w_src, w_edit), source_ids=source, cross_steps=0.5, blend_start=0.4, want_imgs=True)),
             ("plain", dict(want_imgs=True)),
             ("self", dict(cross_steps=0.5, self_steps=0.4, layers=[1])),
             ("no control", dict(cross_steps=0.0)),
             ("scale", dict(guidance_scale=2.0)),
             ("choice top_p", dict(choice_temperature=4.5, top_p=0.9, image_base=5)),
             ("source", dict(source_ids=source, want_imgs=True)),
             ("blend_rows", dict(blend_rows=(w_src, w_edit), blend_threshold=0.9, blend_grow=0, return_mask=True)),
             ("blend_mask", dict(blend_mask=block, blend_start=0.0, return_mask=True, want_imgs=True)),
             ("blend_rows source scale choice", dict(blend_rows=(w_src, w_edit), source_ids=source, guidance_scale=1.5, choice_temperature=2.0,
                                                     blend_threshold=0.9, blend_grow=0, return_mask=True))]
    for name, kw in cases:
        emit(f"control_ids {name}", *pipe.control_ids(*args, **kw))

    # ---- forced_ids
    emit("forced_ids scale", pipe.forced_ids(source, src, B, T, 7, guidance_scale=2.0))
    emit("forced_ids steps", *pipe.forced_ids(source, src, B, T, 7, context_lens=lens_src, choice_temperature=4.5, image_base=3, return_steps=True))
    emit("forced_ids no context", *pipe.forced_ids(source, None, B, T, 7, return_steps=True))

    # ---- diff_mask, both kinds
    for kind in ("tv", "jeffreys"):
        emit(f"diff_mask {kind}", *pipe.diff_mask(img, src, edit, draws=2, kind=kind, threshold=0.8, grow=0, return_score=True))
    emit("diff_mask defaults", *pipe.diff_mask(img, src, edit, return_score=True))
    emit("diff_mask lens", *pipe.diff_mask(img, src, edit, draws=3, mask_ratio=0.4, seed=5, threshold=0.7, grow=0, context_lens=lens_src,
                                           edit_context_lens=lens_edit, return_score=True))

    # ---- the likelihood maps and what is built on them
    emit("token_scores scale", *pipe.token_scores(img, src, draws=2, guidance_scale=2.0))
    emit("token_scores", *pipe.token_scores(img, src, context_lens=lens_src))
    emit("token_scores no text", *pipe.token_scores(img))
    ids = source.clone()
    ids[:, ::7] = V
    emit("token_scores ids", *pipe.token_scores(ids=ids, text=edit, draws=3, seed=2))
    emit("score relative", pipe.score(img, src, relative=True))
    emit("score scale", pipe.score(ids=ids, text=src, guidance_scale=1.5))
    emit("surprise_mask", *pipe.surprise_mask(img, src, return_score=True))
    emit("surprise_mask threshold", *pipe.surprise_mask(img, src, threshold=0.7, grow=0, return_score=True))
    emit("surprise_mask scale", *pipe.surprise_mask(img, edit, threshold=0.8, grow=0, return_score=True, guidance_scale=2.0, draws=2))
    if out:
        out.close()


if __name__ == "__main__":
    main()
