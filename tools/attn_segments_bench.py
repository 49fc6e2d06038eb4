"""Segmented cross-attention against the per-image-length form and the unmasked entry at a regional-prompts shape (default
B=64, H=12, Nq=1024, Nkv=231 = a global prompt and two regions of 77 rows, dh=64): microseconds per launch by hipEvents, bf16
(exp2) and fp32.  A measurement for DESIGN.md section 4u, no gate.  Layout of the masks: rows [0,77) segment 0 (global), [77,154)
segment 1, [154,231) segment 2; the left half of a 32 x 32 token grid attends to segments 0 and 1, the right half to 0 and 2.
Behind them the picked forms of DESIGN.md section 4v (pmhip_attention_pick): each form with every image served, every second one and
none -- the last is what a launch costs whose workgroups all return at once -- and the pair of launches of a half-regional batch.
Behind those the weighted form of DESIGN.md section 4w (pmhip_attention_weighted) under the same masks, with weights cycling through
1/8, 1, 8 and 1.3: the call of ``ops.attention(key_weights=)``, which converts the weights first (pmhip_key_bias, one more launch), and
that conversion alone.
Behind those the picked weighted form of DESIGN.md section 4x (pmhip_attention_pick_weighted, the bias converted once outside the
timed call as the engine does per step): every image served, every second one and none; the three launches of a batch mixed in
thirds (plain, regional, weighted); and the three launches with no weighted image, against the pair of 4v -- the difference is what
the now-third empty launch costs per layer."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from paintmind_amd import ops

dev = torch.device("cuda:0")
B, H, NQ, NKV = (int(x) for x in (sys.argv[1:5] if len(sys.argv) > 4 else (64, 12, 1024, 231)))
NKP = -(-NKV // 64) * 64
g = torch.Generator().manual_seed(0)
ks = (torch.arange(NKV) // -(-NKV // 3)).to(torch.uint8)[None].expand(B, NKV).contiguous().to(dev)
side = int(NQ ** 0.5) or 1
right = ((torch.arange(NQ) % side) >= side // 2).to(torch.int32)
qm = (1 | (2 << right))[None].expand(B, NQ).contiguous().to(dev)
lens = torch.full((B,), NKV, dtype=torch.int32, device=dev)


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


for dtype, exp2 in ((torch.bfloat16, True), (torch.float32, False)):
    q = ((torch.rand(B, H, NQ, 64, generator=g) * 2 - 1) * 0.5).to(dev).to(dtype)
    k = (torch.rand(B, H, NKP, 64, generator=g) * 2 - 1).to(dev).to(dtype)
    vt = (torch.rand(B, H, 64, NKP, generator=g) * 2 - 1).to(dev).to(dtype)
    plain = timed(lambda: ops.attention(q, k, vt, NKV, use_exp2=exp2))
    per_image = timed(lambda: ops.attention(q, k, vt, NKV, use_exp2=exp2, kv_lens=lens))
    seg = timed(lambda: ops.attention(q, k, vt, NKV, use_exp2=exp2, key_segments=ks, query_segments=qm))
    print(f"{dtype} B={B} H={H} Nq={NQ} Nkv={NKV}: unmasked {plain:.1f} us, lens {per_image:.1f} us, segments {seg:.1f} us "
          f"({seg / per_image:.2f} x lens)")
    if hasattr(ops, "key_bias"):
        w = torch.tensor([0.125, 1.0, 8.0, 1.3])[torch.arange(NKV) % 4][None].expand(B, NKV).contiguous().to(dev)
        weighted = timed(lambda: ops.attention(q, k, vt, NKV, use_exp2=exp2, key_segments=ks, query_segments=qm, key_weights=w))
        convert = timed(lambda: ops.key_bias(w, exp2))
        print(f"    weighted form (conversion included): {weighted:.1f} us ({weighted / seg:.2f} x segments, {weighted / per_image:.2f} x lens); "
              f"the conversion alone: {convert:.1f} us")
    if hasattr(ops, "attention_pick"):
        out = torch.empty(B * NQ, H * 64, device=dev, dtype=dtype)
        picks = {"all": torch.zeros(B, dtype=torch.uint8, device=dev), "half": (torch.arange(B) % 2).to(torch.uint8).to(dev),
                 "none": torch.ones(B, dtype=torch.uint8, device=dev)}
        lens_pick = {n: timed(lambda: ops.attention_pick(q, k, vt, NKV, p, 0, out, use_exp2=exp2, kv_lens=lens)) for n, p in picks.items()}
        seg_pick = {n: timed(lambda: ops.attention_pick(q, k, vt, NKV, 1 - p, 1, out, use_exp2=exp2, key_segments=ks, query_segments=qm))
                    for n, p in picks.items()}

        def pair():
            ops.attention_pick(q, k, vt, NKV, picks["half"], 0, out, use_exp2=exp2, kv_lens=lens)
            ops.attention_pick(q, k, vt, NKV, picks["half"], 1, out, use_exp2=exp2, key_segments=ks, query_segments=qm)
        fmt = lambda d: ", ".join(f"{n} served {v:.1f} us" for n, v in d.items())
        print(f"    picked lens form: {fmt(lens_pick)}; picked segments form: {fmt(seg_pick)}; both launches, half and half: {timed(pair):.1f} us")
    if "pmhip_attention_pick_weighted" in getattr(ops._lib, "PROTOTYPES", {}):
        from paintmind_amd.ops import _p, check, pm_dtype, stream_ptr
        lib, bias = ops._lib.load(), ops.key_bias(w, exp2)

        def pick_weighted(p, want):
            check(lib.pmhip_attention_pick_weighted(pm_dtype(dtype), _p(q), _p(k), _p(vt), _p(out), H * 64, B, H, 64, NQ, NKV, NKP, int(exp2), _p(ks),
                                                    _p(qm), _p(bias), _p(p), want, stream_ptr(dev)), "pmhip_attention_pick_weighted")
        w_pick = {n: timed(lambda: pick_weighted(p, 0)) for n, p in picks.items()}
        thirds = (torch.arange(B) % 3).to(torch.uint8).to(dev)

        def three(p):
            ops.attention_pick(q, k, vt, NKV, p, 0, out, use_exp2=exp2, kv_lens=lens)
            ops.attention_pick(q, k, vt, NKV, p, 1, out, use_exp2=exp2, key_segments=ks, query_segments=qm)
            pick_weighted(p, 2)
        mixed, three_half, two_half = timed(lambda: three(thirds)), timed(lambda: three(picks["half"])), timed(pair)
        print(f"    picked weighted form: {fmt(w_pick)}; three launches, a third of each kind: {mixed:.1f} us; three launches, half plain and half "
              f"regional: {three_half:.1f} us against the pair's {two_half:.1f} us (the empty third launch: {three_half - two_half:.1f} us)")
