"""The Flan-T5 tower on the HIP path against Hugging Face's: HIP events on the current device, one process, one
box.  Writes profiles/t5_native_bench.txt.
  The tower: random weights in the Flan-T5-XL shape (24 layers, d_model 2048, 32 heads of 64, d_ff 5120) with a 128-word vocabulary,
  B = 64 prompts of L = 77 rows.  Four arms -- Hugging Face f32 (how the reference loads it), Hugging Face bf16 (tower.to(bfloat16)),
  native f32, native bf16 -- alternate: ROUNDS rounds, each a warm-up and ITERS calls timed one by one; per arm the median over all of
  them, the fastest, and the spread of the round medians.  TFLOP/s counts the multiply-adds of the GEMMs and of Q K^T and P V (2 flops
  each), from the shapes.
  The three new operators alone at the tower's shapes, with the bytes they have to move (and, for the attention, its flops).
  Then ``Pipeline.generate(text)`` on the 12-layer d512 pipeline (bf16, 8 steps, 64 prompts) with the XL-shaped tower as its text model,
  native off (the Hugging Face f32 tower) and on (the native tower in the pipeline's compute dtype)."""
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import paintmind_amd as pm
from paintmind_amd import ops
from paintmind_amd._lib import PART_K, PART_Q, PART_V
from paintmind_amd.generate import Pipeline
from paintmind_amd.modules.encoder import T5TextEmbedder
from paintmind_amd.modules.t5_native import NativeT5Encoder, rel_bias_table

dev = torch.device("cuda:0")
B, L, ROUNDS, ITERS = 64, 77, 3, 5
LAYERS, D, H, F = 24, 2048, 32, 5120
OUT = os.path.join(ROOT, "profiles", "t5_native_bench.txt")
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


class CharTokenizer:
    """one id per character, pad 0, end-of-sequence 1 (the weights are random: only the shapes matter)"""
    pad_token_id, eos_token_id = 0, 1

    def __call__(self, text, max_length=77, add_special_tokens=True, **kw):
        if isinstance(text, str):
            return {"input_ids": [2 + ord(c) % 100 for c in text] + ([1] if add_special_tokens else [])}
        ids = torch.zeros(len(text), max_length, dtype=torch.long)
        for i, s in enumerate(text):
            row = [2 + ord(c) % 100 for c in s][:max_length - 1] + [1]
            ids[i, :len(row)] = torch.tensor(row)
        return {"input_ids": ids}


def xl_tower():
    from transformers import T5Config, T5EncoderModel
    torch.manual_seed(0)
    with torch.device(dev):
        return T5EncoderModel(T5Config(vocab_size=128, d_model=D, d_kv=64, d_ff=F, num_layers=LAYERS, num_heads=H,
                                       feed_forward_proj="gated-gelu")).eval()


def tower_flops(b):
    gemm = 2 * b * L * (4 * D * H * 64 + 3 * D * F)             # q, k, v, o and wi_0, wi_1, wo
    attn = 2 * b * H * 2 * L * L * 64                           # Q K^T and P V
    return LAYERS * (gemm + attn)


def tower(model):
    ids = torch.randint(2, 128, (B, L), generator=torch.Generator().manual_seed(1)).to(dev)
    low = copy.deepcopy(model).to(torch.bfloat16)
    native = NativeT5Encoder(model)
    with torch.no_grad():
        ref = model(input_ids=ids).last_hidden_state
        for name, got in (("Hugging Face bf16", low(input_ids=ids).last_hidden_state.float()), ("native f32", native(ids, dtype=torch.float32)),
                          ("native bf16", native(ids, dtype=torch.bfloat16))):
            d = (got - ref).double()
            say(f"{name} against Hugging Face f32 (not an error measurement: both sides round): RMS {float(d.pow(2).mean().sqrt()):.3g}, "
                f"max abs {float(d.abs().max()):.3g}")

    def hf(m):
        with torch.no_grad():
            m(input_ids=ids)
    arms = {"Hugging Face f32": lambda: hf(model), "Hugging Face bf16": lambda: hf(low),
            "native f32": lambda: native(ids, dtype=torch.float32), "native bf16": lambda: native(ids, dtype=torch.bfloat16)}
    flops = tower_flops(B)
    say(f"tower: {LAYERS} layers, d_model {D}, {H} heads of 64, d_ff {F}; B = {B}, L = {L}: {flops / 1e12:.2f} TFLOP per call "
        f"({tower_flops(1) / 1e9:.0f} GFLOP per prompt); {ROUNDS} rounds x {ITERS} calls per arm, each call between its own events")
    res = alternate(arms)
    for name, (med, best, meds) in res.items():
        say(f"{name}: median {med / 1e3:.2f} ms = {flops / med / 1e6:.0f} TFLOP/s; fastest {best / 1e3:.2f} ms; round medians "
            f"{[round(x / 1e3, 2) for x in meds]} ms, spread (max - min) / min {(max(meds) - min(meds)) / min(meds) * 100:.1f} %")
    for a, b_ in (("native f32", "Hugging Face f32"), ("native bf16", "Hugging Face bf16"), ("native bf16", "Hugging Face f32")):
        say(f"{a} / {b_}: {res[a][0] / res[b_][0]:.3f} of its time")
    del low


def operators(model):
    M = B * L
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn(M, D, device=dev, generator=g)
    w = torch.ones(D, device=dev)
    u = torch.randn(M, 2 * F, device=dev, generator=g)
    bias = rel_bias_table(model.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight, L)
    wqkv = torch.randn(3 * H * 64, D, device=dev, generator=g) * 0.02
    arms, cost = {}, {}
    for dt, size in ((torch.float32, 4), (torch.bfloat16, 2)):
        tag = "f32" if dt == torch.float32 else "bf16"
        arms[f"rmsnorm [{M}, {D}] -> {tag}"] = lambda dt=dt: ops.rmsnorm(x, w, 1e-6, dt)
        cost[f"rmsnorm [{M}, {D}] -> {tag}"] = (M * D * (4 + size), 0)
        arms[f"geglu [{M}, {2 * F}] -> {tag} [{M}, {F}]"] = lambda dt=dt: ops.geglu(u, dt)
        cost[f"geglu [{M}, {2 * F}] -> {tag} [{M}, {F}]"] = (M * F * (8 + size), 0)
        q, k, vt = ops.gemm_heads(x.to(dt), wqkv.to(dt), H, L, [PART_Q, PART_K, PART_V], q_scale=1.0)
        out = torch.empty(M, H * 64, device=dev, dtype=dt)
        name = f"attention_relbias {tag} B {B}, H {H}, L {L}"
        arms[name] = lambda q=q, k=k, vt=vt, out=out: ops.attention_relbias(q, k, vt, bias, out=out)
        cost[name] = (4 * B * H * L * 64 * size, 2 * B * H * 2 * L * L * 64)        # Q, K, V^T read, out written; Q K^T and P V
    say(f"the new operators alone, {ROUNDS} rounds x 10 launches per arm, each launch between its own events")
    for name, (med, best, meds) in alternate(arms, iters=10).items():
        nbytes, flops = cost[name]
        extra = f", {flops / med / 1e6:.1f} TFLOP/s" if flops else ""
        say(f"{name}: median {med:.1f} us = {nbytes / med / 1e6:.2f} TB/s of {nbytes / 2 ** 20:.1f} MiB{extra}; fastest {best:.1f} us; "
            f"spread of the round medians {(max(meds) - min(meds)) / min(meds) * 100:.1f} %")


def pipeline(model):
    emb = T5TextEmbedder(tokenizer=CharTokenizer(), transformer=model)
    torch.manual_seed(0)
    cfg = dict(pm.ver2cfg["bench-uncond-12L-d512"], context_dim=D)
    pipe = Pipeline(pm.Config(cfg), stage1_pretrained=False, text_model=emb).eval().to(dev)
    pipe.set_compute_dtype(torch.bfloat16)
    text = [f"prompt number {i} of the batch" for i in range(B)]

    def gen():
        pipe.generate(text, timesteps=8, topk=5, seed=1)
    say(f"Pipeline.generate(text) on the 12-layer d512 pipeline, bf16, 8 steps, {B} prompts, the XL-shaped tower as text model")
    res = {}
    for _ in range(2):                                               # alternating
        for name, on in (("native off (Hugging Face f32 tower)", False), ("native on (native bf16 tower)", True)):
            emb.use_native(on)
            res.setdefault(name, []).extend(times(gen, iters=3, warm=1))
    for name, v in res.items():
        say(f"{name}: median {statistics.median(v) / 1e3:.1f} ms of {len(v)} (fastest {min(v) / 1e3:.1f} ms) = "
            f"{B / statistics.median(v) * 1e6:.0f} images/s")


if __name__ == "__main__":
    say(f"device: {torch.cuda.get_device_name(0)}")
    model = xl_tower()
    tower(model)
    torch.cuda.empty_cache()
    operators(model)
    torch.cuda.empty_cache()
    pipeline(model)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
