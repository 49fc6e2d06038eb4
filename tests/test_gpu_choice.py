"""MaskGIT's choice temperature on the GPU: the choice form of the re-masking kernel against the float64
restatement of tests/choice_ref.py and against the plain kernel it shares its body with, and the model-level entries against the
operator composition, the eager loop, the lanes and the decode session -- all of those bit for bit."""
import numpy as np
import pytest
import torch

import choice_ref as R
import paintmind_amd as pm
from gpu_common import dev, n, t
from oracle import paintmind_oracle as O
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline, choice_schedule
from util import load_golden, to_torch_sd

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------------------
# operator level
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temp", R.TEMPS)
@pytest.mark.parametrize("B,N,m", R.CASES)
def test_given_noise_against_the_float64_restatement(B, N, m, temp):
    worst = 0
    for seed in R.SEEDS:
        ids, scores, u = R.inputs(B, N, seed)
        out = n(ops.remask(t(ids), t(scores), m, R.MASK_ID, choice_temperature=temp, noise=t(u)))
        masked = out == R.MASK_ID
        assert np.array_equal(out[~masked], ids[~masked])
        worst = max(worst, R.check_selection(masked, scores, u, temp, m))
    print(f"B={B} N={N} m={m} t={temp}: at most {worst} positions within the margin {R.margin(temp):.3e} of a threshold")


@pytest.mark.parametrize("B,N,m", [(2, 16, 3), (3, 100, 37), (4, 1024, 724), (1, 1500, 1), (2, 4096, 4096)])
def test_zero_temperature_is_the_plain_kernel_with_heavy_ties(B, N, m):
    rng = np.random.default_rng(B * N + m)
    scores = np.round(rng.random((B, N)).astype(np.float32), 2)        # heavy ties on purpose
    scores[:, ::7] = -1e5
    ids = rng.integers(0, 50, (B, N)).astype(np.int64)
    want = ops.remask(t(ids), t(scores), m, R.MASK_ID)
    assert np.array_equal(n(want), O.remask(ids, scores, m, R.MASK_ID))
    u = t(rng.random((B, N)).astype(np.float32))
    # the choice kernel at t = 0 (given noise selects it, and is never read), the Philox form of the entry, and the slots form
    assert torch.equal(ops.remask(t(ids), t(scores), m, R.MASK_ID, choice_temperature=0.0, noise=u), want)
    assert torch.equal(ops.remask(t(ids), t(scores), m, R.MASK_ID, choice_temperature=0.0, seed=3, step=2), want)
    slots = ops.pack_slots([(5, b, 1.0, 3, m, 1) for b in range(B)], dev())
    assert torch.equal(ops.remask_slots(t(ids), t(scores), slots, R.MASK_ID, choice=torch.zeros(B, device=dev())), want)


@pytest.mark.parametrize("B,N,m", [(3, 16, 8), (3, 257, 200), (4, 1024, 724), (2, 4096, 2000)])
def test_philox_mode_properties(B, N, m):
    ids, scores, _ = R.inputs(B, N, 11)
    seed, step, base = 0xFEDCBA9876543210, 3, 2 ** 33 + 5
    x, s = t(ids), t(scores)
    got = ops.remask(x.clone(), s, m, R.MASK_ID, choice_temperature=4.5, seed=seed, step=step, row_base=base)
    # the draw is the token draw's Philox at the column word 0xFFFFFFFF
    u = R.philox_u(seed, step, base, B, N)
    assert torch.equal(got, ops.remask(x.clone(), s, m, R.MASK_ID, choice_temperature=4.5, noise=t(u)))
    # an image alone, with its own row base, reproduces its row
    for b in range(1, B):
        one = ops.remask(x[b:b + 1].clone(), s[b:b + 1].contiguous(), m, R.MASK_ID, choice_temperature=4.5, seed=seed, step=step,
                         row_base=base + b * N)
        assert torch.equal(one[0], got[b]), b
    # the result depends on the step, the seed and the temperature
    plain = ops.remask(x.clone(), s, m, R.MASK_ID)
    other_step = ops.remask(x.clone(), s, m, R.MASK_ID, choice_temperature=4.5, seed=seed, step=step + 1, row_base=base)
    other_seed = ops.remask(x.clone(), s, m, R.MASK_ID, choice_temperature=4.5, seed=seed + 1, step=step, row_base=base)
    if m < (scores[0] >= 0).sum():                                  # (m = every taken position leaves nothing to choose)
        assert not torch.equal(got, plain) and not torch.equal(got, other_step) and not torch.equal(got, other_seed)
    for r in (got, other_step, other_seed):
        assert torch.equal((r == R.MASK_ID).sum(1), torch.full((B,), m, device=dev()))
        assert not bool(((r == R.MASK_ID) & (s < 0)).any())


@pytest.mark.parametrize("N", [16, 1024])
def test_slots_form(N):
    B = 5
    ids, scores, _ = R.inputs(B, N, 21)
    recs = [(0x0123456789ABCDEF, 7, 0.0, 1, 1, 0), (77, 2 ** 33 + 5, 0.8, 8, N // 2, 3), None,
            (0xFEDCBA9876543210, 4096, 1.3, 5, max(N // 3, 1), 17), (5, 1, 0.5, 3, 3, 1)]
    choice = [4.5, 0.0, 2.0, 0.5, 4.5]
    x, s = t(ids), t(scores)
    slots = ops.pack_slots(recs, dev())
    got = ops.remask_slots(x.clone(), s, slots, R.MASK_ID, choice=torch.tensor(choice, device=dev()))
    for b, rec in enumerate(recs):
        if rec is None:
            assert torch.equal(got[b], x[b])                          # idle: untouched
            continue
        seed, k, _, _, nm, step = rec
        one = ops.remask(x[b:b + 1].clone(), s[b:b + 1].contiguous(), nm, R.MASK_ID, choice_temperature=choice[b], seed=seed, step=step,
                         row_base=k * N)
        assert torch.equal(got[b], one[0]), b
        if choice[b] == 0.0:                                          # beside images with 4.5: the plain re-masking
            assert torch.equal(got[b], ops.remask(x[b:b + 1].clone(), s[b:b + 1].contiguous(), nm, R.MASK_ID)[0])


def test_bad_arguments_launch_nothing():
    lib = _lib.load()
    ids = torch.arange(32, dtype=torch.long, device=dev()).reshape(2, 16)
    keep = ids.clone()
    import ctypes as C
    for what, rc in R.bad_argument_calls(lib, C.c_void_p(ids.data_ptr())):
        assert rc == _lib.PMHIP_EINVAL, (what, rc)
    for bad in (-1.0, float("nan"), 1000.5):
        with pytest.raises(ValueError):
            ops.remask(ids, torch.rand(2, 16, device=dev()), 3, 64, choice_temperature=bad)
    torch.cuda.synchronize()
    assert torch.equal(ids, keep)


# ------------------------------------------------------------------------------------------------------------------------------
# model level: the tiny pipeline (16 tokens, 64 classes)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_pipe():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False)
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("text_model") for k in missing.missing_keys)
    return pipe.to(dev()).eval()


@pytest.fixture(params=[torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def pipe(request, tiny_pipe):
    tiny_pipe.set_compute_dtype(request.param)
    yield tiny_pipe
    tiny_pipe.set_compute_dtype(torch.float32)


def _start(pipe, B, seed=0):
    """a partially given start: about a third of the positions hold an id"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((B, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long)
    given = torch.rand(B, pipe.num_tokens, generator=g) < 0.3
    return torch.where(given, torch.randint(0, pipe.mask_token_id, ids.shape, generator=g), ids).to(dev())


def test_sample_equals_the_operator_composition(pipe):
    B, N, V = 3, pipe.num_tokens, pipe.mask_token_id
    ctx = pipe.text_model(["a", "b", "c"]).to(dev())
    ids0 = _start(pipe, B)
    for text in (ctx, None):
        for kw in ({}, {"choice_noise": torch.rand(B, N, generator=torch.Generator().manual_seed(1)).to(dev())}):
            got, _ = pipe.sample(ids0, np.float64(0.5), text=text, topk=3, temperature=0.8, seed=9, step=2, image_base=5,
                                 choice_temperature=2.25, **kw)
            logits = pipe.engine().forward(pipe.ids2tokens(ids0), text).reshape(B * N, V)
            _, merged, score = ops.sample_rows(logits, ids0.reshape(-1), V, 3, 0.8, seed=9, step=2, row_base=5 * N)
            want = ops.remask(merged.reshape(B, N), score.reshape(B, N), 8, V, choice_temperature=2.25, noise=kw.get("choice_noise"),
                              seed=9, step=2, row_base=5 * N)
            assert torch.equal(got, want)
            plain, _ = pipe.sample(ids0, np.float64(0.5), text=text, topk=3, temperature=0.8, seed=9, step=2, image_base=5)
            for zero in (None, 0, 0.0):
                same, _ = pipe.sample(ids0, np.float64(0.5), text=text, topk=3, temperature=0.8, seed=9, step=2, image_base=5,
                                      choice_temperature=zero)
                assert torch.equal(same, plain)


def _loop_of_samples(pipe, context, B, T, temperature, topk, seed, base, ct, ids0=None, **kw):
    temps, nmask = pipe._schedule(T, temperature)
    ctemps = choice_schedule(T, ct)
    ids = pipe._start_ids(B, ids0, dev())
    eng = pipe.engine()
    for step in range(T):
        ids, _, _, _ = eng.sample(None, ids, context, topk, temps[step], nmask[step], seed=seed, step=step, image_base=base, want_img=False,
                                  choice_temperature=ctemps[step] if ctemps else None, **kw)
    return ids


@pytest.mark.parametrize("mode", ["context", "unconditional", "guided", "context_lens", "given_start"])
def test_generate_ids_paths_agree(pipe, mode):
    B, T, ct = 4, 5, 4.5
    assert choice_schedule(T, ct)[-1] == 0.0
    context = None if mode == "unconditional" else pipe.text_model(["a", "b", "c", "d"]).to(dev())
    kw = {}
    if mode == "guided":
        kw["guidance_scale"] = 2.5
    if mode == "context_lens":
        L = context.shape[1]
        kw["context_lens"] = [1, L, min(2, L), min(3, L)]
    ids0 = _start(pipe, B, 3) if mode == "given_start" else None      # None: from the all-mask state (unconditional: the shared step 0)
    flags = [False] * T
    want = _loop_of_samples(pipe, context, B, T, 1.0, 3, 77, 12, ct, ids0=ids0, **kw)
    plain, _ = pipe.generate_ids(context, B, T, 1.0, 3, flags, 77, image_base=12, use_graph=False, streams=1, ids0=ids0, **kw)
    assert not torch.equal(want, plain)
    eager, _ = pipe.generate_ids(context, B, T, 1.0, 3, flags, 77, image_base=12, use_graph=False, streams=1, ids0=ids0,
                                 choice_temperature=ct, **kw)
    assert torch.equal(eager, want)
    for _ in range(3):                                               # eager once, capture, replay
        graph, _ = pipe.generate_ids(context, B, T, 1.0, 3, flags, 77, image_base=12, use_graph=True, streams=1, ids0=ids0,
                                     choice_temperature=ct, **kw)
        assert torch.equal(graph, want)
    # one captured loop serves every schedule: another base value replays it
    other, _ = pipe.generate_ids(context, B, T, 1.0, 3, flags, 77, image_base=12, use_graph=True, streams=1, ids0=ids0,
                                 choice_temperature=1.5, **kw)
    assert torch.equal(other, _loop_of_samples(pipe, context, B, T, 1.0, 3, 77, 12, 1.5, ids0=ids0, **kw))
    if ids0 is None:
        for use_graph in (False, True):
            lanes, _ = pipe.generate_ids(context, B, T, 1.0, 3, flags, 77, image_base=12, use_graph=use_graph, streams=2,
                                         choice_temperature=ct, **kw)
            assert torch.equal(lanes, want)
        # an explicit all-mask start takes the loop without the shared step 0: the same ids
        full, _ = pipe.generate_ids(context, B, T, 1.0, 3, flags, 77, image_base=12, use_graph=True, streams=1,
                                    ids0=pipe._start_ids(B, None, dev()), choice_temperature=ct, **kw)
        assert torch.equal(full, want)
    for zero in (None, 0):
        for use_graph in (False, True):
            same, _ = pipe.generate_ids(context, B, T, 1.0, 3, flags, 77, image_base=12, use_graph=use_graph, streams=1, ids0=ids0,
                                        choice_temperature=zero, **kw)
            assert torch.equal(same, plain)


def test_generate_and_region_loops_take_the_keyword(tiny_pipe):
    pipe = tiny_pipe
    a, ia = pipe.generate(["a", "b"], timesteps=4, topk=3, save_interval=2, seed=5, return_ids=True, choice_temperature=4.5)
    b, ib = pipe.generate(["a", "b"], timesteps=4, topk=3, save_interval=2, seed=5, return_ids=True, choice_temperature=4.5, use_graph=False,
                          streams=1)
    p, ip = pipe.generate(["a", "b"], timesteps=4, topk=3, save_interval=2, seed=5, return_ids=True)
    assert torch.equal(ia, ib) and all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(ia, ip)
    # the region loops: the native loop from the region's start ids equals the per-step composition
    img = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(2)).to(dev()) * 2 - 1
    _, ids, _ = pipe.to_latent(img)
    g = pipe.image_size // pipe.patch_size
    inside = torch.zeros(g, g, dtype=torch.bool, device=dev())
    inside[1:3, 1:3] = True
    coord = (pipe.patch_size, pipe.patch_size, 2 * pipe.patch_size, 2 * pipe.patch_size)
    for fn, keep in ((pipe.inpaint, ~inside), (pipe.outpaint, inside)):
        _, loop = fn(img, coord, timesteps=4, topk=3, temperature=1.0, seed=3, return_ids=True, choice_temperature=4.5)
        start = torch.where(keep.reshape(1, -1), ids, torch.full_like(ids, pipe.mask_token_id))
        _, steps = pipe._region_steps(start, None, 4, 3, 1.0, 3, True, 4.5)
        assert torch.equal(loop, steps)
        _, plain = fn(img, coord, timesteps=4, topk=3, temperature=1.0, seed=3, return_ids=True)
        _, zero = fn(img, coord, timesteps=4, topk=3, temperature=1.0, seed=3, return_ids=True, choice_temperature=0)
        assert torch.equal(plain, zero)


# (T, temperature, topk, seed, image index, choice temperature or None), admitted staggered into 3 slots
PLAN = {0: [(6, 1.0, 5, 101, 3, 4.5), (2, 0.7, 1, 102, 9, None)],
        1: [(4, 1.3, 3, 103, 4, None)],
        3: [(3, 0.9, 2, 105, 5, 2.0)],
        6: [(4, 1.0, 5, 106, 2 ** 33 + 1, None), (5, 0.5, 2, 107, 8, 4.5)],
        11: [(3, 1.0, 4, 108, 6, None)]}


@pytest.mark.parametrize("conditional", [True, False], ids=["conditional", "unconditional"])
def test_session_mixes_requests_with_and_without(pipe, conditional):
    S = 3
    contexts = list(pipe.text_model([f"p{i}" for i in range(7)]).to(dev()))
    refs = {}
    for use_graph in (False, True, True):
        s = pipe.decode_session(slots=S, conditional=conditional, use_graph=use_graph, decode=False)
        eng = pipe.engine()
        calls, inner = [], eng.step_slots

        def spy(*a, **kw):
            calls.append(kw.get("choice"))
            # does an occupied slot bring a non-zero choice temperature to this step?
            expect.append(any(r is not None and bool(r.ctemps) and r.ctemps[r.done] != 0.0 for r in s.occupied))
            return inner(*a, **kw)

        eng.step_slots = spy
        try:
            done, tick, number, expect = [], 0, 0, []
            while tick <= max(PLAN) or not s.idle():
                for req in PLAN.get(tick, []):
                    T, temp, topk, seed, k, ct = req
                    h = s.submit(context=contexts[number] if conditional else None, timesteps=T, temperature=temp, topk=topk, seed=seed,
                                 image_index=k, choice_temperature=ct)
                    h.params, h.ctx_row = req, (contexts[number] if conditional else None)
                    number += 1
                done += s.step()
                tick += 1
        finally:
            del eng.step_slots
        # a step without one goes to the entry, the kernels and the graph of a session that never heard of choice temperatures
        assert len(calls) == len(expect) and [c is not None for c in calls] == expect
        assert any(expect) and not all(expect)
        assert len(done) == number == 7
        for f in done:
            h = f.handle
            T, temp, topk, seed, k, ct = h.params
            key = (h.params, h.slot)
            if key not in refs:
                context = None
                if conditional:
                    context = torch.zeros(S, *h.ctx_row.shape, device=dev())
                    context[h.slot] = h.ctx_row
                refs[key], _ = pipe.generate_ids(context, S, T, temp, topk, [False] * T, seed, image_base=k - h.slot, use_graph=False,
                                                 streams=1, choice_temperature=ct)
            assert torch.equal(f.ids, refs[key][h.slot]), (h.params, h.slot, use_graph)


def test_choice_launch_beside_the_plain_one():
    """the cost of the choice form, reported (a few microseconds of a 120 ms step): B = 64, N = 1024, per-family timing"""
    B, N, m = 64, 1024, 724
    ids, scores, _ = R.inputs(B, N, 1)
    x, s = t(ids), t(scores)
    out = {}
    for name, kw in (("plain", {}), ("choice", {"choice_temperature": 4.5, "seed": 1, "step": 2})):
        for _ in range(3):
            ops.remask(x.clone(), s, m, R.MASK_ID, **kw)
        torch.cuda.synchronize()
        ops.timing_reset()
        ops.timing_enable(True)
        try:
            for _ in range(20):
                ops.remask(x.clone(), s, m, R.MASK_ID, **kw)
            torch.cuda.synchronize()
            out[name] = ops.timing_get("sample")
        finally:
            ops.timing_enable(False)
            ops.timing_reset()
    print("re-masking launch, B=64 N=1024:", {k: f"{1e3 * v[1] / v[0]:.1f} us over {v[0]} launches" for k, v in out.items()})
    assert out["plain"][0] == out["choice"][0] == 20
