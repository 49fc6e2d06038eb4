"""MaskGIT's choice temperature without a GPU: the annealed schedule, the validation at every layer (Python and, through the built
library with pointers that are never dereferenced, the C ABI), the plain-torch branch against the float64 restatement of
tests/choice_ref.py, and None / 0 leaving every existing call as it was."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import choice_ref as R
import paintmind_amd as pm
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline, choice_keys, choice_schedule, num_token_masked
from util import load_golden, to_torch_sd


@pytest.fixture(scope="module")
def tiny():
    p, d = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False).eval()
    pipe.load_state_dict(to_torch_sd(p), strict=False)
    return pipe, d


def test_schedule_values():
    for T in (1, 5, 8, 18):
        got = choice_schedule(T, 4.5)
        want = [float(np.float32(4.5 * (1.0 - (s + 1) / T))) for s in range(T)]
        assert got == want and got[-1] == 0.0 and len(got) == T
        assert all(a > b for a, b in zip(got, got[1:])) and all(np.float32(v) == v for v in got)
    assert choice_schedule(5, 4.5)[0] == float(np.float32(3.6))
    assert choice_schedule(8, None) is None and choice_schedule(8, 0) is None and choice_schedule(8, 0.0) is None
    assert choice_schedule(4, 1000.0)[0] == 750.0


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), 1000.5])
def test_python_validation(tiny, bad):
    pipe, d = tiny
    ids0 = torch.from_numpy(d["ids0"])
    with pytest.raises(ValueError):
        choice_schedule(8, bad)
    with pytest.raises(ValueError):
        ops.choice_t(bad)
    with pytest.raises(ValueError):
        pipe.sample(ids0, 0.5, choice_temperature=bad)
    with pytest.raises(ValueError):
        pipe.generate(["a"], timesteps=2, choice_temperature=bad)
    with pytest.raises(ValueError):
        pipe.inpaint(torch.zeros(1, 3, 32, 32), (0, 0, 16, 16), choice_temperature=bad)
    with pytest.raises(ValueError):
        pipe.decode_session(slots=2, conditional=False).submit(timesteps=3, choice_temperature=bad)


def test_native_entries_refuse_bad_arguments_before_a_launch():
    lib = _lib.load()
    for what, rc in R.bad_argument_calls(lib, C.c_void_p(256)):
        assert rc == _lib.PMHIP_EINVAL, (what, rc, lib.pmhip_last_error())
    # the largest valid value passes the choice check and is refused by the next one (null ids)
    assert lib.pmhip_remask_choice(None, None, 3, 64, 2, 16, 1000.0, None, 1, 0, 0, None) == _lib.PMHIP_EINVAL
    assert b"null" in lib.pmhip_last_error()


def test_keywords_exist_with_neutral_defaults():
    want = {(ops.remask, "choice_temperature"): 0.0, (ops.remask, "noise"): None, (ops.remask, "seed"): 0, (ops.remask, "step"): 0,
            (ops.remask, "row_base"): 0, (ops.remask_slots, "choice"): None, (Pipeline.sample, "choice_temperature"): None,
            (Pipeline.sample, "choice_noise"): None, (Pipeline.generate, "choice_temperature"): None,
            (Pipeline.generate_ids, "choice_temperature"): None, (Pipeline.inpaint, "choice_temperature"): None,
            (Pipeline.outpaint, "choice_temperature"): None}
    for (fn, name), default in want.items():
        assert inspect.signature(fn).parameters[name].default == default, (fn.__name__, name)
    from paintmind_amd.serve import DecodeSession
    assert inspect.signature(DecodeSession.submit).parameters["choice_temperature"].default is None
    from paintmind_amd.engine import S2Engine
    for fn, name in ((S2Engine.sample, "choice_temperature"), (S2Engine.sample, "choice_noise"), (S2Engine.generate, "choice_temps"),
                     (S2Engine.step_slots, "choice")):
        assert inspect.signature(fn).parameters[name].default is None


def _cpu_scores(pipe, ids0, ctx, topk, temperature, noise):
    """the scores Pipeline._sample_cpu re-masks by, restated with the same torch operators (bit-identical on one machine)"""
    logits = pipe.tokens2logits(pipe.ids2tokens(ids0), ctx)
    val, ind = logits.topk(topk, dim=-1)
    filtered = torch.full_like(logits, float("-inf")).scatter_(2, ind, val)
    gumbel = -torch.log((-torch.log(noise.clamp(min=1e-20))).clamp(min=1e-20))
    pred = (filtered / max(temperature, 1e-10) + gumbel).argmax(dim=-1)
    is_mask = ids0 == pipe.mask_token_id
    scores = 1 - logits.softmax(dim=-1).gather(2, pred[..., None])[..., 0]
    return scores.masked_fill(~is_mask, -1e5).detach().numpy(), torch.where(is_mask, pred, ids0)


@pytest.mark.parametrize("t", R.TEMPS)
def test_sample_cpu_against_the_restatement(tiny, t):
    pipe, d = tiny
    ids0, ctx, noise = torch.from_numpy(d["ids0"]), torch.from_numpy(d["context"]), torch.from_numpy(d["s5_ctx_noise"])
    B, N = ids0.shape
    scores, merged = _cpu_scores(pipe, ids0, ctx, 5, 0.7, noise)
    assert (scores < 0).any() and (scores >= 0).any()
    nm = num_token_masked(np.float64(0.5), N)
    for seed in R.SEEDS:
        u = torch.from_numpy(R.inputs(B, N, seed)[2])
        ids, _ = pipe.sample(ids0, np.float64(0.5), text=ctx, topk=5, temperature=0.7, noise=noise, choice_temperature=t, choice_noise=u)
        masked = ids.numpy() == pipe.mask_token_id
        assert np.array_equal(ids.numpy()[~masked], merged.numpy()[~masked])
        m_eff = min(nm, int((scores >= 0).sum(1).min()))
        if m_eff == nm:                                            # (enough taken positions: no given one is needed)
            R.check_selection(masked, scores, u.numpy(), t, nm)
        keys = choice_keys(torch.from_numpy(scores), t, u).numpy().astype(np.float64)
        assert np.max(np.abs(keys - R.keys64(scores, u.numpy(), t))) < R.margin(t)


def test_none_and_zero_leave_the_cpu_branch_unchanged(tiny):
    pipe, d = tiny
    ids0, ctx, noise = torch.from_numpy(d["ids0"]), torch.from_numpy(d["context"]), torch.from_numpy(d["s5_ctx_noise"])
    for kw in ({}, {"choice_temperature": None}, {"choice_temperature": 0}, {"choice_temperature": 0.0, "choice_noise": torch.rand(ids0.shape)}):
        ids5, _ = pipe.sample(ids0, np.float64(0.5), text=ctx, topk=5, temperature=0.7, noise=noise, **kw)
        assert np.array_equal(ids5.numpy(), d["s5_ctx_ids"]), kw
    a, ia = pipe.generate(["a", "b"], timesteps=6, topk=5, save_interval=2, seed=5, return_ids=True)
    for ct in (None, 0):
        b, ib = pipe.generate(["a", "b"], timesteps=6, topk=5, save_interval=2, seed=5, return_ids=True, choice_temperature=ct)
        assert torch.equal(ia, ib) and all(torch.equal(x, y) for x, y in zip(a, b))
    # with a choice temperature the seeded loop is reproducible, differs from the plain one, and ends with as many masked tokens
    c, ic = pipe.generate(["a", "b"], timesteps=6, topk=5, save_interval=2, seed=5, return_ids=True, choice_temperature=4.5)
    c2, ic2 = pipe.generate(["a", "b"], timesteps=6, topk=5, save_interval=2, seed=5, return_ids=True, choice_temperature=4.5)
    assert torch.equal(ic, ic2) and not torch.equal(ic, ia)
    assert torch.equal((ic == pipe.mask_token_id).sum(1), (ia == pipe.mask_token_id).sum(1))


def test_cpu_session_request_equals_generate(tiny):
    pipe, _ = tiny
    s = pipe.decode_session(slots=2, conditional=True)
    h1 = s.submit(text="a", timesteps=5, temperature=1.0, topk=3, seed=11, choice_temperature=4.5)
    h2 = s.submit(text="b", timesteps=3, temperature=0.8, topk=2, seed=12)
    assert h1.ctemps == choice_schedule(5, 4.5) and h2.ctemps is None
    done = {f.handle.number: f for f in s.drain()}
    _, w1 = pipe.generate(["a"], timesteps=5, temperature=1.0, topk=3, seed=11, return_ids=True, choice_temperature=4.5)
    _, w2 = pipe.generate(["b"], timesteps=3, temperature=0.8, topk=2, seed=12, return_ids=True)
    assert torch.equal(done[0].ids, w1[0]) and torch.equal(done[1].ids, w2[0])
