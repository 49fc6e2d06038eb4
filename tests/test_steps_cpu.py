"""The eager decode flows without a GPU: the order of operator and engine calls per step that the docstrings
of ``control_ids``, ``forced_ids``, ``diff_mask`` and ``token_scores`` promise for a pipeline with an engine, and the scalar arguments
that tell the calls apart.  The tiny pipeline stays on the CPU; ``Pipeline._on_cpu`` is stubbed to false, ``Pipeline.engine`` to a
recorder, and the ``ops`` entries the flows reach to recorders that compute their results in plain torch.  Only public methods are
called, so the file holds for any commit that has the flows.  Then the step vocabulary itself: two classes, one set of signatures."""
import inspect

import numpy as np
import pytest
import torch

from paintmind_amd import ops
from paintmind_amd.generate import Pipeline
from test_control_cpu import LENS_EDIT, LENS_SRC, PAIRS, _tiny

B, T, SEED, BASE = PAIRS, 3, 7, 3


class Engine:
    """stands in for S2Engine: logs its forwards, returns seeded logits (and accumulates seeded phrase scores)"""
    device = torch.device("cpu")

    def __init__(self, log, N, V):
        self.log, self.N, self.V, self.gen = log, N, V, torch.Generator().manual_seed(5)

    def forward(self, tokens, context=None, **kw):
        assert set(kw) <= {"keys"}
        self.log.append(("forward", dict(images=tokens.shape[0], context=context is not None, keys=kw.get("keys"))))
        return torch.randn(tokens.shape[0], self.N, self.V, generator=self.gen)

    def forward_control(self, tokens, context, **kw):
        self.log.append(("forward_control", dict(kw, images=tokens.shape[0])))
        logits = torch.randn(tokens.shape[0], self.N, self.V, generator=self.gen)
        if not kw.get("score_layers"):
            return logits
        scores = torch.zeros(tokens.shape[0], self.N) if kw.get("scores") is None else kw["scores"]
        return logits, scores.add_(torch.rand(scores.shape, generator=self.gen))


def _score(logits, pred, ids, mask_id):
    s = 1 - logits.softmax(-1).gather(1, pred[:, None])[:, 0]
    return torch.where(ids == mask_id, pred, ids), s.masked_fill(ids != mask_id, -1e5)


@pytest.fixture()
def flows(monkeypatch):
    """-> (pipe, log): every engine call, operator call and decode appends (name, what tells it apart)"""
    pipe, log = _tiny(), []
    eng = Engine(log, pipe.num_tokens, pipe.mask_token_id)
    monkeypatch.setattr(Pipeline, "_on_cpu", lambda self: False)
    monkeypatch.setattr(Pipeline, "engine", lambda self: eng)
    decode = pipe.vqgan.decode_from_indice
    monkeypatch.setattr(pipe.vqgan, "decode_from_indice", lambda ids: (log.append(("decode", dict(ids=ids.clone()))), decode(ids))[1])

    def embed_rows(table, ids, kpad, out_dtype):
        log.append(("embed_rows", {}))
        return table[ids]

    def guidance_combine(cond, uncond, scale, out=None):
        log.append(("guidance_combine", dict(scale=scale, into_cond=out is cond)))
        return out.copy_(uncond + scale * (cond - uncond))

    def sample_rows(logits, ids, mask_id, topk, temperature, **kw):
        log.append(("sample_rows", dict(kw, rows=logits.shape[0], topk=topk)))
        pred = logits.argmax(-1)
        return (pred,) + _score(logits, pred, ids, mask_id)

    def sample_rows_forced(logits, ids, target, mask_id):
        log.append(("sample_rows_forced", dict(rows=logits.shape[0], target=target.clone())))
        return (target.clone(),) + _score(logits, target, ids, mask_id)

    def remask(ids, scores, num_mask, mask_id, **kw):
        log.append(("remask", dict(kw, num_mask=num_mask, images=ids.shape[0])))
        return ids.scatter_(1, scores.topk(num_mask, dim=-1).indices, mask_id)

    def phrase_region(a, b, g, threshold, grow=0):
        log.append(("phrase_region", dict(same=a is b, threshold=threshold, grow=grow)))
        return ((a >= threshold * a.amax(1, keepdim=True)) | (b >= threshold * b.amax(1, keepdim=True))).to(torch.uint8)

    def blend_tokens(mask, *halves):
        log.append(("blend_tokens", {}))
        for s, t in zip(halves[:3], halves[3:]):
            t.copy_(torch.where(mask.reshape(t.shape) != 0, t, s))
        return halves[3:]

    def logit_divergence(a, b, ids=None, mask_id=None, kind="tv", out=None, accumulate=False):
        log.append(("logit_divergence", dict(kind=kind, accumulate=accumulate, rows=a.shape[0], count=out[1].dtype)))
        d = 0.5 * (a.softmax(-1) - b.softmax(-1)).abs().sum(-1)
        out[0].add_(torch.where(ids == mask_id, d, torch.zeros_like(d)))
        out[1].add_((ids == mask_id).to(out[1].dtype))
        return out

    def token_logprob(logits, target, uncond=None, scale=None, ids=None, mask_id=None, out=None, accumulate=False):
        log.append(("token_logprob", dict(accumulate=accumulate, scale=scale, uncond=uncond is not None, rows=logits.shape[0], count=out[3].dtype)))
        scored = (ids == mask_id) & (target != mask_id)
        out[0].add_(torch.where(scored, -torch.ones(len(ids)), torch.zeros(len(ids))))
        out[3].add_(scored.to(out[3].dtype))
        return out

    for fn in (embed_rows, guidance_combine, sample_rows, sample_rows_forced, remask, phrase_region, blend_tokens, logit_divergence, token_logprob):
        monkeypatch.setattr(ops, fn.__name__, fn)
    return pipe, log


def names(log):
    return [name for name, _ in log]


def per_step(log, steps):
    """the log cut in front of every ``embed_rows``: one list per step (or draw)"""
    starts = [i for i, (name, _) in enumerate(log) if name == "embed_rows"]
    assert len(starts) == steps, names(log)
    return [log[a:b] for a, b in zip(starts, starts[1:] + [len(log)])]


def pair_inputs(pipe):
    rows = pipe.text_model(["a", "b", "c", "d"]).cpu()
    L = rows.shape[1]
    rm = np.tile(np.arange(L, dtype=np.int32), (B, 1))
    w_src, w_edit = np.zeros((B, L), np.float32), np.zeros((B, L), np.float32)
    w_src[:, 3:7], w_edit[:, 5:8] = 1.0, 1.0
    source = torch.randint(0, pipe.mask_token_id, (B, pipe.num_tokens), generator=torch.Generator().manual_seed(6))
    return rows[:B].contiguous(), rows[B:].contiguous(), (rm, np.full((B, L), 0.5, np.float32), np.ones((B, L), np.float32)), (w_src, w_edit), source


def check_tail(pipe, step, calls, nmask):
    """what every draw and re-masking of a step carries: the call's seed, the step, the row base of the first image"""
    N = pipe.num_tokens
    for name, kw in calls:
        if name in ("sample_rows", "remask"):
            assert (kw["seed"], kw["step"], kw["row_base"]) == (SEED, step, BASE * N), (step, name, kw)
        if name == "remask":
            assert (kw["num_mask"], kw["images"]) == (nmask[step], B)
        if name in ("sample_rows", "sample_rows_forced"):
            assert kw["rows"] == B * N


def test_control_ids_runs_its_steps_in_the_promised_order(flows):
    pipe, log = flows
    src, edit, ctl, rows, source = pair_inputs(pipe)
    depth = len(pipe.transformer.layers)
    out = pipe.control_ids(src, edit, LENS_SRC, LENS_EDIT, *ctl, B, T, 1.0, 3, SEED, image_base=BASE, guidance_scale=2.0, blend_rows=rows,
                           source_ids=source, cross_steps=0.5, blend_start=0.4, want_imgs=True)
    assert len(out) == 4 and out[0].shape == (B, pipe.num_tokens) and out[2].shape[0] == B
    nmask = [max(int(np.cos(np.pi / 2 * (s + 1) / T) * pipe.num_tokens), 1) for s in range(T)]
    head = ["embed_rows", "forward_control", "forward", "guidance_combine", "sample_rows_forced", "sample_rows"]
    for step, calls in enumerate(per_step(log, T)):
        blend = ["phrase_region", "blend_tokens"] if step >= 2 else []                       # ceil(0.4 * 3) = 2
        tail = ["remask", "decode", "remask", "decode"] if step == T - 1 else ["remask", "remask"]
        assert names(calls) == head + blend + tail, (step, names(calls))
        kw = dict(calls)
        assert kw["forward_control"]["cross_layers"] == (list(range(depth)) if step < 2 else [])      # ceil(0.5 * 3) = 2
        assert kw["forward_control"]["self_layers"] == [] and kw["forward_control"]["score_layers"] == list(range(depth))
        assert kw["forward_control"]["context_lens"] == LENS_SRC + LENS_EDIT and kw["forward_control"]["images"] == 2 * B
        assert ("row_map" in kw["forward_control"]) == (step < 2)
        assert kw["forward"] == dict(images=2 * B, context=False, keys=None)                 # the pass without a context: no keys
        assert kw["guidance_combine"] == dict(scale=2.0, into_cond=True)
        assert torch.equal(kw["sample_rows_forced"]["target"], source.reshape(-1))
        assert kw["sample_rows"]["topk"] == 3 and kw["sample_rows"]["noise"] is None
        if blend:
            assert kw["phrase_region"] == dict(same=False, threshold=0.3, grow=1)
        check_tail(pipe, step, calls, nmask)
    assert torch.equal(log[-3][1]["ids"], source)                                            # the source image: decoded from its tokens


def test_control_ids_without_tap_scale_and_source(flows):
    pipe, log = flows
    src, edit, ctl, _, _ = pair_inputs(pipe)
    pipe.control_ids(src, edit, LENS_SRC, LENS_EDIT, *ctl, B, T, 1.0, 3, SEED, image_base=BASE, cross_steps=0.5, choice_temperature=4.5)
    nmask = [max(int(np.cos(np.pi / 2 * (s + 1) / T) * pipe.num_tokens), 1) for s in range(T)]
    for step, calls in enumerate(per_step(log, T)):
        assert names(calls) == ["embed_rows", "forward_control" if step < 2 else "forward", "sample_rows", "sample_rows", "remask", "remask"]
        kw = dict(calls)
        if step < 2:
            assert "score_layers" not in kw["forward_control"] and kw["forward_control"]["context_lens"] == LENS_SRC + LENS_EDIT
        else:
            assert kw["forward"]["context"] and kw["forward"]["keys"].lens == LENS_SRC + LENS_EDIT
        assert kw["remask"]["choice_temperature"] == float(np.float32(4.5 * (1.0 - (step + 1) / T)))
        check_tail(pipe, step, calls, nmask)


def test_forced_ids_runs_its_steps_in_the_promised_order(flows):
    pipe, log = flows
    src, _, _, _, source = pair_inputs(pipe)
    ids = pipe.forced_ids(source, src, B, T, SEED, image_base=BASE, guidance_scale=2.0, context_lens=LENS_SRC)
    assert ids.shape == (B, pipe.num_tokens)
    nmask = [max(int(np.cos(np.pi / 2 * (s + 1) / T) * pipe.num_tokens), 1) for s in range(T)]
    for step, calls in enumerate(per_step(log, T)):
        assert names(calls) == ["embed_rows", "forward", "forward", "guidance_combine", "sample_rows_forced", "remask"]
        first, second = calls[1][1], calls[2][1]
        assert first["context"] and first["keys"].lens == LENS_SRC and first["images"] == B
        assert second == dict(images=B, context=False, keys=None)
        assert calls[3][1] == dict(scale=2.0, into_cond=True)
        check_tail(pipe, step, calls, nmask)


def test_diff_mask_runs_its_draws_in_the_promised_order(flows):
    pipe, log = flows
    src, edit, _, _, _ = pair_inputs(pipe)
    S = pipe.image_size
    img = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(4)) * 2 - 1
    mask = pipe.diff_mask(img, src, edit, draws=2, kind="jeffreys", context_lens=LENS_SRC, edit_context_lens=LENS_EDIT)
    assert mask.dtype == torch.bool and mask.shape[0] == B
    draws = per_step(log, 2)
    for j, calls in enumerate(draws):
        assert names(calls)[:3] == ["embed_rows", "forward", "logit_divergence"]
        assert calls[1][1]["images"] == 2 * B and calls[1][1]["context"] and calls[1][1]["keys"].lens == LENS_SRC + LENS_EDIT
        assert calls[2][1] == dict(kind="jeffreys", accumulate=True, rows=B * pipe.num_tokens, count=torch.int32)
    assert names(draws[0]) == names(draws[1])[:3] and names(draws[1])[3:] == ["phrase_region"]
    assert draws[1][3][1] == dict(same=True, threshold=0.5, grow=1)


def test_token_scores_runs_its_draws_in_the_promised_order(flows):
    pipe, log = flows
    src, _, _, _, _ = pair_inputs(pipe)
    S = pipe.image_size
    img = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(4)) * 2 - 1
    maps = pipe.token_scores(img, src, draws=2, guidance_scale=2.0, context_lens=LENS_SRC)
    assert all(m.shape[0] == B and m.dtype == torch.float32 for m in maps) and bool((maps.logp == -1).all())
    for calls in per_step(log, 2):
        assert names(calls) == ["embed_rows", "forward", "forward", "token_logprob"]
        first, second = calls[1][1], calls[2][1]
        assert first["context"] and first["keys"].lens == LENS_SRC and first["images"] == B
        assert not second["context"] and second["keys"] is not None and second["keys"].lens is None      # the keys of no context, not None
        assert calls[3][1] == dict(accumulate=True, scale=2.0, uncond=True, rows=B * pipe.num_tokens, count=torch.int32)


def test_the_two_step_classes_have_one_set_of_signatures():
    from paintmind_amd import steps
    public = lambda cls: {n: inspect.signature(f) for n, f in vars(cls).items() if not n.startswith("_") and callable(f)}
    torch_side, hip_side = public(steps.TorchSteps), public(steps.HipSteps)
    assert torch_side and sorted(torch_side) == sorted(hip_side)
    for name in torch_side:
        assert torch_side[name] == hip_side[name], name
    assert inspect.signature(steps.TorchSteps.__init__) == inspect.signature(steps.HipSteps.__init__)
    assert steps.Draw._fields == ("pred", "merged", "score", "rng")
