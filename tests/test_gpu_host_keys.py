"""The key-set record at the engine's door (``ops.Keys``) on the tiny pipeline, B = 2: every entry point of
``S2Engine`` that takes the four keywords computes under ``keys=`` what it computes under them, bit for bit, and the lanes of
``Pipeline.generate`` slice the record as they sliced the arrays."""
import numpy as np
import pytest
import torch

import paintmind_amd as pm
from gpu_common import dev
from paintmind_amd import ops
from paintmind_amd.generate import Pipeline
from util import load_golden, to_torch_sd

pytestmark = pytest.mark.gpu

B, L = 2, 5
LENS = [3, 5]
KS = np.array([[0, 0, 1, 255, 255], [1, 0, 2, 2, 255]], np.uint8)
W = np.array([[1.0, 0.5, 2.0, 7.0, 0.0], [1.0, 1.0, 0.25, 1.0, 3.0]], np.float32)


@pytest.fixture(scope="module")
def tiny_pipe():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False)
    pipe.load_state_dict(to_torch_sd(p), strict=False)
    return pipe.to(dev()).eval()


@pytest.fixture(scope="module")
def data(tiny_pipe):
    pipe = tiny_pipe
    rng = np.random.default_rng(23)
    N = pipe.num_tokens
    qm = (1 | (rng.integers(0, 4, (B, N)) << 1)).astype(np.uint32)        # every token sees segment 0, some 1 and 2 as well
    ids = rng.integers(0, pipe.mask_token_id, (B, N)).astype(np.int64)
    ids[rng.random((B, N)) < 0.7] = pipe.mask_token_id
    eng = pipe.engine()
    return dict(qm=qm, ids=torch.from_numpy(ids).to(dev()),
                tok=torch.from_numpy(rng.standard_normal((B, N, eng.embed_dim)).astype(np.float32)).to(dev()),
                ctx=torch.from_numpy(rng.standard_normal((B, L, eng.context_dim)).astype(np.float32)).to(dev()))


def combo(name, qm):
    seg = dict(context_segments=KS, token_segments=qm)
    return {"lens": dict(context_lens=LENS), "segments": seg, "weights": dict(context_weights=W),
            "weights+lens": dict(context_weights=W, context_lens=LENS), "weights+segments": dict(context_weights=W, **seg)}[name]


@pytest.mark.parametrize("name", ["lens", "segments", "weights", "weights+lens", "weights+segments"])
def test_every_entry_point_under_keys_is_the_entry_point_under_the_keywords(tiny_pipe, data, name):
    pipe = tiny_pipe
    eng, vq = pipe.engine(), pipe.vqgan.engine()
    kw = combo(name, data["qm"])
    keys = ops.host_keys(B, L, pipe.num_tokens, **kw)
    tok, ctx = data["tok"], data["ctx"]
    want = eng.forward(tok, ctx, **kw)
    assert torch.equal(eng.forward(tok, ctx, keys=keys), want)
    assert not torch.equal(want, eng.forward(tok, ctx))                   # (the keys are looked at)

    def step(**how):
        ids, img, pred, score = eng.sample(vq, data["ids"].clone(), ctx, 4, 0.9, 5, seed=7, step=1, want_aux=True, **how)
        return ids, img, pred, score

    for got, exp in zip(step(keys=keys), step(**kw)):
        assert torch.equal(got, exp)

    def loop(**how):
        ids = torch.full((B, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long, device=dev())
        return eng.generate(vq, ids, ctx, [0.9, 0.45], [8, 1], [False, True], 4, seed=7, use_graph=False, **how)

    (ids_k, imgs_k), (ids_w, imgs_w) = loop(keys=keys), loop(**kw)
    assert torch.equal(ids_k, ids_w) and torch.equal(imgs_k, imgs_w)
    with pytest.raises(ValueError, match="none of them beside it"):
        eng.forward(tok, ctx, context_lens=LENS, keys=keys)
    with pytest.raises(ValueError, match="checked for"):
        eng.forward(tok[:1], ctx[:1], keys=keys)


def test_lanes_slice_the_record(tiny_pipe):
    pipe = tiny_pipe
    texts = ["a", "b"]
    Lc = pipe.text_model(texts).shape[1]
    w = np.ones((2, Lc), np.float32)
    w[0, :3], w[1, 1:4] = [2.0, 0.5, 1.5], [0.25, 3.0, 0.0]             # different rows per image: a lane with the other's would differ
    kw = dict(timesteps=3, topk=4, save_interval=2, seed=5, return_ids=True, use_graph=False, context_weights=w)
    one = []
    for more in (dict(), dict(context_lens=[4, Lc], guidance_scale=2.0)):
        imgs1, ids1 = pipe.generate(texts, streams=1, **kw, **more)
        imgs2, ids2 = pipe.generate(texts, streams=2, **kw, **more)
        assert torch.equal(ids1, ids2) and len(imgs1) == len(imgs2) == 2
        assert all(torch.equal(a, b) for a, b in zip(imgs1, imgs2))
        one.append(ids1)
    swapped = pipe.generate(texts, streams=1, **{**kw, "context_weights": w[::-1].copy()})[1]
    assert not torch.equal(swapped, one[0])
