"""The key-set record of the host request path (``ops.host_keys`` / ``ops.Keys``) without a GPU, at B = 2,
L = 5, N = 4: the record of every way to say which context rows a token attends to against arrays written out here, the three
rules (a context is needed; segments exclude lengths; weights fold the lengths into the neutral segments), a record passed on
instead of the arrays, its lanes, the plain-torch ``CondTransformer`` under ``keys=`` against its four keywords, and the one checking
pass of a ``Pipeline.generate`` with weights and lengths."""
import numpy as np
import pytest
import torch

import paintmind_amd as pm
from paintmind_amd import ops
from paintmind_amd.generate import Pipeline
from paintmind_amd.stage2 import CondTransformer
from util import load_golden, to_torch_sd

B, L, N = 2, 5, 4
LENS = [3, 5]
KS = np.array([[0, 0, 1, -1, -1], [1, 0, 2, 2, 255]], np.int64)              # -1 and 255 both say padding
QM = np.array([[1, 3, 2, 3], [1, 5, 7, 2]], np.int64)
W = np.array([[1.0, 0.5, 2.0, 7.0, 0.0], [1.0, 1.0, 0.25, 1.0, 3.0]], np.float32)
ALL = 0xFFFFFFFF

KS_OUT = np.array([[0, 0, 1, 255, 255], [1, 0, 2, 2, 255]], np.uint8)
QM_OUT = QM.astype(np.uint32)
# (the keywords, the record they give: lens, context_segments, token_segments, weights)
COMBOS = {
    "lens": (dict(context_lens=LENS), (LENS, None, None, None)),
    "segments": (dict(context_segments=KS, token_segments=QM), (None, KS_OUT, QM_OUT, None)),
    "weights": (dict(context_weights=W), (None, np.zeros((B, L), np.uint8), np.full((B, N), ALL, np.uint32), W)),
    "weights+lens": (dict(context_weights=W, context_lens=LENS),
                     (None, np.array([[0, 0, 0, 255, 255], [0, 0, 0, 0, 0]], np.uint8), np.full((B, N), ALL, np.uint32), W)),
    "weights+segments": (dict(context_weights=W, context_segments=KS, token_segments=QM), (None, KS_OUT, QM_OUT, W)),
}
EACH = pytest.mark.parametrize("name", list(COMBOS))


def same(got, want):
    if not isinstance(want, np.ndarray):
        return got == want
    return isinstance(got, np.ndarray) and got.dtype == want.dtype and np.array_equal(got, want)


@EACH
def test_the_record_of_every_combination(name):
    kw, want = COMBOS[name]
    keys = ops.host_keys(B, L, N, **kw)
    assert isinstance(keys, ops.Keys) and tuple(keys.shape) == (B, L, N)
    for got, exp, field in zip((keys.lens, keys.context_segments, keys.token_segments, keys.weights), want, ("lens", "cs", "ts", "w")):
        assert same(got, exp), (name, field, got)
    assert keys.cpu_args() == (keys.lens, keys.context_segments, keys.token_segments, keys.weights)
    # tensors and lists are as good as arrays
    as_tensor = {k: torch.as_tensor(v) for k, v in kw.items()}
    again = ops.host_keys(B, L, N, **as_tensor)
    assert all(same(a, b) for a, b in zip(again.cpu_args(), keys.cpu_args()))


def test_a_weight_behind_the_length_does_not_reach_the_result():
    """weights + lengths: the rows behind an image's length are padding (segment 255) whatever their weight says, so the forward
    does not see it"""
    other = W.copy()
    other[0, 3:] = [0.125, 1000.0]                                        # behind LENS[0] = 3
    a, b = ops.host_keys(B, L, N, LENS, context_weights=W), ops.host_keys(B, L, N, LENS, context_weights=other)
    assert a.lens is None and b.lens is None and np.array_equal(a.context_segments, b.context_segments)
    assert (a.context_segments[0, 3:] == 255).all() and (a.context_segments[0, :3] == 0).all()
    tr, x, ctx = tiny_transformer()
    with torch.no_grad():
        assert torch.equal(tr(x, ctx, keys=a), tr(x, ctx, keys=b))
        assert not torch.equal(tr(x, ctx, keys=a), tr(x, ctx, context_lens=LENS))          # (the weights in front of it do)


def test_the_empty_record_and_the_three_rules():
    empty = ops.host_keys(B, L, N)
    assert empty.cpu_args() == (None, None, None, None) and tuple(empty.shape) == (B, L, N)
    assert ops.host_keys(B, 0, N, has_context=False).cpu_args() == (None, None, None, None)
    with pytest.raises(ValueError, match="exclude each other"):
        ops.host_keys(B, L, N, LENS, KS, QM)
    with pytest.raises(ValueError, match="exclude each other"):
        ops.host_keys(B, L, N, LENS, KS, QM, W)
    for kw in (dict(context_lens=LENS), dict(context_segments=KS, token_segments=QM), dict(context_weights=W),
               dict(context_weights=W, context_lens=LENS)):
        with pytest.raises(ValueError, match="needs? a context"):
            ops.host_keys(B, 0, N, has_context=False, **kw)
        with pytest.raises(ValueError, match="needs? a text condition"):
            ops.host_keys(B, 0, N, has_context=False, missing="a text condition", **kw)
    # the primitive checkers' messages come through
    with pytest.raises(ValueError, match="image 1: length 6"):
        ops.host_keys(B, L, N, [3, 6])
    with pytest.raises(ValueError, match="come together"):
        ops.host_keys(B, L, N, context_segments=KS)
    with pytest.raises(ValueError, match="weight .* must be 0 or in"):
        ops.host_keys(B, L, N, context_weights=W * 2.0 ** 21)


def test_a_record_passes_as_it_is_and_only_for_its_shape(monkeypatch):
    keys = ops.host_keys(B, L, N, context_weights=W, context_lens=LENS)
    for checker in ("host_lens", "host_segments", "host_weights"):
        monkeypatch.setattr(ops, checker, lambda *a, **k: pytest.fail("a checked record was checked again"))
    assert ops.host_keys(B, L, N, keys=keys) is keys
    for shape in ((B + 1, L, N), (B, L + 1, N), (B, L, N + 1)):
        with pytest.raises(ValueError, match="checked for"):
            ops.host_keys(*shape, keys=keys)
    with pytest.raises(ValueError, match="none of them beside it"):
        ops.host_keys(B, L, N, LENS, keys=keys)


@EACH
def test_lane_slices_every_array(name):
    keys = ops.host_keys(B, L, N, **COMBOS[name][0])
    for lo, hi in ((0, 1), (1, 2), (0, 2)):
        lane = keys.lane(lo, hi)
        assert tuple(lane.shape) == (hi - lo, L, N) and lane.neutral == keys.neutral
        for got, whole in zip(lane.cpu_args() + (lane.neutral_lens,), keys.cpu_args() + (keys.neutral_lens,)):
            assert (got is None and whole is None) or same(got, whole[lo:hi])
        # a lane is the record of its images alone
        alone = ops.host_keys(hi - lo, L, N, **{k: v[lo:hi] for k, v in COMBOS[name][0].items()})
        assert all(same(a, b) for a, b in zip(lane, alone))


def tiny_transformer():
    torch.manual_seed(3)
    tr = CondTransformer(in_dim=8, dim=64, len_seq=N, dim_head=32, mlp_dim=128, num_head=2, depth=2, dropout=0.0, context_dim=12,
                         num_classes=16).eval()
    g = torch.Generator().manual_seed(4)
    return tr, torch.randn(B, N, 8, generator=g), torch.randn(B, L, 12, generator=g)


@EACH
@torch.no_grad()
def test_the_forward_under_keys_is_the_forward_under_the_keywords(name):
    tr, x, ctx = tiny_transformer()
    kw = COMBOS[name][0]
    want = tr(x, ctx, **kw)
    assert torch.equal(tr(x, ctx, keys=ops.host_keys(B, L, N, **kw)), want)
    assert not torch.equal(want, tr(x, ctx))                              # (the keys are looked at)
    logits, maps = tr(x, ctx, maps_layers=[1], keys=ops.host_keys(B, L, N, **kw))
    assert torch.equal(logits, want) and torch.equal(maps, tr(x, ctx, maps_layers=[1], **kw)[1])
    with pytest.raises(ValueError, match="none of them beside it"):
        tr(x, ctx, context_lens=LENS, keys=ops.host_keys(B, L, N, **kw))


def test_generate_checks_its_weights_once(monkeypatch):
    """a ``Pipeline.generate`` with weights and lengths brings its arrays to the host and checks them in ONE pass, whatever the
    number of steps and forwards behind it"""
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False)
    pipe.load_state_dict(to_torch_sd(p), strict=False)
    pipe = pipe.eval()
    texts = ["a", "b"]
    Lc = pipe.text_model(texts).shape[1]
    w = np.ones((2, Lc), np.float32)
    w[:, 1] = 2.0
    passes = []
    real = ops.host_weights
    monkeypatch.setattr(ops, "host_weights", lambda *a, **k: passes.append(1) or real(*a, **k))
    kw = dict(timesteps=3, topk=3, save_interval=1, seed=5, return_ids=True, context_weights=w, context_lens=[2, Lc])
    _, ids = pipe.generate(texts, **kw)
    assert len(passes) == 1
    _, guided = pipe.generate(texts, guidance_scale=2.0, **kw)
    assert len(passes) == 2 and not torch.equal(guided, ids)
    monkeypatch.undo()
    plain = pipe.generate(texts, **{**kw, "context_weights": None})[1]
    assert not torch.equal(plain, ids)                                    # (and they are used)
