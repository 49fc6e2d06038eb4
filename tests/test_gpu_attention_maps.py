"""pmhip_attention_maps: the head-mean probabilities of one attention launch, in its four forms (plain, a
length per image, a key set per query, key sets and weights), both dtypes, both score units, dim_head 64 (bf16: the MFMA kernel;
f32: the vector-ALU kernel) and 32.  B = 2, Nq = 80 (one full 64-query tile and a partial one), Nkv 1 / 33 / 77 / 129 / 416 with NaN
in the K rows [Nkv, Nkv_pad) and in every K row that takes part in no softmax.

The inputs, the float64 reference and the element-wise bound are those of tests/attnmap_ref.py; tests/test_attention_maps_cpu.py
proves on the CPU that the bound rejects index, head-sum, weight, padding, segment and accumulate faults at exactly these inputs."""
import numpy as np
import pytest
import torch

import abi_frames as A
import attnmap_ref as M
from gpu_common import dev, n, t
from paintmind_amd import _lib, ops

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
MODES = pytest.mark.parametrize("exp2", [True, False], ids=["exp2", "exp"])
DHS = pytest.mark.parametrize("dh", [64, 32])
B, NQ = 2, 80
SIGMAS = (2.0, 8.0)
_REF = {}


def gauss(form, nkv, dh, sigma, exp2):
    """the Gauss case with its float64 reference and bound: computed once, shared by the tests below, never modified"""
    key = (form, nkv, dh, sigma, exp2)
    if key not in _REF:
        d = M.gauss_case(form, nkv, dh, sigma=sigma)
        k = d["k"][:, :, :nkv]
        ref, p, s = M.reference(d["q"], k, d["ok"], d["lay"]["w"], exp2)
        d.update(ref=ref, p=p, s=s, B=M.bound(d["q"], k, ref, p, s, exp2))
        for x in d.values():
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        _REF[key] = d
    return _REF[key]


def form_args(lay, rows=slice(None)):
    kw = {}
    if lay["lens"] is not None:
        kw["kv_lens"] = t(np.array(lay["lens"][rows]))
    if lay["ks"] is not None:
        kw["key_segments"], kw["query_segments"] = t(np.array(lay["ks"][rows])), t(np.array(lay["qm"][rows]).view(np.int32))
    if lay["w"] is not None:
        kw["key_weights"] = t(np.array(lay["w"][rows]))
    return kw


def launch(q, kp, lay, dtype, exp2, nkv, rows=slice(None), **kw):
    """q [B, H, Nq, dh], kp [B, H, Nkv_pad, dh] (numpy) -> the maps tensor f32 [B, Nq, nkv]"""
    return ops.attention_maps(t(np.array(q[rows]), dtype), t(np.array(kp[rows]), dtype), nkv, use_exp2=exp2, **form_args(lay, rows), **kw)


def exact_case(form, nkv, dh):
    lay = M.layout(form, B, NQ, nkv)
    ok = M.allowed(lay, B, NQ, nkv)
    q, k, expect = M.exact_inputs(B, 4, NQ, nkv, dh, ok)
    return q, M.poison(k, ok, -(-nkv // 64) * 64), lay, ok, expect


@DHS
@DTYPES
@MODES
def test_gauss_family_holds_the_bound_in_every_form(dh, dtype, exp2):
    """heads = 3; also: excluded keys exactly 0, every row finite, row sums equal to scale within the summed bound"""
    worst, failures = {}, []
    for form in M.FORMS:
        for nkv in M.NKVS:
            for sigma in SIGMAS:
                d = gauss(form, nkv, dh, sigma, exp2)
                out = n(launch(d["q"], d["k"], d["lay"], dtype, exp2, nkv))
                ratio, idx = M.worst(out, d["ref"], d["B"])
                print(f"{form} Nkv={nkv} sigma={sigma}: err / B {ratio:.4f}")
                worst[form] = max(worst.get(form, 0.0), ratio)
                if ratio > 1.0:
                    failures.append(f"{form} Nkv={nkv} sigma={sigma}: out {out[idx]!r} ref {d['ref'][idx]!r} bound {d['B'][idx]!r} at "
                                    f"(image, query, key) = {idx}: {ratio:.3g} x the bound")
                if not (np.isfinite(out).all() and (out[~d["ok"]] == 0).all() and not np.signbit(out[~d["ok"]]).any()):
                    failures.append(f"{form} Nkv={nkv} sigma={sigma}: an excluded key is not exactly 0.0, or a row is not finite")
                gap = np.abs(out.astype(np.float64).sum(-1) - 1.0) / d["B"].sum(-1)
                if gap.max() > 1.0:
                    failures.append(f"{form} Nkv={nkv} sigma={sigma}: a row sum is {gap.max():.3g} x the summed bound away from 1")
    print(f"maps dim_head {dh} {dtype} exp2={exp2}: largest err / B per form", {k: round(v, 4) for k, v in worst.items()})
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])


@DHS
@DTYPES
@MODES
def test_exact_family_is_bit_exact_in_every_form(dh, dtype, exp2):
    """heads = 4: every map is count / 4"""
    for form in M.FORMS:
        for nkv in M.NKVS:
            q, kp, lay, ok, expect = exact_case(form, nkv, dh)
            out = n(launch(q, kp, lay, dtype, exp2, nkv))
            assert np.array_equal(out, expect), (form, nkv, np.argwhere(out != expect)[:4].tolist())


@DHS
@DTYPES
@MODES
def test_accumulate(dh, dtype, exp2):
    """two launches with scale 1/2, the second accumulating, against the one-launch reference within the bound of the two; on the
    exact family bit for bit; what an excluded key held before an accumulating launch stays"""
    for form in M.FORMS:
        for nkv in (77, 416):
            d = gauss(form, nkv, dh, 2.0, exp2)
            out = launch(d["q"], d["k"], d["lay"], dtype, exp2, nkv, scale=0.5)
            again = launch(d["q"], d["k"], d["lay"], dtype, exp2, nkv, scale=0.5, out=out, accumulate=True)
            assert again.data_ptr() == out.data_ptr()
            got = n(out)
            Bd = 2 * M.bound(d["q"], d["k"][:, :, :nkv], d["ref"], d["p"], d["s"], exp2, scale=0.5, accumulate_out=got)
            ratio, idx = M.worst(got, d["ref"], Bd)
            print(f"{form} Nkv={nkv}: accumulated err / B {ratio:.4f}")
            assert ratio <= 1.0, (form, nkv, idx, ratio)
            q, kp, lay, ok, expect = exact_case(form, nkv, dh)
            out = torch.full((B, NQ, nkv), 7.0, device=dev())
            launch(q, kp, lay, dtype, exp2, nkv, scale=0.5, out=out)
            launch(q, kp, lay, dtype, exp2, nkv, scale=0.5, out=out, accumulate=True)
            assert np.array_equal(n(out), expect), (form, nkv)
            out = torch.full((B, NQ, nkv), 7.0, device=dev())
            launch(q, kp, lay, dtype, exp2, nkv, scale=0.25, out=out, accumulate=True)
            assert np.array_equal(n(out), np.where(ok, 7.0 + 0.25 * expect, 7.0).astype(np.float32)), (form, nkv)


@DHS
@DTYPES
def test_memory_contract(dh, dtype):
    """a framed buffer with ldm > Nkv: guard columns [Nkv, ldm) and the bands around the payload untouched, the payload equal to the
    contiguous launch bit for bit (a result does not depend on the leading dimension)"""
    lib_dtype = _lib.BF16 if dtype == BF else _lib.F32
    for form in M.FORMS:
        for nkv in (33, 129):
            d = gauss(form, nkv, dh, 2.0, True)
            lay = d["lay"]
            kw = form_args(lay)
            bias = ops.key_bias(kw["key_weights"], True) if "key_weights" in kw else None
            q, kp = t(np.array(d["q"]), dtype), t(np.array(d["k"]), dtype)
            for ld in (None, nkv + 1):
                frame = A.framed(B * NQ, nkv, ld=ld, dtype=F32, device=dev())
                A.call("pmhip_attention_maps", lib_dtype, q, kp, frame, frame.ld, B, 3, dh, NQ, nkv, kp.shape[2], 1, kw.get("kv_lens"),
                       kw.get("key_segments"), kw.get("query_segments"), bias, 1.0, 0)
                torch.cuda.synchronize()
                frame.assert_frame_untouched(f"maps {form} Nkv={nkv} ldm={frame.ld}")
                plain = launch(d["q"], d["k"], lay, dtype, True, nkv)
                assert torch.equal(frame.payload().view(B, NQ, nkv), plain), (form, nkv, frame.ld)
                # ... and through the wrapper, a window of a wider buffer
                wide = torch.full((B, NQ, frame.ld), 3.0, device=dev())
                launch(d["q"], d["k"], lay, dtype, True, nkv, out=wide[:, :, :nkv])
                assert torch.equal(wide[:, :, :nkv], plain) and bool((wide[:, :, nkv:] == 3.0).all())


@DHS
@DTYPES
@MODES
def test_repeatable_and_independent_of_the_batch(dh, dtype, exp2):
    for form in M.FORMS:
        for nkv in (77, 416):
            d = gauss(form, nkv, dh, 8.0, exp2)
            a = launch(d["q"], d["k"], d["lay"], dtype, exp2, nkv)
            b = launch(d["q"], d["k"], d["lay"], dtype, exp2, nkv)
            assert torch.equal(a, b), (form, nkv, "the same launch twice")
            for img in range(B):
                alone = launch(d["q"], d["k"], d["lay"], dtype, exp2, nkv, rows=slice(img, img + 1))
                assert torch.equal(alone[0], a[img]), (form, nkv, img, "an image alone")


def test_the_arguments_are_checked():
    q = torch.zeros(2, 2, 16, 64, device=dev())
    k = torch.zeros(2, 2, 64, 64, device=dev())
    ks, qs = torch.zeros(2, 64, dtype=torch.uint8, device=dev()), torch.ones(2, 16, dtype=torch.int32, device=dev())
    w, lens = torch.ones(2, 64, device=dev()), torch.full((2,), 64, dtype=torch.int32, device=dev())
    full = torch.full((2, 16, 64), 1.0 / 64, device=dev())
    assert torch.equal(ops.attention_maps(q, k, 64), full)
    assert torch.equal(ops.attention_maps(q, k, 64, key_segments=ks, query_segments=qs, key_weights=w), full)
    assert torch.equal(ops.attention_maps(q, k, 64, key_weights=w, kv_lens=None), full)
    with pytest.raises(ValueError, match="exclude"):
        ops.attention_maps(q, k, 64, key_weights=w, kv_lens=lens)
    with pytest.raises(ValueError, match="exclude"):
        ops.attention_maps(q, k, 64, key_segments=ks, query_segments=qs, kv_lens=lens)
    with pytest.raises(ValueError, match="come together"):
        ops.attention_maps(q, k, 64, key_segments=ks)
    with pytest.raises(ValueError, match="key_weights"):
        ops.attention_maps(q, k, 64, key_weights=w.double())
    with pytest.raises(ValueError, match="accumulate"):
        ops.attention_maps(q, k, 64, accumulate=True)
    with pytest.raises(ValueError, match="out must be"):
        ops.attention_maps(q, k, 64, out=torch.empty(2, 16, 63, device=dev()))
    with pytest.raises(_lib.PmhipError):
        ops.attention_maps(q.cpu(), k, 64)                                                     # host memory: no CPU fallback
    lib = _lib.load()
    out = torch.empty(2, 16, 64, device=dev())
    P = lambda x: None if x is None else x.data_ptr()

    def rc(dtype=_lib.F32, Q=q, K=k, maps=out, ldm=64, heads=2, dh=64, nkv=64, nkp=64, lens_=None, ks_=None, qs_=None, bias_=None, scale=1.0):
        return lib.pmhip_attention_maps(dtype, P(Q), P(K), P(maps), ldm, 2, heads, dh, 16, nkv, nkp, 0, P(lens_), P(ks_), P(qs_), P(bias_),
                                        scale, 0, None)

    assert rc() == _lib.PMHIP_OK
    assert rc(lens_=lens) == _lib.PMHIP_OK and rc(ks_=ks, qs_=qs) == _lib.PMHIP_OK and rc(ks_=ks, qs_=qs, bias_=w) == _lib.PMHIP_OK
    for bad in (dict(ks_=ks), dict(qs_=qs), dict(bias_=w), dict(lens_=lens, bias_=w), dict(lens_=lens, ks_=ks, qs_=qs),
                dict(lens_=lens, ks_=ks, qs_=qs, bias_=w), dict(ks_=ks, bias_=w), dict(ldm=63), dict(nkp=63), dict(dtype=7), dict(dh=24),
                dict(dh=144), dict(Q=None), dict(K=None), dict(maps=None), dict(nkv=0), dict(heads=0), dict(heads=65),
                dict(scale=float("nan"))):
        assert rc(**bad) == _lib.PMHIP_EINVAL, bad
    torch.cuda.synchronize()
