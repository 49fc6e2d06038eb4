"""pmhip_attention_control: the edited pass of a prompt-to-prompt pair, both dtypes, both score units, dim_head
64 (bf16: the MFMA kernel; f32: the vector-ALU kernel) and 32.  2 pairs, Nq = 80 (one full 64-query group and a tail), (Ls, Lt) in
(1,1) (33,17) (77,77) (129,77) (77,129) (416,231), lengths absent, at 1 / mid and at mid / full, maps with repeats, -1 and entries at
or behind the source length, NaN in every K row and V^T column that may reach nothing.

The inputs, the float64 reference and the element-wise bound are those of tests/control_ref.py; tests/test_control_cpu.py proves on
the CPU that the bound rejects map, blend, gain, length, renormalisation, pair and head faults at exactly these inputs."""
import numpy as np
import pytest
import torch

import abi_frames as A
import attention_probes as P
import control_ref as C
from gpu_common import dev, n, t
from paintmind_amd import _lib, ops

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
MODES = pytest.mark.parametrize("exp2", [True, False], ids=["exp2", "exp"])
DHS = pytest.mark.parametrize("dh", [64, 32])
B, NQ, H = 2, 80, 2
SIGMAS = (2.0, 8.0)
_REF = {}


def gauss(Ls, Lt, dh, sigma, kind, exp2):
    """the case with the kernels' view of it and its float64 reference: computed once, shared by the tests below, never modified"""
    key = (Ls, Lt, dh, sigma, kind, exp2)
    if key not in _REF:
        d = C.case(Ls, Lt, dh, sigma, kind)
        d["ksp"], d["ktp"], d["vtp"] = C.poison(d)
        d["r"] = C.reference(d, exp2)
        for x in list(d.values()) + list(d["r"].values()):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        _REF[key] = d
    return _REF[key]


def operands(d, dtype, rows=slice(None)):
    c = lambda x, dt=None: t(np.array(x[rows]), dt)
    lens = lambda x: None if x is None else c(x)
    return dict(qs=c(d["qs"], dtype), ks=c(d["ksp"], dtype), qt=c(d["qt"], dtype), kt=c(d["ktp"], dtype), vt=c(d["vtp"], dtype),
                row_map=c(d["row_map"]), blend=c(d["blend"]), gain=c(d["gain"]), lens_src=lens(d["lens_s"]), lens_tgt=lens(d["lens_t"]))


def launch(d, dtype, exp2, rows=slice(None), **kw):
    """-> [pairs, H, Nq, dh] float32 / float64-comparable numpy and the raw tensor [pairs * Nq, H * dh]"""
    o = operands(d, dtype, rows)
    o.update(kw)
    Ls, Lt = d["ks"].shape[2], d["kt"].shape[2]
    out = ops.attention_control(o.pop("qs"), o.pop("ks"), o.pop("qt"), o.pop("kt"), o.pop("vt"), Ls, Lt, use_exp2=exp2, **o)
    return out


def heads_view(out, d):
    Bn = out.shape[0] // NQ
    return P.from_out_layout(n(out), Bn, d["qt"].shape[1], NQ, d["qt"].shape[3])


def bound_of(d, dtype, exp2, dh):
    return C.bound(d, d["r"], exp2, mfma=(dtype == BF and dh == 64), bf16_out=(dtype == BF))


@DHS
@DTYPES
@MODES
def test_gauss_family_holds_the_bound(dh, dtype, exp2):
    worst, failures = 0.0, []
    for Ls, Lt in C.SHAPES:
        for kind in C.LENS:
            for sigma in SIGMAS:
                d = gauss(Ls, Lt, dh, sigma, kind, exp2)
                out = heads_view(launch(d, dtype, exp2), d)
                Bd = bound_of(d, dtype, exp2, dh)
                ratio, idx = C.worst(out, d["r"]["ref"], Bd)
                print(f"Ls={Ls} Lt={Lt} {kind} sigma={sigma}: err / B {ratio:.4f}")
                worst = max(worst, ratio)
                if ratio >= 1.0:
                    failures.append(f"Ls={Ls} Lt={Lt} {kind} sigma={sigma}: out {out[idx]!r} ref {d['r']['ref'][idx]!r} bound {Bd[idx]!r} at "
                                    f"(pair, head, query, column) = {idx}: {ratio:.3g} x the bound")
    print(f"control dim_head {dh} {dtype} exp2={exp2}: largest err / B {worst:.4f}")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])


@DHS
@DTYPES
@MODES
def test_exact_family_is_bit_exact(dh, dtype, exp2):
    """heads = 4: every output is a multiple of 1/4 below 32, the same in both units and both dtypes"""
    for Ls, Lt in C.SHAPES:
        for kind in C.LENS:
            d = C.exact_case(Ls, Lt, dh, kind)
            d["ksp"], d["ktp"], d["vtp"] = C.poison(d)
            expect = C.reference(d, exp2)["ref"].astype(np.float32)
            out = heads_view(launch(d, dtype, exp2), d)
            assert np.array_equal(out, expect), (Ls, Lt, kind, np.argwhere(out != expect)[:4].tolist())


@DHS
@DTYPES
@MODES
def test_no_control_is_the_lens_attention_within_the_two_bounds(dh, dtype, exp2):
    """blend == 0, gain == 1: against ops.attention(kv_lens=) on the edited pass, within the SUM of this entry's bound and
    attention_probes' bound of that kernel"""
    kind_of = "bf16" if (dtype == BF and dh == 64) else "f32" if dtype == F32 else "bf16_dh"
    for Ls, Lt in C.SHAPES:
        for kind in C.LENS:
            d0 = gauss(Ls, Lt, dh, 2.0, kind, exp2)
            d = {k: v for k, v in d0.items() if k != "r"}
            d["blend"], d["gain"] = np.zeros_like(d0["blend"]), np.ones_like(d0["gain"])
            r = C.reference(d, exp2)
            o = operands(d, dtype)
            got = heads_view(launch(d, dtype, exp2), d)
            lens_t = o["lens_tgt"] if o["lens_tgt"] is not None else torch.full((B,), Lt, dtype=torch.int32, device=dev())
            plain = heads_view(ops.attention(o["qt"], o["kt"], o["vt"], Lt, use_exp2=exp2, kv_lens=lens_t), d)
            live = (np.arange(Lt)[None, :] < r["nt"][:, None])[:, None, :, None]
            e_t = P.score_error(d["qt"], np.where(live, d["kt"], 0.0), r["st"], exp2)
            Bd = C.bound(d, r, exp2, mfma=(dtype == BF and dh == 64), bf16_out=(dtype == BF)) + P.bound(kind_of, r["ref"], r["A"], e_t, Lt)
            ratio, idx = C.worst(got, plain.astype(np.float64), Bd)
            print(f"Ls={Ls} Lt={Lt} {kind}: |control - lens| / (B + B_lens) {ratio:.4f}")
            assert ratio < 1.0, (Ls, Lt, kind, idx, ratio)
            ratio, idx = C.worst(got, r["ref"], Bd)
            assert ratio < 1.0, (Ls, Lt, kind, idx, ratio)


@DHS
@DTYPES
def test_memory_contract(dh, dtype):
    """a framed output with ldo > heads * dim_head: the gap and the bands around the payload untouched, the payload equal to the
    contiguous launch bit for bit (a result does not depend on the leading dimension)"""
    lib_dtype = _lib.BF16 if dtype == BF else _lib.F32
    for Ls, Lt in ((33, 17), (129, 77)):
        for kind in ("full", "one_mid"):
            d = gauss(Ls, Lt, dh, 2.0, kind, True)
            o = operands(d, dtype)
            plain = launch(d, dtype, True)
            for ld in (None, H * dh + 8):
                frame = A.framed(B * NQ, H * dh, ld=ld, dtype=dtype, device=dev())
                A.call("pmhip_attention_control", lib_dtype, o["qs"], o["ks"], o["qt"], o["kt"], o["vt"], frame, frame.ld, B, H, dh, NQ, Ls,
                       o["ks"].shape[2], Lt, o["kt"].shape[2], 1, o["row_map"], o["blend"], o["gain"], o["lens_src"], o["lens_tgt"])
                torch.cuda.synchronize()
                frame.assert_frame_untouched(f"control Ls={Ls} Lt={Lt} {kind} ldo={frame.ld}")
                assert torch.equal(frame.payload(), plain), (Ls, Lt, kind, frame.ld)
                wide = torch.full((B * NQ, frame.ld), 3.0, device=dev(), dtype=dtype)                    # ... and through the wrapper
                launch(d, dtype, True, out=wide[:, :H * dh])
                assert torch.equal(wide[:, :H * dh], plain) and bool((wide[:, H * dh:] == 3.0).all())


@DHS
@DTYPES
@MODES
def test_repeatable_and_independent_of_the_batch(dh, dtype, exp2):
    for Ls, Lt in ((77, 129), (416, 231)):
        for kind in C.LENS:
            d = gauss(Ls, Lt, dh, 8.0, kind, exp2)
            a, b = launch(d, dtype, exp2), launch(d, dtype, exp2)
            assert torch.equal(a, b), (Ls, Lt, kind, "the same launch twice")
            for pair in range(B):
                alone = launch(d, dtype, exp2, rows=slice(pair, pair + 1))
                assert torch.equal(alone, a[pair * NQ:(pair + 1) * NQ]), (Ls, Lt, kind, pair, "a pair alone")


def test_the_arguments_are_checked():
    z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device=dev())
    q, k, vt = z(2, 2, 16, 64), z(2, 2, 64, 64), z(2, 2, 64, 64)
    rm, bl, gn = z(2, 64, dt=torch.int32), z(2, 64), torch.ones(2, 64, device=dev())
    lens = torch.full((2,), 64, dtype=torch.int32, device=dev())
    assert torch.equal(ops.attention_control(q, k, q, k, vt, 64, 64, rm, bl, gn), z(32, 128))
    assert torch.equal(ops.attention_control(q, k, q, k, vt, 64, 64, rm, bl, gn, lens_src=lens, lens_tgt=lens), z(32, 128))
    for bad in (dict(row_map=rm.float()), dict(blend=bl[:, :63]), dict(gain=gn.double()), dict(lens_src=lens.long()), dict(lens_tgt=lens[:1]),
                dict(out=torch.empty(32, 127, device=dev()))):
        kw = dict(row_map=rm, blend=bl, gain=gn)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.attention_control(q, k, q, k, vt, 64, 64, **kw)
    with pytest.raises(ValueError):
        ops.attention_control(q[:, :1], k, q, k, vt, 64, 64, rm, bl, gn)
    with pytest.raises(_lib.PmhipError):
        ops.attention_control(q.cpu(), k, q, k, vt, 64, 64, rm, bl, gn)                                  # host memory: no CPU fallback
    lib = _lib.load()
    sentinel = 7.0
    out = torch.full((32, 128), sentinel, device=dev())
    qb, kb, vb, ob = q.to(BF), k.to(BF), vt.to(BF), torch.full((32, 136), sentinel, device=dev(), dtype=BF)
    Pt = lambda x: None if x is None else x.data_ptr()

    def rc(dtype=_lib.F32, Qs=q, Ks=k, Qt=q, Kt=k, Vt=vt, O=out, ldo=128, Bn=2, heads=2, dh=64, nq=16, ls=64, lsp=64, lt=64, ltp=64, rm_=rm, bl_=bl,
           gn_=gn):
        return lib.pmhip_attention_control(dtype, Pt(Qs), Pt(Ks), Pt(Qt), Pt(Kt), Pt(Vt), Pt(O), ldo, Bn, heads, dh, nq, ls, lsp, lt, ltp, 0,
                                           Pt(rm_), Pt(bl_), Pt(gn_), None, None, None)

    bf = dict(dtype=_lib.BF16, Qs=qb, Ks=kb, Qt=qb, Kt=kb, Vt=vb, O=ob, ldo=136)
    for bad in (dict(dtype=7), dict(Qs=None), dict(Ks=None), dict(Qt=None), dict(Kt=None), dict(Vt=None), dict(O=None), dict(rm_=None),
                dict(bl_=None), dict(gn_=None), dict(ldo=127), dict(Bn=0), dict(heads=0), dict(heads=65), dict(dh=24), dict(dh=144), dict(nq=0),
                dict(ls=0), dict(lt=0), dict(lsp=63), dict(ltp=63), dict(Bn=40000), dict(bf, ldo=134), dict(bf, lt=61, ltp=62),
                dict(bf, Qt=qb.view(-1)[4:]), dict(bf, O=ob.view(-1)[1:])):
        assert rc(**bad) == _lib.PMHIP_EINVAL, {k: (v if not isinstance(v, torch.Tensor) else tuple(v.shape)) for k, v in bad.items()}
    torch.cuda.synchronize()
    assert bool((out == sentinel).all()) and bool((ob == sentinel).all()), "a refused call wrote to the output"
    assert rc() == _lib.PMHIP_OK and rc(**bf) == _lib.PMHIP_OK
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and bool((ob[:, :128] == 0).all()) and bool((ob[:, 128:] == sentinel).all())
