"""vq.hip held to the quantiser probes (tests/vq_probes.py; tests/test_vq_probes_cpu.py shows what each family rejects).

Every case compares, bit for bit: en and sq of pmhip_vq_prepare with oracle/vq_ref.c; idx with the oracle on every row and, where the
family plants its answer (bitwise copies), with that oracle-free expectation; z_out with zn + (en[idx] - zn) in float32.  The loss is
held to the bound of test_vq_bit_exact_against_c_oracle and must come out with the same bits twice.  All four widths of
pmhip_vq_quantize (E = 8, 16, 32, 64) are launched, with one split (V < 2048) and four, at V = 2047 / 2048 / 2049, with a last
tile of one code (V = 129, 2049) and with fewer codes than a 16-code group (V = 1).
"""
import numpy as np
import pytest
import torch

import vq_probes as P
from abi_frames import call
from gpu_common import dev, n
from gpu_common import t as _t
from oracle import vq_ref
from paintmind_amd import _lib, ops

pytestmark = pytest.mark.gpu

BETA = 0.25
_CACHE = {}


def t(a):
    return _t(np.array(a))                                    # the cached arrays are read-only: hand torch a copy


def _case(case):
    """family and oracle of one case: computed once, never modified"""
    if case not in _CACHE:
        fam = P.build(case)
        en, sq = vq_ref.prepare(fam["cb"])
        idx, zn, dmin, gap = vq_ref.quantize(fam["z"], en, sq)
        with np.errstate(all="ignore"):
            zq = en[idx]
            z_out = zn + (zq - zn)
            mean = float(np.mean((zq.astype(np.float64) - zn.astype(np.float64)) ** 2))
        ref = dict(en=en, sq=sq, idx=idx, zn=zn, dmin=dmin, gap=gap, z_out=z_out, mean=mean)
        for x in ref.values():
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        _CACHE[case] = fam, ref
    return _CACHE[case]


def _check(case):
    fam, ref = _case(case)
    V, what = case[2], P.case_id(case)
    en, sq = ops.vq_prepare(t(fam["cb"]))
    P.assert_bits(n(en), ref["en"], f"{what}: en")
    P.assert_bits(n(sq), ref["sq"], f"{what}: sq")
    z = t(fam["z"])
    z_out, idx, loss = ops.vq_quantize(z, en, sq, BETA)
    P.assert_idx(n(idx), ref["idx"], V, ref["gap"], f"{what}: idx vs oracle/vq_ref.c")
    if fam["expect"] is not None:
        P.assert_idx(n(idx), fam["expect"], V, ref["gap"], f"{what}: idx vs the smallest index among the bitwise copies")
    P.assert_bits(n(z_out), ref["z_out"], f"{what}: z_out")
    m = ref["mean"]
    got = float(n(loss)[0])
    assert abs(got - (1.0 + BETA) * m) < 1e-6 * max(1.0, m), (what, got, (1.0 + BETA) * m)
    z_out2, idx2, loss2 = ops.vq_quantize(z, en, sq, BETA)
    P.assert_bits(n(loss2), n(loss), f"{what}: loss of a second run")
    assert torch.equal(idx2, idx), what
    P.assert_bits(n(z_out2), n(z_out), f"{what}: z_out of a second run")


@pytest.mark.parametrize("case", P.GPU_CASES, ids=P.case_id)
def test_vq_probe(case):
    _check(case)


@pytest.mark.parametrize("M", P.RAGGED_M)
def test_vq_near_tie_ragged_rows(M):
    """one row, one short of a wave, a wave, one more; one short of a block and one more"""
    _check(("near_tie", 32, 1000, M))


@pytest.mark.parametrize("null", ["z_out", "loss_out", "both"])
def test_vq_null_outputs_give_the_same_indices(null):
    """include/pmhip.h lets z_out and loss_out be NULL: idx (and the output that is still asked for) as in the full call"""
    case = ("near_tie", 32, 2304, 600)
    fam, ref = _case(case)
    (M, E), V = fam["z"].shape, case[2]
    en, sq = ops.vq_prepare(t(fam["cb"]))
    z = t(fam["z"])
    z_full, idx_full, loss_full = ops.vq_quantize(z, en, sq, BETA)
    P.assert_idx(n(idx_full), ref["idx"], V, ref["gap"], "full call")
    z_out = None if null in ("z_out", "both") else torch.empty_like(z)
    loss = None if null in ("loss_out", "both") else torch.empty(1, device=dev(), dtype=torch.float32)
    idx = torch.full((M,), -1, device=dev(), dtype=torch.int64)
    scratch = torch.empty(_lib.load().pmhip_vq_scratch_bytes(M, V), device=dev(), dtype=torch.uint8)
    call("pmhip_vq_quantize", z, en, sq, BETA, z_out, idx, loss, scratch, M, V, E)
    torch.cuda.synchronize()
    P.assert_idx(n(idx), n(idx_full), V, ref["gap"], f"{null} = NULL vs the full call")
    if z_out is not None:
        P.assert_bits(n(z_out), n(z_full), "z_out with loss_out = NULL")
    if loss is not None:
        P.assert_bits(n(loss), n(loss_full), "loss with z_out = NULL")


@pytest.mark.parametrize("E", [4, 12, 24, 128])
def test_vq_other_widths_are_refused(E):
    cb, z = t(P.iid(8, 32, E)["cb"]), t(P.iid(8, 32, E)["z"])
    en, sq = ops.vq_prepare(cb)                               # preparation has no width limit
    ref_en, ref_sq = vq_ref.prepare(n(cb))
    P.assert_bits(n(en), ref_en, "en")
    P.assert_bits(n(sq), ref_sq, "sq")
    with pytest.raises(_lib.PmhipError, match=rf"embed_dim {E} not in \{{8,16,32,64\}}") as e:
        ops.vq_quantize(z, en, sq, BETA)
    assert e.value.code != 0
