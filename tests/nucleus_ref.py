"""The float64 restatement of the nucleus (top-p) filter of the token draw (include/pmhip.h,
pmhip_sample_rows_nucleus), shared by tests/test_nucleus_cpu.py and tests/test_gpu_nucleus.py.

The contract, on one row of fp32 logits x: K = the first topk elements of (value desc, column asc); w_i = exp(x_i - max);
Z = the sum of w over K; P = top_p * Z; element i of K is kept iff the mass of the elements of K whose weight is strictly above
w_i is below P.  A plateau of equal weights is therefore kept or dropped whole, the maximum is always kept, and a weight that
underflowed to 0 never is (top_p < 1).  The draw, the merge and the score are O.sample_rows' for the kept set.

The kernels form the sums in fp32, so an element whose mass above lies close to P may fall on either side.  `sets` returns, next
to the exact kept set, MUST (mass above < P - DELTA * Z) and MAY (mass above < P + DELTA * Z): MUST <= kept <= MAY, and an
implementation has to keep all of MUST, nothing outside MAY, and -- the mass above never decreases along the kept order -- a
PREFIX of the band MAY \\ MUST in that order.

DELTA = 1e-4 is derived, not measured: a kernel sum is at most 256 sequential fp32 additions per lane and a 6-level tree,
<= 262 * 2^-24 = 1.6e-5 relative; __expf's argument rounding adds <= |x - max| * log2(e) * 2^-24 to a weight; both act on the
mass above and on Z: under 5e-5 in all, and DELTA doubles that.
"""
import numpy as np

from oracle import paintmind_oracle as O

F = np.float32
DELTA = 1e-4


def sets(logits, topk, top_p, delta=DELTA):
    """logits fp32 [M,V] -> (kept, must, may bool [M,V], order int [M,topk]: K's columns in the kept order)"""
    logits = np.asarray(logits, dtype=F)
    order = O.order_desc_then_index(logits)[:, :topk]
    vals = np.take_along_axis(logits, order, 1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        w = np.exp(vals - vals[:, :1])
    c = np.cumsum(w, axis=1)
    before = c - w                                              # the mass in front of every element of the order
    start = np.ones(w.shape, bool)
    start[:, 1:] = w[:, 1:] != w[:, :-1]
    above = np.maximum.accumulate(np.where(start, before, 0.0), axis=1)      # ... in front of its plateau
    Z = c[:, -1:]
    P = np.float64(F(top_p)) * Z
    out = []
    for bound in (P, P - delta * Z, P + delta * Z):
        m = np.zeros(logits.shape, bool)
        np.put_along_axis(m, order, (above < bound) & (w > 0), 1)
        out.append(m)
    return out[0], out[1], out[2], order


def sample_masked(logits, ids, mask_id, mask, temperature, noise):
    """O.sample_rows with the top-k filter replaced by a given kept mask [M,V] -> (pred, merged, score, pert)"""
    logits = np.asarray(logits, dtype=F)
    filt = np.where(mask, logits, F(-np.inf))
    pert = filt / F(max(temperature, 1e-10)) + O.gumbel_from_uniform(np.asarray(noise, dtype=F))
    pred = pert.argmax(1)
    is_mask = ids == mask_id
    merged = np.where(is_mask, pred, ids)
    probs = O.softmax(logits)
    score = F(1) - np.take_along_axis(probs, pred[:, None], 1)[:, 0]
    score = np.where(is_mask, score, F(-1e5)).astype(F)
    return pred.astype(np.int64), merged.astype(np.int64), score, pert


def sample_rows(logits, ids, mask_id, topk, top_p, temperature, noise):
    """the step under the exact kept set -> (pred, merged, score)"""
    return sample_masked(logits, ids, mask_id, sets(logits, topk, top_p)[0], temperature, noise)[:3]


def allowed(logits, ids, mask_id, topk, top_p, temperature, noise):
    """per row the outcomes an implementation may produce: the winner over MUST plus every prefix (in the kept order) of the band
    MAY \\ MUST -> (list of {pred: (merged, score)} per row, the band's size per row, the smallest relative lead of a winner over
    its runner-up among all those draws)"""
    logits = np.asarray(logits, dtype=F)
    _, must, may, order = sets(logits, topk, top_p)
    M = logits.shape[0]
    band = may & ~must
    pert = logits / F(max(temperature, 1e-10)) + O.gumbel_from_uniform(np.asarray(noise, dtype=F))
    probs = O.softmax(logits)
    is_mask = ids == mask_id
    outcomes, lead = [], np.inf
    for r in range(M):
        base = np.where(must[r], pert[r], F(-np.inf))
        win = int(base.argmax())                                # first maximum: equal values resolve by column
        v1 = base[win]
        base[win] = -np.inf
        v2 = base.max()                                         # the runner-up inside MUST (-inf: MUST is one element)
        cols = np.array([c for c in order[r] if band[r, c]], dtype=np.int64)
        b = pert[r, cols]
        m1 = np.maximum.accumulate(np.concatenate(([v1], b)))  # the best of MUST and the first j band elements
        m2 = np.maximum.accumulate(np.concatenate(([v2], np.minimum(m1[:-1], b))))      # ... and the second best
        decided = np.isfinite(m2) & (m1 != m2)
        if decided.any():
            lead = min(lead, float(((m1 - m2) / np.maximum(np.abs(m1), 1e-30))[decided].min()))
        winners = [win]
        for j in np.flatnonzero(b >= m1[:-1]):                  # a band element that takes the lead when the prefix reaches it
            c = int(cols[j])
            if pert[r, c] > pert[r, winners[-1]] or c < winners[-1]:
                winners.append(c)
        out = {}
        for c in winners:
            out[c] = (c if is_mask[r] else int(ids[r]), F(1) - probs[r, c] if is_mask[r] else F(-1e5))
        outcomes.append(out)
    return outcomes, band.sum(1), lead


def check(got, logits, ids, mask_id, topk, top_p, temperature, noise, what, min_lead=1e-5):
    """got = (pred, merged, score) as numpy arrays.  Every row: pred is one of the allowed outcomes, merged follows, score within
    rtol 1e-4 / atol 1e-6 of that outcome's.  The inputs qualify only when no allowed draw is decided by less than min_lead
    relative in perturbed value -- where device and numpy logarithms may round apart -- (asserted: a property of the inputs, chosen
    on the CPU; exact ties come from equal logits under equal noise and resolve by column on both sides).
    -> the number of rows with a non-empty band"""
    pred, merged, score = got
    outcomes, sizes, lead = allowed(logits, ids, mask_id, topk, top_p, temperature, noise)
    assert lead >= min_lead, (what, "the inputs hold a draw decided by a relative lead of", lead)
    for r in range(len(pred)):
        assert int(pred[r]) in outcomes[r], (what, r, int(pred[r]), sorted(outcomes[r]))
        m, s = outcomes[r][int(pred[r])]
        assert int(merged[r]) == m, (what, r)
        assert np.isclose(score[r], s, rtol=1e-4, atol=1e-6), (what, r, score[r], s)
    return int((sizes > 0).sum())


def torch_restatement(logits, topk, top_p):
    """an independent restatement for rows WITHOUT ties: torch sort + cumsum -> kept bool [M,V] (numpy)"""
    import torch
    x = torch.from_numpy(np.asarray(logits, dtype=F)).double()
    v, i = torch.sort(x, dim=1, descending=True, stable=True)
    v, i = v[:, :topk], i[:, :topk]
    p = torch.softmax(v, dim=1)                                 # w / Z over K
    above = torch.cumsum(p, 1) - p
    keep = above < float(F(top_p))
    return torch.zeros(x.shape, dtype=torch.bool).scatter_(1, i, keep).numpy()


def bad_argument_calls(lib, p):
    """[(what, return code)] of the nucleus entries called with arguments they must refuse before anything is launched; p: a
    pointer value that is never dereferenced (the checks come first)"""
    import ctypes as C
    out = []
    for bad in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        out.append((f"sample_rows_nucleus top_p={bad}",
                    lib.pmhip_sample_rows_nucleus(p, 64, p, 64, 5, bad, 1.0, None, 1, 0, 0, p, p, p, 4, 64, None)))
        out.append((f"pipeline_sample_nucleus top_p={bad}",
                    lib.pmhip_pipeline_sample_nucleus(None, None, p, None, 0, 2, None, 3, 1.0, 4, None, 1, 0, 0, None, None, None, 0, 0.0, 0.0,
                                                      None, bad, None)))
        out.append((f"pipeline_generate_nucleus top_p={bad}",
                    lib.pmhip_pipeline_generate_nucleus(None, None, p, None, 0, 2, None, 2, None, None, None, 3, 1, 0, None, 0, None, None, 0,
                                                        None, 0, 0.0, None, bad)))
    out.append(("sample_rows_nucleus null logits", lib.pmhip_sample_rows_nucleus(None, 64, p, 64, 5, 0.5, 1.0, None, 1, 0, 0, p, p, p, 4, 64, None)))
    out.append(("sample_rows_nucleus topk 0", lib.pmhip_sample_rows_nucleus(p, 64, p, 64, 0, 0.5, 1.0, None, 1, 0, 0, p, p, p, 4, 64, None)))
    out.append(("sample_rows_nucleus topk V+1", lib.pmhip_sample_rows_nucleus(p, 64, p, 64, 65, 0.5, 1.0, None, 1, 0, 0, p, p, p, 4, 64, None)))
    out.append(("sample_rows_nucleus V too large", lib.pmhip_sample_rows_nucleus(p, 16388, p, 16388, 5, 0.5, 1.0, None, 1, 0, 0, p, p, p, 4, 16388, None)))
    out.append(("pipeline_sample_nucleus bad choice", lib.pmhip_pipeline_sample_nucleus(None, None, p, None, 0, 2, None, 3, 1.0, 4, None, 1, 0, 0, None, None,
                                                                                       None, 0, 0.0, -1.0, None, 0.5, None)))
    out.append(("pipeline_sample_nucleus null handle", lib.pmhip_pipeline_sample_nucleus(None, None, p, None, 0, 2, None, 3, 1.0, 4, None, 1, 0, 0, None, None,
                                                                                        None, 0, 0.0, 0.0, None, 0.5, None)))
    return out
