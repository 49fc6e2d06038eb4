"""The float64 restatement of the choice form of the re-masking step, and the inputs the operator tests of
tests/test_choice_cpu.py and tests/test_gpu_choice.py share.

keys64 states the contract of include/pmhip.h (pmhip_remask_choice) in float64 from the fp32 score s and the fp32 uniform u:
    t == 0 or s < 0:  s
    otherwise:        -(t * gumbel(u) + log(max(1 - s, 2^-24)))
A kernel that follows the fp32 recipe deviates from it by a few ulp of the largest magnitude the formula can produce:
|log 2^-24| = 16.64 and |gumbel| <= 16.64 (u a multiple of 2^-24, clamped at 1e-20: between -3.83 and 16.64), i.e. 17 * (1 + t).
`margin` is 64 ulp of fp32 at that magnitude; a position further from the threshold key than the margin has its side decided."""
import numpy as np

from oracle import paintmind_oracle as O

# (B, N, num_mask): N = 16 all in-thread; 100, 257, 513 non-powers of two that cross the element-per-thread classes; 1024 takes
# the three LDS stages; 4096 is the largest class
CASES = [(3, 16, 8), (2, 100, 37), (3, 257, 200), (2, 513, 100), (4, 1024, 724), (2, 1024, 1), (1, 4096, 2000)]
TEMPS = [0.5, 4.5]
SEEDS = [1, 2, 3, 4, 5, 6]
GIVEN = np.float32(-1e5)
MASK_ID = 8192


def margin(t):
    return 64 * 2.0 ** -23 * 17 * (1 + t)


def inputs(B, N, seed):
    """scores 1 - p with p log-uniform in [1e-9, 1] (some below 2^-24: 1 - p rounds to 1), every 7th position given; u a
    multiple of 2^-24; ids below the mask id"""
    rng = np.random.default_rng(seed)
    p = 10.0 ** rng.uniform(-9.0, 0.0, (B, N))
    scores = (1.0 - p).astype(np.float32)
    scores[:, ::7] = GIVEN
    u = (rng.integers(0, 2 ** 24, (B, N)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    ids = rng.integers(0, 50, (B, N)).astype(np.int64)
    return ids, scores, u


def keys64(scores, u, t):
    s = np.asarray(scores, dtype=np.float32).astype(np.float64)
    if t == 0:
        return s
    g = O.gumbel_from_uniform(np.asarray(u, dtype=np.float32).astype(np.float64))
    conf = np.log(np.maximum(1.0 - s, 2.0 ** -24))
    return np.where(s < 0, s, -(np.float64(np.float32(t)) * g + conf))


def check_selection(masked, scores, u, t, m):
    """masked bool [B,N]: what an implementation re-masked.  Per image, with thr the m-th largest key:
    {key > thr + margin} <= masked <= {key >= thr - margin}, exactly m masked, no given position masked; the inputs qualify only
    when at most 2 positions lie within the margin of thr (asserted too).  -> the largest count of such positions"""
    keys = keys64(scores, u, t)
    mg = margin(t)
    worst = 0
    for b in range(keys.shape[0]):
        thr = np.sort(keys[b])[::-1][m - 1]
        near = int((np.abs(keys[b] - thr) <= mg).sum()) - 1          # the threshold element itself aside
        worst = max(worst, near)
        assert near <= 2, (b, near)
        must, may = keys[b] > thr + mg, keys[b] >= thr - mg
        assert np.all(masked[b][must]), (b, "a position above the threshold was not masked")
        assert not np.any(masked[b][~may]), (b, "a position below the threshold was masked")
        assert int(masked[b].sum()) == m, (b, int(masked[b].sum()), m)
        assert not np.any(masked[b][scores[b] < 0]), (b, "a given position was masked")
    return worst


def philox_u(seed, step, row_base, B, N):
    """the uniforms the kernels draw for rows row_base .. row_base + B*N - 1: the token draw's Philox at the column word 0xFFFFFFFF"""
    rows = np.uint64(row_base) + np.arange(B * N, dtype=np.uint64)
    return O.philox_uniform(seed, step, rows, np.full(B * N, 0xFFFFFFFF, dtype=np.uint64)).reshape(B, N)


def bad_argument_calls(lib, p):
    """[(what, return code)] of choice entries called with arguments they must refuse before anything is launched; p: a pointer
    value that is never dereferenced (the checks come first)"""
    out = []
    for t in (-0.5, float("nan"), float("inf"), 1000.5):
        out.append((f"remask_choice t={t}", lib.pmhip_remask_choice(p, p, 3, 64, 2, 16, t, None, 1, 0, 0, None)))
        out.append((f"pipeline_sample_choice t={t}",
                    lib.pmhip_pipeline_sample_choice(None, None, p, None, 0, 2, None, 3, 1.0, 4, None, 1, 0, 0, None, None, None, 0, 0.0, t, None, None)))
    out.append(("remask_choice null ids", lib.pmhip_remask_choice(None, p, 3, 64, 2, 16, 1.0, None, 1, 0, 0, None)))
    out.append(("remask_choice null scores", lib.pmhip_remask_choice(p, None, 3, 64, 2, 16, 1.0, None, 1, 0, 0, None)))
    out.append(("remask_choice_slots null choice", lib.pmhip_remask_choice_slots(p, p, p, None, 64, 2, 16, None)))
    out.append(("remask_choice_slots null slots", lib.pmhip_remask_choice_slots(p, p, None, p, 64, 2, 16, None)))
    out.append(("remask_choice N too large", lib.pmhip_remask_choice(p, p, 3, 64, 2, 4097, 1.0, None, 1, 0, 0, None)))
    return out
