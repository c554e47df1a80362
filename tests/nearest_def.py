"""The contract of ``capdec_nearest_tokens``, restated in fp64 numpy -- what tests/test_prefix_tokens.py checks the HIP path
against.

    xn = x / max(||x||_2, 1e-12),  tn likewise (torch's nnf.normalize),  sim[r, j] = <xn[r], tn[j]>
    ids[r, 0..k) = the k table rows with the largest sim, descending; EQUAL sims in ascending id order; sims their values.

A query row holding a NaN or an inf gets ids -1 and sims NaN; an all-zero row has every sim 0 (ids 0..k-1); a table row
holding a NaN or an inf is an error.

The bound of a compared entry (r, j), j = the table row:

    |sim_hip - sim_fp64| <= 5e-7 * (|xn[r]| . |tn[j]|) + 1e-6 * |sim_fp64|

-- the project's bar for an fp32-accurate product (tests/test_hip_gemm_plans.py: |err| / sum |a||b| < 5e-7) plus an
allowance for the two fp32 norms.  Ids are compared entry by entry; entry j of a row may be skipped only if its fp64 gap to
a neighbouring entry (j-1 or j+1, the (k+1)-th included) is below twice that bound, never a top-1 entry, and at most 1 % of
all entries.
"""
import numpy as np

EPS = 1e-12
PRODUCT_BAR = 5e-7
NORM_BAR = 1e-6
SKIP_CAP = 0.01


def normalize(a):
    a = np.asarray(a, dtype=np.float64)
    return a / np.maximum(np.sqrt((a * a).sum(axis=-1, keepdims=True)), EPS)


def similarities(x, table):
    """-> (sim fp64 [rows, V], bound fp64 [rows, V], bad bool [rows]); the rows of x holding a NaN or an inf count as zero
    rows in sim and are reported in bad"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, np.shape(x)[-1])
    table = np.asarray(table, dtype=np.float64)
    if not np.isfinite(table).all():
        raise ValueError("a table row holds a NaN or an inf")
    bad = ~np.isfinite(x).all(axis=1)
    xn, tn = normalize(np.where(bad[:, None], 0.0, x)), normalize(table)
    sim = xn @ tn.T
    return sim, PRODUCT_BAR * (np.abs(xn) @ np.abs(tn).T) + NORM_BAR * np.abs(sim), bad


def nearest(x, table, k):
    """-> (ids int64 [rows, k], sims fp64 [rows, k])"""
    sim, _, bad = similarities(x, table)
    assert 1 <= k <= sim.shape[1]
    ids = np.argsort(-sim, axis=1, kind="stable")[:, :k]          # stable: equal sims in ascending id order
    sims = np.take_along_axis(sim, ids, axis=1)
    ids[bad], sims[bad] = -1, np.nan
    return ids, sims


def compare(ids, sims, x, table, what=""):
    """check HIP results ids [rows, k] (and sims, may be None) under the rules above; prints and returns
    (largest |error| / bound over the compared entries, entries skipped, entries)"""
    ids = np.asarray(ids).astype(np.int64)
    rows, k = ids.shape
    sim, bound, bad = similarities(x, table)
    V = sim.shape[1]
    assert sim.shape[0] == rows and k <= V
    order = np.argsort(-sim, axis=1, kind="stable")[:, :min(k + 1, V)]
    sorted_sim = np.take_along_axis(sim, order, axis=1)
    want = order[:, :k]
    assert (ids[bad] == -1).all(), f"{what}: a row holding a NaN or an inf must get ids -1"
    if sims is not None:
        assert np.isnan(np.asarray(sims)[bad]).all(), f"{what}: a row holding a NaN or an inf must get NaN sims"
    ok = ~bad
    assert ((ids[ok] >= 0) & (ids[ok] < V)).all(), f"{what}: an id outside the table"
    b = np.take_along_axis(bound, want, axis=1)
    same = ids == want
    gap = np.full((rows, k), np.inf)
    gap[:, 1:] = np.minimum(gap[:, 1:], np.abs(sorted_sim[:, :k - 1] - sorted_sim[:, 1:k]))
    nxt = sorted_sim.shape[1] - 1                                     # (k when there is a (k+1)-th entry, else k - 1)
    gap[:, :nxt] = np.minimum(gap[:, :nxt], np.abs(sorted_sim[:, :nxt] - sorted_sim[:, 1:nxt + 1]))
    skip = ok[:, None] & ~same
    assert (gap[skip] < 2 * b[skip]).all(), \
        f"{what}: {int((gap[skip] >= 2 * b[skip]).sum())} ids differ where the fp64 gap is not below twice the bound"
    assert not skip[:, 0].any(), f"{what}: a top-1 entry differs"
    n_skip, n_all = int(skip.sum()), int(ok.sum()) * k
    assert n_skip <= SKIP_CAP * n_all, f"{what}: {n_skip} of {n_all} entries skipped"
    worst = 0.0
    if sims is not None:
        cmp_ = ok[:, None] & same
        err = np.abs(np.asarray(sims, dtype=np.float64) - np.take_along_axis(sim, want, axis=1))
        ratio = np.where(cmp_, err / np.maximum(b, 1e-300), 0.0)
        ratio[cmp_ & (err == 0)] = 0.0
        worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{what}: max |hip - fp64| / bound {worst:.3f}, skipped {n_skip} of {n_all} entries")
    assert worst <= 1.0, f"{what}: a similarity misses its bound by {worst:.2f}x"
    return worst, n_skip, n_all
