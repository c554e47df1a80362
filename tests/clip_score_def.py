"""The contract of capdec_clip_score (include/capdec.h) restated in fp64 numpy, written from the contract and not from the
kernel: a loop over the groups, one candidate at a time.  The tests hold the HIP results to these values; the CPU tests let
them stand for the Engine (DefEngine in test_clip_score.py)."""
import numpy as np

#: HIP vs definition, per column: every sum is fp64, so only the one rounding to fp32 (6e-8 relative) and the order of an
#: fp64 sum remain -- the project's bound for such values (gap_stats_def.REL_MOMENTS / ABS_MOMENTS)
REL, ABS = 2.4e-7, 1e-10
#: two cosines of one group closer than this many bounds could legitimately come out in either order
TIE_BOUNDS = 4.0


def _usable(row) -> bool:
    """no NaN, no inf, not all zero"""
    return bool(np.isfinite(row).all() and (row != 0).any())


def _cos(a, b) -> float:
    return float(np.dot(a, b) / (np.sqrt(np.dot(a, a)) * np.sqrt(np.dot(b, b))))


def rank(cos32) -> np.ndarray:
    """indices of one group's candidates, best first: descending fp32 cosine, NaN last, equal values by ascending index"""
    keys = [(bool(np.isnan(c)), 0.0 if np.isnan(c) else -float(c), j) for j, c in enumerate(cos32)]
    return np.array([k[2] for k in sorted(keys)], np.int64)


def clip_score(cand, img, offsets, ref=None, ref_offsets=None, w=2.5):
    """-> (scores fp64 [rows, 4] = cos, clip_s, ref_sim, refclip_s; order int32 [rows] of absolute row numbers)"""
    cand, img = np.asarray(cand, np.float32).astype(np.float64), np.asarray(img, np.float32).astype(np.float64)
    offsets = np.asarray(offsets).astype(np.int64)
    assert (ref is None) == (ref_offsets is None)
    if ref is not None:
        ref, ref_offsets = np.asarray(ref, np.float32).astype(np.float64), np.asarray(ref_offsets).astype(np.int64)
    rows, groups = cand.shape[0], len(offsets) - 1
    scores = np.full((rows, 4), np.nan)
    order = np.zeros(rows, np.int32)
    w = float(np.float32(w))
    for g in range(groups):
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        v = img[g]
        refs = ref[int(ref_offsets[g]):int(ref_offsets[g + 1])] if ref is not None else np.zeros((0, cand.shape[1]))
        refs_ok = len(refs) > 0 and all(_usable(r) for r in refs)
        with np.errstate(all="ignore"):
            for r in range(lo, hi):
                c = cand[r]
                if not (_usable(c) and _usable(v)):
                    continue
                cos = _cos(c, v)
                clip_s = w * max(cos, 0.0)
                scores[r, 0], scores[r, 1] = cos, clip_s
                if refs_ok:
                    ref_sim = max(0.0, max(_cos(c, rho) for rho in refs))
                    scores[r, 2] = ref_sim
                    scores[r, 3] = 0.0 if clip_s + ref_sim == 0.0 else 2.0 * clip_s * ref_sim / (clip_s + ref_sim)
        order[lo:hi] = lo + rank(scores[lo:hi, 0].astype(np.float32))
    return scores, order


def bound(want) -> np.ndarray:
    return REL * np.abs(want) + ABS


def within(got, want) -> float:
    """largest |got - want| / bound; the NaNs must sit in the same places"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    m = ~np.isnan(want)
    if not m.any():
        return 0.0
    return float((np.abs(got[m] - want[m]) / bound(want[m])).max())


def assert_order_decidable(scores, offsets, cand):
    """the condition on a test's INPUTS under which the order must come out exactly: inside every group any two fp64 cosines
    are more than TIE_BOUNDS bounds apart, or belong to bit-identical candidate rows"""
    cand = np.asarray(cand, np.float32)
    for g in range(len(offsets) - 1):
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        for i in range(lo, hi):
            for j in range(i + 1, hi):
                a, b = scores[i, 0], scores[j, 0]
                if np.isnan(a) or np.isnan(b):
                    continue
                if abs(a - b) > TIE_BOUNDS * max(bound(a), bound(b)):
                    continue
                assert cand[i].tobytes() == cand[j].tobytes(), f"group {g}: rows {i} and {j} are {abs(a - b):.2e} apart"
