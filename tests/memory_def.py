"""The contract of ``capdec_memory_project``, restated in fp64 numpy -- what tests/test_memory_project.py checks the HIP path
against -- the torch fp32 eager statement of the same formula that sets the bounds, and the input builders.

    xn = x / max(||x||, 1e-12)        mn_j = m_j / max(||m_j||, 1e-12)
    w  = softmax_j(<xn, mn_j> / tau)
    v  = sum_j w_j mn_j               out = v / max(||v||, 1e-12)
    lse = logsumexp_j(<xn, mn_j> / tau);  nearest = argmax_j <xn, mn_j>, the lowest index among equals;  max_sim its value

A query row holding a NaN or an inf gets a NaN out row, NaN lse and max_sim and nearest -1; a memory row holding one is an
error.

Bounds.  ``out`` and ``lse``: 8 x the largest absolute error of the eager statement (torch fp32 on the CPU, ``eager``) against
this definition over the whole case -- every row and component of the case's inputs, measured in the test.  8 is the ratio of
the project's bar for an fp32-accurate product (5e-7 of sum |a||b|, tests/test_hip_gemm_plans.py) to one fp32 ulp: a kernel
may sum in another order than torch, it may not be an order of magnitude worse than what a user gets from torch.
``max_sim``: the bound of tests/nearest_def.py for that (row, memory row).  ``nearest`` must EQUAL the definition's; the
builders and seeds are such that the fp64 gap between the two largest similarities of every row exceeds twice that bound,
which ``compare`` asserts -- no row is skipped.
"""
import numpy as np
import torch

import nearest_def as ND

EPS = 1e-12
EAGER_FACTOR = 8.0


def normalize(a):
    return ND.normalize(a)


def project(x, mem, tau):
    """-> dict(out [rows, d], lse, nearest (int64), max_sim, bad (bool), sim [rows, M]) in fp64"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, np.shape(x)[-1])
    mem = np.asarray(mem, dtype=np.float64)
    if not np.isfinite(mem).all():
        raise ValueError("a memory row holds a NaN or an inf")
    bad = ~np.isfinite(x).all(axis=1)
    xn, mn = normalize(np.where(bad[:, None], 0.0, x)), normalize(mem)
    sim = xn @ mn.T
    z = sim / tau
    zmax = z.max(axis=1, keepdims=True)
    e = np.exp(z - zmax)
    tot = e.sum(axis=1, keepdims=True)
    out = normalize((e / tot) @ mn)
    lse = (zmax + np.log(tot))[:, 0]
    nearest = sim.argmax(axis=1)                    # the first of equal maxima
    max_sim = sim.max(axis=1)
    out[bad], lse[bad], max_sim[bad], nearest[bad] = np.nan, np.nan, np.nan, -1
    return {"out": out, "lse": lse, "nearest": nearest, "max_sim": max_sim, "bad": bad, "sim": sim}


def eager(x, mem, tau):
    """the formula as a user writes it in torch, fp32 on the CPU -> (out, lse) as fp64 numpy; NaN / inf rows count as zero rows"""
    x = torch.from_numpy(np.asarray(x, dtype=np.float32).reshape(-1, np.shape(x)[-1]))
    x = torch.where(torch.isfinite(x).all(dim=1, keepdim=True), x, torch.zeros_like(x))
    m = torch.from_numpy(np.asarray(mem, dtype=np.float32))
    xn, mn = torch.nn.functional.normalize(x, dim=-1), torch.nn.functional.normalize(m, dim=-1)
    z = (xn @ mn.T) / tau
    out = torch.nn.functional.normalize(torch.softmax(z, dim=-1) @ mn, dim=-1)
    return out.double().numpy(), torch.logsumexp(z, dim=-1).double().numpy()


def yardstick(x, mem, tau, want=None):
    """-> (bound of out, bound of lse) = EAGER_FACTOR x max |eager - definition| over the rows of x without a NaN or an inf"""
    want = want or project(x, mem, tau)
    ok = ~want["bad"]
    out, lse = eager(x, mem, tau)
    return (EAGER_FACTOR * float(np.abs(out[ok] - want["out"][ok]).max()),
            EAGER_FACTOR * float(np.abs(lse[ok] - want["lse"][ok]).max()))


def sim_bound(x, mem, rows, cols):
    """the bound of tests/nearest_def.py for the similarity of query row rows[i] and memory row cols[i]"""
    xn = normalize(np.asarray(x, dtype=np.float64).reshape(-1, np.shape(x)[-1])[rows])
    mn = normalize(np.asarray(mem, dtype=np.float64)[cols])
    return ND.PRODUCT_BAR * (np.abs(xn) * np.abs(mn)).sum(axis=1) + ND.NORM_BAR * np.abs((xn * mn).sum(axis=1))


def clear_nearest(x, mem, want):
    """asserts that the two largest fp64 similarities of every good row are more than twice the similarity bound apart (or
    that the memory has one row) -> the bound per row"""
    ok = np.flatnonzero(~want["bad"])
    b = sim_bound(x, mem, ok, want["nearest"][ok])
    if want["sim"].shape[1] > 1:
        top2 = np.partition(want["sim"][ok], -2, axis=1)[:, -2:]
        gap = top2[:, 1] - top2[:, 0]
        assert (gap > 2 * b).all(), f"{int((gap <= 2 * b).sum())} rows whose two best similarities are within twice the bound"
    return ok, b


def compare(got_out, got_info, x, mem, tau, what="", bounds=None, want=None):
    """check HIP results (fp32 arrays; got_info = dict lse / nearest / max_sim or None) for the rows of x; ``bounds`` =
    yardstick(...) of the whole case (default: of these rows).  Prints and returns the largest deviation / bound of out, lse
    and max_sim."""
    want = want or project(x, mem, tau)
    b_out, b_lse = bounds or yardstick(x, mem, tau, want)
    bad = want["bad"]
    got_out = np.asarray(got_out, dtype=np.float64).reshape(want["out"].shape)
    assert np.isnan(got_out[bad]).all(), f"{what}: a row holding a NaN or an inf must come back as NaN"
    assert np.isfinite(got_out[~bad]).all(), f"{what}: a NaN or an inf in a good row"
    ok, b_sim = clear_nearest(x, mem, want)
    f_out = float(np.abs(got_out[ok] - want["out"][ok]).max()) / b_out if ok.size else 0.0
    f_lse = f_sim = 0.0
    if got_info is not None:
        lse = np.asarray(got_info["lse"], dtype=np.float64).reshape(-1)
        near = np.asarray(got_info["nearest"]).astype(np.int64).reshape(-1)
        msim = np.asarray(got_info["max_sim"], dtype=np.float64).reshape(-1)
        assert np.isnan(lse[bad]).all() and np.isnan(msim[bad]).all() and (near[bad] == -1).all(), f"{what}: NaN rows"
        assert (near[ok] == want["nearest"][ok]).all(), \
            f"{what}: nearest differs from the fp64 argmax in rows {ok[near[ok] != want['nearest'][ok]][:8]}"
        if ok.size:
            f_lse = float(np.abs(lse[ok] - want["lse"][ok]).max()) / b_lse
            f_sim = float((np.abs(msim[ok] - want["max_sim"][ok]) / b_sim).max())
    print(f"{what}: deviation / bound: out {f_out:.3f} (bound {b_out:.2e}), lse {f_lse:.3f} (bound {b_lse:.2e}), "
          f"max_sim {f_sim:.3f}")
    assert f_out <= 1.0, f"{what}: out misses its bound by {f_out:.2f}x"
    assert f_lse <= 1.0, f"{what}: lse misses its bound by {f_lse:.2f}x"
    assert f_sim <= 1.0, f"{what}: max_sim misses its bound by {f_sim:.2f}x"
    return f_out, f_lse, f_sim


# ------------------------------------------------------------------------------------------------ input builders
def clustered(M, N, d, seed, spread=0.5, scale=None):
    """(mem [M, d], x [N, d]) fp32: memory rows around max(1, M // 8) centres (cosine about 1 / (1 + spread^2) inside a
    cluster), every query around one centre, so that at tau = 0.01 a handful of rows shares the mass.  ``scale`` = (lo, hi):
    every row of both is multiplied by a factor of its own drawn log-uniformly from that range."""
    rng = np.random.default_rng(seed)
    K = max(1, M // 8)
    centres = rng.normal(0.0, 1.0, (K, d))
    mem = centres[np.arange(M) % K] + spread * rng.normal(0.0, 1.0, (M, d))
    x = centres[rng.integers(0, K, N)] + spread * rng.normal(0.0, 1.0, (N, d))
    if scale is not None:
        lo, hi = np.log(scale[0]), np.log(scale[1])
        mem *= np.exp(rng.uniform(lo, hi, (M, 1)))
        x *= np.exp(rng.uniform(lo, hi, (N, 1)))
    else:
        mem, x = normalize(mem), normalize(x)
    return mem.astype(np.float32), x.astype(np.float32)


def underflowing_tail(d=64, tail=262144, seed=3, drop=0.17):
    """(mem [5 + tail, d], x [1, d]): the query e_1; five rows within 0.05 of it; ``tail`` rows at cosine about ``drop`` below
    the top, all leaning towards e_2: at tau = 0.01 each weighs about e^-17 = 4e-8, together about 2e-3 of the mass"""
    rng = np.random.default_rng(seed)
    x = np.zeros((1, d))
    x[0, 0] = 1.0
    top = np.tile(x, (5, 1)) + 0.05 * rng.normal(0.0, 1.0, (5, d)) / np.sqrt(d)
    c = float(normalize(top)[:, 0].max()) - drop
    u = 0.2 * rng.normal(0.0, 1.0, (tail, d)) / np.sqrt(d)
    u[:, 1] += 1.0
    u[:, 0] = 0.0
    u = normalize(u)
    rest = c * x + np.sqrt(1.0 - c * c) * u
    return np.concatenate([top, rest]).astype(np.float32), x.astype(np.float32)
