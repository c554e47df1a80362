"""The nucleus-sampling contract of ``capdec_decode_sample``, restated in fp64 numpy -- what tests/test_sample.py checks
the HIP path against.  For one row of logits ``l``, ``temperature``, ``top_p`` and one uniform ``u`` in [0, 1):

1. ``s = l / (temperature if temperature > 0 else 1)`` (reference gpt2_prefix_eval.py:165), ``p = softmax(s)``.
2. token j is in the nucleus iff it is the arg-max or ``A(j) <= top_p``, ``A(j)`` = the sum of ``p[i]`` over ``p[i] > p[j]``
   (the reference's filter, :166-175: sort descending, drop where the cumulative sum BEFORE the token exceeds top_p,
   never drop the first; exactly equal probabilities are treated alike).  ``A(j) < 1`` for every token, so ``top_p >= 1``
   keeps the whole vocabulary whatever the rounding of the sums.
3. ``q`` = ``p`` restricted to the nucleus, renormalised; the token is the first j in ascending id order whose running
   sum of ``q`` exceeds ``u``; the last nucleus token if rounding leaves the total below ``u``.
"""
import math

import numpy as np


def scaled(logits, temperature):
    return np.asarray(logits, dtype=np.float64) / (temperature if temperature > 0 else 1.0)


def softmax(s):
    e = np.exp(s - s.max())
    return e / e.sum()


def mass_above(p):
    """A(j) for every token: the sum of the probabilities strictly greater than p[j] (largest first)"""
    a = np.sort(p)[::-1]                                   # descending
    before = np.concatenate(([0.0], np.cumsum(a)))         # before[k] = sum of the k largest
    # number of entries strictly greater than p[j]
    k = len(a) - np.searchsorted(a[::-1], p, side="right")
    return before[k]


def nucleus(p, top_p):
    """bool mask of the nucleus of the distribution p"""
    if top_p >= 1.0:
        return np.ones(len(p), dtype=bool)
    return (mass_above(p) <= top_p) | (p == p.max())


def pick(p, mask, u):
    q = np.where(mask, p, 0.0)
    q = q / q.sum()
    hit = np.nonzero((np.cumsum(q) > u) & mask)[0]
    return int(hit[0]) if len(hit) else int(np.nonzero(mask)[0][-1])


def sample(logits, temperature, top_p, u):
    """-> (token, log-probability of the token under the unfiltered temperature-scaled distribution)"""
    s = scaled(logits, temperature)
    p = softmax(s)
    tok = pick(p, nucleus(p, top_p), u)
    m = s.max()
    return tok, float(s[tok] - (m + math.log(np.exp(s - m).sum())))


def accepted_set(logits, temperature, top_p, u, eps_p, eps_u):
    """the picks over the 9 corners (top_p - eps_p, top_p, top_p + eps_p) x (u - eps_u, u, u + eps_u)"""
    p = softmax(scaled(logits, temperature))
    A = mass_above(p)
    top = p == p.max()
    out = set()
    for tp in (top_p - eps_p, top_p, top_p + eps_p):
        mask = np.ones(len(p), dtype=bool) if tp >= 1.0 else ((A <= tp) | top)
        q = np.where(mask, p, 0.0)
        c = np.cumsum(q / q.sum())
        last = int(np.nonzero(mask)[0][-1])
        for uu in (u - eps_u, u, u + eps_u):
            hit = np.searchsorted(c, uu, side="right")      # first index with c > uu (c is non-decreasing)
            while hit < len(c) and not mask[hit]:           # (a token outside the nucleus adds nothing: never the first to exceed)
                hit += 1
            out.add(int(hit) if hit < len(c) else last)
    return out


def decode(sd, prefix, temperature, top_p, u, n_head=12):
    """sampling decode on the CPU oracle (KV-cached, nothing stops): prefix [N, P, d], u [N, T] -> (ids [N, T], logits
    [N, T, V] fp32 the oracle saw at every step)"""
    import torch
    from oracle import capdec_oracle as O
    N, P, _ = prefix.shape
    T = u.shape[1]
    W = sd["gpt.transformer.wte.weight"]
    cache = [None] * O._n_layer(sd, "gpt.")
    ids = np.zeros((N, T), dtype=np.int64)
    logits = []
    h = O.gpt2_hidden(prefix, sd, n_head, "gpt.", 0, cache)[:, -1]
    for i in range(T):
        lg = (h @ W.t()).numpy()
        logits.append(lg)
        for r in range(N):
            ids[r, i] = sample(lg[r], temperature, top_p, float(u[r, i]))[0]
        if i + 1 < T:
            h = O.gpt2_hidden(W[torch.from_numpy(ids[:, i])].unsqueeze(1), sd, n_head, "gpt.", P + i, cache)[:, -1]
    return ids, np.stack(logits, axis=1)


# ---------------------------------------------------------------------------- chi-square quantile (no scipy in the suite)
def _gammainc_upper(a, x):
    """regularised upper incomplete gamma Q(a, x): the series below a + 1, the continued fraction (modified Lentz) above"""
    if x <= 0:
        return 1.0
    lg = math.lgamma(a)
    if x < a + 1.0:
        term = total = 1.0 / a
        n = a
        for _ in range(100000):
            n += 1.0
            term *= x / n
            total += term
            if abs(term) < abs(total) * 1e-16:
                break
        return 1.0 - total * math.exp(-x + a * math.log(x) - lg)
    tiny = 1e-300
    b = x + 1.0 - a
    c = 1.0 / tiny
    d = 1.0 / b
    h = d
    for i in range(1, 100000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return math.exp(-x + a * math.log(x) - lg) * h


def chi2_upper_quantile(dof, tail):
    """x with P(chi2_dof > x) = tail"""
    lo, hi = 0.0, dof + 20.0 * math.sqrt(2.0 * dof) + 200.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if _gammainc_upper(0.5 * dof, 0.5 * mid) > tail:
            lo = mid
        else:
            hi = mid
    return hi
