"""The logits-processor contract of ``capdec_set_logits_processors`` / ``capdec_set_logit_bias`` (include/capdec.h),
restated in fp64 numpy -- what tests/test_process.py checks the HIP path against.

At step ``i`` a row has raw logits ``l[0..V)`` (before the division by the temperature) and a history ``g = (g_0 ..
g_{i-1})``: the tokens its own hypothesis has generated so far.  In this order:

1. ``theta`` > 0 (1 = off): for every DISTINCT ``j`` in ``g``: ``l[j] <- l[j] / theta`` if ``l[j] > 0`` else ``l[j] * theta``.
2. ``bias`` [V] (None = off): ``l <- l + bias`` (entries finite or ``-inf``).
3. ``m`` (0 = off): if ``i >= m - 1``, for every ``s`` with ``g[s .. s+m-2] == g[i-m+1 .. i-1]``: ``l[g[s+m-1]] <- -inf``.
4. ``min_len`` (0 = off): if ``i < min_len``: ``l[stop] <- -inf`` for every stop id of the call.
5. ``top_k`` (0 = off; sampling only): ``j`` stays iff fewer than ``top_k`` entries are strictly greater than ``l[j]``.

Then ``s = l / temperature`` and the rule of the call (arg-max; log-softmax + the beam bookkeeping; nucleus + draw).
"""
import math

import numpy as np


class Proc:
    """one setting of the processors; ``stops``: the stop ids ``min_len`` bans (the call's stop_id and alt_stop_id)"""

    def __init__(self, theta=1.0, m=0, min_len=0, bias=None, top_k=0):
        self.theta, self.m, self.min_len, self.top_k = float(theta), int(m), int(min_len), int(top_k)
        self.bias = None if bias is None else np.asarray(bias, dtype=np.float64)

    @property
    def scale(self):
        """how much the repetition penalty can magnify an error of a logit"""
        return max(self.theta, 1.0 / self.theta)

    def kw(self):
        """the keywords of the Python entry points (None = off)"""
        return dict(repetition_penalty=self.theta if self.theta != 1.0 else None, no_repeat_ngram_size=self.m or None,
                    min_length=self.min_len or None,
                    logit_bias=None if self.bias is None else self.bias.astype(np.float32))


def banned_ngram(g, m):
    """the tokens step 3 bans after the history g"""
    g = [int(t) for t in g]
    i = len(g)
    if m <= 0 or i < m - 1:
        return []
    tail = g[i - m + 1:] if m > 1 else []
    return [g[s + m - 1] for s in range(0, i - m + 1) if g[s:s + m - 1] == tail]


def process(l, g, p, stops=(), top_k=False):
    """steps 1-4 (and 5 with ``top_k=True``) on one row: l [V] (any float type), g the history -> fp64 [V]"""
    l = np.array(l, dtype=np.float64)
    V = l.shape[0]
    i = len(g)
    if p.theta != 1.0:
        for j in sorted(set(int(t) for t in g)):
            l[j] = l[j] / p.theta if l[j] > 0 else l[j] * p.theta
    if p.bias is not None:
        l = l + p.bias
    for j in banned_ngram(g, p.m):
        l[j] = -np.inf
    if i < p.min_len:
        for s in stops:
            if 0 <= s < V:
                l[s] = -np.inf
    if top_k and p.top_k > 0:
        l = top_k_filter(l, p.top_k)
    return l


def top_k_filter(l, k):
    """j stays iff fewer than k entries are strictly greater than l[j] (ties at the boundary stay)"""
    l = np.asarray(l, dtype=np.float64)
    if k <= 0 or k >= l.shape[0]:
        return l.copy()
    kth = np.sort(l)[-k]
    return np.where(l >= kth, l, -np.inf)


def top2_gap(l):
    """largest minus second largest entry"""
    a = np.partition(l, -2)[-2:]
    return float(a[1] - a[0])


# ---------------------------------------------------------------------------- decode loops on the CPU oracle
def greedy(sd, prefix, p, stop_id, T, alt_stop_id=-1, n_head=12):
    """O.greedy_cached with the processors between the logits and the arg-max: prefix [N, P, d] -> (ids int32 [N, T] zero
    padded, lens int32 [N] including the stop token, gaps fp64 [N, T]: the top-2 gap of the processed logits of every
    emitted token's step, inf elsewhere)"""
    import torch
    from oracle import capdec_oracle as O
    N, P, _ = prefix.shape
    W = sd["gpt.transformer.wte.weight"]
    cache = [None] * O._n_layer(sd, "gpt.")
    ids = np.zeros((N, T), dtype=np.int32)
    lens = np.zeros(N, dtype=np.int32)
    gaps = np.full((N, T), np.inf)
    done = np.zeros(N, dtype=bool)
    h = O.gpt2_hidden(prefix, sd, n_head, "gpt.", 0, cache)[:, -1]
    for i in range(T):
        lg = (h @ W.t()).numpy()
        nxt = np.zeros(N, dtype=np.int64)
        for r in range(N):
            if done[r]:
                continue
            q = process(lg[r], ids[r, :i], p, (stop_id, alt_stop_id))
            nxt[r] = int(np.argmax(q))
            gaps[r, i] = top2_gap(q)
            ids[r, i] = nxt[r]
            lens[r] += 1
            done[r] = nxt[r] in (stop_id, alt_stop_id)
        if done.all() or i == T - 1:
            break
        h = O.gpt2_hidden(W[torch.from_numpy(nxt)].unsqueeze(1), sd, n_head, "gpt.", P + i, cache)[:, -1]
    return ids, lens, gaps


def beam(sd, prefix, p, beam_size, stop_id, T, temperature=1.0, n_head=12, margins=None):
    """O.beam_cached -- the same fp32 arithmetic, op for op -- with the processors applied to every row's logits before
    the division by the temperature; a row's history is its beam's tokens after the previous step's re-ordering.
    -> tokens int32 [N, B, T], seq int32 [N, B], scores fp32 [N, B] in the internal beam order.  ``margins`` (a list)
    receives [N]: the smallest gap between two ADJACENT keys among the best B + 1 candidates over the caption's live steps
    (a swap inside the kept beams changes their order, so every adjacent pair counts, not only the last kept / first
    rejected one)."""
    import torch
    from oracle import capdec_oracle as O
    N, P, d = prefix.shape
    B = beam_size
    nl = O._n_layer(sd, "gpt.")
    cache = [None] * nl
    W = sd["gpt.transformer.wte.weight"]
    V = W.shape[0]
    temp = temperature if temperature > 0 else 1.0

    def processed(h, hist):
        """h [R, d], hist: R histories -> fp32 logits [R, V] after steps 1-4"""
        lg = (h @ W.t()).numpy()
        return torch.from_numpy(np.stack([process(lg[r], hist[r], p, (stop_id,)) for r in range(lg.shape[0])])).float()

    def adjacent_gap(keys):
        t = keys.topk(min(B + 1, keys.shape[-1]), -1).values
        g = t[:, :-1] - t[:, 1:]
        g = torch.where(torch.isnan(g), torch.full_like(g, float("inf")), g)       # (-inf) - (-inf): no decision there
        return g.min(dim=-1).values

    h = O.gpt2_hidden(prefix, sd, n_head, "gpt.", 0, cache)[:, -1]
    logp = (processed(h, [[]] * N) / temp).softmax(-1).log()
    scores, nxt = logp.topk(B, -1)
    margin = adjacent_gap(logp) if margins is not None else torch.full((N,), float("inf"))
    tokens = torch.zeros(N, B, T, dtype=torch.int64)
    tokens[:, :, 0] = nxt
    seq = torch.ones(N, B)
    stopped = nxt.eq(stop_id)
    for i in range(nl):
        cache[i] = [c.repeat_interleave(B, dim=0) for c in cache[i]]
    alive = ~stopped.all(dim=1)
    for i in range(1, T):
        if not bool(alive.any()):
            break
        x = W[nxt.reshape(-1)].unsqueeze(1)
        h = O.gpt2_hidden(x, sd, n_head, "gpt.", P + i - 1, cache)[:, -1]
        hist = tokens[:, :, :i].reshape(N * B, i).numpy()
        logp = (processed(h, hist) / temp).softmax(-1).log().view(N, B, V)
        logp[stopped] = -float("inf")
        logp[stopped, 0] = 0
        ssum = scores[:, :, None] + logp
        seq_new = seq + (~stopped).float()
        avg = ssum / seq_new[:, :, None]
        avg_top, flat = avg.view(N, -1).topk(B, -1)
        if margins is not None:
            gap = adjacent_gap(avg.view(N, -1))
            margin = torch.where(alive & (gap < margin), gap, margin)
        src = flat // V
        tok = flat % V
        seq_sel = torch.gather(seq_new, 1, src)
        tok_hist = torch.gather(tokens, 1, src[:, :, None].expand(-1, -1, T)).clone()
        tok_hist[:, :, i] = tok
        stopped_sel = torch.gather(stopped, 1, src) | tok.eq(stop_id)
        a = alive
        tokens[a] = tok_hist[a]
        seq[a] = seq_sel[a]
        scores[a] = (avg_top * seq_sel)[a]
        stopped[a] = stopped_sel[a]
        nxt = torch.where(a[:, None], tok, nxt)
        rows = (torch.arange(N)[:, None] * B + torch.where(a[:, None], src, torch.arange(B)[None, :])).reshape(-1)
        for l in range(nl):
            cache[l] = [c[rows] for c in cache[l]]
        alive = alive & ~stopped.all(dim=1)
    if margins is not None:
        margins.append(margin)
    return tokens.to(torch.int32), seq.to(torch.int32), scores / seq


# ---------------------------------------------------------------------------- sampling on processed logits
def sample_accepted(l14, p, temperature, top_p, u, eps_l, eps_p, eps_u):
    """l14: a row after steps 1-4 (fp64).  The picks the sampling decode may make when every logit carries an error of up
    to eps_l / 2: the top_k boundary taken at the k-th largest value and eps_l below / above it, and for each of the three
    kept sets sample_def's 9 corners of (top_p, u)"""
    import sample_def as D
    if p.top_k <= 0 or p.top_k >= l14.shape[0]:
        return D.accepted_set(l14, temperature, top_p, u, eps_p, eps_u)
    kth = np.sort(l14)[-p.top_k]
    out = set()
    for keep in (l14 >= kth - eps_l, l14 >= kth, (l14 > kth + eps_l) | (l14 == l14.max())):
        out |= D.accepted_set(np.where(keep, l14, -np.inf), temperature, top_p, u, eps_p, eps_u)
    return out


def logp_of(l14, tok, temperature):
    """log-probability of tok under the temperature-scaled distribution after steps 1-4 (before top_k and top_p)"""
    s = l14 / (temperature if temperature > 0 else 1.0)
    m = s.max()
    return float(s[tok] - (m + math.log(np.exp(s - m).sum())))


def sample_decode(sd, prefix, p, temperature, top_p, u, n_head=12):
    """sample_def.decode with the processors (top_k included) in front of the nucleus: nothing stops -> (ids [N, T], the
    oracle's raw fp32 logits [N, T, V])"""
    import torch
    import sample_def as D
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
            ids[r, i] = D.sample(process(lg[r], ids[r, :i], p, (), top_k=True), temperature, top_p, float(u[r, i]))[0]
        if i + 1 < T:
            h = O.gpt2_hidden(W[torch.from_numpy(ids[:, i])].unsqueeze(1), sd, n_head, "gpt.", P + i, cache)[:, -1]
    return ids, np.stack(logits, axis=1)
