"""The contract of ``capdec_decode_beam_constrained`` (include/capdec.h) -- lexically constrained beam search (Anderson et
al. 2017) by dynamic beam allocation (Post & Vilar 2018) -- as a CPU definition: ``process_def.beam``'s fp32 torch
arithmetic, op for op, with the selection run over the FULL vocabulary of every row, not over short lists, so that a
comparison against it also checks the argument that the HIP path's lists are enough.

A caption has up to 4 phrases of 1..4 tokens; all must occur in it as contiguous runs.  A hypothesis carries ``(met, cur,
pos)``: the bitmask of the phrases matched, the phrase in progress (-1: none) and how many of its tokens are matched.
``adv(state, t)``: (1) if ``cur`` is set and ``phrase[cur][pos] == t``, ``pos += 1``, and at ``pos == len`` the phrase's bit
is set and ``cur``, ``pos`` are cleared -- nothing else; (2) otherwise ``cur`` and ``pos`` are cleared and (3) the
lowest-index unmet phrase that starts with ``t``, if any, is met (length 1) or becomes ``cur`` with ``pos = 1``.
``bank(state)`` = the lengths of the met phrases + ``pos``.

Per step a live row's logits go through the processors, then ``l[stop] <- -inf`` unless its ``met`` is complete, then the
temperature and the log-softmax; a stopped row keeps its single candidate (token 0, log-prob 0, state unchanged).  ``key =
(scores[row] + lp) / seq_new[row]``.  Per caption every candidate with a finite key belongs to the bank of the state it
leads to; the non-empty banks are passed over repeatedly from the highest to the lowest, each visit taking the bank's
best remaining candidate (larger key, then smaller flat index ``slot * V + token``), until ``beam_size`` are taken; the slots
are filled in the order taken.  Step 0 has one row per caption in the empty state.  No phrases: ``process_def.beam``."""
import numpy as np

import process_def as PD

C, L = 4, 4     # phrases per caption, tokens per phrase
EMPTY = (0, -1, 0)


def pack(phrases_per_caption):
    """[[phrase, ...] per caption], a phrase a list of 1..4 ids -> int32 [N, 4, 4], unused places -1"""
    out = np.full((len(phrases_per_caption), C, L), -1, dtype=np.int32)
    for r, phs in enumerate(phrases_per_caption):
        assert len(phs) <= C
        for c, ph in enumerate(phs):
            assert 1 <= len(ph) <= L
            out[r, c, :len(ph)] = ph
    return out


def plen(ph, c):
    n = 0
    while n < L and ph[c][n] >= 0:
        n += 1
    return n


def count(ph):
    n = 0
    while n < C and ph[n][0] >= 0:
        n += 1
    return n


def full(ph):
    return (1 << count(ph)) - 1


def adv(ph, state, t):
    met, cur, pos = state
    t = int(t)
    if cur >= 0 and int(ph[cur][pos]) == t:
        if pos + 1 == plen(ph, cur):
            return (met | (1 << cur), -1, 0)
        return (met, cur, pos + 1)
    for c in range(count(ph)):
        if not (met >> c) & 1 and int(ph[c][0]) == t:
            if plen(ph, c) == 1:
                return (met | (1 << c), -1, 0)
            return (met, c, 1)
    return (met, -1, 0)


def bank(ph, state):
    met, cur, pos = state
    return sum(plen(ph, c) for c in range(C) if (met >> c) & 1) + pos


def special(ph, state):
    """the tokens whose successor state may differ from (met, none, 0)"""
    met, cur, pos = state
    s = set()
    if cur >= 0:
        s.add(int(ph[cur][pos]))
    for c in range(count(ph)):
        if not (met >> c) & 1:
            s.add(int(ph[c][0]))
    return s


def fold(ph, tokens):
    """the state after the tokens, from the empty state"""
    st = EMPTY
    for t in tokens:
        st = adv(ph, st, t)
    return st


def occurs(phrase, tokens):
    phrase, tokens = [int(t) for t in phrase], [int(t) for t in tokens]
    return any(tokens[i:i + len(phrase)] == phrase for i in range(len(tokens) - len(phrase) + 1))


def final_order(met, sc):
    """the returned order of one caption's slots: phrases met descending, score descending, slot ascending"""
    B = len(sc)
    return sorted(range(B), key=lambda b: (-bin(int(met[b])).count("1"), -float(sc[b]), b))


def select(keys, banks, B):
    """keys fp32 [M] (torch), banks int [M] (numpy) -> (the flat indices taken, in order; the smallest gap between adjacent
    keys among the first taken + 1 ranked candidates of any bank)"""
    import torch
    finite = torch.isfinite(keys).numpy()
    ranked = {}
    for b in sorted(set(banks[finite].tolist()), reverse=True):
        idx = np.nonzero(finite & (banks == b))[0]
        o = torch.sort(keys[torch.from_numpy(idx)], descending=True, stable=True).indices.numpy()       # ties: smaller flat index
        ranked[b] = idx[o[:B + 1]]
    taken, used = [], {b: 0 for b in ranked}
    while len(taken) < B and any(used[b] < len(ranked[b]) for b in ranked):
        for b in ranked:                                           # (descending: the dict's insertion order)
            if len(taken) < B and used[b] < len(ranked[b]) and used[b] < B:
                taken.append(int(ranked[b][used[b]]))
                used[b] += 1
    gap = float("inf")
    for b in ranked:
        k = keys[torch.from_numpy(ranked[b][:used[b] + 1])]
        if k.shape[0] > 1:
            gap = min(gap, float((k[:-1] - k[1:]).min()))
    return taken, gap


def constrained_beam(sd, prefix, p, phrases, beam_size, stop_id, T, temperature=1.0, n_head=12):
    """prefix [N, P, d], phrases int32 [N, 4, 4] -> tokens int32 [N, B, T], seq int32 [N, B], scores / seq fp32 [N, B], met
    int32 [N, B] -- all in the internal slot order -- and margin fp32 [N]: the smallest gap between two ADJACENT keys among
    the first (taken + 1) ranked candidates of any bank at any live step of the caption, step 0 included"""
    import torch
    from oracle import capdec_oracle as O
    N, P, d = prefix.shape
    B = beam_size
    phrases = np.asarray(phrases)
    nl = O._n_layer(sd, "gpt.")
    cache = [None] * nl
    W = sd["gpt.transformer.wte.weight"]
    V = W.shape[0]
    temp = temperature if temperature > 0 else 1.0

    def log_probs(h, hist, states, caps):
        """h [R, d]; per row its history, state and caption -> fp32 log-softmax [R, V] after steps 1-4 and the stop ban"""
        lg = (h @ W.t()).numpy()
        rows = []
        for r in range(lg.shape[0]):
            q = PD.process(lg[r], hist[r], p, (stop_id,))
            if states[r][0] != full(phrases[caps[r]]) and 0 <= stop_id < V:
                q[stop_id] = -np.inf
            rows.append(q)
        return (torch.from_numpy(np.stack(rows)).float() / temp).softmax(-1).log()

    def banks_of(ph, state):
        """bank of adv(state, t) for every t [V], and the successor states of the special tokens"""
        out = np.full(V, bank(ph, (state[0], -1, 0)), dtype=np.int64)
        nxt = {}
        for t in special(ph, state):
            nxt[t] = adv(ph, state, t)
            out[t] = bank(ph, nxt[t])
        return out, nxt

    # ---- step 0: one row per caption, the empty state
    h = O.gpt2_hidden(prefix, sd, n_head, "gpt.", 0, cache)[:, -1]
    logp = log_probs(h, [[]] * N, [EMPTY] * N, list(range(N)))
    margin = torch.full((N,), float("inf"))
    scores = torch.full((N, B), -float("inf"))
    nxt = torch.zeros(N, B, dtype=torch.int64)
    states = [[EMPTY] * B for _ in range(N)]
    for r in range(N):
        bk, succ = banks_of(phrases[r], EMPTY)
        taken, gap = select(logp[r], bk, B)
        margin[r] = min(float(margin[r]), gap)
        for slot, t in enumerate(taken):
            scores[r, slot] = logp[r, t]
            nxt[r, slot] = t
            states[r][slot] = succ.get(t, EMPTY)
    tokens = torch.zeros(N, B, T, dtype=torch.int64)
    tokens[:, :, 0] = nxt
    seq = torch.ones(N, B)
    stopped = nxt.eq(stop_id)
    for i in range(nl):
        cache[i] = [c.repeat_interleave(B, dim=0) for c in cache[i]]
    alive = ~stopped.all(dim=1)
    # ---- steps 1 .. T-1
    for i in range(1, T):
        if not bool(alive.any()):
            break
        x = W[nxt.reshape(-1)].unsqueeze(1)
        h = O.gpt2_hidden(x, sd, n_head, "gpt.", P + i - 1, cache)[:, -1]
        hist = tokens[:, :, :i].reshape(N * B, i).numpy()
        logp = log_probs(h, hist, [states[r][b] for r in range(N) for b in range(B)],
                         [r for r in range(N) for _ in range(B)]).view(N, B, V)
        logp[stopped] = -float("inf")
        logp[stopped, 0] = 0
        ssum = scores[:, :, None] + logp
        seq_new = seq + (~stopped).float()
        avg = ssum / seq_new[:, :, None]
        src = torch.arange(B)[None, :].repeat(N, 1)
        tok = nxt.clone()
        avg_top = torch.zeros(N, B)
        new_states = [list(s) for s in states]
        for r in range(N):
            if not bool(alive[r]):
                continue
            bk, succ = [], []
            for b in range(B):
                if bool(stopped[r, b]):                             # the single candidate keeps its state
                    bk.append(np.full(V, bank(phrases[r], states[r][b]), dtype=np.int64))
                    succ.append({0: states[r][b]})
                else:
                    k, s = banks_of(phrases[r], states[r][b])
                    bk.append(k)
                    succ.append(s)
            taken, gap = select(avg[r].reshape(-1), np.concatenate(bk), B)
            if gap < float(margin[r]):
                margin[r] = gap
            assert len(taken) == B, (r, i, taken)
            for slot, flat in enumerate(taken):
                b, t = flat // V, flat % V
                src[r, slot], tok[r, slot], avg_top[r, slot] = b, t, avg[r, b, t]
                new_states[r][slot] = succ[b].get(t, states[r][b] if bool(stopped[r, b]) else (states[r][b][0], -1, 0))
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
        states = new_states
        rows = (torch.arange(N)[:, None] * B + src).reshape(-1)
        for l in range(nl):
            cache[l] = [c[rows] for c in cache[l]]
        alive = alive & ~stopped.all(dim=1)
    met = torch.tensor([[states[r][b][0] for b in range(B)] for r in range(N)], dtype=torch.int32)
    return tokens.to(torch.int32), seq.to(torch.int32), scores / seq, met, margin
