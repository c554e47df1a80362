"""The contract of ``capdec_decode_beam_groups`` (include/capdec.h) -- diverse (group) beam search, Vijayakumar et al. 2016
-- as a CPU definition: ``process_def.beam``'s fp32 torch arithmetic, op for op, with the group loop around the selection.

Beam slots ``g*Bg .. (g+1)*Bg-1`` (``Bg = B / G``) of a caption form group ``g``.  Within a step the groups are processed in
order.  ``lp`` is the log-softmax of the processed, temperature-scaled logits.  A row of group ``g`` that is not stopped
offers token ``j`` at ``lp[j] - lambda * cnt[j]``, ``cnt[j]`` = how many hypotheses the groups before ``g`` selected AT THIS
STEP with token ``j`` from a source that was not stopped; a stopped row keeps its one candidate (token 0, log-prob 0),
neither penalised nor counted.  ``key = (scores[row] + lp_pen) / seq_new[row]``; the group keeps its best ``Bg`` keys over its
own ``Bg x V`` candidates; ``scores[slot] = key * seq_new[src]`` (the PENALISED values accumulate), ``logp[slot] = logp[src] +
(stopped[src] ? 0 : lp)`` (the unpenalised sum).  Step 0 has one row per caption: group ``g`` takes the best ``Bg`` tokens of
``lp - lambda * cnt``.  One group is ``process_def.beam``."""
import numpy as np

import process_def as PD


def diverse_beam(sd, prefix, p, beam_size, groups, diversity, stop_id, T, temperature=1.0, n_head=12):
    """prefix [N, P, d] -> tokens int32 [N, B, T], seq int32 [N, B], scores / seq fp32 [N, B], logp fp32 [N, B] -- all in
    the internal slot order -- and margin fp32 [N]: the smallest gap between two ADJACENT keys among the best Bg + 1
    candidates of any group at any live step of the caption, step 0 included (a decision closer than the numerical error
    of the keys may legitimately fall the other way, and every later group and step depends on it)."""
    import torch
    from oracle import capdec_oracle as O
    N, P, d = prefix.shape
    B, G = beam_size, groups
    assert 1 <= G <= B and B % G == 0 and diversity >= 0
    Bg = B // G
    lam = torch.tensor(float(diversity), dtype=torch.float32)
    nl = O._n_layer(sd, "gpt.")
    cache = [None] * nl
    W = sd["gpt.transformer.wte.weight"]
    V = W.shape[0]
    temp = temperature if temperature > 0 else 1.0

    def processed(h, hist):
        lg = (h @ W.t()).numpy()
        return torch.from_numpy(np.stack([PD.process(lg[r], hist[r], p, (stop_id,)) for r in range(lg.shape[0])])).float()

    def adjacent_gap(keys):
        t = keys.topk(min(Bg + 1, keys.shape[-1]), -1).values
        g = t[:, :-1] - t[:, 1:]
        g = torch.where(torch.isnan(g), torch.full_like(g, float("inf")), g)       # (-inf) - (-inf): no decision there
        return g.min(dim=-1).values

    # ---- step 0: one row per caption
    h = O.gpt2_hidden(prefix, sd, n_head, "gpt.", 0, cache)[:, -1]
    lp0 = (processed(h, [[]] * N) / temp).softmax(-1).log()
    cnt = torch.zeros(N, V)
    margin = torch.full((N,), float("inf"))
    sc_g, tok_g = [], []
    for g in range(G):
        pen = lp0 - lam * cnt
        v, t = pen.topk(Bg, -1)
        margin = torch.minimum(margin, adjacent_gap(pen))
        cnt.scatter_add_(1, t, torch.ones(N, Bg))
        sc_g.append(v)
        tok_g.append(t)
    scores, nxt = torch.cat(sc_g, 1), torch.cat(tok_g, 1)
    logp_acc = torch.gather(lp0, 1, nxt)
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
        logp = (processed(h, hist) / temp).softmax(-1).log().view(N, B, V)
        logp[stopped] = -float("inf")
        logp[stopped, 0] = 0
        seq_new = seq + (~stopped).float()
        cnt = torch.zeros(N, V)
        top_g, src_g, tok_g, lp_g = [], [], [], []
        for g in range(G):
            sl = slice(g * Bg, (g + 1) * Bg)
            lp = logp[:, sl]
            pen = torch.where(stopped[:, sl, None], lp, lp - lam * cnt[:, None, :])
            ssum = scores[:, sl, None] + pen
            avg = ssum / seq_new[:, sl, None]
            avg_top, flat = avg.reshape(N, -1).topk(Bg, -1)
            gap = adjacent_gap(avg.reshape(N, -1))
            margin = torch.where(alive & (gap < margin), gap, margin)
            src_local = flat // V
            tok = flat % V
            live = ~torch.gather(stopped[:, sl], 1, src_local)
            cnt.scatter_add_(1, tok, live.float())
            top_g.append(avg_top)
            src_g.append(src_local + g * Bg)
            tok_g.append(tok)
            lp_g.append(torch.gather(lp.reshape(N, -1), 1, flat))          # (a stopped source's candidate: 0)
        avg_top, src, tok, lp_w = torch.cat(top_g, 1), torch.cat(src_g, 1), torch.cat(tok_g, 1), torch.cat(lp_g, 1)
        seq_sel = torch.gather(seq_new, 1, src)
        tok_hist = torch.gather(tokens, 1, src[:, :, None].expand(-1, -1, T)).clone()
        tok_hist[:, :, i] = tok
        stopped_sel = torch.gather(stopped, 1, src) | tok.eq(stop_id)
        logp_sel = torch.gather(logp_acc, 1, src) + lp_w
        a = alive
        tokens[a] = tok_hist[a]
        seq[a] = seq_sel[a]
        scores[a] = (avg_top * seq_sel)[a]
        logp_acc[a] = logp_sel[a]
        stopped[a] = stopped_sel[a]
        nxt = torch.where(a[:, None], tok, nxt)
        rows = (torch.arange(N)[:, None] * B + torch.where(a[:, None], src, torch.arange(B)[None, :])).reshape(-1)
        for l in range(nl):
            cache[l] = [c[rows] for c in cache[l]]
        alive = alive & ~stopped.all(dim=1)
    return tokens.to(torch.int32), seq.to(torch.int32), scores / seq, logp_acc, margin


def distinct_per_caption(tokens, seq):
    """mean number of distinct sequences among a caption's B hypotheses: tokens [N, B, T], seq [N, B]"""
    t, s = np.asarray(tokens), np.asarray(seq)
    return float(np.mean([len({tuple(t[r, b, :int(s[r, b])]) for b in range(t.shape[1])}) for r in range(t.shape[0])]))
