"""The contract of ``capdec_decode_guided`` (include/capdec.h) -- classifier-free guidance on the greedy and the beam decode,
``guidance_scale`` of ``transformers.generate`` -- as torch on the CPU oracle: ``oracle.capdec_oracle.gpt2_hidden`` with TWO
KV caches (the caption's own prefix and its negative prefix, fed the same tokens), ``process_def.process`` for the logits
processors, the beam bookkeeping of ``process_def.beam`` op for op.  fp32 by default; ``dtype=torch.float64`` runs the same
code in float64 (torch's default dtype is switched for the run, as contrastive_def.py does).

Per hypothesis, with l / m the lm_head logits of its two contexts and gamma = guidance_scale:
    c = log_softmax(l);  u = log_softmax(m);  g = gamma * c + (1 - gamma) * u
    q = process(g, the hypothesis's own tokens);  s = q / temperature;  then arg-max (greedy) or log_softmax(s) and the beam
    step (beam): the beam scores are sums of the RENORMALISED guided log-probabilities.
"""
import collections

import numpy as np
import torch

import process_def as PD

#: gaps [N, T]: the top-2 gap of the processed guided logits of every emitted token's step, inf elsewhere
Greedy = collections.namedtuple("Greedy", "ids lens gaps")
#: internal beam order, as process_def.beam; margin [N] = step_margin.min(1); step_margin [N, T]: the smallest gap between two
#: adjacent keys among the best B + 1 candidates of every live step, inf elsewhere
Beam = collections.namedtuple("Beam", "tokens seq scores margin step_margin")


def _run(fn, sd, prefix, neg, dtype, *args):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        if dtype != torch.float32:
            sd = {k: (v.to(dtype) if torch.is_floating_point(v) else v) for k, v in sd.items()}
        prefix, neg = prefix.to(dtype), neg.to(dtype)
        if neg.dim() == 2:
            neg = neg[None]
        assert neg.shape[1:] == prefix.shape[1:] and neg.shape[0] in (1, prefix.shape[0]), (neg.shape, prefix.shape)
        return fn(sd, prefix, neg.expand(prefix.shape[0], -1, -1).contiguous(), dtype, *args)
    finally:
        torch.set_default_dtype(old)


def guide(l, m, gamma):
    """two rows (or stacks of rows) of raw logits -> the guided logits, in this form: equal rows give g = c up to rounding"""
    return gamma * l.log_softmax(-1) + (1 - gamma) * m.log_softmax(-1)


def guided_greedy(sd, prefix, neg, gamma, p, stop_id, T, alt_stop_id=-1, n_head=12, dtype=torch.float32):
    """prefix [N, P, d], neg [P, d] / [1, P, d] / [N, P, d] -> Greedy(ids int32 [N, T] zero padded, lens int32 [N] including
    the stop token, gaps fp64 [N, T])"""
    return _run(_greedy, sd, prefix, neg, dtype, float(gamma), p, stop_id, T, alt_stop_id, n_head)


def _greedy(sd, prefix, neg, dtype, gamma, p, stop_id, T, alt_stop_id, n_head):
    from oracle import capdec_oracle as O
    N, P, _ = prefix.shape
    W = sd["gpt.transformer.wte.weight"]
    nl = O._n_layer(sd, "gpt.")
    cc, cn = [None] * nl, [None] * nl
    ids = np.zeros((N, T), dtype=np.int32)
    lens = np.zeros(N, dtype=np.int32)
    gaps = np.full((N, T), np.inf)
    done = np.zeros(N, dtype=bool)
    hc = O.gpt2_hidden(prefix, sd, n_head, "gpt.", 0, cc)[:, -1]
    hn = O.gpt2_hidden(neg, sd, n_head, "gpt.", 0, cn)[:, -1]
    for i in range(T):
        g = guide(hc @ W.t(), hn @ W.t(), gamma).numpy()
        nxt = np.zeros(N, dtype=np.int64)
        for r in range(N):
            if done[r]:
                continue
            q = PD.process(g[r], ids[r, :i], p, (stop_id, alt_stop_id))
            nxt[r] = int(np.argmax(q))
            gaps[r, i] = PD.top2_gap(q)
            ids[r, i] = nxt[r]
            lens[r] += 1
            done[r] = nxt[r] in (stop_id, alt_stop_id)
        if done.all() or i == T - 1:
            break
        x = W[torch.from_numpy(nxt)].unsqueeze(1)               # the same tokens go to both contexts
        hc = O.gpt2_hidden(x, sd, n_head, "gpt.", P + i, cc)[:, -1]
        hn = O.gpt2_hidden(x, sd, n_head, "gpt.", P + i, cn)[:, -1]
    return Greedy(ids, lens, gaps)


def guided_beam(sd, prefix, neg, gamma, p, beam_size, stop_id, T, temperature=1.0, n_head=12, dtype=torch.float32):
    """process_def.beam with the guided logits in the place of the raw ones and a second cache that follows the first's
    re-ordering -> Beam(tokens int32 [N, B, T], seq int32 [N, B], scores [N, B] (mean log-probs), margin [N], step_margin
    [N, T]) in the internal beam order"""
    return _run(_beam, sd, prefix, neg, dtype, float(gamma), p, int(beam_size), stop_id, T, temperature, n_head)


def _beam(sd, prefix, neg, dtype, gamma, p, B, stop_id, T, temperature, n_head):
    from oracle import capdec_oracle as O
    N, P, d = prefix.shape
    nl = O._n_layer(sd, "gpt.")
    cc, cn = [None] * nl, [None] * nl
    W = sd["gpt.transformer.wte.weight"]
    V = W.shape[0]
    temp = temperature if temperature > 0 else 1.0

    def processed(hc, hn, hist):
        g = guide(hc @ W.t(), hn @ W.t(), gamma).numpy()
        return torch.from_numpy(np.stack([PD.process(g[r], hist[r], p, (stop_id,)) for r in range(g.shape[0])])).to(dtype)

    def adjacent_gap(keys):
        t = keys.topk(min(B + 1, keys.shape[-1]), -1).values
        g = t[:, :-1] - t[:, 1:]
        g = torch.where(torch.isnan(g), torch.full_like(g, float("inf")), g)       # (-inf) - (-inf): no decision there
        return g.min(dim=-1).values

    hc = O.gpt2_hidden(prefix, sd, n_head, "gpt.", 0, cc)[:, -1]
    hn = O.gpt2_hidden(neg, sd, n_head, "gpt.", 0, cn)[:, -1]
    logp = (processed(hc, hn, [[]] * N) / temp).softmax(-1).log()
    scores, nxt = logp.topk(B, -1)
    step_margin = np.full((N, T), np.inf)
    step_margin[:, 0] = adjacent_gap(logp).double().numpy()
    tokens = torch.zeros(N, B, T, dtype=torch.int64)
    tokens[:, :, 0] = nxt
    seq = torch.ones(N, B)
    stopped = nxt.eq(stop_id)
    for cache in (cc, cn):
        for i in range(nl):
            cache[i] = [c.repeat_interleave(B, dim=0) for c in cache[i]]
    alive = ~stopped.all(dim=1)
    for i in range(1, T):
        if not bool(alive.any()):
            break
        x = W[nxt.reshape(-1)].unsqueeze(1)
        hc = O.gpt2_hidden(x, sd, n_head, "gpt.", P + i - 1, cc)[:, -1]
        hn = O.gpt2_hidden(x, sd, n_head, "gpt.", P + i - 1, cn)[:, -1]
        hist = tokens[:, :, :i].reshape(N * B, i).numpy()
        logp = (processed(hc, hn, hist) / temp).softmax(-1).log().view(N, B, V)
        logp[stopped] = -float("inf")
        logp[stopped, 0] = 0
        ssum = scores[:, :, None] + logp
        seq_new = seq + (~stopped).to(dtype)
        avg = ssum / seq_new[:, :, None]
        avg_top, flat = avg.view(N, -1).topk(B, -1)
        gap = adjacent_gap(avg.view(N, -1)).double().numpy()
        step_margin[alive.numpy(), i] = gap[alive.numpy()]
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
        for cache in (cc, cn):                                  # the partner's cache follows the same re-ordering
            for l in range(nl):
                cache[l] = [c[rows] for c in cache[l]]
        alive = alive & ~stopped.all(dim=1)
    return Beam(tokens.to(torch.int32).numpy(), seq.to(torch.int32).numpy(), (scores / seq).double().numpy(),
                step_margin.min(axis=1), step_margin)
