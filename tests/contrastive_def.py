"""The contract of ``capdec_decode_contrastive`` (include/capdec.h) -- contrastive search, Su et al. 2022 (``penalty_alpha`` /
``top_k`` of ``transformers.generate``) -- as torch on the CPU oracle: ``oracle.capdec_oracle.gpt2_hidden`` (which returns the
ln_f output) with its KV cache, the candidates' caches being the path's cache repeated K times, of which the winner's rows
are kept; ``process_def.process`` for the logits processors.  fp32 by default; ``dtype=torch.float64`` runs the same code
in float64 (torch's default dtype is switched for the run: the oracle's mask constant overflows otherwise).

Per caption, with H the L2-normalised hidden states of the context so far and ``last`` the chosen path's newest one:
    lg = process(last . wte^T);  v_0..v_{K-1} = the K largest (larger value, then smaller token);  p_c = softmax(lg)[v_c]
    h_c = hid(v_c fed at pos = P + t on the path's cache);  sim_c = max_j cos(h_c, H_j), j < pos
    score_c = (1 - alpha) * p_c - alpha * sim_c;  winner = the first arg-max;  emit v_w, append h_w, keep w's cache rows
"""
import collections

import numpy as np
import torch

import process_def as PD

#: what `contrastive` returns; step_margin [N, T]: the margin of every live step (inf elsewhere), margin its minimum
Result = collections.namedtuple("Result", "ids lens trace margin picks step_margin")


def _unit(h):
    return h / h.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def contrastive(sd, prefix, p, top_k, alpha, stop_id, T, alt_stop_id=-1, n_head=12, dtype=torch.float32):
    """prefix [N, P, d] -> Result(ids int32 [N, T] zero padded, lens int32 [N] including the stop token, trace [N, T, 2] = (p, sim)
    of the chosen candidate, margin fp64 [N], picks int [N, T] = the winner's place c in the candidate list, -1 where nothing
    was emitted).  margin: the smallest, over the caption's live steps, of (best - second best score) and of the smallest
    gap between adjacent logits among the best K + 1 (another candidate set changes everything after it)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        return _contrastive(sd, prefix, p, int(top_k), float(alpha), stop_id, T, alt_stop_id, n_head, dtype)
    finally:
        torch.set_default_dtype(old)


def _contrastive(sd, prefix, p, K, alpha, stop_id, T, alt_stop_id, n_head, dtype):
    from oracle import capdec_oracle as O
    if dtype != torch.float32:
        sd = {k: (v.to(dtype) if torch.is_floating_point(v) else v) for k, v in sd.items()}
    prefix = prefix.to(dtype)
    N, P, d = prefix.shape
    W = sd["gpt.transformer.wte.weight"]
    nl = O._n_layer(sd, "gpt.")
    cache = [None] * nl
    hid = O.gpt2_hidden(prefix, sd, n_head, "gpt.", 0, cache)
    H = _unit(hid)                                          # [N, pos, d]
    last = hid[:, -1]
    ids = np.zeros((N, T), dtype=np.int32)
    lens = np.zeros(N, dtype=np.int32)
    trace = np.zeros((N, T, 2), dtype=np.float64)
    picks = np.full((N, T), -1, dtype=np.int64)
    step_margin = np.full((N, T), np.inf)
    done = np.zeros(N, dtype=bool)
    ar = torch.arange(N)
    for t in range(T):
        lg = (last @ W.t()).numpy()
        q = np.stack([PD.process(lg[r], ids[r, :t], p, (stop_id, alt_stop_id)) for r in range(N)])
        q = torch.from_numpy(q).to(dtype)
        sv, si = torch.sort(q, dim=-1, descending=True, stable=True)        # equal values: the smaller token first
        cand = si[:, :K]
        prob = q.softmax(-1).gather(1, cand)                                # [N, K]
        lgap = sv[:, :K] - sv[:, 1:K + 1]
        lgap = torch.where(torch.isnan(lgap), torch.full_like(lgap, float("inf")), lgap).min(dim=-1).values
        cc = [[c.repeat_interleave(K, dim=0) for c in layer] for layer in cache]
        h = O.gpt2_hidden(W[cand.reshape(-1)].unsqueeze(1), sd, n_head, "gpt.", P + t, cc)[:, -1].view(N, K, d)
        sim = torch.einsum("nkd,njd->nkj", _unit(h), H).max(dim=-1).values  # [N, K]
        score = (1 - alpha) * prob - alpha * sim
        w = torch.from_numpy(np.argmax(score.numpy(), axis=1))              # the first arg-max: a tie goes to the lower c
        if K > 1:
            s2 = score.sort(dim=-1, descending=True).values
            sgap = s2[:, 0] - s2[:, 1]
        else:
            sgap = torch.full((N,), float("inf"))
        both = torch.minimum(sgap, lgap).double().numpy()
        for r in range(N):
            if done[r]:
                continue
            c = int(w[r])
            tok = int(cand[r, c])
            ids[r, t] = tok
            lens[r] = t + 1
            trace[r, t] = (float(prob[r, c]), float(sim[r, c]))
            picks[r, t] = c
            step_margin[r, t] = both[r]
            done[r] = tok in (stop_id, alt_stop_id)
        if done.all() or t == T - 1:
            break
        hw = h[ar, w]
        H = torch.cat((H, _unit(hw)[:, None]), dim=1)
        rows = ar * K + w
        cache = [[c[rows] for c in layer] for layer in cc]
        last = hw
    return Result(ids, lens, trace, step_margin.min(axis=1), picks, step_margin)


def distinct_tokens(ids, lens):
    """mean number of distinct tokens per caption"""
    return float(np.mean([len(set(ids[r, :lens[r]].tolist())) for r in range(ids.shape[0])]))
