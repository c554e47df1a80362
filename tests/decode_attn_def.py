"""Teacher-forced GPT-2 decode, restated on the full sequence in float64 -- what tests/test_decode_attention.py checks the
decode-attention kernel (``attn_decode_beams_kernel``) against.

Caption r has prefix rows ``prefix[r]`` [P, d] and tokens ``tok[r, 0..T)``.  The model input is
``cat(prefix[r], wte(tok[r, :T-1])) + wpe``; step i (0 <= i < T) is the logits row at position P-1+i.  Step 0 belongs to
the prefill; steps 1..T-1 are the rows a KV-cached decode computes one at a time, query position q = P-1+i attending to
the keys 0..q.  All T-1 of them are computed here as ONE causal block against K / V of the whole sequence: no cache append,
no ancestor table, no online softmax -- nothing of the kernel's structure.

``hide`` plants a fault: one key position is hidden from every DECODE query (q >= P); the prefix rows and step 0 are
untouched.  The variants are the positions a wrong peel, a wrong tail mask or a wrong own-token term would lose:

    "key0"      key 0                         "prefix_last"  key P-1
    "previous"  key q-1 (the previous token)  "first_token"  key P (the first decoded token's own position)

Self-contained (it does not call the oracle): ``tests/test_decode_attention.py`` pins it in fp32 against
``oracle.greedy_forced``.
"""
import math

import torch

HIDE = ("key0", "prefix_last", "previous", "first_token")


def _ln(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * w + b


def _gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


class Prefilled:
    """the prefix rows of n captions through every block, in ``dtype``: per-layer K / V [n, heads, P, 64] and the final
    hidden row of position P-1 (step 0).  Shared by every ``forced_logits`` call on the same prefixes."""

    def __init__(self, sd, prefix, n_head, dtype=torch.float64, g="gpt."):
        self.dtype, self.n_head, self.t = dtype, n_head, g + "transformer."
        self.sd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(self.t)}
        self.n_layer = 0
        while f"{self.t}h.{self.n_layer}.ln_1.weight" in self.sd:
            self.n_layer += 1
        self.n, self.P, self.d = prefix.shape
        self.kv = [[None, None] for _ in range(self.n_layer)]
        rows = []
        for r in range(self.n):                       # one caption at a time: the score matrix of 1000 positions is 96 MB
            rows.append(self._blocks(prefix[r:r + 1].to(dtype), 0, None, None, r)[:, -1])
        self.h0 = torch.cat(rows)                      # [n, d] after ln_f

    def _blocks(self, x, pos0, past, hide, store_row=None):
        """x [m, L, d] at positions pos0.. -> ln_f(h) [m, L, d].  past: per-layer (K, V) [m, heads, pos0, 64] or None."""
        sd, t, H = self.sd, self.t, self.n_head
        m, L, d = x.shape
        hd = d // H
        h = x + sd[t + "wpe.weight"][pos0:pos0 + L]
        qpos = torch.arange(pos0, pos0 + L)[:, None]
        kpos = torch.arange(0, pos0 + L)[None, :]
        visible = kpos <= qpos
        if hide is not None:
            gone = {"key0": kpos == 0, "prefix_last": kpos == self.P - 1, "previous": kpos == qpos - 1,
                    "first_token": kpos == self.P}[hide]
            visible = visible & ~(gone & (qpos >= self.P))
        for i in range(self.n_layer):
            b = f"{t}h.{i}."
            a = _ln(h, sd[b + "ln_1.weight"], sd[b + "ln_1.bias"])
            qkv = a @ sd[b + "attn.c_attn.weight"] + sd[b + "attn.c_attn.bias"]
            q, k, v = (u.reshape(m, L, H, hd).transpose(1, 2) for u in qkv.split(d, dim=2))
            if store_row is not None:
                for j, u in enumerate((k, v)):
                    self.kv[i][j] = u if store_row == 0 else torch.cat((self.kv[i][j], u))
            if past is not None:
                k, v = torch.cat((past[i][0], k), dim=2), torch.cat((past[i][1], v), dim=2)
            w = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
            w = w.masked_fill(~visible, float("-inf")).softmax(-1)
            o = (w @ v).transpose(1, 2).reshape(m, L, d)
            h = h + o @ sd[b + "attn.c_proj.weight"] + sd[b + "attn.c_proj.bias"]
            f = _ln(h, sd[b + "ln_2.weight"], sd[b + "ln_2.bias"])
            f = _gelu_new(f @ sd[b + "mlp.c_fc.weight"] + sd[b + "mlp.c_fc.bias"])
            h = h + f @ sd[b + "mlp.c_proj.weight"] + sd[b + "mlp.c_proj.bias"]
        return _ln(h, sd[t + "ln_f.weight"], sd[t + "ln_f.bias"])


def forced_logits(pf, tokens, hide=None):
    """tokens [n, T] or [n, B, T] (B rows sharing caption r's prefix) -> logits ``pf.dtype`` [n(, B), T, V]: step i is
    the row that predicts tokens[..., i]; tokens[..., :T-1] are fed."""
    assert hide is None or hide in HIDE
    tok = torch.as_tensor(tokens).long()
    shape = tok.shape
    rep = 1 if tok.dim() == 2 else shape[1]
    tok = tok.reshape(-1, shape[-1])
    T = tok.shape[1]
    W = pf.sd[pf.t + "wte.weight"]
    h0 = pf.h0.repeat_interleave(rep, dim=0)[:, None]
    if T > 1:
        past = [[u.repeat_interleave(rep, dim=0) for u in kv] for kv in pf.kv]
        h = torch.cat((h0, pf._blocks(W[tok[:, :-1]], pf.P, past, hide)), dim=1)
    else:
        h = h0
    return (h @ W.t()).reshape(*shape, W.shape[0])


def stats(logits):
    """-> (arg-max ids int64 [..., T], [..., T, 3] = top-1 logit, top-2 logit, logsumexp): what decode_greedy_forced returns"""
    top = logits.topk(2, -1)
    return top.indices[..., 0], torch.stack((top.values[..., 0], top.values[..., 1], torch.logsumexp(logits, -1)), dim=-1)


def token_logp(logits, tokens):
    """log-prob of tokens[..., i] at step i -> [..., T]"""
    lp = logits - torch.logsumexp(logits, -1, keepdim=True)
    return torch.gather(lp, -1, torch.as_tensor(tokens).long()[..., None])[..., 0]
