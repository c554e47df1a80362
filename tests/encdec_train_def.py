"""The train step of the encoder-decoder mapper (MappingType.TransformerDecoder), restated in float64 as plain torch ops so
that autograd gives its gradients.  Written from the description of the network, not from the kernels:

    ref = linear(x) viewed [B, C, 512]; L pre-LN layers over it (queries, keys and values all from norm1)
    h   = prefix_const for every caption; 2 L pre-LN layers at width d:
          even layers: queries from norm1(h), keys / values from ``ref``
          odd layers:  queries from norm1(h), keys / values from h ITSELF (not from norm1(h))
    a layer: h += project(softmax(q k^T / sqrt(hd)) v);  h += fc2(relu(fc1(norm2(h))))

GPT-2 and the loss come from the oracle's existing functions (oracle/capdec_oracle.py: gpt2_logits), as for the other
mappers.  ``wrong`` names two mistakes a hand-written backward can make; the tests check that each one is far from the truth."""
from __future__ import annotations

from collections import OrderedDict

import torch

ENC = 512
WRONG = ("self_kv_detached", "ref_detached_but_last")


def _ln(x, w, b):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


def _layer(p, pre, x, y, heads=8):
    """one pre-LN layer; keys / values from ``y`` as given (None: from norm1(x), like the queries)"""
    g = lambda k: p[pre + k]
    xn = _ln(x, g("norm1.weight"), g("norm1.bias"))
    y = xn if y is None else y
    n, nq, w = x.shape
    nk, hd = y.shape[1], w // heads
    q = (xn @ g("attn.to_queries.weight").T).reshape(n, nq, heads, hd)
    kv = (y @ g("attn.to_keys_values.weight").T).reshape(n, nk, 2, heads, hd)
    att = (torch.einsum("bnhd,bmhd->bnmh", q, kv[:, :, 0]) * hd ** -0.5).softmax(dim=2)
    o = torch.einsum("bnmh,bmhd->bnhd", att, kv[:, :, 1]).reshape(n, nq, w)
    x = x + o @ g("attn.project.weight").T + g("attn.project.bias")
    f = torch.relu(_ln(x, g("norm2.weight"), g("norm2.bias")) @ g("mlp.fc1.weight").T + g("mlp.fc1.bias"))
    return x + f @ g("mlp.fc2.weight").T + g("mlp.fc2.bias")


def mapper(p, x, wrong=None):
    """``p``: the mapper's tensors by their names in ``clip_project.state_dict()``; x [B, D] -> [B, P, d]"""
    assert wrong is None or wrong in WRONG
    L = 0
    while f"ref_encoder.layers.{L}.norm1.weight" in p:
        L += 1
    ref = (x @ p["linear.weight"].T + p["linear.bias"]).reshape(x.shape[0], -1, ENC)
    for i in range(L):
        ref = _layer(p, f"ref_encoder.layers.{i}.", ref, None)
    pc = p["prefix_const"]
    h = pc.unsqueeze(0).expand(x.shape[0], *pc.shape)
    for i in range(2 * L):
        pre = f"prefix_decoder.layers.{i}."
        if i % 2 == 0:
            y = ref.detach() if wrong == "ref_detached_but_last" and i != 2 * L - 2 else ref
        else:
            y = h.detach() if wrong == "self_kv_detached" else h
        h = _layer(p, pre, h, y)
    return h


def loss_and_grads(sd, tokens, prefix, n_head=12, wrong=None, train_gpt=False, dtype=torch.float64):
    """the step of reference train.py:345-350 on the full state dict ``sd`` ("clip_project." / "gpt." keys) ->
    (loss, {state-dict name: gradient}) for the mapper's tensors, and GPT-2's (the tied wte once) when ``train_gpt``"""
    from oracle import capdec_oracle as O
    w = OrderedDict((k, v.detach().to(dtype).clone()) for k, v in sd.items() if k != "gpt.lm_head.weight")
    leaves = [k for k in w if k.startswith("clip_project.") or (train_gpt and k.startswith("gpt."))]
    for k in leaves:
        w[k].requires_grad_(True)
    p = {k[len("clip_project."):]: v for k, v in w.items() if k.startswith("clip_project.")}
    pe = mapper(p, prefix.to(dtype), wrong)
    P = pe.shape[1]
    tokens = tokens.long()
    hf, _ = O.gpt2_forward_saved(torch.cat((pe, O.wte(tokens, w)), dim=1), w, n_head)       # (plain ops at the weights' dtype)
    logits = hf[:, P - 1:-1] @ w["gpt.transformer.wte.weight"].t()
    loss = torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), tokens.flatten(), ignore_index=0)
    grads = torch.autograd.grad(loss, [w[k] for k in leaves])
    return float(loss.detach()), OrderedDict(zip(leaves, grads))


def subsample(t, count):
    """the fixture's strided subsample of a tensor: at most ``count`` entries, at an ODD stride -- an even one walks down a
    single column of these matrices (their widths are 2^k and 3 * 2^k), and the column of a dead ReLU unit is all zeros"""
    flat = t.detach().flatten()
    return flat[::-(-flat.numel() // count) | 1]
