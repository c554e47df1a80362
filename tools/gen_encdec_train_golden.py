#!/usr/bin/env python3
"""tests/golden/train_step_ed_tiny.npz: the train step of the encoder-decoder mapper (MappingType.TransformerDecoder) with a
frozen GPT-2, from the REFERENCE's own modules on the CPU -- gpt2_prefix.ClipCaptionPrefix in train() mode, its own
loss.backward() -- modelled on gen_train_step of tools/gen_golden.py (same batches, same schedule: lr 2e-3, warm-up 2).

Per iteration: tokens, mask, prefix, lr, the loss, and for each of the 75 tensors the fp32 autograd gradient and the
gradient of the same modules in float64 (copy.deepcopy(model).double()), both on a strided subsample of at most SUB
entries, plus the float64 norm.  Between iterations the weights move by oracle.adamw_transformers, as in gen_train_step --
here on the float64 gradients with float64 moments, the result rounded to fp32: a test can then replay the chain from its
own float64 gradients and arrive at the SAME fp32 weights (an fp32 chain would amplify the last bit of every gradient
through Adam's sign-like first steps), so the float64 gradients of the later iterations are pinned to 1e-9 too.

Every iteration is pinned: the reference's own fp32 gradient must lie within a tenth of the test's bound (3e-3 of the
tensor's largest entry, norm 2e-3) of its float64 gradient.  Iteration 0 always is; should a LATER one fail, the generator
starts over with a smaller lr (recorded in the fixture) -- the bound is never widened.

    python tools/gen_encdec_train_golden.py
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from capdec_amd import synth  # noqa: E402
from encdec_train_def import subsample  # noqa: E402
from gen_golden import OUT, import_reference  # noqa: E402

SUB = 256                       # entries per tensor and iteration: 75 x 3 x 256 x 12 bytes keeps the file well below 1 MB
GRAD_BOUND, NORM_BOUND = 3e-3, 2e-3
P, C, D, NLAY = 10, 10, 512, 2
LENS = [[9, 4, 7], [5, 8, 3], [6, 6, 9]]


def loss_of(model, tokens, prefix, mask):
    logits = model(tokens, prefix, mask).logits[:, P - 1:-1]
    return torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), tokens.flatten(), ignore_index=0)


def run(gpt2_prefix, dims, lr):
    from transformers import GPT2Config, GPT2LMHeadModel, get_linear_schedule_with_warmup
    from oracle import capdec_oracle as O
    cfg = GPT2Config(n_layer=dims.n_layer, n_head=dims.n_head, n_embd=dims.n_embd, vocab_size=dims.vocab, n_positions=dims.n_pos)
    GPT2LMHeadModel.from_pretrained = staticmethod(lambda name, *a, **k: GPT2LMHeadModel(cfg))
    model = gpt2_prefix.ClipCaptionPrefix(P, clip_length=C, prefix_dim=D, num_layers=NLAY,
                                          mapping_type=gpt2_prefix.MappingType.TransformerDecoder)
    model.train()
    assert not model.gpt.training and model.clip_project.training
    sd = synth.hot_state_dict(42, "transformer_decoder", D, P, C, NLAY, dims)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(".attn.bias" in m or ".attn.masked_bias" in m for m in missing)
    names = [k for k, _ in model.named_parameters() if k.startswith("clip_project.")]
    params = list(model.parameters())
    keys = [k for k in model.state_dict() if k.startswith("clip_project.")]
    assert len(params) == len(names) == len(keys) == 3 + 36 * NLAY and sorted(names) == sorted(keys)
    g = torch.Generator().manual_seed(23)
    warm, total = 2, 8
    dummy = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)     # only carries the lr for the real scheduler
    sched = get_linear_schedule_with_warmup(dummy, num_warmup_steps=warm, num_training_steps=total)
    state = {k: (torch.zeros_like(q, dtype=torch.float64), torch.zeros_like(q, dtype=torch.float64)) for k, q in zip(names, params)}
    res = {"sd_crc": np.uint32(synth.state_dict_checksum(sd)), "lr": np.float64(lr), "warmup": np.int32(warm),
           "total": np.int32(total), "keys": np.array(keys), "sub": np.int32(SUB), "geom": np.array([P, C, NLAY, D], np.int32)}
    losses, lrs, worst = [], [], []
    for it, lens in enumerate(LENS):
        L = max(lens)
        tokens = torch.zeros(len(lens), L, dtype=torch.int64)
        mask = torch.zeros(len(lens), P + L)
        mask[:, :P] = 1
        for r, n in enumerate(lens):
            tokens[r, :n] = torch.randint(1, dims.vocab, (n,), generator=g)
            mask[r, P:P + n] = 1
        if it == 1:
            tokens[1, 2] = 0                 # a REAL token with id 0 is ignored by the loss as well (ignore_index=0)
        prefix = synth.synthetic_clip_embeddings(len(lens), D, seed=50 + it)
        model.zero_grad()
        loss = loss_of(model, tokens, prefix, mask)
        loss.backward()
        m64 = copy.deepcopy(model).double()
        m64.zero_grad()
        loss_of(m64, tokens, prefix.double(), mask.double()).backward()
        g64 = dict((k, q.grad.detach()) for k, q in m64.named_parameters() if k.startswith("clip_project."))
        cur_lr = dummy.param_groups[0]["lr"]
        res[f"tokens_{it}"], res[f"mask_{it}"], res[f"prefix_{it}"] = tokens.numpy(), mask.numpy(), prefix.numpy()
        w_it = 0.0
        for k, q in zip(names, params):
            gk = q.grad.detach()
            s32, s64 = subsample(gk, SUB).numpy().copy(), subsample(g64[k], SUB).numpy().copy()
            res[f"grad_{it}_{k}_sub"], res[f"grad64_{it}_{k}_sub"] = s32, s64
            res[f"grad64_{it}_{k}_norm"] = np.float64(g64[k].norm())
            assert np.abs(s64).max() > 0, f"iteration {it}, {k}: the subsample sees no gradient"
            rel = float(np.abs(s32 - s64).max() / np.abs(s64).max())
            nrm = abs(float(gk.double().norm()) / float(g64[k].norm()) - 1.0)
            w_it = max(w_it, rel / GRAD_BOUND, nrm / NORM_BOUND)
            with torch.no_grad():
                p64 = q.data.double()
                O.adamw_transformers(p64, g64[k], state[k][0], state[k][1], it + 1, cur_lr)
                q.data.copy_(p64.float())
        worst.append(w_it)
        losses.append(float(loss.detach()))
        lrs.append(cur_lr)
        dummy.step()
        sched.step()
    res["losses"], res["lrs"] = np.array(losses, np.float32), np.array(lrs, np.float64)
    return res, worst


def main():
    gpt2_prefix = import_reference()[0]
    lr = 2e-3
    while True:
        res, worst = run(gpt2_prefix, synth.GPT2_TINY, lr)
        print(f"lr {lr}: reference fp32 vs float64, worst fraction of the bound per iteration {[f'{w:.2e}' for w in worst]}")
        assert worst[0] <= 0.1, "iteration 0: the reference's fp32 gradient is not within a tenth of the bound of its float64 one"
        if max(worst) <= 0.1:
            break
        lr /= 2
        assert lr > 1e-5, "no lr at which the later iterations can be pinned"
    path = os.path.join(OUT, "train_step_ed_tiny.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    assert size <= 2_000_000, size
    print(f"{path}: {size} bytes; losses {res['losses']} lrs {res['lrs']}")


if __name__ == "__main__":
    main()
