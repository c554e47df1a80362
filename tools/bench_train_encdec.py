#!/usr/bin/env python
"""Time the train step of the encoder-decoder mapper (MappingType.TransformerDecoder) at the reference's own run -- batch 24,
prefix_length 80, clip_length 10, num_layers 4 (GPT-2 small, frozen) -- beside the TransformerMapper(8) step at the same
batch and prefix_length, the step that predates it.  Each figure is the median of ``--steps`` steps after ``--warmup``
steps, host-timed around steps that wait for their loss; one more profiled step per configuration gives the share of the
mapper's attention kernels (forward and backward, the ``attn_mapper`` family of capdec_profile_get) in the step's kernel time.

    python tools/bench_train_encdec.py [--steps 20] [--warmup 5] [--out profiles/train_encdec_bench.txt]

Needs an MI355X."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from capdec_amd import synth  # noqa: E402
from capdec_amd import train as Tr  # noqa: E402
from capdec_amd.gpt2_prefix import ClipCaptionPrefix, MappingType  # noqa: E402

B, P, C, D, LEN = 24, 80, 10, 512, 20


def make(mapping: str, layers: int, dims):
    mt = MappingType.TransformerDecoder if mapping == "transformer_decoder" else MappingType.TransformerEncoder
    m = ClipCaptionPrefix(P, clip_length=C, prefix_dim=D, num_layers=layers, mapping_type=mt, gpt2_dims=dims).to("cuda:0")
    m.load_state_dict(synth.hot_state_dict(42, mapping, D, P, C, layers, dims))
    m.train()
    if mt == MappingType.TransformerDecoder:
        m.clip_project.requires_grad_()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_train_encdec needs an MI355X"
    dims = synth.GPT2_SMALL
    gen = torch.Generator().manual_seed(1)
    tokens = torch.randint(1, dims.vocab, (B, LEN), generator=gen)
    mask = torch.ones(B, P + LEN)
    x = synth.synthetic_clip_embeddings(B, D, seed=1).cuda()
    lines, runs = [], []
    for name, mapping, layers in (("EncoderDecoder(4)", "transformer_decoder", 4), ("TransformerMapper(8)", "transformer_encoder", 8)):
        model = make(mapping, layers, dims)
        opt = Tr.AdamW(model.parameters(), lr=2e-5)
        for _ in range(args.warmup):
            Tr.train_step(model, opt, tokens, mask, x)
        ms = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            Tr.train_step(model, opt, tokens, mask, x)
            ms.append((time.perf_counter() - t0) * 1e3)
        eng = model.engine
        eng.profile_reset()
        eng.profile_enable(True)
        Tr.train_step(model, opt, tokens, mask, x)
        prof = {k: v for k, v in eng.profile_get().items() if v["launches"]}
        eng.profile_enable(False)
        tot = sum(v["ms"] for v in prof.values())
        att = prof.get("attn_mapper", {"ms": 0.0, "launches": 0})
        med = sorted(ms)[len(ms) // 2]
        run = dict(config=name, batch=B, prefix_length=P, clip_length=C, caption_length=LEN, ms_median=med, ms_min=min(ms), ms_max=max(ms),
                   mapper_attention_ms=att["ms"], mapper_attention_launches=att["launches"], profiled_kernel_ms=tot,
                   mapper_attention_share=att["ms"] / tot if tot else None)
        runs.append(run)
        lines.append(f"{name:22s} B {B} P {P} C {C} L_caption {LEN}: {med:8.3f} ms / step (median of {args.steps} after {args.warmup}; "
                     f"min {min(ms):.3f} max {max(ms):.3f}); mapper attention forward + backward {att['ms']:.3f} ms in "
                     f"{att['launches']} launches = {100 * (run['mapper_attention_share'] or 0):.1f} % of {tot:.3f} ms of profiled kernel time")
        print(lines[-1], flush=True)
        model.release()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"bench_train_encdec": runs}))


if __name__ == "__main__":
    main()
