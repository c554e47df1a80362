#!/usr/bin/env python
"""Time ``mapper_forward`` of the encoder-decoder mapper (MappingType.TransformerDecoder) beside the 8-layer
TransformerMapper, the yardstick that predates it: device events around whole calls after warm-up, the configurations
alternating inside every round, then one profiled pass per configuration for the per-family split (capdec_profile_get).
FLOP are the algorithm's, from the shapes (``flop_*`` below) -- what the hoists save is not subtracted.

    python tools/bench_mapper.py [--captions 5000 625] [--rounds 5] [--reps 10] [--out FILE.json]

Needs an MI355X."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from capdec_amd import synth  # noqa: E402
from capdec_amd.engine import Engine  # noqa: E402

D, P, C, d, ENC = 512, 10, 10, 768, 512


def flop_transformer_mapper(L: int) -> float:
    """per caption: linear, then L layers on P + C tokens: qkv 6 d^2, project 2 d^2, MLP (ratio 2) 8 d^2 per token, 4 S^2 d attention"""
    S = P + C
    return 2.0 * D * C * d + L * (S * 16.0 * d * d + 4.0 * S * S * d)


def flop_encdec(L: int) -> float:
    """per caption: linear; L encoder layers on C tokens at 512; 2 L decoder layers on P tokens at d, whose keys / values
    come from C encoder rows (cross, K = 512) or P stream rows (self, K = d)"""
    enc = L * (C * 16.0 * ENC * ENC + 4.0 * C * C * ENC)
    dec = 2 * L * P * 12.0 * d * d + L * (C * 4.0 * ENC * d + 4.0 * P * C * d) + L * (P * 4.0 * d * d + 4.0 * P * P * d)
    return 2.0 * D * C * ENC + enc + dec


def make(kind: str, L: int) -> Engine:
    e = Engine(0)
    if kind == "transformer":
        e.load_mapper_transformer(synth.hot_transformer_mapper_state_dict(43, D, P, C, L))
    else:
        e.load_mapper_encdec(synth.hot_encdec_mapper_state_dict(43, D, P, C, L))
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captions", type=int, nargs="*", default=[5000, 625])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mapper needs an MI355X"
    cfgs = [("TransformerMapper(8)", "transformer", 8, flop_transformer_mapper(8)),
            ("EncoderDecoder(4)", "encdec", 4, flop_encdec(4)),
            ("EncoderDecoder(8)", "encdec", 8, flop_encdec(8))]
    engines = [make(kind, L) for _, kind, L, _ in cfgs]
    result = {"shape": dict(D=D, P=P, C=C, d=d), "rounds": args.rounds, "reps": args.reps, "runs": []}
    for n in args.captions:
        x = synth.synthetic_clip_embeddings(n, D, seed=1).cuda()
        for e in engines:                                   # warm-up: buffers, weight planes, code objects
            for _ in range(3):
                e.mapper_forward(x)
        torch.cuda.synchronize()
        ms = [[] for _ in cfgs]
        for _ in range(args.rounds):
            for i, e in enumerate(engines):                 # alternating: every round times every configuration
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.reps):
                    e.mapper_forward(x)
                b.record()
                b.synchronize()
                ms[i].append(a.elapsed_time(b) / args.reps)
        for i, (name, kind, L, flop) in enumerate(cfgs):
            e = engines[i]
            e.profile_reset()
            e.profile_enable(True)
            for _ in range(3):
                e.mapper_forward(x)
            e.synchronize()
            prof = {k: v for k, v in e.profile_get().items() if v["launches"]}
            e.profile_enable(False)
            tot = sum(v["ms"] for v in prof.values())
            best, med = min(ms[i]), sorted(ms[i])[len(ms[i]) // 2]
            run = dict(config=name, captions=n, ms_median=med, ms_min=best, ms_max=max(ms[i]),
                       gflop_per_caption=flop / 1e9, tflops=flop * n / (med * 1e-3) / 1e12,
                       attention_share=prof.get("attn_mapper", {}).get("ms", 0.0) / tot if tot else None,
                       families={k: dict(ms_per_call=v["ms"] / 3, launches_per_call=v["launches"] / 3) for k, v in prof.items()})
            result["runs"].append(run)
            print(f"{n:5d} captions  {name:32s} {med:8.3f} ms (min {best:.3f} max {max(ms[i]):.3f})  "
                  f"{flop / 1e9:.3f} GFLOP/caption  {run['tflops']:6.1f} TFLOP/s  attention "
                  f"{100 * (run['attention_share'] or 0):.1f} % of the kernel time", flush=True)
    for e in engines:
        e.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"bench_mapper": [{k: r[k] for k in ("config", "captions", "ms_median", "tflops", "attention_share")}
                                       for r in result["runs"]]}))


if __name__ == "__main__":
    main()
