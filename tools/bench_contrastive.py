#!/usr/bin/env python
"""Time the contrastive search beside the beam decode of the same width and the greedy decode, in one process: the engine
calls behind generate2_batch (capdec_decode_greedy), generate_beam_batch at beam K (capdec_decode_beam) and
generate_contrastive_batch (capdec_decode_contrastive with top_k K), alternating inside every round, at every caption
count given.  Device events around whole calls after a warm-up of every variant; then one profiled contrastive call for the
per-family split (capdec_profile_get) and the selection kernel's share of it (family `contrastive_select`).

    python tools/bench_contrastive.py [--captions 625 5000] [--entry-length 67] [--top-k 4] [--alpha 0.6] [--rounds 5]
                                      [--out profiles/contrastive_bench.txt]

Workload: P 10 prefix rows per caption (Gaussian rows with the norm of wte rows), GPT-2-small geometry, hot synthetic
weights (they never emit the stop id: every caption runs all steps), the default GEMM mode.  A contrastive call pushes K
rows per caption through the body like the beam call, one position more (T body steps after the prefill where beam and
greedy run T - 1), but its lm_head sees one row per caption like greedy's.  Needs an MI355X."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

P = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captions", type=int, nargs="+", default=[625, 5000])
    ap.add_argument("--entry-length", type=int, default=67)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--top-k", type=int, default=4)
    ap.add_argument("--alpha", type=float, default=0.6)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from capdec_amd import synth
    from capdec_amd.engine import Engine
    assert torch.cuda.is_available(), "bench_contrastive needs an MI355X"
    dims = synth.GPT2_SMALL
    V, d, T, K, alpha = dims.vocab, dims.n_embd, args.entry_length, args.top_k, args.alpha
    sd = synth.hot_gpt2_state_dict(42, dims)
    e = Engine(0)
    e.load_gpt2(sd, n_head=dims.n_head)
    stop = V + 5
    lines = ["Contrastive search beside the beam and the greedy decode -- tools/bench_contrastive.py", "",
             f"Workload: P {P}, entry_length {T} (no caption stops), top_k = beam = {K}, penalty_alpha {alpha:g}, GPT-2-small "
             f"geometry (V {V}),",
             f"hot synthetic weights, default GEMM mode.  Device events around whole calls, {args.rounds} rounds, the variants "
             "alternating; medians.", ""]
    result = {}
    for n in args.captions:
        g = torch.Generator().manual_seed(1)
        prefix = (torch.randn(n, P, d, generator=g) * 0.15).cuda()
        variants = {
            "greedy": lambda: e.decode_greedy(prefix, stop, T, -1),
            f"beam {K}": lambda: e.decode_beam(prefix, stop, K, T),
            f"contrastive {K}": lambda: e.decode_contrastive(prefix, K, alpha, stop, -1, T, True),
        }
        names = list(variants)
        out = {k: [t.cpu().numpy() for t in fn()] for k, fn in variants.items()}      # warm-up: every shape of the timed window
        torch.cuda.synchronize()
        ms = {k: [] for k in names}
        for _ in range(args.rounds):
            for k in names:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                variants[k]()
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b))
        e.profile_reset()
        e.profile_enable(True)
        variants[names[2]]()
        e.synchronize()
        fam = {f: v for f, v in e.profile_get().items() if v["launches"]}
        e.profile_enable(False)
        chunks = e.decode_chunks()
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        ci, cl, tr = out[names[2]]
        gi, gl = out["greedy"]
        distinct = lambda ids, lens: float(np.mean([len(set(ids[r, :lens[r]].tolist())) for r in range(ids.shape[0])]))
        total = sum(v["ms"] for v in fam.values())
        sel = fam.get("contrastive_select", {"ms": 0.0, "launches": 0})
        lines.append(f"{n} captions ({n * K} candidate rows per step, {chunks} chunk(s)):")
        for k in names:
            m = med[k]
            lines.append(f"    {k:16s} {m:10.2f} ms per call (min {min(ms[k]):.2f}, max {max(ms[k]):.2f})  {n / (m * 1e-3):9.1f} "
                         f"captions/s  ratio to greedy {m / med['greedy']:6.3f}")
        lines.append(f"    distinct tokens per caption: contrastive {distinct(ci, cl):.2f}, greedy {distinct(gi, gl):.2f} of {T}; "
                     f"mean max-cosine of the chosen candidates {float(tr[..., 1].mean()):.3f}")
        lines.append(f"    one profiled contrastive call: {total:.2f} ms in kernels; contrastive_select {sel['ms']:.3f} ms in "
                     f"{sel['launches']} launches = {100.0 * sel['ms'] / max(total, 1e-9):.2f} % (prefill history + {T} selections)")
        for f, v in sorted(fam.items(), key=lambda kv_: -kv_[1]["ms"]):
            lines.append(f"        {f:26s} {v['ms']:10.3f} {v['launches']:7d}")
        lines.append("")
        result[str(n)] = dict({k: dict(ms_median=med[k], captions_per_s=n / (med[k] * 1e-3)) for k in names},
                              select_ms=sel["ms"], select_share=sel["ms"] / max(total, 1e-9), kernels_ms=total, chunks=chunks)
    e.close()
    lines += ["Measured: the above, one process, one MI355X.  Not measured: other top_k, captions that stop, logits processors,",
              "contexts beyond 77 positions (the history read of a selection grows with the position), HBM traffic counters."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench_contrastive": result}))


if __name__ == "__main__":
    main()
