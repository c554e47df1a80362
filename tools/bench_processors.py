#!/usr/bin/env python
"""Time the decode with logits processors beside the same call without them, in one process: greedy and beam 5 at 5000 and
625 captions, three variants alternating inside every round -- no processor (the fused lm_head + selection), repetition
penalty 1.3 + no-repeat bigrams + minimum length 4 (materialised logits, logits_process_kernel, logits_select_kernel), and the
same plus a logit bias (one more pass over the logits).  Device events around whole calls after a warm-up of every
(call, variant); then one profiled call per (call, variant) for the per-family split (capdec_profile_get).

    python tools/bench_processors.py [--captions 5000,625] [--entry-length 67] [--rounds 3] [--out profiles/processors_bench.txt]

Workload: P 10 prefix rows per caption (Gaussian rows with the norm of wte rows), GPT-2-small geometry, hot synthetic
weights (they never emit the stop id: every caption runs all steps), the default GEMM mode.  Bytes from the shapes: the fp32
logits of one step are rows x ld x 4 bytes (ld = 50304): 5.03 GB for the 25 000 rows of beam 5 at 5000 captions.  A processed
step writes them once (the lm_head GEMM) and reads them once (the selection): 10.06 GB of traffic; the bias pass reads and
writes them once more: 20.1 GB.  Needs an MI355X."""
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
    ap.add_argument("--captions", default="5000,625")
    ap.add_argument("--entry-length", type=int, default=67)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from capdec_amd import synth
    from capdec_amd.engine import Engine
    assert torch.cuda.is_available(), "bench_processors needs an MI355X"
    dims = synth.GPT2_SMALL
    V, d, T = dims.vocab, dims.n_embd, args.entry_length
    sizes = [int(s) for s in args.captions.split(",")]
    ld = (V + 63) // 64 * 64
    sd = synth.hot_gpt2_state_dict(42, dims)
    g = torch.Generator().manual_seed(1)
    prefix = (torch.randn(max(sizes), P, d, generator=g) * 0.15).cuda()
    e = Engine(0)
    e.load_gpt2(sd, n_head=dims.n_head)
    stop = V + 5
    proc = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=4)
    variants = {"plain": {}, "processors": proc, "processors+bias": dict(proc, logit_bias=np.zeros(V, dtype=np.float32))}
    calls = {}
    for n in sizes:
        calls[f"greedy {n}"] = (n, 1, lambda kw, n=n: e.decode_greedy(prefix[:n], stop, T, -1, **kw))
        calls[f"beam5 {n}"] = (n, 5, lambda kw, n=n: e.decode_beam(prefix[:n], stop, 5, T, **kw))

    out_ids = {}
    for cname, (n, beam, fn) in calls.items():                 # warm-up: every shape of the timed window
        for vname, kw in variants.items():
            out_ids[cname, vname] = fn(kw)[0].cpu().numpy()
    torch.cuda.synchronize()
    ms = {k: [] for k in out_ids}
    for _ in range(args.rounds):
        for cname, (n, beam, fn) in calls.items():
            for vname, kw in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn(kw)
                b.record()
                b.synchronize()
                ms[cname, vname].append(a.elapsed_time(b))
    fam = {}
    for cname, (n, beam, fn) in calls.items():
        for vname, kw in variants.items():
            e.profile_reset()
            e.profile_enable(True)
            fn(kw)
            e.synchronize()
            fam[cname, vname] = {k: v for k, v in e.profile_get().items() if v["launches"]}
            e.profile_enable(False)
    e.close()

    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    lines = ["Decode with logits processors beside the same call without them -- tools/bench_processors.py", "",
             f"Workload: P {P}, entry_length {T} (no caption stops: {T - 1} decode steps after the prefill), GPT-2-small geometry "
             f"(V {V}, rows padded to {ld}),",
             "hot synthetic weights, default GEMM mode, CAPDEC_SAMPLE_ROWS rows of logits materialised at a time (default 2048).",
             f"Variants: plain = no processor (fused lm_head + selection); processors = repetition_penalty 1.3, "
             f"no_repeat_ngram_size 2, min_length 4;",
             f"processors+bias = the same plus an all-zero logit bias.  Device events around whole calls, {args.rounds} rounds, "
             f"the variants alternating; medians.", ""]
    result = {}
    for cname, (n, beam, fn) in calls.items():
        rows = n * beam
        gb = rows * ld * 4 / 1e9
        base = med[cname, "plain"]
        lines.append(f"{cname}: {rows} rows per step; logits of one step {gb:.2f} GB (written once, read once; the bias pass reads "
                     f"and writes them once more)")
        for vname in variants:
            m = med[cname, vname]
            changed = int((out_ids[cname, vname] != out_ids[cname, "plain"]).reshape(n, -1).any(axis=1).sum())
            lines.append(f"    {vname:16s} {m:10.2f} ms per call (min {min(ms[cname, vname]):.2f}, max {max(ms[cname, vname]):.2f})  "
                         f"{m / T:8.3f} ms per step  {n / (m * 1e-3):9.1f} captions/s  ratio to plain {m / base:5.2f}  "
                         f"captions changed {changed} of {n}")
            result[f"{cname} / {vname}"] = dict(ms_median=m, ms_per_step=m / T, ratio_to_plain=m / base, captions_changed=changed)
        lines.append("")
    for cname in calls:
        for vname in variants:
            lines.append(f"per family, one profiled call of {cname} / {vname} (ms, launches):")
            for k, v in sorted(fam[cname, vname].items(), key=lambda kv: -kv[1]["ms"]):
                lines.append(f"    {k:26s} {v['ms']:10.3f} {v['launches']:7d}")
    lines += ["",
              "The processors' kernels (logits_process_kernel, logits_select_kernel) are timed in the `select` family; the plain",
              "lm_head GEMM that materialises the logits appears under its GEMM family instead of the fused *_lmhead_topk one.",
              "Measured: the above, one process, one MI355X.  Not measured: other GEMM modes, other CAPDEC_SAMPLE_ROWS, captions that",
              "stop, the sampling decode with top_k, HBM traffic counters."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench_processors": result}))


if __name__ == "__main__":
    main()
