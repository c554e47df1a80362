#!/usr/bin/env python
"""Time the lexically constrained beam search beside the plain beam decode on the same logits route, in one process:
capdec_decode_beam with an all-zero logit_bias (which sends it through the materialised logits, the route the constrained
call always takes) -- the yardstick, run TWICE per round so that its own repeat gives the run-to-run noise -- and
capdec_decode_beam_constrained with 0 phrases and the same bias, then with 0, 1 and 4 phrases per caption, alternating
inside every round.  Device events around whole calls after a warm-up of every variant; then one profiled call per variant
for the per-family split (capdec_profile_get).

    python tools/bench_constrained.py [--captions 625 5000] [--entry-length 67] [--rounds 3] [--out profiles/constrained_bench.txt]

Workload: P 10 prefix rows per caption (Gaussian rows with the norm of wte rows), GPT-2-small geometry, hot synthetic
weights, beam 5, a stop id outside the vocabulary (every caption runs all steps), the default GEMM mode.  Phrases: two
random tokens each, drawn once.  Between the yardstick and the 0-phrase call with the same zero bias only the
selection kernel (logits_select_forced_kernel for logits_select_kernel) and the bookkeeping kernels (constrained_beam_*
for beam_init / beam_step; beam_finalize_kernel ends both) differ, all timed in the `select` family; without the bias the constrained call also saves the
processors' pass over the logits; with phrases the trajectories differ too.  Needs an MI355X."""
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from capdec_amd import synth
    from capdec_amd.engine import Engine
    assert torch.cuda.is_available(), "bench_constrained needs an MI355X"
    dims = synth.GPT2_SMALL
    V, d, T, B = dims.vocab, dims.n_embd, args.entry_length, args.beam
    sd = synth.hot_gpt2_state_dict(42, dims)
    e = Engine(0)
    e.load_gpt2(sd, n_head=dims.n_head)
    stop = V + 5
    zero = np.zeros(V, dtype=np.float32)
    lines = ["Lexically constrained beam search beside the plain beam decode on the same logits route -- tools/bench_constrained.py", ""]
    result = {}
    for n in args.captions:
        g = torch.Generator().manual_seed(1)
        prefix = (torch.randn(n, P, d, generator=g) * 0.15).cuda()
        rng = np.random.default_rng(3)

        def table(k):
            t = np.full((n, 4, 4), -1, dtype=np.int32)
            t[:, :k, :2] = rng.integers(0, V, size=(n, k, 2))
            return t

        tabs = {k: table(k) for k in (0, 1, 4)}
        variants = {"beam, zero bias (yardstick)": lambda: e.decode_beam(prefix, stop, B, T, logit_bias=zero),
                    "beam, zero bias (again)": lambda: e.decode_beam(prefix, stop, B, T, logit_bias=zero)}
        variants["constrained, 0 phrases, zero bias"] = lambda: e.decode_beam_constrained(prefix, tabs[0], stop, B, T, logit_bias=zero)
        for k in (0, 1, 4):
            variants[f"constrained, {k} phrases"] = lambda k=k: e.decode_beam_constrained(prefix, tabs[k], stop, B, T)
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
        fam = {}
        for k in names[1:]:
            e.profile_reset()
            e.profile_enable(True)
            variants[k]()
            e.synchronize()
            fam[k] = {f: v for f, v in e.profile_get().items() if v["launches"]}
            e.profile_enable(False)
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        base = med[names[0]]
        noise = abs(med[names[1]] - base) / base
        spread = max((max(ms[k]) - min(ms[k])) / base for k in names[:2])
        same0 = all(np.array_equal(a, b) for k in names[2:4] for a, b in zip(out[k][:4], out[names[0]]))
        full = {k: float((out[f"constrained, {k} phrases"][4][:, 0] == (1 << k) - 1).mean()) for k in (1, 4)}
        lines += [f"Workload: {n} captions, beam {B}, P {P}, entry_length {T} (no caption stops: {T - 1} decode steps after the "
                  f"prefill), {n * B} rows per step,",
                  f"GPT-2-small geometry (V {V}), hot synthetic weights, default GEMM mode.  Device events around whole calls, "
                  f"{args.rounds} rounds,", "the variants alternating; medians.", ""]
        for k in names:
            m = med[k]
            lines.append(f"    {k:34s} {m:10.2f} ms per call (min {min(ms[k]):.2f}, max {max(ms[k]):.2f})  {m / T:8.3f} ms per step  "
                         f"{n / (m * 1e-3):9.1f} captions/s  ratio to the yardstick {m / base:6.3f}")
            result[f"{n}: {k}"] = dict(ms_median=m, ratio=m / base)
        lines += ["", f"run-to-run noise of the yardstick: its two medians differ by {noise * 100:.2f} %; largest (max - min) / median of "
                      f"either {spread * 100:.2f} %",
                  f"0 phrases, with and without the zero bias, returns the ids, lengths, scores and order of the yardstick bit for bit: "
                  f"{same0}",
                  f"best row holds every phrase: 1 phrase {full[1] * 100:.1f} % of the captions, 4 phrases {full[4] * 100:.1f} % "
                  f"(8 forced tokens in {T})", ""]
        for k in names[1:]:
            lines.append(f"per family, one profiled call of {k} (ms, launches):")
            for f, v in sorted(fam[k].items(), key=lambda kv_: -kv_[1]["ms"]):
                lines.append(f"    {f:26s} {v['ms']:10.3f} {v['launches']:7d}")
        lines.append("")
        ref = fam[names[1]]
        for k in names[2:]:
            delta = {f: fam[k].get(f, {"ms": 0.0})["ms"] - ref.get(f, {"ms": 0.0})["ms"] for f in set(fam[k]) | set(ref)}
            top = sorted(delta.items(), key=lambda kv_: -abs(kv_[1]))[:3]
            lines.append(f"{k} against the yardstick: {med[k] - base:+.2f} ms per call ({(med[k] / base - 1) * 100:+.2f} %); per family "
                         f"(profiled calls) " + ", ".join(f"{f} {v:+.2f} ms" for f, v in top)
                         + f"; `select` is {ref['select']['ms']:.2f} ms of the yardstick's call")
        lines += ["", ""]
    e.close()
    lines += ["The selection kernel, the bookkeeping kernels and the finalize are timed in the `select` family, next to the logits",
              "processors.  `constrained, 0 phrases, zero bias` is the like-for-like comparison: the yardstick's launches with",
              "logits_select_forced_kernel and constrained_beam_* in the place of logits_select_kernel and beam_init / beam_step",
              "(beam_finalize_kernel ends both).  The constrained calls WITHOUT the bias are faster than the yardstick by what the",
              "yardstick pays for being forced onto this route: logits_process_kernel reads and writes every logits row once more to",
              "add the zero bias, a pass the constrained call does not need (the `select` deltas above).  With phrases the other",
              "families run the same launches on other tokens and ancestor tables: the banks keep hypotheses that the plain beam",
              "would drop, and the decode attention's time grows (the `attn_decode` deltas above) as it does for any beam decode",
              "whose hypotheses share less history; the K/V-slot statistic that would show this was not read here.",
              "Measured: the above, one process, one MI355X.  Not measured: other widths, captions that stop, processors together",
              "with phrases, HBM traffic counters."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench_constrained": result}))


if __name__ == "__main__":
    main()
