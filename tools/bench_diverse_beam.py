#!/usr/bin/env python
"""Time the diverse (group) beam search beside the plain beam decode of the same width, in one process: capdec_decode_beam
with beam 6, capdec_decode_beam_groups with beam 6 in one group (the same results through the group kernels) and in three
groups with diversity penalty 0.5, alternating inside every round.  Device events around whole calls after a warm-up of every
variant; then one profiled call per variant for the per-family split (capdec_profile_get).

    python tools/bench_diverse_beam.py [--captions 625] [--entry-length 67] [--rounds 5] [--out profiles/diverse_beam_bench.txt]

Workload: P 10 prefix rows per caption (Gaussian rows with the norm of wte rows), GPT-2-small geometry, hot synthetic
weights (they never emit the stop id: every caption runs all steps), the default GEMM mode.  Only the two bookkeeping
kernels differ between the calls (group_beam_init_kernel / group_beam_step_kernel for beam_init_kernel / beam_step_kernel,
one launch per step either way, timed in the `select` family) -- and the trajectories: other tokens are fed, and other
ancestor tables reach the decode attention.  Needs an MI355X."""
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
    ap.add_argument("--captions", type=int, default=625)
    ap.add_argument("--entry-length", type=int, default=67)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--beam", type=int, default=6)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--penalty", type=float, default=0.5)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from capdec_amd import synth
    from capdec_amd.engine import Engine
    assert torch.cuda.is_available(), "bench_diverse_beam needs an MI355X"
    dims = synth.GPT2_SMALL
    V, d, T, n, B, G, lam = dims.vocab, dims.n_embd, args.entry_length, args.captions, args.beam, args.groups, args.penalty
    sd = synth.hot_gpt2_state_dict(42, dims)
    g = torch.Generator().manual_seed(1)
    prefix = (torch.randn(n, P, d, generator=g) * 0.15).cuda()
    e = Engine(0)
    e.load_gpt2(sd, n_head=dims.n_head)
    stop = V + 5
    variants = {
        f"beam {B}": lambda: e.decode_beam(prefix, stop, B, T),
        f"groups {B}/1": lambda: e.decode_beam_groups(prefix, stop, B, 1, lam, T),
        f"groups {B}/{G} lambda {lam:g}": lambda: e.decode_beam_groups(prefix, stop, B, G, lam, T),
    }
    names = list(variants)
    out = {k: [t.cpu().numpy() for t in fn()] for k, fn in variants.items()}          # warm-up: every shape of the timed window
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
    fam, kvs = {}, {}
    for k in names:
        e.profile_reset()
        e.profile_enable(True)
        variants[k]()
        e.synchronize()
        fam[k] = {f: v for f, v in e.profile_get().items() if v["launches"]}
        e.profile_enable(False)
        kvs[k] = e.decode_counters()
    e.close()

    def distinct(ids, lens):
        return float(np.mean([len({tuple(ids[r, b, :int(lens[r, b])]) for b in range(ids.shape[1])}) for r in range(ids.shape[0])]))

    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    base = med[names[0]]
    same_g1 = all(np.array_equal(a, b) for a, b in zip(out[names[1]][:4], out[names[0]]))
    lines = ["Diverse (group) beam search beside the plain beam decode -- tools/bench_diverse_beam.py", "",
             f"Workload: {n} captions, P {P}, entry_length {T} (no caption stops: {T - 1} decode steps after the prefill), "
             f"{n * B} rows per step,",
             f"GPT-2-small geometry (V {V}), hot synthetic weights, default GEMM mode.  Device events around whole calls, "
             f"{args.rounds} rounds,",
             "the variants alternating; medians.", ""]
    result = {}
    for k in names:
        m = med[k]
        dis = distinct(out[k][0], out[k][1])
        lines.append(f"    {k:26s} {m:10.2f} ms per call (min {min(ms[k]):.2f}, max {max(ms[k]):.2f})  {m / T:8.3f} ms per step  "
                     f"{n / (m * 1e-3):9.1f} captions/s  ratio to {names[0]} {m / base:6.3f}  distinct sequences per caption "
                     f"{dis:.2f} of {B}")
        result[k] = dict(ms_median=m, ms_per_step=m / T, ratio=m / base, distinct_per_caption=dis)
    lines += ["", f"groups {B}/1 returns the ids, lengths, scores and order of beam {B} bit for bit: {same_g1}", ""]
    for k in names:
        kv = kvs[k]
        lines.append(f"per family, one profiled call of {k} (ms, launches); distinct K/V slots per attended position "
                     f"{kv.get('kv_slots_per_position', float('nan')):.3f}:")
        for f, v in sorted(fam[k].items(), key=lambda kv_: -kv_[1]["ms"]):
            lines.append(f"    {f:26s} {v['ms']:10.3f} {v['launches']:7d}")
    lines.append("")
    for k in names[1:]:
        delta = {f: fam[k].get(f, {"ms": 0.0})["ms"] - fam[names[0]].get(f, {"ms": 0.0})["ms"] for f in set(fam[k]) | set(fam[names[0]])}
        top = sorted(delta.items(), key=lambda kv_: -abs(kv_[1]))[:3]
        lines.append(f"{k} against {names[0]}: {med[k] - base:+.2f} ms per call; per family (profiled calls) "
                     + ", ".join(f"{f} {v:+.2f} ms" for f, v in top)
                     + f"; `select` is {fam[names[0]]['select']['ms']:.2f} ms of the plain call")
    lines += ["",
              "Where a difference exceeds the `select` family's own share it is not the bookkeeping: groups that are pushed apart share",
              "less history, so the decode attention reads more distinct K/V slots per attended position (the statistic above; 1 =",
              "the beams share their whole history, beam = nothing) and its time grows with that traffic, as attention.hip's",
              "converged / diverged phases do for any beam decode whose hypotheses diverge.",
              "The bookkeeping kernels (beam_init / beam_step, group_beam_init / group_beam_step) are timed in the `select` family,",
              "next to the top-k merge and the finalize; everything else runs the same launches on other tokens and ancestor tables.",
              "Measured: the above, one process, one MI355X.  Not measured: other widths and group counts, captions that stop, logits",
              "processors together with groups, HBM traffic counters."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench_diverse_beam": result}))


if __name__ == "__main__":
    main()
