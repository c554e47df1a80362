#!/usr/bin/env python
"""Time the nucleus-sampling decode (``capdec_decode_sample``) beside the greedy decode it shares its loop with: device
events around whole calls after warm-up, the configurations alternating inside every round, then one profiled pass per
configuration for the per-family split (capdec_profile_get).  Workload: TransformerMapper(8) prefixes, P 10, T 67,
GPT-2-small geometry, synthetic weights (nothing stops: every caption runs all 67 steps).

    python tools/bench_sample.py [--captions 5000 625] [--rounds 3] [--reps 2] [--modes greedy sample ...] [--out FILE.json]

Modes: ``greedy``; ``sample`` (temperature 0.7, top_p 0.8, device Philox); ``sample_p1`` (temperature 1, top_p 1: no
nucleus search); ``sample_t1`` (temperature 1, top_p 0.8: the widest nuclei).  ``--tree DIR`` imports ``capdec_amd`` from
another checkout with its own built library (greedy across two commits: run the two trees alternately, one process
each).  Bytes the sampling path adds per decode step, from the shapes: rows x ld x 4 written by the lm_head GEMM and read
once by ``sample_top_p_kernel`` (ld = the vocabulary rounded up to 64).  Needs an MI355X."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

D, P, C, T = 512, 10, 10, 67
MODES = {"greedy": None, "sample": (0.7, 0.8), "sample_p1": (1.0, 1.0), "sample_t1": (1.0, 0.8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captions", type=int, nargs="*", default=[5000, 625])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--modes", nargs="*", default=["greedy", "sample"], choices=sorted(MODES))
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from capdec_amd import synth
    from capdec_amd.engine import Engine
    assert torch.cuda.is_available(), "bench_sample needs an MI355X"
    dims = synth.GPT2_SMALL
    sd = synth.hot_state_dict(42, "transformer_encoder", D, P, C, 8, dims)
    e = Engine(0)
    e.load_gpt2(sd, n_head=dims.n_head)
    e.load_mapper_transformer(sd)
    ld = (dims.vocab + 63) // 64 * 64
    stop = dims.vocab + 5                                   # never drawn: every caption runs T steps

    def call(mode, prefix, seed):
        if MODES[mode] is None:
            return e.decode_greedy(prefix, stop, T, -1)
        t, p = MODES[mode]
        return e.decode_sample(prefix, stop, T, t, p, seed=seed, alt_stop_id=-1)

    result = {"tree": os.path.abspath(args.tree), "shape": dict(D=D, P=P, T=T, vocab=dims.vocab, ld=ld), "rounds": args.rounds,
              "reps": args.reps, "runs": []}
    for n in args.captions:
        prefix = e.mapper_forward(synth.synthetic_clip_embeddings(n, D, seed=1).cuda())
        for m in args.modes:                                # warm-up: buffers, weight planes, code objects
            call(m, prefix, 0)
        torch.cuda.synchronize()
        ms = {m: [] for m in args.modes}
        for r in range(args.rounds):
            for m in args.modes:                            # alternating: every round times every mode
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for k in range(args.reps):
                    ids, lens = call(m, prefix, 1 + r * args.reps + k)
                b.record()
                b.synchronize()
                assert int(lens.min()) == T
                ms[m].append(a.elapsed_time(b) / args.reps)
        for m in args.modes:
            med = sorted(ms[m])[len(ms[m]) // 2]
            run = dict(mode=m, captions=n, ms_median=med, ms_min=min(ms[m]), ms_max=max(ms[m]), captions_per_s=n / (med * 1e-3),
                       logits_gb_per_step=(2.0 * n * ld * 4 / 1e9) if MODES[m] else 0.0)
            if not args.no_profile:
                e.profile_reset()
                e.profile_enable(True)
                call(m, prefix, 99)
                e.synchronize()
                prof = {k: v for k, v in e.profile_get().items() if v["launches"]}
                e.profile_enable(False)
                run["families"] = {k: dict(ms_per_call=v["ms"], launches_per_call=v["launches"]) for k, v in prof.items()}
            result["runs"].append(run)
            print(f"{n:5d} captions  {m:10s} {med:9.2f} ms (min {min(ms[m]):.2f} max {max(ms[m]):.2f})  "
                  f"{run['captions_per_s']:8.1f} captions/s", flush=True)
        if "greedy" in args.modes:
            g = next(r for r in result["runs"] if r["captions"] == n and r["mode"] == "greedy")
            for r in result["runs"]:
                if r["captions"] == n and r["mode"] != "greedy":
                    r["ratio_to_greedy"] = r["ms_median"] / g["ms_median"]
                    print(f"{n:5d} captions  {r['mode']} / greedy = {r['ratio_to_greedy']:.3f}", flush=True)
    e.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"bench_sample": [{k: r.get(k) for k in ("mode", "captions", "ms_median", "captions_per_s", "ratio_to_greedy")}
                                       for r in result["runs"]]}))


if __name__ == "__main__":
    main()
