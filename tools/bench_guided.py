#!/usr/bin/env python
"""Time the guided decode (classifier-free guidance, capdec_decode_guided) beside the plain greedy and beam decodes, in one
process on one engine: decode_guided at guidance_scale gamma (beam 1 and beam B), decode_greedy, decode_beam at beam B, and
the two plain calls with one logits processor set (min_length 1), which puts them on the materialised-logits route the
guided decode always takes.  The engine's timer (device events around the call) after one warm-up call of every variant,
the variants alternating inside every round; then one profiled guided call per beam width for the per-family split
(capdec_profile_get) and the share of the combine and mirror kernels (family `guided`).

    python tools/bench_guided.py [--captions 625] [--entry-length 67] [--beam 5] [--gamma 1.5] [--rounds 5]
                                 [--out profiles/guided_bench.txt]

Workload: the headline one -- P 10, GPT-2-small geometry, hot synthetic weights (no caption stops), prefixes from the
8-layer TransformerMapper for synthetic CLIP embeddings, the negative prefix the mapper's output for the all-zero
embedding (one for all captions), default GEMM mode.  Needs an MI355X."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

P = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captions", type=int, nargs="+", default=[625])
    ap.add_argument("--entry-length", type=int, default=67)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--gamma", type=float, default=1.5)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from capdec_amd import synth
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    assert torch.cuda.is_available(), "bench_guided needs an MI355X"
    T, B, gamma = args.entry_length, args.beam, args.gamma
    model = ClipCaptionModel(P, clip_length=10, prefix_dim=512, num_layers=8,
                             mapping_type=MappingType.TransformerEncoder).to("cuda:0").eval()
    model.load_state_dict(synth.hot_state_dict(42, "transformer_encoder", 512, P))
    e = model.engine
    stop = 13
    lines = ["Guided decode (classifier-free guidance) beside the plain greedy and beam decodes -- tools/bench_guided.py", "",
             f"Workload: P {P}, entry_length {T}, guidance_scale {gamma:g}, beam {B}, GPT-2-small geometry, hot synthetic weights, "
             "TransformerMapper",
             "prefixes, negative prefix = the mapper's output for the zero embedding (one for all), default GEMM mode.  The "
             f"engine's timer around whole calls, {args.rounds}",
             "rounds, the variants alternating; medians.  'proc' = the plain call with min_length 1 set: the materialised-logits "
             "route.", ""]
    result = {}
    for n in args.captions:
        emb = synth.synthetic_clip_embeddings(n, 512, seed=0).to("cuda:0")
        prefix = model.clip_project(emb).reshape(n, P, -1).contiguous()
        neg = model.clip_project(torch.zeros(1, 512, device="cuda:0")).reshape(1, P, -1).contiguous()
        variants = {
            "greedy": lambda: e.decode_greedy(prefix, stop, T, -1),
            "greedy proc": lambda: e.decode_greedy(prefix, stop, T, -1, min_length=1),
            "guided greedy": lambda: e.decode_guided(prefix, neg, gamma, stop, 1, T, 1.0, -1),
            f"beam {B}": lambda: e.decode_beam(prefix, stop, B, T),
            f"beam {B} proc": lambda: e.decode_beam(prefix, stop, B, T, min_length=1),
            f"guided beam {B}": lambda: e.decode_guided(prefix, neg, gamma, stop, B, T),
        }
        names = list(variants)
        out = {k: [t.cpu() for t in fn()] for k, fn in variants.items()}       # warm-up: every shape of the timed window
        torch.cuda.synchronize()
        ms = {k: [] for k in names}
        for _ in range(args.rounds):
            for k in names:
                e._sync_stream()
                e.timer_start()
                variants[k]()
                ms[k].append(e.timer_stop_ms())
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        lens = {k: float(out[k][1].float().mean()) for k in names}
        differ = int((out["guided greedy"][0] != out["greedy"][0]).any(dim=1).sum())
        lines.append(f"{n} captions (mean emitted length: greedy {lens['greedy']:.1f}, guided greedy {lens['guided greedy']:.1f}; "
                     f"{differ} of {n} guided greedy captions differ from the plain ones):")
        for k in names:
            m = med[k]
            lines.append(f"    {k:16s} {m:10.2f} ms per call (min {min(ms[k]):.2f}, max {max(ms[k]):.2f})  {n / (m * 1e-3):9.1f} captions/s")
        ratios = {}
        for gk, plain in (("guided greedy", "greedy"), (f"guided beam {B}", f"beam {B}")):
            ratios[gk] = (med[gk] / med[plain], med[gk] / med[plain + " proc"])
            lines.append(f"    {gk} / {plain}: {ratios[gk][0]:.3f}; / {plain} proc: {ratios[gk][1]:.3f}")
        prof = {}
        for gk in ("guided greedy", f"guided beam {B}"):
            e.profile_reset()
            e.profile_enable(True)
            variants[gk]()
            e.synchronize()
            fam = {f: v for f, v in e.profile_get().items() if v["launches"]}
            e.profile_enable(False)
            total = sum(v["ms"] for v in fam.values())
            g = fam.get("guided", {"ms": 0.0, "launches": 0})
            prof[gk] = dict(kernels_ms=total, guided_ms=g["ms"], guided_share=g["ms"] / max(total, 1e-9))
            lines.append(f"    one profiled {gk} call: {total:.2f} ms in kernels; guided (combine + mirror) {g['ms']:.3f} ms in "
                         f"{g['launches']} launches = {100.0 * g['ms'] / max(total, 1e-9):.2f} %; rows per step "
                         f"{e.decode_step_rows()[0]}, {e.decode_chunks()} chunk(s)")
            for f, v in sorted(fam.items(), key=lambda kv_: -kv_[1]["ms"]):
                lines.append(f"        {f:26s} {v['ms']:10.3f} {v['launches']:7d}")
        lines.append("")
        result[str(n)] = dict({k: dict(ms_median=med[k], captions_per_s=n / (med[k] * 1e-3)) for k in names},
                              ratios={k: dict(plain=a, plain_proc=b) for k, (a, b) in ratios.items()}, profile=prof)
    lines += ["Measured: the above, one process, one MI355X.  Not measured: per-caption negatives (the same launches), captions "
              "that stop,", "other beam widths, the bf16 mode, HBM traffic counters."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench_guided": result}))


if __name__ == "__main__":
    main()
