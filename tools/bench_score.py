#!/usr/bin/env python
"""Time scoring given captions (``capdec_score``) beside the path that existed before it, in one process: the materialised
logits of ``capdec_gpt2_logits(all_positions)`` followed by ``capdec_cross_entropy`` (what ``train.validation_loss`` does per
batch), over the same captions in blocks that fit.  Device events around whole passes after a warm-up, the two paths
alternating inside every round; then one profiled pass per path for the per-family split (capdec_profile_get), and the
device memory each path takes, in a fresh context each.

    python tools/bench_score.py [--captions 5000] [--block 256] [--rounds 3] [--out profiles/score_bench.txt]

Workload: P 10 prefix rows per caption (Gaussian rows with the norm of wte rows: the timing does not depend on their
values), caption lengths uniform in 8..20, GPT-2-small geometry, hot synthetic weights, the default GEMM mode.  The
materialised path pads every caption to 20 tokens, label 0 = ignored.  Bytes from the shapes: the materialised path writes
and reads (P + 20) x V x 4 bytes of logits per caption (6.03 MB at V 50257); scoring reads ~6 KB per scored row in
label_logit_kernel on top of the fused head's per-tile partials.  Needs an MI355X."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

P, LMIN, LMAX = 10, 8, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captions", type=int, default=5000)
    ap.add_argument("--block", type=int, default=256, help="captions per block of the materialised path (256 x 30 x V x 4 = 1.5 GB)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from capdec_amd import synth
    from capdec_amd.engine import Engine
    assert torch.cuda.is_available(), "bench_score needs an MI355X"
    dims = synth.GPT2_SMALL
    V, d, n = dims.vocab, dims.n_embd, args.captions
    sd = synth.hot_gpt2_state_dict(42, dims)
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(LMIN, LMAX + 1, (n,), generator=g)
    tokens = torch.randint(1, V, (n, LMAX), generator=g, dtype=torch.int64)
    tokens[torch.arange(LMAX)[None, :] >= lens[:, None]] = 0                  # right padding, like the train dataset
    prefix = (torch.randn(n, P, d, generator=g) * 0.15).cuda()
    tok_dev, lens_host = tokens.to(torch.int32).cuda(), lens.numpy()
    n_tok = int(lens.sum())

    def new_engine():
        e = Engine(0)
        e.load_gpt2(sd, n_head=dims.n_head)
        return e

    def run_score(e):
        _, s, c = e.score(prefix, tok_dev, lens_host, ignore_id=-1)
        return s, c

    def run_materialised(e):
        total = torch.zeros((), device="cuda", dtype=torch.float64)
        for b0 in range(0, n, args.block):
            t = tok_dev[b0:b0 + args.block]
            embeds = torch.cat((prefix[b0:b0 + args.block], e.wte(t)), dim=1)
            logits = e.gpt2_logits(embeds, all_positions=True)
            loss = e.cross_entropy(logits[:, P - 1:-1], t, ignore_index=0)    # the block's mean over its real tokens
            total += loss.double() * int(lens[b0:b0 + args.block].sum())
        return total

    paths = {"score": run_score, "materialised": run_materialised}
    # ---- memory: a fresh context per path; what the device lost (library workspaces + torch's allocator) over one pass
    mem = {}
    for name, fn in paths.items():
        e = new_engine()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        free0, base = torch.cuda.mem_get_info()[0], torch.cuda.memory_allocated()
        fn(e)
        torch.cuda.synchronize()
        mem[name] = dict(device_bytes=free0 - torch.cuda.mem_get_info()[0],
                         torch_peak_bytes=torch.cuda.max_memory_allocated() - base)
        e.close()
        torch.cuda.empty_cache()
    # ---- time: one context, both paths warm, alternating
    e = new_engine()
    s, c = run_score(e)
    nll_score = -float(s.double().sum()) / float(c.sum())
    nll_mat = float(run_materialised(e)) / n_tok
    chunks = e.score_chunks()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(args.rounds):
        for name, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(e)
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    fam = {}
    for name, fn in paths.items():
        e.profile_reset()
        e.profile_enable(True)
        fn(e)
        e.synchronize()
        fam[name] = {k: v for k, v in e.profile_get().items() if v["launches"]}
        e.profile_enable(False)
    e.close()

    lines = ["Scoring given captions (capdec_score) beside materialised logits + capdec_cross_entropy -- tools/bench_score.py",
             "",
             f"Workload: {n} captions, P {P}, lengths uniform in {LMIN}..{LMAX} ({n_tok} scored tokens), GPT-2-small geometry "
             f"(V {V}), hot synthetic weights,",
             f"default GEMM mode.  score: one call, {chunks} chunk(s) of <= CAPDEC_SCORE_ROWS padded rows.  materialised: blocks of "
             f"{args.block} captions padded to {LMAX} tokens,",
             f"fp32 logits [{args.block}, {P + LMAX}, {V}] = {args.block * (P + LMAX) * V * 4 / 1e9:.2f} GB per block.  Device events "
             f"around whole passes, {args.rounds} rounds, the two paths alternating.",
             "",
             f"mean NLL per token: score {nll_score:.6f}, materialised {nll_mat:.6f} (difference {abs(nll_score - nll_mat):.2e})",
             ""]
    result = {"captions": n, "tokens": n_tok, "chunks": chunks, "paths": {}}
    for name in paths:
        med = sorted(ms[name])[len(ms[name]) // 2]
        result["paths"][name] = dict(ms_median=med, ms_min=min(ms[name]), ms_max=max(ms[name]), captions_per_s=n / (med * 1e-3),
                                     **mem[name])
        lines.append(f"{name:13s} {med:9.2f} ms per pass (min {min(ms[name]):.2f}, max {max(ms[name]):.2f})  "
                     f"{n / (med * 1e-3):9.1f} captions/s  {n_tok / (med * 1e-3):11.1f} tokens/s")
    lines.append("")
    for name in paths:
        lines.append(f"{name:13s} device memory taken by one pass in a fresh context {mem[name]['device_bytes'] / 1e9:7.3f} GB "
                     f"(of which torch tensors at their peak {mem[name]['torch_peak_bytes'] / 1e9:.3f} GB)")
    lines.append("")
    for name in paths:
        lines.append(f"per family, one profiled pass of {name} (ms, launches):")
        for k, v in sorted(fam[name].items(), key=lambda kv: -kv[1]["ms"]):
            lines.append(f"    {k:14s} {v['ms']:9.3f} {v['launches']:7d}")
    lines += ["",
              "Measured: the above, one process, one MI355X.  Not measured: other GEMM modes, other length distributions, captions",
              "sorted by length, HBM traffic counters; torch-side work of the materialised path (the cat, the slice copy in front of",
              "capdec_cross_entropy) is inside its time and appears in no family."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench_score": result}))


if __name__ == "__main__":
    main()
