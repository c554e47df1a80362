#!/usr/bin/env python
"""Time ``capdec_embed_moments`` and ``capdec_group_distances`` at the reference's own sizes.

    python tools/bench_gap_stats.py [--rounds 20] [--out profiles/gap_stats_bench.txt]

Moments: 20 000 (get_centers_info) and 200 000 (get_variance_info) pairs x 640, normalize on -- both sides with d_pair, both
sides without, and the image side alone (a third of the fp64 work per byte: if the call were bound by fp64 arithmetic it
would read about three times as fast as the other two) -- bytes read over time beside the 6.3 TB/s a float4 copy reaches on
this chip, and the same computation in fp32 torch on 16 CPU threads (the reference's own expressions).  Distances: 5000
groups of five x 7680 (P 10 x 768 prefixes) and x 640 (CLIP embeddings), through an index.  Device events around whole calls (each call
synchronises before it returns, so launch and synchronise overhead is inside), after a warm-up; medians.  Needs an MI355X;
``--from-json FILE`` renders the same report from the JSON line an earlier run printed, without one."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HBM_COPY_TBS = 6.3      # measured float4 copy rate of the chip
CACHE_BYTES = 256e6     # Infinity Cache: an input below this, timed warm, is not read from HBM


def med(v):
    return sorted(v)[len(v) // 2]


def timed(fn, rounds, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def torch_moments(a, b):
    """the reference's expressions (others/modality_offset_calculator.py:10-24, :31-44), fp32 on the host"""
    a = a / torch.norm(a, dim=1, keepdim=True)
    b = b / torch.norm(b, dim=1, keepdim=True)
    d = b - a
    return (a.mean(0), b.mean(0), d.mean(0), a.std(0), b.std(0), d.std(0), d.abs().mean(0))


MOMENT_VARIANTS = (("a, b, d_pair", 2, 16), ("a, b", 2, 11), ("a alone", 1, 5))      # name, sides read, fp64 operations per pair
DIM = 640


def measure(args):
    """-> the result dict the report is rendered from (and that the last output line carries as JSON)"""
    sys.path.insert(0, os.path.abspath(args.tree))
    from capdec_amd.engine import Engine
    assert torch.cuda.is_available(), "bench_gap_stats needs an MI355X"
    e = Engine(0)
    g = torch.Generator().manual_seed(1)
    result = {"rounds": args.rounds, "groups": args.groups, "moments": {}, "distances": {}}
    torch.set_num_threads(16)
    for n in args.sizes:
        a = torch.randn(n, DIM, generator=g) * 0.04 + 0.03
        b = torch.randn(n, DIM, generator=g) * 0.04 - 0.05
        t0 = time.perf_counter()
        torch_moments(a, b)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        torch_moments(a, b)
        cpu_ms = min(cpu_ms, (time.perf_counter() - t0) * 1e3)
        da, db = a.cuda(), b.cuda()
        result["moments"][str(n)] = {"cpu_ms": cpu_ms}
        calls = {"a, b, d_pair": lambda: e.embed_moments(da, db, True, True), "a, b": lambda: e.embed_moments(da, db, True, False),
                 "a alone": lambda: e.embed_moments(da, None, True, False)}
        for name, _, _ in MOMENT_VARIANTS:
            ms = timed(calls[name], args.rounds)
            result["moments"][str(n)][name] = dict(ms_median=med(ms), ms_min=min(ms), ms_max=max(ms))
        del da, db
    groups = args.groups
    ids = np.repeat(np.arange(groups), 5)
    perm = np.random.default_rng(2).permutation(groups * 5)
    order = np.argsort(ids[perm], kind="stable")                     # rows of one image, scattered over the array
    index = torch.tensor(perm[order].astype(np.int32)).cuda()
    offsets = (np.arange(groups + 1) * 5).astype(np.int32)
    for W in (7680, 640):
        x = torch.randn(groups * 5, W, generator=g).cuda()
        ms = timed(lambda: e.group_distances(x, offsets, index), args.rounds)
        result["distances"][str(W)] = dict(ms_median=med(ms), ms_min=min(ms), ms_max=max(ms))
        del x
    e.close()
    return result


def render(result) -> str:
    """the whole report from a result dict: every line of profiles/gap_stats_bench.txt comes from here"""
    lines = ["capdec_embed_moments and capdec_group_distances at the reference's sizes -- tools/bench_gap_stats.py", "",
             f"Device events around whole calls (launches + the call's own synchronise), {result.get('rounds', 20)} rounds after 3 warm-up calls, "
             "medians.",
             f"Memory rate for comparison: {HBM_COPY_TBS} TB/s (float4 copy).  fp64 work per pair of input elements: 9 operations in the",
             "column pass + 7 in the norm / d_pair pass (3 and 2 for the image side alone).", ""]
    rates = {}
    for key, r in sorted(result["moments"].items(), key=lambda kv: int(kv[0])):
        n, cpu_ms = int(key), r["cpu_ms"]
        resident = " -- the input fits the 256 MB Infinity Cache and is timed warm: its rates are cache rates, not HBM's" \
            if 2 * n * DIM * 4 <= CACHE_BYTES else ""
        lines.append(f"moments, {n} pairs x {DIM}, normalize on (fp32 torch on 16 CPU threads, best of 2: {cpu_ms:.1f} ms){resident}")
        for name, sides, ops in MOMENT_VARIANTS:
            v = r[name]
            m, nbytes = v["ms_median"], sides * n * DIM * 4
            rate = nbytes / (m * 1e-3) / 1e12
            rates[(n, name)] = rate
            lines.append(f"    {name:14s} {m:8.3f} ms (min {v['ms_min']:.3f}, max {v['ms_max']:.3f})  {nbytes / 1e6:8.1f} MB read  {rate:6.3f} TB/s "
                         f"= {100 * rate / HBM_COPY_TBS:5.1f} % of the copy rate  {ops * n * DIM / (m * 1e-3) / 1e12:6.2f} T fp64 op/s  "
                         f"{cpu_ms / m:7.1f} x the CPU")
        lines.append("")
    groups = result.get("groups", 5000)
    for key, v in sorted(result["distances"].items(), key=lambda kv: -int(kv[0])):
        W, m = int(key), v["ms_median"]
        nbytes = groups * 5 * W * 4
        rate = nbytes / (m * 1e-3) / 1e12
        lines.append(f"distances, {groups} groups of five x {W}, through an index: {m:8.3f} ms (min {v['ms_min']:.3f}, max {v['ms_max']:.3f})  "
                     f"{nbytes / 1e6:7.1f} MB read  {rate:6.3f} TB/s = {100 * rate / HBM_COPY_TBS:5.1f} % of the copy rate"
                     + (" (cache-resident input, timed warm: not an HBM rate)" if nbytes <= CACHE_BYTES else ""))
    big = max(int(k) for k in result["moments"])
    twice = 2 * 2 * big * DIM * 4 / (result["moments"][str(big)]["a, b, d_pair"]["ms_median"] * 1e-3) / 1e12
    lines += ["", "What bounds the moments call.  Not fp64 arithmetic: the image side alone does a third of the fp64 work per byte, and a call",
              f"bound by it would read about three times as fast as the other two.  They read at {rates[(big, 'a, b, d_pair')]:.2f}, "
              f"{rates[(big, 'a, b')]:.2f} and {rates[(big, 'a alone')]:.2f} TB/s at {big} pairs.",
              "Memory is NOT excluded.  The kernel reads every row from global memory twice (norm pass, then column pass of the same",
              "block); with several 160-330 KB slabs live per CU the second read is not known to hit L2 or the Infinity Cache, and this",
              f"tool counts no HBM bytes.  If the traffic is twice the input, the largest call moves {twice:.1f} TB/s "
              f"= {100 * twice / HBM_COPY_TBS:.0f} % of the copy rate",
              "(launch and synchronise time included), and memory is the likely bound.",
              "", "Distances.  One block per group; up to 2048 columns a group is walked by one wave, beyond by four.",
              "", "Measured: the above, one process, one MI355X.  Not measured by this tool: per-kernel times (the fold and finish launches are",
              "inside the call times; a kernel trace is a run of its own), HBM traffic counters, other widths."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 200000])
    ap.add_argument("--groups", type=int, default=5000)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--from-json", default=None, help="render the report from a saved result (the JSON line of an earlier run) "
                                                      "instead of measuring")
    args = ap.parse_args()
    if args.from_json:
        with open(args.from_json) as f:
            result = [json.loads(ln) for ln in f if ln.startswith('{"bench_gap_stats"')][-1]["bench_gap_stats"]
    else:
        result = measure(args)
    text = render(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench_gap_stats": result}))


if __name__ == "__main__":
    main()
