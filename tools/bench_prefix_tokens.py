#!/usr/bin/env python
"""Time the prefix interpretation (``capdec_nearest_tokens``) at the headline size: 5000 captions x P 10 = 50 000 prefix rows
against GPT-2's 50 257 tokens at d 768 (3.86 TFLOP), k = 1 and k = 5, default GEMM mode, the cached normalised wte.

    python tools/bench_prefix_tokens.py [--rows 50000] [--rounds 5] [--out profiles/prefix_tokens_bench.txt]

Device events around whole calls after a warm-up (the warm-up builds the normalised wte and its operand planes), k = 1 and
k = 5 alternating inside every round; the clock is sampled through rocm-smi by a side thread during ~3 s more of the same
calls, outside the timed rounds.
Then, in the same process, one profiled pass (capdec_profile_get) of one 16 384-row block -- the unit the call works in, one
fused launch -- beside the fused lm_head at the same row count: the lm_head launch of a one-step greedy decode (k = 1) and of
a one-step beam-5 decode (three candidates per tile plus the exact second pass, as the decode loop runs it) over 16 384
captions of one prefix row.  FLOPs from the shapes: 2 x rows x 50 257 x 768.  Needs an MI355X."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import threading
import time

import torch

BLOCK = 16384      # rows per block of capdec_nearest_tokens (nearest.hip: NEAREST_ROWS)


def sclk_mhz():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=20).stdout
        for k, v in json.loads(out).get("card0", {}).items():
            if "sclk" in k.lower():
                return float(str(v).strip("()").lower().replace("mhz", ""))
    except Exception:      # noqa: BLE001  (no rocm-smi, another format: the clock is then reported as not measured)
        pass
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from capdec_amd import synth
    from capdec_amd.engine import Engine
    assert torch.cuda.is_available(), "bench_prefix_tokens needs an MI355X"
    dims = synth.GPT2_SMALL
    V, d, rows = dims.vocab, dims.n_embd, args.rows
    flops = 2.0 * rows * V * d
    e = Engine(0)
    e.load_gpt2(synth.hot_gpt2_state_dict(42, dims), n_head=dims.n_head)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(rows, d, generator=g) * 0.6).cuda()          # (the norms do not matter: the rows are normalised first)
    ks = (1, 5)
    for k in ks:
        e.nearest_tokens(x, k)
    torch.cuda.synchronize()
    ms = {k: [] for k in ks}
    for _ in range(args.rounds):
        for k in ks:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            e.nearest_tokens(x, k)
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    rounds = args.rounds
    # ---- the clock under this load: the same calls for ~3 s more, untimed, while a side thread asks rocm-smi
    clocks, stop = [], threading.Event()

    def sample():
        while not stop.is_set():
            c = sclk_mhz()
            if c:
                clocks.append(c)
            time.sleep(0.3)

    th = threading.Thread(target=sample, daemon=True)
    th.start()
    t_end = time.time() + 3.0
    while time.time() < t_end:
        for k in ks:
            e.nearest_tokens(x, k)
    stop.set()
    th.join()

    # ---- one profiled block beside the fused lm_head at the same row count
    def profiled(fn):
        e.profile_reset()
        e.profile_enable(True)
        fn()
        e.synchronize()
        out = {name: v for name, v in e.profile_get().items() if v["launches"]}
        e.profile_enable(False)
        return out

    xb = x[:BLOCK].contiguous()
    fam = {f"nearest k {k}": profiled(lambda k=k: e.nearest_tokens(xb, k)) for k in ks}
    one = (torch.randn(BLOCK, 1, d, generator=g) * 0.6).cuda()
    lm_err = None
    try:
        e.decode_greedy(one, V + 5, 1, -1)                         # (warm-up: KV cache, operand planes of every weight)
        e.decode_beam(one, V + 5, 5, 1)
        fam["lm_head k 1 (greedy step)"] = profiled(lambda: e.decode_greedy(one, V + 5, 1, -1))
        fam["lm_head k 5 (beam step)"] = profiled(lambda: e.decode_beam(one, V + 5, 5, 1))
    except Exception as err:      # noqa: BLE001  (reported below as not measured)
        lm_err = str(err)
    e.close()

    def med(v):
        return sorted(v)[len(v) // 2]

    lines = ["Prefix interpretation (capdec_nearest_tokens) at the headline size -- tools/bench_prefix_tokens.py", "",
             f"Workload: {rows} rows x {V} tokens x d {d} = {flops / 1e12:.2f} TFLOP per call, Gaussian rows, GPT-2-small hot synthetic wte "
             "(normalised copy cached), default",
             f"GEMM mode (two fp16 planes), blocks of {BLOCK} rows.  Device events around whole calls, {rounds} rounds, k = 1 and k = 5 "
             "alternating.",
             (f"sclk under the same calls, after the timed rounds: median {med(clocks):.0f} MHz, min {min(clocks):.0f}, max {max(clocks):.0f} "
              f"({len(clocks)} rocm-smi samples)" if clocks else "sclk: not measured (no rocm-smi reading)"), ""]
    result = {"rows": rows, "rounds": rounds, "sclk_mhz": med(clocks) if clocks else None, "k": {}}
    for k in ks:
        m = med(ms[k])
        result["k"][k] = dict(ms_median=m, ms_min=min(ms[k]), ms_max=max(ms[k]), tflops=flops / (m * 1e-3) / 1e12)
        lines.append(f"k = {k}: {m:8.3f} ms per call (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})  {flops / (m * 1e-3) / 1e12:7.1f} TFLOP/s "
                     f"(whole call: normalise + fused GEMM + merge)")
    lines.append("")
    for name, f in fam.items():
        lines.append(f"per family, one profiled pass of {name} at {BLOCK} rows (ms, launches):")
        for fk, v in sorted(f.items(), key=lambda kv: -kv[1]["ms"]):
            lines.append(f"    {fk:26s} {v['ms']:9.3f} {v['launches']:5d}")
    lines.append("")

    def per_launch(f, name):
        return f[name]["ms"] / f[name]["launches"] if name in f and f[name]["launches"] else None

    if lm_err is None:
        for k, lm in ((1, "lm_head k 1 (greedy step)"), (5, "lm_head k 5 (beam step)")):
            a = per_launch(fam[f"nearest k {k}"], "nearest_topk")
            b = per_launch(fam[lm], "gemm_f16x2p_lmhead_topk")
            if a and b:
                result["k"][k]["ratio_to_lm_head"] = a / b
                n_lm = fam[lm]["gemm_f16x2p_lmhead_topk"]["launches"]
                second = fam[lm].get("lmhead_second_pass")
                lines.append(f"k = {k}: nearest_topk {a:.3f} ms per launch / gemm_f16x2p_lmhead_topk {b:.3f} ms per launch "
                             f"({n_lm} launch(es) in the pass) = {a / b:.2f}"
                             + (f"; the lm_head's exact second pass adds {second['ms']:.3f} ms over {second['launches']} launch(es)"
                                if second else ""))
    else:
        lines.append(f"fused lm_head at {BLOCK} rows: not measured ({lm_err})")
    lines += ["",
              "Measured: the above, one process, one MI355X.  Not measured: the other GEMM modes, a caller's table (normalised and",
              "packed on every call), HBM traffic counters."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench_prefix_tokens": result}))


if __name__ == "__main__":
    main()
