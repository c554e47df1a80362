"""Times the projection onto a support memory (capdec_memory_load / capdec_memory_project) at the size of the COCO training
captions -- M = 566 747 synthetic rows, d in {512, 640}, N in {1, 625, 5000} -- beside eager torch fp32 on the same GPU in the
same run (``softmax((xn @ mn.T) / tau) @ mn``, N chunked so that the similarity block fits), and writes the table to --out.

    python tools/bench_memory_project.py --out profiles/memory_project_bench.txt

Runs on the GPU only.  Every timed window is a host clock around calls that end in a device synchronise, after one warm-up
call of the same shape; the windows repeat the call until ``--min-seconds`` have passed.  The rate counts the 4 N M d useful
flops of the two products and is an end-to-end rate of the call (normalisation, partials and merge included), not a kernel's.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

M_COCO = 566747
EAGER_BLOCK_BYTES = 2 << 30          # the [rows, M] similarity block eager works on at a time


def timed(fn, min_seconds, sync):
    fn()
    sync()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        sync()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds or n >= 50:
            return 1e3 * dt / n, n


def eager_project(x, mn, tau, rows_per_block):
    out = []
    xn = torch.nn.functional.normalize(x, dim=-1)
    for r0 in range(0, x.shape[0], rows_per_block):
        w = torch.softmax((xn[r0:r0 + rows_per_block] @ mn.T) / tau, dim=-1)
        out.append(torch.nn.functional.normalize(w @ mn, dim=-1))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=M_COCO, help="memory rows")
    ap.add_argument("--dims", type=int, nargs="+", default=[512, 640])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 625, 5000])
    ap.add_argument("--tau", type=float, default=0.01)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_memory_project: no GPU -- this benchmark measures nothing without one")
    from capdec_amd.engine import Engine
    dev = torch.device("cuda:0")
    eng = Engine(0)
    sync = lambda: torch.cuda.synchronize(dev)      # noqa: E731
    lines = [f"projection onto a support memory: M = {a.rows} rows, tau = {a.tau}, {torch.cuda.get_device_name(0)}",
             "ms per call (host clock around synchronised calls, after a warm-up call; calls timed in brackets); TFLOP/s = 4 N M d / time,",
             "the end-to-end rate of the call; eager = torch fp32 normalize / matmul / softmax / matmul on the same GPU, same run",
             "",
             f"{'d':>4} {'N':>5} | {'memory_load ms':>14} | {'memory_project ms':>18} {'TFLOP/s':>8} | {'eager ms':>14} {'TFLOP/s':>8} | {'eager / ours':>12} | max |ours - eager|"]
    for d in a.dims:
        g = torch.Generator(device="cpu").manual_seed(d)
        centres = torch.randn(4096, d, generator=g)
        mem = (centres[torch.randint(0, 4096, (a.rows,), generator=g)] + 0.5 * torch.randn(a.rows, d, generator=g)).to(dev)
        load_ms, load_n = timed(lambda: eng.memory_load(mem), a.min_seconds, sync)
        mn = torch.nn.functional.normalize(mem, dim=-1)
        for n in a.queries:
            x = (centres[torch.randint(0, 4096, (n,), generator=g)] + 0.5 * torch.randn(n, d, generator=g)).to(dev)
            ms, calls = timed(lambda: eng.memory_project(x, temperature=a.tau), a.min_seconds, sync)
            blk = max(1, min(n, EAGER_BLOCK_BYTES // (4 * a.rows)))
            ems, ecalls = timed(lambda: eager_project(x, mn, a.tau, blk), a.min_seconds, sync)
            diff = float((eng.memory_project(x, temperature=a.tau) - eager_project(x, mn, a.tau, blk)).abs().max())
            flops = 4.0 * n * a.rows * d
            lines.append(f"{d:>4} {n:>5} | {load_ms:>10.2f} [{load_n:>2}] | {ms:>14.3f} [{calls:>2}] {flops / ms / 1e9:>8.2f} | "
                         f"{ems:>9.3f} [{ecalls:>2}] {flops / ems / 1e9:>8.2f} | {ems / ms:>12.2f} | {diff:.2e}")
            print(lines[-1], flush=True)
        del mem, mn
        eng.memory_free()
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    eng.close()


if __name__ == "__main__":
    main()
