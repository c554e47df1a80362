#!/usr/bin/env python
"""Time the supervised modality bridger's training (``capdec_bridger_train_epoch``) beside eager torch on the same GPU.

    python tools/bench_bridger.py [--steps 2000] [--epochs 5] [--out profiles/bridger_bench.txt]

One epoch of ``--steps`` steps at the reference's shape -- ``MLP(640, 640, 640, 8)``, batch 32, ``SGD(lr=0.001,
momentum=0.9)``, ``MSELoss`` -- over rows resident on the device.  The baseline is the same module as torch ``nn.Linear``
layers trained by eager torch on the same GPU in the same run: ``zero_grad``, forward, ``MSELoss``, ``backward``,
``optimizer.step`` per batch, the batches sliced from the resident tensors without a ``DataLoader`` (kinder to torch than
the reference's loop).  Both sides: a warm-up epoch, then ``--epochs`` epochs timed alternately with a host clock around
work that ends in a device synchronise; medians and the spread (max - min).  Also the forward of 5000 rows.  The launches
per step of the HIP side are the ones its host loop issues (2 L + 1); torch's were not counted.  Needs an MI355X."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH, LAYERS, BATCH, LR, MOMENTUM = 640, 8, 32, 0.001, 0.9


def med(v):
    return sorted(v)[len(v) // 2]


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


class TorchBridger(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.layers = torch.nn.ModuleList(torch.nn.Linear(WIDTH, WIDTH) for _ in range(LAYERS))
        for layer in self.layers:
            torch.nn.init.eye_(layer.weight)

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = F.relu(layer(x)) if i < LAYERS - 1 else layer(x)
        return x


def measure(args):
    sys.path.insert(0, ROOT)
    from capdec_amd.engine import Engine
    assert torch.cuda.is_available(), "bench_bridger needs an MI355X"
    e = Engine(0)
    g = torch.Generator().manual_seed(1)
    n = args.steps * BATCH
    x = F.normalize(torch.randn(n, WIDTH, generator=g).abs(), dim=1).cuda()
    y = F.normalize(x.cpu() * 0.5 + torch.randn(n, WIDTH, generator=g).abs(), dim=1).cuda()
    torch.manual_seed(2)
    model = TorchBridger().cuda()
    sd = model.state_dict()
    e.bridger_load([sd[f"layers.{i}.weight"].cpu() for i in range(LAYERS)], [sd[f"layers.{i}.bias"].cpu() for i in range(LAYERS)])
    criterion = torch.nn.MSELoss()
    optimizer = torch.optim.SGD(model.parameters(), lr=LR, momentum=MOMENTUM)
    losses = {}

    def hip_epoch():
        e.bridger_train_epoch(x, y, BATCH, LR, MOMENTUM)
        e.synchronize()
        _, total, steps = e.bridger_loss(reset=True)
        losses.setdefault("hip", []).append(total / steps)

    def torch_epoch():
        running = torch.zeros((), device="cuda")
        for r0 in range(0, n, BATCH):
            optimizer.zero_grad()
            loss = criterion(model(x[r0:r0 + BATCH]).view(-1), y[r0:r0 + BATCH].view(-1))
            loss.backward()
            optimizer.step()
            running += loss.detach()                      # no .item(): torch is not made to wait once per step
        losses.setdefault("torch", []).append(float(running) / args.steps)

    hip_epoch()                                          # warm-up epochs
    torch_epoch()
    hip_ms, torch_ms = [], []
    for _ in range(args.epochs):                         # alternating
        hip_ms.append(clocked(hip_epoch))
        torch_ms.append(clocked(torch_epoch))
    rows = x[:5000].contiguous()
    e.bridger_forward(rows)
    with torch.no_grad():
        model(rows)
        fwd_hip = [clocked(lambda: e.bridger_forward(rows)) for _ in range(11)]
        fwd_torch = [clocked(lambda: model(rows)) for _ in range(11)]
    return {"steps": args.steps, "epochs": args.epochs, "hip_ms": hip_ms, "torch_ms": torch_ms, "fwd_hip_ms": fwd_hip,
            "fwd_torch_ms": fwd_torch, "loss_hip": losses["hip"], "loss_torch": losses["torch"],
            "device": torch.cuda.get_device_name(0)}


def render(r):
    steps = r["steps"]
    hm, tm = med(r["hip_ms"]), med(r["torch_ms"])
    hs, ts = max(r["hip_ms"]) - min(r["hip_ms"]), max(r["torch_ms"]) - min(r["torch_ms"])
    lines = [
        "Supervised modality bridger: one epoch of training, HIP (capdec_bridger_train_epoch) beside eager torch on the same GPU",
        f"device: {r['device']}",
        f"MLP({WIDTH}, {WIDTH}, {WIDTH}, {LAYERS}), batch {BATCH}, SGD(lr={LR}, momentum={MOMENTUM}), MSELoss; {steps} steps = {steps * BATCH} rows resident on the device",
        f"a warm-up epoch each, then {r['epochs']} epochs each, alternating; host clock around work that ends in a device synchronise",
        "",
        f"{'':24}{'median ms':>12}{'spread ms':>12}{'us / step':>12}    epochs (ms)",
        f"{'HIP epoch':24}{hm:12.1f}{hs:12.1f}{hm * 1e3 / steps:12.1f}    {' '.join('%.1f' % v for v in r['hip_ms'])}",
        f"{'eager torch epoch':24}{tm:12.1f}{ts:12.1f}{tm * 1e3 / steps:12.1f}    {' '.join('%.1f' % v for v in r['torch_ms'])}",
        "",
        f"torch / HIP = {tm / hm:.2f}; the difference of the medians, {tm - hm:.1f} ms, against the two spreads together, {hs + ts:.1f} ms: "
        + ("HIP is faster by more than the spreads" if tm - hm > hs + ts else "NOT faster by more than the spreads"),
        f"launches per step, HIP: {2 * LAYERS + 1} = {LAYERS} forward + 1 loss + {LAYERS} backward-with-update (what the host loop issues); torch's were not counted",
        f"mean loss of the last timed epoch: HIP {r['loss_hip'][-1]:.6g}, torch {r['loss_torch'][-1]:.6g} (the same data and initial weights; "
        "the two sides have trained the same number of epochs)",
        "",
        f"forward of 5000 rows (one call, synchronised), median of 11: HIP {med(r['fwd_hip_ms']):.3f} ms, eager torch {med(r['fwd_torch_ms']):.3f} ms",
        "",
        "Not measured: kernel times (no profiler run), HBM traffic, torch's launch count, the reference's own loop with a DataLoader",
        "and loss.item() per step (slower than the baseline here).",
    ]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--from-json", default=None, help="render the report from the JSON line of an earlier run")
    args = ap.parse_args()
    r = json.load(open(args.from_json)) if args.from_json else measure(args)
    text = render(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
