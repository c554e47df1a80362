#!/usr/bin/env python
"""Time ``capdec_clip_score`` and a whole CLIP rerank at the size of a COCO test split.

    python tools/bench_clip_score.py [--rounds 200] [--out profiles/clip_score_bench.txt]

(a) The kernel alone: 5000 images x 5 candidates x 5 references at d 512 and d 640, with and without references -- call time
    and the algorithmic traffic (rows + groups + ref_rows) d 4 bytes over it, beside eager torch doing the same on the same
    GPU (normalize, batched matmul, clamp, max, sort; fp32).  The inputs of that size fit the Infinity Cache and are timed
    warm, so a tenfold call (50 000 images) that does not fit is timed as well.
(b) A whole rerank of the same 25 000 candidates through the CLIP ViT-B/32-shaped synthetic text tower, fp32 and
    precision="fp16", on synthetic token rows in batches of 2048: the tower's time and the scoring's.
(c) On the CPU: ``ClipBPE.tokenize`` on 25 000 short captions over a synthetic merges list -- the host step in front of (b).
Device events around whole calls (each Engine call synchronises before it returns, so launch, the offsets' copy and the
synchronise are inside), after a warm-up; medians.  (a) and (b) need an MI355X; ``--from-json FILE`` renders the report from
the JSON line an earlier run printed."""
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
PER = 5                 # candidates and references per image


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
    return dict(ms_median=med(ms), ms_min=min(ms), ms_max=max(ms))


def torch_score(cand, img, ref, w=2.5):
    """the same four columns and order in eager torch, fp32: cand [G, 5, d], img [G, d], ref [G, 5, d] or None"""
    c = torch.nn.functional.normalize(cand, dim=-1)
    v = torch.nn.functional.normalize(img, dim=-1)
    cos = torch.bmm(c, v.unsqueeze(-1)).squeeze(-1)
    clip = w * cos.clamp(min=0)
    order = cos.sort(dim=-1, descending=True, stable=True).indices
    if ref is None:
        return cos, clip, order
    r = torch.nn.functional.normalize(ref, dim=-1)
    rs = torch.bmm(c, r.transpose(1, 2)).max(-1).values.clamp(min=0)
    return cos, clip, rs, 2 * clip * rs / (clip + rs), order


def synthetic_captions(n, seed=3):
    """(merges, captions): 2000 made-up words of 3 to 8 letters, each built by its own chain of merges (so a word is one token
    after len - 1 merges, as frequent words are under the real list), and n captions of 8 to 12 words drawn with a Zipf-like
    skew"""
    rng = np.random.default_rng(seed)
    words = sorted({"".join(rng.choice(list("abcdefghijklmnopqrstuvwxyz"), int(rng.integers(3, 9)))) for _ in range(2000)})
    merges, seen = [], set()
    for wd in words:
        parts = list(wd[:-1]) + [wd[-1] + "</w>"]
        left = parts[0]
        for p in parts[1:]:
            if (left, p) not in seen:
                seen.add((left, p))
                merges.append((left, p))
            left += p
    prob = 1.0 / np.arange(1, len(words) + 1)
    prob /= prob.sum()
    caps = [" ".join(rng.choice(words, int(rng.integers(8, 13)), p=prob)) + "." for _ in range(n)]
    return merges, caps


def measure_cpu(args):
    from capdec_amd.bpe import ClipBPE
    merges, caps = synthetic_captions(args.groups * PER)
    out = {"captions": len(caps), "merges": len(merges), "s": []}
    for _ in range(3):          # a fresh tokenizer each time: the first pass fills its word cache, as a real run's does
        bpe = ClipBPE(merges)
        t0 = time.perf_counter()
        toks = bpe.tokenize(caps, truncate=True)
        out["s"].append(time.perf_counter() - t0)
    out["tokens_per_caption"] = float((toks != 0).sum(1).double().mean())
    return out


def measure(args):
    """-> the result dict the report is rendered from (and that the last output line carries as JSON)"""
    sys.path.insert(0, os.path.abspath(args.tree))
    result = {"rounds": args.rounds, "groups": args.groups, "big_groups": args.big_groups, "kernel": {}, "rerank": {},
              "tokenize": measure_cpu(args)}
    if args.cpu_only:
        return result
    from capdec_amd import clip as cclip, synth
    from capdec_amd.engine import Engine
    assert torch.cuda.is_available(), "bench_clip_score needs an MI355X"
    e = Engine(0)
    g = torch.Generator().manual_seed(1)
    for d in (512, 640):
        for G in (args.groups, args.big_groups):
            scale = 10.0 ** (torch.rand(G * PER, 1, generator=g) * 2 - 1)
            cand = (torch.randn(G * PER, d, generator=g) * scale).cuda()
            img = torch.randn(G, d, generator=g).cuda()
            ref = torch.randn(G * PER, d, generator=g).cuda()
            off = np.arange(G + 1, dtype=np.int64) * PER
            rounds = args.rounds if G == args.groups else max(5, args.rounds // 10)
            r = {"with": timed(lambda: e.clip_score(cand, img, off, ref, off), rounds),
                 "without": timed(lambda: e.clip_score(cand, img, off), rounds),
                 "torch with": timed(lambda: torch_score(cand.view(G, PER, d), img, ref.view(G, PER, d)), rounds),
                 "torch without": timed(lambda: torch_score(cand.view(G, PER, d), img, None), rounds)}
            # the two agree (fp32 eager against the fp64 sums): the comparison times the same computation
            s, o = e.clip_score(cand, img, off, ref, off)
            t = torch_score(cand.view(G, PER, d), img, ref.view(G, PER, d))
            r["max_abs_diff"] = max(float((s[:, k].view(G, PER) - t[k]).abs().max()) for k in range(4))
            r["orders_differing"] = int(((o.view(G, PER) - torch.arange(G, device=o.device)[:, None] * PER) != t[4]).any(1).sum())
            result["kernel"][f"{d}x{G}"] = r
            del cand, img, ref
    sd = {k: v for k, v in synth.hot_clip_state_dict(43, synth.CLIP_VIT_B32).items() if not k.startswith("visual.")}
    n = args.groups * PER
    tokens = synth.synthetic_clip_tokens(n, seed=21)
    img = torch.randn(args.groups, 512, generator=g).cuda()
    off = np.arange(args.groups + 1, dtype=np.int64) * PER
    for precision in ("fp32", "fp16"):
        model, _ = cclip.load(sd, device=0, precision=precision)
        feats = []

        def tower():
            feats.clear()
            feats.extend(model.encode_text(tokens[b0:b0 + 2048]).float() for b0 in range(0, n, 2048))
        tw = timed(tower, args.tower_rounds, warm=1)
        cand = torch.cat(feats)
        sc = timed(lambda: model._engine.clip_score(cand, img, off), args.rounds)
        result["rerank"][precision] = {"tower": tw, "score": sc}
        model._engine.close()
        del model, cand
    e.close()
    return result


def render(result) -> str:
    """the whole report from a result dict: every line of profiles/clip_score_bench.txt comes from here"""
    G, big = result["groups"], result["big_groups"]
    lines = ["capdec_clip_score and a whole CLIP rerank -- tools/bench_clip_score.py", "",
             f"Device events around whole calls (launch, the offsets' copy and the call's own synchronise inside), {result['rounds']} rounds",
             f"after 3 warm-up calls ({max(5, result['rounds'] // 10)} rounds at the tenfold size), medians.  Memory rate for comparison: {HBM_COPY_TBS} TB/s (float4 copy).",
             "Algorithmic traffic: (rows + groups + ref_rows) d 4 bytes.", ""]
    if result["kernel"]:
        lines.append(f"(a) the kernel alone, {PER} candidates and {PER} references per image; eager torch (fp32: normalize, bmm, clamp, max, sort) beside it")
        for key, r in result["kernel"].items():
            d, g = (int(v) for v in key.split("x"))
            for name, refs in (("with", 1), ("without", 0)):
                nbytes = (g * PER * (1 + refs) + g) * d * 4
                v, t = r[name], r["torch " + name]
                rate = nbytes / (v["ms_median"] * 1e-3) / 1e12
                warm = " (fits the Infinity Cache, timed warm: not an HBM rate)" if nbytes <= CACHE_BYTES else ""
                lines.append(f"    d {d}, {g:6d} images, {name:7s} references: {v['ms_median']:8.3f} ms (min {v['ms_min']:.3f}, max {v['ms_max']:.3f})  "
                             f"{nbytes / 1e6:7.1f} MB  {rate:6.3f} TB/s = {100 * rate / HBM_COPY_TBS:5.1f} % of the copy rate{warm}")
                lines.append(f"    {'':44s}torch {t['ms_median']:8.3f} ms (min {t['ms_min']:.3f}, max {t['ms_max']:.3f})  "
                             f"= {t['ms_median'] / v['ms_median']:5.2f} x the kernel's call")
            lines.append(f"    {'':10s}largest |HIP - torch| over the four columns {r['max_abs_diff']:.2e}; images whose order differs: {r['orders_differing']}")
        lines.append("")
    if result["rerank"]:
        lines.append(f"(b) a whole rerank: {G * PER} synthetic token rows through the CLIP ViT-B/32-shaped text tower in batches of 2048, then the scoring")
        for p, r in result["rerank"].items():
            tw, sc = r["tower"]["ms_median"], r["score"]["ms_median"]
            lines.append(f"    {p}: tower {tw:9.2f} ms (min {r['tower']['ms_min']:.2f}, max {r['tower']['ms_max']:.2f}) = {G * PER / tw:7.1f} k captions/s;  "
                         f"scoring {sc:7.3f} ms (min {r['score']['ms_min']:.3f}, max {r['score']['ms_max']:.3f}) = {100 * sc / (tw + sc):5.2f} % of the two")
        lines.append("")
    t = result["tokenize"]
    lines += [f"(c) on the CPU, one thread: ClipBPE.tokenize on {t['captions']} captions of 8 to 12 made-up words ({t['tokens_per_caption']:.1f} tokens a caption with",
              f"    SOT and EOT; {t['merges']} synthetic merges; a fresh tokenizer each run, so the word cache fills during it): "
              + ", ".join(f"{s:.2f}" for s in t["s"]) + " s",
              f"    = {t['captions'] / med(t['s']) / 1e3:.1f} k captions/s.  The real merges list is longer and real words split into more pieces: not measured."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--tower-rounds", type=int, default=3)
    ap.add_argument("--groups", type=int, default=5000)
    ap.add_argument("--big-groups", type=int, default=50000)
    ap.add_argument("--cpu-only", action="store_true", help="part (c) alone: needs no GPU")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--from-json", default=None, help="render the report from a saved result (the JSON line of an earlier run) "
                                                      "instead of measuring")
    args = ap.parse_args()
    if args.from_json:
        with open(args.from_json) as f:
            result = [json.loads(ln) for ln in f if ln.startswith('{"bench_clip_score"')][-1]["bench_clip_score"]
    else:
        sys.path.insert(0, os.path.abspath(args.tree))
        result = measure(args)
    text = render(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench_clip_score": result}))


if __name__ == "__main__":
    main()
