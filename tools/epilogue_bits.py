#!/usr/bin/env python3
"""Bit-exact record of what the GEMM epilogues and the decode-step LayerNorm produce (tests/test_epilogue_bits.py).

    python tools/epilogue_bits.py --write     # on a GPU, at the commit whose results are the reference
    python tools/epilogue_bits.py             # on a GPU, at any later commit: compares bit for bit, exit status 1 on a difference

Everything runs on ``synth.GPT2_TINY`` (2 layers, d 768, vocab 1531) in the default f16x2 GEMM mode:

  logits    gpt2_logits of 100 sequences x 3 positions = 300 rows (the last 256-row tile holds 44 live rows)
  beam      beam 5, prefix 10, T 4 on 3300 captions = 16 500-row decode steps (the large-row LayerNorm form)
  stop      the same with a stop bias that ends about half the captions after the first step, compaction on: the qkv
            scatter epilogue runs with a caption map
  special   logits of a model whose c_fc columns 0, 8, 16, ... receive exactly +70 000, -70 000, +inf, 1e-5, 1e-40, -0.0
            (weight column zeroed, bias set), and the saturated-quad count of that call; "special_nan" adds a NaN column
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "epilogue_bits.npz")
STOP_ID = 13
N_CAP, BEAM, P, T = 3300, 5, 10, 4
STOP_ALPHAS = (8.0, 10.0, 12.0, 14.0, 16.0, 20.0, 26.0)
SPECIALS = (70000.0, -70000.0, float("inf"), 1e-5, 1e-40, -0.0)      # one per quad: column 8 * i of c_fc (NaN: the next one)


def _bits(t):
    """a tensor's bytes as an integer array: NaN payloads and the sign of zero take part in the comparison"""
    a = t.detach().cpu().contiguous().numpy()
    return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize]).copy()


def _row_hashes(t):
    """SHA-256 of the bytes of every row of a [..., V] tensor, uint8 [rows, 32]: the 300 x 1531 logits are 1.8 MB, their
    row digests 10 KB, and equal digests are equal bits"""
    import hashlib
    a = t.detach().cpu().contiguous().numpy()
    a = a.reshape(-1, a.shape[-1])
    return np.stack([np.frombuffer(hashlib.sha256(r.tobytes()).digest(), dtype=np.uint8) for r in a])


def _engine(sd):
    from capdec_amd.engine import Engine
    e = Engine(0)
    e.load_gpt2(sd)
    e.decode_counters()
    return e


def _prefix(n, seed):
    from capdec_amd import synth
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, P, synth.GPT2_TINY.n_embd, generator=g) * 0.3


def special_state_dict(with_nan):
    """hot-init weights whose c_fc pre-activations in the chosen columns ARE the special values, in both layers"""
    from capdec_amd import synth
    dims = synth.GPT2_TINY
    sd = {k: v.clone() for k, v in synth.hot_gpt2_state_dict(42, dims).items()}
    sd["gpt.lm_head.weight"] = sd["gpt.transformer.wte.weight"]
    vals = list(SPECIALS) + ([float("nan")] if with_nan else [])
    for i in range(dims.n_layer):
        w, b = sd[f"gpt.transformer.h.{i}.mlp.c_fc.weight"], sd[f"gpt.transformer.h.{i}.mlp.c_fc.bias"]
        for j, v in enumerate(vals):
            w[:, 8 * j] = 0.0
            b[8 * j] = v
    return sd


def expected_saturated(rows, n_layer):
    """+70 000 and +inf survive gelu_new beyond 65504 (one quad each, per row and layer); -70 000 becomes -0"""
    return 2 * rows * n_layer


def run_logits():
    from capdec_amd import synth
    dims = synth.GPT2_TINY
    g = torch.Generator().manual_seed(11)
    x = torch.randn(100, 3, dims.n_embd, generator=g) * 0.3
    out = {}
    e = _engine(synth.hot_gpt2_state_dict(42, dims))
    out["logits"] = _row_hashes(e.gpt2_logits(x))
    out["logits_saturated"] = np.int64(e.decode_counters()["saturated_quads"])
    e.close()
    for name, nan in (("special", False), ("special_nan", True)):
        e = _engine(special_state_dict(nan))
        out[name] = _row_hashes(e.gpt2_logits(x))
        out[name + "_saturated"] = np.int64(e.decode_counters()["saturated_quads"])
        e.close()
    return out


def _beam(e, pe, tag, out):
    i, l, s, _ = e.decode_beam(pe, STOP_ID, BEAM, T)
    out[tag + "_ids"], out[tag + "_lens"], out[tag + "_scores"] = _bits(i), _bits(l), _bits(s)


def run_beams(alpha=None):
    """-> (arrays, alpha): ``alpha`` None searches STOP_ALPHAS for the bias after which the second step runs nearest to
    half the rows (what --write records)"""
    from capdec_amd import synth
    dims = synth.GPT2_TINY
    sd = synth.hot_gpt2_state_dict(42, dims)
    pe = _prefix(N_CAP, 23)
    out = {}
    e = _engine(sd)
    _beam(e, pe, "beam", out)
    e.close()
    best = None
    for a in (STOP_ALPHAS if alpha is None else (float(alpha),)):
        e = _engine(synth.with_stop_bias(sd, STOP_ID, a))
        e.set_compact(True)
        cur = {}
        _beam(e, pe, "stop", cur)
        rows, st = e.decode_step_rows(), e.decode_stats()
        e.close()
        second = rows[1] if len(rows) > 1 else 0
        print(f"stop bias {a}: step rows {rows}, compactions {st['compactions']}")
        if best is None or abs(second - N_CAP * BEAM / 2) < best[0]:
            best = (abs(second - N_CAP * BEAM / 2), a, cur, rows, st["compactions"])
    out.update(best[2])
    out["stop_rows"] = np.asarray(best[3], dtype=np.int64)
    out["stop_compactions"] = np.int64(best[4])
    return out, best[1]


def run_all(alpha=None):
    out = run_logits()
    b, alpha = run_beams(alpha)
    out.update(b)
    out["stop_alpha"] = np.float64(alpha)
    return out


def compare(got, ref):
    """names whose arrays differ (shape, dtype or any bit)"""
    bad = []
    for k in sorted(ref.keys()):
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(a, b):
            bad.append(k)
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--write", action="store_true", help="record this tree's results as the golden file")
    ap.add_argument("--golden", default=GOLDEN)
    a = ap.parse_args()
    if a.write:
        out = run_all()
        os.makedirs(os.path.dirname(a.golden), exist_ok=True)
        np.savez_compressed(a.golden, **out)
        print(f"wrote {a.golden}: stop alpha {float(out['stop_alpha'])}, stop rows {out['stop_rows'].tolist()}, saturated "
              f"{int(out['logits_saturated'])} / {int(out['special_saturated'])} / {int(out['special_nan_saturated'])} "
              f"(expected {expected_saturated(300, 2)} for the special models)")
        return 0
    ref = np.load(a.golden)
    got = run_all(float(ref["stop_alpha"]))
    bad = compare(got, ref)
    print("identical" if not bad else f"DIFFERENT: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
