#!/usr/bin/env python
"""Generate tests/golden/gap_stats.npz: what the REFERENCE's ``others/modality_offset_calculator.py`` and
``predictions_runner.calc_distances_of_ready_embeddings`` return and print on seeded synthetic embeddings (build container
only: the reference is imported from its checkout, with tools/gen_golden.py's shims plus empty stand-ins for torchvision,
skimage and wandb).  Only inputs and results are written -- numbers, never reference source.

Stored: the inputs as fp16 (exact in fp32); the reference's returned tensors and lists; the numbers parsed from its print
lines, with how many decimals each was printed with; per quantity ``floor_*`` = max |reference - fp64 definition|
(tests/gap_stats_def.py) as measured here, and ``floor_rel_*`` the largest of them relative to the value, over the
quantities the reference returns unrounded.

The generator asserts that no coarse print line (the ``:.2f`` ones) sits near a rounding tie: the definition's value is at
least 1e-5 |value| away from every half-step, orders above any bound the tests use.

usage: python tools/gen_gap_golden.py
"""
from __future__ import annotations

import contextlib
import importlib.util
import io
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gap_stats_def as D       # noqa: E402
import gen_golden               # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gap_stats.npz")
GROUP_SIZES = [5, 5, 5, 2, 5, 5, 5, 5, 5, 3, 5, 5, 5, 5, 5, 4, 5, 5, 5, 5]      # 17 of five, one each of 2, 3 and 4


def import_reference():
    """-> (the reference's modality_offset_calculator, its predictions_runner)"""
    gen_golden.import_reference()       # first: transformers looks for a real torchvision while it is imported
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sk = types.ModuleType("skimage")
    sk.io = types.ModuleType("skimage.io")
    for name, mod in (("torchvision", tv), ("torchvision.transforms", tv.transforms), ("skimage", sk), ("skimage.io", sk.io),
                      ("wandb", types.ModuleType("wandb"))):
        sys.modules.setdefault(name, mod)
    import predictions_runner as ref_runner
    spec = importlib.util.spec_from_file_location("ref_modality_offset_calculator",
                                                  os.path.join(gen_golden.REF, "others", "modality_offset_calculator.py"))
    ref_moc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_moc)
    return ref_moc, ref_runner


def make_inputs():
    rng = np.random.default_rng(20240611)
    n, dim = 200, 640
    sign = rng.choice([-1.0, 1.0], dim)
    centre = sign * rng.uniform(0.02, 0.04, dim)
    offset = -sign * rng.uniform(0.06, 0.09, dim)         # planted: the text side sits `offset` away, on the other side of 0,
                                                          # so that the offset survives the normalisation of the rows
    shared = rng.normal(0.0, 0.03, (n, dim))
    images = (centre + shared + rng.normal(0.0, 0.01, (n, dim))) * rng.uniform(5.0, 15.0, (n, 1))
    texts = (centre + offset + shared + rng.normal(0.0, 0.01, (n, dim))) * rng.uniform(1.0, 3.0, (n, 1))
    clip_rows, prefix_rows, ids = [], [], []
    for k, g in enumerate(GROUP_SIZES):
        c = rng.normal(0.0, 1.0, 640)
        c /= np.linalg.norm(c)
        p = rng.normal(0.0, 1.0, 1536)
        for _ in range(g):
            r = c + 0.3 * rng.normal(0.0, 1.0, 640) / np.sqrt(640)
            clip_rows.append(r / np.linalg.norm(r))
            prefix_rows.append(p + 0.4 * rng.normal(0.0, 1.0, 1536))
            ids.append(1000 + 7 * k)
    return dict(images=images.astype(np.float16), texts=texts.astype(np.float16),
                group_clip=np.array(clip_rows).astype(np.float16), group_prefix=np.array(prefix_rows).astype(np.float16),
                group_ids=np.array(ids, np.int64))


def captured(fn, *a, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*a, **kw)
    return out, buf.getvalue()


def parsed(text, count):
    nums = D.parse_numbers(text)
    assert len(nums) == count, (count, text)
    return np.array([v for v, _, _ in nums], np.float64), np.array([k for _, k, _ in nums], np.int64)


def main():
    ref_moc, ref_runner = import_reference()
    inp = make_inputs()
    out = dict(inp)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "coco_clip_embeddings"))
        with open(os.path.join(tmp, "coco_clip_embeddings", "oscar_split_RN50x4_train_with_text_embeddings.pkl"), "wb") as f:
            pickle.dump({"clip_embedding": torch.from_numpy(inp["images"]), "captions": [],
                         "clip_embedding_text_dave": torch.from_numpy(inp["texts"])}, f)
        os.chdir(tmp)
        try:
            centers, centers_text = captured(ref_moc.get_centers_info)
            _, variance_text = captured(ref_moc.get_variance_info)
            d = {}
            for r, i in enumerate(inp["group_ids"]):
                d.setdefault(int(i), []).append((inp["group_prefix"][r].astype(np.float32), inp["group_clip"][r].astype(np.float32)))
            dist, dist_text = captured(ref_runner.calc_distances_of_ready_embeddings, d, out_file=None)
            try:
                captured(ref_runner.calc_distances_of_ready_embeddings, d, out_file=os.path.join(tmp, "dist.pkl"))
                raise AssertionError("the reference did not exit")
            except SystemExit:
                pass
            with open(os.path.join(tmp, "dist.pkl"), "rb") as f:
                saved = pickle.load(f)
        finally:
            os.chdir(cwd)
    # ---- the reference's results
    names = ("center_text", "center_image", "offset_to_add_in_training", "offset_to_add_in_inference")
    for name, t in zip(names, centers):
        assert tuple(t.shape) == (1, 640) and t.dtype == torch.float32
        out["ref_" + name] = t.numpy()
    out["ref_centers_numbers"], out["ref_centers_decimals"] = parsed(centers_text, 8)
    out["ref_variance_numbers"], out["ref_variance_decimals"] = parsed(variance_text, 3)
    for name, v in zip(("distances", "distances_l2", "distances_clip", "distances_l2_clip"), dist[:4]):
        out["ref_" + name] = np.array(v, np.float64)
    out["ref_data_size"] = np.int64(dist[4])
    np.testing.assert_array_equal(np.array(saved["distances_clip"], np.float64), out["ref_distances_clip"])
    out["ref_max_distances_l1"] = np.array(saved["max_distances_l1"], np.float64)
    out["ref_distance_numbers"], out["ref_distance_decimals"] = parsed(dist_text, 15)
    # ---- floors against the definition
    m = D.moments(inp["images"].astype(np.float32), inp["texts"].astype(np.float32), normalize=True)
    planted = min(float(np.abs(m[k]).min()) for k in ("mean_a", "mean_b", "mean_diff"))
    print(f"smallest |mean| of a column: {planted:.3e}")
    assert planted >= 1e-3
    index, offsets, _ = D.offsets_by_image(inp["group_ids"].tolist())
    pre = D.group_distances(inp["group_prefix"].astype(np.float32), offsets, index)
    clp = D.group_distances(inp["group_clip"].astype(np.float32), offsets, index)
    five = clp[:, 7] == 5
    assert five.sum() == 17 and len(offsets) - 1 == 20 == int(out["ref_data_size"])
    defs = {"center_text": m["mean_b"][None], "center_image": m["mean_a"][None], "offset_to_add_in_training": -m["mean_diff"][None],
            "offset_to_add_in_inference": m["mean_diff"][None], "distances": pre[five, 0], "distances_l2": pre[five, 1],
            "distances_clip": clp[five, 0], "distances_l2_clip": clp[five, 1], "max_distances_l1": clp[five, 2]}
    rel = {"moments": 0.0, "distances": 0.0}
    for name, v in defs.items():
        err = np.abs(out["ref_" + name] - v)
        out["floor_" + name] = np.float64(err.max())
        fam = "distances" if "distances" in name else "moments"
        rel[fam] = max(rel[fam], float((err / np.abs(v)).max()))
        print(f"{name:28s} floor {err.max():.3e}   relative {float((err / np.abs(v)).max()):.3e}")
    out["floor_rel_moments"], out["floor_rel_distances"] = np.float64(rel["moments"]), np.float64(rel["distances"])
    for name, nums in (("centers", D.centers_numbers(m)), ("variance", D.variance_numbers(m)), ("distance", D.distance_numbers(pre, clp))):
        nums = np.array(nums, np.float64)
        ref, dec = out[f"ref_{name}_numbers"], out[f"ref_{name}_decimals"]
        out[f"floor_{name}_numbers"] = np.abs(ref - nums)
        for v, r, k in zip(nums, ref, dec):
            step = 10.0 ** -int(k)
            if step > 1e-5 * abs(v):                          # a coarse print: no tie, and the print is the rounding
                assert abs((abs(v) / step) % 1.0 - 0.5) * step > 1e-5 * abs(v), (name, v, "sits at a rounding tie")
                assert abs(r - v) <= step / 2, (name, v, r)
            print(f"{name:10s} printed {r!r:24} definition {v:.17g}")
    # the per-pair L-inf values are bit-identical: an fp32 difference is exact in fp64, and rounding is monotonic
    x = inp["group_clip"].astype(np.float32)
    for k in range(len(offsets) - 1):
        rows = x[index[offsets[k]:offsets[k + 1]]]
        for i in range(len(rows)):
            for j in range(i + 1, len(rows)):
                assert np.float32(np.abs(rows[i].astype(np.float64) - rows[j].astype(np.float64)).max()) == np.abs(rows[i] - rows[j]).max()
    stored = sum(out[k].nbytes for k in ("images", "texts", "group_clip", "group_prefix"))
    assert stored < 1_000_000, stored
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, inputs {stored} bytes")
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == "__main__":
    main()
