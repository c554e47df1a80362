"""Noise variance and modality offset from embeddings: ``capdec_embed_moments`` / ``capdec_group_distances``, their Engine
methods, and the reference's ``others/modality_offset_calculator.py`` and distance ablations (predictions_runner.py:18-95,
:235-251) under its names, against the fp64 restatement of the contract in tests/gap_stats_def.py and against what the
reference itself returned and printed (tests/golden/gap_stats.npz, tools/gen_gap_golden.py).

Bounds (gap_stats_def.py).  Definition vs reference: 4 floor + 2.4e-7 |value|, floor = max |reference - definition| stored
with the fixture.  Moments, HIP vs definition: 2.4e-7 |def| + 1e-10 (two fp32 ulps: every sum is fp64).  Distances, HIP vs
definition: 4e-7 |def| on the six statistics, c and g exact, column 2 of a two-row group bit-exact.  Facades vs reference:
4 floor + those.  A standard deviation OVER the per-image values (the STD of a print line) moves by at most the largest
change of one value, so its bound is taken on the largest value, not on itself.  Every test prints the largest deviation it
measured, as a fraction of its bound.

Measured on the MI355X (max deviation / bound):
  moments vs definition        0.247 (dim 512), 0.248 (640), 0.248 (36), 0.230 (70 001 x 64), 0.246 (zero row, inf, dim 1024)
  distances vs definition      0.179 (W 4), 0.180 (640), 0.134 (2048), 0.115 (2052), 0.121 (7680), 0.165 (30 720)
  facades vs the fixture       0.227; no print line excluded as a tie
  end to end                   tower 4.5e-6, mapper 2.1e-7 from the oracle; statistics 0.120 (W 512) and 0.109 (W 7680)
"""
import contextlib
import ctypes as C
import inspect
import io
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gap_stats_def as D                                 # noqa: E402
from capdec_amd import synth                              # noqa: E402

T = torch.from_numpy
R = 64                                                    # the slab height of gap_stats.hip (GAP_SLAB)
STATS = D.MOMENT_ROWS


def planted(n, dim, seed):
    """(images, texts) fp32 [n, dim]: column centres of 0.03..0.05, the text side planted 0.08..0.12 away on the other side
    of zero (so the offset survives the normalisation of the rows), little noise, and different row scales for the sides"""
    rng = np.random.default_rng(seed)
    sign = rng.choice([-1.0, 1.0], dim)
    centre = sign * rng.uniform(0.03, 0.05, dim)
    offset = -sign * rng.uniform(0.08, 0.12, dim)
    shared = rng.normal(0.0, 0.004, (n, dim))
    a = (centre + shared + rng.normal(0.0, 0.002, (n, dim))) * rng.uniform(5.0, 15.0, (n, 1))
    b = (centre + offset + shared + rng.normal(0.0, 0.002, (n, dim))) * rng.uniform(1.0, 3.0, (n, 1))
    return a.astype(np.float32), b.astype(np.float32)


def ragged(sizes, W, seed, scale=1.0):
    """rows of the groups one after another [sum sizes, W] fp32, the offsets, and a permutation that scatters them"""
    rng = np.random.default_rng(seed)
    rows = []
    for g in sizes:
        c = rng.normal(0.0, 1.0, W)
        rows += [c + 0.3 * rng.normal(0.0, 1.0, W) for _ in range(g)]
    x = (np.array(rows) * scale).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return x, offsets, rng.permutation(len(rows)).astype(np.int32)


class DefEngine:
    """stands for the Engine where there is no GPU: the two calls answered by the definition"""
    device = torch.device("cpu")

    def embed_moments(self, a, b=None, normalize=True, return_pair=False):
        m = D.moments(a.float().numpy(), None if b is None else b.float().numpy(), normalize)
        out = {k: T(m[k].astype(np.float32)) for k in STATS}
        if return_pair:
            out["pair"] = T(m["pair"].astype(np.float32))
        return out

    def group_distances(self, x, offsets, index=None):
        return T(D.group_distances(x.float().numpy(), offsets, None if index is None else index.numpy()).astype(np.float32))


def _prototype(header, name):
    bare = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", bare, flags=re.S)
    assert m, f"include/capdec.h does not declare {name}"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


# ===================================================================================== CPU
def test_abi_surface():
    """both prototypes are in the header, _capi.SIGNATURES agrees with them, gap_stats.hip is built, the library exports
    both symbols and the ABI number stays 6"""
    from capdec_amd import _capi, build
    header = open(os.path.join(ROOT, "include", "capdec.h")).read()
    for name, count in (("capdec_embed_moments", 8), ("capdec_group_distances", 8)):
        params = _prototype(header, name)
        res, args = _capi.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(params) == count, name
        for p, a in zip(params, args):                  # every int parameter is a c_int, every pointer a pointer
            assert (a is C.c_int) == (p.startswith("int ") and "*" not in p), (p, a)
    assert _capi.SIGNATURES["capdec_group_distances"][1][5] is _capi.c_int_p      # h_offsets is a HOST array
    assert re.search(r"#define\s+CAPDEC_ABI_VERSION\s+6\b", header) and _capi.ABI_VERSION == 6
    assert "gap_stats.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "capdec_amd", "csrc", "gap_stats.hip")).read()
    assert re.search(r"GAP_SLAB\s*=\s*%d\b" % R, src), "the tests' slab height is not the kernel's"
    lib = _capi.load_library()
    assert hasattr(lib, "capdec_embed_moments") and hasattr(lib, "capdec_group_distances")
    assert lib.capdec_abi_version() == 6


def test_reference_names_and_parameters():
    """the six functions of the reference under its names; its parameters first and under its names"""
    from capdec_amd import modality_offset_calculator as M, predictions_runner as PR
    from capdec_amd.engine import Engine
    P = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert P(PR.count_ready_parphrased_embeddings) == ["embeddings_dict"]
    assert P(PR.calc_distances_of_ready_embeddings) == ["embeddings_dict", "out_file"]
    assert inspect.signature(PR.calc_distances_of_ready_embeddings).parameters["out_file"].default == 'embeddings_distances.pkl'
    assert P(M.get_centers_info) == ["path_or_data", "limit", "engine"]
    assert inspect.signature(M.get_centers_info).parameters["limit"].default == 20000
    assert P(M.get_variance_info) == ["path_or_data", "limit", "engine"]
    assert inspect.signature(M.get_variance_info).parameters["limit"].default == 200000
    assert P(M.save_centers_info_to_pickle) == ["out_path", "path_or_data", "limit", "engine"]
    assert P(M.get_precalculated_centers) == ["path"]
    assert M.DEFAULT_EMBEDDINGS == 'coco_clip_embeddings/oscar_split_RN50x4_train_with_text_embeddings.pkl'
    assert M.DEFAULT_CENTERS == 'CLIP_embeddings_centers_info.pkl'
    assert P(PR.paraphrase_distances) == ["prefix_embed", "clip_embed", "image_ids", "engine"]
    assert P(PR.paraphrase_distance_ablation) == ["data", "clip_model", "model", "tokenize", "dont_normalize_prefix",
                                                  "modality_offset", "text_batch"]
    assert P(PR.image_text_distance) == ["image_embeddings", "text_embeddings", "engine"]
    assert P(PR.estimate_noise_variance) == ["text_embeddings", "image_ids", "normalize", "engine"]
    assert "--noise_variance 0.016" in PR.estimate_noise_variance.__doc__
    assert P(Engine.embed_moments) == ["self", "a", "b", "normalize", "return_pair"]
    assert P(Engine.group_distances) == ["self", "x", "offsets", "index"]
    assert PR.count_ready_parphrased_embeddings({1: [0] * 5, 2: None, 3: [0] * 4, 4: [0] * 5}) == 2


def _fixture_defs(g):
    m = D.moments(g["images"].astype(np.float32), g["texts"].astype(np.float32), True)
    index, offsets, ids = D.offsets_by_image(g["group_ids"].tolist())
    pre = D.group_distances(g["group_prefix"].astype(np.float32), offsets, index)
    clp = D.group_distances(g["group_clip"].astype(np.float32), offsets, index)
    return m, pre, clp, index, offsets


def test_definition_vs_reference_fixture(golden):
    """every tensor the reference returned and every number it printed, against the definition on the fixture's inputs:
    within 4 floor + 2.4e-7 |value|; the per-pair L-inf values bit-identical"""
    g = golden("gap_stats")
    m, pre, clp, index, offsets = _fixture_defs(g)
    five = clp[:, 7] == 5
    assert int(g["ref_data_size"]) == len(offsets) - 1 == 20 and int(five.sum()) == 17
    assert sorted(clp[~five, 7].tolist()) == [2, 3, 4]
    assert min(float(np.abs(m[k]).min()) for k in ("mean_a", "mean_b", "mean_diff")) >= 1e-3
    defs = {"center_text": m["mean_b"][None], "center_image": m["mean_a"][None], "offset_to_add_in_training": -m["mean_diff"][None],
            "offset_to_add_in_inference": m["mean_diff"][None], "distances": pre[five, 0], "distances_l2": pre[five, 1],
            "distances_clip": clp[five, 0], "distances_l2_clip": clp[five, 1], "max_distances_l1": clp[five, 2]}
    worst = 0.0
    for name, v in defs.items():
        floor = float(g["floor_" + name])
        assert floor <= 4e-7 * float(np.abs(v).max()), (name, floor)       # the stored floors are the size the issue states
        worst = max(worst, D.within(g["ref_" + name], v, D.REL_REF, floor=floor))
    for name, nums in (("centers", D.centers_numbers(m)), ("variance", D.variance_numbers(m)), ("distance", D.distance_numbers(pre, clp))):
        scales = [abs(v) for v in nums]
        if name == "distance":      # a mean or a STD over the per-image values moves by at most the largest change of one value
            cols = [pre[five, 0], pre[five, 1], clp[five, 0], clp[five, 1], clp[:, 4], clp[:, 5], clp[five, 2], clp[five, 3]]
            scales = [float(np.abs(cols[i // 2]).max()) for i in range(15)]
        for v, r, f, k, sc in zip(nums, g[f"ref_{name}_numbers"], g[f"floor_{name}_numbers"], g[f"ref_{name}_decimals"], scales):
            if 10.0 ** -int(k) > 1e-5 * abs(v):        # a coarse print (':.2f'): its floor is the print's rounding, so the
                assert f"{v:.{int(k)}f}" == f"{r:.{int(k)}f}", (name, v, r)      # definition must print the same digits
                continue
            assert float(f) <= 4e-7 * sc, (name, v, float(f))      # the stored floors are the size the issue states
            worst = max(worst, D.within(r, v, D.REL_REF, floor=float(f)))
    print(f"definition vs reference: max deviation / bound {worst:.3f}")
    assert worst <= 1.0
    x = g["group_clip"].astype(np.float32)
    pairs = 0
    for k in range(len(offsets) - 1):
        rows = x[index[offsets[k]:offsets[k + 1]]]
        for i in range(len(rows)):
            for j in range(i + 1, len(rows)):
                want = np.abs(rows[i] - rows[j]).max()                     # the reference's fp32 expression (:55)
                assert np.float32(np.abs(rows[i].astype(np.float64) - rows[j].astype(np.float64)).max()).tobytes() == want.tobytes()
                pairs += 1
    print(f"per-pair L-inf: {pairs} pairs bit-identical")


def test_definition_edges():
    """one row: NaN deviations; a zero row under normalize: NaN exactly where torch has it; one-row groups; a NaN in a group"""
    a, b = planted(6, 8, 1)
    m = D.moments(a[:1], b[:1])
    assert all(np.isnan(m[k]).all() for k in ("std_a", "std_b", "std_diff")) and np.isfinite(m["mean_diff"]).all()
    a[2] = 0.0
    m = D.moments(a, b)
    ta, tb = T(a.copy()), T(b.copy())
    ta /= torch.norm(ta, dim=1, keepdim=True)
    tb /= torch.norm(tb, dim=1, keepdim=True)
    want = {"mean_a": ta.mean(0), "mean_b": tb.mean(0), "mean_diff": (tb - ta).mean(0), "std_a": ta.std(0), "std_b": tb.std(0),
            "std_diff": (tb - ta).std(0), "absmean_diff": (tb - ta).abs().mean(0)}
    for k in STATS:
        np.testing.assert_array_equal(np.isnan(m[k]), torch.isnan(want[k]).numpy(), k)
        D.within(m[k], want[k].numpy().astype(np.float64), 1e-5)
    assert np.isnan(m["pair"][2]).all() and np.isfinite(np.delete(m["pair"], 2, axis=0)).all()
    only_a = D.moments(a)
    assert set(only_a) == set(STATS) and all((only_a[k] == 0).all() for k in STATS if k not in ("mean_a", "std_a"))
    x, offsets, _ = ragged([1, 2], 8, 3)
    out = D.group_distances(x, offsets)
    assert out[0].tolist() == [0, 0, 0, 0, 0, 0, 0, 1] and out[1, 6:].tolist() == [1, 2]
    assert out[1, 2] == np.abs(x[1].astype(np.float64) - x[2]).max() and abs(out[1, 3] - out[1, 1] * np.sqrt(8)) < 1e-15
    x[2, 5] = np.nan
    assert np.isnan(D.group_distances(x, offsets)[1, :6]).all()
    with pytest.raises(AssertionError):
        D.within(np.array([1.0, np.nan]), np.array([1.0, 2.0]), 1e-6)
    assert D.within(np.array([1.0 + 1e-6]), np.array([1.0]), 1e-7) > 1.0


def test_pickle_round_trip(tmp_path, golden, capsys):
    """the file the facade writes goes through formats.load_modality_offset, and through a plain pickle.load with the
    reference's four keys as fp32 [1, D] tensors (what the reference's get_precalculated_centers returns); an
    embeddings_generator pickle is accepted in place of the tensors"""
    from capdec_amd import formats, modality_offset_calculator as M
    g = golden("gap_stats")
    images, texts = T(g["images"]), T(g["texts"])
    m = D.moments(g["images"].astype(np.float32), g["texts"].astype(np.float32), True)
    out = str(tmp_path / "centers.pkl")
    M.save_centers_info_to_pickle(out, (images, texts), engine=DefEngine())
    text = capsys.readouterr().out
    assert "norm of diff =" in text and text.rstrip().endswith("saved centers info to pickle successfully")
    with open(out, "rb") as f:
        d = pickle.load(f)
    assert list(d) == ["center_text", "center_image", "offset_to_add_in_training", "offset_to_add_in_inference"]
    for k, want in (("center_text", m["mean_b"]), ("center_image", m["mean_a"]), ("offset_to_add_in_training", -m["mean_diff"]),
                    ("offset_to_add_in_inference", m["mean_diff"])):
        assert torch.is_tensor(d[k]) and d[k].dtype == torch.float32 and tuple(d[k].shape) == (1, 640) and d[k].device.type == "cpu"
        np.testing.assert_array_equal(d[k].numpy()[0], want.astype(np.float32))
        np.testing.assert_array_equal(M.get_precalculated_centers(out)[k].numpy(), d[k].numpy())
    for which in ("offset_to_add_in_inference", "offset_to_add_in_training"):
        assert torch.equal(formats.load_modality_offset(out, which), d[which])
    assert torch.equal(d["offset_to_add_in_training"], -d["offset_to_add_in_inference"])
    emb = str(tmp_path / "embeddings.pkl")
    formats.save_embeddings_pickle(emb, [{"image_id": i, "caption": ""} for i in range(200)], texts, images, half=True)
    got = M.get_centers_info(emb, limit=150, engine=DefEngine())
    want = D.moments(g["images"][:150].astype(np.float32), g["texts"][:150].astype(np.float32), True)
    np.testing.assert_array_equal(got[3].numpy()[0], want["mean_diff"].astype(np.float32))
    capsys.readouterr()


def test_facade_lines_from_the_definition(golden, capsys):
    """the facades' print lines, with the definition standing for the engine, carry the reference's text and its numbers"""
    from capdec_amd import modality_offset_calculator as M, predictions_runner as PR
    g = golden("gap_stats")
    data = (T(g["images"]), T(g["texts"]))
    M.get_centers_info(data, engine=DefEngine())
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith("Offset analysis: L2 norm=") and lines[1].startswith("STD of Offset analysis: L2 norm=")
    assert [s for _, _, s in D.parse_numbers("\n".join(lines))] == [f"{v:.2f}" for v in g["ref_centers_numbers"]]
    norms = M.get_variance_info(data, engine=DefEngine())
    lines = capsys.readouterr().out.splitlines()
    assert [ln.split("=")[0] for ln in lines] == ["STD norm of diff ", "STD norm of image embeddings ", "STD norm of text embeddings "]
    assert D.within(np.array(norms), g["ref_variance_numbers"], 2 * D.REL_REF, floor=float(g["floor_variance_numbers"].max())) <= 1.0
    pre, clp, ids = PR.paraphrase_distances(T(g["group_prefix"]), T(g["group_clip"]), g["group_ids"].tolist(), DefEngine())
    assert ids == list(dict.fromkeys(g["group_ids"].tolist())) and pre.shape == clp.shape == (20, 8)
    PR._print_distances(pre, clp)
    text = capsys.readouterr().out
    assert text.count("\n\n\n ") == 8 and "Taking max out of the 10 L2 between 5 annotations of same image CLIP: " in text
    assert len(D.parse_numbers(text)) == 15


def test_engine_argument_checks():
    """what the Engine methods refuse before they reach the library"""
    from capdec_amd._capi import CapdecError
    from capdec_amd.engine import Engine
    e = Engine.__new__(Engine)
    with pytest.raises(CapdecError, match=r"\[n, dim\]"):
        Engine.embed_moments(e, torch.zeros(4, 8), torch.zeros(4, 12))
    with pytest.raises(CapdecError, match="return_pair"):
        Engine.embed_moments(e, torch.zeros(4, 8), None, True, True)
    with pytest.raises(CapdecError, match=r"\[rows, W\]"):
        Engine.group_distances(e, torch.zeros(8), [0, 1])


# ===================================================================================== GPU
@pytest.fixture(scope="module")
def eng():
    from capdec_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _moments(eng, a, b, normalize=True, pair=False, half=False):
    cast = (lambda t: T(t).half()) if half else T
    out = eng.embed_moments(cast(a), None if b is None else cast(b), normalize=normalize, return_pair=pair)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_moments(got, a, b, normalize, what, planted_check=True):
    want = D.moments(a, b, normalize)
    if planted_check:                                    # no compared mean sits at the absolute floor
        assert min(float(np.abs(want[k]).min()) for k in (("mean_a", "mean_b", "mean_diff") if b is not None else ("mean_a",))) >= 1e-3
    worst = 0.0
    for k in STATS + (("pair",) if "pair" in got else ()):
        assert got[k].dtype == np.float32
        w = D.within(got[k], want[k], D.REL_MOMENTS, D.ABS_MOMENTS)
        assert w <= 1.0, f"{what}: {k} deviates by {w:.2f} bounds"
        worst = max(worst, w)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [512, 640, 36])
def test_moments_vs_definition(eng, dim):
    """n around the slab height, normalize on and off, without b, with and without d_pair, fp16 input"""
    worst = 0.0
    for n in (1, 2, 5, R - 1, R, R + 1, 3 * R + 7):
        a, b = planted(n, dim, 100 + n)
        for normalize in (True, False):
            for pair in (False, True):
                worst = max(worst, _check_moments(_moments(eng, a, b, normalize, pair), a, b, normalize, f"n {n} dim {dim}"))
            got = _moments(eng, a, None, normalize)
            worst = max(worst, _check_moments(got, a, None, normalize, f"n {n} dim {dim}, no b"))
            assert all((got[k] == 0).all() for k in STATS if k not in ("mean_a", "std_a"))
    a, b = planted(R + 9, dim, 7)
    ah, bh = a.astype(np.float16), b.astype(np.float16)
    worst = max(worst, _check_moments(_moments(eng, ah, bh, True, True, half=True), ah.astype(np.float32), bh.astype(np.float32),
                                      True, f"fp16 input dim {dim}"))
    print(f"moments dim {dim}: max deviation / bound {worst:.3f}")


@pytest.mark.gpu
def test_moments_many_slabs(eng):
    """70 001 x 64: 1094 slabs, more partial sums than one fold takes"""
    a, b = planted(70001, 64, 11)
    worst = _check_moments(_moments(eng, a, b, True, True), a, b, True, "70001 x 64")
    print(f"moments 70001 x 64: max deviation / bound {worst:.3f}")


@pytest.mark.gpu
def test_moments_nan_and_invariants(eng):
    """a zero row under normalize: NaN in exactly the quantities torch gives it in; the same call twice: the same bits; the
    first 100 rows' d_pair do not depend on n; refusals leave the context usable"""
    from capdec_amd._capi import CapdecError
    n, dim = 3 * R + 7, 640
    a, b = planted(n, dim, 5)
    one = _moments(eng, a, b, True, True)
    two = _moments(eng, a, b, True, True)
    assert all(one[k].tobytes() == two[k].tobytes() for k in one)
    head = _moments(eng, a[:100], b[:100], True, True)
    assert head["pair"].tobytes() == one["pair"][:100].tobytes()
    z = a.copy()
    z[R + 3] = 0.0
    got = _moments(eng, z, b, True, True)
    ta, tb = T(z.copy()), T(b.copy())
    ta /= torch.norm(ta, dim=1, keepdim=True)
    tb /= torch.norm(tb, dim=1, keepdim=True)
    want = {"mean_a": ta.mean(0), "mean_b": tb.mean(0), "mean_diff": (tb - ta).mean(0), "std_a": ta.std(0), "std_b": tb.std(0),
            "std_diff": (tb - ta).std(0), "absmean_diff": (tb - ta).abs().mean(0),
            "pair": torch.stack([(tb - ta).norm(dim=1), (tb - ta).abs().max(dim=1).values], 1)}
    for k in want:
        np.testing.assert_array_equal(np.isnan(got[k]), torch.isnan(want[k]).numpy(), k)
    assert np.isnan(got["pair"][R + 3]).all() and int(np.isnan(got["pair"]).sum()) == 2 and np.isnan(got["mean_a"]).all()
    worst = _check_moments(got, z, b, True, "zero row", planted_check=False)
    y = b.copy()
    y[5, 17] = np.inf                                    # without normalize an inf stays an inf where torch keeps one
    worst = max(worst, _check_moments(_moments(eng, a, y, False, True), a, y, False, "inf entry", planted_check=False))
    for bad, msg in (((torch.zeros(4, 1028), torch.zeros(4, 1028)), "multiple of 4"), ((torch.zeros(4, 6), torch.zeros(4, 6)), "multiple of 4"),
                     ((torch.zeros(0, 8), torch.zeros(0, 8)), "at least 1")):
        with pytest.raises(CapdecError, match=msg):
            eng.embed_moments(*bad)
    again = _moments(eng, a, b, True, True)
    assert all(one[k].tobytes() == again[k].tobytes() for k in one)
    # a constant column: the one-pass variance may come out a hair below or above 0; the header promises a std that is
    # not NaN, not negative and at most about 1e-8 sqrt(n) |mean| (here: 1e-7 |mean|, n = 199)
    k = a.copy()
    k[:, 7], k[:, 11] = np.float32(0.1), np.float32(-3.3)
    flat = _moments(eng, k, b, False)["std_a"][[7, 11]]
    print(f"std of a constant column: {flat.tolist()}")
    assert np.isfinite(flat).all() and (flat >= 0).all() and (flat <= 1e-7 * np.array([0.1, 3.3])).all()
    a4, b4 = planted(9, 1024, 3)
    worst = max(worst, _check_moments(_moments(eng, a4, b4, True, True), a4, b4, True, "dim 1024"))
    print(f"moments invariants: max deviation / bound {worst:.3f}")


def _check_groups(got, x, offsets, index, what):
    want = D.group_distances(x, offsets, index)
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_array_equal(got[:, 6:], want[:, 6:], what)
    w = D.within(got[:, :6], want[:, :6], D.REL_DIST)
    assert w <= 1.0, f"{what}: deviates by {w:.2f} bounds"
    two = want[:, 7] == 2
    assert got[two, 2].tobytes() == want[two, 2].astype(np.float32).tobytes(), f"{what}: L-inf of a two-row group is not exact"
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("W", [4, 640, 2048, 2052, 7680, 30720])
def test_distances_vs_definition(eng, W):
    """group sizes 1 to 8 in one call; 1, 2 and (at W 4, 640 and 7680) 300 groups; a permuting index and the identity.
    2048 and 2052: either side of the width from which four waves walk a group instead of one"""
    worst = 0.0
    cases = [[8, 1, 5, 2, 7, 3, 6, 4], [5], [2, 5]]
    if W <= 640 or W == 7680:                             # 300 groups of mixed sizes on the one-wave and on the four-wave path
        cases.append((np.arange(300) * 7 % 8 + 1).tolist())
    for i, sizes in enumerate(cases):
        x, offsets, perm = ragged(sizes, W, 40 + i, scale=0.05 if i % 2 else 1.0)
        got = eng.group_distances(T(x), offsets).cpu().numpy()
        worst = max(worst, _check_groups(got, x, offsets, None, f"W {W}, {len(sizes)} groups, identity"))
        scattered = np.empty_like(x)
        scattered[perm] = x                               # row r of x now lies at perm[r]
        via = eng.group_distances(T(scattered), T(offsets), T(perm)).cpu().numpy()
        worst = max(worst, _check_groups(via, scattered, offsets, perm, f"W {W}, {len(sizes)} groups, index"))
        assert via.tobytes() == got.tobytes()             # the same rows in the same order: the same bits
    assert eng.group_distances(torch.zeros(3, W), [0]).shape == (0, 8)
    print(f"distances W {W}: max deviation / bound {worst:.3f}")


@pytest.mark.gpu
def test_distances_refusals(eng):
    """nine rows, a width that is no multiple of 4, a descending offset, an index outside the rows: each is refused, and the
    same engine then answers a good call"""
    from capdec_amd._capi import CapdecError
    x, offsets, perm = ragged([3, 5, 1], 64, 9)
    xt = T(x)
    for kw, msg in ((dict(offsets=[0, 9]), "more than 8"), (dict(offsets=[0, 3, 2, 9]), "ascend"), (dict(offsets=[0, 3, 3]), "ascend"),
                    (dict(offsets=[0, 3, 10]), "past the rows"), (dict(offsets=[-1, 3]), "negative"),
                    (dict(offsets=offsets, index=T(np.where(perm == 4, 9, perm).astype(np.int32))), "outside"),
                    (dict(offsets=offsets, index=T(np.where(perm == 0, -1, perm).astype(np.int32))), "outside")):
        with pytest.raises(CapdecError, match=msg):
            eng.group_distances(xt, **kw)
        _check_groups(eng.group_distances(xt, offsets).cpu().numpy(), x, offsets, None, "after a refusal")
    with pytest.raises(CapdecError, match="multiple of 4"):
        eng.group_distances(torch.zeros(4, 6), [0, 4])
    worst = _check_groups(eng.group_distances(xt, offsets, T(perm)).cpu().numpy(), x, offsets, perm, "after the refusals")
    print(f"distances after the refusals: max deviation / bound {worst:.3f}")


def _printed(fn, *a, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*a, **kw)
    return out, D.parse_numbers(buf.getvalue()), buf.getvalue()


@pytest.mark.gpu
def test_facades_vs_reference_fixture(eng, golden, tmp_path):
    """the two facades on the fixture's inputs reproduce what the reference returned (4 floor + the HIP bounds) and what it
    printed (to the printed precision; no line of the fixture sits at a rounding tie, so none is excluded)"""
    from capdec_amd import formats, modality_offset_calculator as M, predictions_runner as PR
    g = golden("gap_stats")
    m, pre, clp, index, offsets = _fixture_defs(g)
    data = (T(g["images"]), T(g["texts"]))
    worst, excluded = 0.0, 0
    # ---- modality_offset_calculator
    got, nums, _ = _printed(M.get_centers_info, data, engine=eng)
    for t, name in zip(got, ("center_text", "center_image", "offset_to_add_in_training", "offset_to_add_in_inference")):
        assert tuple(t.shape) == (1, 640) and t.dtype == torch.float32
        worst = max(worst, D.within(t.numpy(), g["ref_" + name], D.REL_MOMENTS, D.ABS_MOMENTS, float(g["floor_" + name])))
    rel = 4 * float(g["floor_rel_moments"]) + D.REL_MOMENTS
    assert len(nums) == 8
    for p, r, k, v in zip(nums, g["ref_centers_numbers"], g["ref_centers_decimals"], D.centers_numbers(m)):
        ok = D.printed_agree(p, (float(r), int(k), f"{r:.{int(k)}f}"), v, rel * abs(v))
        excluded += ok is None
        assert ok is not False, (p, r)
    norms, nums, _ = _printed(M.get_variance_info, data, engine=eng)
    assert len(nums) == 3
    for p, r, f, v in zip(nums, g["ref_variance_numbers"], g["floor_variance_numbers"], D.variance_numbers(m)):
        w = abs(p[0] - r) / (4 * f + 2 * D.REL_MOMENTS * abs(v) + 1e-16)     # (the norm's own fp32 rounding on top)
        worst = max(worst, w)
    np.testing.assert_array_equal([p[0] for p in nums], norms)
    out = str(tmp_path / "centers.pkl")
    _printed(M.save_centers_info_to_pickle, out, data, engine=eng)
    assert torch.equal(formats.load_modality_offset(out), got[3]) and torch.equal(M.get_precalculated_centers(out)["center_text"], got[0])
    # ---- calc_distances_of_ready_embeddings
    d = {}
    for r, i in enumerate(g["group_ids"].tolist()):
        d.setdefault(i, []).append((g["group_prefix"][r].astype(np.float32), g["group_clip"][r].astype(np.float32)))
    assert PR.count_ready_parphrased_embeddings(d) == 17
    pkl = str(tmp_path / "distances.pkl")
    ret, nums, text = _printed(PR.calc_distances_of_ready_embeddings, d, out_file=pkl)      # returns: it does not exit
    assert ret[4] == int(g["ref_data_size"]) and text.rstrip().endswith(f"Saved distances to {pkl} and finished")
    with open(pkl, "rb") as f:
        saved = pickle.load(f)
    assert list(saved) == ["distances_clip", "distances_l2_clip", "max_distances_l1"]
    lists = dict(zip(("distances", "distances_l2", "distances_clip", "distances_l2_clip"), ret[:4]), max_distances_l1=saved["max_distances_l1"])
    assert saved["distances_clip"] == ret[2] and saved["distances_l2_clip"] == ret[3]
    for name, v in lists.items():
        assert isinstance(v, list) and len(v) == 17
        worst = max(worst, D.within(np.array(v), g["ref_" + name], D.REL_DIST, floor=float(g["floor_" + name])))
    ret2, nums2, _ = _printed(PR.calc_distances_of_ready_embeddings, d, out_file=None)
    assert ret2 == ret and [p[2] for p in nums2] == [p[2] for p in nums]
    five = clp[:, 7] == 5
    cols = [pre[five, 0], pre[five, 1], clp[five, 0], clp[five, 1], clp[:, 4], clp[:, 5], clp[five, 2], clp[five, 3]]
    assert len(nums) == 15
    for i, (p, r, f) in enumerate(zip(nums, g["ref_distance_numbers"], g["floor_distance_numbers"])):
        scale = float(np.abs(cols[i // 2]).max())        # a mean or a STD moves by at most the largest change of one value
        worst = max(worst, abs(p[0] - r) / (4 * f + D.REL_DIST * scale))
    print(f"facades vs the reference fixture: max deviation / bound {worst:.3f}; print lines excluded as ties: {excluded}")
    assert worst <= 1.0 and excluded == 0


@pytest.mark.gpu
def test_end_to_end_ablation(eng):
    """12 images x 5 captions through the CLIP-tiny text tower and a tiny MLP mapper: paraphrase_distance_ablation against
    oracle tower -> normalise -> oracle mapper -> definition.  The two inputs' HIP-vs-oracle deviations are measured here
    (and held to the tower's 5e-4 and the mapper's 2e-4 of tests/test_hip_parity.py); a statistic may move by the
    definition's Lipschitz constant times them: 2 max-row L-inf deviation for columns 0, 2, 3, 5, 2 max-row L2 deviation
    for column 4 and that / W for column 1, plus the kernel's own 4e-7 |def|."""
    from capdec_amd import clip as cclip, predictions_runner as PR
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    from oracle import capdec_oracle as O
    dims, cdims, P = synth.GPT2_TINY, synth.CLIP_TINY, 10
    csd = synth.hot_clip_state_dict(43, cdims)
    clip_model, _ = cclip.load(csd, device=0)
    model = ClipCaptionModel(P, clip_length=10, prefix_dim=cdims.embed_dim, num_layers=8, mapping_type=MappingType.MLP,
                             gpt2_dims=dims).to("cuda:0").eval()
    sd = synth.hot_state_dict(7, "mlp", cdims.embed_dim, P, 10, 8, dims)
    model.load_state_dict(sd)
    rows = synth.synthetic_clip_tokens(60, seed=21)
    data = [{"image_id": 500 + (i * 7) % 12, "caption": f"caption number {i}"} for i in range(60)]      # interleaved images
    table = {d["caption"]: rows[i] for i, d in enumerate(data)}
    tokenize = lambda texts: torch.stack([table[t] for t in texts])       # noqa: E731  (stands for clip.tokenize: no BPE file here)
    pre, clp, ids = PR.paraphrase_distance_ablation(data, clip_model, model, tokenize, text_batch=25)
    index, offsets, want_ids = D.offsets_by_image([d["image_id"] for d in data])
    assert ids == want_ids and pre.shape == clp.shape == (12, 8) and (clp[:, 7] == 5).all()
    # ---- the oracle's inputs, and how far the HIP inputs are from them
    raw_o = O.clip_encode_text(rows, csd, cdims.text_heads)
    x_o = O.normalize_prefix(raw_o)
    pe_o = O.clip_project(x_o, sd, "mlp", P).reshape(60, -1)
    raw_h = clip_model.encode_text(rows).float()
    x_h = model.engine.normalize_prefix(raw_h)
    pe_h = model.clip_project(x_h).reshape(60, -1)
    tower = float((raw_h.cpu() - raw_o).abs().max())
    mapper = float((pe_h.cpu() - O.clip_project(x_h.cpu(), sd, "mlp", P).reshape(60, -1)).abs().max())
    print(f"inputs: tower |hip - oracle| {tower:.2e} (5e-4), mapper on the same rows {mapper:.2e} (2e-4)")
    assert tower <= 5e-4 and mapper <= 2e-4
    worst = 0.0
    for got, hip, orc in ((clp, x_h, x_o), (pre, pe_h, pe_o)):
        dev = (hip.cpu().double() - orc.double()).numpy()
        einf, e2, W = float(np.abs(dev).max()), float(np.sqrt((dev * dev).sum(axis=1)).max()), dev.shape[1]
        want = D.group_distances(orc.numpy(), offsets, index)
        np.testing.assert_array_equal(got[:, 6:], want[:, 6:])
        lip = np.array([2 * einf, 2 * e2 / W, 2 * einf, 2 * einf, 2 * e2, 2 * einf])
        ratio = np.abs(got[:, :6] - want[:, :6]) / (lip + D.REL_DIST * np.abs(want[:, :6]))
        print(f"W {W}: row deviation L-inf {einf:.2e}, L2 {e2:.2e}; statistics: max deviation / bound {float(ratio.max()):.3f}")
        worst = max(worst, float(ratio.max()))
    assert worst <= 1.0
    # ---- the two scalars
    ids_of = [d["image_id"] for d in data]
    nv = PR.estimate_noise_variance(raw_h, ids_of, normalize=True, engine=model.engine)
    full = model.engine.group_distances(x_h, offsets, T(index)).cpu().numpy()
    assert nv == float(full[:, 2].astype(np.float64).mean())
    i58, o58, _ = D.offsets_by_image(ids_of[:58])        # two images are left with four captions
    nv58 = PR.estimate_noise_variance(x_h[:58], ids_of[:58], normalize=False, engine=model.engine)
    part = model.engine.group_distances(x_h[:58], o58, T(i58)).cpu().numpy()
    assert sorted(part[:, 7].tolist()) == [4.0] * 2 + [5.0] * 10 and nv58 == float(part[:, 2].astype(np.float64).mean())
    img = synth.synthetic_clip_embeddings(60, cdims.embed_dim, seed=3, normalize=False)
    dist = PR.image_text_distance(img, raw_h, engine=eng)
    pair = eng.embed_moments(img, raw_h, normalize=True, return_pair=True)["pair"].cpu().numpy()
    assert dist == float(pair[:, 0].astype(np.float64).mean())
    want_pair = D.moments(img.numpy(), raw_h.cpu().numpy(), True)["pair"]
    assert D.within(pair, want_pair, D.REL_MOMENTS, D.ABS_MOMENTS) <= 1.0
    print(f"noise variance estimate {nv:.5f}; image-text distance {dist:.5f}")
    model.release()
