"""CLIPScore and CLIP reranking of candidate captions: ``capdec_clip_score``, ``Engine.clip_score``, the facades of
``capdec_amd/clip_score.py`` and ``make_preds(..., clip_rerank=...)``, against the fp64 restatement of the contract in
tests/clip_score_def.py.  The score is not in the reference, so there is no fixture: the contract (include/capdec.h) is the
specification.

Bound, HIP vs definition: 2.4e-7 |def| + 1e-10 on each of the four columns (every sum is fp64: one rounding to fp32 and the
order of an fp64 sum remain; w enters before the rounding).  The order must equal the definition's exactly; the inputs are
built -- and asserted on the definition's values, on the CPU -- so that inside a group two cosines are more than 4 bounds
apart or belong to bit-identical rows.  Every test prints the largest deviation it measured, as a fraction of the bound.

Measured on the MI355X (max deviation / bound):
  kernel vs definition         0.099 (d 1), 0.237 (36), 0.236 (512), 0.237 (640), 0.227 (2048); every order exact
  after the refusals           0.237 (d 36)
  towers to score              0.241 (6 images x 3 candidates + 2 references, d 512)
  decode to rerank             0.227; the CLIP-best beam is not the LM-best one for 6 of 8 images
"""
import ctypes as C
import functools
import inspect
import os
import re
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import clip_score_def as D                                # noqa: E402
from capdec_amd import synth                              # noqa: E402

T = torch.from_numpy
COLS = ("cos", "clip_s", "ref_sim", "refclip_s")
SOT, EOT = 49406, 49407


# ===================================================================================== stand-ins
class DefEngine:
    """stands for the Engine where there is no GPU: the call answered by the definition"""
    device = torch.device("cpu")

    def clip_score(self, cand, img, offsets, ref=None, ref_offsets=None, w=2.5):
        s, o = D.clip_score(cand.float().numpy(), img.float().numpy(), np.asarray(offsets),
                            None if ref is None else ref.float().numpy(), None if ref_offsets is None else np.asarray(ref_offsets), w)
        return T(s.astype(np.float32)), T(o)


def fake_tokenize(texts):
    """stands for clip.tokenize (no BPE file here): valid SOT ... EOT rows, 1 to 12 tokens long, a function of the text"""
    out = torch.zeros(len(texts), 77, dtype=torch.int64)
    for r, t in enumerate(texts):
        assert isinstance(t, str)
        rng = np.random.default_rng(zlib.crc32(t.encode()))
        L = 1 + int(rng.integers(0, 12))
        out[r, 0], out[r, 1 + L] = SOT, EOT
        out[r, 1:1 + L] = T(rng.integers(1, SOT, L))
    return out


class FakeClip:
    """a text tower on the CPU: a row's feature is the scaled sum of the table rows of its tokens"""

    def __init__(self, d=24):
        self._engine = DefEngine()
        self.table = T(np.random.default_rng(5).normal(0, 1, (997, d)).astype(np.float32))
        self.batches = []

    def encode_text(self, tokens):
        assert tokens.dim() == 2 and tokens.shape[1] == 77 and (tokens[:, 0] == SOT).all()
        self.batches.append(int(tokens.shape[0]))
        body = (tokens > 0) & (tokens < SOT)
        return (self.table[tokens % 997] * body[..., None]).sum(1) * 3.0


class FakeTok:
    """stands for the GPT-2 tokenizer: a caption is its ids"""

    def __init__(self, stop):
        self.stop = stop

    def encode(self, s):
        return [self.stop]

    def decode(self, ids):
        return " ".join(str(int(v)) for v in ids)


def _def_on_texts(clip_model, feats_img, lists, refs=None, w=2.5, tokenize=fake_tokenize):
    """the definition on the features ``clip_model`` gives the texts -> (scores fp64 [rows, 4], order, offsets, cand rows)"""
    enc = lambda ls: clip_model.encode_text(tokenize([t for ts in ls for t in ts])).float().cpu().numpy()      # noqa: E731
    off = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int64)
    cand = enc(lists)
    ref = roff = None
    if refs is not None:
        roff = np.concatenate([[0], np.cumsum([len(t) for t in refs])]).astype(np.int64)
        ref = enc(refs)
    s, o = D.clip_score(cand, feats_img.float().cpu().numpy(), off, ref, roff, w)
    return s, o, off, cand


# ===================================================================================== the kernel's test call
SIZES = [3, 0, 1, 2, 5, 63, 64, 4]          # candidates per group: 0, 1, 2, 5, 63, 64 between two other groups
NREF = [5, 1, 17, 0, 1, 17, 5, 17]          # references per group: 0, 1, 5, 17 (17 x 2048 x 4 B: several slabs)
DIMS = [1, 36, 512, 640, 2048]


def _unit(rng, d):
    v = rng.normal(0, 1, d)
    return v / np.sqrt((v * v).sum())


def _near(rng, v, alpha, d):
    """a row whose cosine to the unit row v is about alpha, at a scale in 1e-3 .. 1e3"""
    if d == 1:
        return np.array([alpha]) * v * 10.0 ** rng.uniform(-3, 3)
    n = _unit(rng, d)
    n = n - (n * v).sum() * v
    n /= np.sqrt((n * n).sum())
    return (alpha * v + np.sqrt(1 - alpha * alpha) * n) * 10.0 ** rng.uniform(-3, 3)


@functools.lru_cache(maxsize=None)
def case(d):
    """the call of test 1 at width d: (cand, img, offsets, ref, ref_offsets) fp32 / int64, with the planted rows.  At d == 1
    every cosine is +1 or -1, so every group takes its candidates from two values: equal cosines are bit-identical rows"""
    rng = np.random.default_rng(1000 + d)
    img, cand, ref = [], [], []
    for g, (nc, nr) in enumerate(zip(SIZES, NREF)):
        v = _unit(rng, d)
        img.append(v * 10.0 ** rng.uniform(-3, 3))
        if d == 1:
            two = [_near(rng, v, 1.0, d), _near(rng, v, -1.0, d)]
            cand += [two[1 if (7 * j + g) % 3 == 0 else 0] for j in range(nc)]
        else:
            cand += [_near(rng, v, rng.uniform(-0.3, 0.95), d) for _ in range(nc)]
        ref += [_near(rng, v, rng.uniform(-0.3, 0.95) if d > 1 else rng.choice([-1.0, 1.0]), d) for _ in range(nr)]
    cand, img, ref = (np.array(x).astype(np.float32) for x in (cand, img, ref))
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    roff = np.concatenate([[0], np.cumsum(NREF)]).astype(np.int64)
    e = min(d - 1, 17)
    g5 = off[4]
    cand[g5 + 3] = cand[g5 + 1]                            # a bit-identical pair
    if d > 1:
        cand[g5] = -np.abs(cand[g5 + 2]) * np.sign(img[4])  # a negative cosine for certain
    cand[off[5] + 10, e] = np.nan                          # a NaN row
    cand[off[6] + 7, e] = np.inf                           # an inf row
    cand[off[6] + 20] = 0.0                                # an all-zero candidate
    img[3] = 0.0                                           # an all-zero image row: its two candidates are NaN
    ref[roff[7] + 9, e] = np.nan                           # a NaN reference row: columns 2 and 3 of the last group
    return cand, img, off, ref, roff


@functools.lru_cache(maxsize=None)
def case_def(d, w):
    cand, img, off, ref, roff = case(d)
    s, o = D.clip_score(cand, img, off, ref, roff, w)
    D.assert_order_decidable(s, off, cand)                 # the condition on the inputs
    return s, o


def subset(d, gs):
    """the groups ``gs`` of case(d), in that order, as a call of their own, and the rows of the full call they came from"""
    cand, img, off, ref, roff = case(d)
    rows = np.concatenate([np.arange(off[g], off[g + 1]) for g in gs] + [np.zeros(0, np.int64)]).astype(np.int64)
    rrows = np.concatenate([np.arange(roff[g], roff[g + 1]) for g in gs] + [np.zeros(0, np.int64)]).astype(np.int64)
    o2 = np.concatenate([[0], np.cumsum([SIZES[g] for g in gs])]).astype(np.int64)
    r2 = np.concatenate([[0], np.cumsum([NREF[g] for g in gs])]).astype(np.int64)
    return (cand[rows], img[list(gs)], o2, ref[rrows], r2), rows


def _prototype(header, name):
    bare = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", bare, flags=re.S)
    assert m, f"include/capdec.h does not declare {name}"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


# ===================================================================================== CPU
def test_abi_surface():
    """the prototype is in the header, _capi.SIGNATURES agrees with it (13 parameters, ints are c_int, both offset arrays the
    host pointer type), clipscore.hip is built, the library exports the symbol and the ABI number stays 6"""
    from capdec_amd import _capi, build
    header = open(os.path.join(ROOT, "include", "capdec.h")).read()
    params = _prototype(header, "capdec_clip_score")
    res, args = _capi.SIGNATURES["capdec_clip_score"]
    assert res is C.c_int and len(args) == len(params) == 13
    for p, a in zip(params, args):
        assert (a is C.c_int) == (p.startswith("int ") and "*" not in p), (p, a)
        assert (a is C.c_float) == p.startswith("float w"), (p, a)
    assert "h_offsets" in params[5] and args[5] is _capi.c_int_p and "h_ref_offsets" in params[9] and args[9] is _capi.c_int_p
    assert re.search(r"#define\s+CAPDEC_ABI_VERSION\s+6\b", header) and _capi.ABI_VERSION == 6
    assert "clipscore.hip" in build.SOURCES and "score.hip" in build.SOURCES
    lib = _capi.load_library()
    assert hasattr(lib, "capdec_clip_score") and lib.capdec_abi_version() == 6


def test_definition_sanity():
    """cases worked out by hand"""
    v = np.array([[3.0, 4.0, 0.0]], np.float32)
    s, o = D.clip_score(v * 7, v, [0, 1])                  # identical direction: cos 1, clip_s = w
    assert s[0, 0] == 1.0 and s[0, 1] == 2.5 and np.isnan(s[0, 2:]).all() and o.tolist() == [0]
    assert D.clip_score(v * 7, v, [0, 1], w=1.0)[0][0, 1] == 1.0
    s, _ = D.clip_score(np.array([[0.0, 0.0, 2.0]], np.float32), v, [0, 1])      # orthogonal
    assert s[0, 0] == 0.0 and s[0, 1] == 0.0
    # antiparallel, with a reference: refclip_s follows from ref_sim alone -- 0 when both are 0
    for ref, want_sim in ((-v, 1.0), (v, 0.0)):
        s, _ = D.clip_score(-2 * v, v, [0, 1], ref, [0, 1])
        assert s[0, 0] == -1.0 and s[0, 1] == 0.0 and s[0, 2] == want_sim and s[0, 3] == 0.0
    # two references: candidate (1, 0), image (0.6, 0.8): cos 0.6, clip_s 1.5; references (0.8, 0.6) and (0, 1): ref_sim 0.8;
    # harmonic mean 2 * 1.5 * 0.8 / 2.3 = 2.4 / 2.3
    s, _ = D.clip_score(np.array([[1.0, 0.0]], np.float32), np.array([[0.6, 0.8]], np.float32), [0, 1],
                        np.array([[0.8, 0.6], [0.0, 1.0]], np.float32), [0, 2])
    assert abs(s[0, 0] - 0.6) < 1e-7 and abs(s[0, 1] - 1.5) < 3e-7 and abs(s[0, 2] - 0.8) < 1e-7 and abs(s[0, 3] - 2.4 / 2.3) < 3e-7
    # an empty group between two others; a group without references beside one with
    c = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], np.float32)
    im = np.array([[1.0, 0.0], [5.0, 5.0], [0.0, 2.0]], np.float32)
    s, o = D.clip_score(c, im, [0, 1, 1, 3], np.array([[0.0, 3.0]], np.float32), [0, 0, 0, 1])
    assert s.shape == (3, 4) and o.tolist() == [0, 1, 2] and s[0, 0] == 1.0 and np.isnan(s[0, 2:]).all()
    assert s[1, 2] == 1.0 and abs(s[2, 2] - np.sqrt(0.5)) < 1e-15 and s[1, 0] == 1.0
    # the order: descending fp32 cosine, NaN last, equal values by row; bad rows
    assert D.rank(np.array([0.1, np.nan, 0.7, 0.1, np.nan, -0.2], np.float32)).tolist() == [2, 0, 3, 5, 1, 4]
    bad = np.array([[1.0, 0.0], [np.nan, 1.0], [0.0, 0.0], [np.inf, 1.0], [0.5, 0.5]], np.float32)
    s, o = D.clip_score(bad, np.array([[1.0, 1.0]], np.float32), [0, 5], np.array([[1.0, 0.0], [0.0, 0.0]], np.float32), [0, 2])
    assert np.isnan(s[1:4]).all() and np.isfinite(s[[0, 4], :2]).all() and np.isnan(s[:, 2:]).all() and o.tolist() == [4, 0, 1, 2, 3]
    assert np.isnan(D.clip_score(bad, np.zeros((1, 2), np.float32), [0, 5])[0]).all()
    with pytest.raises(AssertionError):
        D.within(np.array([1.0, np.nan]), np.array([1.0, 2.0]))
    assert D.within(np.array([1.0 + 1e-6]), np.array([1.0])) > 1.0
    with pytest.raises(AssertionError):                    # two different rows with the same cosine are not decidable
        D.assert_order_decidable(np.array([[0.5] * 4, [0.5] * 4]), [0, 2], np.array([[1.0, 2.0], [2.0, 4.0]], np.float32))


@pytest.mark.parametrize("d", DIMS)
def test_inputs_are_decidable(d):
    """the condition on the kernel test's inputs holds, and the planted rows are what they are meant to be"""
    cand, img, off, ref, roff = case(d)
    s, o = case_def(d, 2.5)
    assert len(cand) == sum(SIZES) and len(ref) == sum(NREF) and cand.dtype == np.float32
    g5 = off[4]
    assert s[g5 + 1].tobytes() == s[g5 + 3].tobytes() and list(o[off[4]:off[5]]).index(g5 + 1) + 1 == list(o[off[4]:off[5]]).index(g5 + 3)
    assert (s[off[4]:off[5], 0] < 0).any()
    assert np.isnan(s[[off[5] + 10, off[6] + 7, off[6] + 20]]).all() and np.isnan(s[off[3]:off[4]]).all()
    assert np.isnan(s[off[7]:, 2:]).all() and np.isfinite(s[off[7]:, :2]).all()
    assert np.isnan(s[off[3]:off[4], 2:]).all() and int(np.isnan(s[:, 0]).sum()) == 5
    assert o[off[6 + 1] - 2:off[7]].tolist() == [off[6] + 7, off[6] + 20]      # the NaN rows last, by row
    scale = np.abs(np.concatenate([cand[np.isfinite(cand).all(1)].ravel(), ref[np.isfinite(ref).all(1)].ravel()]))
    assert scale.max() / scale[scale > 0].min() > 1e3


def test_facades_on_the_definition():
    """clip_score, rerank_by_clip and score_predictions with the definition for the engine, a CPU text tower and a fake
    tokenizer: ragged lists, the shapes of what comes back, the corpus means over every image's first candidate"""
    from capdec_amd import clip_score as CS
    from capdec_amd._capi import CapdecError
    clip = FakeClip()
    feats = T(np.random.default_rng(2).normal(0, 1, (4, 24)).astype(np.float32))
    lists = [["a cat", "a dog on a mat", "two birds"], [], ["a very long caption " * 3], ["x", "y"]]
    refs = [["cat", "a cat sits"], ["unused"], [], ["x", "z", "w"]]
    res = CS.clip_score(clip, feats, lists, refs, tokenize=fake_tokenize, w=2.0, text_batch=4)
    assert clip.batches == [4, 2, 4, 2]                    # six candidates, then six references, in batches of four
    s, o, off, cand = _def_on_texts(clip, feats, lists, refs, 2.0)
    D.assert_order_decidable(s, off, cand)
    for k, name in enumerate(COLS):
        assert isinstance(res[name], list) and [len(a) for a in res[name]] == [3, 0, 1, 2]
        np.testing.assert_array_equal(np.concatenate(res[name]), s[:, k].astype(np.float32))
        assert all(a.dtype == np.float32 for a in res[name])
    assert [x.tolist() for x in res["order"]] == [(o[off[g]:off[g + 1]] - off[g]).tolist() for g in range(4)]
    first = s.astype(np.float32)[[0, 3, 4]].astype(np.float64)      # every image's FIRST candidate; image 1 has none
    assert res["CLIPScore"] == first[:, 1].mean() and isinstance(res["CLIPScore"], float)
    assert np.isnan(res["RefCLIPScore"]) and np.isnan(first[1, 3])       # image 2 has no references: the mean says so
    full = CS.clip_score(clip, feats[[0, 3]], [lists[0], lists[3]], [refs[0], refs[3]], tokenize=fake_tokenize)
    s2 = _def_on_texts(clip, feats[[0, 3]], [lists[0], lists[3]], [refs[0], refs[3]])[0].astype(np.float32).astype(np.float64)
    assert full["RefCLIPScore"] == s2[[0, 3], 3].mean() and full["CLIPScore"] == s2[[0, 3], 1].mean()
    # one string per image: arrays [N]; no references: NaN columns and NaN RefCLIPScore
    flat = CS.clip_score(clip, feats, ["a", "b", "c", "d"], tokenize=fake_tokenize)
    assert all(flat[n].shape == (4,) for n in COLS) and np.isnan(flat["ref_sim"]).all() and np.isnan(flat["RefCLIPScore"])
    assert [x.tolist() for x in flat["order"]] == [[0]] * 4 and flat["CLIPScore"] == flat["clip_s"].astype(np.float64).mean()
    # rerank_by_clip: every list reordered, nothing else changed
    ranked, cos = CS.rerank_by_clip(clip, feats, lists, tokenize=fake_tokenize, return_scores=True)
    assert ranked == CS.rerank_by_clip(clip, feats, lists, tokenize=fake_tokenize)
    assert [sorted(r) for r in ranked] == [sorted(x) for x in lists] and lists[0] == ["a cat", "a dog on a mat", "two birds"]
    for g in range(4):
        assert ranked[g] == [lists[g][i] for i in o[off[g]:off[g + 1]] - off[g]]
        assert (np.diff(cos[g]) <= 0).all() and cos[g].tolist() == s[off[g]:off[g + 1], 0].astype(np.float32)[o[off[g]:off[g + 1]] - off[g]].tolist()
    assert any(r != x for r, x in zip(ranked, lists))      # (something did move)
    # score_predictions: the list make_preds writes, references by image id
    preds = [{"caption": lists[g][0], "image_id": 70 + g} for g in (0, 2, 3)]
    by_id = {70: refs[0], 72: ["a long one"], 73: refs[3], 99: ["never used"]}
    sp = CS.score_predictions(preds, feats[[0, 2, 3]], clip, by_id, tokenize=fake_tokenize)
    want = _def_on_texts(clip, feats[[0, 2, 3]], [[p["caption"]] for p in preds], [by_id[p["image_id"]] for p in preds])[0].astype(np.float32)
    assert sp["image_id"] == [70, 72, 73] and all(sp[n].shape == (3,) for n in COLS)
    np.testing.assert_array_equal(np.stack([sp[n] for n in COLS], 1), want)
    assert sp["CLIPScore"] == want[:, 1].astype(np.float64).mean() and sp["RefCLIPScore"] == want[:, 3].astype(np.float64).mean()
    assert np.isnan(CS.score_predictions(preds, feats[[0, 2, 3]], clip, tokenize=fake_tokenize)["RefCLIPScore"])
    for call in (lambda: CS.score_predictions(preds, feats[[0, 2, 3]], clip, {70: ["a"]}, tokenize=fake_tokenize),
                 lambda: CS.clip_score(clip, feats, lists[:3], tokenize=fake_tokenize),
                 lambda: CS.clip_score(clip, feats, ["a", ["b"], "c", "d"], tokenize=fake_tokenize),
                 lambda: CS.clip_score(clip, feats, lists, ["a", "b", "c", "d"], tokenize=fake_tokenize),
                 lambda: CS.rerank_by_clip(clip, feats, ["a", "b", "c", "d"], tokenize=fake_tokenize)):
        with pytest.raises(CapdecError):
            call()
    sig = inspect.signature(CS.clip_score).parameters
    assert list(sig) == ["clip_model", "image_features", "candidates", "references", "tokenize", "w", "text_batch"]
    assert sig["w"].default == 2.5 and sig["text_batch"].default == 2048 and sig["tokenize"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(CS.rerank_by_clip).parameters) == ["clip_model", "image_features", "texts", "tokenize", "return_scores"]
    assert list(inspect.signature(CS.score_predictions).parameters) == ["preds", "image_features", "clip_model", "references", "tokenize", "w"]


def test_default_tokenizer_truncates(monkeypatch):
    """without a tokenize argument the module calls capdec_amd.clip.tokenize so that an over-long caption is truncated"""
    from capdec_amd import clip as cclip, clip_score as CS
    seen = []

    def spy(texts, context_length=77, truncate=False):
        seen.append((list(texts), truncate))
        return fake_tokenize(texts)
    monkeypatch.setattr(cclip, "tokenize", spy)
    CS.clip_score(FakeClip(), torch.ones(1, 24), ["word " * 200])
    assert seen == [(["word " * 200], True)]


def test_make_preds_reranks_on_the_definition(monkeypatch):
    """make_preds(..., clip_rerank=...) with the decode replaced by fixed beams: all five beams of the shard are scored against
    embeddings[lo:hi] and the CLIP-best one is written; the keywords are last and keyword-only; beam=False raises; without the
    keywords nothing of it runs"""
    from capdec_amd import predictions_runner as PR
    from capdec_amd._capi import CapdecError
    ps = inspect.signature(PR.make_preds).parameters
    assert list(ps)[-2:] == ["clip_rerank", "clip_tokenize"]
    assert all(ps[k].kind is inspect.Parameter.KEYWORD_ONLY and ps[k].default is None for k in ("clip_rerank", "clip_tokenize"))
    n, B, L = 6, 5, 7
    rng = np.random.default_rng(9)
    ids = T(rng.integers(0, 500, (n, B, L)).astype(np.int32))
    lens = T(rng.integers(2, L + 1, (n, B)).astype(np.int32))
    scores = T(np.sort(rng.normal(0, 1, (n, B)))[:, ::-1].astype(np.float32).copy())
    x = T(rng.normal(0, 1, (n, 24)).astype(np.float32))
    seen = {}

    def beams(model, pe, stop, beam_size, entry_length, **kw):
        seen["pe"] = pe
        return ids, lens, scores, None
    monkeypatch.setattr(PR, "prefix_from_embeddings", lambda model, emb, *a, **kw: emb)
    monkeypatch.setattr(PR, "decode_beam_ids", beams)
    monkeypatch.setattr(PR, "decode_constrained_beam_ids", lambda model, pe, phrases, *a, **kw: (ids, lens, scores, None, None))
    monkeypatch.setattr(PR, "_phrases_of", lambda tok, n, words, wid: np.zeros((n, 4, 4), np.int32))
    clip, tok = FakeClip(), FakeTok(999)
    data = [{"image_id": 10 + i} for i in range(n)]
    text = lambda r, b: tok.decode(ids[r, b, :int(lens[r, b])].tolist())      # noqa: E731
    plain = PR.make_preds(data, x, None, tok, None, beam=True)
    assert [p["caption"] for p in plain] == [text(r, 0) for r in range(n)] and not clip.batches
    lists = [[text(r, b) for b in range(B)] for r in range(n)]
    s, o, off, cand = _def_on_texts(clip, x, lists)
    D.assert_order_decidable(s, off, cand)
    best = [int(o[off[r]] - off[r]) for r in range(n)]
    assert any(best) and torch.equal(seen["pe"], x)
    clip.batches.clear()
    for kw in ({}, {"force_words": [["w"]] * n}):
        got = PR.make_preds(data, x, None, tok, None, beam=True, clip_rerank=clip, clip_tokenize=fake_tokenize, **kw)
        assert got == [{"caption": text(r, best[r]), "image_id": 10 + r} for r in range(n)]
    assert clip.batches == [n * B, n * B]
    with pytest.raises(CapdecError, match="beam"):
        PR.make_preds(data, x, None, tok, None, beam=False, clip_rerank=clip, clip_tokenize=fake_tokenize)
    assert PR.make_preds(data, x, None, tok, None, beam=True) == plain


def test_engine_argument_checks():
    """what Engine.clip_score refuses before it reaches the library"""
    from capdec_amd._capi import CapdecError
    from capdec_amd.engine import Engine
    e = Engine.__new__(Engine)
    z = torch.zeros
    for args, msg in (((z(4), z(1, 8), [0, 4]), r"\[rows, d\]"), ((z(4, 8), z(1, 6), [0, 4]), r"\[rows, d\]"),
                      ((z(4, 8), z(1, 8), [0, 4], z(3, 6), [0, 3]), r"\[ref_rows, d\]"), ((z(4, 8), z(2, 8), [0, 4]), "image rows"),
                      ((z(4, 8), z(1, 8), [0.0, 4.0]), "32 bits"), ((z(4, 8), z(1, 8), [0, 2 ** 31]), "32 bits"),
                      ((z(4, 8), z(1, 8), []), r"groups \+ 1"), ((z(4, 8), z(1, 8), [0, 4], z(3, 8), [0, 1, 3]), "ref_offsets must have")):
        with pytest.raises(CapdecError, match=msg):
            Engine.clip_score(e, *args)
    assert list(inspect.signature(Engine.clip_score).parameters) == ["self", "cand", "img", "offsets", "ref", "ref_offsets", "w"]
    assert inspect.signature(Engine.clip_score).parameters["w"].default == 2.5


# ===================================================================================== GPU
@pytest.fixture(scope="module")
def eng():
    from capdec_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _run(eng, call, w=2.5):
    cand, img, off, ref, roff = call
    s, o = eng.clip_score(T(cand), T(img), off, None if ref is None else T(ref), roff, w)
    assert s.dtype == torch.float32 and o.dtype == torch.int32 and s.is_cuda and o.is_cuda
    assert tuple(s.shape) == (len(cand), 4) and tuple(o.shape) == (len(cand),)
    return s.cpu().numpy(), o.cpu().numpy()


def _check(got, want, what):
    (s, o), (ws, wo) = got, want
    worst = 0.0
    for k, name in enumerate(COLS):
        f = D.within(s[:, k], ws[:, k])
        assert f <= 1.0, f"{what}: {name} deviates by {f:.2f} bounds"
        worst = max(worst, f)
    np.testing.assert_array_equal(o, wo, what)             # every group, none excluded
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_kernel_vs_definition(eng, d):
    """the four columns within the bound and the order exact, for w 2.5 and 1.0, with and without references"""
    call = case(d)
    worst = 0.0
    for w in (2.5, 1.0):
        got = _run(eng, call, w)
        worst = max(worst, _check(got, case_def(d, w), f"d {d} w {w}"))
        g5 = call[2][4]
        assert got[0][g5 + 1].tobytes() == got[0][g5 + 3].tobytes()      # bit-identical rows: bit-identical scores
    bare = _run(eng, call[:3] + (None, None))
    want = case_def(d, 2.5)
    assert np.isnan(bare[0][:, 2:]).all() and bare[0][:, :2].tobytes() == _run(eng, call)[0][:, :2].tobytes()
    np.testing.assert_array_equal(bare[1], want[1])
    print(f"kernel vs definition d {d}: max deviation / bound {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("d", [36, 640, 2048])
def test_invariance(eng, d):
    """a group's scores and order are the same bits alone, in reversed group order, and with or without its neighbours"""
    full = _run(eng, case(d))
    off = case(d)[2]
    G = len(SIZES)
    for gs in [(g,) for g in range(G)] + [tuple(range(G))[::-1], (4, 5, 6), (5,), (7, 2, 5, 0), (6, 6)]:
        call, rows = subset(d, gs)
        s, o = _run(eng, call)
        np.testing.assert_array_equal(s.view(np.uint32), full[0][rows].view(np.uint32), f"d {d} groups {gs}")
        for k, g in enumerate(gs):                         # the order, after undoing the row shift
            lo = call[2][k]
            np.testing.assert_array_equal(o[lo:lo + SIZES[g]] - lo, full[1][off[g]:off[g + 1]] - off[g], f"d {d} groups {gs}")
    again = _run(eng, case(d))
    assert again[0].tobytes() == full[0].tobytes() and again[1].tobytes() == full[1].tobytes()
    cand, img, o2, ref, roff = case(d)
    odd = T(np.concatenate([np.zeros(1, np.float32), cand.ravel()])).to("cuda:0")[1:].view(-1, d)      # rows not 16-byte aligned
    assert odd.data_ptr() % 16 == 4
    s, o = eng.clip_score(odd, T(img), o2, T(ref), roff)
    assert s.cpu().numpy().tobytes() == full[0].tobytes() and o.cpu().numpy().tobytes() == full[1].tobytes()


@pytest.mark.gpu
def test_refusals(eng):
    """every refusal of the contract, through the Engine (the error text) and through the library with outputs pre-filled
    with a sentinel (untouched); a valid call afterwards is within the bound; empty calls return empty tensors"""
    from capdec_amd import _capi
    from capdec_amd._capi import CapdecError
    d = 36
    cand, img, off, ref, roff = case(d)
    want = case_def(d, 2.5)
    rows, groups, rrows = len(cand), len(SIZES), len(ref)
    dev = lambda a: T(a).to("cuda:0")                      # noqa: E731
    xc, xi, xr = dev(cand), dev(img), dev(ref)
    scores = torch.full((rows, 4), -7.0, device="cuda:0")
    order = torch.full((rows,), -7, device="cuda:0", dtype=torch.int32)
    i32 = lambda a: np.ascontiguousarray(np.asarray(a, np.int32))      # noqa: E731

    def raw(o=off, ro=roff, d_=d, rows_=rows, rrows_=rrows, with_ref=True, with_roff=True):
        o, ro = i32(o), i32(ro)
        eng._sync_stream()
        return eng.lib.capdec_clip_score(eng._h, xc.data_ptr(), rows_, d_, xi.data_ptr(), o.ctypes.data_as(_capi.c_int_p), groups,
                                         xr.data_ptr() if with_ref else None, rrows_,
                                         ro.ctypes.data_as(_capi.c_int_p) if with_roff else None, 2.5, scores.data_ptr(), order.data_ptr())
    bump = lambda a, k, v: np.concatenate([a[:k], a[k:] + v])          # noqa: E731
    swapped = off.copy()
    swapped[2], swapped[3] = off[3] + 1, off[2]
    big = off.copy()
    big[6] += 2                                            # the groups of 63 and 64 become 65 and 62
    assert np.diff(big).max() == 65
    refusals = (("offsets descend", dict(o=swapped), "descend"), ("offsets start past 0", dict(o=bump(off, 0, 1), rows_=rows + 1), "start at 0"),
                ("offsets end before rows", dict(rows_=rows + 1), "end at rows"), ("a group above 64", dict(o=big), "more than 64"),
                ("d 0", dict(d_=0), "1..2048"), ("d 2049", dict(d_=2049), "1..2048"),
                ("d_ref alone", dict(with_roff=False), "go together"), ("h_ref_offsets alone", dict(with_ref=False), "go together"),
                ("reference offsets descend", dict(ro=np.concatenate([roff[:2], [0], roff[3:]])), "descend"),
                ("reference offsets start past 0", dict(ro=bump(roff, 0, 1), rrows_=rrows + 1), "start at 0"),
                ("reference offsets end before ref_rows", dict(rrows_=rrows + 1), "end at ref_rows"))
    for what, kw, msg in refusals:
        assert raw(**kw) != 0, what
        assert msg in eng.lib.capdec_last_error().decode(), (what, eng.lib.capdec_last_error())
        assert bool((scores == -7.0).all()) and bool((order == -7).all()), f"{what}: an output was written"
    # ... and through the Engine, which raises with the library's text
    for kw, msg in ((dict(offsets=swapped), "descend"), (dict(offsets=bump(off, 0, 1)), "start at 0"), (dict(offsets=off[:-1]), "image rows"),
                    (dict(offsets=bump(off, groups, -1)), "end at rows"), (dict(offsets=big), "more than 64"),
                    (dict(ref=None), "go together"), (dict(ref_offsets=None), "go together"),
                    (dict(ref_offsets=bump(roff, groups, 1)), "end at ref_rows")):
        args = dict(cand=xc, img=xi, offsets=off, ref=xr, ref_offsets=roff)
        args.update(kw)
        with pytest.raises(CapdecError, match=msg):
            eng.clip_score(**args)
    with pytest.raises(CapdecError, match="1..2048"):
        eng.clip_score(torch.zeros(2, 2049), torch.zeros(1, 2049), [0, 2])
    assert raw() == 0                                      # the valid call, into the same buffers
    worst = _check((scores.cpu().numpy(), order.cpu().numpy()), want, "after the refusals")
    # empty calls
    s, o = eng.clip_score(torch.zeros(0, d), torch.zeros(0, d), [0])
    assert tuple(s.shape) == (0, 4) and tuple(o.shape) == (0,) and s.dtype == torch.float32 and o.dtype == torch.int32
    s, o = eng.clip_score(torch.zeros(0, d), torch.zeros(3, d), [0, 0, 0, 0], torch.zeros(0, d), [0, 0, 0, 0])
    assert tuple(s.shape) == (0, 4) and tuple(o.shape) == (0,)
    s, o = eng.clip_score(torch.zeros(0, d), xi[:3], [0, 0, 0, 0], xr[:6], [0, 5, 6, 6])
    assert tuple(s.shape) == (0, 4) and tuple(o.shape) == (0,)
    worst = max(worst, _check(_run(eng, case(d)), want, "after the empty calls"))
    print(f"after the refusals: max deviation / bound {worst:.3f}")


@pytest.fixture(scope="module")
def clip_tiny():
    from capdec_amd import clip as cclip
    model, _ = cclip.load(synth.hot_clip_state_dict(43, synth.CLIP_TINY), device=0)
    return model


@pytest.mark.gpu
def test_towers_to_score(clip_tiny):
    """6 images x (3 candidates + 2 references) through the CLIP-tiny towers: clip_score against the definition applied to
    the features the HIP towers returned (the towers have their own tests: this isolates the new kernel)"""
    from capdec_amd import clip_score as CS
    feats = clip_tiny.encode_image(synth.synthetic_images(6, seed=8)).float()
    lists = [[f"image {g} candidate {k} " + "word " * (g + k) for k in range(3)] for g in range(6)]
    refs = [[f"reference {k} of image {g}" for k in range(2)] for g in range(6)]
    res = CS.clip_score(clip_tiny, feats, lists, refs, tokenize=fake_tokenize)
    s, o, off, cand = _def_on_texts(clip_tiny, feats, lists, refs)
    D.assert_order_decidable(s, off, cand)
    assert np.isfinite(s).all() and len({len(np.flatnonzero(r)) for r in fake_tokenize([t for ts in lists for t in ts]).numpy()}) > 3
    worst = 0.0
    for k, name in enumerate(COLS):
        assert [len(a) for a in res[name]] == [3] * 6
        worst = max(worst, D.within(np.concatenate(res[name]), s[:, k]))
    assert worst <= 1.0
    assert [x.tolist() for x in res["order"]] == [(o[off[g]:off[g + 1]] - off[g]).tolist() for g in range(6)]
    got = np.stack([np.concatenate(res[n]) for n in COLS], 1)
    assert res["CLIPScore"] == got[::3, 1].astype(np.float64).mean() and res["RefCLIPScore"] == got[::3, 3].astype(np.float64).mean()
    assert abs(res["CLIPScore"] - s[::3, 1].mean()) <= D.bound(np.abs(s[::3, 1]).max())
    print(f"towers to score: max deviation / bound {worst:.3f}; CLIPScore {res['CLIPScore']:.4f} RefCLIPScore {res['RefCLIPScore']:.4f}")


@pytest.mark.gpu
def test_decode_to_rerank(clip_tiny):
    """a GPT2-tiny caption model and CLIP-tiny on 8 embeddings: rerank_by_clip(generate_beam_batch(...)) gives the definition's
    order on the same texts; make_preds(..., clip_rerank=...) writes for every image the beam whose definition cosine is
    largest; make_preds without the keywords returns what it returned before"""
    from capdec_amd import clip_score as CS, predictions_runner as PR
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    from capdec_amd.gpt2_prefix_eval import generate_beam_batch
    dims, P, W, n = synth.GPT2_TINY, 10, synth.CLIP_TINY.embed_dim, 8
    model = ClipCaptionModel(P, clip_length=10, prefix_dim=W, num_layers=8, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0").eval()
    model.load_state_dict(synth.hot_state_dict(7, "mlp", W, P, 10, 8, dims))
    x = synth.synthetic_clip_embeddings(n, W, seed=5, normalize=False).to("cuda:0")
    tok = FakeTok(dims.vocab + 5)                          # never emitted: every step runs
    data = [{"image_id": 40 + i} for i in range(n)]
    before = PR.make_preds(data, x, model, tok, None, beam=True, entry_length=8)
    texts = generate_beam_batch(model, tok, PR.prefix_from_embeddings(model, x), entry_length=8)
    assert [len(t) for t in texts] == [5] * n and [t[0] for t in texts] == [p["caption"] for p in before]
    s, o, off, cand = _def_on_texts(clip_tiny, x, texts)
    D.assert_order_decidable(s, off, cand)                 # no image has two beams within the tie gap
    ranked, cos = CS.rerank_by_clip(clip_tiny, x, texts, tokenize=fake_tokenize, return_scores=True)
    worst = 0.0
    for g in range(n):
        idx = o[off[g]:off[g + 1]] - off[g]
        assert ranked[g] == [texts[g][i] for i in idx]
        worst = max(worst, D.within(cos[g], s[off[g]:off[g + 1], 0][idx]))
    assert worst <= 1.0
    got = PR.make_preds(data, x, model, tok, None, beam=True, entry_length=8, clip_rerank=clip_tiny, clip_tokenize=fake_tokenize)
    assert got == [{"caption": ranked[g][0], "image_id": 40 + g} for g in range(n)]
    moved = sum(g["caption"] != b["caption"] for g, b in zip(got, before))
    print(f"decode to rerank: max deviation / bound {worst:.3f}; the CLIP-best beam is not the LM-best one for {moved} of {n} images")
    assert PR.make_preds(data, x, model, tok, None, beam=True, entry_length=8) == before
    model.release()
