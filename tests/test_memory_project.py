"""Projection onto a support memory: ``capdec_memory_load / _free / _project`` (memory.hip), their Engine methods,
``support_memory.SupportMemory`` and ``predictions_runner``'s ``support_memory=``, against the fp64 restatement of the contract
in tests/memory_def.py.

Bounds (memory_def): ``out`` and ``lse`` 8 x the largest error of the torch fp32 eager statement of the formula (CPU) against
the definition over the whole case, measured in the test; ``max_sim`` the bound of tests/nearest_def.py; ``nearest`` equal to
the fp64 argmax in every row (the top-two gap of every row is asserted to exceed twice the similarity bound -- on the CPU for
every GPU case in test_inputs_have_clear_nearest, and again inside every comparison).  A geometry case is one (d, M) with 67
query rows: its yardstick is taken over all 67, and the calls with 1, QTILE - 1, QTILE + 1 and 2 QTILE + 3 rows (prefixes of
the same 67) are all held to it.  Every test prints its largest deviation as a fraction of its bound.

The kernel has ONE regime: every chunk of MEM_CHUNK memory rows writes its partial whatever the row count, so there is no
threshold above which a block walks several chunks, and the invariance test names none.

The query tile is MEM_QTILE = 64 rows up to d = 512 and 32 rows at d = 640 (memory.hip: mem_groups); the row counts
1, QTILE - 1, QTILE + 1 and 2 QTILE + 3 leave a ragged last tile at either height.

Measured on the MI355X (largest deviation / bound: out, lse, max_sim):
  geometry, 13 (d, M) cases x 4 row counts     out 0.127, lse 0.154, max_sim 0.234 at most (d 640 M 6181; d 64 M 1; d 640 M 6181);
                                               every nearest equal to the fp64 argmax
  temperature 1.0 / 0.05 / 0.01 / 0.002        out 0.834 / 0.250 / 0.110 / 0.076, lse 0.260 / 0.085 / 0.113 / 0.155, max_sim 0.209
  underflowing tail (262 149 rows)             out 0.003, lse 0.432, max_sim 0.046
  special rows                                 out 0.103, lse 0.097, max_sim 0.129; duplicates: |max_sim - 1| 0.040 of its bound
  invariance (70 rows, 3 chunks + 37)          out 0.077, lse 0.096, max_sim 0.172; every comparison of bits equal
  life cycle                                   out 0.055, lse 0.106, max_sim 0.096 at most
"""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import memory_def as D                                    # noqa: E402
from capdec_amd import synth                              # noqa: E402
from capdec_amd._capi import CapdecError                  # noqa: E402

T = torch.from_numpy
SRC = open(os.path.join(ROOT, "capdec_amd", "csrc", "memory.hip")).read()
QTILE, MTILE, CHUNK = (int(re.search(r"MEM_%s\s*=\s*(\d+)" % n, SRC).group(1)) for n in ("QTILE", "MTILE", "CHUNK"))
NAMES = ("capdec_memory_load", "capdec_memory_free", "capdec_memory_project")
ROWS = (1, QTILE - 1, QTILE + 1, 2 * QTILE + 3)           # the row counts of a geometry case: prefixes of its 2 QTILE + 3 rows
BIG = 3 * CHUNK + 37
GEOMETRY = [(64, 1), (64, MTILE - 1), (64, MTILE + 1), (64, CHUNK), (64, CHUNK + 1), (64, BIG),
            (512, 1), (512, MTILE + 1), (512, CHUNK + 1), (512, BIG),
            (640, MTILE - 1), (640, CHUNK), (640, BIG)]
TAUS = (1.0, 0.05, 0.01, 0.002)
_cache = {}


def case(kind, *key):
    """(mem, x, tau, definition, bounds) of a named case: built, defined and measured against eager once per session"""
    if (kind, key) not in _cache:
        if kind == "geometry":
            d, M = key
            mem, x = D.clustered(M, ROWS[-1], d, seed=1000 * d + M)
            tau = 0.01
        elif kind == "temperature":
            mem, x = D.clustered(CHUNK + 1, QTILE + 1, 512, seed=7, scale=(1e-3, 1e3))
            tau = key[0]
        elif kind == "tail":
            mem, x = D.underflowing_tail()
            tau = 0.01
        elif kind == "special":
            mem, x = D.clustered(CHUNK + 1, QTILE + 2, 64, seed=11)
            mem[5] = 0.0                                   # a zero memory row
            mem[[100, 700, CHUNK]] = x[-1]                 # exact duplicates of the last query, which is asked on its own
            tau = 0.01
        elif kind == "invariance":
            mem, x = D.clustered(BIG, 70, 512, seed=21)
            tau = 0.01
        want = D.project(x, mem, tau)
        _cache[(kind, key)] = (mem, x, tau, want, D.yardstick(x, mem, tau, want))
    return _cache[(kind, key)]


def rows_of(want, sl):
    return {k: (v[sl] if isinstance(v, np.ndarray) else v) for k, v in want.items()}


def _prototype(header, name):
    bare = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", bare, flags=re.S)
    assert m, f"include/capdec.h does not declare {name}"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


class DefEngine:
    """stands for the Engine where there is no GPU: the memory calls answered by the definition"""
    device = torch.device("cpu")

    def __init__(self):
        self.memory, self._memory_owner, self.loads, self.calls = None, None, 0, []

    def normalize_prefix(self, x, normalize=True, offset=None):
        x = x.double()
        if normalize:
            x = x / x.norm(2, -1, keepdim=True)
        if offset is not None:
            x = x + offset.double()
        self.calls.append("normalize")
        return x.float()

    def memory_load(self, mem):
        self.mem, self.memory, self._memory_owner = mem.numpy().copy(), tuple(mem.shape), None
        self.loads += 1

    def memory_project(self, x, temperature=0.01, return_info=False):
        self.calls.append(("project", temperature))
        w = D.project(x.numpy(), self.mem, temperature)
        out = T(w["out"].astype(np.float32)).reshape(x.shape)
        info = {"lse": T(w["lse"].astype(np.float32)), "nearest": T(w["nearest"].astype(np.int32)),
                "max_sim": T(w["max_sim"].astype(np.float32))}
        return (out, info) if return_info else out


# ===================================================================================== CPU
def test_abi_surface():
    """the three prototypes are in the header, _capi.SIGNATURES agrees with them, memory.hip is built, the library exports
    the symbols, the ABI number stays 6 and the source names its tile and chunk constants"""
    from capdec_amd import _capi, build
    header = open(os.path.join(ROOT, "include", "capdec.h")).read()
    for name, count in zip(NAMES, (4, 1, 9)):
        ps = _prototype(header, name)
        res, args = _capi.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(ps) == count, name
        for p, a in zip(ps, args):
            assert (a is C.c_int) == (p.startswith("int ") and "*" not in p), (p, a)
            assert (a is C.c_float) == (p.startswith("float ") and "*" not in p), (p, a)
    assert re.search(r"#define\s+CAPDEC_ABI_VERSION\s+6\b", header) and _capi.ABI_VERSION == 6
    assert "memory.hip" in build.SOURCES
    assert QTILE >= 1 and MTILE >= 2 and CHUNK % MTILE == 0 and CHUNK > MTILE
    lib = _capi.load_library()
    assert all(hasattr(lib, n) for n in NAMES) and lib.capdec_abi_version() == 6


def test_definition_against_eager():
    """the fp64 definition and the torch fp32 statement of the formula agree on small cases; one memory row returns its unit
    vector; NaN / inf query rows come back as NaN / -1; a NaN in the memory is refused"""
    for M, N, d, tau in ((1, 3, 32, 0.01), (7, 5, 32, 1.0), (50, 9, 64, 0.01), (300, 4, 96, 0.05)):
        mem, x = D.clustered(M, N, d, seed=M + N)
        want = D.project(x, mem, tau)
        out, lse = D.eager(x, mem, tau)
        assert np.abs(out - want["out"]).max() < 2e-5 and np.abs(lse - want["lse"]).max() < 1e-3
        assert np.allclose(np.linalg.norm(want["out"], axis=1), 1.0, atol=1e-12)
        if M == 1:
            assert np.allclose(want["out"], np.tile(D.normalize(mem), (N, 1)), atol=1e-15) and (want["nearest"] == 0).all()
    mem, x = D.clustered(20, 4, 32, seed=3)
    x[1, 3], x[2, 0] = np.nan, np.inf
    want = D.project(x, mem, 0.01)
    assert list(want["bad"]) == [False, True, True, False] and list(want["nearest"][1:3]) == [-1, -1]
    assert np.isnan(want["out"][1:3]).all() and np.isnan(want["lse"][1:3]).all() and np.isfinite(want["out"][[0, 3]]).all()
    mem[4, 4] = np.nan
    with pytest.raises(ValueError):
        D.project(x, mem, 0.01)


def test_inputs_have_clear_nearest():
    """every input of the GPU tests: the two best fp64 similarities of every row are more than twice the similarity bound
    apart, so ``nearest`` is compared in every row; the tail case is the one the issue describes"""
    keys = [("geometry", k) for k in GEOMETRY] + [("temperature", (t,)) for t in TAUS] + [("tail", ()), ("invariance", ())]
    for kind, key in keys:
        mem, x, _, want, bounds = case(kind, *key)
        D.clear_nearest(x, mem, want)
        assert bounds[0] > 0 and bounds[1] > 0, (kind, key)
    mem, x, _, want, _ = case("special")
    D.clear_nearest(x[:-1], mem, rows_of(want, slice(0, -1)))
    mem, x, tau, want, _ = case("tail")
    z = want["sim"][0] / tau
    e = np.exp(z - z.max())
    assert mem.shape == (262149, 64) and 1e-3 < e[5:].sum() / e.sum() < 4e-3 and 2e-8 < e[5:].max() / e.max() < 8e-8
    assert (want["sim"][0, :5] > 0.95).all()


def test_support_memory_facade(tmp_path):
    """from_pickle on a pickle written by formats.save_embeddings_pickle, nearest_captions, loading on first use and
    reloading when the engine holds another memory"""
    from capdec_amd import formats
    from capdec_amd.support_memory import SupportMemory
    mem, x = D.clustered(40, 6, 32, seed=2)
    caps = [{"image_id": i, "caption": f"caption {i}"} for i in range(40)]
    path = str(tmp_path / "emb.pkl")
    formats.save_embeddings_pickle(path, caps, text_embeddings=T(mem), image_embeddings=T(x))
    eng = DefEngine()
    sm = SupportMemory.from_pickle(path, engine=eng)
    assert len(sm) == 40 and sm.dim == 32 and sm.captions[7] == "caption 7" and eng.loads == 0
    want = D.project(x, mem, 0.01)
    out, info = sm.project(T(x), return_info=True)
    assert eng.loads == 1 and np.abs(out.numpy() - want["out"]).max() < 1e-6
    assert sm.nearest_captions(T(x)) == [f"caption {j}" for j in want["nearest"]] and eng.loads == 1
    assert torch.equal(sm(T(x)), out)                               # __call__ is project
    assert np.abs(sm(T(x), temperature=1.0).numpy() - D.project(x, mem, 1.0)["out"]).max() < 1e-6
    assert np.abs(sm(T(x).reshape(2, 3, 32)).numpy().reshape(6, 32) - want["out"]).max() < 1e-6
    other = SupportMemory(T(mem[:10]), engine=eng)
    assert other.nearest(T(x)).max() < 10 and eng.loads == 2        # the engine now holds the other memory ...
    assert sm.nearest_captions(T(x)) == [f"caption {j}" for j in want["nearest"]] and eng.loads == 3     # ... so this one reloads
    eng.memory_load(T(mem[:5]))                                     # a load behind its back
    assert torch.equal(sm(T(x)), out) and eng.loads == 5
    with pytest.raises(CapdecError):
        other.nearest_captions(T(x))                                # built without captions
    with pytest.raises(CapdecError):
        sm(T(x[:, :16]))
    with pytest.raises(CapdecError):
        SupportMemory(T(mem), captions=["a"], engine=eng)


def test_predictions_runner_applies_projection():
    """prefix_from_embeddings: normalise (+ offset), THEN project, THEN clip_project; bridger plus memory raises; without a
    memory no new keyword travels; signatures keep the reference's parameters first"""
    from capdec_amd import predictions_runner as PR
    from capdec_amd.support_memory import SupportMemory
    mem, x = D.clustered(30, 4, 32, seed=5, scale=(0.1, 10.0))
    offset = np.linspace(-0.05, 0.05, 32).astype(np.float32)
    eng = DefEngine()

    class Model:
        engine, prefix_length = eng, 2

        def clip_project(self, v):
            eng.calls.append("clip_project")
            self.seen = v
            return v.repeat(1, 2)
    model, sm = Model(), SupportMemory(T(mem), engine=eng)
    pe = PR.prefix_from_embeddings(model, T(x), False, T(offset), support_memory=sm, projection_temperature=0.05)
    assert eng.calls == ["normalize", ("project", 0.05), "clip_project"] and tuple(pe.shape) == (4, 2, 32)
    want = D.project(D.normalize(x) + offset, mem, 0.05)["out"]
    assert np.abs(model.seen.numpy() - want).max() < 1e-6
    assert np.allclose(np.linalg.norm(model.seen.numpy(), axis=1), 1.0, atol=1e-6)
    with pytest.raises(CapdecError):
        PR.prefix_from_embeddings(model, T(x), support_memory=sm, modality_bridger=lambda v: v)
    eng.calls.clear()
    PR.prefix_from_embeddings(model, T(x))
    assert eng.calls == ["normalize", "clip_project"]
    seen, real = {}, PR.prefix_from_embeddings
    PR.prefix_from_embeddings = lambda m, e, dn=False, off=None, **kw: seen.update(kw) or (_ for _ in ()).throw(KeyError("stop"))
    try:
        for kw in ({}, {"support_memory": sm}, {"support_memory": sm, "projection_temperature": 0.5}):
            seen.clear()
            with pytest.raises(KeyError):
                PR.caption_ids(model, T(x), 0, **kw)
            assert seen == ({**{"projection_temperature": 0.01}, **kw} if kw else {})
    finally:
        PR.prefix_from_embeddings = real
    P = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert P(PR.prefix_from_embeddings)[:4] == ["model", "embeddings", "dont_normalize_prefix", "modality_offset"]
    assert P(PR.make_preds)[:9] == ["data", "embeddings", "model", "tokenizer", "out_path", "beam", "entry_length",
                                    "dont_normalize_prefix", "modality_offset"]
    assert P(PR.make_preds_from_images)[:6] == ["data", "images", "clip_model", "preprocess", "model", "tokenizer"]
    for f in (PR.prefix_from_embeddings, PR.caption_ids, PR.make_preds, PR.make_preds_from_images):
        ps = inspect.signature(f).parameters
        assert ps["support_memory"].kind is inspect.Parameter.KEYWORD_ONLY and ps["support_memory"].default is None
        assert ps["projection_temperature"].kind is inspect.Parameter.KEYWORD_ONLY and ps["projection_temperature"].default == 0.01


# ===================================================================================== GPU
@pytest.fixture(scope="module")
def eng():
    from capdec_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def run(eng, x, tau=0.01, info=True):
    got = eng.memory_project(T(np.ascontiguousarray(x)), temperature=tau, return_info=info)
    if not info:
        return got.cpu().numpy(), None
    return got[0].cpu().numpy(), {k: v.cpu().numpy() for k, v in got[1].items()}


def same_bits(a, b):
    return all(np.array_equal(p.view(np.int32), q.view(np.int32)) for p, q in zip(a, b))


def flat(out, info):
    return [out, info["lse"], info["nearest"], info["max_sim"]]


@pytest.mark.gpu
@pytest.mark.parametrize("d,M", GEOMETRY)
def test_geometry(eng, d, M):
    """one chunk, several chunks, a ragged last memory tile and a ragged last query tile, at three widths; one memory row
    returns that row's unit vector"""
    mem, x, tau, want, bounds = case("geometry", d, M)
    eng.memory_load(T(mem))
    worst = np.zeros(3)
    for n in ROWS:
        out, info = run(eng, x[:n], tau)
        worst = np.maximum(worst, D.compare(out, info, x[:n], mem, tau, f"d {d} M {M} N {n}", bounds, rows_of(want, slice(0, n))))
        if M == 1:
            assert np.abs(out - D.normalize(mem)).max() <= bounds[0] and (info["nearest"] == 0).all()
    out_only, _ = run(eng, x, tau, info=False)                      # the three optional outputs left out
    assert same_bits([out_only], [out])
    print(f"geometry d {d} M {M}: worst deviation / bound out {worst[0]:.3f} lse {worst[1]:.3f} max_sim {worst[2]:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("tau", TAUS)
def test_temperature_and_scale(eng, tau):
    """from nearly uniform weights to nearly an argmax; rows of x and of the memory scaled by 1e-3 .. 1e3: the normalisation
    is inside"""
    mem, x, _, want, bounds = case("temperature", tau)
    eng.memory_load(T(mem))
    out, info = run(eng, x, tau)
    D.compare(out, info, x, mem, tau, f"tau {tau}", bounds, want)
    assert np.abs(np.linalg.norm(out.astype(np.float64), axis=1) - 1.0).max() < 1e-6


@pytest.mark.gpu
def test_underflowing_tail(eng):
    """262 144 weights of 4e-8 each carry 2e-3 of the mass: they may not be rounded away"""
    mem, x, tau, want, bounds = case("tail")
    eng.memory_load(T(mem))
    out, info = run(eng, x, tau)
    D.compare(out, info, x, mem, tau, "underflowing tail", bounds, want)
    top = D.project(x, mem[:5], tau)["out"]
    assert np.abs(top - want["out"]).max() > 5 * bounds[0]           # (dropping the tail would miss the bound five times over)


@pytest.mark.gpu
def test_special_rows(eng):
    """a zero memory row; exact duplicates of a query in the memory; a NaN and an inf row among the queries; a NaN in the
    memory is refused and the memory loaded before still answers"""
    mem, x, tau, want, bounds = case("special")
    eng.memory_load(T(mem))
    good = x[:-1]
    out, info = run(eng, good, tau)
    D.compare(out, info, good, mem, tau, "zero memory row", bounds, rows_of(want, slice(0, -1)))
    o1, i1 = run(eng, x[-1:], tau)                                   # the duplicated query
    b = D.sim_bound(x[-1:], mem, [0], [100])[0]
    print(f"duplicates: |max_sim - 1| / bound {abs(float(i1['max_sim'][0]) - 1.0) / b:.3f}")
    assert int(i1["nearest"][0]) == 100 and abs(float(i1["max_sim"][0]) - 1.0) <= b
    assert np.abs(o1 - want["out"][-1:]).max() <= bounds[0] and abs(float(i1["lse"][0]) - want["lse"][-1]) <= bounds[1]
    mixed = np.insert(good, [1, QTILE], 0.0, axis=0)                 # rows 1 and QTILE + 1 of the call are bad
    mixed[1, 7], mixed[QTILE + 1, 0] = np.nan, np.inf
    keep = [i for i in range(len(mixed)) if i not in (1, QTILE + 1)]
    om, im = run(eng, mixed, tau)
    D.compare(om, im, mixed, mem, tau, "NaN and inf query rows", bounds)
    assert same_bits(flat(om[keep], {k: v[keep] for k, v in im.items()}), flat(out, info))
    broken = mem.copy()
    broken[CHUNK - 1, 3] = np.nan
    with pytest.raises(CapdecError, match="NaN or an inf"):
        eng.memory_load(T(broken))
    assert same_bits(flat(*run(eng, good, tau)), flat(out, info))    # the memory loaded before still answers


@pytest.mark.gpu
def test_invariance(eng):
    """a row alone, inside QTILE + 1 rows and inside 70 rows, at a memory of 3 chunks and a ragged tile: the four outputs are
    bit-identical; so are two identical calls.  (The kernel has no regime in which a block walks several chunks.)"""
    mem, x, tau, want, bounds = case("invariance")
    eng.memory_load(T(mem))
    full = flat(*run(eng, x, tau))
    assert same_bits(flat(*run(eng, x, tau)), full)
    D.compare(full[0], dict(zip(("lse", "nearest", "max_sim"), full[1:])), x, mem, tau, "70 rows", bounds, want)
    part = flat(*run(eng, x[:QTILE + 1], tau))
    assert same_bits(part, [a[:QTILE + 1] for a in full])
    for r in (0, 5, QTILE - 1, QTILE):
        alone = flat(*run(eng, x[r:r + 1], tau))
        assert same_bits(alone, [a[r:r + 1] for a in full]) and same_bits(alone, [a[r:r + 1] for a in part]), r
    for r in (QTILE + 1, 69):
        assert same_bits(flat(*run(eng, x[r:r + 1], tau)), [a[r:r + 1] for a in full]), r
    moved = flat(*run(eng, x[::-1].copy(), tau))                     # the same rows in other tile positions
    assert same_bits([a[::-1] for a in moved], full)


@pytest.mark.gpu
def test_life_cycle(eng):
    """a second memory of another M and d replaces the first; free, then project, raises; the argument errors"""
    mem_a, x_a = D.clustered(MTILE + 1, 5, 64, seed=31)
    mem_b, x_b = D.clustered(3 * MTILE + 5, 7, 128, seed=32)
    eng.memory_load(T(mem_a))
    out, info = run(eng, x_a)
    D.compare(out, info, x_a, mem_a, 0.01, "first memory")
    eng.memory_load(T(mem_b))
    assert eng.memory == (3 * MTILE + 5, 128)
    out, info = run(eng, x_b.reshape(7, 1, 128))                     # x may be [..., d]
    assert out.shape == (7, 1, 128) and info["nearest"].shape == (7, 1)
    D.compare(out, info, x_b, mem_b, 0.01, "second memory")
    assert eng.memory_project(torch.zeros(0, 128)).shape == (0, 128)
    with pytest.raises(CapdecError, match="d is not the loaded memory's"):
        run(eng, x_a)
    for tau in (0.0, -0.01, float("nan"), float("inf")):
        with pytest.raises(CapdecError, match="temperature must be positive and finite"):
            run(eng, x_b, tau)
    rc = eng.lib.capdec_memory_project(eng._h, None, -1, 128, 0.01, None, None, None, None)
    assert rc != 0 and b"negative row count" in eng.lib.capdec_last_error()
    for shape in ((1, 48), (1, 672), (1, 16)):
        with pytest.raises(CapdecError, match="multiple of 32"):
            eng.memory_load(torch.zeros(*shape))
    buf = torch.zeros(4, 64, device="cuda:0")
    for rows, d in ((0, 64), (4, 48), (4, 672)):
        assert eng.lib.capdec_memory_load(eng._h, buf.data_ptr(), rows, d) != 0
        assert b"memory_load" in eng.lib.capdec_last_error()
    assert same_bits(flat(*run(eng, x_b)), flat(out.reshape(7, 128), {k: v.reshape(7) for k, v in info.items()}))    # refused loads changed nothing
    eng.memory_free()
    with pytest.raises(CapdecError, match="no memory is loaded"):
        run(eng, x_b)
    eng.memory_free()                                                # freeing twice is fine
    eng.memory_load(T(mem_a))
    D.compare(*run(eng, x_a), x_a, mem_a, 0.01, "loaded again")


class FakeTok:
    def __init__(self, stop):
        self.stop = stop

    def encode(self, s):
        return [self.stop]

    def decode(self, ids):
        return " ".join(str(int(v)) for v in ids)


@pytest.mark.gpu
def test_end_to_end_make_preds(eng):
    """make_preds(..., support_memory=mem) gives the captions of make_preds on embeddings projected beforehand (unit rows, so
    the normalisation in front leaves them as they are up to its own rounding -- hence dont_normalize_prefix there); they
    differ from the un-projected call; make_preds_from_images takes the keyword"""
    from capdec_amd import predictions_runner as PR
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    from capdec_amd.support_memory import SupportMemory
    dims, P, W = synth.GPT2_TINY, 10, 64
    model = ClipCaptionModel(P, clip_length=10, prefix_dim=W, num_layers=8, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0").eval()
    model.load_state_dict(synth.hot_state_dict(7, "mlp", W, P, 10, 8, dims))
    x = synth.synthetic_clip_embeddings(6, W, seed=5, normalize=False)
    texts = synth.synthetic_clip_embeddings(300, W, seed=6, normalize=True)
    sm = SupportMemory(texts, captions=[f"text {i}" for i in range(300)], engine=eng)
    data = [{"image_id": 40 + i} for i in range(6)]
    tok = FakeTok(dims.vocab + 5)                          # never emitted: every step runs
    plain = PR.make_preds(data, x, model, tok, None, beam=False, entry_length=8)
    assert sm.engine is eng                                # (loads the memory)
    projected = eng.memory_project(model.engine.normalize_prefix(x), temperature=0.05)
    for beam in (False, True):
        got = PR.make_preds(data, x, model, tok, None, beam=beam, entry_length=8, support_memory=sm, projection_temperature=0.05)
        want = PR.make_preds(data, projected, model, tok, None, beam=beam, entry_length=8, dont_normalize_prefix=True)
        assert got == want
        if not beam:
            assert any(g["caption"] != p["caption"] for g, p in zip(got, plain))
    assert len(sm.nearest_captions(x)) == 6
    with pytest.raises(CapdecError):
        PR.make_preds(data, x, model, tok, None, support_memory=sm, modality_bridger=lambda v: v)

    class Clip:
        def encode_image(self, batch):
            return batch

    class Pre:
        def batch(self, ims):
            return torch.stack([T(np.asarray(im, dtype=np.float32)) for im in ims]).to("cuda:0")
    got = PR.make_preds_from_images(data, list(x.cpu().numpy()), Clip(), Pre(), model, tok, None, beam=False, entry_length=8,
                                    support_memory=sm, projection_temperature=0.05)
    assert got == PR.make_preds(data, x, model, tok, None, beam=False, entry_length=8, support_memory=sm, projection_temperature=0.05)
    model.release()
