"""Prefix interpretation and editing: ``capdec_nearest_tokens`` / ``Engine.nearest_tokens`` and the reference's
``get_prefix_tokens`` / ``add_embedding_from_text`` / ``generate_text`` / ``re_caption`` / ``remove_token`` / ``try_all_places``
(gpt2_prefix_eval.py:201-251) against the fp64 restatement of the contract in tests/nearest_def.py and the reference's own
results in tests/golden/prefix_tokens_tiny.npz (tools/gen_golden.py).

Bounds (nearest_def.py): |sim_hip - sim_fp64| <= 5e-7 (|xn| . |tn|) + 1e-6 |sim_fp64| per compared entry; ids entry by entry,
an entry skipped only where its fp64 gap to a neighbour is below twice that bound, never a top-1 entry, at most 1 % of all.
Beam results against the fixture: the bars of tests/test_hip_parity.py for decode_tiny (same order, ids and lengths, scores
within 1e-4).  Every comparison prints the maximum it measured.

Measured on the MI355X (max |hip - fp64| / bound; entries skipped):
  planted (test 1)         f16x2, bf16, f16 0.317; bf16x3 0.543; f32 0.672 (k = 3 and k = 1 alike); 0 skipped, none allowed
  real prefixes (test 2)   f16x2 0.180 (k = 5: 0 of 3200, k = 8: 0 of 5120 skipped); f32 0.356 (0 of 3200, 0 of 5120)
  past one block (test 6)  0.101, batch-invariant 0.099; 0 of 40 skipped
  explicit tables (test 3) 0.310 at most over the 54 shapes; beam scores against the fixture (test 8) within 1.5e-6
"""
import ctypes as C
import functools
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as nnf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import nearest_def as D                                   # noqa: E402
from capdec_amd import synth                              # noqa: E402

DIMS = synth.GPT2_TINY
V, P = DIMS.vocab, 10
MODES = ["f16x2", "bf16x3", "f32", "bf16", "f16"]
T = torch.from_numpy


class IdTok:
    """the fixture's tokenizer: ``encode`` reads a string of ids ('.' is the stop token), ``decode`` returns the id list"""

    def __init__(self, stop):
        self.stop = stop

    def encode(self, s):
        return [self.stop] if s == "." else [int(w) for w in s.split()]

    def decode(self, ids):
        return [int(i) for i in ids]


@functools.lru_cache(maxsize=None)
def _sd():
    return synth.hot_state_dict(42, "mlp", 512, P, dims=DIMS)


@functools.lru_cache(maxsize=None)
def _wte():
    return _sd()["gpt.transformer.wte.weight"].numpy().copy()


@functools.lru_cache(maxsize=None)
def _real_prefixes(n=64):
    from oracle import capdec_oracle as O
    return O.clip_project(synth.synthetic_clip_embeddings(n, 512, seed=0), _sd(), "mlp", P).reshape(n * P, -1).numpy().copy()


@functools.lru_cache(maxsize=None)
def _planted():
    """64 rows sum_i w_i wte_n[idx_i], w = (1, 0.85, 0.7), scaled by logspace(-3, 3); ids 0 and V-1 in every place"""
    gen = torch.Generator().manual_seed(5)
    idx = np.stack([(torch.randperm(V - 2, generator=gen)[:3] + 1).numpy() for _ in range(64)])
    for place in range(3):
        idx[place, place], idx[3 + place, place] = 0, V - 1
    tn = D.normalize(_wte())
    x = (np.array([1.0, 0.85, 0.7])[None, :, None] * tn[idx]).sum(axis=1) * np.logspace(-3, 3, 64)[:, None]
    return x.astype(np.float32), idx


# ===================================================================================== CPU
REFERENCE_NAMES = {
    "get_prefix_tokens": ["prefix_embed", "embeddings", "tokenizer"],
    "add_embedding_from_text": ["add_in", "prefix_embed", "tokenizer", "model", "where"],
    "generate_text": ["prefix_embed", "tokenizer", "model", "use_beam"],
    "re_caption": ["add_in", "prefix_embed", "tokenizer", "model", "where", "use_beam"],
    "remove_token": ["prefix_embed", "tokenizer", "model", "embeddings", "where", "use_beam"],
    "try_all_places": ["add_in", "prefix_embed", "tokenizer", "model", "use_beam"],
}


def test_abi_surface():
    """the library exports capdec_nearest_tokens; the header's prototype and _capi.SIGNATURES agree; the ABI number stays"""
    from capdec_amd import _capi
    header = open(os.path.join(ROOT, "include", "capdec.h")).read()
    bare = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"\bint\s+capdec_nearest_tokens\s*\(([^;{]*?)\)\s*;", bare, flags=re.S)
    assert m, "include/capdec.h does not declare capdec_nearest_tokens"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    res, args = _capi.SIGNATURES["capdec_nearest_tokens"]
    assert res is C.c_int and len(args) == len(params) == 9
    for p, a in zip(params, args):                      # every int parameter is a c_int, every pointer a void pointer
        assert (a is C.c_int) == (p.startswith("int ") and "*" not in p), (p, a)
    assert re.search(r"#define\s+CAPDEC_ABI_VERSION\s+6\b", header) and _capi.ABI_VERSION == 6
    lib = _capi.load_library()
    assert hasattr(lib, "capdec_nearest_tokens")
    from capdec_amd import build
    assert "nearest.hip" in build.SOURCES


def test_reference_names_and_parameters():
    """gpt2_prefix_eval exports the six functions of reference :201-251 with the reference's parameter names, the batched
    forms, and ClipCaptionModel.get_embedding (which reference :204 calls)"""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd.gpt2_prefix import ClipCaptionModel
    for name, params in REFERENCE_NAMES.items():
        assert list(inspect.signature(getattr(E, name)).parameters) == params, name
    assert inspect.signature(E.re_caption).parameters["use_beam"].default is True
    assert inspect.signature(E.remove_token).parameters["use_beam"].default is True
    assert inspect.signature(E.try_all_places).parameters["use_beam"].default is True
    assert list(inspect.signature(E.prefix_token_ids).parameters) == ["model", "embed", "k"]
    assert list(inspect.signature(E.get_prefix_tokens_batch).parameters) == ["model", "tokenizer", "embed"]
    assert callable(ClipCaptionModel.get_embedding)


def test_definition_vs_reference_formula_and_fixture(golden):
    """nearest_def agrees with the reference's two lines (:248-249 on the table of :259-260) in torch fp32 on the fixture's
    prefixes, and with the ids the reference itself produced.  Pins the checker."""
    g = golden("prefix_tokens_tiny")
    assert synth.state_dict_checksum(_sd()) == int(g["sd_crc"]), "RNG drift"
    pe = g["prefix_embed"]
    emb = nnf.normalize(T(_wte()), 2, 1)
    ids, sims = D.nearest(pe.reshape(-1, pe.shape[-1]), _wte(), 2)
    for r in range(pe.shape[0]):
        sim = torch.einsum('pd,nd->pn', nnf.normalize(T(pe[r]), 2, 1), emb)
        np.testing.assert_array_equal(sim.argmax(-1).numpy(), ids[r * P:(r + 1) * P, 0])
        np.testing.assert_allclose(sim.max(-1).values.numpy(), sims[r * P:(r + 1) * P, 0], atol=2e-6)
    np.testing.assert_array_equal(ids[:, 0].reshape(-1, P), g["prefix_ids"])
    print(f"smallest top-1 gap on the fixture: {float((sims[:, 0] - sims[:, 1]).min()):.2e}")


def test_definition_edges():
    """ties in ascending id order, the zero row, non-finite rows, a non-finite table, and compare()'s own rules"""
    table = np.array([[1.0, 0.0], [0.0, 2.0], [3.0, 0.0], [1.0, 1.0]])
    ids, sims = D.nearest(np.array([[5.0, 0.0], [0.0, 0.0], [np.nan, 1.0], [np.inf, 1.0]]), table, 3)
    assert ids[0].tolist() == [0, 2, 3] and sims[0, 0] == sims[0, 1] == 1.0
    assert ids[1].tolist() == [0, 1, 2] and (sims[1] == 0).all()
    assert (ids[2:] == -1).all() and np.isnan(sims[2:]).all()
    with pytest.raises(ValueError):
        D.nearest(np.ones((1, 2)), np.array([[1.0, np.nan]]), 1)
    x = np.array([[1.0, 0.2], [0.3, 1.0]])
    ids, sims = D.nearest(x, table, 2)
    D.compare(ids, sims, x, table, "self")
    with pytest.raises(AssertionError):
        D.compare(ids[:, ::-1], None, x, table, "swapped")
    with pytest.raises(AssertionError):
        D.compare(ids, sims + 1e-5, x, table, "shifted")


def test_engine_argument_checks():
    """what Engine.nearest_tokens refuses before it reaches the library"""
    from capdec_amd._capi import CapdecError
    from capdec_amd.engine import Engine
    e = Engine.__new__(Engine)
    with pytest.raises(CapdecError, match="table"):
        Engine.nearest_tokens(e, torch.zeros(2, 64), 1, table=torch.zeros(5, 32))
    with pytest.raises(CapdecError, match="integer"):
        Engine.nearest_tokens(e, torch.zeros(2, 64), 1.5)


# ===================================================================================== GPU
@pytest.fixture(scope="module")
def eng():
    from capdec_amd.engine import Engine
    e = Engine(0)
    e.load_gpt2(_sd())
    yield e
    e.close()


def _run(eng, x, k, table=None):
    ids, sims = eng.nearest_tokens(T(np.ascontiguousarray(x)), k, table=None if table is None else T(table), return_sims=True)
    return ids.cpu().numpy(), sims.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_planted_tokens_exact(eng, mode):
    """test 1: the planted ids, in order, at k = 3 and k = 1, in every GEMM mode; no entry may be skipped"""
    x, idx = _planted()
    ref_ids, ref_sims = D.nearest(x, _wte(), 4)
    np.testing.assert_array_equal(ref_ids[:, :3], idx)                 # the input is what it claims to be ...
    gap = float((ref_sims[:, :-1] - ref_sims[:, 1:]).min())
    print(f"smallest adjacent fp64 gap among the first four: {gap:.3f}")
    assert gap > 1e-3                                                  # ... with gaps three orders above the bound
    eng.set_gemm_mode(mode)
    try:
        for k in (3, 1):
            ids, sims = _run(eng, x, k)
            np.testing.assert_array_equal(ids, idx[:, :k])
            worst, skipped, _ = D.compare(ids, sims, x, _wte(), f"planted {mode} k {k}")
            assert skipped == 0
    finally:
        eng.set_gemm_mode("f16x2")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f16x2", "f32"])
def test_real_prefixes(eng, mode):
    """test 2: 64 embeddings through the MLP mapper = 640 prefix rows against the tiny wte, k = 5 and 8"""
    x = _real_prefixes()
    eng.set_gemm_mode(mode)
    try:
        for k in (5, 8):
            ids, sims = _run(eng, x, k)
            D.compare(ids, sims, x, _wte(), f"real prefixes {mode} k {k}")
    finally:
        eng.set_gemm_mode("f16x2")


@pytest.mark.gpu
def test_explicit_tables_and_limits(eng):
    """test 3: table_rows x d x query rows around the tile sizes (d = 96: the native fp32 kernel), k = min(8, table_rows);
    every refusal leaves the context usable"""
    from capdec_amd._capi import CapdecError
    from capdec_amd.engine import Engine
    gen = torch.Generator().manual_seed(11)
    worst = 0.0
    for d in (64, 96, 768):
        for n in (1, 5, 127, 128, 129, 300):
            table = torch.randn(n, d, generator=gen).numpy()
            for rows in (1, 127, 129):
                x = (torch.randn(rows, d, generator=gen) * 3.0).numpy()
                ids, sims = _run(eng, x, min(8, n), table)
                worst = max(worst, D.compare(ids, sims, x, table, f"table {n} x {d}, {rows} rows")[0])
    print(f"explicit tables: max |hip - fp64| / bound {worst:.3f}")
    table, x = torch.randn(5, 64, generator=gen).numpy(), torch.randn(3, 64, generator=gen).numpy()
    for kw, msg in ((dict(k=6), "exceeds"), (dict(k=0), "1..8"), (dict(k=9), "1..8")):
        with pytest.raises(CapdecError, match=msg):
            eng.nearest_tokens(T(x), table=T(table), **kw)
    with pytest.raises(CapdecError, match="multiple of 32"):
        eng.nearest_tokens(torch.zeros(3, 48), 1, table=torch.ones(5, 48))
    with pytest.raises(CapdecError, match="n_embd"):
        eng.nearest_tokens(torch.zeros(3, 64), 1)
    bare = Engine(0)
    try:
        with pytest.raises(CapdecError, match="not loaded"):
            bare.nearest_tokens(torch.zeros(3, 768), 1)
        ids, sims = _run(bare, x, 5, table)
        D.compare(ids, sims, x, table, "after the refusals, context without GPT-2")
    finally:
        bare.close()
    assert eng.nearest_tokens(torch.zeros(0, 768), 3).shape == (0, 3)
    ids, sims = _run(eng, x, 5, table)
    D.compare(ids, sims, x, table, "after the refusals")


@pytest.mark.gpu
def test_ties_in_ascending_id_order(eng):
    """test 4: table rows 7 and 900 identical, the query a multiple of them: ids start [7, 900], the two sims bit-equal"""
    table = _wte().copy()
    table[900] = table[7]
    x = (3.7 * table[7])[None].astype(np.float32)
    emb = nnf.normalize(T(table), 2, 1)
    sim = torch.einsum('pd,nd->pn', nnf.normalize(T(x), 2, 1), emb)
    assert int(sim.argmax(-1)[0]) == 7                                 # torch's own arg-max takes the lower id too
    for k in (2, 5):
        ids, sims = _run(eng, x, k, table)
        assert ids[0, :2].tolist() == [7, 900]
        assert sims[0, 0].tobytes() == sims[0, 1].tobytes() and abs(float(sims[0, 0]) - 1.0) < 2e-6
        D.compare(ids, sims, x, table, f"ties k {k}")


@pytest.mark.gpu
def test_special_rows(eng):
    """test 5: the zero row; a NaN row and an inf row get -1 / NaN and leave their neighbours alone; a zero table row has
    sim 0; a table with a NaN row is refused and nothing is written"""
    from capdec_amd._capi import CapdecError
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(9, 768, generator=gen).numpy()
    x[2] = 0.0
    x[4, 100] = np.nan
    x[6, 767] = -np.inf
    k = 4
    ids, sims = _run(eng, x, k)
    D.compare(ids, sims, x, _wte(), "special rows")
    assert ids[2].tolist() == [0, 1, 2, 3] and (sims[2] == 0).all()
    assert (ids[[4, 6]] == -1).all() and np.isnan(sims[[4, 6]]).all()
    clean = np.delete(x, [4, 6], axis=0)
    ids2, sims2 = _run(eng, clean, k)
    np.testing.assert_array_equal(np.delete(ids, [4, 6], axis=0), ids2)
    np.testing.assert_array_equal(np.delete(sims, [4, 6], axis=0), sims2)
    q = torch.randn(1, 64, generator=gen).numpy()                      # every other table row points away from the query:
    small = -q * np.arange(1, 6)[:, None] + 0.05 * torch.randn(5, 64, generator=gen).numpy()
    small[1] = 0.0                                                     # the zero row's sim 0 is the largest
    ids, sims = _run(eng, q, 3, small)
    D.compare(ids, sims, q, small, "zero table row")
    assert ids[0, 0] == 1 and sims[0, 0] == 0.0 and sims[0, 1] < -0.9
    table = _wte()[:300].copy()
    table[40, 5] = np.nan
    t, xs = T(table).cuda(), T(x).cuda()
    out_i = torch.full((9, k), -7, dtype=torch.int32, device="cuda")
    out_s = torch.full((9, k), -7.0, dtype=torch.float32, device="cuda")
    eng._sync_stream()
    rc = eng.lib.capdec_nearest_tokens(eng._h, xs.data_ptr(), 9, 768, t.data_ptr(), 300, k, out_i.data_ptr(), out_s.data_ptr())
    assert rc != 0 and b"table row" in eng.lib.capdec_last_error()
    torch.cuda.synchronize()
    assert (out_i.cpu() == -7).all() and (out_s.cpu() == -7.0).all()
    with pytest.raises(CapdecError, match="table row"):
        eng.nearest_tokens(xs, k, table=t)
    ids, sims = _run(eng, x, k)                                        # the context is still usable
    D.compare(ids, sims, x, _wte(), "after the refused table")


@pytest.mark.gpu
def test_past_one_block(eng):
    """test 6: 16 384 + 130 rows against the tiny wte, k = 5 -- the wide tile, a second block, a ragged last row tile; with
    batch-invariant mode on, eight rows run alone are bit-identical to their results inside the batch"""
    rows, k = 16384 + 130, 5
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(rows, 768, generator=gen).numpy()
    pick = np.array([0, 127, 128, 2047, 2048, 16383, 16384, rows - 1])
    ids, sims = _run(eng, x, k)
    D.compare(ids[pick], sims[pick], x[pick], _wte(), "past one block")
    eng.set_batch_invariant(True)
    try:
        ids_b, sims_b = _run(eng, x, k)
        D.compare(ids_b[pick], sims_b[pick], x[pick], _wte(), "past one block, batch-invariant")
        ids_a, sims_a = _run(eng, x[pick], k)
        np.testing.assert_array_equal(ids_a, ids_b[pick])
        assert sims_a.tobytes() == sims_b[pick].tobytes()
        one_i, one_s = _run(eng, x[16384:16385], k)
        assert one_i.tobytes() == ids_b[16384:16385].tobytes() and one_s.tobytes() == sims_b[16384:16385].tobytes()
    finally:
        eng.set_batch_invariant(False)


@pytest.mark.gpu
def test_cache_follows_the_weights(golden):
    """test 7: the cached normalised wte equals the explicit table; it follows capdec_load_gpt2 and a full-scope train step"""
    from capdec_amd import train as Tr
    from capdec_amd.engine import Engine
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    x, k = _real_prefixes()[:130], 5
    e = Engine(0)
    try:
        e.load_gpt2(_sd())
        ids, sims = _run(e, x, k)
        ids_t, sims_t = _run(e, x, k, _wte())
        np.testing.assert_array_equal(ids, ids_t)
        D.compare(ids, sims, x, _wte(), "cached wte")
        D.compare(ids_t, sims_t, x, _wte(), "wte as a table")
        other = synth.hot_gpt2_state_dict(7, DIMS)
        e.load_gpt2(other)
        w7 = other["gpt.transformer.wte.weight"].numpy()
        ids7, sims7 = _run(e, x, k)
        D.compare(ids7, sims7, x, w7, "after load_gpt2 with another seed")
        assert not np.array_equal(ids7, ids)
    finally:
        e.close()
    g = golden("train_full_tiny")
    model = ClipCaptionModel(P, clip_length=10, prefix_size=512, num_layers=8, mapping_type=MappingType.MLP,
                             gpt2_dims=DIMS).to("cuda:0")
    model.load_state_dict(_sd())
    model.train()
    model.gpt.config.resid_pdrop = model.gpt.config.embd_pdrop = model.gpt.config.attn_pdrop = 0.0
    before_i, before_s = _run(model.engine, x, k)
    D.compare(before_i, before_s, x, _wte(), "before the train step")
    opt = Tr.AdamW(model.parameters(), lr=1e-3)
    Tr.train_step(model, opt, T(g["tokens"]), T(g["mask"]), T(g["prefix"]))
    after_i, after_s = _run(model.engine, x, k)
    w = model.state_dict()["gpt.transformer.wte.weight"].numpy()
    assert not np.array_equal(w, _wte())
    D.compare(after_i, after_s, x, w, "after the train step")
    tab_i, _ = _run(model.engine, x, k, w)
    np.testing.assert_array_equal(after_i, tab_i)
    assert after_s.tobytes() != before_s.tobytes()
    model.release()


def _beam_matches(E, model, prefix, stop, g, name, i):
    ids, lens, scores, order = (t.cpu().numpy()[0] for t in E.decode_beam_ids(model, prefix, stop, 5, 67))
    go = g[f"{name}_beam_order"][i]
    np.testing.assert_array_equal(order, go)
    np.testing.assert_array_equal(ids, g[f"{name}_beam_tokens"][i][go])
    np.testing.assert_array_equal(lens, g[f"{name}_beam_seqlen"][i][go].astype(np.int32))
    err = float(np.abs(scores - g[f"{name}_beam_scores"][i][go]).max())
    assert err <= 1e-4
    return err, [int(t) for t in ids[0, :int(lens[0])]]


@pytest.mark.gpu
def test_python_surface_vs_reference_fixture(golden):
    """test 8: the reference's functions on the fixture's prefixes"""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    g = golden("prefix_tokens_tiny")
    model = ClipCaptionModel(P, clip_length=10, prefix_dim=512, num_layers=8, mapping_type=MappingType.MLP,
                             gpt2_dims=DIMS).to("cuda:0").eval()
    model.load_state_dict(_sd())
    assert synth.state_dict_checksum(_sd()) == int(g["sd_crc"]), "RNG drift"
    pe = T(g["prefix_embed"]).cuda()
    n = pe.shape[0]
    stop, add_in = int(g["stop_id"]), " ".join(str(int(t)) for t in g["add_in"])
    m = len(g["add_in"])
    tok = IdTok(stop)
    emb = nnf.normalize(T(_wte()), 2, 1).cuda()
    # ---- prefix tokens: the model (cached wte) and a tensor as `embeddings`; the batched forms
    for r in range(n):
        assert E.get_prefix_tokens(pe[r:r + 1], model, tok) == g["prefix_ids"][r].tolist()
        assert E.get_prefix_tokens(pe[r:r + 1], emb, tok) == g["prefix_ids"][r].tolist()
    assert E.get_prefix_tokens_batch(model, tok, pe) == g["prefix_ids"].tolist()
    ids, sims = E.prefix_token_ids(model, pe, 3)
    assert ids.shape == (n, P, 3) and sims.shape == (n, P, 3) and ids.dtype == torch.int32
    np.testing.assert_array_equal(ids[..., 0].cpu().numpy(), g["prefix_ids"])
    D.compare(ids.reshape(-1, 3).cpu().numpy(), sims.reshape(-1, 3).cpu().numpy(), g["prefix_embed"].reshape(n * P, -1), _wte(),
              "prefix_token_ids")
    # ---- add_embedding_from_text: the reference's cat at every kind of position
    rows = model.engine.wte(T(g["add_in"])).unsqueeze(0)
    assert torch.equal(model.get_embedding(T(g["add_in"]).cuda()), rows[0])
    for where, want in ((0, torch.cat((rows, pe[:1]), 1)), (3, torch.cat((pe[:1, :3], rows, pe[:1, 3:]), 1)),
                        (-1, torch.cat((pe[:1], rows), 1)), (P, torch.cat((pe[:1], rows), 1))):
        got = E.add_embedding_from_text(add_in, pe[:1], tok, model, where)
        assert got.shape == (1, P + m, DIMS.n_embd) and torch.equal(got, want), where
    # ---- remove_token
    removed = [int(v) for v in g["removed"]]
    keep = [i for i in range(P) if i not in removed]
    worst = 0.0
    for r in range(n):
        text, sent = E.remove_token(pe[r:r + 1], tok, model, emb, removed, use_beam=False)
        assert sent == g["remove_sent"][r].tolist()
        assert E.remove_token(pe[r:r + 1], tok, model, model, removed, use_beam=False)[1] == sent
        assert text == g["remove_greedy_ids"][r][:int(g["remove_greedy_lens"][r])].tolist()
        err, best = _beam_matches(E, model, pe[r:r + 1, keep], stop, g, "remove", r)
        worst = max(worst, err)
        assert E.remove_token(pe[r:r + 1], tok, model, emb, removed)[0] == best
    # ---- re_caption
    i = 0
    for r in g["recap_rows"]:
        for where in g["recap_where"]:
            r, where = int(r), int(where)
            assert E.re_caption(add_in, pe[r:r + 1], tok, model, where, use_beam=False) == \
                g["recap_greedy_ids"][i][:int(g["recap_greedy_lens"][i])].tolist()
            err, best = _beam_matches(E, model, E.add_embedding_from_text(add_in, pe[r:r + 1], tok, model, where), stop, g,
                                      "recap", i)
            worst = max(worst, err)
            assert E.re_caption(add_in, pe[r:r + 1], tok, model, where) == best
            i += 1
    # ---- try_all_places: one decode call for the P places
    calls = []
    greedy, beam = model.engine.decode_greedy, model.engine.decode_beam
    model.engine.decode_greedy = lambda *a, **kw: (calls.append("greedy"), greedy(*a, **kw))[1]
    model.engine.decode_beam = lambda *a, **kw: (calls.append("beam"), beam(*a, **kw))[1]
    try:
        for j, r in enumerate(int(v) for v in g["places_rows"]):
            del calls[:]
            lens = g["places_greedy_lens"][j * P:(j + 1) * P]
            got = E.try_all_places(add_in, pe[r:r + 1], tok, model, use_beam=False)
            st = model.engine.decode_stats()
            assert calls == ["greedy"]
            assert got == [g["places_greedy_ids"][j * P + i][:int(lens[i])].tolist() for i in range(P)]
            # ONE call carried all P captions: after the prefill, caption i stays in the batch for its len - 1 steps at least
            assert st["steps"] <= 67 and st["row_steps"] >= int(lens.sum()) - P > 67
            del calls[:]
            got = E.try_all_places(add_in, pe[r:r + 1], tok, model)
            assert calls == ["beam"]
            for i in range(P):
                err, best = _beam_matches(E, model, E.add_embedding_from_text(add_in, pe[r:r + 1], tok, model, i), stop, g,
                                          "places", j * P + i)
                worst = max(worst, err)
                assert got[i] == best
    finally:
        model.engine.decode_greedy, model.engine.decode_beam = greedy, beam
    print(f"beam scores vs the fixture: max |hip - reference| {worst:.2e} (bar 1e-4)")
    # ---- batch-invariant mode: the batched decode is the P single decodes
    model.engine.set_batch_invariant(True)
    try:
        for use_beam in (False, True):
            assert E.try_all_places(add_in, pe[5:6], tok, model, use_beam) == \
                [E.re_caption(add_in, pe[5:6], tok, model, i, use_beam) for i in range(P)]
    finally:
        model.engine.set_batch_invariant(False)
    model.release()
