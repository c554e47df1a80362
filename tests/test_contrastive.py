"""Contrastive search (``capdec_decode_contrastive``; ``Engine.decode_contrastive``; ``generate_contrastive*``) against the
CPU definition of its contract in tests/contrastive_def.py.

Bounds.  A caption must match the definition exactly -- tokens and lengths; the trace (p, sim of every chosen candidate)
within 1e-4, the project's beam-score bound -- unless its margin is below GAP = 1e-4: the smallest, over its live steps, of
(best - second best score) and of the smallest gap between adjacent logits among the best K + 1.  Below it a decision may
fall either way, so such a caption may differ from the first near-tie step on (everything before it must still match).  At
most 2 of a case's 16 captions may be below the margin -- asserted on the CPU for the definition alone -- and at least 14
of 16 must be identical on the GPU.  penalty_alpha = 0 and top_k = 1 must give greedy's tokens.
"""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import contrastive_def as CD
import process_def as PD
from capdec_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 1e-4
UNCLEAR_CAP = 2               # captions of 16 whose margin may be below GAP
TRACE_TOL = 1e-4
P, T12 = 10, 12
DIMS = {"tiny": synth.GPT2_TINY, "small": synth.GPT2_SMALL}
PROC = dict(theta=1.3, m=2, min_len=4)

#: name -> (top_k, penalty_alpha, processors); tiny geometry, seed 42 hot weights, P 10, T 12, 16 captions, stop id 744
CASES = {
    "k4": (4, 0.6, None),
    "k8": (8, 0.6, None),
    "k5": (5, 0.3, None),
    "k4_proc": (4, 0.6, PROC),
}


# ------------------------------------------------------------------------------------- cases (computed once, shared)
@functools.lru_cache(maxsize=None)
def _weights(geom):
    return synth.hot_state_dict(42, "mlp", 512, P, dims=DIMS[geom])


@functools.lru_cache(maxsize=None)
def _prefix(geom, n):
    from oracle import capdec_oracle as O
    x = synth.synthetic_clip_embeddings(n, 512, seed=0)
    return O.clip_project(x, _weights(geom), "mlp", P).reshape(n, P, -1)


@functools.lru_cache(maxsize=None)
def _greedy_def(stop):
    dims, sd, prefix = DIMS["tiny"], _weights("tiny"), _prefix("tiny", 32)[:16].contiguous()
    return PD.greedy(sd, prefix, PD.Proc(), stop, T12, -1, dims.n_head)


@functools.lru_cache(maxsize=None)
def _stop():
    """the token the unprocessed greedy run of all 32 prefixes (definition, nothing stops) emits most often in its first
    three steps, as test_diverse_beam.py chooses it: 744"""
    dims = DIMS["tiny"]
    ids = PD.greedy(_weights("tiny"), _prefix("tiny", 32), PD.Proc(), dims.vocab + 5, T12, -1, dims.n_head)[0]
    return int(np.bincount(ids[:, :3].reshape(-1)).argmax())


def _tiny_case():
    """-> dims, weights, 16 prefixes (the first 16 of synthetic_clip_embeddings(32, 512, seed=0)), stop id"""
    return DIMS["tiny"], _weights("tiny"), _prefix("tiny", 32)[:16].contiguous(), _stop()


@functools.lru_cache(maxsize=None)
def _tiny_def(K, alpha, proc=False, dtype=torch.float32, stops=True):
    dims, sd, prefix, stop = _tiny_case()
    p = PD.Proc(**PROC) if proc else PD.Proc()
    return CD.contrastive(sd, prefix, p, K, alpha, stop if stops else -1, T12, n_head=dims.n_head, dtype=dtype)


# ===================================================================================== CPU: the definition
def test_alpha_zero_and_one_candidate_are_greedy():
    """penalty_alpha = 0 (K 4) and K = 1 (alpha 0.6) give process_def.greedy's ids and lens exactly, with and without
    processors"""
    dims, sd, prefix, stop = _tiny_case()
    assert stop == 744
    for p in (PD.Proc(), PD.Proc(**PROC)):
        ids, lens, _ = PD.greedy(sd, prefix, p, stop, T12, -1, dims.n_head)
        for K, alpha in ((4, 0.0), (1, 0.6)):
            r = CD.contrastive(sd, prefix, p, K, alpha, stop, T12, n_head=dims.n_head)
            np.testing.assert_array_equal(r.ids, ids)
            np.testing.assert_array_equal(r.lens, lens)
            assert (r.picks[r.picks >= 0] == 0).all()


@pytest.mark.parametrize("name", list(CASES))
def test_margin_cap_and_float64(name):
    """the GPU comparison keeps something to assert: at most 2 of a case's 16 captions have a margin below 1e-4, and the
    fp32 and float64 runs of the definition give identical ids.  Measured (definition alone; captions below 1e-4 / smallest
    margin / non-top-1 winners of decisions / max |trace fp32 - fp64|): k4 0 / 9.8e-4 / 32 of 158 / 4.8e-6; k8 0 / 3.6e-4 /
    33 of 156 / 4.8e-6; k5 0 / 1.4e-3 / 9 of 157 / 4.8e-6; k4_proc 0 / 3.9e-4 / 26 of 182 / 4.9e-6.  And the feature acts:
    with nothing stopping, (K 4, alpha 0.6) picks a candidate other than the most probable one in at least 20 of its 192
    decisions (measured 40; distinct tokens per caption 10.8 against greedy's 8.25)."""
    K, alpha, proc = CASES[name]
    r = _tiny_def(K, alpha, proc is not None)
    r64 = _tiny_def(K, alpha, proc is not None, torch.float64)
    unclear = int((r.margin < GAP).sum())
    print(f"definition {name}: smallest margin {r.margin.min():.2e}, captions below {GAP:g}: {unclear} of 16, non-top-1 "
          f"winners {int((r.picks > 0).sum())} of {int((r.picks >= 0).sum())}, max |trace fp32 - fp64| "
          f"{np.abs(r.trace - r64.trace).max():.2e}")
    np.testing.assert_array_equal(r.ids, r64.ids)
    np.testing.assert_array_equal(r.lens, r64.lens)
    assert np.abs(r.trace - r64.trace).max() < TRACE_TOL / 4
    assert unclear <= UNCLEAR_CAP, unclear
    stop = _stop()
    for i in range(16):
        L = int(r.lens[i])
        assert 1 <= L <= T12 and (L == T12 or r.ids[i, L - 1] == stop) and stop not in r.ids[i, :L - 1], (i, r.ids[i])
        assert (r.ids[i, L:] == 0).all() and (r.picks[i, :L] >= 0).all() and (r.picks[i, :L] < K).all()
        if proc is not None:
            assert L == T12 or L > PROC["min_len"]
            grams = [tuple(r.ids[i, k:k + 2]) for k in range(L - 1)]
            assert len(grams) == len(set(grams)), (i, r.ids[i])
    if name == "k4":
        assert sorted(r.lens.tolist())[:6] == [1, 3, 5, 8, 10, 11] and int((r.lens < T12).sum()) == 6
        free = _tiny_def(4, 0.6, False, torch.float32, False)
        g = _greedy_def(-1)
        acts = int((free.picks > 0).sum())
        print(f"definition k4, nothing stops: non-top-1 winners {acts} of {int((free.picks >= 0).sum())}, distinct tokens "
              f"per caption {CD.distinct_tokens(free.ids, free.lens):.2f} (greedy {CD.distinct_tokens(g[0], g[1]):.2f})")
        assert int((free.picks >= 0).sum()) == 192 and acts >= 20, acts
        assert CD.distinct_tokens(free.ids, free.lens) > CD.distinct_tokens(g[0], g[1])


# ===================================================================================== CPU: header, binding, arguments
def test_header_and_binding():
    from capdec_amd import _capi
    header = open(os.path.join(ROOT, "include", "capdec.h")).read()
    m = re.search(r"\bint\s+capdec_decode_contrastive\s*\(([^;]*)\)\s*;", header)
    assert m, "prototype missing"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "d_prefix", "n", "P", "top_k", "penalty_alpha", "stop_id",
                                                         "alt_stop_id", "entry_length", "d_ids", "d_lens", "d_trace"]
    assert re.search(r"#define\s+CAPDEC_ABI_VERSION\s+6\b", header) and _capi.ABI_VERSION == 6
    res, argtypes = _capi.SIGNATURES["capdec_decode_contrastive"]
    want = []
    for a in args:                                              # the ctypes signature, argument by argument
        want.append(C.c_void_p if "*" in a else C.c_float if a.startswith("float") else C.c_int)
    assert res is C.c_int and argtypes == want
    lib = _capi.load_library()
    assert hasattr(lib, "capdec_decode_contrastive") and lib.capdec_abi_version() == 6
    assert lib.capdec_decode_contrastive(None, None, 1, 10, 4, 0.6, 13, -1, 12, None, None, None) != 0
    assert b"decode_contrastive" in lib.capdec_last_error()
    for word in ("penalty_alpha", "score_c = (1 - a) * p_c - a * sim_c", "tie going to the lower c", "top_k\n * outside 1..8",
                 "head_dim other than 64"):
        assert word in header, word
    from capdec_amd import build
    assert "contrastive.hip" in build.SOURCES


class _Untouchable:
    """a library / handle that fails the test when anything reaches it"""

    def __getattr__(self, name):
        raise AssertionError(f"the refused call reached the library: {name}")


def test_argument_checks():
    """the façade's refusals come before anything touches the device or the context's processor state"""
    from capdec_amd._capi import CapdecError
    from capdec_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.lib, e._h = _Untouchable(), None
    pe = torch.zeros(2, P, 8)
    for kw in (dict(top_k=0), dict(top_k=9), dict(top_k=-1), dict(top_k=4.0), dict(top_k=True), dict(top_k="4"),
               dict(penalty_alpha=-0.1), dict(penalty_alpha=1.01), dict(penalty_alpha=float("nan")),
               dict(penalty_alpha=float("inf")), dict(penalty_alpha="0.6"), dict(penalty_alpha=None),
               dict(entry_length=0), dict(entry_length=12.0)):
        with pytest.raises(CapdecError):
            Engine.decode_contrastive(e, pe, **dict(dict(top_k=4, penalty_alpha=0.6, stop_id=13), **kw), repetition_penalty=1.3)
    seen = []
    e._decode_contrastive = lambda *a: seen.append(a[1:]) or "D"
    assert Engine.decode_contrastive(e, pe, 4, 0.6, 13, -1, 12) == "D" and seen == [(4, 0.6, 13, -1, 12, False)]
    assert Engine.decode_contrastive(e, pe, 1, 0, 13, 764, 12, True) == "D" and seen[-1] == (1, 0.0, 13, 764, 12, True)
    assert Engine.decode_contrastive(e, pe, np.int64(8), 1, 13) == "D" and seen[-1] == (8, 1.0, 13, -1, 67, False)


def test_python_surface():
    """the new functions and their defaults; generate2 / generate2_batch / generate_beam keep their signatures"""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd.engine import Engine
    sig = inspect.signature(Engine.decode_contrastive).parameters
    assert list(sig)[:8] == ["self", "prefix_embed", "top_k", "penalty_alpha", "stop_id", "alt_stop_id", "entry_length",
                             "return_trace"]
    assert (sig["top_k"].default, sig["penalty_alpha"].default, sig["alt_stop_id"].default, sig["entry_length"].default,
            sig["return_trace"].default) == (4, 0.6, -1, 67, False)
    for fn in (Engine.decode_contrastive, E.decode_contrastive_ids, E.generate_contrastive_batch):
        s = inspect.signature(fn).parameters
        for name in ("repetition_penalty", "no_repeat_ngram_size", "min_length", "logit_bias"):
            assert s[name].kind is inspect.Parameter.KEYWORD_ONLY and s[name].default is None, (fn.__name__, name)
    g = inspect.signature(E.generate_contrastive).parameters
    assert list(g) == ["model", "tokenizer", "tokens", "prompt", "embed", "entry_length", "top_k", "penalty_alpha", "stop_token"]
    assert (g["entry_length"].default, g["top_k"].default, g["penalty_alpha"].default, g["stop_token"].default) == (67, 4, 0.6, ".")
    assert list(inspect.signature(E.generate_contrastive_batch).parameters)[:7] == [
        "model", "tokenizer", "embed", "entry_length", "top_k", "penalty_alpha", "stop_token"]
    assert list(inspect.signature(E.generate2).parameters) == ["model", "tokenizer", "tokens", "prompt", "embed", "entry_count",
                                                               "entry_length", "top_p", "temperature", "stop_token"]
    assert list(inspect.signature(E.generate_beam).parameters) == ["model", "tokenizer", "beam_size", "prompt", "embed",
                                                                   "entry_length", "temperature", "stop_token"]


# ===================================================================================== GPU
@pytest.fixture(scope="module")
def eng():
    from capdec_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _vs_definition(got, want, rows, what):
    """captions `rows` of a HIP result (ids, lens, trace) against the definition's Result for those captions: a caption at or
    above the margin must be identical, one below it must match up to its first near-tie step -> (identical, differ on a
    near-tie)"""
    ids, lens, trace = got
    same = skipped = 0
    worst = 0.0
    for j, r in enumerate(rows):
        L = int(want.lens[j])
        eq = np.array_equal(ids[r], want.ids[j]) and lens[r] == L
        if eq:
            err = float(np.abs(trace[r] - want.trace[j]).max())
            assert err <= TRACE_TOL, (what, r, err)
            assert (trace[r, L:] == 0).all()
            worst = max(worst, err)
            same += 1
            continue
        assert want.margin[j] < GAP, (what, r, ids[r], want.ids[j], lens[r], L, want.margin[j])
        t0 = int(np.nonzero(want.step_margin[j] < GAP)[0][0])          # everything before the first near tie still matches
        np.testing.assert_array_equal(ids[r, :t0], want.ids[j, :t0])
        assert lens[r] > t0 and np.abs(trace[r, :t0] - want.trace[j, :t0]).max(initial=0.0) <= TRACE_TOL
        skipped += 1
    print(f"{what}: {len(rows)} captions, {same} identical ({int((want.margin < GAP).sum())} had a margin < {GAP:g}), {skipped} "
          f"differ from such a tie on; max |trace - def| {worst:.2e}")
    return same, skipped


def _check_structure(ids, lens, T, stops):
    for r in range(ids.shape[0]):
        L = int(lens[r])
        assert 1 <= L <= T and (ids[r, L:] == 0).all(), (r, ids[r])
        assert not any(s in ids[r, :L - 1] for s in stops) and (L == T or ids[r, L - 1] in stops), (r, ids[r])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_vs_definition(eng, name):
    """tiny geometry, T 12, 16 captions, stop id 744: ids and lens are the definition's for every caption with a margin of
    at least 1e-4, the trace within 1e-4; at least 14 of 16 identical.  Measured on an MI355X: 16 of 16 identical in every case;
    max |trace - def| k4 3.6e-6, k8 3.6e-6, k5 3.2e-6, k4_proc 3.4e-6"""
    K, alpha, proc = CASES[name]
    dims, sd, prefix, stop = _tiny_case()
    eng.load_gpt2(sd, n_head=dims.n_head)
    kw = PD.Proc(**proc).kw() if proc else {}
    got = _np(eng.decode_contrastive(prefix, K, alpha, stop, -1, T12, True, **kw))
    _check_structure(got[0], got[1], T12, [stop])
    same, skipped = _vs_definition(got, _tiny_def(K, alpha, proc is not None), list(range(16)), f"hip contrastive {name}")
    assert same + skipped == 16 and same >= 14, (same, skipped)


@pytest.mark.gpu
@pytest.mark.parametrize("K,alpha", [(4, 0.0), (1, 0.6)])
def test_greedy_equivalence(eng, K, alpha):
    """penalty_alpha = 0 and top_k = 1 give capdec_decode_greedy's ids and lens on the same engine; a caption whose greedy
    top-2 logit gap (definition) came below 1e-4 at some step may differ from that step on"""
    dims, sd, prefix, stop = _tiny_case()
    eng.load_gpt2(sd, n_head=dims.n_head)
    gi, gl = _np(eng.decode_greedy(prefix, stop, T12, -1))
    ci, cl, tr = _np(eng.decode_contrastive(prefix, K, alpha, stop, -1, T12, True))
    gaps = _greedy_def(stop)[2]
    same = 0
    for r in range(16):
        if np.array_equal(ci[r], gi[r]) and cl[r] == gl[r]:
            same += 1
            continue
        assert gaps[r].min() < GAP, (r, ci[r], gi[r], gaps[r].min())
        t0 = int(np.nonzero(gaps[r] < GAP)[0][0])
        np.testing.assert_array_equal(ci[r, :t0], gi[r, :t0])
    assert same >= 14, same
    assert np.isfinite(tr).all() and (tr[..., 0] >= 0).all() and (tr[..., 0] <= 1).all() and (np.abs(tr[..., 1]) <= 1 + 1e-5).all()


@pytest.mark.gpu
def test_captions_that_stop_and_compaction(eng):
    """stop id 744, K 4: the definition's lengths are 1..12 and six captions stop early.  ids and lens equal the
    definition; compaction on and off give identical results; with it on the launches shrink (capdec_decode_stats /
    capdec_decode_step_rows), with it off every step carries all 64 rows"""
    dims, sd, prefix, stop = _tiny_case()
    eng.load_gpt2(sd, n_head=dims.n_head)
    want = _tiny_def(4, 0.6)
    assert int((want.lens < T12).sum()) == 6 and want.lens.min() == 1 and want.lens.max() == T12
    try:
        eng.set_compact(True)
        on = _np(eng.decode_contrastive(prefix, 4, 0.6, stop, -1, T12, True))
        st, rows = eng.decode_stats(), eng.decode_step_rows()
        assert st["steps"] == T12 and st["compactions"] >= 1 and len(rows) == T12, (st, rows)
        assert rows[0] == 64 and rows[-1] < 64 and all(a >= b for a, b in zip(rows, rows[1:])), rows
        assert st["row_steps"] == sum(rows) < 64 * T12
        eng.set_compact(False)
        off = _np(eng.decode_contrastive(prefix, 4, 0.6, stop, -1, T12, True))
        st, rows = eng.decode_stats(), eng.decode_step_rows()
        assert st["compactions"] == 0 and rows == [64] * T12 and st["row_steps"] == 64 * T12, (st, rows)
    finally:
        eng.set_compact(True)
    for a, b in zip(on, off):
        np.testing.assert_array_equal(a, b)
    same, skipped = _vs_definition(on, want, list(range(16)), "hip contrastive, captions that stop")
    assert same + skipped == 16 and same >= 14
    np.testing.assert_array_equal(on[1][want.margin >= GAP], want.lens[want.margin >= GAP])


@pytest.mark.gpu
def test_chunking_and_single_captions():
    """batch-invariant mode and a KV budget that holds 6 captions (their K/V and their hidden-state history): the 16
    captions run as 3 chunks, and their ids, lens and trace are those of the one-chunk run and of every caption decoded
    alone"""
    from capdec_amd import _capi
    from capdec_amd.engine import Engine
    dims, sd, prefix, stop = _tiny_case()
    K, alpha = 4, 0.6
    e = Engine(0)
    try:
        e.load_gpt2(sd, n_head=dims.n_head)
        e.set_batch_invariant(True)
        run = lambda x: _np(e.decode_contrastive(x, K, alpha, stop, -1, T12, True))
        res = run(prefix)
        assert e.decode_chunks() == 1
        ctx = P + T12
        per_cap = K * ctx * dims.n_embd * 2 * 4 * dims.n_layer + ctx * dims.n_embd * 4
        _capi.check(e.lib.capdec_set_kv_budget(e._h, per_cap * 6 + per_cap // 2), "budget")
        chunked = run(prefix)
        assert e.decode_chunks() == 3
        for a, b in zip(chunked, res):
            np.testing.assert_array_equal(a, b)
        for r in range(16):
            one = run(prefix[r:r + 1].contiguous())
            for a, b in zip(one, res):
                np.testing.assert_array_equal(a[0], b[r])
        same, skipped = _vs_definition(res, _tiny_def(K, alpha), list(range(16)), "hip contrastive, batch-invariant")
        assert same + skipped == 16 and same >= 14
    finally:
        e.close()


@functools.lru_cache(maxsize=None)
def _long_def():
    dims, sd = DIMS["tiny"], _weights("tiny")
    return CD.contrastive(sd, _prefix("tiny", 32)[:2].contiguous(), PD.Proc(), 4, 0.6, -1, 101, n_head=dims.n_head)


@pytest.mark.gpu
def test_history_tile_boundaries(eng):
    """2 captions, P 10, T 101, nothing stops: the position fed crosses 63 / 64 / 65 and reaches 110 (tiny's n_positions is
    128), so the selection's history loop runs every remainder of its four-row tiles.  Against the definition, with the
    near-tie rule per caption.  Measured: smallest margins of the two captions 7.3e-4 and 1.6e-4 (no step below 1e-4),
    both identical to the definition on an MI355X, max |trace - def| 3.2e-6"""
    dims, sd = DIMS["tiny"], _weights("tiny")
    prefix = _prefix("tiny", 32)[:2].contiguous()
    eng.load_gpt2(sd, n_head=dims.n_head)
    want = _long_def()
    assert (want.lens == 101).all()
    print("definition, T 101: margins", want.margin, "first near ties", [np.nonzero(m < GAP)[0][:1] for m in want.step_margin])
    got = _np(eng.decode_contrastive(prefix, 4, 0.6, -1, -1, 101, True))
    assert (got[1] == 101).all()
    same, skipped = _vs_definition(got, want, [0, 1], "hip contrastive, 101 steps")
    assert same + skipped == 2


@functools.lru_cache(maxsize=None)
def _small_def():
    dims, sd = DIMS["small"], _weights("small")
    return CD.contrastive(sd, _prefix("small", 8)[:4].contiguous(), PD.Proc(), 4, 0.6, -1, T12, n_head=dims.n_head)


@pytest.mark.gpu
def test_real_vocabulary(eng):
    """GPT-2 small's geometry (12 layers, V = 50257: the fused lm_head's 393 tiles feed the candidate lists), 4 captions,
    K 4, T 12, nothing stops.  Measured: smallest margin 1.0e-3, 4 of 4 identical, max |trace - def| 6.2e-6"""
    dims, sd = DIMS["small"], _weights("small")
    prefix = _prefix("small", 8)[:4].contiguous()
    eng.load_gpt2(sd, n_head=dims.n_head)
    got = _np(eng.decode_contrastive(prefix, 4, 0.6, -1, -1, T12, True))
    same, skipped = _vs_definition(got, _small_def(), list(range(4)), "hip contrastive, small geometry")
    assert same + skipped == 4


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(golden):
    """top_k outside 1..8, penalty_alpha outside [0, 1] or not finite, a context one position too long (greedy still takes
    it) and a head_dim other than 64 (already at load_gpt2; the decode call keeps its own check behind it) are refused on the
    host through capdec_last_error; the next greedy decode matches its fixture"""
    from capdec_amd import _capi
    from capdec_amd.engine import Engine
    g, dims = golden("decode_tiny"), synth.GPT2_TINY
    sd = synth.hot_state_dict(42, "mlp", 640, 10, dims=dims)
    pe, stop = torch.from_numpy(g["greedy_prefix_embed"]), int(g["greedy_stop_id"])
    e = Engine(0)
    try:
        e.load_gpt2(sd, n_head=dims.n_head)
        raw = lambda K, a, T=12: e._decode_contrastive(pe, K, a, stop, 764, T, False)
        for K in (0, 9, -1):
            with pytest.raises(_capi.CapdecError, match="top_k"):
                raw(K, 0.6)
        for a in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(_capi.CapdecError, match="penalty_alpha"):
                raw(4, a)
        T_long = dims.n_pos - 10 + 1
        with pytest.raises(_capi.CapdecError, match="n_positions"):
            raw(4, 0.6, T_long)
        e.decode_greedy(pe, stop, T_long, 764)                  # greedy needs one position less
        raw(4, 0.6, T_long - 1)
        with pytest.raises(_capi.CapdecError, match="head_dim"):     # refused where the geometry enters: the loader
            e.load_gpt2(sd, n_head=6)
        e.load_gpt2(sd, n_head=dims.n_head)
        gi, gl = e.decode_greedy(pe, stop, 12, 764)
        np.testing.assert_array_equal(gi.cpu().numpy(), g["greedy_ids_T12"])
        np.testing.assert_array_equal(gl.cpu().numpy(), g["greedy_lens_T12"])
        ids, lens = _np(raw(4, 0.6))
        _check_structure(ids, lens, 12, [stop, 764])
    finally:
        e.close()


@pytest.mark.gpu
def test_bf16_mode_runs():
    """bf16 GEMM operands and KV cache: the call runs, lengths are valid, the trace is finite (not compared)"""
    from capdec_amd.engine import Engine
    dims, sd, prefix, stop = _tiny_case()
    e = Engine(0)
    try:
        e.set_gemm_mode("bf16")
        e.load_gpt2(sd, n_head=dims.n_head)
        ids, lens, tr = _np(e.decode_contrastive(prefix, 4, 0.6, stop, -1, T12, True))
        _check_structure(ids, lens, T12, [stop])
        assert np.isfinite(tr).all() and (tr[..., 0] >= 0).all() and (tr[..., 0] <= 1).all()
        assert (ids >= 0).all() and (ids < dims.vocab).all()
    finally:
        e.close()


class _Tok:
    """'.' -> 13, 'never' -> an id outside the vocabulary, any other text -> three tokens"""

    def encode(self, s):
        return {".": [13], "never": [DIMS["tiny"].vocab + 5]}.get(s, [5, 9, 11])

    def decode(self, toks):
        return " ".join(str(int(t)) for t in toks)


@pytest.mark.gpu
def test_generate_functions():
    """generate_contrastive_batch decodes what decode_contrastive_ids returns (764 is the second stop id, as in generate2);
    generate_contrastive takes one caption, keeps a prompt's tokens in front, and picks up model.logits_processors, which is
    cleared from the engine after the call; penalty_alpha = 0 is generate2's text"""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd._capi import CapdecError
    from capdec_amd.engine import LogitsProcessors
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    dims, sd, prefix, _ = _tiny_case()
    model = ClipCaptionModel(P, prefix_dim=512, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0").eval()
    model.load_state_dict(sd)
    tok = _Tok()
    text = lambda row, L: " ".join(str(int(t)) for t in row[:L])
    ids, lens = _np(E.decode_contrastive_ids(model, prefix[:4], 13, 4, 0.6, T12))
    _check_structure(ids, lens, T12, [13, 764])
    texts = E.generate_contrastive_batch(model, tok, prefix[:4], T12)
    assert texts == [text(ids[r], lens[r]) for r in range(4)]
    one = E.generate_contrastive(model, tok, embed=prefix[2:3].to("cuda:0"), entry_length=T12)
    assert one == texts[2]
    with pytest.raises(CapdecError):
        E.generate_contrastive(model, tok, embed=prefix[:2], entry_length=T12)
    g2 = E.generate2_batch(model, tok, prefix[:4], T12)
    assert E.generate_contrastive_batch(model, tok, prefix[:4], T12, penalty_alpha=0.0) == g2
    assert E.generate_contrastive_batch(model, tok, prefix[:4], T12, top_k=1) == g2
    # a prompt: its tokens stay in front
    pre = model.gpt.transformer.wte(torch.tensor([[5, 9, 11]], device="cuda:0"))
    pi, pl = _np(E.decode_contrastive_ids(model, pre, tok.encode("never")[0], 4, 0.6, T12))
    out = E.generate_contrastive(model, tok, prompt="a prompt", entry_length=T12, stop_token="never")
    assert out == text([5, 9, 11] + pi[0, :pl[0]].tolist(), 3 + int(pl[0]))
    # model.logits_processors
    model.logits_processors = LogitsProcessors(repetition_penalty=1.3, no_repeat_ngram_size=2)
    with_p = E.generate_contrastive(model, tok, embed=prefix[2:3], entry_length=T12)
    model.logits_processors = None
    wi, wl = _np(E.decode_contrastive_ids(model, prefix[2:3], 13, 4, 0.6, T12, repetition_penalty=1.3, no_repeat_ngram_size=2))
    assert with_p == text(wi[0], wl[0])
    assert E.generate_contrastive(model, tok, embed=prefix[2:3], entry_length=T12) == one      # cleared
