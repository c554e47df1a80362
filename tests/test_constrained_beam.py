"""Lexically constrained beam search (``capdec_decode_beam_constrained``; ``Engine.decode_beam_constrained``;
``generate_constrained_beam*``) against the CPU definition of its contract in tests/constrained_def.py, which selects over
the full vocabulary of every row and so also checks that the HIP path's short lists are enough.

Bounds.  The comparison is the project's beam bar (tests/test_diverse_beam.py): a caption must match the definition exactly
-- tokens, lengths, order, met; scores within 1e-4 -- unless two adjacent keys among the first (taken + 1) ranked
candidates of one of its banks came within KEY_GAP = 1e-4 at some live step (the margin constrained_def returns), in which
case the decision may fall either way and everything after it differs.  At most 2 of a case's 16 captions may be below the
margin -- asserted on the CPU for the definition alone, so that the GPU comparison keeps something to assert.  No phrases
must be the plain beam on the same logits route bit for bit.
"""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import constrained_def as CD
import process_def as PD
import test_diverse_beam as TD
from capdec_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_GAP = TD.KEY_GAP
UNCLEAR_CAP = TD.UNCLEAR_CAP
P, T12 = TD.P, TD.T12
PROC = TD.PROC
DIMS = TD.DIMS

#: name -> (beam, processors); tiny geometry, seed 42 hot weights, P 10, T 12, 16 captions, phrases from default_rng(7)
CASES = {"b5": (5, None), "b3": (3, None), "b8": (8, None), "b5_proc": (5, PROC)}


# ------------------------------------------------------------------------------------- cases (computed once, shared)
def _phrases(n, vocab, stop, seed=7):
    """caption r gets [0, 1, 2, 4][r % 4] phrases of rng.integers(1, 5) tokens each, drawn from the ids without the stop id"""
    rng = np.random.default_rng(seed)
    ids = np.array([t for t in range(vocab) if t != stop])
    out = []
    for r in range(n):
        out.append([[int(t) for t in rng.choice(ids, size=int(rng.integers(1, 5)))] for _ in range([0, 1, 2, 4][r % 4])])
    return out


@functools.lru_cache(maxsize=None)
def _tiny_phrases():
    dims, sd, prefix, stop = TD._tiny_case()
    return CD.pack(_phrases(16, dims.vocab, stop))


@functools.lru_cache(maxsize=None)
def _tiny_def(B, proc=False):
    dims, sd, prefix, stop = TD._tiny_case()
    p = PD.Proc(**PROC) if proc else PD.Proc()
    return CD.constrained_beam(sd, prefix, p, _tiny_phrases(), B, stop, T12, n_head=dims.n_head)


@functools.lru_cache(maxsize=None)
def _small_case():
    dims, sd = DIMS["small"], TD._weights("small")
    prefix, stop = TD._prefix("small", 8)[:4].contiguous(), TD._stop("small", 8)
    rng = np.random.default_rng(7)
    ids = np.array([t for t in range(dims.vocab) if t != stop])
    phrases = CD.pack([[[int(t) for t in rng.choice(ids, size=int(rng.integers(1, 5)))] for _ in range([1, 2, 4, 0][r])]
                       for r in range(4)])
    return dims, sd, prefix, stop, phrases


@functools.lru_cache(maxsize=None)
def _small_def():
    dims, sd, prefix, stop, phrases = _small_case()
    return CD.constrained_beam(sd, prefix, PD.Proc(), phrases, 5, stop, T12, n_head=dims.n_head)


# ===================================================================================== CPU: the definition
def test_no_phrases_is_the_plain_beam_definition():
    """no phrases (beam 5): tokens, lengths and scores are process_def.beam's, exactly, with and without processors; met
    is zero"""
    dims, sd, prefix, stop = TD._tiny_case()
    none = CD.pack([[] for _ in range(16)])
    for p in (PD.Proc(), PD.Proc(**PROC)):
        tok, seq, sc = PD.beam(sd, prefix, p, 5, stop, T12, n_head=dims.n_head)
        t1, s1, c1, met, _ = CD.constrained_beam(sd, prefix, p, none, 5, stop, T12, n_head=dims.n_head)
        np.testing.assert_array_equal(t1.numpy(), tok.numpy())
        np.testing.assert_array_equal(s1.numpy(), seq.numpy())
        np.testing.assert_array_equal(c1.numpy(), sc.numpy())
        assert not met.any()


def test_adv_and_bank():
    E = CD.EMPTY
    # a shared first token between two phrases: the lowest-index unmet phrase starts; once it is met the other one does
    ph = CD.pack([[[7, 8], [7, 9]]])[0]
    assert CD.adv(ph, E, 7) == (0, 0, 1) and CD.bank(ph, (0, 0, 1)) == 1
    assert CD.adv(ph, (0, 0, 1), 8) == (1, -1, 0) and CD.bank(ph, (1, -1, 0)) == 2
    assert CD.adv(ph, (0, 0, 1), 9) == (0, -1, 0)                  # no back-tracking: [7, 9] is not matched through phrase 0
    assert CD.adv(ph, (1, -1, 0), 7) == (1, 1, 1) and CD.adv(ph, (1, 1, 1), 9) == (3, -1, 0)
    assert CD.bank(ph, (3, -1, 0)) == 4 and CD.fold(ph, [7, 8, 3, 7, 9]) == (3, -1, 0) and CD.full(ph) == 3
    assert CD.special(ph, E) == {7} and CD.special(ph, (0, 0, 1)) == {7, 8} and CD.special(ph, (3, -1, 0)) == set()
    # the same phrase twice: it has to occur twice
    ph = CD.pack([[[4, 5], [4, 5]]])[0]
    assert CD.fold(ph, [4, 5]) == (1, -1, 0) and CD.fold(ph, [4, 5, 4, 5]) == (3, -1, 0) and CD.bank(ph, (1, 1, 1)) == 3
    # a mismatch that restarts a phrase: [4, 4, 5] -- the second 4 breaks the run and starts it again
    assert CD.adv(ph, (0, 0, 1), 4) == (0, 0, 1) and CD.fold(ph, [4, 4, 5]) == (1, -1, 0)
    ph = CD.pack([[[1, 2, 3]]])[0]
    assert CD.fold(ph, [1, 2, 1, 2, 3]) == (1, -1, 0) and CD.fold(ph, [1, 2, 9, 3]) == (0, -1, 0)
    assert [CD.bank(ph, CD.fold(ph, [1, 2, 3][:k])) for k in range(4)] == [0, 1, 2, 3]
    # a token that continues the phrase in progress does nothing else: it does not start another phrase
    ph = CD.pack([[[1, 2, 3], [2, 6]]])[0]
    assert CD.fold(ph, [1, 2]) == (0, 0, 2) and CD.fold(ph, [1, 2, 6]) == (0, -1, 0) and CD.fold(ph, [2, 6]) == (2, -1, 0)
    # a single-token phrase is met at once, also while another phrase is lost
    ph = CD.pack([[[1, 2], [6]]])[0]
    assert CD.adv(ph, E, 6) == (2, -1, 0) and CD.adv(ph, (0, 0, 1), 6) == (2, -1, 0) and CD.bank(ph, (2, 0, 1)) == 2
    assert CD.count(ph) == 2 and CD.plen(ph, 0) == 2 and CD.plen(ph, 1) == 1 and CD.plen(ph, 2) == 0
    assert CD.occurs([1, 2], [5, 1, 2]) and not CD.occurs([1, 2], [1, 5, 2])
    assert CD.final_order([1, 3, 0, 3], [-1.0, -3.0, -0.5, -2.0]) == [3, 1, 0, 2]


def test_select_round_robin():
    """banks descending, one candidate per visit, until B are taken; ties to the smaller flat index; the margin looks at
    the first taken + 1 of every bank"""
    keys = torch.tensor([-1.0, -2.0, -3.0, -0.5, -9.0, -9.0, -float("inf")])
    banks = np.array([0, 0, 0, 2, 1, 1, 3])
    taken, gap = CD.select(keys, banks, 5)
    assert taken == [3, 4, 0, 5, 1]                     # bank 2, 1, 0, then (bank 2 used up) 1, 0
    assert gap == 0.0                                   # bank 1: both taken at the same key
    taken, gap = CD.select(keys, banks, 2)
    assert taken == [3, 4] and gap == 0.0               # bank 1: the one taken against the next
    taken, gap = CD.select(keys[:4], banks[:4], 3)
    assert taken == [3, 0, 1] and gap == 1.0


@pytest.mark.parametrize("name", list(CASES))
def test_margin_cap_definition_alone(name):
    """the GPU comparison keeps something to assert: at most 2 of a case's 16 captions have a margin below 1e-4, and the
    constraints do something: every caption has a hypothesis with all its phrases met, contiguously, and no hypothesis
    stops before that.  Measured (definition alone; captions below 1e-4 / smallest margin): b5 0 / 4.0e-4; b3 0 / 6.6e-4;
    b8 2 / 1.2e-5; b5_proc 0 / 4.3e-4."""
    B, proc = CASES[name]
    tok, seq, sc, met, margin = _tiny_def(B, proc is not None)
    unclear = int((margin < KEY_GAP).sum())
    print(f"definition {name}: smallest margin {float(margin.min()):.2e}, captions below {KEY_GAP:g}: {unclear} of 16")
    assert unclear <= UNCLEAR_CAP, unclear
    dims, sd, prefix, stop = TD._tiny_case()
    phrases = _tiny_phrases()
    t, s, m = tok.numpy(), seq.numpy(), met.numpy()
    for r in range(16):
        full = CD.full(phrases[r])
        assert (m[r] == full).any(), (r, m[r], full)
        for b in range(B):
            L = int(s[r, b])
            row = t[r, b, :L]
            assert CD.fold(phrases[r], row)[0] == m[r, b]
            assert all(CD.occurs(phrases[r][c][:CD.plen(phrases[r], c)], row) for c in range(4) if (m[r, b] >> c) & 1)
            assert 1 <= L <= T12 and stop not in row[:-1] and (L == T12 or row[-1] == stop), (r, b, row)
            if stop in row:
                assert m[r, b] == full, (r, b, row, m[r, b])


# ===================================================================================== CPU: header, binding, surface
def test_header_and_binding():
    import ctypes as C
    from capdec_amd import _capi, build
    header = open(os.path.join(ROOT, "include", "capdec.h")).read()
    m = re.search(r"\bint\s+capdec_decode_beam_constrained\s*\(([^;]*)\)\s*;", header)
    assert m, "prototype missing"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "d_prefix", "d_phrases", "n", "P", "beam", "stop_id", "entry_length",
                                                         "temperature", "d_ids", "d_lens", "d_scores", "d_order", "d_met"]
    res, argtypes = _capi.SIGNATURES["capdec_decode_beam_constrained"]
    want = [C.c_void_p if "*" in a else C.c_float if a.startswith("float") else C.c_int for a in args]
    assert res is C.c_int and argtypes == want
    assert re.search(r"#define\s+CAPDEC_ABI_VERSION\s+6\b", header) and _capi.ABI_VERSION == 6      # no new ABI number
    lib = _capi.load_library()
    assert lib.capdec_decode_beam_constrained(None, None, None, 1, 10, 5, 13, 12, 1.0, None, None, None, None, None) != 0
    assert b"decode_beam_constrained" in lib.capdec_last_error()
    header = re.sub(r"\s*\n \* ?", " ", header)
    for word in ("a token id outside the vocabulary", "a phrase that holds stop_id", "a hole in front of a used place",
                 "beam outside 1..8", "bank(state)"):
        assert word in header, word
    assert "constrained.hip" in build.SOURCES


def test_python_surface_and_word_encoding():
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd import predictions_runner as R
    from capdec_amd._capi import CapdecError
    from capdec_amd.engine import Engine, pack_phrases
    sig = inspect.signature(Engine.decode_beam_constrained).parameters
    assert list(sig)[:7] == ["self", "prefix_embed", "phrases", "stop_id", "beam_size", "entry_length", "temperature"]
    assert (sig["beam_size"].default, sig["entry_length"].default, sig["temperature"].default) == (5, 67, 1.0)
    for fn in (Engine.decode_beam_constrained, E.decode_constrained_beam_ids, E.generate_constrained_beam_batch):
        s = inspect.signature(fn).parameters
        for name in ("repetition_penalty", "no_repeat_ngram_size", "min_length", "logit_bias"):
            assert s[name].kind is inspect.Parameter.KEYWORD_ONLY and s[name].default is None, (fn.__name__, name)
    s = inspect.signature(E.generate_constrained_beam).parameters
    assert list(s) == ["model", "tokenizer", "beam_size", "prompt", "embed", "force_words", "force_words_ids", "entry_length",
                       "temperature", "stop_token"]
    assert (s["beam_size"].default, s["entry_length"].default, s["temperature"].default, s["stop_token"].default) == (5, 67, 1., '.')
    s = inspect.signature(E.generate_constrained_beam_batch).parameters
    assert s["return_met"].default is False and s["force_words"].default is None
    s = inspect.signature(R.make_preds).parameters
    assert s["force_words"].kind is inspect.Parameter.KEYWORD_ONLY and s["force_words"].default is None
    assert list(inspect.signature(E.generate_beam).parameters) == ["model", "tokenizer", "beam_size", "prompt", "embed",
                                                                   "entry_length", "temperature", "stop_token"]

    class Tok:
        def encode(self, s):
            assert s.startswith(" ")                               # the word as it stands inside a sentence
            return list(range(100, 100 + len(s) - 1))

    assert E.encode_force_words(Tok(), ["ab", "c"]) == [[100, 101], [100]]
    with pytest.raises(CapdecError, match="'abcde'"):              # five tokens
        E.encode_force_words(Tok(), ["ab", "abcde"])
    with pytest.raises(CapdecError, match="'five'"):               # five words
        E.encode_force_words(Tok(), ["a", "b", "c", "d", "five"])
    ph = E._phrases_of(Tok(), 2, [["ab"], []], None)
    assert ph.shape == (2, 4, 4) and ph.dtype == np.int32 and ph[0, 0].tolist() == [100, 101, -1, -1] and (ph[1] == -1).all()
    assert (E._phrases_of(Tok(), 3, None, None) == -1).all()
    np.testing.assert_array_equal(E._phrases_of(Tok(), 1, None, [[[5, 6], [7]]]), pack_phrases([[[5, 6], [7]]]))
    for bad in (dict(force_words=[["a"]], force_words_ids=[[[1]]]), dict(force_words=[["a"], ["b"]], force_words_ids=None),
                dict(force_words=None, force_words_ids=[[[1, 2, 3, 4, 5]]]), dict(force_words=None, force_words_ids=[[[]]]),
                dict(force_words=None, force_words_ids=[[[1]] * 5])):
        with pytest.raises(CapdecError):
            E._phrases_of(Tok(), 1, **bad)


def test_engine_argument_checks():
    """the Python refusals come before anything touches the device or the context's processor state"""
    from capdec_amd._capi import CapdecError
    from capdec_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.lib, e._h = TD._Untouchable(), None
    pe = torch.zeros(2, P, 8)
    ok = [[[1, 2]], []]
    for phrases, kw in ((ok, dict(beam_size=0)), (ok, dict(beam_size=9)), (ok, dict(beam_size=2.0)), ([[[1]]], {}),
                        (np.zeros((2, 4, 3), np.int32), {}), ([[[1, 2, 3, 4, 5]], []], {}), ([[[1]] * 5, []], {})):
        with pytest.raises(CapdecError):
            Engine.decode_beam_constrained(e, pe, phrases, 13, **kw, repetition_penalty=1.3)
    seen = []
    e._decode_beam_constrained = lambda *a: seen.append(a) or "D"
    assert Engine.decode_beam_constrained(e, pe, ok, 13, 4, 12) == "D"
    assert seen[0][1].tolist() == CD.pack(ok).tolist() and seen[0][2:] == (13, 4, 12, 1.0)


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
    """captions `rows` of a HIP result (ids, lens, scores, order, met) against the definition's (tokens, seq, scores, met,
    margin) for those captions: every caption above the margin identical -> (identical, differ on a near-tie)"""
    i1, l1, s1, o1, m1 = got
    tok, seq, sc, met, margin = want
    clear = (margin > KEY_GAP).numpy()
    same = skipped = 0
    worst = 0.0
    for j, r in enumerate(rows):
        oj = np.array(CD.final_order(met[j].numpy(), sc[j].numpy()))
        wt, wl, ws, wm = tok[j].numpy()[oj], seq[j].numpy()[oj], sc[j].numpy()[oj], met[j].numpy()[oj]
        eq = (np.array_equal(o1[r], oj) and np.array_equal(i1[r], wt) and np.array_equal(l1[r], wl)
              and np.array_equal(m1[r], wm) and np.allclose(s1[r], ws, atol=1e-4, rtol=0))
        if eq:
            same += 1
            worst = max(worst, float(np.abs(s1[r] - ws).max()))
        elif not clear[j]:
            assert np.isfinite(s1[r]).all()
            skipped += 1
        else:
            np.testing.assert_array_equal(o1[r], oj)
            np.testing.assert_array_equal(i1[r], wt)
            np.testing.assert_array_equal(l1[r], wl)
            np.testing.assert_array_equal(m1[r], wm)
            np.testing.assert_allclose(s1[r], ws, atol=1e-4, rtol=0)
    print(f"{what}: {len(rows)} captions, {same} identical ({int((~clear).sum())} had a margin < {KEY_GAP:g}), {skipped} differ "
          f"on such a tie; max |score - def| {worst:.2e}")
    return same, skipped


def _check_properties(got, phrases, B, T, stop):
    """recomputed on the host from the returned ids: met is adv folded over the row; every met phrase occurs contiguously;
    no row holds the stop token before its met is complete; rows are ordered by (met count, score); the pad is zero"""
    ids, lens, scores, order, met = got
    assert ids.shape[1:] == (B, T) and lens.shape[1] == B and order.shape[1] == B and met.shape[1] == B
    assert np.isfinite(scores).all()
    for r in range(ids.shape[0]):
        ph = phrases[r]
        assert sorted(order[r].tolist()) == list(range(B)), order[r]
        keys = [(-bin(int(met[r, b])).count("1"), -float(scores[r, b])) for b in range(B)]
        assert keys == sorted(keys), (r, met[r], scores[r])
        for b in range(B):
            L = int(lens[r, b])
            row = ids[r, b, :L]
            assert 1 <= L <= T and (ids[r, b, L:] == 0).all(), (r, b, ids[r, b])
            assert CD.fold(ph, row)[0] == met[r, b], (r, b, row, met[r, b])
            for c in range(4):
                if (met[r, b] >> c) & 1:
                    assert CD.occurs(ph[c][:CD.plen(ph, c)], row), (r, b, c, row)
            assert stop not in row[:-1] and (L == T or row[-1] == stop), (r, b, row)
            if stop in row:
                assert met[r, b] == CD.full(ph), (r, b, row, met[r, b])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_vs_definition(eng, name):
    """tiny geometry, T 12, 16 captions with 0, 1, 2 or 4 phrases: for every caption with a margin above 1e-4 tokens,
    lengths, order and met are the definition's exactly, scores within 1e-4; at least 14 of 16 identical; the properties
    hold on every returned row"""
    B, proc = CASES[name]
    dims, sd, prefix, stop = TD._tiny_case()
    eng.load_gpt2(sd, n_head=dims.n_head)
    kw = PD.Proc(**proc).kw() if proc else {}
    got = _np(eng.decode_beam_constrained(prefix, _tiny_phrases(), stop, B, T12, **kw))
    _check_properties(got, _tiny_phrases(), B, T12, stop)
    same, skipped = _vs_definition(got, _tiny_def(B, proc is not None), list(range(16)), f"hip constrained beam {name}")
    assert same + skipped == 16 and same >= 14, (same, skipped)


@pytest.mark.gpu
@pytest.mark.parametrize("n,B,T", [(16, 5, T12), (4, 8, 67)])
def test_no_phrases_is_the_plain_beam_bit_for_bit(eng, n, B, T):
    """no phrases: ids, lens, scores and order are Engine.decode_beam's on the same route (an all-zero logit_bias sends it
    through the materialised logits), array_equal, and so is the distinct-K/V-slot statistic (kv_slots_per_position, in
    [1, B]); met is zero; once more with processors set (logits_select_kernel against logits_select_forced_kernel on the
    same processed logits)"""
    dims, sd, prefix, stop = TD._tiny_case()
    eng.load_gpt2(sd, n_head=dims.n_head)
    none = np.full((n, 4, 4), -1, dtype=np.int32)
    zero = np.zeros(dims.vocab, dtype=np.float32)
    kv_of = lambda: eng.decode_counters()["kv_slots_per_position"]
    want = _np(eng.decode_beam(prefix[:n], stop, B, T, logit_bias=zero))
    kv_want = kv_of()
    for kw in (dict(logit_bias=zero), {}):                     # (without any processor the call takes the same route)
        got = _np(eng.decode_beam_constrained(prefix[:n], none, stop, B, T, **kw))
        kv = kv_of()
        for a, b in zip(got[:4], want):
            np.testing.assert_array_equal(a, b)
        assert not got[4].any()
        assert kv == kv_want and 1.0 <= kv <= B, (kv, kv_want)
    if T == T12:
        kw = dict(PD.Proc(**PROC).kw(), logit_bias=zero)
        want = _np(eng.decode_beam(prefix[:n], stop, B, T, **kw))
        kv_want = kv_of()
        got = _np(eng.decode_beam_constrained(prefix[:n], none, stop, B, T, **kw))
        kv = kv_of()
        for a, b in zip(got[:4], want):
            np.testing.assert_array_equal(a, b)
        assert not got[4].any()
        assert kv == kv_want and 1.0 <= kv <= B, (kv, kv_want)


@pytest.mark.gpu
def test_stopping_compaction_chunks():
    """48 captions that stop (stop bias on token 13), T 16, beam 5, batch-invariant mode: the results do not depend on
    finished-caption compaction nor on a KV budget that forces 4 chunks (the phrase table, the states and d_met go through
    the compaction map and the chunk offset); the properties hold; 8 captions spread over the batch match the definition"""
    from capdec_amd import _capi
    from capdec_amd.engine import Engine
    e = Engine(0)
    try:
        dims, sd, n, T, stop, B = DIMS["tiny"], TD._weights("tiny", True), 48, 16, 13, 5
        prefix = TD._prefix("tiny", n, True)
        phrases = CD.pack(_phrases(n, dims.vocab, stop, seed=11))
        e.load_gpt2(sd, n_head=dims.n_head)
        e.set_batch_invariant(True)
        run = lambda: _np(e.decode_beam_constrained(prefix, phrases, stop, B, T))
        res = run()
        _check_properties(res, phrases, B, T, stop)
        assert res[1].min() < T and len(set(res[1].reshape(-1).tolist())) > 3 and e.decode_chunks() == 1
        assert e.decode_stats()["compactions"] >= 1
        e.set_compact(False)
        for a, b in zip(run(), res):
            np.testing.assert_array_equal(a, b)
        assert e.decode_stats()["compactions"] == 0
        e.set_compact(True)
        per_cap = (P + T - 1) * dims.n_embd * 2 * 4 * dims.n_layer
        _capi.check(e.lib.capdec_set_kv_budget(e._h, per_cap * B * 13), "budget")
        for a, b in zip(run(), res):
            np.testing.assert_array_equal(a, b)
        assert e.decode_chunks() == 4
        pick = np.linspace(0, n - 1, 8).astype(np.int64)
        want = CD.constrained_beam(sd, prefix[pick], PD.Proc(), phrases[pick], B, stop, T, n_head=dims.n_head)
        same, skipped = _vs_definition(res, want, list(pick), "hip constrained beam, captions that stop")
        assert same + skipped == 8
    finally:
        e.close()


@pytest.mark.gpu
def test_real_vocabulary(eng):
    """GPT-2 small's geometry (V = 50257: the one-pass selection over a long row, the beam * vocab flat index), 4 captions
    with 1, 2, 4 and 0 phrases, beam 5, T 12"""
    dims, sd, prefix, stop, phrases = _small_case()
    eng.load_gpt2(sd, n_head=dims.n_head)
    got = _np(eng.decode_beam_constrained(prefix, phrases, stop, 5, T12))
    _check_properties(got, phrases, 5, T12, stop)
    same, skipped = _vs_definition(got, _small_def(), list(range(4)), "hip constrained beam, small geometry")
    assert same + skipped == 4


@pytest.mark.gpu
def test_refusals(eng):
    """each bad input of the contract is an error reported through capdec_last_error, before any launch: the decode
    statistics are still those of the call before"""
    from capdec_amd._capi import CapdecError
    dims, sd, prefix, stop = TD._tiny_case()
    eng.load_gpt2(sd, n_head=dims.n_head)
    good = CD.pack([[[3, 4]], [[5]]])
    eng.decode_beam_constrained(prefix[:2], good, stop, 3, 6)
    before = eng.decode_stats()
    other = next(t for t in range(20) if t != stop)

    def table(edit):
        t = good.copy()
        edit(t)
        return t

    bad = {
        "outside the vocabulary": table(lambda t: t.__setitem__((0, 0, 1), dims.vocab)),
        "outside the vocabulary ": table(lambda t: t.__setitem__((1, 0, 0), -2)),
        "holds the stop token": table(lambda t: t.__setitem__((1, 0, 0), stop)),
        "a hole in front of a used place": table(lambda t: t.__setitem__((0, 0, 3), other)),
        "a hole in front of a used place ": table(lambda t: t.__setitem__((1, 2, 0), other)),
    }
    for words, t in bad.items():
        with pytest.raises(CapdecError, match=words.strip()):
            eng._decode_beam_constrained(prefix[:2], t, stop, 3, 6, 1.0)
        assert eng.decode_stats() == before, words
    for beam in (0, 9):
        with pytest.raises(CapdecError, match="beam size must be in 1..8"):
            eng._decode_beam_constrained(prefix[:2], good, stop, beam, 6, 1.0)
    # ... and the context goes on working
    got = _np(eng.decode_beam_constrained(prefix[:2], good, stop, 3, 6))
    _check_properties(got, good, 3, 6, stop)


class _Tok:
    """'.' -> 13, ' w<k>' -> the token k, ' pair' -> two tokens, any other text -> three tokens"""

    def encode(self, s):
        if s == ".":
            return [13]
        if s == " pair":
            return [21, 22]
        m = re.fullmatch(r" w(\d+)", s)
        return [int(m.group(1))] if m else [5, 9, 11]

    def decode(self, toks):
        return " ".join(str(int(t)) for t in toks)


@pytest.mark.gpu
def test_generate_functions():
    """generate_constrained_beam_batch returns the decoded rows in the returned order (and met with return_met);
    generate_constrained_beam takes one caption, words or ids; make_preds passes force_words through"""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd._capi import CapdecError
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    dims, sd, prefix, stop = TD._tiny_case()
    B = 5
    model = ClipCaptionModel(P, prefix_dim=512, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0").eval()
    model.load_state_dict(sd)
    tok = _Tok()
    text = lambda row, L: " ".join(str(int(t)) for t in row[:L])
    words = [["w30", "pair"], [], ["w7"], ["pair", "w40", "w41", "w42"]]
    phrases = CD.pack([[[30], [21, 22]], [], [[7]], [[21, 22], [40], [41], [42]]])
    np.testing.assert_array_equal(E._phrases_of(tok, 4, words, None), phrases)
    ids, lens, scores, order, met = _np(E.decode_constrained_beam_ids(model, prefix[:4], phrases, 13, B, T12))
    _check_properties((ids, lens, scores, order, met), phrases, B, T12, 13)
    texts, m2 = E.generate_constrained_beam_batch(model, tok, prefix[:4], B, force_words=words, entry_length=T12, return_met=True)
    assert texts == [[text(ids[r, b], lens[r, b]) for b in range(B)] for r in range(4)]
    np.testing.assert_array_equal(m2, met)
    assert met[0, 0] == 3 and "30" in texts[0][0].split() and "21 22" in texts[0][0]
    assert E.generate_constrained_beam_batch(model, tok, prefix[:4], B, force_words_ids=[[[30], [21, 22]], [], [[7]],
                                             [[21, 22], [40], [41], [42]]], entry_length=T12) == texts
    one = E.generate_constrained_beam(model, tok, B, embed=prefix[:1].to("cuda:0"), force_words=words[0], entry_length=T12)
    assert one == texts[0]
    assert E.generate_constrained_beam(model, tok, B, embed=prefix[2:3], force_words_ids=[[7]], entry_length=T12) == texts[2]
    # no words: generate_beam's texts
    assert E.generate_constrained_beam(model, tok, B, embed=prefix[1:2], entry_length=T12) == texts[1]
    with pytest.raises(CapdecError):
        E.generate_constrained_beam(model, tok, B, embed=prefix[:2], force_words=["w7"], entry_length=T12)
    # make_preds: the best caption of every image holds its words
    from capdec_amd import predictions_runner as R
    emb = synth.synthetic_clip_embeddings(4, 512, seed=0)
    preds = R.make_preds([{"image_id": r} for r in range(4)], emb, model, tok, beam=True, entry_length=T12, force_words=words)
    assert [d["image_id"] for d in preds] == list(range(4)) and "21 22" in preds[0]["caption"] and "7" in preds[2]["caption"].split()
    assert preds[1]["caption"] == R.make_preds([{"image_id": 1}], emb[1:2], model, tok, beam=True, entry_length=T12,
                                               logit_bias=np.zeros(dims.vocab, np.float32))[0]["caption"]
    with pytest.raises(CapdecError, match="'too long a word'"):
        tok5 = type("T5", (_Tok,), {"encode": lambda self, s: [1, 2, 3, 4, 5] if "too long" in s else _Tok.encode(self, s)})()
        E.generate_constrained_beam(model, tok5, B, embed=prefix[:1], force_words=["too long a word"], entry_length=T12)
