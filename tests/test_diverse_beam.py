"""Diverse (group) beam search (``capdec_decode_beam_groups``; ``Engine.decode_beam_groups``; ``generate_diverse_beam*``)
against the CPU definition of its contract in tests/diverse_def.py.

Bounds.  The comparison is the project's beam bar (tests/test_process.py, tests/test_hip_parity.py): a caption must match the
definition exactly -- tokens, lengths, order; scores within 1e-4 -- unless two adjacent candidate keys among the best
Bg + 1 of one of its groups came within KEY_GAP = 1e-4 at some live step (the margin diverse_def returns), in which case the
decision may fall either way and everything after it differs.  ``logp`` is a sum of ``lens`` log-probs, each under the same
1e-4 bar: within 1e-4 * lens.  At most 2 of a case's 16 captions may be below the margin -- asserted on the CPU for the
definition alone, so that the GPU comparison keeps something to assert.  One group must be the plain beam bit for bit.
"""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import diverse_def as DD
import process_def as PD
from capdec_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_GAP = 1e-4
UNCLEAR_CAP = 2               # captions of 16 whose margin may be below KEY_GAP
P, T12 = 10, 12
DIMS = {"tiny": synth.GPT2_TINY, "small": synth.GPT2_SMALL}
PROC = dict(theta=1.3, m=2, min_len=4)

#: name -> (beam, groups, lambda, processors); tiny geometry, seed 42 hot weights, P 10, T 12, 16 captions
CASES = {
    "b6g3": (6, 3, 0.5, None),
    "b4g2": (4, 2, 1.0, None),
    "b8g4": (8, 4, 0.5, None),
    "b8g2": (8, 2, 0.5, None),
    "b5g5": (5, 5, 0.5, None),
    "b6g3_proc": (6, 3, 0.5, PROC),
}
SMALL_CASES = {"b4g2": (4, 2, 0.5), "b8g4": (8, 4, 1.0)}


# ------------------------------------------------------------------------------------- cases (computed once, shared)
@functools.lru_cache(maxsize=None)
def _weights(geom, stop_bias=False):
    sd = synth.hot_state_dict(42, "mlp", 512, P, dims=DIMS[geom])
    return synth.with_stop_bias(sd, 13, 10.0) if stop_bias else sd


@functools.lru_cache(maxsize=None)
def _prefix(geom, n, stop_bias=False):
    from oracle import capdec_oracle as O
    x = synth.synthetic_clip_embeddings(n, 512, seed=0)
    return O.clip_project(x, _weights(geom, stop_bias), "mlp", P).reshape(n, P, -1)


@functools.lru_cache(maxsize=None)
def _stop(geom, n):
    """the token the unprocessed greedy run (definition, nothing stops) emits most often in its first three steps"""
    dims = DIMS[geom]
    ids = PD.greedy(_weights(geom), _prefix(geom, n), PD.Proc(), dims.vocab + 5, T12, -1, dims.n_head)[0]
    return int(np.bincount(ids[:, :3].reshape(-1)).argmax())


def _tiny_case():
    """-> dims, weights, 16 prefixes (the first 16 of test_process.py's 32), stop id"""
    return DIMS["tiny"], _weights("tiny"), _prefix("tiny", 32)[:16].contiguous(), _stop("tiny", 32)


@functools.lru_cache(maxsize=None)
def _tiny_def(B, G, lam, proc=False):
    dims, sd, prefix, stop = _tiny_case()
    p = PD.Proc(**PROC) if proc else PD.Proc()
    return DD.diverse_beam(sd, prefix, p, B, G, lam, stop, T12, n_head=dims.n_head)


@functools.lru_cache(maxsize=None)
def _small_def(B, G, lam):
    dims, sd = DIMS["small"], _weights("small")
    return DD.diverse_beam(sd, _prefix("small", 8)[:4].contiguous(), PD.Proc(), B, G, lam, _stop("small", 8), T12, n_head=dims.n_head)


# ===================================================================================== CPU: the definition
def test_one_group_is_the_plain_beam_definition():
    """G = 1 (lambda 0.7, beam 5): tokens, lengths and scores are process_def.beam's, exactly, with and without
    processors; the margin is process_def.beam's too"""
    dims, sd, prefix, stop = _tiny_case()
    for p in (PD.Proc(), PD.Proc(**PROC)):
        mg = []
        tok, seq, sc = PD.beam(sd, prefix, p, 5, stop, T12, n_head=dims.n_head, margins=mg)
        t1, s1, c1, lp, margin = DD.diverse_beam(sd, prefix, p, 5, 1, 0.7, stop, T12, n_head=dims.n_head)
        np.testing.assert_array_equal(t1.numpy(), tok.numpy())
        np.testing.assert_array_equal(s1.numpy(), seq.numpy())
        np.testing.assert_array_equal(c1.numpy(), sc.numpy())
        np.testing.assert_array_equal(margin.numpy(), mg[0].numpy())
        # nothing is penalised: the unpenalised sum is the score's sum
        np.testing.assert_allclose(lp.numpy(), (c1 * s1).numpy(), atol=1e-5 * T12)


def test_every_group_alone_is_the_greedy_beam():
    """G = B = 4 with lambda 0: every group is a beam of one that nothing penalises -- its tokens equal process_def.beam at
    beam 1, its score within 1e-6"""
    dims, sd, prefix, stop = _tiny_case()
    tok1, seq1, sc1 = PD.beam(sd, prefix, PD.Proc(), 1, stop, T12, n_head=dims.n_head)
    tok, seq, sc, lp, _ = DD.diverse_beam(sd, prefix, PD.Proc(), 4, 4, 0.0, stop, T12, n_head=dims.n_head)
    for g in range(4):
        np.testing.assert_array_equal(tok[:, g].numpy(), tok1[:, 0].numpy())
        np.testing.assert_array_equal(seq[:, g].numpy(), seq1[:, 0].numpy())
        np.testing.assert_allclose(sc[:, g].numpy(), sc1[:, 0].numpy(), atol=1e-6, rtol=0)


@pytest.mark.parametrize("name", list(CASES))
def test_margin_cap_definition_alone(name):
    """the GPU comparison keeps something to assert: at most 2 of a case's 16 captions have a margin below 1e-4.  Measured
    (definition alone; captions below 1e-4 / smallest margin / distinct sequences per caption): b6g3 2 / 6.2e-6 / 5.69 of 6;
    b4g2 0 / 1.2e-4 / 3.94 of 4; b8g4 2 / 6.2e-6 / 7.62 of 8; b8g2 2 / 1.5e-5 / 7.69 of 8; b5g5 0 / 2.7e-4 / 4.56 of 5;
    b6g3_proc 0 / 1.1e-4 / 6.00 of 6.  And the feature does something: (6, 3, 0.5) gives at least 5 distinct sequences per
    caption on average where lambda = 0 -- three identical groups of two -- gives at most 3 (measured 2.00)."""
    B, G, lam, proc = CASES[name]
    tok, seq, sc, lp, margin = _tiny_def(B, G, lam, proc is not None)
    unclear = int((margin < KEY_GAP).sum())
    distinct = DD.distinct_per_caption(tok.numpy(), seq.numpy())
    print(f"definition {name}: smallest margin {float(margin.min()):.2e}, captions below {KEY_GAP:g}: {unclear} of 16, "
          f"distinct sequences per caption {distinct:.2f} of {B}")
    assert torch.isfinite(sc).all() and torch.isfinite(lp).all()
    assert unclear <= UNCLEAR_CAP, unclear
    dims, sd, prefix, stop = _tiny_case()
    t, s = tok.numpy(), seq.numpy()
    for r in range(16):
        for b in range(B):
            L = int(s[r, b])
            assert 1 <= L <= T12 and (L == T12 or t[r, b, L - 1] == stop) and stop not in t[r, b, :L - 1], (r, b, t[r, b])
            if proc is not None:
                assert L == T12 or L > PROC["min_len"]
                grams = [tuple(t[r, b, k:k + 2]) for k in range(L - 1)]
                assert len(grams) == len(set(grams)), (r, b, t[r, b])
    if name == "b6g3":
        assert distinct >= 5.0, distinct
        t0, s0 = _tiny_def(6, 3, 0.0)[:2]
        same = DD.distinct_per_caption(t0.numpy(), s0.numpy())
        print(f"definition b6g3 with lambda 0: distinct sequences per caption {same:.2f}")
        assert same <= 3.0, same
        # the penalised scores are never above the unpenalised means
        assert (sc <= lp / seq + 1e-5).all()


# ===================================================================================== CPU: header, binding, arguments
def test_header_and_binding():
    from capdec_amd import _capi
    header = open(os.path.join(ROOT, "include", "capdec.h")).read()
    m = re.search(r"\bint\s+capdec_decode_beam_groups\s*\(([^;]*)\)\s*;", header)
    assert m, "prototype missing"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "d_prefix", "n", "P", "beam", "groups", "diversity_penalty", "stop_id",
                                                         "entry_length", "temperature", "d_ids", "d_lens", "d_scores", "d_order",
                                                         "d_logp"]
    assert re.search(r"#define\s+CAPDEC_ABI_VERSION\s+6\b", header) and _capi.ABI_VERSION == 6
    res, argtypes = _capi.SIGNATURES["capdec_decode_beam_groups"]
    want = []
    for a in args:                                              # the ctypes signature, argument by argument
        want.append(C.c_void_p if "*" in a else C.c_float if a.startswith("float") else C.c_int)
    assert res is C.c_int and argtypes == want
    lib = _capi.load_library()
    assert hasattr(lib, "capdec_decode_beam_groups") and lib.capdec_abi_version() == 6
    assert lib.capdec_decode_beam_groups(None, None, 1, 10, 6, 3, 0.5, 13, 12, 1.0, None, None, None, None, None) != 0
    assert b"decode_beam_groups" in lib.capdec_last_error()
    for word in ("groups < 1", "groups > beam", "beam % groups", "capdec_set_debug_diverge is not honoured"):
        assert word in header, word
    from capdec_amd import build
    assert "diverse.hip" in build.SOURCES


class _Untouchable:
    """a library / handle that fails the test when anything reaches it"""

    def __getattr__(self, name):
        raise AssertionError(f"the refused call reached the library: {name}")


def test_argument_checks():
    """the refusals come before anything touches the device or the context's processor state"""
    from capdec_amd._capi import CapdecError
    from capdec_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.lib, e._h = _Untouchable(), None
    pe = torch.zeros(2, P, 8)
    for kw in (dict(num_beam_groups=0), dict(num_beam_groups=7), dict(num_beam_groups=4), dict(num_beam_groups=-3),
               dict(diversity_penalty=-1.0), dict(diversity_penalty=float("nan")), dict(diversity_penalty=float("inf")),
               dict(diversity_penalty="0.5"), dict(num_beam_groups=2.0), dict(beam_size=9, num_beam_groups=3),
               dict(beam_size=0, num_beam_groups=1)):
        with pytest.raises(CapdecError):
            Engine.decode_beam_groups(e, pe, 13, **dict(dict(beam_size=6, num_beam_groups=3, diversity_penalty=0.5), **kw),
                                      repetition_penalty=1.3)
    seen = []
    e._decode_beam_groups = lambda *a: seen.append(a[1:]) or "D"
    assert Engine.decode_beam_groups(e, pe, 13, 6, 3, 0.5, 12) == "D" and seen == [(13, 6, 3, 0.5, 12, 1.0)]
    assert Engine.decode_beam_groups(e, pe, 13, 6, 6, 0, 12) == "D" and seen[-1] == (13, 6, 6, 0.0, 12, 1.0)


def test_python_surface():
    """the new functions and their defaults; generate_beam / generate_beam_batch keep their signatures"""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd.engine import Engine
    sig = inspect.signature(Engine.decode_beam_groups).parameters
    assert list(sig)[:8] == ["self", "prefix_embed", "stop_id", "beam_size", "num_beam_groups", "diversity_penalty",
                             "entry_length", "temperature"]
    assert (sig["beam_size"].default, sig["num_beam_groups"].default, sig["diversity_penalty"].default,
            sig["entry_length"].default, sig["temperature"].default) == (6, 3, 0.5, 67, 1.0)
    for fn in (Engine.decode_beam_groups, E.decode_diverse_beam_ids, E.generate_diverse_beam_batch):
        s = inspect.signature(fn).parameters
        for name in ("repetition_penalty", "no_repeat_ngram_size", "min_length", "logit_bias"):
            assert s[name].kind is inspect.Parameter.KEYWORD_ONLY and s[name].default is None, (fn.__name__, name)
    assert list(inspect.signature(E.generate_diverse_beam_batch).parameters)[:10] == [
        "model", "tokenizer", "embed", "beam_size", "num_beam_groups", "diversity_penalty", "entry_length", "temperature",
        "stop_token", "per_group"]
    assert list(inspect.signature(E.generate_diverse_beam).parameters)[:7] == [
        "model", "tokenizer", "beam_size", "num_beam_groups", "diversity_penalty", "prompt", "embed"]
    assert list(inspect.signature(E.generate_beam).parameters) == ["model", "tokenizer", "beam_size", "prompt", "embed",
                                                                   "entry_length", "temperature", "stop_token"]
    assert list(inspect.signature(E.generate_beam_batch).parameters)[:7] == ["model", "tokenizer", "embed", "beam_size",
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
    """captions `rows` of a HIP result (ids, lens, scores, order, logp) against the definition's (tokens, seq, scores,
    logp, margin) for those captions: every caption above the margin identical -> (identical, differ on a near-tie)"""
    i1, l1, s1, o1, p1 = got
    tok, seq, sc, lp, margin = want
    order = sc.argsort(dim=-1, descending=True, stable=True)
    clear = (margin > KEY_GAP).numpy()
    same = skipped = 0
    worst_s = worst_p = 0.0
    for j, r in enumerate(rows):
        oj = order[j]
        wl = seq[j][oj].numpy()
        eq = (np.array_equal(o1[r], oj.numpy()) and np.array_equal(i1[r], tok[j][oj].numpy()) and np.array_equal(l1[r], wl)
              and np.allclose(s1[r], sc[j][oj].numpy(), atol=1e-4, rtol=0)
              and (np.abs(p1[r] - lp[j][oj].numpy()) <= 1e-4 * wl).all())
        if eq:
            same += 1
            worst_s = max(worst_s, float(np.abs(s1[r] - sc[j][oj].numpy()).max()))
            worst_p = max(worst_p, float((np.abs(p1[r] - lp[j][oj].numpy()) / wl).max()))
        elif not clear[j]:
            assert np.isfinite(s1[r]).all() and (np.diff(s1[r]) <= 0).all() and np.isfinite(p1[r]).all()
            skipped += 1
        else:
            np.testing.assert_array_equal(o1[r], oj.numpy())
            np.testing.assert_array_equal(i1[r], tok[j][oj].numpy())
            np.testing.assert_array_equal(l1[r], wl)
            np.testing.assert_allclose(s1[r], sc[j][oj].numpy(), atol=1e-4, rtol=0)
            assert (np.abs(p1[r] - lp[j][oj].numpy()) <= 1e-4 * wl).all(), (r, p1[r], lp[j][oj].numpy())
    print(f"{what}: {len(rows)} captions, {same} identical ({int((~clear).sum())} had a margin < {KEY_GAP:g}), {skipped} differ "
          f"on such a tie; max |score - def| {worst_s:.2e}, max |logp - def| / len {worst_p:.2e}")
    return same, skipped


def _check_structure(got, B, G, T, stop):
    """every group contributes exactly Bg rows, scores descend, rows are zero after their length, lens include the stop"""
    ids, lens, scores, order, logp = got
    Bg = B // G
    assert ids.shape[1:] == (B, T) and lens.shape[1] == B and order.shape[1] == B
    assert np.isfinite(scores).all() and np.isfinite(logp).all() and (np.diff(scores, axis=1) <= 0).all()
    for r in range(ids.shape[0]):
        assert sorted(order[r].tolist()) == list(range(B)), order[r]
        assert np.bincount(order[r] // Bg, minlength=G).tolist() == [Bg] * G
        for b in range(B):
            L = int(lens[r, b])
            assert 1 <= L <= T and (ids[r, b, L:] == 0).all(), (r, b, ids[r, b])
            assert stop not in ids[r, b, :L - 1] and (L == T or ids[r, b, L - 1] == stop), (r, b, ids[r, b])


@pytest.mark.gpu
@pytest.mark.parametrize("n,B,T", [(16, 5, T12), (4, 8, 67)])
def test_one_group_is_the_plain_beam_bit_for_bit(eng, n, B, T):
    """G = 1: ids, lens, scores and order are Engine.decode_beam's, array_equal, for lambda 0 and 0.7 (beam 8 at T 67: the
    long history through the LDS staging), and so is the distinct-K/V-slot statistic (kv_slots_per_position, in [1, B]);
    logp is finite and, nothing being penalised, the score's sum; once more with processors set"""
    dims, sd, prefix, stop = _tiny_case()
    eng.load_gpt2(sd, n_head=dims.n_head)
    runs = [({}, 0.0), ({}, 0.7)]
    if T == T12:
        runs.append((PD.Proc(**PROC).kw(), 0.7))
    for kw, lam in runs:
        want = _np(eng.decode_beam(prefix[:n], stop, B, T, **kw))
        kv_want = eng.decode_counters()["kv_slots_per_position"]
        got = _np(eng.decode_beam_groups(prefix[:n], stop, B, 1, lam, T, **kw))
        kv = eng.decode_counters()["kv_slots_per_position"]
        for a, b in zip(got[:4], want):
            np.testing.assert_array_equal(a, b)
        assert kv == kv_want and 1.0 <= kv <= B, (kv, kv_want)
        assert np.isfinite(got[4]).all()
        np.testing.assert_allclose(got[4], got[2] * got[1], atol=1e-5 * T, rtol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_vs_definition(eng, name):
    """tiny geometry, T 12, 16 captions: for every caption with a margin above 1e-4 tokens, lengths and order are the
    definition's exactly, scores within 1e-4, logp within 1e-4 * lens; at least 14 of 16 identical"""
    B, G, lam, proc = CASES[name]
    dims, sd, prefix, stop = _tiny_case()
    eng.load_gpt2(sd, n_head=dims.n_head)
    kw = PD.Proc(**proc).kw() if proc else {}
    got = _np(eng.decode_beam_groups(prefix, stop, B, G, lam, T12, **kw))
    _check_structure(got, B, G, T12, stop)
    same, skipped = _vs_definition(got, _tiny_def(B, G, lam, proc is not None), list(range(16)), f"hip diverse beam {name}")
    assert same + skipped == 16 and same >= 14, (same, skipped)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SMALL_CASES))
def test_real_vocabulary(eng, name):
    """GPT-2 small's geometry (V = 50257: the fused lm_head's 393 tiles feed the candidate lists), 4 captions, T 12"""
    B, G, lam = SMALL_CASES[name]
    dims, sd = DIMS["small"], _weights("small")
    prefix, stop = _prefix("small", 8)[:4].contiguous(), _stop("small", 8)
    eng.load_gpt2(sd, n_head=dims.n_head)
    got = _np(eng.decode_beam_groups(prefix, stop, B, G, lam, T12))
    _check_structure(got, B, G, T12, stop)
    want = _small_def(B, G, lam)
    same, skipped = _vs_definition(got, want, list(range(4)), f"hip diverse beam, small geometry, {name}")
    assert same + skipped == 4


@pytest.mark.gpu
def test_stopping_compaction_chunks():
    """48 captions that stop (stop bias on token 13), T 16, (6, 3, 0.5), batch-invariant mode: the results do not depend on
    finished-caption compaction nor on a KV budget that forces 4 chunks (the per-chunk offsets include d_logp); 8 captions
    spread over the batch match the definition; every row is zero after its length, which includes the stop token"""
    from capdec_amd import _capi
    from capdec_amd.engine import Engine
    e = Engine(0)
    try:
        dims, sd, n, T, stop = DIMS["tiny"], _weights("tiny", True), 48, 16, 13
        B, G, lam = 6, 3, 0.5
        prefix = _prefix("tiny", n, True)
        e.load_gpt2(sd, n_head=dims.n_head)
        e.set_batch_invariant(True)
        run = lambda: _np(e.decode_beam_groups(prefix, stop, B, G, lam, T))
        res = run()
        _check_structure(res, B, G, T, stop)
        assert res[1].min() < T and len(set(res[1].reshape(-1).tolist())) > 3 and e.decode_chunks() == 1
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
        want = DD.diverse_beam(sd, prefix[pick], PD.Proc(), B, G, lam, stop, T, n_head=dims.n_head)
        same, skipped = _vs_definition(res, want, list(pick), "hip diverse beam, captions that stop")
        assert same + skipped == 8
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
    """generate_diverse_beam_batch returns the decoded rows best first, and with per_group the best row of each group in
    group order; generate_diverse_beam takes one caption, keeps a prompt's tokens in front, and picks up
    model.logits_processors, which is cleared from the engine after the call"""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd._capi import CapdecError
    from capdec_amd.engine import LogitsProcessors
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    dims, sd, prefix, stop = _tiny_case()
    B, G, lam, Bg = 6, 3, 0.5, 2
    model = ClipCaptionModel(P, prefix_dim=512, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0").eval()
    model.load_state_dict(sd)
    tok = _Tok()
    text = lambda row, L: " ".join(str(int(t)) for t in row[:L])
    ids, lens, scores, order, logp = _np(E.decode_diverse_beam_ids(model, prefix[:4], 13, B, G, lam, T12))
    _check_structure((ids, lens, scores, order, logp), B, G, T12, 13)
    texts = E.generate_diverse_beam_batch(model, tok, prefix[:4], B, G, lam, T12)
    assert texts == [[text(ids[r, b], lens[r, b]) for b in range(B)] for r in range(4)]
    best = E.generate_diverse_beam_batch(model, tok, prefix[:4], B, G, lam, T12, per_group=True)
    for r in range(4):
        assert len(best[r]) == G
        for g in range(G):
            first = int(np.nonzero(order[r] // Bg == g)[0][0])
            assert best[r][g] == texts[r][first]
    one = E.generate_diverse_beam(model, tok, B, G, lam, embed=prefix[2:3].to("cuda:0"), entry_length=T12)
    assert one == texts[2]
    assert E.generate_diverse_beam(model, tok, B, G, lam, embed=prefix[2:3], entry_length=T12, per_group=True) == best[2]
    with pytest.raises(CapdecError):
        E.generate_diverse_beam(model, tok, B, G, lam, embed=prefix[:2], entry_length=T12)
    # a prompt: its tokens stay in front, the row is cut at seq_lengths as generate_beam cuts it
    pre = model.gpt.transformer.wte(torch.tensor([[5, 9, 11]], device="cuda:0"))
    pi, pl = _np(E.decode_diverse_beam_ids(model, pre, tok.encode("never")[0], B, G, lam, T12))[:2]
    out = E.generate_diverse_beam(model, tok, B, G, lam, prompt="a prompt", entry_length=T12, stop_token="never")
    assert (pl == T12).all() and len(out) == B
    for b in range(B):
        assert out[b] == text([5, 9, 11] + pi[0, b].tolist(), T12)
    # model.logits_processors
    model.logits_processors = LogitsProcessors(repetition_penalty=1.3, no_repeat_ngram_size=2)
    with_p = E.generate_diverse_beam(model, tok, B, G, lam, embed=prefix[2:3], entry_length=T12)
    model.logits_processors = None
    wi, wl = _np(E.decode_diverse_beam_ids(model, prefix[2:3], 13, B, G, lam, T12, repetition_penalty=1.3, no_repeat_ngram_size=2))[:2]
    assert with_p == [text(wi[0, b], wl[0, b]) for b in range(B)] and with_p != one
    assert E.generate_diverse_beam(model, tok, B, G, lam, embed=prefix[2:3], entry_length=T12) == one      # cleared
