"""Classifier-free guidance on the greedy and the beam decode (``capdec_decode_guided``; ``Engine.decode_guided``;
``generate_guided*``) against the CPU definition of its contract in tests/guided_def.py.

Bounds (the project's own).  Tokens and lengths are identical, beam scores within 1e-4, beam order identical -- unless the
caption's margin in the definition is below GAP = 1e-4: the smallest, over its live steps, top-2 gap of the processed guided
logits (greedy) or gap between adjacent keys among the best B + 1 (beam).  Below it a decision may fall either way.  A greedy
caption may then differ from its first near-tie step on and must match before it.  A beam caption's returned rows are
re-ordered and re-parented at every step, so no prefix of them is pinned by the steps before the tie: such a caption must
still have valid lengths and finite, descending scores.  At most 2 of a case's 16 captions may be below the margin --
asserted on the CPU for the definition alone -- and at least 14 of 16 must be identical on the GPU.
"""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import guided_def as GD
import process_def as PD
from capdec_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 1e-4
UNCLEAR_CAP = 2               # captions of 16 whose margin may be below GAP
SCORE_TOL = 1e-4
P, T12 = 10, 12
DIMS = {"tiny": synth.GPT2_TINY, "small": synth.GPT2_SMALL}
PROC = dict(theta=1.3, m=2, min_len=4)

#: name -> (beam, guidance_scale, negative, processors); tiny geometry, seed 42 hot weights, P 10, T 12, 16 captions, stop 744
CASES = {
    "greedy_g15_mean": (1, 1.5, "mean", False),
    "greedy_g3_per": (1, 3.0, "per", False),
    "greedy_g15_per_proc": (1, 1.5, "per", True),
    "beam5_g15_per": (5, 1.5, "per", False),
    "beam5_g3_mean": (5, 3.0, "mean", False),
    "beam5_g15_per_proc": (5, 1.5, "per", True),
}
#: the cases in which captions stop early (greedy: definition lens 1, 3, 4, 5; beam 2: two captions done after 3 and 5 steps)
STOP_CASES = {"greedy": (1, 1.1, "mean", False), "beam2": (2, 1.1, "mean", False)}


# ------------------------------------------------------------------------------------- cases (computed once, shared)
@functools.lru_cache(maxsize=None)
def _weights(geom):
    return synth.hot_state_dict(42, "mlp", 512, P, dims=DIMS[geom])


@functools.lru_cache(maxsize=None)
def _prefix(geom, n, seed=0):
    from oracle import capdec_oracle as O
    x = synth.synthetic_clip_embeddings(n, 512, seed=seed)
    return O.clip_project(x, _weights(geom), "mlp", P).reshape(n, P, -1)


@functools.lru_cache(maxsize=None)
def _negative(kind):
    """mean: the mean of all 32 prefixes [1, P, d]; per: the mapper's output for 16 other CLIP embeddings [16, P, d]"""
    if kind == "mean":
        return _prefix("tiny", 32).mean(dim=0, keepdim=True).contiguous()
    return _prefix("tiny", 16, 3).contiguous()


@functools.lru_cache(maxsize=None)
def _stop():
    """the token the unprocessed greedy run of all 32 prefixes (definition, nothing stops) emits most often in its first
    three steps, as test_contrastive.py chooses it: 744"""
    dims = DIMS["tiny"]
    ids = PD.greedy(_weights("tiny"), _prefix("tiny", 32), PD.Proc(), dims.vocab + 5, T12, -1, dims.n_head)[0]
    return int(np.bincount(ids[:, :3].reshape(-1)).argmax())


def _tiny_case():
    """-> dims, weights, 16 prefixes (the first 16 of synthetic_clip_embeddings(32, 512, seed=0)), stop id"""
    return DIMS["tiny"], _weights("tiny"), _prefix("tiny", 32)[:16].contiguous(), _stop()


def _proc(on):
    return PD.Proc(**PROC) if on else PD.Proc()


@functools.lru_cache(maxsize=None)
def _tiny_def(beam, gamma, neg, proc=False, dtype=torch.float32):
    """the definition of a tiny case; neg: "mean", "per" or "self" (the captions' own prefixes)"""
    dims, sd, prefix, stop = _tiny_case()
    q = prefix if neg == "self" else _negative(neg)
    if beam == 1:
        return GD.guided_greedy(sd, prefix, q, gamma, _proc(proc), stop, T12, -1, dims.n_head, dtype)
    return GD.guided_beam(sd, prefix, q, gamma, _proc(proc), beam, stop, T12, 1.0, dims.n_head, dtype)


@functools.lru_cache(maxsize=None)
def _plain_def(beam, proc=False):
    """the unguided definition (process_def): greedy -> (ids, lens, gaps); beam -> (tokens, seq, scores, margin) as numpy"""
    dims, sd, prefix, stop = _tiny_case()
    if beam == 1:
        return PD.greedy(sd, prefix, _proc(proc), stop, T12, -1, dims.n_head)
    m = []
    tok, seq, sc = PD.beam(sd, prefix, _proc(proc), beam, stop, T12, 1.0, dims.n_head, margins=m)
    return tok.numpy(), seq.numpy(), sc.numpy(), m[0].numpy()


def _margin(r):
    return r.gaps.min(axis=1) if isinstance(r, GD.Greedy) else r.margin


def _sorted_beams(r):
    """a definition's beams in the returned order: by score descending, equal scores by slot -> (order, ids, lens, scores)"""
    order = np.argsort(-r.scores, axis=1, kind="stable")
    take = lambda a: np.take_along_axis(a, order.reshape(order.shape + (1,) * (a.ndim - 2)), axis=1)
    return order, take(r.tokens), take(r.seq), take(r.scores)


def _check_structure(ids, lens, T, stops):
    ids, lens = ids.reshape(-1, ids.shape[-1]), lens.reshape(-1)
    for r in range(ids.shape[0]):
        L = int(lens[r])
        assert 1 <= L <= T and (ids[r, L:] == 0).all(), (r, ids[r], L)
        assert not any(s in ids[r, :L - 1] for s in stops) and (L == T or ids[r, L - 1] in stops), (r, ids[r])


# ===================================================================================== CPU: the definition
def test_off_and_equal_prefixes_of_the_definition():
    """without processors the definition at gamma = 1 gives process_def.greedy / process_def.beam ids and lens exactly, for
    both negatives; with the captions' own prefixes as negatives and gamma = 2 it gives the same ids"""
    assert _stop() == 744
    gi, gl, _ = _plain_def(1)
    bt, bs, _, _ = _plain_def(5)
    for neg, gamma in (("mean", 1.0), ("per", 1.0), ("self", 2.0)):
        r = _tiny_def(1, gamma, neg)
        np.testing.assert_array_equal(r.ids, gi)
        np.testing.assert_array_equal(r.lens, gl)
        b = _tiny_def(5, gamma, neg)
        np.testing.assert_array_equal(b.tokens, bt)
        np.testing.assert_array_equal(b.seq, bs)


@pytest.mark.parametrize("name", list(CASES))
def test_margins_float64_and_effect(name):
    """the GPU comparison keeps something to assert: at most 2 of a case's 16 captions have a margin below 1e-4; the fp32
    and float64 runs of the definition agree on every caption at or above the margin, beam scores within 2.5e-5 (a quarter
    of the 1e-4 bound); at least 12 of 16 captions differ from the unguided definition under the same processors.  Measured
    (definition alone; captions below 1e-4 / smallest margin / captions that differ from the unguided ones / max |score
    fp32 - fp64|): greedy_g15_mean 0 / 7.2e-3 / 16; greedy_g3_per 0 / 2.0e-2 / 16; greedy_g15_per_proc 0 / 4.6e-3 / 16;
    beam5_g15_per 1 / 16 / 2.8e-6; beam5_g3_mean 0 / 16 / 6.3e-6; beam5_g15_per_proc 1 / 16 / 3.5e-6."""
    beam, gamma, neg, proc = CASES[name]
    r, r64 = _tiny_def(beam, gamma, neg, proc), _tiny_def(beam, gamma, neg, proc, torch.float64)
    margin = _margin(r)
    clear = margin >= GAP
    unclear = int((~clear).sum())
    stop = _stop()
    if beam == 1:
        base = _plain_def(1, proc)[0]
        differ = int((r.ids != base).any(axis=1).sum())
        print(f"definition {name}: smallest margin {margin.min():.2e}, captions below {GAP:g}: {unclear} of 16, {differ} differ "
              f"from the unguided ones, lens {sorted(r.lens.tolist())}")
        np.testing.assert_array_equal(r.ids[clear], r64.ids[clear])
        np.testing.assert_array_equal(r.lens[clear], r64.lens[clear])
        _check_structure(r.ids, r.lens, T12, [stop])
        ids = r.ids
    else:
        base = _plain_def(beam, proc)[0]
        differ = int((r.tokens != base).any(axis=(1, 2)).sum())
        err = float(np.abs(r.scores[clear] - r64.scores[clear]).max())
        print(f"definition {name}: smallest margin {margin.min():.2e}, captions below {GAP:g}: {unclear} of 16, {differ} differ "
              f"from the unguided ones, max |score fp32 - fp64| {err:.2e}")
        np.testing.assert_array_equal(r.tokens[clear], r64.tokens[clear])
        np.testing.assert_array_equal(r.seq[clear], r64.seq[clear])
        assert err < SCORE_TOL / 4, err
        assert np.isfinite(r.scores).all() and (r.scores <= 0).all()
        # a beam's length is seq (stopped beams no longer count); the stop token ends it, zeros follow
        for t, L in zip(r.tokens.reshape(-1, T12), r.seq.reshape(-1)):
            assert 1 <= L <= T12 and (t[L:] == 0).all() and stop not in t[:L - 1] and (L == T12 or t[L - 1] == stop), (t, L)
        ids = r.tokens.reshape(-1, T12)
    assert unclear <= UNCLEAR_CAP, unclear
    assert differ >= 12, differ
    if proc:
        lens = (r.lens if beam == 1 else r.seq).reshape(-1)
        for row, L in zip(ids, lens):
            assert L == T12 or L > PROC["min_len"]
            grams = [tuple(row[k:k + 2]) for k in range(L - 1)]
            assert len(grams) == len(set(grams)), row


# ===================================================================================== CPU: header, binding, arguments
def test_header_and_binding():
    from capdec_amd import _capi
    header = open(os.path.join(ROOT, "include", "capdec.h")).read()
    m = re.search(r"\bint\s+capdec_decode_guided\s*\(([^;]*)\)\s*;", header)
    assert m, "prototype missing"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "ctx", "d_prefix", "d_neg_prefix", "neg_n", "n", "P", "beam", "guidance_scale", "stop_id", "alt_stop_id", "entry_length",
        "temperature", "d_ids", "d_lens", "d_scores", "d_order"]
    assert re.search(r"#define\s+CAPDEC_ABI_VERSION\s+6\b", header) and _capi.ABI_VERSION == 6
    res, argtypes = _capi.SIGNATURES["capdec_decode_guided"]
    want = [C.c_void_p if "*" in a else C.c_float if a.startswith("float") else C.c_int for a in args]
    assert res is C.c_int and argtypes == want
    lib = _capi.load_library()
    assert hasattr(lib, "capdec_decode_guided") and lib.capdec_abi_version() == 6
    assert lib.capdec_decode_guided(None, None, None, 1, 1, 10, 1, 1.5, 13, -1, 12, 1.0, None, None, None, None) != 0
    assert b"decode_guided" in lib.capdec_last_error()
    for word in ("g_j = gamma * c_j + (1 - gamma) * u_j", "guidance_scale == 1 means off", "repetition_penalty always\n *      multiplies",
                 "renormalised", "neg_n other than 1 or n"):
        assert word in header, word
    from capdec_amd import build
    assert "guided.hip" in build.SOURCES


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
    pe, neg = torch.zeros(4, P, 8), torch.zeros(1, P, 8)
    ok = dict(negative_embed=neg, guidance_scale=1.5, stop_id=13)
    for kw in (dict(guidance_scale=0.5), dict(guidance_scale=0.999), dict(guidance_scale=0), dict(guidance_scale=-2.0),
               dict(guidance_scale=float("nan")), dict(guidance_scale=float("inf")), dict(guidance_scale=-float("inf")),
               dict(guidance_scale="1.5"), dict(guidance_scale=None), dict(guidance_scale=True),
               dict(negative_embed=torch.zeros(1, P + 1, 8)), dict(negative_embed=torch.zeros(1, P, 16)),
               dict(negative_embed=torch.zeros(P + 1, 8)), dict(negative_embed=torch.zeros(2, P, 8)),
               dict(negative_embed=torch.zeros(5, P, 8)), dict(negative_embed=torch.zeros(1, 1, P, 8)),
               dict(negative_embed=torch.zeros(1, P, 8, dtype=torch.int32)), dict(negative_embed=None),
               dict(beam_size=0), dict(beam_size=9), dict(beam_size=-1), dict(beam_size=5.0), dict(beam_size=True),
               dict(entry_length=0), dict(entry_length=12.0)):
        with pytest.raises(CapdecError):
            Engine.decode_guided(e, pe, **dict(ok, **kw), repetition_penalty=1.3)
    with pytest.raises(CapdecError):
        Engine.decode_guided(e, torch.zeros(P, 8), **ok, repetition_penalty=1.3)
    seen = []
    e._decode_guided = lambda *a: seen.append((tuple(a[1].shape),) + a[2:]) or ("I", "L", "S", "O")
    assert Engine.decode_guided(e, pe, neg, 1.5, 13) == ("I", "L", "S", "O") and seen == [((1, P, 8), 1.5, 13, 1, 67, 1.0, 764)]
    assert Engine.decode_guided(e, pe, neg[0], 1, 13, 5, 12, 0.7, -1) == ("I", "L", "S") and seen[-1] == ((1, P, 8), 1.0, 13, 5, 12, 0.7, -1)
    assert Engine.decode_guided(e, pe, torch.zeros(4, P, 8), np.float32(3), 13, np.int64(8), return_order=True) == ("I", "L", "S", "O")
    assert seen[-1] == ((4, P, 8), 3.0, 13, 8, 67, 1.0, 764)


def test_python_surface():
    """the new functions and their defaults; generate2 / generate2_batch / generate_beam / generate_beam_batch keep their
    signatures"""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd.engine import Engine
    sig = inspect.signature(Engine.decode_guided).parameters
    assert list(sig)[:9] == ["self", "prefix_embed", "negative_embed", "guidance_scale", "stop_id", "beam_size", "entry_length",
                             "temperature", "alt_stop_id"]
    assert (sig["beam_size"].default, sig["entry_length"].default, sig["temperature"].default, sig["alt_stop_id"].default) == \
        (1, 67, 1.0, 764)
    assert sig["guidance_scale"].default is inspect.Parameter.empty
    for fn in (Engine.decode_guided, E.decode_guided_ids, E.generate_guided_batch):
        s = inspect.signature(fn).parameters
        for name in ("repetition_penalty", "no_repeat_ngram_size", "min_length", "logit_bias"):
            assert s[name].kind is inspect.Parameter.KEYWORD_ONLY and s[name].default is None, (fn.__name__, name)
    b = inspect.signature(E.generate_guided_batch).parameters
    assert list(b)[:8] == ["model", "tokenizer", "embed", "negative_embed", "guidance_scale", "beam_size", "entry_length", "stop_token"]
    assert (b["guidance_scale"].default, b["beam_size"].default, b["entry_length"].default, b["stop_token"].default) == (1.5, 1, 67, ".")
    g = inspect.signature(E.generate_guided).parameters
    assert list(g)[:8] == ["model", "tokenizer", "tokens", "prompt", "embed", "negative_embed", "guidance_scale", "beam_size"]
    assert (g["negative_embed"].default, g["guidance_scale"].default, g["beam_size"].default, g["entry_length"].default) == (None, 1.5, 1, 67)
    assert inspect.signature(E.decode_guided_ids).parameters["guidance_scale"].default == 1.5
    kw = ["repetition_penalty", "no_repeat_ngram_size", "min_length", "logit_bias"]
    assert list(inspect.signature(E.generate2).parameters) == ["model", "tokenizer", "tokens", "prompt", "embed", "entry_count",
                                                               "entry_length", "top_p", "temperature", "stop_token"]
    assert list(inspect.signature(E.generate2_batch).parameters) == ["model", "tokenizer", "embed", "entry_length", "stop_token"] + kw
    assert list(inspect.signature(E.generate_beam).parameters) == ["model", "tokenizer", "beam_size", "prompt", "embed",
                                                                   "entry_length", "temperature", "stop_token"]
    assert list(inspect.signature(E.generate_beam_batch).parameters) == ["model", "tokenizer", "embed", "beam_size", "entry_length",
                                                                         "temperature", "stop_token"] + kw
    for fn, want in ((E.generate2, (1, 67, 0.8, 1., ".")), (E.generate_beam, (5, None, None, 67, 1., "."))):
        assert tuple(p.default for p in list(inspect.signature(fn).parameters.values())[-len(want):]) == want


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
    """captions `rows` of a HIP result -- (ids, lens) or (ids, lens, scores, order) -- against the definition's result for
    those captions, under the module's bounds -> (identical, differ on a near-tie)"""
    same = skipped = 0
    worst = 0.0
    margin = _margin(want)
    if isinstance(want, GD.Greedy):
        ids, lens = got
        for j, r in enumerate(rows):
            if np.array_equal(ids[r], want.ids[j]) and lens[r] == want.lens[j]:
                same += 1
                continue
            assert margin[j] < GAP, (what, r, ids[r], want.ids[j], lens[r], want.lens[j], margin[j])
            t0 = int(np.nonzero(want.gaps[j] < GAP)[0][0])             # everything before the first near tie still matches
            np.testing.assert_array_equal(ids[r, :t0], want.ids[j, :t0])
            assert lens[r] > t0
            skipped += 1
    else:
        ids, lens, scores, order = got
        o, wi, wl, ws = _sorted_beams(want)
        for j, r in enumerate(rows):
            err = float(np.abs(scores[r] - ws[j]).max())
            if np.array_equal(ids[r], wi[j]) and np.array_equal(lens[r], wl[j]) and np.array_equal(order[r], o[j]) and err <= SCORE_TOL:
                worst = max(worst, err)
                same += 1
                continue
            assert margin[j] < GAP, (what, r, ids[r], wi[j], lens[r], wl[j], order[r], o[j], err, margin[j])
            assert np.isfinite(scores[r]).all() and (np.diff(scores[r]) <= 0).all() and (lens[r] >= 1).all()
            skipped += 1
    print(f"{what}: {len(rows)} captions, {same} identical ({int((margin < GAP).sum())} had a margin < {GAP:g}), {skipped} differ "
          f"from such a tie on; max |score - def| {worst:.2e}")
    return same, skipped


def _run(e, case, prefix=None, neg=None, rows=None, stop=None, T=T12):
    """one guided decode of a tiny case on engine e (captions `rows` of it) -> numpy (ids, lens[, scores, order])"""
    beam, gamma, negname, proc = case
    prefix = _tiny_case()[2] if prefix is None else prefix
    neg = _negative(negname) if neg is None else neg
    if rows is not None:
        prefix = prefix[rows].contiguous()
        neg = neg if neg.shape[0] == 1 else neg[rows].contiguous()
    kw = _proc(proc).kw() if proc else {}
    return _np(e.decode_guided(prefix, neg, gamma, _stop() if stop is None else stop, beam, T, 1.0, -1, return_order=True, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_vs_definition(eng, name):
    """tiny geometry, T 12, 16 captions, stop id 744, the six cases: tokens, lengths, beam order identical and beam scores
    within 1e-4 for every caption with a margin of at least 1e-4; at least 14 of 16 identical.  Measured on an MI355X: 16 of
    16 identical in every case; max |score - def| beam5_g15_per 3.3e-6, beam5_g3_mean 4.7e-6, beam5_g15_per_proc 2.9e-6"""
    dims, sd, prefix, stop = _tiny_case()
    eng.load_gpt2(sd, n_head=dims.n_head)
    got = _run(eng, CASES[name])
    _check_structure(got[0], got[1], T12, [stop])
    same, skipped = _vs_definition(got, _tiny_def(*CASES[name]), list(range(16)), f"hip guided {name}")
    assert same + skipped == 16 and same >= 14, (same, skipped)


@pytest.mark.gpu
@pytest.mark.parametrize("proc", [False, True])
def test_scale_one_is_the_plain_call(eng, proc):
    """guidance_scale = 1 gives decode_greedy / decode_beam results of the same engine bit for bit (ids, lens, scores, order),
    with and without processors, whatever the negative prefix"""
    dims, sd, prefix, stop = _tiny_case()
    eng.load_gpt2(sd, n_head=dims.n_head)
    kw = _proc(proc).kw() if proc else {}
    for neg in (_negative("mean"), _negative("per")):
        plain = eng.decode_greedy(prefix, stop, T12, 764, **kw)
        got = eng.decode_guided(prefix, neg, 1.0, stop, 1, T12, 1.0, 764, **kw)
        assert len(got) == 2 and all(torch.equal(a, b) for a, b in zip(got, plain))
        plain = eng.decode_beam(prefix, stop, 5, T12, 0.9, **kw)
        got = eng.decode_guided(prefix, neg, 1, stop, 5, T12, 0.9, return_order=True, **kw)
        assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, plain))
        assert len(eng.decode_guided(prefix, neg, 1.0, stop, 5, T12, 0.9, **kw)) == 3
    assert eng.decode_step_rows()[0] == 80                      # no negative rows: 16 captions x 5 beams


@pytest.mark.gpu
def test_equal_prefixes(eng):
    """negative_embed = prefix_embed and gamma = 2: u = c, so g = c up to rounding and the tokens are the plain decode's for
    every caption whose plain margin (unguided definition) is at least 1e-4, beam scores within 1e-4 -- the test of the
    pairing: a partner row that is fed the wrong token, the wrong parent or the wrong cache slot makes u != c.  Captions
    stop (id 744), so compacted steps are part of it."""
    dims, sd, prefix, stop = _tiny_case()
    eng.load_gpt2(sd, n_head=dims.n_head)
    gi, gl = _np(eng.decode_greedy(prefix, stop, T12, -1))
    ids, lens = _np(eng.decode_guided(prefix, prefix, 2.0, stop, 1, T12, 1.0, -1))
    clear = _plain_def(1)[2].min(axis=1) >= GAP
    assert clear.sum() >= 14 and (gl < T12).sum() >= 4
    np.testing.assert_array_equal(ids[clear], gi[clear])
    np.testing.assert_array_equal(lens[clear], gl[clear])
    bi, bl, bs, bo = _np(eng.decode_beam(prefix, stop, 5, T12))
    ids, lens, scores, order = _np(eng.decode_guided(prefix, prefix, 2.0, stop, 5, T12, return_order=True))
    clear = _plain_def(5)[3] >= GAP
    assert clear.sum() >= 14
    np.testing.assert_array_equal(ids[clear], bi[clear])
    np.testing.assert_array_equal(lens[clear], bl[clear])
    np.testing.assert_array_equal(order[clear], bo[clear])
    err = np.abs(scores[clear] - bs[clear]).max()
    print(f"equal prefixes, gamma 2: {int(clear.sum())} clear captions identical to the plain beam decode, max |score - plain| {err:.2e}")
    assert err <= SCORE_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STOP_CASES))
def test_captions_that_stop_and_compaction(eng, name):
    """(gamma 1.1, mean): the greedy definition's lengths start 1, 3, 4, 5 (four captions stop early; the issue's (1.5, mean) has
    three), beam 2 has two captions whose beams all stop.  Compaction on and off give identical ids / lens / scores;
    with it on the launches shrink (both halves are counted), with it off every step carries all rows; both equal the
    definition under the margin rule"""
    case = STOP_CASES[name]
    beam = case[0]
    dims, sd, prefix, stop = _tiny_case()
    eng.load_gpt2(sd, n_head=dims.n_head)
    want = _tiny_def(*case)
    full = 2 * 16 * beam
    if beam == 1:
        assert sorted(want.lens.tolist())[:5] == [1, 3, 4, 5, 12] and int((want.lens < T12).sum()) == 4
    else:
        assert sorted(np.isfinite(want.step_margin).sum(axis=1).tolist())[:3] == [3, 5, 12]
    try:
        eng.set_compact(True)
        on = _run(eng, case)
        st, rows = eng.decode_stats(), eng.decode_step_rows()
        assert st["steps"] == T12 and st["compactions"] >= 1 and len(rows) == T12 - 1, (st, rows)
        # (greedy: the caption of length 1 is gone before step 1 already)
        assert rows[0] == (full - 2 if beam == 1 else full) and rows[-1] < rows[0] and all(a >= b for a, b in zip(rows, rows[1:])), rows
        assert all(r % (2 * beam) == 0 for r in rows) and st["row_steps"] == sum(rows) < full * (T12 - 1)
        eng.set_compact(False)
        off = _run(eng, case)
        st, rows = eng.decode_stats(), eng.decode_step_rows()
        assert st["compactions"] == 0 and rows == [full] * (T12 - 1) and st["row_steps"] == full * (T12 - 1), (st, rows)
    finally:
        eng.set_compact(True)
    for a, b in zip(on, off):
        np.testing.assert_array_equal(a, b)
    _check_structure(on[0], on[1], T12, [stop])
    same, skipped = _vs_definition(on, want, list(range(16)), f"hip guided {name}, captions that stop")
    assert same + skipped == 16 and same >= 14


@pytest.mark.gpu
@pytest.mark.parametrize("sample_rows", [None, 7])
def test_chunking_row_blocks_and_single_captions(sample_rows):
    """batch-invariant mode and a KV budget that holds 6 caption pairs: the 16 captions run as 3 chunks, and their results are
    bit for bit those of the one-chunk run and of every caption decoded alone (with its own negative), for greedy and beam 5
    with per-caption negatives; all equal the definition under the margin rule.  Once with the default logits blocks, once on
    an engine created under CAPDEC_SAMPLE_ROWS=7, where beam 5's 80 cond rows cross logits blocks inside captions."""
    from capdec_amd import _capi
    from capdec_amd.engine import Engine
    dims, sd, prefix, stop = _tiny_case()
    old = os.environ.get("CAPDEC_SAMPLE_ROWS")
    if sample_rows is not None:
        os.environ["CAPDEC_SAMPLE_ROWS"] = str(sample_rows)
    try:
        e = Engine(0)
    finally:
        if sample_rows is not None:
            if old is None:
                del os.environ["CAPDEC_SAMPLE_ROWS"]
            else:
                os.environ["CAPDEC_SAMPLE_ROWS"] = old
    try:
        e.load_gpt2(sd, n_head=dims.n_head)
        e.set_batch_invariant(True)
        ctx = P + T12 - 1
        for name in ("greedy_g15_per", "beam5_g15_per"):
            case = (1 if name.startswith("greedy") else 5, 1.5, "per", False)
            beam = case[0]
            _capi.check(e.lib.capdec_set_kv_budget(e._h, 192 << 30), "budget")
            res = _run(e, case)
            assert e.decode_chunks() == 1
            per_pair = 2 * beam * ctx * dims.n_embd * 2 * 4 * dims.n_layer
            _capi.check(e.lib.capdec_set_kv_budget(e._h, per_pair * 6 + per_pair // 2), "budget")
            chunked = _run(e, case)
            assert e.decode_chunks() == 3
            for a, b in zip(chunked, res):
                np.testing.assert_array_equal(a, b)
            for r in range(16):
                one = _run(e, case, rows=slice(r, r + 1))
                for a, b in zip(one, res):
                    np.testing.assert_array_equal(a[0], b[r])
            same, skipped = _vs_definition(res, _tiny_def(*case), list(range(16)), f"hip guided {name}, batch-invariant")
            assert same + skipped == 16 and same >= 14
    finally:
        e.close()


@functools.lru_cache(maxsize=None)
def _small_def(beam):
    dims, sd = DIMS["small"], _weights("small")
    prefix, neg = _prefix("small", 8)[:4].contiguous(), _prefix("small", 4, 3).contiguous()
    if beam == 1:
        return GD.guided_greedy(sd, prefix, neg, 1.5, PD.Proc(), -1, T12, -1, dims.n_head)
    return GD.guided_beam(sd, prefix, neg, 1.5, PD.Proc(), beam, -1, T12, 1.0, dims.n_head)


@pytest.mark.gpu
@pytest.mark.parametrize("beam", [1, 5])
def test_real_vocabulary(eng, beam):
    """GPT-2 small's geometry (12 layers, V = 50257, ld = 50304: the combine kernel's 16-byte accesses and pad columns over
    393 tiles' worth of row), 4 captions, gamma 1.5 with per-caption negatives, T 12, nothing stops; the margin rule
    decides"""
    dims, sd = DIMS["small"], _weights("small")
    prefix, neg = _prefix("small", 8)[:4].contiguous(), _prefix("small", 4, 3).contiguous()
    eng.load_gpt2(sd, n_head=dims.n_head)
    want = _small_def(beam)
    print(f"definition, small geometry, beam {beam}: margins", _margin(want))
    got = _np(eng.decode_guided(prefix, neg, 1.5, -1, beam, T12, 1.0, -1, return_order=True))
    assert (got[1] == T12).all() and got[0].min() >= 0 and got[0].max() < dims.vocab
    same, skipped = _vs_definition(got, want, list(range(4)), f"hip guided, small geometry, beam {beam}")
    assert same + skipped == 4


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(golden):
    """guidance_scale 0.5 / NaN / inf, neg_n neither 1 nor n, a beam outside 1..8 and a context one position too long are
    refused on the host through capdec_last_error; after each refusal a plain greedy decode gives the fixture's ids"""
    from capdec_amd import _capi
    from capdec_amd.engine import Engine
    g, dims = golden("decode_tiny"), synth.GPT2_TINY
    sd = synth.hot_state_dict(42, "mlp", 640, 10, dims=dims)
    pe, stop = torch.from_numpy(g["greedy_prefix_embed"]), int(g["greedy_stop_id"])
    n = int(pe.shape[0])
    assert n > 2
    e = Engine(0)
    try:
        e.load_gpt2(sd, n_head=dims.n_head)

        def still_fine():
            gi, gl = e.decode_greedy(pe, stop, 12, 764)
            np.testing.assert_array_equal(gi.cpu().numpy(), g["greedy_ids_T12"])
            np.testing.assert_array_equal(gl.cpu().numpy(), g["greedy_lens_T12"])

        raw = lambda gamma, neg=pe[:1], beam=1, T=12: e._decode_guided(pe, neg.contiguous(), gamma, stop, beam, T, 1.0, 764)
        for gamma in (0.5, float("nan"), float("inf"), -float("inf"), 0.0):
            with pytest.raises(_capi.CapdecError, match="guidance_scale"):
                raw(gamma)
            still_fine()
        with pytest.raises(_capi.CapdecError, match="neg_n"):
            raw(1.5, pe[:2])
        still_fine()
        for beam in (0, 9):
            with pytest.raises(_capi.CapdecError, match="beam"):
                raw(1.5, beam=beam)
        still_fine()
        T_long = dims.n_pos - 10 + 2
        with pytest.raises(_capi.CapdecError, match="n_positions"):
            raw(1.5, T=T_long)
        still_fine()
        ids, lens = _np(raw(1.5, T=T_long - 1))                 # the longest context the plain calls take
        _check_structure(ids, lens, T_long - 1, [stop, 764])
        ids, lens = _np(raw(1.5, pe))
        _check_structure(ids, lens, 12, [stop, 764])
        still_fine()
    finally:
        e.close()


@pytest.mark.gpu
def test_bf16_mode_runs():
    """bf16 GEMM operands and KV cache: the call runs, lengths are valid, scores are finite (nothing is compared)"""
    from capdec_amd.engine import Engine
    dims, sd, prefix, stop = _tiny_case()
    e = Engine(0)
    try:
        e.set_gemm_mode("bf16")
        e.load_gpt2(sd, n_head=dims.n_head)
        ids, lens = _np(e.decode_guided(prefix, _negative("mean"), 1.5, stop, 1, T12, 1.0, -1))
        _check_structure(ids, lens, T12, [stop])
        assert (ids >= 0).all() and (ids < dims.vocab).all()
        ids, lens, scores = _np(e.decode_guided(prefix, _negative("per"), 1.5, stop, 5, T12))
        _check_structure(ids, lens, T12, [stop])
        assert np.isfinite(scores).all() and (scores <= 0).all() and (np.diff(scores, axis=1) <= 0).all()
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
    """generate_guided_batch decodes what decode_guided_ids returns; generate_guided(embed=...) is row 0 of the batch form for
    beam 1 (a string) and beam 5 (the list of beams); negative_embed=None is model.clip_project(zeros); model.logits_processors
    is honoured and cleared from the engine after the call"""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd._capi import CapdecError
    from capdec_amd.engine import LogitsProcessors
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    dims, sd, prefix, _ = _tiny_case()
    model = ClipCaptionModel(P, prefix_dim=512, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0").eval()
    model.load_state_dict(sd)
    tok = _Tok()
    text = lambda row, L: " ".join(str(int(t)) for t in row[:L])
    emb, neg = prefix[:4], _negative("per")[:4]
    ids, lens = _np(E.decode_guided_ids(model, emb, neg, 13, 1.5, 1, T12))
    _check_structure(ids, lens, T12, [13, 764])
    texts = E.generate_guided_batch(model, tok, emb, neg, 1.5, 1, T12)
    assert texts == [text(ids[r], lens[r]) for r in range(4)]
    assert texts != E.generate2_batch(model, tok, emb, T12)
    assert E.generate_guided_batch(model, tok, emb, neg, 1.0, 1, T12) == E.generate2_batch(model, tok, emb, T12)
    bi, bl, bs = _np(E.decode_guided_ids(model, emb, neg, 13, 1.5, 5, T12))
    beams = E.generate_guided_batch(model, tok, emb, neg, 1.5, 5, T12)
    assert beams == [[text(bi[r, b], bl[r, b]) for b in range(5)] for r in range(4)]
    one = E.generate_guided(model, tok, embed=emb[:1].to("cuda:0"), negative_embed=neg[:1], entry_length=T12)
    assert isinstance(one, str) and one == texts[0]
    assert E.generate_guided(model, tok, embed=emb[:1], negative_embed=neg[0], beam_size=5, entry_length=T12) == beams[0]
    with pytest.raises(CapdecError):
        E.generate_guided(model, tok, embed=emb[:2], negative_embed=neg[:1], entry_length=T12)
    # the default negative: the mapper's output for the all-zero CLIP embedding
    zero = model.clip_project(torch.zeros(1, 512, device="cuda:0")).reshape(1, P, -1)
    assert E.generate_guided_batch(model, tok, emb, None, 1.5, 1, T12) == E.generate_guided_batch(model, tok, emb, zero, 1.5, 1, T12)
    assert E.generate_guided(model, tok, embed=emb[2:3], entry_length=T12) == \
        E.generate_guided(model, tok, embed=emb[2:3], negative_embed=zero, entry_length=T12)
    assert E.generate_guided(model, tok, embed=emb[2:3], beam_size=5, entry_length=T12) == \
        E.generate_guided_batch(model, tok, emb[2:3], zero, 1.5, 5, T12)[0]
    # model.logits_processors
    model.logits_processors = LogitsProcessors(repetition_penalty=1.3, no_repeat_ngram_size=2)
    with_p = E.generate_guided(model, tok, embed=emb[:1], negative_embed=neg[:1], entry_length=T12)
    model.logits_processors = None
    wi, wl = _np(E.decode_guided_ids(model, emb[:1], neg[:1], 13, 1.5, 1, T12, repetition_penalty=1.3, no_repeat_ngram_size=2))
    assert with_p == text(wi[0], wl[0]) and with_p != one
    assert E.generate_guided(model, tok, embed=emb[:1], negative_embed=neg[:1], entry_length=T12) == one      # cleared
