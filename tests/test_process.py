"""Logits processors (``capdec_set_logits_processors`` / ``capdec_set_logit_bias``; ``Engine.decode_*`` keywords) against the
fp64 restatement of their contract in tests/process_def.py.

Bounds.  The project's logits bar is delta = 2e-4 (absolute, HIP against the CPU oracle).  The repetition penalty multiplies
or divides a logit by theta, so a processed logit carries at most delta * max(theta, 1 / theta), and the difference of two
of them eps = 2 delta max(theta, 1 / theta): a greedy token may legitimately differ from the fp64 arg-max only where the
processed top-2 gap is below eps.  So every token the HIP path emits must have a processed fp64 logit within eps of its
step's maximum (processed on the oracle's logits, along the HIP trajectory), and at most 1 % of a case's steps may be
ambiguous (top-2 gap < eps) -- asserted on the CPU for the oracle alone, and again on the GPU along the HIP trajectory.
Beam search is compared with the definition's beam loop through the margin mechanism of tests/test_hip_parity.py: a
caption may differ only where two adjacent candidate keys among its best beam + 1 come within 1e-4 at some step.  Sampling:
the accepted set of tests/test_sample.py on the processed logits, with the top_k boundary taken eps below and above as well.
"""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import process_def as PD
from capdec_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA = 2e-4
AMBIGUOUS_CAP = 0.01          # greedy: share of steps whose processed top-2 gap is below eps
SAMPLE_AMBIGUOUS_CAP = 0.03   # sampling: tests/test_sample.py's cap
KEY_GAP = 1e-4                # beam: a decision between two adjacent keys closer than this is a numerical tie
P, T12 = 10, 12
DIMS = {"tiny": synth.GPT2_TINY, "small": synth.GPT2_SMALL}


def _eps(p):
    return 2.0 * DELTA * p.scale


# ------------------------------------------------------------------------------------- cases (computed once, shared)
@functools.lru_cache(maxsize=None)
def _weights(geom, stop_bias=False):
    sd = synth.hot_state_dict(42, "mlp", 512, P, dims=DIMS[geom])
    return synth.with_stop_bias(sd, 13, 10.0) if stop_bias else sd


@functools.lru_cache(maxsize=None)
def _prefix(geom, n, seed=0, stop_bias=False):
    """hot weights (seed 42, MLP mapper, P 10) and the oracle's prefix embeddings of n synthetic CLIP rows"""
    from oracle import capdec_oracle as O
    x = synth.synthetic_clip_embeddings(n, 512, seed=seed)
    return O.clip_project(x, _weights(geom, stop_bias), "mlp", P).reshape(n, P, -1)


@functools.lru_cache(maxsize=None)
def _plain(geom, n, T):
    """the unprocessed greedy decode of the case (definition, nothing stops) -> ids [n, T]"""
    dims = DIMS[geom]
    return PD.greedy(_weights(geom), _prefix(geom, n), PD.Proc(), dims.vocab + 5, T, -1, dims.n_head)[0]


def _early_token(ids):
    """the token an unprocessed run emits most often in its first three steps: the stop id of the min_length cases"""
    return int(np.bincount(ids[:, :3].reshape(-1)).argmax())


def _bias(V, ids, avoid):
    """+4 on six ids and -inf on three, among them the unprocessed run's most frequent token (never `avoid`: the stop id)"""
    counts = np.bincount(ids.reshape(-1), minlength=V)
    counts[avoid] = -1
    hot = int(counts.argmax())
    rng = np.random.default_rng(5)
    rest = [int(t) for t in rng.permutation(V) if t not in (hot, avoid)][:8]
    b = np.zeros(V, dtype=np.float32)
    b[[hot] + rest[:2]] = -np.inf
    b[rest[2:]] = 4.0
    return b


#: name -> (geometry, captions, steps, which processors)
GREEDY_CASES = {
    "theta1.3": ("tiny", 32, T12, dict(theta=1.3)),
    "theta0.8": ("tiny", 32, T12, dict(theta=0.8)),
    "m2": ("tiny", 32, T12, dict(m=2)),
    "m1": ("tiny", 32, T12, dict(m=1)),
    "minlen4": ("tiny", 32, T12, dict(min_len=4)),
    "bias": ("tiny", 32, T12, dict(bias=True)),
    "all": ("tiny", 32, T12, dict(theta=1.3, m=2, min_len=4, bias=True)),
    "small_all": ("small", 8, T12, dict(theta=1.3, m=2, min_len=4, bias=True)),
    "T67_m3": ("tiny", 32, 67, dict(m=3)),
}


@functools.lru_cache(maxsize=None)
def _greedy_case(name):
    """-> dims, sd, prefix, T, Proc, stop id (the early token where min_length acts, else a token that never comes)"""
    geom, n, T, kw = GREEDY_CASES[name]
    dims = DIMS[geom]
    plain = _plain(geom, n, T)
    stop = _early_token(plain) if kw.get("min_len") else dims.vocab + 5
    kw = dict(kw)
    if kw.pop("bias", False):
        kw["bias"] = _bias(dims.vocab, plain, stop if stop < dims.vocab else -1)
    return dims, _weights(geom), _prefix(geom, n), T, PD.Proc(**kw), stop


@functools.lru_cache(maxsize=None)
def _beam_case(n=16):
    """tiny geometry, (1.3, 2, 4) and a bias; the stop id is the early token of the unprocessed greedy run"""
    dims = DIMS["tiny"]
    plain = _plain("tiny", 32, T12)
    stop = _early_token(plain)
    p = PD.Proc(theta=1.3, m=2, min_len=4, bias=_bias(dims.vocab, plain, stop))
    return dims, _weights("tiny"), _prefix("tiny", 32)[:n].contiguous(), p, stop


@functools.lru_cache(maxsize=None)
def _beam_def(B, n):
    dims, sd, prefix, p, stop = _beam_case()
    mg = []
    tok, seq, sc = PD.beam(sd, prefix[:n], p, B, stop, T12, n_head=dims.n_head, margins=mg)
    return tok, seq, sc, mg[0]


SAMPLE_PROC = PD.Proc(theta=1.2, top_k=20)
SAMPLE_T, SAMPLE_TOP_P = 0.7, 0.8


@functools.lru_cache(maxsize=None)
def _uniforms(n, T):
    return torch.rand(n, T, generator=torch.Generator().manual_seed(4321))


def _check_greedy_steps(logits, ids, lens, p, stops, what):
    """logits [n, T, V] (oracle, teacher-forced on ids): every emitted token's processed fp64 logit within eps of its
    step's maximum -> (ambiguous share, smallest top-2 gap)"""
    eps = _eps(p)
    bad, ambiguous, steps, worst, smallest = [], 0, 0, 0.0, np.inf
    for r in range(ids.shape[0]):
        for i in range(int(lens[r])):
            q = PD.process(logits[r, i], ids[r, :i], p, stops)
            short = float(q.max() - q[int(ids[r, i])])
            gap = PD.top2_gap(q)
            worst, smallest = max(worst, short), min(smallest, gap)
            ambiguous += gap < eps
            steps += 1
            if not short <= eps:
                bad.append((r, i, int(ids[r, i]), int(np.argmax(q)), short))
    share = ambiguous / float(steps)
    print(f"{what}: {steps} steps, eps {eps:.2e}, smallest top-2 gap {smallest:.2e}, ambiguous share {100 * share:.2f} %, "
          f"largest shortfall of an emitted token {worst:.2e}, tokens outside eps {len(bad)}")
    assert not bad, bad[:8]
    assert share <= AMBIGUOUS_CAP, share
    return share, smallest


def _check_stop_structure(ids, lens, T, stops, min_len=0):
    for r in range(ids.shape[0]):
        L = int(lens[r])
        assert 1 <= L <= T
        assert not np.isin(ids[r, :L - 1], stops).any(), (r, ids[r])
        assert L == T or ids[r, L - 1] in stops, (r, ids[r])
        assert L == T or L > min_len, (r, L)
        assert (ids[r, L:] == 0).all(), (r, ids[r])


# ===================================================================================== CPU: the definition
def _hf_process(l, g, theta, m, min_len, stop, top_k):
    """the installed transformers classes in the contract's order (no bias: transformers has no such processor)"""
    from transformers import (MinLengthLogitsProcessor, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                              TopKLogitsWarper)
    ids = torch.tensor([list(g)], dtype=torch.long)
    s = torch.from_numpy(np.array(l, dtype=np.float64))[None, :]
    if theta != 1.0:
        s = RepetitionPenaltyLogitsProcessor(theta)(ids, s)
    if m > 0:
        s = NoRepeatNGramLogitsProcessor(m)(ids, s)
    if min_len > 0:
        s = MinLengthLogitsProcessor(min_len, stop)(ids, s)
    if top_k > 0:
        s = TopKLogitsWarper(top_k)(ids, s)
    return s[0].numpy()


@pytest.mark.parametrize("V", [1531, 50257])
def test_definition_is_the_transformers_processors(V):
    """process_def == transformers' RepetitionPenalty / NoRepeatNGram / MinLength / TopK classes on random logits (std 4,
    some exactly 0) and random histories: with duplicate tokens, over a small alphabet so that n-grams do repeat, at
    m = 1, 2, 3, at i < m - 1 (nothing banned) and at i = 0, with penalties on both sides of 1"""
    rng = np.random.default_rng(V)
    seen_ban = seen_short = seen_zero = 0
    for trial in range(24):
        l = rng.standard_normal(V) * 4.0
        i = [0, 1, 2, 5, 11, 40][trial % 6]
        alphabet = rng.choice(V, size=4, replace=False)
        g = [int(t) for t in rng.choice(alphabet, size=i)]
        l[rng.choice(V, size=5, replace=False)] = 0.0
        if i:
            l[g[0]] = 0.0                                      # a penalised logit that is exactly 0
            seen_zero += 1
        theta = [1.3, 0.8, 1.0, 2.0][trial % 4]
        m = [1, 2, 3, 0][(trial // 2) % 4]
        min_len = [0, 4, 50][trial % 3]
        top_k = [0, 20, 1, V + 3][trial % 4]
        stop = int(alphabet[1])
        p = PD.Proc(theta=theta, m=m, min_len=min_len, top_k=top_k)
        mine = PD.process(l, g, p, (stop,), top_k=True)
        ref = _hf_process(l, g, theta, m, min_len, stop, top_k)
        np.testing.assert_array_equal(mine, ref)
        seen_ban += len(PD.banned_ngram(g, m)) > 0
        seen_short += m > 0 and i < m - 1
        if i >= 2 and len(set(g)) < len(g) and theta != 1.0:   # a token that occurs twice is penalised once
            j = max(set(g), key=g.count)
            want = l[j] / theta if l[j] > 0 else l[j] * theta
            once = PD.process(l, g, PD.Proc(theta=theta), ())
            assert once[j] == want
    assert seen_ban >= 6 and seen_short >= 1 and seen_zero >= 12


def test_definition_edges():
    """m = 1 bans every token of the history; ties at the top_k boundary stay; -inf in the bias bans; the order is penalty,
    bias, bans: a banned token stays banned whatever its bias, and the bias is not penalised"""
    l = np.array([1.0, 2.0, -1.0, 2.0, 0.5, 3.0])
    assert np.isneginf(PD.process(l, [1, 4, 1], PD.Proc(m=1), ())).tolist() == [False, True, False, False, True, False]
    assert np.isneginf(PD.process(l, [], PD.Proc(m=1), ())).sum() == 0
    assert np.isneginf(PD.top_k_filter(l, 2)).tolist() == [True, False, True, False, True, False]      # 3.0 and both 2.0
    assert np.isneginf(PD.top_k_filter(l, 1)).sum() == 5 and np.isneginf(PD.top_k_filter(l, 6)).sum() == 0
    b = np.array([0.0, 5.0, 0.0, -np.inf, 0.0, 0.0])
    q = PD.process(l, [1, 2], PD.Proc(theta=2.0, bias=b), ())
    assert q.tolist() == [1.0, 2.0 / 2.0 + 5.0, -1.0 * 2.0, -np.inf, 0.5, 3.0]
    q = PD.process(l, [5, 0, 5], PD.Proc(m=2, bias=np.full(6, 7.0)), ())      # "5 0" came before: 0 is banned after 5
    assert np.isneginf(q).tolist() == [True, False, False, False, False, False]
    assert PD.banned_ngram([3, 4, 3, 4, 3], 3) == [4] and PD.banned_ngram([3], 3) == [] and PD.banned_ngram([3, 4], 3) == []
    q = PD.process(l, [0, 1], PD.Proc(min_len=3), (5, 2))
    assert np.isneginf(q).tolist() == [False, False, True, False, False, True]
    assert not np.isneginf(PD.process(l, [0, 1, 1], PD.Proc(min_len=3), (5, 2))).any()


def test_everything_off_is_the_oracle():
    """with no processor set the definition's greedy loop is O.greedy_cached and its beam loop O.beam_cached, exactly"""
    from oracle import capdec_oracle as O
    dims, sd, prefix = DIMS["tiny"], _weights("tiny", True), _prefix("tiny", 8, 0, True)
    ids, lens, _ = PD.greedy(sd, prefix, PD.Proc(), 13, T12, 764, dims.n_head)
    oi, ol = O.greedy_cached(sd, prefix, 13, T12, 764, dims.n_head)
    np.testing.assert_array_equal(ids, oi.numpy())
    np.testing.assert_array_equal(lens, ol.numpy())
    assert lens.min() < T12
    tok, seq, sc = PD.beam(sd, prefix, PD.Proc(), 5, 13, T12, n_head=dims.n_head)
    ot, os_, oc = O.beam_cached(sd, prefix, 5, 13, T12, n_head=dims.n_head)
    np.testing.assert_array_equal(tok.numpy(), ot.numpy())
    np.testing.assert_array_equal(seq.numpy(), os_.numpy())
    np.testing.assert_array_equal(sc.numpy(), oc.numpy())


# ===================================================================================== CPU: conditions of the GPU tests
@pytest.mark.parametrize("name", list(GREEDY_CASES))
def test_greedy_ambiguity_cap_oracle_alone(name):
    """the acceptance of the GPU test is narrow: along the definition's own greedy trajectory at most 1 % of the steps have
    a processed top-2 gap below eps = 2 delta max(theta, 1 / theta), and the full setting bites -- at least half of the
    captions differ from the unprocessed decode.  Measured (oracle alone; steps / eps / smallest top-2 gap / ambiguous
    steps / captions changed): theta1.3 384 / 5.2e-4 / 5.3e-4 / 0 / 31 of 32; theta0.8 384 / 5.0e-4 / 3.2e-3 / 0 / 31; m2 384 /
    4.0e-4 / 3.2e-3 / 0 / 20; m1 384 / 4.0e-4 / 5.3e-4 / 0 / 31; minlen4 349 / 4.0e-4 / 3.2e-3 / 0 / 12; bias 384 / 4.0e-4 /
    3.9e-3 / 0 / 26; all 336 / 5.2e-4 / 6.1e-3 / 0 / 32; small geometry, all (8 captions) 84 / 5.2e-4 / 2.6e-2 / 0 / 8 of 8;
    T67_m3 2144 / 4.0e-4 / 2.6e-4 / 1 (0.05 %) / 29."""
    dims, sd, prefix, T, p, stop = _greedy_case(name)
    geom, n = GREEDY_CASES[name][:2]
    ids, lens, gaps = PD.greedy(sd, prefix, p, stop, T, -1, dims.n_head)
    _check_stop_structure(ids, lens, T, [stop], p.min_len)
    live = np.arange(T)[None, :] < lens[:, None]
    share = float((gaps[live] < _eps(p)).mean())
    changed = int((ids != _plain(geom, n, T)).any(axis=1).sum())
    print(f"oracle {name}: {int(live.sum())} steps, eps {_eps(p):.2e}, smallest top-2 gap {gaps[live].min():.2e}, "
          f"ambiguous share {100 * share:.2f} %, captions changed {changed} of {n}")
    assert share <= AMBIGUOUS_CAP, share
    if name in ("all", "small_all"):
        assert 2 * changed >= n, changed
    if p.bias is not None:
        assert not np.isin(ids[live], np.nonzero(np.isneginf(p.bias))[0]).any()
    if p.m:
        for r in range(n):
            grams = [tuple(ids[r, s:s + p.m]) for s in range(int(lens[r]) - p.m + 1)]
            assert len(grams) == len(set(grams)), (r, ids[r])


@pytest.mark.parametrize("B,n", [(5, 16), (3, 4), (8, 4)])
def test_beam_margin_cap_oracle_alone(B, n):
    """the margin mechanism leaves the GPU beam test something to assert: among the 16 captions of the beam-5 case at most 2
    have a decision between adjacent keys of their best six closer than 1e-4.  Measured (definition alone, tiny geometry,
    (1.3, 2, 4) + bias): beam 5: smallest gap 1.01e-4, 0 of 16 captions below 1e-4; beam 3 (4 captions): 4.7e-4, 0; beam 8
    (4 captions): 2.6e-4, 0."""
    tok, seq, sc, margin = _beam_def(B, n)
    unclear = int((margin < KEY_GAP).sum())
    print(f"definition beam {B}, {n} captions: smallest adjacent key gap {float(margin.min()):.2e}, captions below {KEY_GAP:g}: {unclear}")
    assert torch.isfinite(sc).all()
    if (B, n) == (5, 16):
        assert unclear <= 2, unclear
    dims, sd, prefix, p, stop = _beam_case()
    banned = np.nonzero(np.isneginf(p.bias))[0]
    t, s = tok.numpy(), seq.numpy()
    for r in range(n):
        for b in range(B):
            L = int(s[r, b])
            assert not np.isin(t[r, b, :L], banned).any()
            assert L == T12 or (L > p.min_len and t[r, b, L - 1] == stop), (r, b, t[r, b])
            grams = [tuple(t[r, b, k:k + 2]) for k in range(L - 1)]
            assert len(grams) == len(set(grams)), (r, b, t[r, b])


def _check_sample_steps(logits, ids, u, logp, what):
    """logits [n, T, V] (oracle, teacher-forced on ids): every token in its step's accepted set -> ambiguous share"""
    p, temperature, top_p = SAMPLE_PROC, SAMPLE_T, SAMPLE_TOP_P
    eps_l, eps_p = _eps(p), _eps(p) / temperature
    n, T = ids.shape
    ambiguous, bad, worst = 0, [], 0.0
    for r in range(n):
        for i in range(T):
            l14 = PD.process(logits[r, i], ids[r, :i], p, ())
            acc = PD.sample_accepted(l14, p, temperature, top_p, float(u[r, i]), eps_l, eps_p, eps_p)
            ambiguous += len(acc) > 1
            if int(ids[r, i]) not in acc:
                bad.append((r, i, int(ids[r, i]), sorted(acc)))
            if logp is not None:
                worst = max(worst, abs(float(logp[r, i]) - PD.logp_of(l14, int(ids[r, i]), temperature)))
    share = ambiguous / float(n * T)
    print(f"{what}: {n * T} steps, ambiguous share {100 * share:.2f} %, picks outside the accepted set {len(bad)}, "
          f"max |logp - fp64| {worst:.2e} (bound {eps_p:.2e})")
    assert not bad, bad[:8]
    assert share <= SAMPLE_AMBIGUOUS_CAP, share
    if logp is not None:
        assert worst <= eps_p, worst
    return share


def test_sampling_ambiguity_cap_oracle_alone():
    """tiny geometry, temperature 0.7, top_p 0.8, top_k 20, theta 1.2, 32 captions x 12 steps of fixed uniforms: along the
    definition's own trajectory at most 3 % of the steps accept more than one token (measured: 1.56 % of 384)"""
    dims = DIMS["tiny"]
    u = _uniforms(32, T12).numpy()
    ids, logits = PD.sample_decode(_weights("tiny"), _prefix("tiny", 32), SAMPLE_PROC, SAMPLE_T, SAMPLE_TOP_P, u, dims.n_head)
    _check_sample_steps(logits, ids, u, None, "definition, sampling")


# ===================================================================================== CPU: host logic
def test_header_binding_and_struct():
    """both symbols are declared and bound, the ABI number is still 6, the struct mirrors the header's"""
    from capdec_amd import _capi
    header = open(os.path.join(ROOT, "include", "capdec.h")).read()
    assert re.search(r"\bint\s+capdec_set_logits_processors\s*\(", header)
    assert re.search(r"\bint\s+capdec_set_logit_bias\s*\(", header)
    assert re.search(r"typedef struct \{ float repetition_penalty; int no_repeat_ngram_size; int min_length; int top_k; \} "
                     r"capdec_logits_processors;", header)
    assert re.search(r"#define\s+CAPDEC_ABI_VERSION\s+6\b", header) and _capi.ABI_VERSION == 6
    assert [f[0] for f in _capi.LogitsProcessors._fields_] == ["repetition_penalty", "no_repeat_ngram_size", "min_length", "top_k"]
    assert C.sizeof(_capi.LogitsProcessors) == 16 and _capi.LogitsProcessors.repetition_penalty.offset == 0
    lib = _capi.load_library()
    assert hasattr(lib, "capdec_set_logits_processors") and hasattr(lib, "capdec_set_logit_bias")
    assert lib.capdec_set_logits_processors(None, None) != 0 and b"null context" in lib.capdec_last_error()
    for ignoring in ("capdec_decode_greedy_forced", "capdec_score", "capdec_gpt2_logits", "train step"):
        assert ignoring in header[header.index("IGNORE the processors") - 200:header.index("IGNORE the processors")]


def test_argument_checks():
    from capdec_amd._capi import CapdecError
    from capdec_amd.engine import LogitsProcessors
    assert not LogitsProcessors().active and LogitsProcessors.of(None) is None
    assert LogitsProcessors.of(None, repetition_penalty=1.0, min_length=0) is None
    assert LogitsProcessors(top_k=3).active and LogitsProcessors(logit_bias=[0.0]).active
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.3), dict(repetition_penalty=float("nan")),
               dict(repetition_penalty=float("inf")), dict(repetition_penalty="2"), dict(no_repeat_ngram_size=-1),
               dict(min_length=-4), dict(top_k=-1), dict(top_k=2.5), dict(min_length=True)):
        with pytest.raises(CapdecError):
            LogitsProcessors(**kw)
    base = LogitsProcessors(repetition_penalty=1.3, min_length=4)
    p = LogitsProcessors.of(base, min_length=6, top_k=None)
    assert (p.repetition_penalty, p.min_length, p.top_k) == (1.3, 6, 0)
    with pytest.raises(CapdecError):
        LogitsProcessors.of(dict(repetition_penalty=1.3))


class _FakeLib:
    """records the two state calls; everything succeeds"""

    def __init__(self):
        self.calls = []

    def capdec_set_logits_processors(self, h, p):
        st = None if p is None else p._obj
        self.calls.append(("proc", None if st is None else (round(st.repetition_penalty, 6), st.no_repeat_ngram_size,
                                                             st.min_length, st.top_k)))
        return 0

    def capdec_set_logit_bias(self, h, b, n):
        self.calls.append(("bias", None if b is None else [b[i] for i in range(n)]))
        return 0


def test_set_call_clear_also_when_the_call_raises():
    from capdec_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.lib, e._h = _FakeLib(), None
    seen = []
    e._decode_greedy = lambda *a: seen.append(("greedy", list(e.lib.calls))) or "G"
    e._decode_beam = lambda *a: seen.append(("beam", list(e.lib.calls))) or "B"
    e._decode_sample = lambda *a: seen.append(("sample", list(e.lib.calls))) or "S"
    pe = torch.zeros(2, P, 8)
    assert Engine.decode_greedy(e, pe, 13, 12) == "G" and e.lib.calls == []          # nothing given: the state is not touched
    assert Engine.decode_greedy(e, pe, 13, 12, repetition_penalty=1.3, logit_bias=[0.0, -np.inf, 2.0]) == "G"
    assert seen[-1][1] == [("proc", (1.3, 0, 0, 0)), ("bias", [0.0, -np.inf, 2.0])]           # set before the call ...
    assert e.lib.calls[2:] == [("proc", None), ("bias", None)]                                  # ... cleared after it
    e.lib.calls.clear()
    assert Engine.decode_beam(e, pe, 13, 5, 12, no_repeat_ngram_size=2, min_length=4) == "B"
    assert e.lib.calls == [("proc", (1.0, 2, 4, 0)), ("proc", None), ("bias", None)]
    e.lib.calls.clear()
    assert Engine.decode_sample(e, pe, 13, 12, top_k=20) == "S"
    assert e.lib.calls == [("proc", (1.0, 0, 0, 20)), ("proc", None), ("bias", None)]
    e.lib.calls.clear()

    def boom(*a):
        raise RuntimeError("decode failed")
    e._decode_greedy = boom
    with pytest.raises(RuntimeError, match="decode failed"):
        Engine.decode_greedy(e, pe, 13, 12, min_length=3)
    assert e.lib.calls == [("proc", (1.0, 0, 3, 0)), ("proc", None), ("bias", None)]


class _FakeTok:
    def encode(self, s):
        return [13]

    def decode(self, toks):
        return " ".join(str(int(t)) for t in toks)


class _FakeEngine:
    def __init__(self):
        self.calls = []

    def decode_greedy(self, embed, stop, T, alt, **kw):
        self.calls.append(("greedy", kw))
        n = embed.shape[0]
        return torch.arange(n * T, dtype=torch.int32).reshape(n, T), torch.full((n,), 3, dtype=torch.int32)

    def decode_beam(self, embed, stop, B, T, temperature, **kw):
        self.calls.append(("beam", kw))
        n = embed.shape[0]
        return (torch.ones(n, B, T, dtype=torch.int32), torch.full((n, B), 2, dtype=torch.int32), torch.zeros(n, B),
                torch.zeros(n, B, dtype=torch.int32))

    def decode_sample(self, embed, stop, T, temperature, top_p, seed, u, alt, return_logp, **kw):
        self.calls.append(("sample", kw))
        n = embed.shape[0]
        return torch.ones(n, T, dtype=torch.int32), torch.full((n,), 2, dtype=torch.int32)


class _FakeModel:
    def __init__(self, processors=None):
        self.engine = _FakeEngine()
        if processors is not None:
            self.logits_processors = processors

    def eval(self):
        return self


def test_generate_functions_pick_up_the_models_processors():
    """generate2 / generate_beam keep the reference's signatures and read model.logits_processors; the batched functions
    start from it and put their own keywords on top; without either, the engine is called exactly as before (no keyword)"""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd import predictions_runner as PR
    from capdec_amd.engine import LogitsProcessors
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    assert list(inspect.signature(E.generate2).parameters) == ["model", "tokenizer", "tokens", "prompt", "embed", "entry_count",
                                                               "entry_length", "top_p", "temperature", "stop_token"]
    assert list(inspect.signature(E.generate_beam).parameters) == ["model", "tokenizer", "beam_size", "prompt", "embed",
                                                                   "entry_length", "temperature", "stop_token"]
    for fn in (E.decode_greedy_ids, E.decode_beam_ids, E.sample_ids, E.generate2_batch, E.generate_beam_batch,
               E.generate_samples, E.generate_samples_batch, PR.caption_ids, PR.make_preds, PR.make_preds_from_images,
               PR.make_preds_from_captions):
        sig = inspect.signature(fn).parameters
        for name in ("repetition_penalty", "no_repeat_ngram_size", "min_length", "logit_bias"):
            assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is None, (fn.__name__, name)
        assert ("top_k" in sig) == (fn in (E.sample_ids, E.generate_samples, E.generate_samples_batch)), fn.__name__
    assert ClipCaptionModel(P, prefix_dim=512, mapping_type=MappingType.MLP, gpt2_dims=synth.GPT2_TINY).logits_processors is None
    pe = torch.zeros(1, P, 8)
    plain = _FakeModel()
    E.generate2(plain, _FakeTok(), embed=pe, entry_length=12)
    E.generate_beam(plain, _FakeTok(), embed=pe, entry_length=12)
    E.generate2_batch(plain, _FakeTok(), pe, 12)
    E.generate_samples(plain, _FakeTok(), embed=pe, entry_length=12, seed=1)
    assert plain.engine.calls == [("greedy", {}), ("beam", {}), ("greedy", {}), ("sample", {})]
    bias = np.zeros(4, dtype=np.float32)
    m = _FakeModel(LogitsProcessors(repetition_penalty=1.3, no_repeat_ngram_size=2, top_k=7, logit_bias=bias))
    E.generate2(m, _FakeTok(), embed=pe, entry_length=12)
    E.generate_beam(m, _FakeTok(), embed=pe, entry_length=12)
    E.generate_beam_batch(m, _FakeTok(), pe, 5, 12, min_length=4, repetition_penalty=1.0)
    E.generate_samples_batch(m, _FakeTok(), pe, 2, 12, seed=1, top_k=9)
    want = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, logit_bias=bias)
    assert m.engine.calls[0] == ("greedy", want) and m.engine.calls[1] == ("beam", want)           # top_k: sampling only
    assert m.engine.calls[2] == ("beam", dict(no_repeat_ngram_size=2, min_length=4, logit_bias=bias))
    assert m.engine.calls[3] == ("sample", dict(want, top_k=9))


# ===================================================================================== GPU
@pytest.fixture(scope="module")
def eng():
    from capdec_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _oracle_logits(sd, prefix, ids, n_head):
    """the logits behind every step of `ids` [n, T]: one causal call over cat(prefix, wte(ids[:, :-1])) -> [n, T, V]"""
    from oracle import capdec_oracle as O
    Pn = prefix.shape[1]
    x = torch.cat((prefix, O.wte(torch.as_tensor(ids[:, :-1], dtype=torch.long), sd)), dim=1)
    return O.gpt2_logits(x, sd, n_head)[:, Pn - 1:].numpy()


def _np(ts):
    return [t.cpu().numpy() for t in ts]


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["tiny", "small"])
def test_zero_bias_forces_the_new_path_and_changes_nothing(golden, geom):
    """a bias of all zeros sends every step through lm_head_logits + logits_process_kernel + logits_select_kernel: greedy ids
    and lens are the reference fixtures' at T 12 and 67, beam tokens, lengths and order are exact and scores within 1e-4.
    The small geometry runs the select kernel at V = 50257 = 785 x 64 + 17 (a row that ends inside a float4 group)."""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    g, dims = golden("decode_" + geom), DIMS[geom]
    zero = np.zeros(dims.vocab, dtype=np.float32)
    model = ClipCaptionModel(10, prefix_dim=640, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0").eval()
    sd = synth.hot_state_dict(42, "mlp", 640, 10, dims=dims)
    assert synth.state_dict_checksum(sd) == int(g["greedy_sd_crc"]), "RNG drift"
    model.load_state_dict(sd)
    pe, stop = torch.from_numpy(g["greedy_prefix_embed"]), int(g["greedy_stop_id"])
    for el in (12, 67):
        ids, lens = _np(E.decode_greedy_ids(model, pe, stop, el, logit_bias=zero))
        np.testing.assert_array_equal(ids, g[f"greedy_ids_T{el}"])
        np.testing.assert_array_equal(lens, g[f"greedy_lens_T{el}"])
    model = ClipCaptionModel(10, clip_length=10, prefix_dim=512, num_layers=8, mapping_type=MappingType.TransformerEncoder,
                             gpt2_dims=dims).to("cuda:0").eval()
    sd = synth.hot_state_dict(42, "transformer_encoder", 512, 10, dims=dims)
    assert synth.state_dict_checksum(sd) == int(g["beam_sd_crc"]), "RNG drift"
    model.load_state_dict(sd)
    pe = torch.from_numpy(g["beam_prefix_embed"])
    for el in (12, 67):
        for name, st in (("nostop", dims.vocab + 5), ("stop", int(g["beam_stop_id"]))):
            ids, lens, scores, order = _np(E.decode_beam_ids(model, pe, st, 5, el, logit_bias=zero))
            gt, gl = g[f"beam_{name}_tokens_T{el}"], g[f"beam_{name}_seqlen_T{el}"]
            gs, go = g[f"beam_{name}_scores_T{el}"], g[f"beam_{name}_order_T{el}"]
            np.testing.assert_array_equal(order, go)
            for r in range(pe.shape[0]):
                np.testing.assert_array_equal(ids[r], gt[r][go[r]])
                np.testing.assert_array_equal(lens[r], gl[r][go[r]].astype(np.int32))
                np.testing.assert_allclose(scores[r], gs[r][go[r]], atol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GREEDY_CASES))
def test_greedy_vs_definition(eng, name):
    """every token the HIP greedy decode emits has a processed fp64 logit (the definition on the oracle's logits, along the
    HIP trajectory) within eps of its step's maximum; at most 1 % of the steps are ambiguous; the rows stop where the
    contract says (never before min_length).  Shares measured for the oracle alone: test_greedy_ambiguity_cap_oracle_alone
    (one ambiguous step, in T67_m3: 0.05 %; small geometry, all processors, 8 captions: smallest gap 2.6e-2 against eps 5.2e-4)."""
    dims, sd, prefix, T, p, stop = _greedy_case(name)
    eng.load_gpt2(sd, n_head=dims.n_head)
    ids, lens = _np(eng.decode_greedy(prefix, stop, T, -1, **p.kw()))
    _check_stop_structure(ids, lens, T, [stop], p.min_len)
    logits = _oracle_logits(sd, prefix, ids, dims.n_head)
    _check_greedy_steps(logits, ids, lens, p, (stop, -1), f"hip greedy {name}")
    if name in ("all", "small_all"):
        geom, n = GREEDY_CASES[name][:2]
        assert 2 * int((ids != _plain(geom, n, T)).any(axis=1).sum()) >= n


def _beam_vs_definition(got, want, rows, what):
    """captions `rows` of a HIP beam result (ids, lens, scores, order) against the definition's (tokens, seq, scores,
    margin) for those captions: every clear caption identical -> (identical, tied and different)"""
    i1, l1, s1, o1 = got
    tok, seq, sc, margin = want
    order = sc.argsort(dim=-1, descending=True)
    clear = (margin > KEY_GAP).numpy()
    same = skipped = 0
    for j, r in enumerate(rows):
        oj = order[j]
        eq = (np.array_equal(o1[r], oj.numpy()) and np.array_equal(i1[r], tok[j][oj].numpy())
              and np.array_equal(l1[r], seq[j][oj].numpy()) and np.allclose(s1[r], sc[j][oj].numpy(), atol=1e-4, rtol=0))
        if eq:
            same += 1
        elif not clear[j]:
            assert np.isfinite(s1[r]).all() and (np.diff(s1[r]) <= 0).all()
            skipped += 1
        else:
            np.testing.assert_array_equal(o1[r], oj.numpy())
            np.testing.assert_array_equal(i1[r], tok[j][oj].numpy())
            np.testing.assert_array_equal(l1[r], seq[j][oj].numpy())
            np.testing.assert_allclose(s1[r], sc[j][oj].numpy(), atol=1e-4)
    print(f"{what}: {len(rows)} captions, {same} identical ({int((~clear).sum())} had a key gap < {KEY_GAP:g}), "
          f"{skipped} differ on such a tie")
    return same, skipped


@pytest.mark.gpu
@pytest.mark.parametrize("B,n", [(5, 16), (3, 4), (8, 4)])
def test_beam_vs_definition(eng, B, n):
    """tiny geometry, (1.3, 2, 4) and a bias, T 12: tokens, lengths, order exact and scores within 1e-4 against the
    definition's beam loop for every caption without a near-tie between adjacent keys; beam 5: at least 15 of 16 identical"""
    dims, sd, prefix, p, stop = _beam_case()
    eng.load_gpt2(sd, n_head=dims.n_head)
    got = _np(eng.decode_beam(prefix[:n], stop, B, T12, **p.kw()))
    same, skipped = _beam_vs_definition(got, _beam_def(B, n), list(range(n)), f"hip beam {B}")
    assert same + skipped == n
    if (B, n) == (5, 16):
        assert same >= 15, same


@pytest.mark.gpu
def test_sampling_vs_definition(eng):
    """temperature 0.7, top_p 0.8, top_k 20, theta 1.2, fixed uniforms: every drawn token in its step's accepted set, at most
    3 % ambiguous steps, logp (the distribution after steps 1-4, before top_k and top_p) within 2 eps / temperature.
    top_k = 1 is exactly the greedy decode with the same processors, top_k >= V is top_k = 0."""
    dims, sd, prefix = DIMS["tiny"], _weights("tiny"), _prefix("tiny", 32)
    p, u, V = SAMPLE_PROC, _uniforms(32, T12), DIMS["tiny"].vocab
    eng.load_gpt2(sd, n_head=dims.n_head)
    run = lambda **kw: _np(eng.decode_sample(prefix, V + 5, T12, SAMPLE_T, SAMPLE_TOP_P, u=u, alt_stop_id=-1,
                                             return_logp=True, repetition_penalty=p.theta, **kw))
    ids, lens, logp = run(top_k=p.top_k)
    assert (lens == T12).all() and ids.min() >= 0 and ids.max() < V
    logits = _oracle_logits(sd, prefix, ids, dims.n_head)
    _check_sample_steps(logits, ids, u.numpy(), logp, "hip sampling")
    gi, gl = _np(eng.decode_greedy(prefix, V + 5, T12, -1, repetition_penalty=p.theta))
    i1, l1, _ = run(top_k=1)
    np.testing.assert_array_equal(i1, gi)
    np.testing.assert_array_equal(l1, gl)
    for a, b in zip(run(top_k=V), run()):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(run(top_k=V + 7), run(top_k=0)):
        np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
def test_row_blocks_compaction_chunks(monkeypatch):
    """a context whose row blocks hold 7 rows (CAPDEC_SAMPLE_ROWS=7), 48 captions that stop, greedy and beam 5 (240 rows:
    block edges fall inside a caption's beams): in batch-invariant mode the ids do not depend on finished-caption
    compaction nor on a KV budget that forces several chunks, and 8 captions spread over the batch match the definition"""
    from capdec_amd import _capi
    from capdec_amd.engine import Engine
    monkeypatch.setenv("CAPDEC_SAMPLE_ROWS", "7")
    e = Engine(0)
    monkeypatch.delenv("CAPDEC_SAMPLE_ROWS")
    try:
        dims, sd, n, T, stop = DIMS["tiny"], _weights("tiny", True), 48, 16, 13
        prefix = _prefix("tiny", n, 0, True)
        plain = PD.greedy(sd, prefix, PD.Proc(), dims.vocab + 5, T, -1, dims.n_head)[0]
        p = PD.Proc(theta=1.3, m=2, min_len=4, bias=_bias(dims.vocab, plain, stop))
        e.load_gpt2(sd, n_head=dims.n_head)
        e.set_batch_invariant(True)
        greedy = lambda: _np(e.decode_greedy(prefix, stop, T, -1, **p.kw()))
        beam = lambda: _np(e.decode_beam(prefix, stop, 5, T, **p.kw()))
        gi, gl = greedy()
        bres = beam()
        _check_stop_structure(gi, gl, T, [stop], p.min_len)
        assert gl.min() < T and len(set(gl.tolist())) > 3 and e.decode_chunks() == 1
        e.set_compact(False)
        for a, b in zip(greedy(), (gi, gl)):
            np.testing.assert_array_equal(a, b)
        assert e.decode_stats()["compactions"] == 0
        for a, b in zip(beam(), bres):
            np.testing.assert_array_equal(a, b)
        e.set_compact(True)
        per_cap = (P + T - 1) * dims.n_embd * 2 * 4 * dims.n_layer
        _capi.check(e.lib.capdec_set_kv_budget(e._h, per_cap * 13), "budget")
        for a, b in zip(greedy(), (gi, gl)):
            np.testing.assert_array_equal(a, b)
        assert e.decode_chunks() == 4 and e.decode_stats()["compactions"] >= 1
        _capi.check(e.lib.capdec_set_kv_budget(e._h, per_cap * 5 * 13), "budget")
        for a, b in zip(beam(), bres):
            np.testing.assert_array_equal(a, b)
        assert e.decode_chunks() == 4
        pick = np.linspace(0, n - 1, 8).astype(np.int64)
        logits = _oracle_logits(sd, prefix[pick], gi[pick], dims.n_head)
        _check_greedy_steps(logits, gi[pick], gl[pick], p, (stop, -1), "hip greedy, 7-row blocks")
        mg = []
        tok, seq, sc = PD.beam(sd, prefix[pick], p, 5, stop, T, n_head=dims.n_head, margins=mg)
        same, skipped = _beam_vs_definition(bres, (tok, seq, sc, mg[0]), list(pick), "hip beam 5, 7-row blocks")
        assert same + skipped == 8 and same >= 7
    finally:
        e.close()


@pytest.mark.gpu
def test_refusals_and_clearing(golden):
    """every refusal reports through capdec_last_error / CapdecError and leaves the context usable; after clearing, greedy
    and beam results are bit-identical to those of a context that never had processors set"""
    from capdec_amd import _capi
    from capdec_amd.engine import Engine, LogitsProcessors
    g, dims = golden("decode_tiny"), DIMS["tiny"]
    V = dims.vocab
    sd = synth.hot_state_dict(42, "mlp", 640, 10, dims=dims)
    pe, stop = torch.from_numpy(g["greedy_prefix_embed"]), int(g["greedy_stop_id"])
    fresh = Engine(0)
    e = Engine(0)
    try:
        with pytest.raises(_capi.CapdecError, match="not loaded"):
            e.set_logit_bias(np.zeros(V, dtype=np.float32))
        for x in (fresh, e):
            x.load_gpt2(sd, n_head=dims.n_head)
        want_g = _np(fresh.decode_greedy(pe, stop, 12))
        want_b = _np(fresh.decode_beam(pe, stop, 5, 12))
        np.testing.assert_array_equal(want_g[0], g["greedy_ids_T12"])
        for bad in ((0.0, 0, 0, 0), (-1.3, 0, 0, 0), (float("nan"), 0, 0, 0), (float("inf"), 0, 0, 0), (1.3, -1, 0, 0),
                    (1.3, 0, -2, 0), (1.3, 0, 0, -3)):
            st = _capi.LogitsProcessors(*bad)
            assert e.lib.capdec_set_logits_processors(e._h, C.byref(st)) != 0, bad
            assert b"set_logits_processors" in e.lib.capdec_last_error()
        few = np.full(V, -np.inf, dtype=np.float32)
        few[:1025] = 0.0
        for b, msg in ((np.zeros(V - 1, dtype=np.float32), "one entry per vocabulary token"),
                       (np.concatenate((np.zeros(V - 1, dtype=np.float32), [np.nan])), "NaN"),
                       (np.concatenate((np.zeros(V - 1, dtype=np.float32), [np.inf])), "inf"), (few, "1026")):
            with pytest.raises(_capi.CapdecError, match=msg):
                e.set_logit_bias(b)
        with pytest.raises(_capi.CapdecError):
            e.decode_greedy(pe, stop, 12, repetition_penalty=0.0)
        with pytest.raises(_capi.CapdecError):
            e.decode_beam(pe, stop, 5, 12, logit_bias=np.zeros(V + 1, dtype=np.float32))
        few[1025] = 0.0                                        # 1026 finite entries: accepted
        e.set_logit_bias(few)
        e.set_logit_bias(None)
        for a, b in zip(_np(e.decode_greedy(pe, stop, 12)), want_g):        # every refusal left the context as it was
            np.testing.assert_array_equal(a, b)
        # persistent state: set, decode, clear
        e.set_logits_processors(LogitsProcessors(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=4))
        bias = np.zeros(V, dtype=np.float32)
        bias[int(np.bincount(want_g[0][:, 0]).argmax())] = -np.inf
        e.set_logit_bias(bias)
        gi, gl = _np(e.decode_greedy(pe, stop, 12))
        assert (gi != want_g[0]).any() and (gl >= np.minimum(5, 12)).all()
        bi = _np(e.decode_beam(pe, stop, 5, 12))[0]
        assert (bi != want_b[0]).any()
        e.set_logits_processors(None)
        e.set_logit_bias(None)
        for a, b in zip(_np(e.decode_greedy(pe, stop, 12)), want_g):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(_np(e.decode_beam(pe, stop, 5, 12)), want_b):
            np.testing.assert_array_equal(a, b)
        # the keyword form clears after itself
        e.decode_greedy(pe, stop, 12, repetition_penalty=1.3, logit_bias=bias)
        for a, b in zip(_np(e.decode_greedy(pe, stop, 12)), want_g):
            np.testing.assert_array_equal(a, b)
    finally:
        e.close()
        fresh.close()
