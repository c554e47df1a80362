"""Nucleus-sampling decode (``capdec_decode_sample`` / ``Engine.decode_sample`` / ``generate_samples*``) against the fp64
restatement of its contract in tests/sample_def.py.

Bounds.  The project's logits bar is delta = 2e-4 (absolute, HIP against the CPU oracle).  A logit error of delta moves a
temperature-scaled logit by delta / temperature, hence an un-normalised probability by that much relatively and a
normalised one -- and any partial sum of them -- by at most 2 delta / temperature.  So a pick may legitimately differ from
the fp64 definition only where top_p or the uniform lies within eps = 2 delta / temperature of a partial sum: the HIP token
has to lie in the set of fp64 picks over the 9 corners (top_p - eps, top_p, top_p + eps) x (u - eps, u, u + eps) at EVERY
step, and at most 3 % of a case's steps may have more than one token in that set (asserted on the CPU for the oracle
alone, and again on the GPU along the HIP path's own trajectory).  logp is the difference of two quantities that each
carry the logits bar: 2 delta / temperature.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import sample_def as D
from capdec_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA = 2e-4
AMBIGUOUS_CAP = 0.03
P, T12, NCAP = 10, 12, 64
#: (geometry, temperature, top_p).  GPT-2-small geometry at temperature 1 (top_p 0.8 / 0.95) stays out: its nuclei hold
#: ~74 tokens and 10 % / 23 % of the steps are ambiguous.
CASES = [("tiny", 1.0, 0.8), ("tiny", 0.7, 0.8), ("tiny", 0.7, 0.95), ("small", 0.7, 0.8)]
#: a vocabulary above 51 200 (50 values per lane): the sampling kernel's variant that re-reads the row instead of holding
#: it in registers.  Two layers like the tiny geometry; the logits have the law of the small geometry's (every vocabulary
#: row is an i.i.d. Gaussian), so the case is small's first one.
GPT2_BIGVOCAB = synth.GPT2Dims(n_layer=2, vocab=51300, n_pos=128)
CASES_ALL = CASES + [("bigvocab", 0.7, 0.8)]
DIMS = {"tiny": synth.GPT2_TINY, "small": synth.GPT2_SMALL, "bigvocab": GPT2_BIGVOCAB}


def _eps(temperature):
    return 2.0 * DELTA / temperature


def _case(geom, n=NCAP, T=T12, seed=0):
    """hot weights (MLP mapper, P 10), the oracle's prefix embeddings of n synthetic CLIP rows, fixed uniforms [n, T]"""
    from oracle import capdec_oracle as O
    dims = DIMS[geom]
    sd = synth.hot_state_dict(42, "mlp", 512, P, dims=dims)
    x = synth.synthetic_clip_embeddings(n, 512, seed=seed)
    prefix = O.clip_project(x, sd, "mlp", P).reshape(n, P, -1)
    u = torch.rand(n, T, generator=torch.Generator().manual_seed(1234 + seed))
    return dims, sd, prefix, u


def _check_steps(logits, ids, u, temperature, top_p, logp=None, what=""):
    """logits [n, T, V] (oracle), ids [n, T], u [n, T]: every token in its step's accepted set; -> ambiguous share"""
    eps = _eps(temperature)
    n, T = ids.shape
    ambiguous, bad, worst_lp = 0, [], 0.0
    for r in range(n):
        for i in range(T):
            acc = D.accepted_set(logits[r, i], temperature, top_p, float(u[r, i]), eps, eps)
            ambiguous += len(acc) > 1
            if int(ids[r, i]) not in acc:
                bad.append((r, i, int(ids[r, i]), sorted(acc)))
            if logp is not None:
                s = D.scaled(logits[r, i], temperature)
                m = s.max()
                want = s[int(ids[r, i])] - (m + math.log(np.exp(s - m).sum()))
                worst_lp = max(worst_lp, abs(float(logp[r, i]) - want))
    share = ambiguous / float(n * T)
    print(f"{what}: {n * T} steps, ambiguous share {100 * share:.2f} %, picks outside the accepted set {len(bad)}, "
          f"max |logp - fp64| {worst_lp:.2e} (bound {eps:.2e})")
    assert not bad, bad[:8]
    assert share <= AMBIGUOUS_CAP, share
    if logp is not None:
        assert worst_lp <= eps, worst_lp
    return share


# ===================================================================================== CPU
def _reference_filter(logits, top_p):
    """reference gpt2_prefix_eval.py:166-175, literally (on fp64 logits [1, V]) -> the tokens left finite"""
    import torch.nn.functional as nnf
    filter_value = -float("Inf")
    logits = logits.clone()
    sorted_logits, sorted_indices = torch.sort(logits, descending=True)
    cumulative_probs = torch.cumsum(nnf.softmax(sorted_logits, dim=-1), dim=-1)
    sorted_indices_to_remove = cumulative_probs > top_p
    sorted_indices_to_remove[..., 1:] = sorted_indices_to_remove[..., :-1].clone()
    sorted_indices_to_remove[..., 0] = 0
    indices_to_remove = sorted_indices[sorted_indices_to_remove]
    logits[:, indices_to_remove] = filter_value
    return torch.isfinite(logits[0]).numpy()


@pytest.mark.parametrize("V", [1531, 50257])
@pytest.mark.parametrize("top_p", [0.0, 0.8, 1.0])
def test_definition_is_the_reference_filter(V, top_p):
    """the nucleus of sample_def == the tokens the reference's filter leaves finite (random logits, std 4; no ties).  The
    two may differ only on tokens whose mass-above lies within fp64 rounding (1e-12) of top_p: at top_p = 1 the reference's
    running sum can round above 1 over the last, ~1e-16 tokens, where the definition (A(j) < 1 always) keeps them."""
    g = torch.Generator().manual_seed(V + int(10 * top_p))
    for _ in range(4):
        logits = torch.randn(1, V, generator=g, dtype=torch.float64) * 4.0
        p = D.softmax(D.scaled(logits[0].numpy(), 1.0))
        mine = D.nucleus(p, top_p)
        ref = _reference_filter(logits, top_p)
        diff = np.nonzero(mine != ref)[0]
        assert np.all(np.abs(D.mass_above(p)[diff] - top_p) <= 1e-12), (len(diff), diff[:8])
        assert mine[int(np.argmax(p))] and ref[int(np.argmax(p))]
        if top_p <= 0:
            assert mine.sum() == 1
        if top_p < 1:
            assert len(diff) == 0


def test_definition_edges():
    """top_p <= 0 is the arg-max whatever u; top_p >= 1 is the inverse CDF of softmax; ties are treated alike; the last
    nucleus token when u is not exceeded"""
    logits = np.array([0.5, 2.0, -1.0, 2.0, 1.0])
    p = D.softmax(D.scaled(logits, 1.0))
    assert D.nucleus(p, 0.0).tolist() == [False, True, False, True, False]          # the tied arg-maxes, nothing else
    assert D.nucleus(p, 1.0).all()
    assert D.nucleus(p, 2 * p[1]).tolist() == [False, True, False, True, True]      # A(4) = 2 p[1] <= top_p
    for u in (0.0, 0.3, 0.999):
        assert D.sample(np.array([0.0, 3.0, 1.0]), 0.7, 0.0, u)[0] == 1
    c = np.cumsum(p)
    for u in (0.0, 0.2, 0.5, 0.77, 0.999):
        assert D.sample(logits, 1.0, 1.0, u)[0] == int(np.nonzero(c > u)[0][0])
    assert D.pick(p, D.nucleus(p, 0.0), 1.0) == 3
    tok, lp = D.sample(logits, 0.5, 1.0, 0.0)
    assert tok == 0 and abs(lp - math.log(D.softmax(logits / 0.5)[0])) < 1e-12


def test_header_binding_and_argument_checks():
    """the symbol is declared and bound, the ABI version is still 6, the shape of u is checked and a NaN top_p is refused
    before anything is launched (by the Python host and by the C entry point itself)"""
    from capdec_amd import _capi
    from capdec_amd.engine import Engine
    header = open(os.path.join(ROOT, "include", "capdec.h")).read()
    assert re.search(r"\bint\s+capdec_decode_sample\s*\(", header)
    assert re.search(r"#define\s+CAPDEC_ABI_VERSION\s+6\b", header) and _capi.ABI_VERSION == 6
    res, args = _capi.SIGNATURES["capdec_decode_sample"]
    assert res is C.c_int and len(args) == 14 and args[7] is C.c_float and args[8] is C.c_float and args[9] is C.c_uint64
    lib = _capi.load_library()
    assert lib.capdec_abi_version() == 6 and hasattr(lib, "capdec_decode_sample")
    rc = lib.capdec_decode_sample(None, None, 0, 10, 13, 764, 12, 1.0, float("nan"), 0, None, None, None, None)
    assert rc != 0 and b"NaN" in lib.capdec_last_error()
    e = Engine.__new__(Engine)                     # no context: both checks come before the first use of one
    pe = torch.zeros(3, 10, 768)
    with pytest.raises(_capi.CapdecError, match="NaN"):
        Engine.decode_sample(e, pe, 13, 12, top_p=float("nan"))
    with pytest.raises(_capi.CapdecError, match="NaN"):
        Engine.decode_sample(e, pe, 13, 12, temperature=float("nan"))
    with pytest.raises(_capi.CapdecError, match="entry_length"):
        Engine.decode_sample(e, pe, 13, 12, u=torch.zeros(3, 11))
    with pytest.raises(_capi.CapdecError, match="entry_length"):
        Engine.decode_sample(e, pe, 13, 12, u=torch.zeros(12))


@pytest.mark.parametrize("geom,temperature,top_p", CASES_ALL)
def test_ambiguity_cap_oracle_alone(geom, temperature, top_p):
    """the acceptance set of the GPU test is narrow: along the oracle's own sampled trajectory (64 captions x 12 steps,
    eps = 2 delta / temperature) at most 3 % of the steps accept more than one token.  Measured shares (oracle alone, all
    768 steps): tiny 1.0 / 0.8: 0.78 %; tiny 0.7 / 0.8: 0.13 %; tiny 0.7 / 0.95: 1.82 %; small 0.7 / 0.8: 1.30 %;
    bigvocab 0.7 / 0.8: 0.39 % (with 32 captions, 384 steps, the first four: 0.52 %, 0.26 %, 2.34 %, 1.04 %)."""
    dims, sd, prefix, u = _case(geom)
    ids, logits = D.decode(sd, prefix, temperature, top_p, u.numpy(), dims.n_head)
    assert ids.min() >= 0 and ids.max() < dims.vocab
    _check_steps(logits, ids, u.numpy(), temperature, top_p, what=f"oracle {geom} t={temperature} top_p={top_p}")


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


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["tiny", "small"])
def test_top_p_zero_is_greedy_and_the_reference(golden, geom):
    """top_p = 0 keeps the arg-max only: whatever the temperature and the uniforms, ids and lens are those of
    decode_greedy_ids and of the reference's generate2 (tests/golden/decode_*.npz), at T 12 and T 67"""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    g, dims = golden("decode_" + geom), DIMS[geom]
    model = ClipCaptionModel(10, prefix_dim=640, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0").eval()
    sd = synth.hot_state_dict(42, "mlp", 640, 10, dims=dims)
    assert synth.state_dict_checksum(sd) == int(g["greedy_sd_crc"]), "RNG drift"
    model.load_state_dict(sd)
    pe, stop = torch.from_numpy(g["greedy_prefix_embed"]), int(g["greedy_stop_id"])
    for el in (12, 67):
        gi, gl = E.decode_greedy_ids(model, pe, stop, el)
        for k, (temperature, top_p) in enumerate([(1.0, 0.0), (0.7, 0.0), (1.3, -1.0)]):
            u = torch.rand(pe.shape[0], el, generator=torch.Generator().manual_seed(el + k))
            for kw in (dict(u=u), dict(seed=5 + k)):
                ids, lens = E.sample_ids(model, pe, stop, el, top_p=top_p, temperature=temperature, **kw)
                np.testing.assert_array_equal(ids.cpu().numpy(), gi.cpu().numpy())
                np.testing.assert_array_equal(lens.cpu().numpy(), gl.cpu().numpy())
                np.testing.assert_array_equal(ids.cpu().numpy(), g[f"greedy_ids_T{el}"])
                np.testing.assert_array_equal(lens.cpu().numpy(), g[f"greedy_lens_T{el}"])


@pytest.mark.gpu
@pytest.mark.parametrize("geom,temperature,top_p", CASES_ALL)
def test_injected_uniforms_vs_definition(eng, geom, temperature, top_p):
    """fixed uniforms, nothing stops: every token the HIP path drew lies in its step's accepted set (fp64 definition on the
    oracle's logits along the HIP trajectory), at most 3 % of the steps are ambiguous, logp within 2 delta / temperature.
    Ambiguous shares re-measured on the CPU with this eps over all 768 steps of a case (the oracle's own trajectory, same
    prefixes and uniforms): tiny 1.0 / 0.8: 0.78 %; tiny 0.7 / 0.8: 0.13 %; tiny 0.7 / 0.95: 1.82 %; small 0.7 / 0.8:
    1.30 %; bigvocab (V 51 300, the kernel variant that re-reads the row) 0.7 / 0.8: 0.39 %.  The share along the HIP
    trajectory is printed by the test before it is asserted; it differs from these only where the two trajectories part."""
    dims, sd, prefix, u = _case(geom)
    eng.load_gpt2(sd, n_head=dims.n_head)
    ids, lens, logp = eng.decode_sample(prefix, dims.vocab + 5, T12, temperature, top_p, u=u, alt_stop_id=-1,
                                        return_logp=True)
    ids, lens, logp = ids.cpu().numpy(), lens.cpu().numpy(), logp.cpu().numpy()
    assert (lens == T12).all() and ids.min() >= 0 and ids.max() < dims.vocab
    logits = _oracle_logits(sd, prefix, ids, dims.n_head)
    _check_steps(logits, ids, u.numpy(), temperature, top_p, logp, what=f"hip {geom} t={temperature} top_p={top_p}")


@pytest.mark.gpu
def test_vocabulary_above_register_budget_top_p_zero_is_greedy(eng):
    """V 51 300 (the kernel variant that re-reads the row): at top_p 0 and at a top_p below every arg-max's probability the
    ids are decode_greedy's at any temperature -- the arg-max is exactly exp(0) in every pass of the kernel, so the row
    always has a token to write"""
    dims, sd, prefix, u = _case("bigvocab", 16)
    eng.load_gpt2(sd, n_head=dims.n_head)
    gi, gl = [t.cpu().numpy() for t in eng.decode_greedy(prefix, dims.vocab + 5, T12, -1)]
    assert (gl == T12).all()
    for temperature, top_p in [(1.0, 0.0), (0.7, 0.0), (1.3, 1e-6), (0.37, 1e-6)]:
        for kw in (dict(u=u), dict(seed=3)):
            ids, lens = [t.cpu().numpy() for t in eng.decode_sample(prefix, dims.vocab + 5, T12, temperature, top_p,
                                                                    alt_stop_id=-1, **kw)]
            np.testing.assert_array_equal(ids, gi)
            np.testing.assert_array_equal(lens, gl)


@pytest.mark.gpu
def test_benchmark_size_vs_definition(eng):
    """5000 captions, GPT-2-small geometry, T 67, temperature 0.7, top_p 0.8, injected uniforms (the step's logits are
    materialised in row blocks): the synthetic weights never stop, so every caption has 67 tokens; 32 captions spread over
    the batch are checked step by step like test_injected_uniforms_vs_definition"""
    n, T, temperature, top_p = 5000, 67, 0.7, 0.8
    dims, sd, prefix, u = _case("small", n, T, seed=3)
    eng.load_gpt2(sd, n_head=dims.n_head)
    ids, lens, logp = eng.decode_sample(prefix, dims.vocab + 5, T, temperature, top_p, u=u, alt_stop_id=-1, return_logp=True)
    ids, lens, logp = ids.cpu().numpy(), lens.cpu().numpy(), logp.cpu().numpy()
    assert (lens == T).all() and ids.min() >= 0 and ids.max() < dims.vocab
    pick = np.linspace(0, n - 1, 32).astype(np.int64)
    logits = _oracle_logits(sd, prefix[pick], ids[pick], dims.n_head)
    _check_steps(logits, ids[pick], u.numpy()[pick], temperature, top_p, logp[pick], what="hip small 5000 x 67")


def _stop_case(n=48, seed=0):
    """tiny geometry whose captions stop: a constant on the stop token's logit (synth.with_stop_bias, alpha 10: the stop
    token carries ~16 % of a step's probability on average)"""
    from oracle import capdec_oracle as O
    dims = synth.GPT2_TINY
    sd = synth.with_stop_bias(synth.hot_state_dict(42, "mlp", 512, P, dims=dims), 13, 10.0)
    x = synth.synthetic_clip_embeddings(n, 512, seed=seed)
    return dims, sd, O.clip_project(x, sd, "mlp", P).reshape(n, P, -1)


def _check_stop_structure(ids, lens, T, stops):
    for r in range(ids.shape[0]):
        L = int(lens[r])
        assert 1 <= L <= T
        assert not np.isin(ids[r, :L - 1], stops).any(), (r, ids[r])
        assert L == T or ids[r, L - 1] in stops, (r, ids[r])
        assert (ids[r, L:] == 0).all(), (r, ids[r])


@pytest.mark.gpu
def test_philox_seed_chunking_compaction(eng):
    """device Philox keyed by (seed, caption index, step): the same seed repeats, another seed differs; in batch-invariant
    mode a caption's tokens do not depend on finished-caption compaction nor on the KV budget's chunking (three or more
    chunks).  The API has no caption-index offset, so "caption i alone" is covered through chunking only: a chunk's
    captions run without the others and keep their index within the call."""
    from capdec_amd import _capi
    dims, sd, prefix = _stop_case()
    n, T = prefix.shape[0], 16
    eng.load_gpt2(sd, n_head=dims.n_head)
    eng.set_batch_invariant(True)
    try:
        run = lambda seed: [t.cpu().numpy() for t in eng.decode_sample(prefix, 13, T, 1.0, 0.9, seed=seed, return_logp=True)]
        ids, lens, logp = run(7)
        _check_stop_structure(ids, lens, T, [13, 764])
        assert lens.min() < T and len(set(lens.tolist())) > 3              # captions do stop, at different steps
        assert eng.decode_stats()["compactions"] >= 1
        for a, b in zip(run(7), (ids, lens, logp)):
            np.testing.assert_array_equal(a, b)
        ids8, lens8, _ = run(8)
        assert (ids8 != ids).any()
        eng.set_compact(False)
        for a, b in zip(run(7), (ids, lens, logp)):
            np.testing.assert_array_equal(a, b)
        assert eng.decode_stats()["compactions"] == 0
        eng.set_compact(True)
        per_cap = (P + T - 1) * dims.n_embd * 2 * 4 * dims.n_layer          # fp32 K and V of one caption
        assert eng.decode_chunks() == 1
        _capi.check(eng.lib.capdec_set_kv_budget(eng._h, per_cap * 13), "budget")       # 48 captions -> chunks of 13
        for a, b in zip(run(7), (ids, lens, logp)):
            np.testing.assert_array_equal(a, b)
        assert eng.decode_chunks() == 4                                                 # 13 + 13 + 13 + 9
    finally:
        _capi.check(eng.lib.capdec_set_kv_budget(eng._h, 192 << 30), "budget")
        eng.set_compact(True)
        eng.set_batch_invariant(False)


@pytest.mark.gpu
def test_philox_distribution(eng):
    """one prefix replicated over 20 000 rows, one step: Pearson's chi-square of the drawn tokens against the fp64 q
    (top_p 1, temperature 1; tokens with an expected count below 5 lumped; bound: the 1 - 1e-6 quantile at the resulting
    degrees of freedom), and at top_p 0.8 no token outside the nucleus (of top_p + eps: the logits bar)"""
    from oracle import capdec_oracle as O
    n = 20000
    dims, sd, prefix, _ = _case("tiny", 1)
    eng.load_gpt2(sd, n_head=dims.n_head)
    p = D.softmax(D.scaled(O.gpt2_logits(prefix, sd, dims.n_head)[0, -1].numpy(), 1.0))
    rep = prefix.expand(n, -1, -1).contiguous()
    ids, lens = eng.decode_sample(rep, dims.vocab + 5, 1, 1.0, 1.0, seed=2024, alt_stop_id=-1)
    ids = ids.cpu().numpy()[:, 0]
    assert (lens.cpu().numpy() == 1).all()
    counts = np.bincount(ids, minlength=dims.vocab).astype(np.float64)
    expect = n * p
    big = expect >= 5.0
    obs = np.append(counts[big], counts[~big].sum())
    exp = np.append(expect[big], expect[~big].sum())
    assert exp[-1] >= 5.0
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    bound = D.chi2_upper_quantile(len(exp) - 1, 1e-6)
    print(f"chi-square {chi2:.1f} at {len(exp) - 1} degrees of freedom (bound {bound:.1f}); distinct tokens {int((counts > 0).sum())}")
    assert chi2 <= bound
    ids8, _ = eng.decode_sample(rep, dims.vocab + 5, 1, 1.0, 0.8, seed=2025, alt_stop_id=-1)
    inside = D.nucleus(p, 0.8 + _eps(1.0))
    drawn = np.unique(ids8.cpu().numpy())
    assert inside[drawn].all(), drawn[~inside[drawn]]
    assert len(drawn) > 1


@pytest.mark.gpu
def test_stopping_and_generate_samples(eng):
    """captions that stop: lens include the stop token, ids are zero after it, alt_stop_id stops a row exactly where the
    token appears (and nowhere else); generate_samples_batch returns entry_count texts per caption decoded from exactly
    ids[:len], each repeat with draws of its own"""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    dims, sd, prefix = _stop_case()
    n, T = prefix.shape[0], 16
    eng.load_gpt2(sd, n_head=dims.n_head)
    eng.set_batch_invariant(True)       # (a row's logits must not depend on when the others leave the batch)
    try:
        ids, lens = [t.cpu().numpy() for t in eng.decode_sample(prefix, 13, T, 1.0, 0.9, seed=11, alt_stop_id=-1)]
        _check_stop_structure(ids, lens, T, [13])
        assert lens.min() < T < lens.sum()
        # the most frequent token that is not the stop token becomes the second stop id
        body = np.concatenate([ids[r, :lens[r]] for r in range(n)])
        alt = int(np.bincount(body[body != 13]).argmax())
        ids2, lens2 = [t.cpu().numpy() for t in eng.decode_sample(prefix, 13, T, 1.0, 0.9, seed=11, alt_stop_id=alt)]
        _check_stop_structure(ids2, lens2, T, [13, alt])
        cut = 0
        for r in range(n):
            hit = np.nonzero(ids[r, :lens[r]] == alt)[0]
            L = int(hit[0]) + 1 if len(hit) else int(lens[r])
            cut += len(hit) > 0 and L < lens[r]
            assert lens2[r] == L and (ids2[r, :L] == ids[r, :L]).all(), r
        assert cut >= 1
    finally:
        eng.set_batch_invariant(False)

    class Tok:
        def encode(self, s):
            return [13]

        def decode(self, toks):
            return " ".join(str(int(t)) for t in toks)

    model = ClipCaptionModel(P, prefix_dim=512, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0").eval()
    model.load_state_dict(sd)
    texts = E.generate_samples_batch(model, Tok(), prefix, entry_count=3, entry_length=T, top_p=0.9, temperature=1.0, seed=21)
    ids3, lens3 = [t.cpu().numpy() for t in E.sample_ids(model, prefix.repeat_interleave(3, dim=0), 13, T, 0.9, 1.0, seed=21)]
    _check_stop_structure(ids3, lens3, T, [13, E.ALT_STOP_ID])
    assert len(texts) == n and all(len(t) == 3 for t in texts)
    for r in range(n):
        for e in range(3):
            assert texts[r][e] == " ".join(str(int(t)) for t in ids3[3 * r + e, :lens3[3 * r + e]])
    assert sum(len(set(t)) >= 2 for t in texts) > n // 2
    one = E.generate_samples(model, Tok(), embed=prefix[5:6], entry_count=3, entry_length=T, top_p=0.9, seed=21)
    assert isinstance(one, list) and len(one) == 3 and all(isinstance(t, str) for t in one)
    # seed=None: the key is a function of torch's global seed and of the number of keys the process has drawn so far
    from capdec_amd import train as TR
    torch.manual_seed(99)
    drawn = TR._seed_counter[0]
    a = E.generate_samples(model, Tok(), embed=prefix[5:6], entry_count=4, entry_length=T)
    b = E.generate_samples(model, Tok(), embed=prefix[5:6], entry_count=4, entry_length=T)
    assert TR._seed_counter[0] == drawn + 2 and len(a) == 4 and b != a      # a fresh key per call
    torch.manual_seed(99)
    TR._seed_counter[0] = drawn
    assert E.generate_samples(model, Tok(), embed=prefix[5:6], entry_count=4, entry_length=T) == a      # the same key again
    torch.manual_seed(100)
    TR._seed_counter[0] = drawn
    assert E.generate_samples(model, Tok(), embed=prefix[5:6], entry_count=4, entry_length=T) != a      # torch's seed counts


@pytest.mark.gpu
def test_errors_leave_the_context_usable(golden):
    """a refused sampling call (NaN top_p straight into the C ABI; a context beyond n_positions) reports through
    capdec_last_error and the next greedy decode still matches its fixture"""
    from capdec_amd import _capi
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    g, dims = golden("decode_tiny"), synth.GPT2_TINY
    model = ClipCaptionModel(10, prefix_dim=640, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0").eval()
    model.load_state_dict(synth.hot_state_dict(42, "mlp", 640, 10, dims=dims))
    pe, stop = torch.from_numpy(g["greedy_prefix_embed"]), int(g["greedy_stop_id"])
    e = model.engine
    p = pe.to("cuda:0").contiguous()
    ids = torch.empty(8, 12, device="cuda:0", dtype=torch.int32)
    lens = torch.empty(8, device="cuda:0", dtype=torch.int32)
    rc = e.lib.capdec_decode_sample(e._h, p.data_ptr(), 8, 10, stop, 764, 12, 1.0, float("nan"), 0, None, ids.data_ptr(),
                                    lens.data_ptr(), None)
    assert rc != 0 and b"NaN" in e.lib.capdec_last_error()
    with pytest.raises(_capi.CapdecError, match="n_positions"):
        e.decode_sample(pe, stop, entry_length=dims.n_pos, top_p=0.8)
    with pytest.raises(_capi.CapdecError):
        e.decode_sample(pe, stop, 12, u=torch.zeros(8, 13))
    gi, gl = E.decode_greedy_ids(model, pe, stop, 12)
    np.testing.assert_array_equal(gi.cpu().numpy(), g["greedy_ids_T12"])
    np.testing.assert_array_equal(gl.cpu().numpy(), g["greedy_lens_T12"])
    si, sl = e.decode_sample(pe, stop, 12, top_p=0.8, seed=1)
    _check_stop_structure(si.cpu().numpy(), sl.cpu().numpy(), 12, [stop, 764])
