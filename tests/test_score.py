"""Scoring given captions (``capdec_score`` / ``Engine.score`` / ``score_ids`` / ``score_captions`` / ``train.token_nll``)
against the fp64 restatement of its contract in tests/score_def.py.

Bounds, from this project's own bars (test_train_step_forward_vs_reference_golden: 2e-4 on logits, 1e-4 on logsumexp, 1e-4
on the loss): a per-token logp is a logit minus a logsumexp, 2e-4 + 1e-4 = 3e-4 absolute (at temperature t both terms
scale by 1 / t < 2 in the cases here; the bound is kept at 3e-4 all the same); a mean NLL against the reference's recorded
loss: 1e-4.  Every test prints the maximum it measured.
"""
import ctypes as C
import functools
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import score_def as D                                     # noqa: E402
from capdec_amd import synth                              # noqa: E402

LOGP_TOL = 3e-4
NLL_TOL = 1e-4
P = 10
DIMS = {"tiny": synth.GPT2_TINY, "small": synth.GPT2_SMALL}


def _sd(geom="tiny"):
    return synth.hot_state_dict(42, "mlp", 512, P, dims=DIMS[geom])


def _prefix(sd, n, seed=0):
    from oracle import capdec_oracle as O
    return O.clip_project(synth.synthetic_clip_embeddings(n, 512, seed=seed), sd, "mlp", P).reshape(n, P, -1)


def _oracle_logits(sd, prefix, tokens, n_head):
    """the oracle's logits at the scored positions: [n, L, V], index i = position P-1+i of cat(prefix, wte(tokens[:, :-1]))"""
    from oracle import capdec_oracle as O
    V = sd["gpt.transformer.wte.weight"].shape[0]
    t = torch.as_tensor(np.asarray(tokens), dtype=torch.long)[:, :-1]
    t = torch.where((t < 0) | (t >= V), torch.zeros_like(t), t)         # (an id outside the vocabulary is never looked up)
    x = torch.cat((prefix, O.wte(t, sd)), dim=1)
    return O.gpt2_logits(x, sd, DIMS["tiny"].n_head if n_head is None else n_head)[:, prefix.shape[1] - 1:].numpy()


@functools.lru_cache(maxsize=None)
def _oracle_case():
    """tiny geometry, MLP-mapper prefixes, n 6, L 9, lens [9, 4, 7, 1, 0, 9].  Labels: id 0 as a real token, id V-1 (the
    padded last 128-column tile), and in every caption one label that is the oracle's arg-max at its position (logp near 0,
    not only the ~ -16 of random labels).  Past a caption's length the row holds arbitrary ids -- one of them outside the
    vocabulary: padding is never looked up and taints nothing."""
    dims = DIMS["tiny"]
    V = dims.vocab
    sd = _sd()
    lens = np.array([9, 4, 7, 1, 0, 9], dtype=np.int64)
    n, L = len(lens), 9
    prefix = _prefix(sd, n)
    tokens = torch.randint(1, V - 1, (n, L), generator=torch.Generator().manual_seed(77)).numpy().astype(np.int64)
    tokens[0, 2], tokens[5, 0] = 0, 0
    tokens[0, 5], tokens[2, 1] = V - 1, V - 1
    where = {0: 7, 1: 3, 2: 4, 3: 0, 5: 8}                  # caption -> the position whose label becomes the arg-max
    first = _oracle_logits(sd, prefix, tokens, dims.n_head)  # (the arg-max at i depends on tokens[:i] only)
    for r, i in where.items():
        tokens[r, i] = int(first[r, i].argmax())
    tokens[1, 6] = V + 7                                     # padding (len 4)
    logits = _oracle_logits(sd, prefix, tokens, dims.n_head)
    for r, i in where.items():
        assert int(logits[r, i].argmax()) == tokens[r, i]
    return dims, sd, prefix, tokens, lens, logits, where


def _report(what, got, want, tol):
    ok = np.isfinite(want)
    worst = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
    print(f"{what}: max |hip - fp64| {worst:.3e} (bound {tol:.1e})")
    return worst


# ===================================================================================== CPU
@pytest.mark.parametrize("geom", ["tiny", "small"])
def test_definition_gives_the_reference_train_loss(golden, geom):
    """score_def on the oracle's train-forward logits, labels != 0: -sum(logp) / count is the loss the reference recorded
    (train.py:349), within 1e-5 (measured: 9e-7 tiny, 3.2e-6 small).  Pins the checker; passes without the feature."""
    from oracle import capdec_oracle as O
    g, dims = golden(f"train_forward_{geom}"), DIMS[geom]
    sd = _sd(geom)
    assert synth.state_dict_checksum(sd) == int(g["sd_crc"]), "RNG drift"
    tokens, prefix = torch.from_numpy(g["tokens"]), torch.from_numpy(g["prefix"])
    logits = O.train_forward(sd, tokens, prefix, "mlp", P, n_head=dims.n_head)[:, P - 1:-1].numpy()
    logp, s, c, top1 = D.score(logits, g["tokens"], None, ignore_id=0)
    assert c.sum() == int((g["tokens"] != 0).sum()) and (logp[g["tokens"] == 0] == 0).all()
    diff = abs(D.mean_nll(s, c) - float(g["train_loss"]))
    print(f"score_def vs train_loss ({geom}): {diff:.2e}")
    assert diff < 1e-5
    real = g["mask"][:, P - 1:-1] > 0
    np.testing.assert_array_equal(top1[real], g["argmax"][:, P - 1:-1][real])


def test_definition_edges():
    """lens, ignore_id, ids outside the vocabulary, temperature"""
    logits = np.log(np.array([[[0.5, 0.25, 0.25], [0.1, 0.2, 0.7], [0.3, 0.3, 0.4]]]))
    logp, s, c, _ = D.score(logits, [[0, 2, 1]], [2])
    np.testing.assert_allclose(logp, [[np.log(0.5), np.log(0.7), 0.0]], atol=1e-12)
    assert c[0] == 2 and abs(s[0] - np.log(0.35)) < 1e-12
    logp, s, c, _ = D.score(logits, [[0, 2, 1]], None, ignore_id=0)
    assert logp[0, 0] == 0 and c[0] == 2
    logp, s, c, _ = D.score(logits, [[0, 5, 1]])              # 5 is outside: NaN as a label, and as the input of position 2
    assert np.isfinite(logp[0, 0]) and np.isnan(logp[0, 1]) and np.isnan(logp[0, 2]) and np.isnan(s[0]) and c[0] == 3
    logp, s, c, _ = D.score(logits, [[0, 1, 5]])              # the last label is nobody's input
    assert np.isfinite(logp[0, :2]).all() and np.isnan(logp[0, 2])
    logp, s, c, _ = D.score(logits, [[0, 2, 1]], [0])
    assert (logp == 0).all() and s[0] == 0 and c[0] == 0
    logp, _, _, _ = D.score(logits, [[0, 2, 1]], temperature=0.5)
    assert abs(logp[0, 0] - np.log(0.25 / (0.25 + 2 * 0.0625))) < 1e-12


def test_abi_surface():
    """include/capdec.h declares capdec_score and capdec_score_chunks, _capi binds both with matching argument counts, the
    ABI version is still 6.  Fails without the feature."""
    from capdec_amd import _capi
    header = open(os.path.join(ROOT, "include", "capdec.h")).read()
    assert re.search(r"#define\s+CAPDEC_ABI_VERSION\s+6\b", header) and _capi.ABI_VERSION == 6
    bare = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name in ("capdec_score", "capdec_score_chunks"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", bare, flags=re.S)
        assert m, name
        res, args = _capi.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(m.group(1).split(",")), (name, args)
    args = _capi.SIGNATURES["capdec_score"][1]
    assert len(args) == 13 and args[8] is C.c_float and args[3] is _capi.c_int_p
    lib = _capi.load_library()
    assert lib.capdec_abi_version() == 6 and hasattr(lib, "capdec_score") and hasattr(lib, "capdec_score_chunks")
    from capdec_amd.engine import Engine
    e = Engine.__new__(Engine)                     # no context: the checks come before the first use of one
    with pytest.raises(_capi.CapdecError, match="NaN"):
        Engine.score(e, torch.zeros(2, 10, 768), torch.zeros(2, 4, dtype=torch.int32), temperature=float("nan"))
    with pytest.raises(_capi.CapdecError, match="tokens"):
        Engine.score(e, torch.zeros(2, 10, 768), torch.zeros(3, 4, dtype=torch.int32))
    config = open(os.path.join(ROOT, "capdec_amd", "csrc", "config.h")).read()
    assert "CAPDEC_SCORE_ROWS" in config


def test_score_captions_host_logic():
    """K texts per row repeat the prefix row K times (row-major: row r, candidate e -> r * K + e), lens come from the
    tokenizer, the result has the shape of `texts`; a ragged list is refused"""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd._capi import CapdecError

    class Tok:
        def encode(self, s):
            return [int(w) for w in s.split()]

    calls = []

    class StubEngine:
        def score(self, embed, tokens, lens, ignore_id, temperature, return_top1):
            calls.append((embed.clone(), tokens.clone(), list(lens), ignore_id, temperature, return_top1))
            n = tokens.shape[0]
            lens_t = torch.tensor(lens)
            s = torch.stack([-tokens[r, :lens[r]].float().sum() for r in range(n)])
            return torch.zeros(tokens.shape), s, lens_t.to(torch.int32)

    model = SimpleNamespace(engine=StubEngine())
    embed = torch.arange(3, dtype=torch.float32)[:, None, None].expand(3, 2, 4).contiguous()
    texts = [["5 6 7", "1"], ["2 2", "9 9 9 9"], ["3", "4 4"]]
    out = E.score_captions(model, Tok(), embed, texts, temperature=0.7)
    emb, tok, lens, ign, temp, top1 = calls[-1]
    assert emb.shape == (6, 2, 4) and emb[:, 0, 0].tolist() == [0, 0, 1, 1, 2, 2]
    assert lens == [3, 1, 2, 4, 1, 2] and tok.shape == (6, 4) and tok.dtype == torch.int32
    assert tok[3].tolist() == [9, 9, 9, 9] and tok[1].tolist() == [1, 0, 0, 0]
    assert ign == -1 and temp == 0.7 and top1 is False
    assert out == [[(-18.0, 3), (-1.0, 1)], [(-4.0, 2), (-36.0, 4)], [(-3.0, 1), (-8.0, 2)]]
    flat = E.score_captions(model, Tok(), embed, ["5 6", "1", "2 2 2"])
    assert calls[-1][0].shape == (3, 2, 4) and calls[-1][2] == [2, 1, 3]
    assert flat == [(-11.0, 2), (-1.0, 1), (-6.0, 3)]
    with pytest.raises(CapdecError):
        E.score_captions(model, Tok(), embed, [["1", "2"], ["3"], ["4", "5"]])
    with pytest.raises(CapdecError):
        E.score_captions(model, Tok(), embed, ["1", ["2"], "3"])
    with pytest.raises(CapdecError):
        E.score_captions(model, Tok(), embed, ["1", "2"])


# ===================================================================================== GPU
@pytest.fixture(scope="module")
def eng():
    from capdec_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _check_against(what, got, want, tol=LOGP_TOL):
    """got / want = (logp, sum, count[, top1]): logp within tol (NaN where the definition is NaN), exactly 0 where the
    definition is exactly 0 by rule, count exact, sum within tol x count -> the measured maximum"""
    logp, s, c = got[:3]
    wlogp, ws, wc = want[:3]
    np.testing.assert_array_equal(np.isnan(logp), np.isnan(wlogp))
    worst = _report(what, logp, wlogp, tol)
    assert worst <= tol
    np.testing.assert_array_equal(c, wc)
    np.testing.assert_array_equal(np.isnan(s), np.isnan(ws))
    ok = np.isfinite(ws)
    assert (np.abs(s[ok] - ws[ok]) <= tol * np.maximum(wc[ok], 1)).all(), (s, ws)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("temperature,ignore_id", [(1.0, -1), (0.7, -1), (1.0, 0)])
def test_score_vs_oracle(eng, temperature, ignore_id):
    """n 6, L 9, lens [9, 4, 7, 1, 0, 9] (see _oracle_case): logp within 3e-4 of score_def on the oracle's logits, exactly 0
    past len (and at ignored labels), count exact, sum within 3e-4 x count, top1 the oracle's arg-max where its margin is
    clear.  Measured max |logp - fp64|: see DESIGN.md "Scoring"."""
    dims, sd, prefix, tokens, lens, logits, where = _oracle_case()
    eng.load_gpt2(sd, n_head=dims.n_head)
    want = D.score(logits, tokens, lens, ignore_id, temperature)
    got = _np(eng.score(prefix, torch.from_numpy(tokens), lens, ignore_id, temperature, return_top1=True))
    _check_against(f"score t={temperature} ignore={ignore_id}", got, want)
    logp, top1 = got[0], got[3]
    L = tokens.shape[1]
    past = np.arange(L)[None, :] >= lens[:, None]
    assert (logp[past] == 0).all() and (top1[past] == 0).all()
    if ignore_id == 0:
        assert logp[0, 2] == 0 and logp[5, 0] == 0 and got[2].tolist() == [8, 4, 7, 1, 0, 8]
    else:
        for r, i in where.items():
            assert logp[r, i] > -3.0 / temperature, (r, i, logp[r, i])       # the arg-max label: nowhere near the ~ -16
    top2 = np.sort(logits, -1)[..., -2:]
    clear = ((top2[..., 1] - top2[..., 0]) > 1e-3) & ~past
    np.testing.assert_array_equal(top1[clear], want[3][clear])
    assert eng.score_chunks() == 1


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["tiny", "small"])
def test_reference_train_loss_and_argmax(golden, geom):
    """the train_forward fixtures (the reference's own numbers), lens = L, ignore_id = 0: -sum(sum) / sum(count) within 1e-4
    of train_loss; top1 equals the fixture's arg-max at every real position"""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    g, dims = golden(f"train_forward_{geom}"), DIMS[geom]
    sd = _sd(geom)
    assert synth.state_dict_checksum(sd) == int(g["sd_crc"]), "RNG drift"
    model = ClipCaptionModel(P, prefix_dim=512, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0").eval()
    model.load_state_dict(sd)
    tokens = torch.from_numpy(g["tokens"])
    embed = model.clip_project(torch.from_numpy(g["prefix"])).view(-1, P, dims.n_embd)
    logp, s, c, top1 = _np(E.score_ids(model, embed, tokens, None, ignore_id=0, return_top1=True))
    assert int(c.sum()) == int((g["tokens"] != 0).sum())
    nll = -float(s.astype(np.float64).sum()) / float(c.sum())
    print(f"score vs reference train_loss ({geom}): {abs(nll - float(g['train_loss'])):.3e} (bound {NLL_TOL:.0e})")
    assert abs(nll - float(g["train_loss"])) <= NLL_TOL
    real = g["mask"][:, P - 1:-1] > 0
    np.testing.assert_array_equal(top1[real], g["argmax"][:, P - 1:-1][real])


CHUNK_LENS = [1, 3, 9, 2, 5, 7, 9]


def _chunk_child():
    """(child process, CAPDEC_SCORE_ROWS=40 in its environment) 7 captions with lens 1..9 at P 10: >= 3 chunks, within
    3e-4 of the oracle, input order kept; batch-invariant: bit-identical to the unchunked call of a second context"""
    from capdec_amd.engine import Engine
    dims, sd = DIMS["tiny"], _sd()
    lens = np.array(CHUNK_LENS)
    n, L = len(lens), 9
    prefix = _prefix(sd, n, seed=5)
    tokens = torch.randint(0, dims.vocab, (n, L), generator=torch.Generator().manual_seed(5)).numpy().astype(np.int64)
    want = D.score(_oracle_logits(sd, prefix, tokens, dims.n_head), tokens, lens)
    assert os.environ.get("CAPDEC_SCORE_ROWS") == "40"
    small = Engine(0)
    del os.environ["CAPDEC_SCORE_ROWS"]
    whole = Engine(0)                                # (the knobs are read once, when a context is created)
    for e in (small, whole):
        e.load_gpt2(sd, n_head=dims.n_head)
    run = lambda e: _np(e.score(prefix, torch.from_numpy(tokens), lens, return_top1=True))
    got = run(small)
    chunks = small.score_chunks()
    print("chunks", chunks)
    assert chunks >= 3
    _check_against("chunked", got, want)
    got1 = run(whole)
    assert whole.score_chunks() == 1
    _check_against("unchunked", got1, want)
    for e in (small, whole):
        e.set_batch_invariant(True)
    a, b = run(small), run(whole)
    assert small.score_chunks() >= 3 and whole.score_chunks() == 1
    _check_against("chunked, batch-invariant", a, want)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.int32) if x.dtype == np.float32 else x,
                                      y.view(np.int32) if y.dtype == np.float32 else y)
    small.close()
    whole.close()
    print("chunk child ok")


@pytest.mark.gpu
def test_chunking_fresh_process():
    """a fresh process with CAPDEC_SCORE_ROWS=40 (see _chunk_child)"""
    env = dict(os.environ, CAPDEC_SCORE_ROWS="40")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--chunk-child"], env=env, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "chunk child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.gpu
def test_cross_path_greedy_forced(eng):
    """KV-cached decode against batched scoring: decode_greedy_forced on 8 captions, T 12 (four fed their own greedy ids,
    four random ids).  Wherever the step's top-1 / top-2 margin exceeds 1e-3, top1 equals its ids; where the forced token
    is the arg-max, logp is within 3e-4 of stats[..., 0] - stats[..., 2]"""
    dims, sd = DIMS["tiny"], _sd()
    n, T = 8, 12
    prefix = _prefix(sd, n, seed=2)
    eng.load_gpt2(sd, n_head=dims.n_head)
    greedy, _ = eng.decode_greedy(prefix, dims.vocab + 5, T, -1)
    forced = torch.randint(0, dims.vocab, (n, T), generator=torch.Generator().manual_seed(3)).to(torch.int32)
    forced[:4] = greedy[:4].cpu()
    ids, stats = _np(eng.decode_greedy_forced(prefix, forced))
    logp, s, c, top1 = _np(eng.score(prefix, forced, return_top1=True))
    clear = (stats[..., 0] - stats[..., 1]) > 1e-3
    assert clear.mean() > 0.9
    np.testing.assert_array_equal(top1[clear], ids[clear])
    hit = (forced.numpy() == ids) & clear
    assert hit.sum() >= 4 * T - 4                                 # (the four captions fed their own greedy ids)
    worst = _report("score vs decode_greedy_forced", logp[hit], (stats[..., 0] - stats[..., 2])[hit], LOGP_TOL)
    assert worst <= LOGP_TOL and (c == T).all()


@pytest.mark.gpu
def test_cross_path_beam(eng, golden):
    """decode_beam, beam 5, T 12, with the fixture's stop id (it ends some beams early): sum / lens of the scored beams is
    within 3e-4 of the returned scores, for all 5 beams"""
    dims, sd = DIMS["tiny"], _sd()              # (the fixture's GPT-2: the mapper has a generator stream of its own)
    g = golden("decode_tiny")
    prefix, stop, T = torch.from_numpy(g["beam_prefix_embed"]), int(g["beam_stop_id"]), 12
    eng.load_gpt2(sd, n_head=dims.n_head)
    ids, lens, scores, _ = _np(eng.decode_beam(prefix, stop, 5, T))
    n = prefix.shape[0]
    assert lens.min() < T and (lens >= 1).all()                   # some beams do stop early
    logp, s, c = _np(eng.score(prefix.repeat_interleave(5, dim=0), torch.from_numpy(ids.reshape(n * 5, T)), lens.reshape(-1)))
    np.testing.assert_array_equal(c, lens.reshape(-1))
    mean = s / lens.reshape(-1)
    worst = _report("score vs decode_beam", mean, scores.reshape(-1), LOGP_TOL)
    assert worst <= LOGP_TOL


@pytest.mark.gpu
def test_cross_path_sample(eng):
    """decode_sample(temperature 0.7, injected u, captions that stop): score(temperature 0.7) on its ids is within 3e-4 of
    the logp it reported, up to lens; both are 0 after"""
    dims = DIMS["tiny"]
    sd = synth.with_stop_bias(_sd(), 13, 10.0)
    n, T = 16, 12
    prefix = _prefix(sd, n, seed=4)
    u = torch.rand(n, T, generator=torch.Generator().manual_seed(9))
    eng.load_gpt2(sd, n_head=dims.n_head)
    ids, lens, slogp = eng.decode_sample(prefix, 13, T, 0.7, 0.9, u=u, alt_stop_id=-1, return_logp=True)
    logp, s, c = _np(eng.score(prefix, ids, lens.cpu(), temperature=0.7))
    lens, slogp = lens.cpu().numpy(), slogp.cpu().numpy()
    assert lens.min() < T
    np.testing.assert_array_equal(c, lens)
    worst = _report("score vs decode_sample", logp, slogp, LOGP_TOL)
    assert worst <= LOGP_TOL
    past = np.arange(T)[None, :] >= lens[:, None]
    assert (logp[past] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bf16x3", "f32", "bf16", "f16"])
def test_gemm_modes(monkeypatch, mode):
    """CAPDEC_GEMM_MODE bf16x3 / f32: test_score_vs_oracle's bound against the oracle.  bf16 / f16: against the same mode's
    materialised path -- capdec_gpt2_logits(all positions) then an fp64 log_softmax gather on the host, every caption at
    full length so both paths launch the block stack on the same rows; the operand rounding is the same on both sides
    (label_logit_kernel rounds like the mode's GEMM) and only the fp32 summation order differs: 3e-4 holds here too."""
    from capdec_amd.engine import Engine
    dims, sd, prefix, tokens, lens, logits, _ = _oracle_case()
    monkeypatch.setenv("CAPDEC_GEMM_MODE", mode)
    e = Engine(0)
    try:
        assert e.gemm_mode() == mode
        e.load_gpt2(sd, n_head=dims.n_head)
        if mode in ("bf16x3", "f32"):
            got = _np(e.score(prefix, torch.from_numpy(tokens), lens))
            _check_against(f"mode {mode} vs oracle", got, D.score(logits, tokens, lens))
        else:
            tok = tokens.copy()
            tok[1, 6] = 5                                     # every id a real one: all captions at full length
            t = torch.from_numpy(tok)
            embeds = torch.cat((prefix.to(e.device), e.wte(t[:, :-1])), dim=1)
            mat = e.gpt2_logits(embeds, all_positions=True)[:, P - 1:].cpu().numpy()
            got = _np(e.score(prefix, t, None))
            _check_against(f"mode {mode} vs its own materialised logits", got, D.score(mat, tok, None))
            far = float(np.abs(got[0] - D.score(_oracle_logits(sd, prefix, tok, dims.n_head), tok, None)[0]).max())
            print(f"mode {mode}: max |logp - fp32 oracle| {far:.3e} (the mode's own precision; not asserted)")
    finally:
        e.close()


@pytest.mark.gpu
def test_guards(eng):
    """an input id V + 3 in caption 2 of 4: that caption's logp is NaN from that position on and its sum is NaN, the other
    three stay within the bound; P + L - 1 > n_positions is refused with an error string and the context still scores"""
    from capdec_amd._capi import CapdecError
    dims, sd = DIMS["tiny"], _sd()
    n, L, bad_at = 4, 9, 3
    prefix = _prefix(sd, n, seed=6)
    tokens = torch.randint(0, dims.vocab, (n, L), generator=torch.Generator().manual_seed(6)).numpy().astype(np.int64)
    tokens[2, bad_at] = dims.vocab + 3
    want = D.score(_oracle_logits(sd, prefix, tokens, dims.n_head), tokens)
    assert np.isnan(want[0][2, bad_at:]).all() and np.isfinite(want[0][2, :bad_at]).all() and np.isnan(want[1][2])
    eng.load_gpt2(sd, n_head=dims.n_head)
    got = _np(eng.score(prefix, torch.from_numpy(tokens)))
    _check_against("guards", got, want)
    assert np.isnan(got[0][2, bad_at:]).all() and np.isnan(got[1][2]) and np.isfinite(got[1][[0, 1, 3]]).all()
    long = dims.n_pos - P + 2
    with pytest.raises(CapdecError, match="n_positions"):
        eng.score(prefix, torch.zeros(n, long, dtype=torch.int32))
    with pytest.raises(CapdecError, match="length"):
        eng.score(prefix, torch.from_numpy(tokens), [L + 1, 1, 1, 1])
    again = _np(eng.score(prefix, torch.from_numpy(tokens)))
    np.testing.assert_array_equal(np.isnan(again[0]), np.isnan(got[0]))
    _check_against("guards, after the refused calls", again, want)


@pytest.mark.gpu
def test_token_nll_is_validation_loss_on_one_batch(golden):
    """train.token_nll on a dataset that is one full batch equals validation_loss within 1e-4 (and the reference's loss)"""
    from capdec_amd import train as TR
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    g, dims = golden("train_forward_tiny"), DIMS["tiny"]
    model = ClipCaptionModel(P, prefix_dim=512, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0")
    model.load_state_dict(_sd())
    data = [(torch.from_numpy(g["tokens"][r]), torch.from_numpy(g["mask"][r]), torch.from_numpy(g["prefix"][r]))
            for r in range(3)]
    model.train()
    nll = TR.token_nll(model, data, 3)
    assert model.training
    val = TR.validation_loss(model, data, 3)
    print(f"token_nll {nll:.6f} validation_loss {val:.6f} reference {float(g['train_loss']):.6f}")
    assert abs(nll - val) <= NLL_TOL and abs(nll - float(g["train_loss"])) <= NLL_TOL
    assert abs(TR.token_nll(model, data, 2) - nll) <= 1e-6         # every item counts whatever the batching


if __name__ == "__main__":
    if "--chunk-child" in sys.argv:
        _chunk_child()
