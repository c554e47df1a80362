"""The sparse route of the fused lm_head (decode.hip: lm_head_sparse): the first pass keeps no candidates per (row, 128-column
tile); per row, the tiles whose maximum reaches the row's fifth largest tile maximum are computed again with the k = 5
epilogue by a launch grouped by tile, and merged.  It must give the k = 5 result bit for bit -- compared here with the
three-candidate route (CAPDEC_LMHEAD_SPARSE=0) and the five-per-tile route (CAPDEC_LMHEAD_K3=0), on random weights, on
weights whose vocabulary tiles repeat (exact ties: the cap on pairs per row, the full second pass, column order inside the
merge), at the row threshold of the wide tile and on a vocabulary that is a whole number of tiles.  The route is the
default from 12288 rows (LM_SPARSE_MIN_ROWS, common.h); the tests run a few thousand rows, so they select it with
CAPDEC_LMHEAD_SPARSE=2, which takes it from the first row of the wide tile, and compare the default as well."""
import numpy as np
import pytest

from capdec_amd import synth
from test_hip_parity import _beam_rows_vs_oracle, _report

CAP = 8                      # LM_SPARSE_CAP (common.h)
DIMS = synth.GPT2Dims(n_layer=2, vocab=128 * 47 + 17, n_pos=128)      # 48 column tiles, the last one 17 columns wide
ROUTES = {"sparse": {"CAPDEC_LMHEAD_SPARSE": "2"}, "default": {}, "k3": {"CAPDEC_LMHEAD_SPARSE": "0"}, "k5": {"CAPDEC_LMHEAD_K3": "0"}}


def _beam(monkeypatch, env, sd, pe, stop, T):
    from capdec_amd.engine import Engine
    for k in ("CAPDEC_LMHEAD_SPARSE", "CAPDEC_LMHEAD_K3"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = Engine(0)
    e.load_gpt2(sd)
    out = tuple(t.cpu().numpy() for t in e.decode_beam(pe, stop, 5, T))
    second, rs = e.second_pass_rows(), e.decode_stats()["row_steps"]
    e.close()
    return out, second, rs


def _inputs(dims, n, repeat_tiles=0, seed=7):
    from oracle import capdec_oracle as O
    sd = synth.hot_state_dict(seed, "mlp", 512, 10, dims=dims)
    if repeat_tiles:         # tiles 1 .. repeat_tiles of the vocabulary repeat tile 0: identical logits in every row (tied lm_head: one tensor)
        w = sd["gpt.transformer.wte.weight"]
        for j in range(1, repeat_tiles + 1):
            w[128 * j:128 * j + 128] = w[0:128]
    x = synth.synthetic_clip_embeddings(n, 512, seed=77)
    return sd, O.clip_project(x, sd, "mlp", 10).reshape(n, 10, -1)


def _same(a, b, what):
    for x, y, name in zip(a, b, ("ids", "lens", "scores", "order")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {name}")


@pytest.mark.gpu
def test_routes_agree_bit_for_bit(monkeypatch):
    """440 captions x beam 5 x T 10 (2200 rows: the wide tile from the second step on) on 48 tiles: ids, lengths, scores and
    order are equal under the sparse route, the default (3 per tile at this row count), CAPDEC_LMHEAD_SPARSE=0 and
    CAPDEC_LMHEAD_K3=0; the sparse route recomputes no row over all tiles unless tile maxima really tie (the count is
    reported); 10 captions go against the oracle."""
    n, T, stop = 440, 10, 13
    sd, pe = _inputs(DIMS, n)
    outs, second = {}, {}
    for name, env in ROUTES.items():
        outs[name], second[name], rs = _beam(monkeypatch, env, sd, pe, stop, T)
    _report(f"[lm_head sparse] V = {DIMS.vocab}: full second pass for {second['sparse']} of {rs} (row, step) pairs "
            f"(3 per tile: {second['k3']})")
    _same(outs["sparse"], outs["k3"], "sparse vs 3 per tile")
    _same(outs["sparse"], outs["k5"], "sparse vs 5 per tile")
    _same(outs["sparse"], outs["default"], "sparse vs default")
    assert second["k5"] == 0
    assert second["default"] == second["k3"]   # 2200 rows: below LM_SPARSE_MIN_ROWS the default is the 3-per-tile route
    assert second["sparse"] == 0, second       # random fp32 tile maxima: an exact five-way tie does not happen
    rows = sorted(np.random.default_rng(3).choice(n, 10, replace=False).tolist())
    ok, ties = _beam_rows_vs_oracle(outs["sparse"], sd, pe, rows, stop, T, DIMS.n_head, f"sparse lm_head, V = {DIMS.vocab}")
    assert ok + ties == len(rows) and ok >= len(rows) - 1, (ok, ties)


@pytest.mark.gpu
@pytest.mark.parametrize("repeat_tiles", [9, 2, 40])
def test_tied_tiles(monkeypatch, repeat_tiles):
    """Ten equal vocabulary tiles: a row whose top 5 reach into them has more than CAP tiles at its fifth tile maximum and
    takes the full second pass (positive count).  Three equal tiles stay within CAP: equal values from different tiles meet
    in the sparse merge, which must keep them in ascending column order.  With 41 of the 48 tiles equal most rows take the
    full pass, more than one of its slices holds.  The HIP routes agree bit for bit either way (the oracle's order among
    exactly equal logits is not defined: not compared)."""
    n, T, stop = 440, 10, 13
    sd, pe = _inputs(DIMS, n, repeat_tiles=repeat_tiles)
    outs, second = {}, {}
    for name, env in ROUTES.items():
        outs[name], second[name], rs = _beam(monkeypatch, env, sd, pe, stop, T)
    _report(f"[lm_head sparse] {repeat_tiles + 1} equal tiles: full second pass for {second['sparse']} of {rs} (row, step) pairs")
    _same(outs["sparse"], outs["k3"], "sparse vs 3 per tile")
    _same(outs["sparse"], outs["k5"], "sparse vs 5 per tile")
    _same(outs["sparse"], outs["default"], "sparse vs default")
    if repeat_tiles + 1 > CAP:
        assert second["sparse"] > 0, second
    ids = outs["sparse"][0]
    assert (ids < 128 * (repeat_tiles + 1)).any()          # tokens of the repeated tiles are really chosen


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2048, 2049])
def test_row_threshold_and_whole_tiles(monkeypatch, n):
    """2048 / 2049 captions: the FIRST step selects over R = captions rows -- exactly the row count from which the lm_head takes
    the wide tile, and one past it (a partial last row tile of one row) -- the later ones over captions x 5; the vocabulary is
    a whole number of tiles (no partial column tile)."""
    dims = synth.GPT2Dims(n_layer=2, vocab=128 * 48, n_pos=128)
    T, stop = 3, 13
    sd, pe = _inputs(dims, n, seed=11)
    a, second, rs = _beam(monkeypatch, ROUTES["sparse"], sd, pe, stop, T)
    b, _, _ = _beam(monkeypatch, ROUTES["k5"], sd, pe, stop, T)
    _report(f"[lm_head sparse] {n} captions, V = {dims.vocab}: full second pass for {second} of {rs} (row, step) pairs")
    _same(a, b, f"sparse vs 5 per tile, {n} captions")


def test_selection_rule_covers_the_top5():
    """The rule the select kernel applies, in numpy: with T5 the fifth largest tile maximum of a row, the tiles whose maximum
    is >= T5 hold the row's top 5 under the tie rule (value descending, column ascending), and merging the per-tile top 5 of
    those tiles alone gives exactly that top 5.  1000 rows of 48 tiles x 128 columns; values on a coarse grid so that ties
    -- inside a tile, across tiles, and at T5 -- are everywhere; a third of the rows repeat whole tiles."""
    rng = np.random.default_rng(0)
    rows, nt, w = 1000, 48, 128
    x = np.round(rng.normal(size=(rows, nt * w)).astype(np.float32) * 4) / 4          # 0.25 grid: thousands of exact ties per row
    for r in range(0, rows, 3):
        for j in rng.choice(np.arange(1, nt), size=int(rng.integers(1, 10)), replace=False):
            x[r, j * w:(j + 1) * w] = x[r, :w]
    x[:, -(w - 17):] = -np.inf                                                       # a partial last tile
    cols = np.arange(nt * w)
    many = 0
    for r in range(rows):
        v = x[r]
        order = np.lexsort((cols, -v))                                               # value descending, then column ascending
        top = order[:5]
        m = v.reshape(nt, w).max(axis=1)
        t5 = np.sort(m)[-5]
        sel = np.flatnonzero(m >= t5)
        many += len(sel) > CAP
        assert np.isin(top // w, sel).all(), (r, top, sel)
        cand = np.concatenate([t * w + np.lexsort((np.arange(w), -v[t * w:(t + 1) * w]))[:5] for t in sel])
        merged = cand[np.lexsort((cand, -v[cand]))][:5]
        np.testing.assert_array_equal(merged, top)
    assert many > 50           # the construction does produce rows beyond the cap (the kernel sends those to the full pass)
