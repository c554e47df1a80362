"""The step loop of every decode driver against the host model of it: exact per-step rows, steps, compactions, row-steps.

Greedy, beam 5, sampling, guided greedy, guided beam 5 and contrastive search (top_k 4) all run the same loop: poll the alive
count when the schedule says so, compact when it pays, launch na * rows_per_caption rows.  ``loop_model`` of
tests/test_decode_sched.py is that loop on the host.  It is fed the alive counts that the call's OWN returned lengths imply
(a caption whose longest beam has length L is still generating at the poll in front of step i exactly when L > i), so
numerical ties cannot disturb the expectation: whatever the device decoded, its statistics must be the model's.

Tiny synthetic GPT-2 whose captions stop at staggered steps (synth.with_stop_bias).  The stop bias was chosen on the CPU
definitions of the drivers: alpha 10 spreads the greedy family's lengths over 1..12, the beam drivers -- a caption ends when
all five beams have -- need 14 (at 10 no guided beam caption ends within 12 tokens); at 18 the 1700-caption beam run falls
from 8500 rows to ~200 within 24 steps."""
import functools

import pytest

from capdec_amd import synth
from test_decode_sched import alive_from_lengths, loop_model

P, T, N, STOP = 10, 12, 16, 13
BIG_N, BIG_T, BIG_ALPHA = 1700, 24, 18.0

#: driver -> (first step, activation rows per caption, stop bias of the 16-caption case)
DRIVERS = {
    "greedy": (1, 1, 10.0),
    "beam5": (1, 5, 14.0),
    "sample": (1, 1, 10.0),
    "guided_greedy": (1, 2, 10.0),
    "guided_beam5": (1, 10, 14.0),
    "contrastive4": (0, 4, 10.0),
}


@functools.lru_cache(maxsize=None)
def _weights(alpha):
    dims = synth.GPT2_TINY
    return synth.with_stop_bias(synth.hot_state_dict(42, "mlp", 512, P, dims=dims), STOP, alpha)


@functools.lru_cache(maxsize=None)
def _prefix(n, alpha):
    from oracle import capdec_oracle as O
    x = synth.synthetic_clip_embeddings(n, 512, seed=0)
    return O.clip_project(x, _weights(alpha), "mlp", P).reshape(n, P, -1).contiguous()


@pytest.fixture(scope="module")
def eng():
    from capdec_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _decode(e, driver, prefix, T):
    """one call -> the captions' lengths (the longest beam's for the beam drivers) as a list"""
    if driver == "greedy":
        lens = e.decode_greedy(prefix, STOP, T)[1]
    elif driver == "beam5":
        lens = e.decode_beam(prefix, STOP, 5, T)[1].max(dim=1).values
    elif driver == "sample":
        lens = e.decode_sample(prefix, STOP, T, 1.0, 0.9, seed=7)[1]
    elif driver == "guided_greedy":
        lens = e.decode_guided(prefix, prefix.mean(dim=0, keepdim=True), 1.5, STOP, 1, T, 1.0, -1)[1]
    elif driver == "guided_beam5":
        lens = e.decode_guided(prefix, prefix.mean(dim=0, keepdim=True), 1.5, STOP, 5, T)[1].max(dim=1).values
    else:
        lens = e.decode_contrastive(prefix, 4, 0.6, STOP, -1, T)[1]
    return [int(v) for v in lens.cpu()]


def _expected(driver, chunks, T):
    """the model over the chunks of a call (lists of caption lengths): per-step rows add up step by step"""
    first, rpc, _ = DRIVERS[driver]
    rows, steps, compactions = [], 0, 0
    for lens in chunks:
        m = loop_model(len(lens), first, T, rpc, True, alive_from_lengths(lens, first, T))
        rows += [0] * (len(m.rows) - len(rows))
        for i, r in enumerate(m.rows):
            rows[i] += r
        steps, compactions = max(steps, m.steps), compactions + m.compactions
    return rows, dict(steps=steps, compactions=compactions, row_steps=sum(rows))


def _check(e, driver, prefix, T, chunk=None):
    lens = _decode(e, driver, prefix, T)
    rows, stats = e.decode_step_rows(), e.decode_stats()
    chunk = chunk or len(lens)
    want_rows, want_stats = _expected(driver, [lens[c0:c0 + chunk] for c0 in range(0, len(lens), chunk)], T)
    print(f"{driver}: {len(lens)} captions, lengths {sorted(lens)[:8]}..{max(lens)}, rows {rows}, {stats}")
    assert rows == want_rows, (rows, want_rows)
    assert stats == want_stats, (stats, want_stats)
    return lens, rows, stats


@pytest.mark.gpu
@pytest.mark.parametrize("driver", list(DRIVERS))
def test_step_rows_of_every_driver(eng, driver):
    """16 captions, T 12, one chunk, compaction on"""
    alpha = DRIVERS[driver][2]
    eng.load_gpt2(_weights(alpha), n_head=synth.GPT2_TINY.n_head)
    eng.set_compact(True)
    lens, rows, stats = _check(eng, driver, _prefix(N, alpha), T)
    assert eng.decode_chunks() == 1
    assert min(lens) < T and len(set(lens)) >= 3, lens          # captions do stop, at different steps


@pytest.mark.gpu
def test_every_tier_on_the_device(eng):
    """beam 5 over 1700 captions, T 24: the first step launches >= 8192 rows, the last < 512"""
    eng.load_gpt2(_weights(BIG_ALPHA), n_head=synth.GPT2_TINY.n_head)
    eng.set_compact(True)
    lens, rows, stats = _check(eng, "beam5", _prefix(BIG_N, BIG_ALPHA), BIG_T)
    assert eng.decode_chunks() == 1
    assert rows[0] >= 8192 and rows[-1] < 512, rows
    assert any(2048 <= r < 8192 for r in rows) and any(512 <= r < 2048 for r in rows), rows


@pytest.mark.gpu
def test_two_chunks_add_up(eng):
    """a KV budget that holds 8 of the 16 beam-5 captions: the statistics are the sum of the two chunks' models"""
    from capdec_amd import _capi
    dims, alpha = synth.GPT2_TINY, DRIVERS["beam5"][2]
    eng.load_gpt2(_weights(alpha), n_head=dims.n_head)
    eng.set_compact(True)
    per_cap = 5 * (P + T - 1) * dims.n_embd * 2 * 4 * dims.n_layer           # fp32 K and V of one caption's beams
    try:
        _capi.check(eng.lib.capdec_set_kv_budget(eng._h, per_cap * 8 + per_cap // 2), "budget")
        _check(eng, "beam5", _prefix(N, alpha), T, chunk=8)
        assert eng.decode_chunks() == 2
    finally:
        _capi.check(eng.lib.capdec_set_kv_budget(eng._h, 192 << 30), "budget")
