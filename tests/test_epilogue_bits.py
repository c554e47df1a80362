"""What the GEMM epilogues and the decode-step LayerNorm write, bit for bit.

The epilogues of gemm_epilogue_lds.h were rewritten for less vector-ALU work per piece -- interior tiles without bounds
tests, a saturation count kept in a register, per-column work of the qkv scatter hoisted out of the passes -- under the
rule that no output bit changes.  ``tests/golden/epilogue_bits.npz`` holds what the commit BEFORE that change produced
(``python tools/epilogue_bits.py --write`` on an MI355X at that commit); these tests run the same cases on this tree:

* logits of 300 rows (a last row tile with 44 live rows), beam-5 decodes of 3300 captions (16 500-row steps) without and
  with captions that stop (the qkv scatter with a caption map after compaction): row digests / ids / lengths / scores equal;
* a model whose c_fc pre-activations in chosen columns are exactly +70 000, -70 000, +inf, 1e-5, 1e-40, -0.0 (and NaN):
  equal logits, and the saturated-quad count equal to the golden AND to what the values imply -- one count per saturated
  quad, so a quad counted zero times or twice fails;
* the f16x2 format itself, independent of any earlier commit: a numpy restatement of the definition in bf16x3.h, its
  properties on the CPU, and the GEMM of the packed-A path against the fp64 product of the operands the restatement
  reconstructs (1e-6 of sum |a||b|);
* rows [0, 300) of the 3300-caption decode against the same 300 captions decoded alone, batch-invariant mode: the
  large-row and the small-row LayerNorm launches give the same bits.
"""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import pytest
import torch

_spec = importlib.util.spec_from_file_location("epilogue_bits_tool", os.path.join(ROOT, "tools", "epilogue_bits.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(tool.GOLDEN)


@pytest.fixture(scope="module")
def logits_now():
    return tool.run_logits()


@pytest.fixture(scope="module")
def beams_now(golden):
    return tool.run_beams(float(golden["stop_alpha"]))[0]


def _same(got, ref, names):
    for k in names:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        if not np.array_equal(a, b):
            rows = np.nonzero((a != b).reshape(a.shape[0], -1).any(1))[0] if a.ndim else []
            raise AssertionError(f"{k}: {len(rows)} of {a.shape[0] if a.ndim else 1} rows differ, first {list(rows[:8])}")


# ------------------------------------------------------------------------------------------ goldens of the parent commit
@gpu
def test_logits_300_rows_bit_equal(golden, logits_now):
    """(a) gpt2_logits, 100 x 3 positions: every row's SHA-256 equals the golden's; nothing saturates"""
    assert golden["logits"].shape == (300, 32)
    _same(logits_now, golden, ["logits", "logits_saturated"])
    assert int(logits_now["logits_saturated"]) == 0


@gpu
def test_beam_16500_rows_bit_equal(golden, beams_now):
    """(b) beam 5, P 10, T 4 on 3300 captions: ids, lengths and scores"""
    assert golden["beam_ids"].shape == (tool.N_CAP, tool.BEAM, tool.T)
    _same(beams_now, golden, ["beam_ids", "beam_lens", "beam_scores"])


@gpu
def test_beam_with_caption_map_bit_equal(golden, beams_now):
    """(c) the same with a stop bias and compaction: the second step runs on about half the rows, so the qkv scatter
    writes through a caption map; the row counts of the steps are part of the comparison"""
    rows = golden["stop_rows"].tolist()
    assert rows[0] == tool.N_CAP * tool.BEAM and 0.35 * rows[0] < rows[1] < 0.65 * rows[0], rows
    assert int(golden["stop_compactions"]) >= 1
    _same(beams_now, golden, ["stop_ids", "stop_lens", "stop_scores", "stop_rows", "stop_compactions"])


@gpu
def test_special_values_through_the_packed_epilogue(golden, logits_now):
    """+70 000 and +inf leave gelu_new beyond 65504: one saturated quad each per row and layer (300 rows, 2 layers);
    -70 000 becomes -0, 1e-5 / 1e-40 / -0.0 stay below 2^-14 (high plane 0).  With the NaN column every row of the second
    layer is NaN (NaN is not a saturation: fmaxf drops it), so only the first layer counts."""
    assert int(golden["special_saturated"]) == tool.expected_saturated(300, 2) == 1200
    assert int(golden["special_nan_saturated"]) == tool.expected_saturated(300, 1) == 600
    _same(logits_now, golden, ["special", "special_saturated", "special_nan", "special_nan_saturated"])


# ------------------------------------------------------------------------------------------ the format, from its definition
def split_f16x2(a):
    """bf16x3.h: hi = fp16(a) (0 when |a| < 2^-14), lo = fp16((a - hi) * 2^11); |a| clamped to 65504; NaN kept"""
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.where(np.isnan(a), a, np.clip(a, np.float32(-65504.0), np.float32(65504.0))).astype(np.float32)
        hi = np.where(np.abs(c) < np.float32(2.0 ** -14), np.float16(0.0), c.astype(np.float16)).astype(np.float16)
        lo = ((c - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi, lo


def join_f16x2(hi, lo):
    return hi.astype(np.float64) + lo.astype(np.float64) * 2.0 ** -11


def _edge_matrix(rows, cols, seed):
    g = np.random.default_rng(seed)
    a = (g.standard_normal((rows, cols)) * np.exp2(g.integers(-20, 14, (rows, cols)))).astype(np.float32)
    edge = np.array([2.0 ** -14, -2.0 ** -14, np.nextafter(np.float32(2.0 ** -14), np.float32(0)), 1e-5, -1e-5, 1e-40, -0.0, 0.0,
                     65504.0, -65504.0, 65520.0, 7e4, -7e4, 1e6, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -12, 1.0 + 2.0 ** -23, 2049.0],
                    dtype=np.float32)
    a[np.arange(len(edge)) * 3 % rows, np.arange(len(edge)) * 5 % cols] = edge
    return a


def test_f16x2_definition_on_the_cpu():
    a = _edge_matrix(256, 64, 3)
    hi, lo = split_f16x2(a)
    c = np.clip(a, -65504.0, 65504.0).astype(np.float64)
    err = np.abs(join_f16x2(hi, lo) - c)
    big = np.abs(c) >= 2.0 ** -14
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    # hi rounds c to 11 bits: |c - hi| <= 2^-11 2^e for c in [2^e, 2^(e+1)); lo rounds that remainder to 11 bits again
    assert (err[big] <= np.abs(c[big]) * 2.0 ** -22).all()
    assert (err[~big] <= 2.0 ** -26).all() and (hi[~big] == 0).all()  # carried by the scaled low plane alone
    assert (np.abs(join_f16x2(hi, lo)) <= 65504.0).all()
    h, l = split_f16x2(np.array([np.nan, np.inf, -np.inf, 7e4, -0.0], dtype=np.float32))
    assert np.isnan(h[0]) and h[1] == 65504.0 and h[2] == -65504.0 and h[3] == 65504.0 and l[1] == l[2] == l[3] == 0
    assert h[4] == 0 and not np.signbit(h[4]) and l[4] == 0 and np.signbit(l[4])


@gpu
def test_f16x2_gemm_equals_the_product_of_the_split_operands(monkeypatch):
    """256 x 64 with edge values through the packed-A GEMM (CAPDEC_HOOK_PACKA): the result is the fp64 product of what
    the numpy split reconstructs (clamped elements included), to 1e-6 of sum |a||b| -- the kernel's planes hold what the
    definition says"""
    from capdec_amd.engine import Engine
    monkeypatch.setenv("CAPDEC_HOOK_PACKA", "1")
    eng = Engine(0)
    eng.set_gemm_mode("f16x2")
    try:
        a = _edge_matrix(256, 64, 3)
        bt = (np.random.default_rng(4).standard_normal((64, 64)) * 0.2).astype(np.float32)
        out = eng.gemm(torch.from_numpy(a), torch.from_numpy(bt)).cpu().numpy().astype(np.float64)
    finally:
        eng.close()
    ar, br = join_f16x2(*split_f16x2(a)), join_f16x2(*split_f16x2(bt))
    ref = ar @ br.T
    scale = np.abs(ar) @ np.abs(br).T
    worst = float((np.abs(out - ref) / scale).max())
    print("f16x2 GEMM against the split operands: max |err| / sum|a||b| =", worst)
    assert worst < 1e-6, worst


# ------------------------------------------------------------------------------------------ LayerNorm: large-row form against small-row form
@gpu
def test_layernorm_large_rows_equal_small_rows():
    """16 500-row steps take the large-row LayerNorm launch (rows >= 16384), 1500-row steps the other one; in the
    batch-invariant mode the GEMMs and the attention do not depend on the batch, so captions [0, 300) must come out the
    same bits either way"""
    from capdec_amd import synth
    from capdec_amd.engine import Engine
    pe = tool._prefix(tool.N_CAP, 23)
    e = Engine(0)
    try:
        e.load_gpt2(synth.hot_gpt2_state_dict(42, synth.GPT2_TINY))
        e.set_batch_invariant(True)
        big = e.decode_beam(pe, tool.STOP_ID, tool.BEAM, tool.T)[:3]
        assert e.decode_step_rows()[0] == tool.N_CAP * tool.BEAM >= 16384
        small = e.decode_beam(pe[:300], tool.STOP_ID, tool.BEAM, tool.T)[:3]
    finally:
        e.set_batch_invariant(False)
        e.close()
    for name, a, b in zip(("ids", "lengths", "scores"), big, small):
        assert np.array_equal(tool._bits(a[:300]), tool._bits(b)), name
