"""MappingType.TransformerDecoder: the encoder-decoder mapper (reference transformer_mapper.py:130-145) in HIP.

The yardstick is the reference class itself, run by tools/gen_golden.py (``mapper_encdec``, ``decode_encdec_tiny``) on the
hot weights of ``synth.hot_encdec_mapper_state_dict``: tests/golden/mapper_encdec_{512,640,p5,p40}.npz hold inputs, the
fp32 output, the float64 output and the weights' checksum.  Shapes the fixtures do not cover (more than one chunk,
prefix_length != clip_length both ways) are judged by ``restate`` below, a float64-capable restatement of the algorithm
written from its description; the CPU tests first pin it to the fixtures (1e-5 in fp32, 1e-9 in float64), and show that
the mistake a fused [q|k|v] projection would make -- the odd decoder layers taking keys from norm1(x) instead of x -- is
hundreds of bounds away, so it cannot hide inside a tolerance.

Bounds: 2e-4 absolute on outputs of rms 1..10 (the bound of the 8-layer TransformerMapper against its fixture,
test_hip_parity.py), 3e-4 for the 40 x 40 geometry (as that file's 80-token case).  The reference's own fp32 rounding,
|fp32 - float64|, is 1.4e-6 .. 5.7e-6 on the fixtures: under a tenth of the bound.

Measured on an MI355X (max |HIP - fixture|, default mode): 4.8e-6, 5.4e-6, 3.1e-6, 1.4e-6 for 512 / 640 / p5 / p40 -- under
3 % of the bounds; up to 8.3e-6 in the f32 and bf16x3 modes ("Encoder-decoder mapper")."""
import math
import os
import re

import numpy as np
import pytest
import torch

from capdec_amd import synth

T = torch.from_numpy
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("512", "640", "p5", "p40")
ATOL = {"512": 2e-4, "640": 2e-4, "p5": 2e-4, "p40": 3e-4}      # the TransformerMapper tests' bounds, not what these kernels give
ENC = 512


# ----------------------------------------------------------------------------------- the restatement
def _ln(x, w, b):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


def _layer(sd, p, x, y, heads=8):
    """one pre-LN layer: queries from norm1(x), keys / values from ``y`` AS GIVEN (None: from norm1(x) too)"""
    g = lambda k: sd[p + k].to(x.dtype)
    xn = _ln(x, g("norm1.weight"), g("norm1.bias"))
    y = xn if y is None else y
    n, nq, w = x.shape
    hd = w // heads
    q = (xn @ g("attn.to_queries.weight").T).reshape(n, nq, heads, hd)
    kv = (y @ g("attn.to_keys_values.weight").T).reshape(n, y.shape[1], 2, heads, hd)
    att = (torch.einsum("bnhd,bmhd->bnmh", q, kv[:, :, 0]) * hd ** -0.5).softmax(dim=2)
    o = torch.einsum("bnmh,bmhd->bnhd", att, kv[:, :, 1]).reshape(n, nq, w)
    x = x + o @ g("attn.project.weight").T + g("attn.project.bias")
    h = torch.relu(_ln(x, g("norm2.weight"), g("norm2.bias")) @ g("mlp.fc1.weight").T + g("mlp.fc1.bias"))
    return x + h @ g("mlp.fc2.weight").T + g("mlp.fc2.bias")


def restate(sd, x, dtype=torch.float64, wrong=False, prefix="clip_project."):
    """x [n, D] -> [n, P, d].  ``wrong``: the odd decoder layers take keys / values from norm1(x) (what a fused projection
    of one input computes) -- NOT the reference."""
    x = x.to(dtype)
    pc = sd[prefix + "prefix_const"].to(dtype)
    L = 0
    while f"{prefix}ref_encoder.layers.{L}.norm1.weight" in sd:
        L += 1
    ref = (x @ sd[prefix + "linear.weight"].to(dtype).T + sd[prefix + "linear.bias"].to(dtype)).reshape(x.shape[0], -1, ENC)
    for i in range(L):
        ref = _layer(sd, f"{prefix}ref_encoder.layers.{i}.", ref, None)
    h = pc.unsqueeze(0).expand(x.shape[0], *pc.shape)
    for i in range(2 * L):
        p = f"{prefix}prefix_decoder.layers.{i}."
        h = _layer(sd, p, h, ref) if i % 2 == 0 else _layer(sd, p, h, None if wrong else h)
    return h


def _case(golden, tag):
    g = golden("mapper_encdec_" + tag)
    D, P, C, L, seed = (int(v) for v in g["geom"])
    sd = synth.hot_encdec_mapper_state_dict(seed, D, P, C, L)
    assert synth.state_dict_checksum(sd) == int(g["crc"]), "RNG drift"
    return g, sd, (D, P, C, L)


#: geometries judged by the restatement alone: (D, P, C, L, weight seed, bound)
RESTATED = {"chunks": (512, 10, 10, 2, 46, 2e-4), "p5c7": (512, 5, 7, 3, 44, 2e-4), "p12c3": (512, 12, 3, 2, 47, 2e-4),
            "cmax": (512, 4, 204, 1, 48, 3e-4)}        # the longest clip_length whose keys fit the LDS at head_dim 96


# ----------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("tag", CASES)
def test_restatement_equals_reference_fixture(golden, tag):
    g, sd, _ = _case(golden, tag)
    x = T(g["x"])
    with torch.no_grad():
        e32 = float((restate(sd, x, torch.float32) - T(g["y"])).abs().max())
        e64 = float((restate(sd, x, torch.float64) - T(g["y_f64"])).abs().max())
    print(f"restatement vs reference, {tag}: fp32 {e32:.2e}, float64 {e64:.2e}")
    assert e32 <= 1e-5
    assert e64 <= 1e-9


@pytest.mark.parametrize("tag", CASES)
def test_fixture_conditioning_and_wrong_variant_is_visible(golden, tag):
    """(i) the reference's own fp32 rounding is at most a tenth of the bound; (ii) keys from norm1(x) in the odd decoder
    layers land at least 100 bounds away; (iii) the outputs' rms is in 1..10 like the TransformerMapper fixtures"""
    g, sd, _ = _case(golden, tag)
    y64 = T(g["y_f64"])
    floor = float((T(g["y"]).double() - y64).abs().max())
    with torch.no_grad():
        wrong = float((restate(sd, T(g["x"]), wrong=True) - y64).abs().max())
    rms = float(y64.pow(2).mean().sqrt())
    print(f"{tag}: floor {floor:.2e} (recorded {float(g['floor']):.2e}), wrong variant {wrong:.3f}, rms {rms:.2f}")
    assert floor <= ATOL[tag] / 10
    assert wrong >= 100 * ATOL[tag]
    assert 1.0 <= rms <= 10.0


@pytest.mark.parametrize("name", sorted(RESTATED))
def test_restated_geometries_are_well_conditioned(name):
    """the same three conditions for the geometries the GPU tests judge by the restatement (the floor is the
    restatement's own fp32 run against its float64 run)"""
    D, P, C, L, seed, atol = RESTATED[name]
    sd = synth.hot_encdec_mapper_state_dict(seed, D, P, C, L)
    x = synth.synthetic_clip_embeddings(4, D, seed=5)
    with torch.no_grad():
        y64 = restate(sd, x)
        floor = float((restate(sd, x, torch.float32).double() - y64).abs().max())
        wrong = float((restate(sd, x, wrong=True) - y64).abs().max())
    rms = float(y64.pow(2).mean().sqrt())
    print(f"{name}: floor {floor:.2e}, wrong variant {wrong:.3f}, rms {rms:.2f}")
    assert floor <= atol / 10 and wrong >= 100 * atol and 1.0 <= rms <= 10.0


def test_surface_keys_and_strict_load(golden):
    from capdec_amd.gpt2_prefix import ClipCaptionModel, ClipCaptionPrefix, MappingType as MT
    from capdec_amd.transformer_mapper import TransformerEncoderDecoder
    g = golden("mapper_encdec_512")
    m = ClipCaptionModel(10, prefix_dim=512, num_layers=4, mapping_type=MT.TransformerDecoder, gpt2_dims=synth.GPT2_TINY)
    assert isinstance(m.clip_project, TransformerEncoderDecoder)
    assert m.clip_project._keys() == [str(k) for k in g["keys"]]
    assert (m.clip_project.dim_clip, m.clip_project.dim_embedding, m.clip_project.prefix_length,
            m.clip_project.clip_length, m.clip_project.num_layers) == (512, 768, 10, 10, 4)
    sd = synth.hot_encdec_mapper_state_dict(43, 512, 10, 10, 4, prefix="")
    assert list(sd) != m.clip_project._keys() and sorted(sd) == sorted(m.clip_project._keys())
    m.clip_project.load_state_dict(sd)
    bad = dict(sd)
    del bad["prefix_decoder.layers.3.attn.to_keys_values.weight"]
    with pytest.raises(RuntimeError, match="Missing key"):
        m.clip_project.load_state_dict(bad)
    bad = dict(sd)
    bad["prefix_const"] = torch.zeros(9, 768)
    with pytest.raises(RuntimeError, match="size mismatch for prefix_const"):
        m.clip_project.load_state_dict(bad)
    # shapes of the two kinds of decoder layer
    assert tuple(sd["prefix_decoder.layers.0.attn.to_keys_values.weight"].shape) == (1536, 512)
    assert tuple(sd["prefix_decoder.layers.1.attn.to_keys_values.weight"].shape) == (1536, 768)
    assert tuple(sd["linear.weight"].shape) == (10 * 512, 512)
    # ClipCaptionPrefix may be built with it (its parameters() only lists keys)
    ClipCaptionPrefix(10, prefix_dim=512, num_layers=4, mapping_type=MT.TransformerDecoder, gpt2_dims=synth.GPT2_TINY)


def test_hot_state_dict_round_trip(golden):
    g = golden("decode_encdec_tiny")
    sd = synth.hot_state_dict(42, "transformer_decoder", 512, 10, 10, 4, synth.GPT2_TINY)
    assert synth.state_dict_checksum(sd) == int(g["sd_crc"])
    mapper = {k: v for k, v in sd.items() if k.startswith("clip_project.")}
    assert synth.state_dict_checksum(mapper) == synth.state_dict_checksum(synth.hot_encdec_mapper_state_dict(43, 512, 10, 10, 4))
    assert synth.state_dict_checksum(mapper) == int(golden("mapper_encdec_512")["crc"])
    with pytest.raises(ValueError):
        synth.hot_state_dict(42, "transformer_decoder_", 512, 10, 10, 4, synth.GPT2_TINY)


def test_abi_version_6_and_symbol():
    from capdec_amd import _capi
    header = open(os.path.join(ROOT, "include", "capdec.h")).read()
    assert int(re.search(r"#define CAPDEC_ABI_VERSION (\d+)", header).group(1)) == 6 == _capi.ABI_VERSION
    assert re.search(r"\bint capdec_load_mapper_encdec\(capdec_ctx \*\w+, const capdec_edmapper_weights \*\w+\);", header)
    assert "capdec_load_mapper_encdec" in _capi.SIGNATURES
    fields = [f[0] for f in _capi.EDMapperWeights._fields_]
    assert fields[:9] == ["prefix_dim", "prefix_length", "clip_length", "num_layers", "num_heads", "d", "enc_dim",
                          "enc_mlp_hidden", "dec_mlp_hidden"]
    struct = re.search(r"\nstruct capdec_edmapper_weights \{(.*?)\};", header, flags=re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", " ", struct, flags=re.S)
    assert re.findall(r"\*?\b(\w+)\s*[,;]", struct) == fields


def test_edmapper_struct_layout_matches_ctypes(tmp_path):
    """size and every field offset of capdec_edmapper_weights as the C compiler lays them out = the ctypes mirror"""
    import ctypes as C
    import subprocess
    from capdec_amd import _capi
    cls, cname = _capi.EDMapperWeights, "capdec_edmapper_weights"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "capdec.h"', 'int main(void) {',
             f'  printf("size %zu\\n", sizeof({cname}));']
    lines += [f'  printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert C.sizeof(cls) == int(got.pop("size"))
    assert {f: getattr(cls, f).offset for f, _ in cls._fields_} == {k: int(v) for k, v in got.items()}


# ----------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def eng():
    from capdec_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _err(y, want):
    return float((y.double().cpu() - torch.as_tensor(want).double()).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f16x2", "f32", "bf16x3", "bf16", "f16"])
@pytest.mark.parametrize("tag", CASES)
def test_encdec_mapper_vs_reference_fixture(eng, golden, tag, mode):
    """every GEMM mode: the mapper is promised fp32-accurate in all of them"""
    g, sd, (D, P, C, L) = _case(golden, tag)
    eng.set_gemm_mode(mode)
    try:
        eng.load_mapper_encdec(sd)
        assert eng.mapper["kind"] == "transformer_decoder" and eng.mapper["clip_length"] == C and eng.mapper["num_layers"] == L
        y = eng.mapper_forward(T(g["x"]))
    finally:
        eng.set_gemm_mode("f16x2")
    assert tuple(y.shape) == g["y"].shape
    e = _err(y, g["y"])
    print(f"encdec mapper {tag} {mode}: max |HIP - reference| {e:.2e} (bound {ATOL[tag]:.0e}, floor {float(g['floor']):.1e})")
    assert e <= ATOL[tag]


@pytest.mark.gpu
def test_encdec_mapper_past_one_chunk_and_batch_invariance(eng):
    D, P, C, L, seed, atol = RESTATED["chunks"]
    n = 8192 + 300
    sd = synth.hot_encdec_mapper_state_dict(seed, D, P, C, L)
    eng.load_mapper_encdec(sd)
    x = synth.synthetic_clip_embeddings(n, D, seed=6)
    y = eng.mapper_forward(x).cpu()
    assert tuple(y.shape) == (n, P, 768)
    assert bool(torch.isfinite(y).all())
    assert bool((y.abs().amax(dim=(1, 2)) > 0).all()), "an output row was never written"
    assert bool((y.reshape(n * P, -1).abs().amax(dim=1) > 0).all())
    rows = list(range(4)) + list(range(8190, 8194)) + list(range(n - 8, n))
    with torch.no_grad():
        want = restate(sd, x[rows])
    e = _err(y[rows], want)
    print(f"encdec mapper, {n} captions: max |HIP - restatement| on {len(rows)} rows {e:.2e} (bound {atol:.0e})")
    assert e <= atol
    # the same captions alone, in a batch of 7 and in the large batch: bit-identical under batch invariance
    eng.set_batch_invariant(True)
    try:
        big = eng.mapper_forward(x).cpu()
        seven = eng.mapper_forward(x[8189:8196]).cpu()
        one = eng.mapper_forward(x[8192:8193]).cpu()
    finally:
        eng.set_batch_invariant(False)
    assert _err(big[rows], want) <= atol
    assert torch.equal(seven, big[8189:8196])
    assert torch.equal(one[0], big[8192])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["p5c7", "p12c3"])
def test_encdec_mapper_prefix_length_differs_from_clip_length(eng, name):
    D, P, C, L, seed, atol = RESTATED[name]
    sd = synth.hot_encdec_mapper_state_dict(seed, D, P, C, L)
    eng.load_mapper_encdec(sd)
    x = synth.synthetic_clip_embeddings(5, D, seed=7)
    y = eng.mapper_forward(x)
    assert tuple(y.shape) == (5, P, 768)
    with torch.no_grad():
        e = _err(y, restate(sd, x))
    print(f"encdec mapper {name} (P {P}, C {C}): max |HIP - restatement| {e:.2e} (bound {atol:.0e})")
    assert e <= atol


@pytest.mark.gpu
def test_encdec_mapper_empty_batch_and_reloads(golden):
    """n = 0; MLP -> enc-dec -> TransformerMapper -> enc-dec on ONE context gives the fixture results each time"""
    from capdec_amd.engine import Engine
    g, sd, (D, P, C, L) = _case(golden, "512")
    gm = golden("mappers")
    e = Engine(0)
    try:
        e.load_mapper_mlp(synth.hot_mlp_mapper_state_dict(43, 512, 10))
        np.testing.assert_allclose(e.mapper_forward(T(gm["x_512"])).cpu().reshape(4, -1).numpy(), gm["mlp_512"], atol=2e-5)
        e.load_mapper_encdec(sd)
        assert tuple(e.mapper_forward(torch.zeros(0, 512)).shape) == (0, P, 768)
        assert _err(e.mapper_forward(T(g["x"])), g["y"]) <= ATOL["512"]
        e.load_mapper_transformer(synth.hot_transformer_mapper_state_dict(43, 512, 10, 10, 8))
        np.testing.assert_allclose(e.mapper_forward(T(gm["x_512"])).cpu().numpy(), gm["tm_512"], atol=2e-4)
        g5, sd5, _ = _case(golden, "p5")
        e.load_mapper_encdec(sd5)
        assert _err(e.mapper_forward(T(g5["x"])), g5["y"]) <= ATOL["p5"]
        e.load_mapper_encdec(sd)
        assert _err(e.mapper_forward(T(g["x"])), g["y"]) <= ATOL["512"]
    finally:
        e.close()


def _model(dims=synth.GPT2_TINY):
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    m = ClipCaptionModel(10, clip_length=10, prefix_dim=512, num_layers=4, mapping_type=MappingType.TransformerDecoder,
                         gpt2_dims=dims).to("cuda:0").eval()
    sd = synth.hot_state_dict(42, "transformer_decoder", 512, 10, 10, 4, dims)
    m.load_state_dict(sd)
    return m, sd


class FakeTok:
    def __init__(self, stop):
        self.stop = stop

    def encode(self, s):
        return [self.stop]

    def decode(self, ids):
        return " ".join(str(int(i)) for i in ids)


@pytest.mark.gpu
def test_encdec_decode_vs_reference_golden(golden):
    """end to end against the reference's generate2 / generate_beam (the criteria of test_decode_tiny): greedy ids and
    lengths identical; beam ids, lengths and order identical, scores within 1e-4; every caption of the fixture"""
    from capdec_amd import gpt2_prefix_eval as E
    g = golden("decode_encdec_tiny")
    dims = synth.GPT2_TINY
    model, sd = _model(dims)
    assert synth.state_dict_checksum(sd) == int(g["sd_crc"]), "RNG drift"
    try:
        # ---- greedy
        x = T(g["greedy_x"])
        pe = model.clip_project(x).reshape(8, 10, -1)
        e = _err(pe, g["greedy_prefix_embed"])
        print(f"decode fixture, greedy prefix: max |HIP - reference| {e:.2e}")
        assert e <= 2e-4
        stop = int(g["greedy_stop_id"])
        ids, lens = E.decode_greedy_ids(model, pe, stop, 12)             # from our own prefix: the whole path
        np.testing.assert_array_equal(lens.cpu().numpy(), g["greedy_lens_T12"])
        np.testing.assert_array_equal(ids.cpu().numpy(), g["greedy_ids_T12"])
        ids, lens = E.decode_greedy_ids(model, pe, dims.vocab + 5, 12, alt_stop_id=-1)
        np.testing.assert_array_equal(ids.cpu().numpy(), g["greedy_ids_nostop"])
        want = [" ".join(str(int(v)) for v in g["greedy_ids_T12"][r][:int(g["greedy_lens_T12"][r])]) for r in range(8)]
        assert E.generate2_batch(model, FakeTok(stop), pe, entry_length=12) == want
        for r in range(8):
            assert int(g["greedy_lens_T12"][r]) > 1
            assert E.generate2(model, FakeTok(stop), embed=pe[r:r + 1], entry_length=12) == want[r]
        # ---- beam
        nb = g["beam_x"].shape[0]
        pe = model.clip_project(T(g["beam_x"])).reshape(nb, 10, -1)
        e = _err(pe, g["beam_prefix_embed"])
        print(f"decode fixture, beam prefix: max |HIP - reference| {e:.2e}")
        assert e <= 2e-4
        for name, st in (("nostop", dims.vocab + 5), ("stop", int(g["beam_stop_id"]))):
            ids, lens, scores, order = (t.cpu().numpy() for t in E.decode_beam_ids(model, pe, st, 5, 12))
            gt, gl = g[f"beam_{name}_tokens_T12"], g[f"beam_{name}_seqlen_T12"]
            gs, go = g[f"beam_{name}_scores_T12"], g[f"beam_{name}_order_T12"]
            np.testing.assert_array_equal(order, go)
            for r in range(nb):
                np.testing.assert_array_equal(ids[r], gt[r][go[r]])
                np.testing.assert_array_equal(lens[r], gl[r][go[r]].astype(np.int32))
                np.testing.assert_allclose(scores[r], gs[r][go[r]], atol=1e-4)
        st = int(g["beam_stop_id"])
        for r in range(nb):
            gt, gl, go = g["beam_stop_tokens_T12"][r], g["beam_stop_seqlen_T12"][r], g["beam_stop_order_T12"][r]
            want = [" ".join(str(int(v)) for v in gt[b][:int(gl[b])]) for b in go]
            assert E.generate_beam(model, FakeTok(st), embed=pe[r:r + 1], entry_length=12) == want
        # ---- forward (logits / loss without autograd) runs through the same mapper
        tokens = torch.tensor(g["greedy_ids_T12"][:2, :6])
        out = model(tokens, x[:2], labels=tokens)
        assert tuple(out.logits.shape) == (2, 16, dims.vocab) and math.isfinite(float(out.loss))
    finally:
        model.release()


@pytest.mark.gpu
def test_train_step_refuses_encdec_mapper_and_context_survives(golden):
    from capdec_amd import train as TR
    from capdec_amd._capi import CapdecError
    g = golden("decode_encdec_tiny")
    model, sd = _model()
    try:
        x = T(g["greedy_x"])
        tokens = torch.tensor(g["greedy_ids_T12"][:, :6])
        opt = TR.AdamW(model.parameters(), lr=1e-4)
        with pytest.raises(CapdecError, match="inference-only"):
            TR.train_step(model, opt, tokens, None, x)
        eng = model.engine
        with pytest.raises(CapdecError, match="train_step: the encoder-decoder mapper is inference-only"):     # the C ABI itself
            eng.train_step(x, tokens, 1e-4)
        y = eng.mapper_forward(x)
        assert _err(y, g["greedy_prefix_embed"]) <= 2e-4
    finally:
        model.release()


@pytest.mark.gpu
def test_oversized_clip_length_is_refused_on_the_host(eng, golden):
    """one 96-wide head's K, V (padded rows of 97) and P = 4 query rows, plus a score row for each of the block's four
    wavefronts, need (2 C 97 + 4 * 96 + 4 C) * 4 bytes (the launch's own formula, attn_cross_lds_bytes): more than 160 KB
    from C = 205.  The refusal is a CAPDEC_CHECK on the host -- no launch -- and the context goes on working."""
    from capdec_amd._capi import CapdecError
    P = RESTATED["cmax"][1]
    lds = lambda c: (2 * c * 97 + P * 96 + 4 * c) * 4
    C = next(c for c in range(1, 4096) if lds(c) > 160 * 1024)
    assert lds(C - 1) <= 160 * 1024 and 200 < C < 220 and C - 1 == RESTATED["cmax"][2]
    g, sd, _ = _case(golden, "512")
    eng.load_mapper_encdec(sd)
    big = synth.hot_encdec_mapper_state_dict(48, 512, P, C, 1)
    with pytest.raises(CapdecError, match="LDS"):
        eng.load_mapper_encdec(big)
        eng.mapper_forward(synth.synthetic_clip_embeddings(1, 512, seed=1))
    eng.load_mapper_encdec(sd)
    assert _err(eng.mapper_forward(T(g["x"])), g["y"]) <= ATOL["512"]
    # the largest clip_length that fits does run (the blocks use more than 64 KB of dynamic LDS)
    ok = synth.hot_encdec_mapper_state_dict(48, 512, P, C - 1, 1)
    eng.load_mapper_encdec(ok)
    x = synth.synthetic_clip_embeddings(2, 512, seed=1)
    y = eng.mapper_forward(x)
    assert bool(torch.isfinite(y).all())
    with torch.no_grad():
        assert _err(y, restate(ok, x)) <= RESTATED["cmax"][5]
