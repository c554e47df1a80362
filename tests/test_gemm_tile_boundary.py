"""The persistent f16x2 GEMM (gemm_f16x2p_kernel<true, 4>) across the tiles of one block, and the decode results that hang on
it and on the fused lm_head.  Its epilogue requests a tile's bias and residual quads ahead of the LDS transposition
(gemm_epilogue_lds.h, AHEAD); a block's next tile re-uses the LDS the slabs lay in.  Needs an MI355X: ``pytest -m gpu``.

* f16x2 products through Engine.gemm on grids where a block walks 2 and 3 tiles (594 and 1170 tiles on 512 blocks, ragged
  edges -- rows and columns whose ahead-of-use loads are clamped into the matrix --, K = 64 / 128 / 768: K = 64 is a ring
  that re-sends its last k-step), every element against an fp64 product (computed on the device).  Bounds are the
  project's: plain product |out - fp64| / (|a| . |bt|^T) < 5e-7; with an epilogue atol 2e-5, rtol 1e-5.
* The same product in the batch-invariant mode, whole and in row slices of <= 512 tiles (one tile per block: no tile
  boundary inside a block): bit for bit the same.  A stage or a slab read early or stale shows as a wrong tile here.
* The two flagship shapes (25 000 rows) on seeded rows plus both rows of every 128-row tile edge.
* The launches are observed under rocprofv3 --kernel-trace (the way tests/test_hip_gemm_plans.py checks its claims).
* Beam decode of T = 3 at 640 and 25 000 rows (lse and top-5 of the fused lm_head decide every id and score; c_proj and
  mlp.c_proj of the 25 000-row steps are persistent launches with a residual): bit for bit what the commit before the
  epilogue change produced (tests/golden/tile_boundary_beam.npz, written by ``--write-golden`` on that commit).
"""
import importlib.util
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "tile_boundary_beam.npz")
KNOBS = ("CAPDEC_GEMM_MODE", "CAPDEC_HOOK_PACKA", "CAPDEC_HOOK_CACHE", "CAPDEC_H2W", "CAPDEC_PP", "CAPDEC_SPLITK",
         "CAPDEC_SPLITK_MID", "CAPDEC_X1_SPLITK", "CAPDEC_H2_PERSIST", "CAPDEC_FUSE_LN", "CAPDEC_X3_PACKA", "CAPDEC_X3_CHAIN",
         "CAPDEC_BATCH_INVARIANT")
# (M, N): 33 x 18 = 594 tiles (a second tile for 82 of the 512 blocks), 65 x 18 = 1170 tiles (two or three per block),
# and a ragged last row / column tile
SHAPES = ((4224, 2304), (8320, 2304), (4200, 2300))
KS = (64, 128, 768)
EPILOGUES = ("plain", "bias_gelu", "bias_resid_ldr")
PERSIST_BLOCKS = 512


def _env(**kw):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ["CAPDEC_HOOK_PACKA"] = "1"          # pre-packed A: the LayerNorm -> GEMM path of the decode step
    os.environ.update(kw)


@pytest.fixture(scope="module")
def engine():
    from capdec_amd.engine import Engine
    saved = {k: os.environ.get(k) for k in KNOBS}
    _env()
    eng = Engine(0)
    eng.set_gemm_mode("f16x2")
    yield eng
    eng.close()
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _operands(M, N, K, dev):
    g = torch.Generator().manual_seed(M * 31 + N * 7 + K)
    bt = (torch.randn(N, K, generator=g) * 0.2).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    a = torch.randn(M, K, generator=g).to(dev)
    resid = torch.randn(M, N, generator=g).to(dev)
    return a, bt, bias, resid


def _gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def _run(eng, epi, a, bt, bias, resid):
    """one Engine.gemm call of epilogue ``epi``; bias_resid_ldr reads the residual through a row stride ldr = N + 4 > N"""
    M, N = a.shape[0], bt.shape[0]
    if epi == "plain":
        return eng.gemm(a, bt)
    if epi == "bias_gelu":
        return eng.gemm(a, bt, bias=bias, act=3)
    wide = torch.full((M, N + 4), 555.0, device=a.device)
    wide[:, :N] = resid
    out = eng.gemm(a, bt, bias=bias, resid=wide[:, :N])
    torch.cuda.synchronize()
    return out


def _check(tag, got, epi, ref, scale, bias, resid):
    if epi == "plain":
        ratio = float(((got.double() - ref).abs() / scale).max())
        print(f"[tile boundary] {tag} plain: max |err| / sum|a||b| = {ratio:.3e} (bound 5e-7)")
        assert ratio < 5e-7, (tag, ratio)
        return
    y = ref + bias.double()
    y = _gelu_new(y) if epi == "bias_gelu" else y + resid.double()
    y = y.float()
    worst = float(((got - y).abs() - 1e-5 * y.abs()).max())
    print(f"[tile boundary] {tag} {epi}: max (|err| - rtol |y|) = {worst:.3e} (atol 2e-5)")
    assert worst <= 2e-5, (tag, epi, worst)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_walked_tiles_vs_fp64(engine, M, N, K):
    dev = engine.device
    a, bt, bias, resid = _operands(M, N, K, dev)
    ref = a.double() @ bt.double().t()
    scale = a.double().abs() @ bt.double().abs().t()
    for epi in EPILOGUES:
        got = _run(engine, epi, a, bt, bias, resid)
        torch.cuda.synchronize()
        _check(f"{M}x{N}x{K}", got, epi, ref, scale, bias, resid)


@pytest.mark.parametrize("M,N,K", [(8320, 2304, 768), (8320, 2304, 64), (4200, 2300, 128)])
def test_walked_tiles_equal_one_tile_per_block_bit_for_bit(M, N, K):
    """batch-invariant mode (no split-K, no launch-size dependent kernel): the whole product against row slices of at most
    512 tiles, in which no block has a second tile"""
    from capdec_amd.engine import Engine
    saved = {k: os.environ.get(k) for k in KNOBS}
    _env()
    eng = Engine(0)
    try:
        eng.set_gemm_mode("f16x2")
        eng.set_batch_invariant(True)
        a, bt, bias, resid = _operands(M, N, K, eng.device)
        tiles_n = -(-N // 128)
        step = (PERSIST_BLOCKS // tiles_n) * 128                 # 28 row tiles x 18 = 504 tiles
        assert -(-M // 128) * tiles_n > PERSIST_BLOCKS and (step // 128) * tiles_n <= PERSIST_BLOCKS
        for epi in EPILOGUES:
            whole = _run(eng, epi, a, bt, bias, resid)
            parts = [_run(eng, epi, a[r:r + step], bt, bias, resid[r:r + step]) for r in range(0, M, step)]
            torch.cuda.synchronize()
            sliced = torch.cat(parts)
            same = whole.view(torch.int32) == sliced.view(torch.int32)
            bad = (~same).nonzero()
            print(f"[tile boundary] {M}x{N}x{K} {epi}: {int((~same).sum())} elements differ from the sliced product")
            assert bool(same.all()), (epi, "first differing (row, column)", bad[0].tolist(), "tile", (bad[0] // 128).tolist())
    finally:
        eng.close()
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


FLAGSHIP = ((25000, 768, 768, "bias_resid_ldr"), (25000, 2304, 768, "bias_gelu"))


@pytest.mark.parametrize("M,N,K,epi", FLAGSHIP)
def test_flagship_shapes_vs_fp64(engine, M, N, K, epi):
    """c_proj / mlp.c_proj (1176 tiles on 512 blocks, with the residual) and the qkv width at 25 000 rows: 512 seeded rows
    plus the last row of every 128-row tile and the first of the next"""
    dev = engine.device
    a, bt, bias, resid = _operands(M, N, K, dev)
    got = _run(engine, epi, a, bt, bias, resid)
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(5)
    edges = torch.arange(128, M, 128)
    rows = torch.unique(torch.cat([torch.randint(0, M, (512,), generator=g), edges - 1, edges,
                                   torch.tensor([0, M - 1])])).to(dev)
    ref = a[rows].double() @ bt.double().t()
    _check(f"{M}x{N}x{K} rows", got[rows], epi, ref, None, bias, resid[rows])


# ------------------------------------------------------------------------------------------------ what was launched
def _plans_module():
    spec = importlib.util.spec_from_file_location("capdec_gemm_plans", os.path.join(ROOT, "tests", "test_hip_gemm_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TRACED = [(M, N, 64) for M, N in SHAPES] + [(25000, 768, 768)]


def _run_traced():
    from capdec_amd.engine import Engine
    _env()
    eng = Engine(0)
    eng.set_gemm_mode("f16x2")
    for M, N, K in TRACED:
        a, bt, bias, resid = _operands(M, N, K, eng.device)
        eng.gemm(a, bt, bias=bias, resid=resid)
        torch.cuda.synchronize()
        print("ran", M, N, K, flush=True)
    eng.close()


def test_cases_reach_the_persistent_kernel(tmp_path):
    """the shapes above run gemm_f16x2p_kernel<true, 4> on 512 blocks of 256 threads (observed, not assumed)"""
    P = _plans_module()
    exe = shutil.which("rocprofv3") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "rocprofv3")
    assert os.path.exists(exe), "rocprofv3 not found: the launched kernels cannot be observed (this test does not skip)"
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run(["timeout", "-k", "10", "240", exe, "--kernel-trace", "--output-format", "csv", "-d", str(tmp_path), "--",
                        sys.executable, os.path.abspath(__file__), "--run-traced"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    groups = P.launches_by_gemm(P._read_kernel_trace(str(tmp_path)))
    seen = [g[:4] for g in groups]
    print("[tile boundary] traced:", seen)
    assert seen == [P.H2P + (PERSIST_BLOCKS, 256)] * len(TRACED), seen


# ------------------------------------------------------------------------------------------------ fused lm_head
BEAM_CASES = (("r640", 128, {}), ("r640_wide", 128, {"CAPDEC_H2W": "2"}), ("r25000", 5000, {}))


def _beam(n, env):
    """beam-5 decode of T = 3 on a one-layer GPT-2 of vocabulary 1531 (12 column tiles): n x 5 rows from the second step
    on -- 25 000 rows: 98 x 12 = 1176 lm_head tiles of 256 x 128 on 512 blocks; 640 rows: the 128-row kernel (as shipped) or,
    with the wide tile forced, 36 tiles"""
    from capdec_amd import synth
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    from capdec_amd import gpt2_prefix_eval as E
    saved = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        dims = synth.GPT2Dims(n_layer=1, vocab=1531, n_pos=64)
        sd = synth.hot_state_dict(42, "mlp", 512, 10, dims=dims)
        model = ClipCaptionModel(10, prefix_dim=512, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0").eval()
        model.load_state_dict(sd)
        x = synth.synthetic_clip_embeddings(n, 512, seed=3)
        pe = model.clip_project(x).reshape(n, 10, -1)
        ids, lens, scores, _ = E.decode_beam_ids(model, pe, 1530, 5, 3)[:4]
        torch.cuda.synchronize()
        return ids.cpu().numpy().astype(np.int16), lens.cpu().numpy().astype(np.int8), scores.cpu().numpy()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("tag,n,env", BEAM_CASES, ids=[c[0] for c in BEAM_CASES])
def test_lm_head_beam_results_bit_for_bit(tag, n, env):
    want = np.load(GOLDEN)
    ids, lens, scores = _beam(n, env)
    np.testing.assert_array_equal(ids, want[tag + "_ids"])
    np.testing.assert_array_equal(lens, want[tag + "_lens"])
    np.testing.assert_array_equal(scores.view(np.int32), want[tag + "_scores"].view(np.int32))


if __name__ == "__main__":
    if sys.argv[1:] == ["--run-traced"]:
        _run_traced()
    elif len(sys.argv) == 3 and sys.argv[1] == "--write-golden":       # run on the commit whose results are the reference
        out = {}
        for tag, n, env in BEAM_CASES:
            out[tag + "_ids"], out[tag + "_lens"], out[tag + "_scores"] = _beam(n, env)
        np.savez_compressed(sys.argv[2], **out)
        print("wrote", sys.argv[2], {k: v.shape for k, v in out.items()})
    else:
        sys.exit("usage: test_gemm_tile_boundary.py --run-traced | --write-golden FILE")
