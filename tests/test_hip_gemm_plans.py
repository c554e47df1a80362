"""Every GEMM kernel and planner regime, element by element against an fp64 product.  Needs an MI355X: ``pytest -m gpu``.

CASES is a table: precision mode, environment knobs, shape, strides, epilogue -- and the kernel, block count, workgroup
size and split-K slice count the case CLAIMS to reach (the decisions of gemm_plan(), gemm_plan.h; tests/test_gemm_plan.py
checks the packed rows against that planner without a GPU).  ``test_gemm_plan_case`` runs each case through the
capdec_gemm_f32 hook in a fresh Engine and compares ALL elements with the fp64 CPU product;
``test_cases_run_the_kernels_they_claim`` runs this file as a script (every case once, in table order) in a child
process under ``rocprofv3 --kernel-trace`` and checks each claim against the launch that was observed, so that a
threshold that moves in a planner turns a case red instead of silently re-routing it to another kernel.

Bounds (the project's existing ones): plain product in the fp32-accurate modes |out - ref| / (|a| . |bt|^T) < 5e-7; one-plane
modes < 5e-7 against the fp64 product of the bf16- / fp16-rounded operands and > 1e-5 away from the unrounded product;
with an epilogue atol 2e-5 (3e-5 one-plane), rtol 1e-5 against the fp64 result cast to fp32."""
import collections
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# every knob a case may set: cleared before each case, so a case runs under exactly its own environment
KNOBS = ("CAPDEC_GEMM_MODE", "CAPDEC_HOOK_PACKA", "CAPDEC_HOOK_CACHE", "CAPDEC_H2W", "CAPDEC_PP", "CAPDEC_SPLITK",
         "CAPDEC_SPLITK_MID", "CAPDEC_X1_SPLITK", "CAPDEC_H2_PERSIST", "CAPDEC_FUSE_LN", "CAPDEC_X3_PACKA", "CAPDEC_X3_CHAIN",
         "CAPDEC_BATCH_INVARIANT")

# ---- kernels as (name, template arguments): what the trace shows, mangled or demangled (kernel_signature)
H2P = ("gemm_f16x2p_kernel", (1, 4))                      # 128 x 128, two accumulator sets, float4 epilogue through LDS
H2P_SC = ("gemm_f16x2p_kernel", (0, 4))                   # ... scalar epilogue (N % 4 != 0 or an unaligned stride)
H2P_SK = ("gemm_f16x2p_splitk_kernel", (0,))               # split-K of the 128 x 128 kernels: one template over KIND (0 = two planes)
PP10 = ("gemm_pp_kernel", (4, 2, 2, 2, 5, 1))             # ping-pong 256 x 128 (P256x128), 512 threads
PP14 = ("gemm_pp_kernel", (4, 2, 2, 3, 4, 0))             # ping-pong 256 x 192 (P256x192s)
PP10_SK = ("gemm_pp_splitk_kernel", (4, 2, 2, 2, 5, 1))
PP14_SK = ("gemm_pp_splitk_kernel", (4, 2, 2, 3, 4, 0))
W2 = ("gemm_h2w_kernel", (2, 2, 4, 2, 3, 2))              # one accumulator set, 256 x 128 (W256x128)
W8 = ("gemm_h2w_kernel", (2, 2, 2, 3, 4, 2))              # one accumulator set, 128 x 192 (W128x192)
X3P = ("gemm_bf16x3p_kernel", (1,))
X3P_SC = ("gemm_bf16x3p_kernel", (0,))
X3P_SK = ("gemm_bf16x3p_splitk_kernel", ())
X3 = ("gemm_bf16x3_kernel", ())                           # fp32 A split inside the kernel (no packed A)
F32 = ("gemm_f32_kernel", (32, 2))
F32_BK16 = ("gemm_f32_kernel", (16, 3))                   # N >= 3072 or K >= 2048
KIND = {"f16": 1, "bf16": 2}


def X1(mode, vec4=True):                                  # one-plane kernels: <VEC4, KIND, ring depth 3 (vec4) / 4>
    return ("gemm_x1_kernel", (int(vec4), KIND[mode], 3 if vec4 else 4))


def X1_SK(mode):
    return ("gemm_f16x2p_splitk_kernel", (KIND[mode],))


Case = collections.namedtuple("Case", "id mode env M N K kernel blocks wg S bias act resid lda ldc ldr")
PACKA = {"CAPDEC_HOOK_PACKA": "1"}
CACHE = {"CAPDEC_HOOK_PACKA": "1", "CAPDEC_HOOK_CACHE": "1"}
CASES = []


def tiles(M, N, bm=128, bn=128):
    return -(-M // bm) * -(-N // bn)


def case(id, mode, env, shape, kernel, blocks, wg=256, S=1, bias=False, act=0, resid=None, lda=0, ldc=0, ldr=0):
    """resid: None | "sep" (its own tensor) | "alias" (the output itself, h += ...); lda / ldc / ldr: 0 = dense"""
    M, N, K = shape
    CASES.append(Case(id, mode, dict(env), M, N, K, kernel, blocks, wg, S, bias, act, resid, lda, ldc, ldr))


# (bias, act, resid): act 0..3 with bias and residual, and each of bias / residual / both absent
EPILOGUES = [(True, 0, "sep"), (True, 1, "sep"), (True, 2, "sep"), (True, 3, "sep"), (True, 3, None), (False, 0, "sep"),
             (False, 2, None)]


def family(id, mode, env, shape, kernel, blocks, wg=256, S=1, epilogues=True):
    """the plain product and, on this shape of the kernel family, every epilogue"""
    case(id, mode, env, shape, kernel, blocks, wg, S)
    if epilogues:
        for b, act, r in EPILOGUES:
            case(f"{id}-epi-b{int(b)}a{act}r{int(r is not None)}", mode, env, shape, kernel, blocks, wg, S, bias=b, act=act, resid=r)


def E(*dicts, **kw):
    out = {}
    for d in dicts:
        out.update(d)
    out.update({k: str(v) for k, v in kw.items()})
    return out


# ---------------------------------------------------------------- persistent blocks: a second tile per block
family("h2p-persist", "f16x2", PACKA, (3125, 3072, 768), H2P, 512)                        # 600 tiles on 512 blocks
family("h2p-persist-scalar", "f16x2", PACKA, (3125, 3070, 768), H2P_SC, 512)              # N % 4 != 0: 600 tiles on 512 blocks
family("x1-persist-bf16", "bf16", {}, (5000, 3072, 768), X1("bf16"), 768)                 # 960 tiles on 768 slots
case("x1-persist-f16", "f16", {}, (5000, 3072, 768), X1("f16"), 768)
case("h2p-block-per-tile", "f16x2", PACKA, (1000, 50257, 768), H2P_SC, 3144)              # above four rounds: one block per tile
case("h2p-no-persist", "f16x2", E(PACKA, CAPDEC_H2_PERSIST=0), (3125, 3072, 768), H2P, 600)
case("x1-no-persist", "bf16", E(CAPDEC_H2_PERSIST=0), (3125, 3072, 768), X1("bf16"), 600)
case("x1-one-round", "bf16", {}, (3125, 3072, 768), X1("bf16"), 600)                      # 600 tiles <= 768 slots
# ---------------------------------------------------------------- split-K of the 128 x 128 kernels: regimes (a) and (b)
for mode, sk in (("f16x2", H2P_SK), ("bf16x3", X3P_SK)):
    case(f"splitk-a-edge-{mode}", mode, PACKA, (512, 768, 768), sk, 24 * 6, S=6)
    family(f"splitk-b-first-{mode}", mode, PACKA, (513, 768, 768), sk, 30 * 3, S=3, epilogues=mode == "bf16x3")
H2W0 = E(PACKA, CAPDEC_H2W=0)
family("splitk-b-3125", "f16x2", H2W0, (3125, 768, 768), H2P_SK, 150 * 3, S=3)
case("splitk-b-1500", "f16x2", H2W0, (1500, 2304, 768), H2P_SK, 216 * 2, S=2)
for knob in ("CAPDEC_SPLITK_MID", "CAPDEC_SPLITK"):
    case(f"splitk-b-3125-{knob[7:].lower()}-off", "f16x2", E(H2W0, **{knob: 0}), (3125, 768, 768), H2P, 150)
    case(f"splitk-b-1500-{knob[7:].lower()}-off", "f16x2", E(H2W0, **{knob: 0}), (1500, 2304, 768), H2P, 216)
case("splitk-a-512-mid-off", "f16x2", E(PACKA, CAPDEC_SPLITK_MID=0), (512, 768, 768), H2P_SK, 24 * 6, S=6)   # (a) is not (b)
case("splitk-a-512-off", "f16x2", E(PACKA, CAPDEC_SPLITK=0), (512, 768, 768), H2P, 24)
# ---------------------------------------------------------------- ping-pong kernels, planner-chosen and forced
case("pp10-plan-3125", "f16x2", PACKA, (3125, 768, 3072), PP10_SK, 78 * 3, 512, S=3)
family("pp10-plan-2100", "f16x2", PACKA, (2100, 768, 768), PP10_SK, 54 * 4, 512, S=4)
case("pp10-plan-640", "f16x2", PACKA, (640, 768, 3072), PP10_SK, 18 * 12, 512, S=12)
case("pp14-plan-unsplit", "f16x2", CACHE, (3125, 3072, 768), PP14, 208, 512)              # 13 x 16 tiles of 256 x 192
case("pp14-plan-split", "f16x2", CACHE, (1500, 2304, 768), PP14_SK, 72 * 3, 512, S=3)
family("pp10-forced-persist", "f16x2", E(PACKA, CAPDEC_H2W=10), (3125, 3072, 768), PP10, 256, 512)    # 312 tiles on 256 blocks
family("pp14-forced-persist", "f16x2", E(PACKA, CAPDEC_H2W=14), (5000, 3072, 768), PP14, 256, 512)    # 320 tiles on 256 blocks
family("pp14-forced-split", "f16x2", E(PACKA, CAPDEC_H2W=14), (3125, 768, 768), PP14_SK, 52 * 4, 512, S=4)
case("pp-off", "f16x2", E(PACKA, CAPDEC_PP=0), (3125, 768, 3072), H2P_SK, 150 * 3, S=3)
# ---------------------------------------------------------------- single-accumulator wide tiles
case("h2w8-plan", "f16x2", CACHE, (8192, 768, 768), W8, 256)                               # 64 x 4 tiles of 128 x 192
family("h2w2-forced-persist", "f16x2", E(PACKA, CAPDEC_H2W=2), (6000, 3072, 768), W2, 512)  # 576 tiles on 512 blocks
family("h2w8-forced-persist", "f16x2", E(PACKA, CAPDEC_H2W=8), (3125, 6144, 768), W8, 512)  # 800 tiles on 512 blocks
# ---------------------------------------------------------------- one-plane split-K (the hook takes gemm_packed's decision)
for mode in ("bf16", "f16"):
    family(f"x1-splitk-a-{mode}", mode, PACKA, (333, 1024, 768), X1_SK(mode), 24 * 6, S=6, epilogues=mode == "bf16")
    case(f"x1-splitk-b-{mode}", mode, PACKA, (3125, 768, 3072), X1_SK(mode), 150 * 3, S=3)
    off = E(PACKA, CAPDEC_X1_SPLITK=0)
    case(f"x1-splitk-a-{mode}-off", mode, off, (333, 1024, 768), X1(mode), 24)
    case(f"x1-splitk-b-{mode}-off", mode, off, (3125, 768, 3072), X1(mode), 150)
    # without the flag (the existing bf16 hook tests, the micro-benchmarks) the hook never splits them
    family(f"x1-hook-default-{mode}", mode, {}, (333, 1024, 768), X1(mode), 24, epilogues=mode == "f16")
# ---------------------------------------------------------------- three-plane kernels, native fp32
family("x3p-unsplit", "bf16x3", PACKA, (3125, 3072, 768), X3P, 600)
family("x3-unpacked-a", "bf16x3", {}, (300, 1531, 768), X3, 36)
case("x3-unpacked-a-small", "bf16x3", {}, (5, 130, 64), X3, 2)
for mode in ("f16x2", "bf16x3", "f32", "bf16", "f16"):                                     # K % 64 != 0: native fp32 in every mode
    family(f"f32-k96-{mode}", mode, {}, (257, 333, 96), F32, 9, epilogues=mode == "f32")
    case(f"f32-k32-{mode}", mode, {}, (1, 8, 32), F32, 1)
case("f32-mode-k768", "f32", {}, (300, 1531, 768), F32, 36)
case("f32-mode-bk16", "f32", {}, (77, 768, 3072), F32_BK16, 6)
# ---------------------------------------------------------------- tile edges: a tile multiple, one below, one above, M = 1
UNSPLIT = E(PACKA, CAPDEC_SPLITK=0, CAPDEC_H2W=0)
for M, N in ((1, 128), (127, 129), (128, 128), (129, 127), (129, 132), (128, 124)):
    v4 = N % 4 == 0
    case(f"edge-h2p-{M}x{N}", "f16x2", UNSPLIT, (M, N, 128), H2P if v4 else H2P_SC, tiles(M, N))
    case(f"edge-x1-{M}x{N}", "bf16", {}, (M, N, 128), X1("bf16", v4), tiles(M, N))
    case(f"edge-x3p-{M}x{N}", "bf16x3", UNSPLIT, (M, N, 128), X3P if v4 else X3P_SC, tiles(M, N))
    case(f"edge-x3-{M}x{N}", "bf16x3", {}, (M, N, 128), X3, tiles(M, N))
    case(f"edge-f32-{M}x{N}", "f32", {}, (M, N, 128), F32, tiles(M, N))
for M, N in ((1, 124), (127, 128), (129, 132)):                                            # K = 256: S = 2 in regime (a)
    case(f"edge-h2p-splitk-{M}x{N}", "f16x2", E(PACKA, CAPDEC_H2W=0), (M, N, 256), H2P_SK, tiles(M, N) * 2, S=2)
    case(f"edge-x3p-splitk-{M}x{N}", "bf16x3", PACKA, (M, N, 256), X3P_SK, tiles(M, N) * 2, S=2)
    case(f"edge-x1-splitk-{M}x{N}", "bf16", PACKA, (M, N, 768), X1_SK("bf16"), tiles(M, N) * 6, S=6)
for M, N in ((1, 128), (255, 124), (256, 128), (257, 132)):                                # M <= 512: a forced geometry runs unsplit
    case(f"edge-pp10-{M}x{N}", "f16x2", E(PACKA, CAPDEC_H2W=10), (M, N, 128), PP10, tiles(M, N, 256, 128), 512)
    case(f"edge-h2w2-{M}x{N}", "f16x2", E(PACKA, CAPDEC_H2W=2, CAPDEC_SPLITK=0), (M, N, 128), W2, tiles(M, N, 256, 128))
for M, N in ((1, 192), (255, 188), (256, 192), (257, 196)):
    case(f"edge-pp14-{M}x{N}", "f16x2", E(PACKA, CAPDEC_H2W=14), (M, N, 128), PP14, tiles(M, N, 256, 192), 512)
for M, N in ((1, 192), (127, 188), (128, 192), (129, 196)):
    case(f"edge-h2w8-{M}x{N}", "f16x2", E(PACKA, CAPDEC_H2W=8, CAPDEC_SPLITK=0), (M, N, 128), W8, tiles(M, N, 128, 192))
for N in (191, 193):          # the wide tiles need the float4 epilogue: a forced geometry at N % 4 != 0 keeps the 128 x 128 kernel
    case(f"edge-h2w8-scalar-129x{N}", "f16x2", E(PACKA, CAPDEC_H2W=8), (129, N, 128), H2P_SC, tiles(129, N))
    case(f"edge-pp14-scalar-257x{N}", "f16x2", E(PACKA, CAPDEC_H2W=14), (257, N, 128), H2P_SC, tiles(257, N))
# ---------------------------------------------------------------- ring wrap: one stage, a few, many (ring depths 3..5)
for K in (64, 320, 3072):
    s = {64: 1, 320: 2, 3072: 24}[K]                                                       # regime (a): S depends on K only
    case(f"ring-h2p-k{K}", "f16x2", UNSPLIT, (129, 132, K), H2P, 4)
    case(f"ring-x3p-k{K}", "bf16x3", UNSPLIT, (129, 132, K), X3P, 4)
    case(f"ring-x1-k{K}", "bf16", {}, (129, 132, K), X1("bf16"), 4)
    case(f"ring-x3-k{K}", "bf16x3", {}, (129, 132, K), X3, 4)
    case(f"ring-pp10-k{K}", "f16x2", E(PACKA, CAPDEC_H2W=10), (257, 132, K), PP10, 4, 512)
    case(f"ring-pp14-k{K}", "f16x2", E(PACKA, CAPDEC_H2W=14), (257, 196, K), PP14, 4, 512)
    case(f"ring-h2w2-k{K}", "f16x2", E(PACKA, CAPDEC_H2W=2, CAPDEC_SPLITK=0), (257, 132, K), W2, 4)
    case(f"ring-h2w8-k{K}", "f16x2", E(PACKA, CAPDEC_H2W=8, CAPDEC_SPLITK=0), (129, 196, K), W8, 4)
    if s > 1:
        case(f"ring-h2p-splitk-k{K}", "f16x2", E(PACKA, CAPDEC_H2W=0), (129, 132, K), H2P_SK, 4 * s, S=s)
        case(f"ring-x3p-splitk-k{K}", "bf16x3", PACKA, (129, 132, K), X3P_SK, 4 * s, S=s)
case("ring-x1-splitk-k3072", "bf16", PACKA, (129, 132, 3072), X1_SK("bf16"), 4 * 24, S=24)
case("ring-x1-splitk-k320-none", "bf16", PACKA, (129, 132, 320), X1("bf16"), 4)      # 10 k-steps per slice: not whole stage pairs
# ---------------------------------------------------------------- strides and aliasing, as the product call sites pass them
SH = (333, 1024, 256)
for tag, mode, env, kern, blocks, S in (("h2-default", "f16x2", {}, H2P_SK, 48, 2),                  # Engine.gemm's usual path
                                        ("h2-default-unsplit", "f16x2", {"CAPDEC_SPLITK": "0"}, H2P, 24, 1),
                                        ("bf16", "bf16", {}, X1("bf16"), 24, 1),
                                        ("f32", "f32", {}, F32, 24, 1)):
    lda = 2 * SH[2] + 4
    # (a row-strided A leaves the hook's packed path, which needs lda == K: the one-plane modes then take the f16x2 route of gemm())
    k_lda, b_lda, s_lda = (H2P_SK, 48, 2) if mode == "bf16" else (kern, blocks, S)
    family(f"stride-{tag}", mode, env, SH, kern, blocks, S=S, epilogues=tag == "h2-default")
    case(f"stride-{tag}-lda", mode, env, SH, k_lda, b_lda, S=s_lda, lda=lda)
    case(f"stride-{tag}-ldc", mode, env, SH, kern, blocks, S=S, ldc=SH[1] + 12)
    case(f"stride-{tag}-all", mode, env, SH, k_lda, b_lda, S=s_lda, bias=True, act=3, resid="sep", lda=lda, ldc=SH[1] + 12, ldr=SH[1] + 4)
    case(f"stride-{tag}-alias", mode, env, SH, kern, blocks, S=S, bias=True, resid="alias")
    case(f"stride-{tag}-alias-ldc", mode, env, SH, kern, blocks, S=S, bias=True, act=3, resid="alias", ldc=SH[1] + 12)
for tag, env, kern, blocks, wg, S, shape in (("packa-splitk", PACKA, H2P_SK, 48, 256, 2, SH),
                                             ("packa-persist", PACKA, H2P, 512, 256, 1, (3125, 3072, 768)),
                                             ("packa-pp10", PACKA, PP10_SK, 216, 512, 4, (2100, 768, 768)),
                                             ("packa-pp14", E(PACKA, CAPDEC_H2W=14), PP14, 256, 512, 1, (5000, 3072, 768)),
                                             ("packa-h2w8", E(PACKA, CAPDEC_H2W=8), W8, 512, 256, 1, (3125, 6144, 768))):
    N = shape[1]
    case(f"stride-{tag}-ldc", "f16x2", env, shape, kern, blocks, wg, S=S, bias=True, act=3, resid="sep", ldc=N + 12, ldr=N + 4)
    case(f"stride-{tag}-alias-ldc", "f16x2", env, shape, kern, blocks, wg, S=S, bias=True, resid="alias", ldc=N + 12)
# (ldr % 4 != 0: the residual cannot be read as float4 -> the scalar epilogue, unsplit)
case("stride-packa-ldr-odd", "f16x2", PACKA, SH, H2P_SC, 24, bias=True, act=1, resid="sep", ldr=SH[1] + 3)

CASES.sort(key=lambda c: (c.M, c.N, c.K))          # (stable) cases of one shape together: each fp64 reference is computed once
assert len({c.id for c in CASES}) == len(CASES)
SINGLE = ("bf16", "f16")
SENTINEL = -1234.5


# ------------------------------------------------------------------------------------------------ operands, references
class _Shape:
    """operands of one (M, N, K) and their fp64 products (lazily, per rounding of the operands)"""

    def __init__(self, M, N, K):
        # (B and the bias depend on (N, K) only and A is drawn after them, so shapes that differ in M alone -- 512 / 513 rows
        #  on the two sides of the split-K regime boundary -- share B and the leading rows of A)
        g = torch.Generator().manual_seed(N * 31 + K)
        self.bt = torch.randn(N, K, generator=g) * 0.2          # (|bt| < 16: the single-accumulator tiles are allowed)
        self.bias = torch.randn(N, generator=g)
        self.a = torch.randn(M, K, generator=g)                 # asymmetric operands: a transposed result cannot pass
        self.resid = torch.randn(M, N, generator=torch.Generator().manual_seed(M * 7919 + N))
        self._ref = {}

    def ref(self, rounding=None):
        if rounding not in self._ref:
            a, bt = self.a, self.bt
            if rounding == "bf16":
                a, bt = a.bfloat16(), bt.bfloat16()
            elif rounding == "f16":
                a, bt = a.half(), bt.half()
            a, bt = a.double(), bt.double()
            self._ref[rounding] = (a @ bt.t(), a.abs() @ bt.abs().t())
        return self._ref[rounding]


_shapes = collections.OrderedDict()


def _shape(M, N, K):
    key = (M, N, K)
    if key not in _shapes:
        while len(_shapes) >= 2:
            _shapes.popitem(last=False)
        _shapes[key] = _Shape(M, N, K)
    _shapes.move_to_end(key)
    return _shapes[key]


def _gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def _set_env(c, setenv, delenv):
    for k in KNOBS:
        delenv(k)
    for k, v in c.env.items():
        setenv(k, v)


def _launch(c, a, bt, bias, resid):
    """one hook call of case ``c`` in a fresh Engine on device operands; returns (out view, whole output allocation).
    Every operand stays alive until the engine is closed (CAPDEC_HOOK_CACHE keys its planes by device address)."""
    from capdec_amd.engine import Engine
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    try:
        eng.set_gemm_mode(c.mode)
        a_d = a.to(dev)
        if c.lda:
            wide = torch.full((c.M, c.lda), 777.0, device=dev)         # what a wrong row stride would read
            wide[:, :c.K] = a_d
            a_d = wide[:, :c.K]
        bt_d = bt.to(dev)
        ldc = c.ldc or c.N
        big = torch.full((c.M + 3, ldc), SENTINEL, device=dev)
        out = big[:c.M, :c.N]
        r_d = None
        if c.resid == "alias":
            out.copy_(resid.to(dev))
            r_d = out
        elif c.resid == "sep":
            r_d = resid.to(dev)
            if c.ldr:
                rw = torch.full((c.M, c.ldr), 555.0, device=dev)
                rw[:, :c.N] = r_d
                r_d = rw[:, :c.N]
        got = eng.gemm(a_d, bt_d, bias=bias.to(dev) if c.bias else None, resid=r_d, act=c.act, out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        keep = (a_d, bt_d, r_d)       # noqa: F841
    finally:
        eng.close()
    return out, big


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_gemm_plan_case(c, monkeypatch):
    _set_env(c, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    sh = _shape(c.M, c.N, c.K)
    out, big = _launch(c, sh.a, sh.bt, sh.bias, sh.resid)
    big = big.cpu()
    got = big[:c.M, :c.N]
    # the padding columns and the rows past M are untouched, bit for bit
    sent = torch.tensor(SENTINEL).view(torch.int32)
    assert bool((big[c.M:].view(torch.int32) == sent).all()), "rows past M were written"
    assert bool((big[:c.M, c.N:].view(torch.int32) == sent).all()), "padding columns were written"
    # which operand rounding the launch computes with: the one-plane modes round both operands -- but only on the hook's
    # packed path (lda == K, K % 64 == 0); elsewhere they take the fp32-accurate route of gemm()
    single = c.mode in SINGLE and not c.lda and c.K % 64 == 0
    ref, scale = sh.ref(c.mode if single else None)
    plain = not c.bias and c.act == 0 and c.resid is None
    if plain:
        ratio = float(((got.double() - ref).abs() / scale).max())
        print(f"[gemm plan] {c.id}: {c.kernel[0]}{list(c.kernel[1])} max |err| / sum|a||b| = {ratio:.3e} (bound 5e-7)")
        assert ratio < 5e-7, (c.id, ratio)
        if single:
            away = float(((got.double() - sh.ref(None)[0]).abs() / scale).max())
            print(f"[gemm plan] {c.id}: distance from the unrounded product {away:.3e} (must exceed 1e-5)")
            assert away > 1e-5, (c.id, away)
        return
    y = ref + sh.bias.double() if c.bias else ref.clone()
    y = [y, torch.tanh(y), torch.relu(y), _gelu_new(y)][c.act]
    if c.resid:
        y = y + sh.resid.double()
    y = y.float()
    err = (got - y).abs()
    atol = 3e-5 if single else 2e-5
    worst = float((err - 1e-5 * y.abs()).max())
    print(f"[gemm plan] {c.id}: {c.kernel[0]}{list(c.kernel[1])} max (|err| - rtol |y|) = {worst:.3e} (atol {atol:g})")
    np.testing.assert_allclose(got.numpy(), y.numpy(), atol=atol, rtol=1e-5, err_msg=c.id)


def test_engine_gemm_rejects_bad_out():
    from capdec_amd.engine import Engine
    from capdec_amd._capi import CapdecError
    eng = Engine(0)
    a, bt = torch.randn(4, 64), torch.randn(8, 64)
    with pytest.raises(CapdecError):
        eng.gemm(a, bt, out=torch.empty(4, 9, device="cuda:0"))
    with pytest.raises(CapdecError):
        eng.gemm(a, bt, out=torch.empty(8, 4, device="cuda:0").t())
    eng.close()


# ------------------------------------------------------------------------------------------------ GPT-2 block stack
LN_DIMS = dict(n_layer=2, vocab=1531, n_pos=256)
LN_ROWS = ((16, 77), (15, 77))       # 1232 rows; 1155 rows (not a multiple of the reduce kernel's four rows per block)


def _logits(env, sd, x, mode=None):
    from capdec_amd.engine import Engine
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        eng = Engine(0)
        if mode:
            eng.set_gemm_mode(mode)
        eng.load_gpt2(sd)
        got = eng.gpt2_logits(x, all_positions=True).cpu()
        eng.close()
    finally:
        for k in env:
            os.environ.pop(k, None)
    return got


def _ln_inputs(n, L):
    from capdec_amd import synth
    dims = synth.GPT2Dims(**LN_DIMS)
    sd = synth.hot_gpt2_state_dict(42, dims)
    x = torch.randn(n, L, dims.n_embd, generator=torch.Generator().manual_seed(100 + n)) * 0.6
    return dims, sd, x


@pytest.fixture
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("n,L", LN_ROWS, ids=[f"{n}x{L}" for n, L in LN_ROWS])
def test_fused_splitk_layernorm_reduce_vs_oracle_and_unfused(n, L, clean_env):
    """splitk_reduce_ln_kernel (split-K reduce + bias + residual + the NEXT LayerNorm, from 1024 rows) where it lives:
    capdec_gpt2_logits on >= 1024 rows, every position against the oracle (3e-4 abs, the bound of
    test_gpt2_logits_every_prefill_attention_form_vs_oracle).  At 1232 rows attn.c_proj splits S = 3 on the 128 x 128
    split kernel and mlp.c_proj S = 8 on the ping-pong split kernel, both into the fused reduce (the trace test checks
    it).  CAPDEC_FUSE_LN=0 -- splitk_reduce_kernel, then layernorm_packed_kernel -- must give the same logits BIT FOR BIT:
    the fused kernel's comment claims the LayerNorm of layernorm_packed_kernel."""
    from oracle import capdec_oracle as O
    dims, sd, x = _ln_inputs(n, L)
    want = O.gpt2_logits(x, sd, dims.n_head)
    fused = _logits({}, sd, x)
    unfused = _logits({"CAPDEC_FUSE_LN": "0"}, sd, x)
    print(f"[fused ln] {n} x {L}: fused vs oracle {float((fused - want).abs().max()):.3e}, unfused vs oracle "
          f"{float((unfused - want).abs().max()):.3e}, fused vs unfused {float((fused - unfused).abs().max()):.3e}")
    np.testing.assert_allclose(fused.numpy(), want.numpy(), atol=3e-4)
    np.testing.assert_allclose(unfused.numpy(), want.numpy(), atol=3e-4)
    np.testing.assert_array_equal(fused.numpy(), unfused.numpy())


@pytest.mark.parametrize("knob,mode", [("CAPDEC_X3_PACKA", "bf16x3"), ("CAPDEC_X3_CHAIN", "f16x2"), ("CAPDEC_X3_CHAIN", "bf16x3")])
def test_block_stack_knobs_vs_oracle(knob, mode, clean_env):
    """CAPDEC_X3_PACKA=0 (bf16x3 mode: LayerNorm writes fp32, the GEMM splits A itself) and CAPDEC_X3_CHAIN=0 (attention and
    the fc epilogue write fp32 instead of packed operands): the same 1232 rows against the oracle at the same bound"""
    from oracle import capdec_oracle as O
    n, L = LN_ROWS[0]
    dims, sd, x = _ln_inputs(n, L)
    want = O.gpt2_logits(x, sd, dims.n_head)
    got = _logits({knob: "0"}, sd, x, mode)
    print(f"[block stack knob] {knob}=0, {mode}: max |err| {float((got - want).abs().max()):.3e} (bound 3e-4)")
    np.testing.assert_allclose(got.numpy(), want.numpy(), atol=3e-4)


# ------------------------------------------------------------------------------------------------ what was launched
def kernel_signature(name):
    """(kernel, template arguments as integers) of a traced GEMM / split-K reduce launch, from the mangled or the demangled
    name; None for every other kernel"""
    m = re.search(r"(gemm_[a-z0-9_]*?kernel|splitk_reduce(?:_ln)?_kernel)", name)
    if not m or "pack" in m.group(1):
        return None
    rest = name[m.end():]
    if name.lstrip().startswith("_Z"):
        args = tuple(int(v) for v in re.findall(r"L[a-z](\d+)E", rest))
    else:
        args = tuple({"true": 1, "false": 0}.get(v) if v in ("true", "false") else int(v)
                     for v in re.findall(r"\b(\d+|true|false)\b", rest))
    return m.group(1), args


def _read_kernel_trace(src):
    spec = importlib.util.spec_from_file_location("capdec_trace_summary", os.path.join(ROOT, "tools", "trace_summary.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.read_kernel_trace(src)


def launches_by_gemm(rows):
    """the traced launches as one group per GEMM launch, in order: (kernel, args, blocks, workgroup, [reduce kernels that
    followed it])"""
    groups = []
    for _, _, name, grid, wg in rows:
        sig = kernel_signature(name)
        if sig is None:
            continue
        if sig[0].startswith("splitk_reduce"):
            assert groups, "a split-K reduce before any GEMM launch"
            groups[-1][4].append(sig[0])
            continue
        threads, wgs = int(str(grid).split("x")[0]), int(str(wg).split("x")[0])
        groups.append((sig[0], sig[1], threads // wgs, wgs, []))
    return groups


def _script(argv):
    return [sys.executable, os.path.abspath(__file__)] + argv


def test_kernel_signature_reads_both_name_forms():
    assert kernel_signature("_ZN6capdec21gemm_pp_splitk_kernelINS_4PGeoILi4ELi2ELi2ELi2ELi5ELb1EEEEEvPKDF16_S4_Pfiiiiiif") == PP10_SK
    assert kernel_signature("void capdec::gemm_pp_splitk_kernel<capdec::PGeo<4, 2, 2, 2, 5, true> >") == PP10_SK
    assert kernel_signature("_ZN6capdec18gemm_f16x2p_kernelILb1ELi4EEEvPKDF16_S2_PfiiiiPKfS5_iiiiPcNS_10QkvScatterE") == H2P
    assert kernel_signature("_ZN6capdec15gemm_h2w_kernelINS_4WGeoILi2ELi2ELi2ELi3ELi4ELi2EEEEEvPKDF16_S4_PfiiiiPKfS7_iiiiPcf") == W8
    assert kernel_signature("_ZN6capdec18gemm_bf16x3_kernelEPKfiPKDF16bPfiiiiS1_S1_iiii") == X3          # not a template: no arguments
    assert kernel_signature("capdec::gemm_bf16x3_kernel(float const*, int, __bf16 const*, float*, int, int, int, int)") == X3
    assert kernel_signature("capdec::splitk_reduce_ln_kernel") == ("splitk_reduce_ln_kernel", ())
    assert kernel_signature("capdec::pack_planes_h2_kernel") is None


def test_cases_run_the_kernels_they_claim(tmp_path, clean_env):
    """this file as a script -- every case once, in table order, then the two logits runs of the fused-reduce test -- in
    a fresh child process under rocprofv3 --kernel-trace (nothing else traced); the i-th GEMM launch of the trace belongs
    to the i-th case.  Per case: kernel name and template geometry, grid = claimed blocks x workgroup size, a
    splitk_reduce launch present exactly for the split rows."""
    exe = shutil.which("rocprofv3") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "rocprofv3")
    assert os.path.exists(exe), "rocprofv3 not found: the launched kernels cannot be observed (this test does not skip)"
    t0 = time.time()
    r = subprocess.run(_script(["--run-all"]), capture_output=True, text=True, timeout=1200)
    untraced = time.time() - t0
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    limit = int(120 + 5 * untraced)
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit), exe, "--kernel-trace", "--output-format", "csv", "-d", str(tmp_path),
                        "--"] + _script(["--run-all"]), capture_output=True, text=True)
    print(f"[gemm plan trace] {len(CASES)} cases: {untraced:.1f} s untraced, {time.time() - t0:.1f} s under rocprofv3")
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    groups = launches_by_gemm(_read_kernel_trace(str(tmp_path)))
    assert len(groups) >= len(CASES), f"{len(groups)} GEMM launches traced for {len(CASES)} cases"
    bad, reached = [], collections.Counter()
    for c, (kern, args, blocks, wg, reduces) in zip(CASES, groups):
        claimed = (c.kernel[0], c.kernel[1], c.blocks, c.wg, ["splitk_reduce_kernel"] if c.S > 1 else [])
        seen = (kern, args, blocks, wg, reduces)
        reached[kern + (str(list(args)) if args else "")] += 1
        if claimed != seen:
            bad.append(f"{c.id} [{c.mode} {c.env} {(c.M, c.N, c.K)}]: claimed {claimed}, observed {seen}")
    for k, v in sorted(reached.items()):
        print(f"[gemm plan trace] {v:4d} cases reached {k}")
    assert not bad, "\n".join(bad)
    # the logits runs: 1232 rows, default, then CAPDEC_FUSE_LN=0
    tail = groups[len(CASES):]
    assert len(tail) % 2 == 0 and tail, len(tail)
    fused, unfused = tail[:len(tail) // 2], tail[len(tail) // 2:]
    assert [g[:4] for g in fused] == [g[:4] for g in unfused], "CAPDEC_FUSE_LN changed a GEMM launch"
    rows = LN_ROWS[0][0] * LN_ROWS[0][1]
    want = {H2P_SK + (tiles(rows, 768) * 3, 256), PP10_SK + (tiles(rows, 768, 256, 128) * 8, 512)}
    into_ln = [g for g in fused if g[4] == ["splitk_reduce_ln_kernel"]]
    assert {g[:4] for g in into_ln} == want, into_ln
    assert all(g[4] in ([], ["splitk_reduce_kernel"]) for g in fused if g not in into_ln), fused
    assert all(g[4] == (["splitk_reduce_kernel"] if f[4] else []) for g, f in zip(unfused, fused)), unfused


def _run_all():
    """script mode: every case once in table order (operands drawn on the host once per shape, no references), then the
    logits runs; prints one line per case"""
    cur = None
    for c in CASES:
        _set_env(c, os.environ.__setitem__, lambda k: os.environ.pop(k, None))
        if cur is None or cur[0] != (c.M, c.N, c.K):
            g = torch.Generator().manual_seed(1)
            cur = ((c.M, c.N, c.K), torch.randn(c.M, c.K, generator=g), torch.randn(c.N, c.K, generator=g) * 0.2,
                   torch.randn(c.N, generator=g), torch.randn(c.M, c.N, generator=g))
        _launch(c, *cur[1:])
        print("ran", c.id, flush=True)
    n, L = LN_ROWS[0]
    _, sd, x = _ln_inputs(n, L)
    for env in ({}, {"CAPDEC_FUSE_LN": "0"}):
        _logits(env, sd, x)
        print("ran logits", env, flush=True)


if __name__ == "__main__":
    if sys.argv[1:] == ["--run-all"]:
        _run_all()
    elif sys.argv[1:] == ["--list"]:
        for c in CASES:
            print(c.id, c.mode, c.env, (c.M, c.N, c.K), c.kernel, c.blocks, c.wg, c.S)
    else:
        sys.exit("usage: test_hip_gemm_plans.py --run-all | --list")
