"""The weight-gradient product of the train step, ``gemm_tn`` (csrc/gemm_dispatch.hip: dW = dY^T X, both operands through the
transposing packer, K = the token rows padded to 64), at every plan it reaches -- element by element against fp64.

CASES is a table: rows, (N1, N2), row strides -- and the kernel, template geometry, slice count, block count and workgroup
size the case CLAIMS to reach.  ``test_cases_get_the_plans_they_claim`` (no GPU) checks each claim against the host planner
(gemm_plan.h) fed as gemm_tn feeds it; ``test_gemm_tn_case`` runs each case through the ``capdec_gemm_tn_f32`` hook
(``Engine.gemm_tn``) in a fresh Engine, with NaN around the operands and a sentinel around the output, and compares ALL
elements with the fp64 product; ``test_cases_run_the_kernels_they_claim`` runs this file as a script in a child process
under ``rocprofv3 --kernel-trace`` and matches the i-th GEMM launch against the i-th claim.

The two cases at 2720 rows run the K (2752) of the benchmark's mapper; the others sit on the smallest K that reaches their
plan.  Bound (the project's existing one for a plain product in the fp32-accurate modes, tests/test_hip_gemm_plans.py):
|out - ref| / (|Xa|^T . |Xb|) < 5e-7."""
import collections
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pytest
import torch

from tests import test_gemm_plan as GP
from tests import test_hip_gemm_plans as T
from tests.test_gemm_plan import planner                      # noqa: F401  (the fixture: the planner program, built once)
from tests.test_hip_gemm_plans import kernel_signature, launches_by_gemm, _read_kernel_trace      # noqa: F401

H2P, H2P_SK, PP10_SK = T.H2P, T.H2P_SK, T.PP10_SK
SENTINEL = T.SENTINEL
BOUND = 5e-7

Case = collections.namedtuple("Case", "id rows N1 N2 lda ldb ldc invariant kernel S blocks wg")
CASES = []


def case(id, rows, shape, kernel, S, blocks, wg=256, lda=0, ldb=0, ldc=0, invariant=False):
    """lda / ldb / ldc: 0 = dense (N1 / N2 / N2)"""
    N1, N2 = shape
    CASES.append(Case(id, rows, N1, N2, lda or N1, ldb or N2, ldc or N2, invariant, kernel, S, blocks, wg))


# ---- 768 x 768 (attn.c_proj, the mapper's project) from the last unsplit K up to the benchmark's
case("below-split", 448, (768, 768), H2P, 1, 36)
case("first-split", 449, (768, 768), H2P_SK, 2, 72)                        # K 512
case("ldc", 512, (768, 768), H2P_SK, 2, 72, ldc=780)
case("ld-odd", 512, (768, 768), H2P_SK, 2, 72, lda=771, ldb=773)           # the packer reads single floats: any row stride
case("invariant", 512, (768, 768), H2P, 1, 36, invariant=True)
case("s3", 768, (768, 768), H2P_SK, 3, 108)
case("pp-s11", 1408, (768, 768), PP10_SK, 11, 198, 512)
case("pp-s14", 1792, (768, 768), PP10_SK, 14, 252, 512)
case("s8", 2040, (768, 768), H2P_SK, 8, 288)                               # K 2048: the benchmark's GPT-2 rows
case("s10", 2560, (768, 768), H2P_SK, 10, 360)
case("bench-proj", 2720, (768, 768), H2P_SK, 2, 72)                        # K 2752: the benchmark's mapper rows
# ---- the other weight shapes of the train step
case("bench-qkv", 2720, (2304, 768), PP10_SK, 4, 216, 512)                 # 43 k-steps per slice
case("qkv-first", 512, (2304, 768), PP10_SK, 4, 216, 512)
case("fc-pp", 330, (3072, 768), PP10_SK, 3, 216, 512)                      # K 384
case("fc-s2", 512, (3072, 768), H2P_SK, 2, 288)
case("mlpproj-s3", 768, (768, 3072), H2P_SK, 3, 432)
case("kv-pp7", 896, (1536, 768), PP10_SK, 7, 252, 512)
case("fc2-s7", 1792, (768, 1536), H2P_SK, 7, 504)
case("wte-tiny", 600, (1531, 768), H2P_SK, 2, 144, lda=1536)               # K 640; N1 % 128 != 0
case("wte", 300, (50257, 768), H2P, 1, 2358, lda=50304)                    # K 320; one block per tile
case("lin640", 34, (30720, 640), H2P, 1, 512)                              # K 64; persistent blocks

assert len({c.id for c in CASES}) == len(CASES)


def ceil64(n):
    return (n + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------ the planner, no GPU
def planner_input(c):
    """what gemm_tn hands to launch_packed and launch_packed to gemm_plan() -- restated ONLY here: two fp16 planes, M = N1,
    N = N2, K = the rows padded to 64, a bare epilogue (float4 stores on aligned rows, wide_ok unset), split allowed unless
    the context is batch-invariant"""
    return dict(fmt=GP.FMT["f16x2"], M=c.N1, N=c.N2, K=ceil64(c.rows), vec4=int(c.N2 % 4 == 0 and c.ldc % 4 == 0), wide_ok=0,
                invariant=int(c.invariant), split_ok=int(not c.invariant), packed_out=0, resid_packed=0, scatter=0)


def test_cases_get_the_plans_they_claim(planner):              # noqa: F811
    plans = planner([planner_input(c) for c in CASES])
    bad = []
    for c, p in zip(CASES, plans):
        claimed = (c.kernel, c.S, c.blocks, c.wg)
        got = (GP.planned_kernel(T, "f16x2", p), p["S"], p["grid"], p["threads"])
        if claimed != got:
            bad.append(f"{c.id}: claimed {claimed}, planned {got}")
        assert p["ws_bytes"] == (c.S * c.N1 * c.N2 * 4 if c.S > 1 else 0), (c.id, p)
    assert not bad, "\n".join(bad)
    # what the table is for: both split kernels, an odd slice length, ping-pong slice counts above 8, K % 256 != 0
    kinds = {c.kernel[0] for c in CASES}
    assert kinds == {"gemm_f16x2p_kernel", "gemm_f16x2p_splitk_kernel", "gemm_pp_splitk_kernel"}
    by_id = {c.id: c for c in CASES}
    assert ceil64(by_id["bench-qkv"].rows) // 16 // by_id["bench-qkv"].S == 43
    assert max(c.S for c in CASES if c.kernel == PP10_SK) > 8
    assert any(ceil64(c.rows) % 256 for c in CASES if c.S > 1)


# ------------------------------------------------------------------------------------------------ operands, references
class _Operands:
    """Xa [rows, N1] = randn, Xb [rows, N2] = 0.2 randn (asymmetric: a transposed result cannot pass), drawn on the host,
    and -- lazily, once -- the fp64 product Xa^T Xb with its scale |Xa|^T |Xb|"""

    def __init__(self, rows, N1, N2):
        g = torch.Generator().manual_seed(rows * 7919 + N1 * 31 + N2)
        self.xa = torch.randn(rows, N1, generator=g)
        self.xb = torch.randn(rows, N2, generator=g) * 0.2
        self._ref = None

    def ref(self):
        if self._ref is None:
            a, b = self.xa.double(), self.xb.double()
            self._ref = (a.t() @ b, a.abs().t() @ b.abs())
        return self._ref


_operands = collections.OrderedDict()


def _ops(c):
    key = (c.rows, c.N1, c.N2)
    if key not in _operands:
        while len(_operands) >= 2:
            _operands.popitem(last=False)
        _operands[key] = _Operands(*key)
    _operands.move_to_end(key)
    return _operands[key]


def _launch(c, xa, xb):
    """one hook call of case ``c`` in a fresh Engine; returns the whole output allocation [N1 + 3, ldc] on the host.
    The operands sit in the leading [rows, N] block of [rows + 3, ld] allocations filled with NaN: a read past ``rows`` or
    past the N1 / N2 columns of a wider row turns the output NaN."""
    from capdec_amd.engine import Engine
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    try:
        if c.invariant:
            eng.set_batch_invariant(True)
        a_big = torch.full((c.rows + 3, c.lda), float("nan"), device=dev)
        b_big = torch.full((c.rows + 3, c.ldb), float("nan"), device=dev)
        a_big[:c.rows, :c.N1] = xa.to(dev)
        b_big[:c.rows, :c.N2] = xb.to(dev)
        big = torch.full((c.N1 + 3, c.ldc), SENTINEL, device=dev)
        out = big[:c.N1, :c.N2]
        got = eng.gemm_tn(a_big[:c.rows, :c.N1], b_big[:c.rows, :c.N2], out=out)
        assert got.data_ptr() == out.data_ptr() and got.stride(0) == c.ldc
        torch.cuda.synchronize()
        return big.cpu()
    finally:
        eng.close()


def _report(line):
    from tests.test_hip_parity import _report as report
    report(line)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_gemm_tn_case(c):
    ops = _ops(c)
    big = _launch(c, ops.xa, ops.xb)
    got = big[:c.N1, :c.N2]
    sent = torch.tensor(SENTINEL).view(torch.int32)
    assert bool((big[c.N1:].view(torch.int32) == sent).all()), "rows past N1 were written"
    assert bool((big[:c.N1, c.N2:].view(torch.int32) == sent).all()), "padding columns were written"
    assert bool(torch.isfinite(got).all()), "NaN / inf in the output: something past the operands was read"
    ref, scale = ops.ref()
    ratio = float(((got.double() - ref).abs() / scale).max())
    _report(f"[gemm_tn] {c.id}: rows {c.rows} (K {ceil64(c.rows)}) ({c.N1}, {c.N2}) ld {c.lda}/{c.ldb}/{c.ldc} "
            f"{c.kernel[0]}{list(c.kernel[1])} S {c.S}: max |err| / (|Xa|^T |Xb|) = {ratio:.3e} (bound {BOUND:g})")
    assert ratio < BOUND, (c.id, ratio)


@pytest.mark.gpu
def test_engine_gemm_tn_rejects_bad_arguments():
    from capdec_amd.engine import Engine
    from capdec_amd._capi import CapdecError
    eng = Engine(0)
    try:
        xa, xb = torch.randn(70, 8), torch.randn(70, 12)
        with pytest.raises(CapdecError):
            eng.gemm_tn(xa, torch.randn(69, 12))
        with pytest.raises(CapdecError):
            eng.gemm_tn(xa, xb, out=torch.empty(12, 8, device="cuda:0"))
        with pytest.raises(CapdecError):
            eng.gemm_tn(xa, xb, out=torch.empty(12, 8, device="cuda:0").t())
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ what was launched
@pytest.mark.gpu
def test_cases_run_the_kernels_they_claim(tmp_path):
    """this file as a script -- every case once, in table order -- in ONE fresh child process under rocprofv3 --kernel-trace
    (nothing else traced).  The i-th GEMM launch of the trace belongs to the i-th case: kernel name and template geometry,
    grid = claimed blocks x workgroup size, a splitk_reduce_kernel launch exactly where S > 1.  The time limit of the traced
    run is 120 s + 5 x the untraced run's time (the sizing of tests/test_hip_gemm_plans.py)."""
    exe = shutil.which("rocprofv3") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "rocprofv3")
    assert os.path.exists(exe), "rocprofv3 not found: the launched kernels cannot be observed (this test does not skip)"
    script = [sys.executable, os.path.abspath(__file__), "--run-all"]
    env = {k: v for k, v in os.environ.items() if k not in T.KNOBS}
    t0 = time.time()
    r = subprocess.run(script, capture_output=True, text=True, timeout=600, env=env)
    untraced = time.time() - t0
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    limit = int(120 + 5 * untraced)
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit), exe, "--kernel-trace", "--output-format", "csv", "-d", str(tmp_path),
                        "--"] + script, capture_output=True, text=True, env=env)
    print(f"[gemm_tn trace] {len(CASES)} cases: {untraced:.1f} s untraced, {time.time() - t0:.1f} s under rocprofv3 "
          f"(limit {limit} s)")
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    groups = launches_by_gemm(_read_kernel_trace(str(tmp_path)))
    assert len(groups) == len(CASES), f"{len(groups)} GEMM launches traced for {len(CASES)} cases"
    bad = []
    for c, (kern, args, blocks, wg, reduces) in zip(CASES, groups):
        claimed = (c.kernel[0], c.kernel[1], c.blocks, c.wg, ["splitk_reduce_kernel"] if c.S > 1 else [])
        seen = (kern, args, blocks, wg, reduces)
        if claimed != seen:
            bad.append(f"{c.id} [rows {c.rows} ({c.N1}, {c.N2})]: claimed {claimed}, observed {seen}")
    assert not bad, "\n".join(bad)


def _run_all():
    """script mode: every case once in table order (operands drawn on the host, no references); one line per case"""
    for c in CASES:
        g = torch.Generator().manual_seed(1)
        _launch(c, torch.randn(c.rows, c.N1, generator=g), torch.randn(c.rows, c.N2, generator=g) * 0.2)
        print("ran", c.id, flush=True)


if __name__ == "__main__":
    if sys.argv[1:] == ["--run-all"]:
        _run_all()
    elif sys.argv[1:] == ["--list"]:
        for c in CASES:
            print(*c)
    else:
        sys.exit("usage: test_gemm_tn.py --run-all | --list")
