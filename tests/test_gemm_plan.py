"""The packed-GEMM launch planner (capdec_amd/csrc/gemm_plan.h) on the host: no GPU needed.

A small stand-alone C++ program around the header reads planner inputs and prints plans.  Checked:
  * every packed-kernel row of CASES in test_hip_gemm_plans.py gets the kernel, template arguments, block count, workgroup
    size and slice count it claims (those claims are checked against a kernel trace on the GPU by that file);
  * invariants of the plan over a grid of shapes, formats and flag combinations under the default Tuning."""
import importlib.util
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "capdec_amd", "csrc")

FMT = {"bf16x3": 0, "f16x2": 1, "bf16": 2, "f16": 3}           # PLAN_* of gemm_plan.h
IN_FIELDS = ("fmt", "M", "N", "K", "vec4", "wide_ok", "invariant", "split_ok", "packed_out", "resid_packed", "scatter",
             "splitk", "splitk_mid", "h2_persist", "h2w", "pp")
OUT_FIELDS = ("kernel", "geo", "bm", "bn", "threads", "ns", "vec4", "S", "grid", "ws_bytes")

MAIN = r"""
#include <cstdio>
#include "gemm_plan.h"
using namespace capdec;
static const char *name(int k) {
    switch (k) {
        case GK_H2P: return "h2p";
        case GK_H2P_SPLITK: return "h2p_splitk";
        case GK_X1: return "x1";
        case GK_X1_SPLITK: return "x1_splitk";
        case GK_X3P: return "x3p";
        case GK_X3P_SPLITK: return "x3p_splitk";
        case GK_H2W: return "h2w";
        case GK_PP: return "pp";
        case GK_PP_SPLITK: return "pp_splitk";
    }
    return "?";
}
int main() {
    int v[16];
    for (;;) {
        for (int i = 0; i < 16; ++i)
            if (scanf("%d", &v[i]) != 1) return i == 0 ? 0 : 1;
        Tuning t;
        t.splitk = v[11]; t.splitk_mid = v[12]; t.h2_persist = v[13]; t.h2w = v[14]; t.pp = v[15];
        GemmPlanIn in;
        in.fmt = v[0]; in.M = v[1]; in.N = v[2]; in.K = v[3];
        in.vec4 = v[4]; in.wide_ok = v[5]; in.invariant = v[6]; in.split_ok = v[7];
        in.packed_out = v[8]; in.resid_packed = v[9]; in.scatter = v[10];
        in.tune = &t;
        const GemmPlan p = gemm_plan(in);
        printf("%s %d %d %d %d %d %d %d %d %zu\n", name(p.kernel), p.geo, p.bm, p.bn, p.threads, p.ns, (int)p.vec4, p.S,
               p.grid, p.ws_bytes);
    }
}
"""


def build_planner(tmp, flags=()):
    src = os.path.join(tmp, "gemm_plan_main.cpp")
    with open(src, "w") as f:
        f.write(MAIN)
    exe = os.path.join(tmp, "gemm_plan_main" + ("_san" if flags else ""))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", *flags, "-I", CSRC, src, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = build_planner(str(tmp_path_factory.mktemp("gemm_plan")))

    def run(inputs):
        """inputs: dicts over IN_FIELDS (missing knobs: the Tuning defaults) -> dicts over OUT_FIELDS, in order"""
        defaults = dict(splitk=1, splitk_mid=1, h2_persist=512, h2w=1, pp=1)
        text = "".join(" ".join(str(int({**defaults, **i}[k])) for k in IN_FIELDS) + "\n" for i in inputs)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(inputs)
        plans = []
        for line in out:
            vals = line.split()
            plans.append(dict(zip(OUT_FIELDS, [vals[0]] + [int(x) for x in vals[1:]])))
        return plans
    return run


def tiles(M, N, bm=128, bn=128):
    return -(-M // bm) * -(-N // bn)


# ------------------------------------------------------------------------------------------------ a. the CASES table
def _cases_module():
    spec = importlib.util.spec_from_file_location("capdec_gemm_plan_cases", os.path.join(ROOT, "tests", "test_hip_gemm_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def hook_input(c):
    """Planner input of a CASES row -- the routing of the capdec_gemm_f32 hook (gemm_dispatch.hip), restated ONLY here.
    None: the row does not reach a packed kernel."""
    env = c.env
    packa, cache = env.get("CAPDEC_HOOK_PACKA") == "1", env.get("CAPDEC_HOOK_CACHE") == "1"
    single = c.mode in ("bf16", "f16")
    h2w = int(env.get("CAPDEC_H2W", 1))
    if c.mode == "f32" or c.K % 64 != 0:
        return None
    if (packa or single) and not c.lda:                    # the hook's packed path: both operands in the mode's format
        fmt = FMT[c.mode]
        split_ok = not single or (packa and env.get("CAPDEC_X1_SPLITK", "1") != "0")
        # max |b| < 16 is known for a cached weight, and measured per call when a geometry is forced
        wide_ok = fmt == FMT["f16x2"] and (cache or h2w >= 2)
    elif c.mode == "f16x2" or single:                      # gemm(): fp32 activations packed as two fp16 planes
        fmt, split_ok, wide_ok = FMT["f16x2"], True, cache
    else:
        return None                                        # bf16x3 mode, fp32 A: the kernel splits A itself
    ldc = c.ldc or c.N
    ldr = {None: 0, "alias": ldc, "sep": c.ldr or c.N}[c.resid]
    vec4 = c.N % 4 == 0 and ldc % 4 == 0 and ldr % 4 == 0      # (torch allocations and their row starts are 16-byte aligned)
    return dict(fmt=fmt, M=c.M, N=c.N, K=c.K, vec4=vec4, wide_ok=wide_ok, invariant=0, split_ok=split_ok, packed_out=0,
                resid_packed=0, scatter=0, splitk=env.get("CAPDEC_SPLITK", "1") != "0",
                splitk_mid=env.get("CAPDEC_SPLITK_MID", "1") != "0", h2_persist=int(env.get("CAPDEC_H2_PERSIST", 512)),
                h2w=h2w, pp=env.get("CAPDEC_PP", "1") != "0")


def planned_kernel(T, mode, p):
    """the (name, template arguments) a plan launches, in the notation of test_hip_gemm_plans.py"""
    k = p["kernel"]
    if k == "h2p":
        return ("gemm_f16x2p_kernel", (p["vec4"], p["ns"]))
    if k == "h2p_splitk":
        return T.H2P_SK
    if k == "x1":
        return ("gemm_x1_kernel", (p["vec4"], T.KIND[mode], p["ns"]))
    if k == "x1_splitk":
        return T.X1_SK(mode)
    if k == "x3p":
        return ("gemm_bf16x3p_kernel", (p["vec4"],))
    if k == "x3p_splitk":
        return T.X3P_SK
    if k == "h2w":                                         # WGeo<WM, WN, TI, TJ, NS, MINW>: 2 x 2 wavefronts of (TI x TJ) x 32 x 32
        return ("gemm_h2w_kernel", (2, 2, p["bm"] // 64, p["bn"] // 64, p["ns"], 2))
    name = "gemm_pp_kernel" if k == "pp" else "gemm_pp_splitk_kernel"      # PGeo<WM, WN, TI, TJ, NS, TWOACC>: 4 x 2 wavefronts
    return (name, (4, 2, p["bm"] // 128, p["bn"] // 64, p["ns"], int(p["geo"] == 10)))


def test_cases_table_gets_the_plans_it_claims(planner):
    T = _cases_module()
    unpacked = (T.X3, T.F32, T.F32_BK16)
    rows = [(c, hook_input(c)) for c in T.CASES]
    for c, i in rows:
        assert (i is None) == (c.kernel in unpacked), c.id
    packed = [(c, i) for c, i in rows if i is not None]
    plans = planner([i for _, i in packed])
    checked, bad = 0, []
    for (c, _), p in zip(packed, plans):
        claimed = (c.kernel, c.blocks, c.wg, c.S)
        got = (planned_kernel(T, c.mode, p), p["grid"], p["threads"], p["S"])
        if claimed != got:
            bad.append(f"{c.id}: claimed {claimed}, planned {got}")
        checked += 1
    assert not bad, "\n".join(bad)
    assert checked == sum(c.kernel not in unpacked for c in T.CASES) and checked > 200, checked


# ------------------------------------------------------------------------------------------------ b. invariants over a grid
GRID_M = (1, 127, 128, 129, 512, 513, 640, 1500, 2100, 3125, 5000, 8191, 8192, 25000)
GRID_N = (124, 128, 192, 768, 1024, 2304, 3072, 50257)
GRID_K = (64, 128, 256, 320, 768, 3072)
FLAGS = ("vec4", "wide_ok", "invariant", "split_ok", "packed_out", "resid_packed", "scatter")


def grid_inputs():
    for fmt, N, K, flags, M in itertools.product(FMT.values(), GRID_N, GRID_K, itertools.product((0, 1), repeat=len(FLAGS)), GRID_M):
        yield dict(fmt=fmt, M=M, N=N, K=K, **dict(zip(FLAGS, flags)))


def test_plan_invariants_over_the_grid(planner):
    inputs = list(grid_inputs())
    plans = planner(inputs)
    small = {}                                   # (fmt, N, K, flags) -> S of every M <= 512
    for i, p in zip(inputs, plans):
        M, N, K, S = i["M"], i["N"], i["K"], p["S"]
        assert p["ws_bytes"] == (S * M * N * 4 if S > 1 else 0), (i, p)
        if S > 1:
            assert i["split_ok"] and i["vec4"] and not i["scatter"] and not i["resid_packed"] and not i["invariant"], (i, p)
            assert p["kernel"].endswith("_splitk") and p["grid"] == tiles(M, N, p["bm"], p["bn"]) * S, (i, p)
        else:
            assert S == 1 and not p["kernel"].endswith("_splitk"), (i, p)
            assert 1 <= p["grid"] <= tiles(M, N, p["bm"], p["bn"]), (i, p)
        assert (K // 16) % S == 0, (i, p)
        assert p["vec4"] == i["vec4"], (i, p)
        if i["invariant"] and i["fmt"] == FMT["f16x2"]:
            assert (p["kernel"], p["bm"], p["bn"], S) == ("h2p", 128, 128, 1), (i, p)
        if i["fmt"] in (FMT["f16x2"], FMT["bf16x3"]) and M <= 512:      # batch-size independence of the small-batch regime
            small.setdefault((i["fmt"], N, K) + tuple(i[f] for f in FLAGS), set()).add(S)
    assert len(inputs) == 4 * len(GRID_M) * len(GRID_N) * len(GRID_K) * 2 ** len(FLAGS)
    assert small and all(len(s) == 1 for s in small.values()), [k for k, s in small.items() if len(s) > 1][:5]
    assert any(s != {1} for s in small.values())
