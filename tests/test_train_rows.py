"""The whole train step at the row counts where its weight-gradient GEMMs split K.

Every dW = dY^T X of the step is a GEMM whose K is the number of token rows of the batch (gemm_tn, csrc/gemm_dispatch.hip);
up to 448 rows every shape runs the unsplit 128 x 128 kernel, from 449 rows on almost every shape runs a split-K plan, and
the row-parallel backward kernels (ln_param_grad_kernel, colsum_kernel, ce_bwd_kernel) run many row blocks.  Two geometries
on the tiny GPT-2 (768-d, 12 heads, 2 layers, V = 1531) with a two-layer TransformerMapper, prefix_length = clip_length = 40,
640-d embeddings, ragged right-padded captions (row 0 of full length):

  first-split       B = 8,  L = 24:  512 GPT-2 rows,  640 mapper rows  (K 512 / 640: the first K values that split)
  reference-batch   B = 34, L = 20: 2040 GPT-2 rows, 2720 mapper rows  (K 2048 / 2752: the benchmark's train_step workload)

each in the frozen scope (loss, every mapper gradient) and in the full scope with dropout 0.1 under injected keep-masks
(every tensor), against ``oracle.capdec_oracle.train_step_loss_and_grads`` run in FLOAT64.  The comparison rule is that of
test_train_step_long_sequences_vs_oracle (tests/train_compare_def.py): loss within 3e-4, every entry within 3e-3 of the
tensor's largest, norms within 2e-3, no allowance for GPT-2 tensors, the ReLU near-tie allowance for the mapper's.  The
allowance is a condition on the inputs: the float32 oracle is held to the same rule against the float64 one first, and its
per-tensor counts are reported next to the device's.  With the seeds below the float32 oracle stays inside the rule on the
two CPUs it was run on -- on one, a single tensor beyond the bar (first-split full scope, layers.0.mlp.fc1.weight, 41 of
1 179 648 entries, largest 4.7e-3 of scale); on the other a ReLU of layer 1 switches (layers.1.mlp.fc1.weight up to 663
entries, largest 6.2e-2; norm2.weight 27 of 768, largest 5.9e-3) -- and the device uses the allowance for no tensor: its
worst entry is 2e-6 to 4e-6 of the tensor's largest (profiles/train_rows.txt).

``test_weight_gradient_plans`` (no GPU) states the plan of every dW product of both geometries through the host planner,
so a threshold edit that moves these batches off the split plans fails there; the last test runs the four cases again in
a child process on the native fp32 GEMM (CAPDEC_TRAIN_F16X2=0: transpose_pad with K padded to 32, gemm_f32_kernel at
K >= 2048)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from capdec_amd import synth                                            # noqa: E402
from tests import test_gemm_plan as GP                                  # noqa: E402
from tests.test_gemm_plan import planner                                # noqa: E402,F401  (the fixture: the planner program)
from tests.train_compare_def import compare_gradients                   # noqa: E402

DIMS, P, D, NLAY = synth.GPT2_TINY, 40, 640, 2
GEOMETRIES = {"first-split": (8, 24), "reference-batch": (34, 20)}       # name -> (B, L)
SCOPES = ("frozen", "full_dropout")
SD_SEED, TOKEN_SEED, EMBEDDING_SEED = 13, 77, 5
CASES = [(g, s) for g in GEOMETRIES for s in SCOPES]


def rows(geometry):
    """(GPT-2 rows, loss rows, mapper rows, embedding rows) of a geometry"""
    B, L = GEOMETRIES[geometry]
    return B * (P + L), B * L, B * 2 * P, B


def ceil64(n):
    return (n + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------ the plans, no GPU
def weight_gradient_products(geometry):
    """(name, rows, out, in) of every dW product of one full-scope step (train_step.hip, train_mapper.hip), per layer kind"""
    R, Rl, M, B = rows(geometry)
    d, hid = DIMS.n_embd, 2 * DIMS.n_embd
    return [("wte", Rl, DIMS.vocab, d), ("c_attn", R, 3 * d, d), ("attn.c_proj", R, d, d), ("c_fc", R, 4 * d, d),
            ("mlp.c_proj", R, d, 4 * d), ("mapper qkv", M, 3 * d, d), ("mapper project", M, d, d), ("mapper fc1", M, hid, d),
            ("mapper fc2", M, d, hid), ("mapper linear", B, P * d, D)]


# (kernel, S, blocks) per product, in the order of weight_gradient_products
PLANS = {
    "first-split": [("h2p", 1, 72), ("pp_splitk", 4, 216), ("h2p_splitk", 2, 72), ("h2p_splitk", 2, 288), ("h2p_splitk", 2, 288),
                    ("pp_splitk", 4, 216), ("h2p_splitk", 2, 72), ("h2p_splitk", 2, 144), ("h2p_splitk", 2, 144), ("h2p", 1, 512)],
    "reference-batch": [("h2p_splitk", 2, 144), ("pp_splitk", 4, 216), ("h2p_splitk", 8, 288), ("h2p_splitk", 2, 288),
                        ("h2p_splitk", 2, 288), ("pp_splitk", 4, 216), ("h2p_splitk", 2, 72), ("h2p_splitk", 2, 144),
                        ("h2p_splitk", 2, 144), ("h2p", 1, 512)],
}


def test_weight_gradient_plans(planner):                     # noqa: F811
    for geometry in GEOMETRIES:
        prods = weight_gradient_products(geometry)
        plans = planner([dict(fmt=GP.FMT["f16x2"], M=out, N=inn, K=ceil64(r), vec4=1, wide_ok=0, invariant=0, split_ok=1,
                              packed_out=0, resid_packed=0, scatter=0) for _, r, out, inn in prods])
        got = [(p["kernel"], p["S"], p["grid"]) for p in plans]
        print(geometry, got)
        assert got == PLANS[geometry], (geometry, list(zip((n for n, *_ in prods), got)))
        kinds = {k for k, _, _ in got}
        assert {"h2p_splitk", "pp_splitk"} <= kinds, (geometry, kinds)
        for (name, r, out, inn), (k, S, _) in zip(prods, got):
            if (out, inn) == (DIMS.n_embd, DIMS.n_embd):
                assert S > 1 and k.endswith("_splitk"), (geometry, name, k, S)
    assert [rows(g)[:3] for g in GEOMETRIES] == [(512, 192, 640), (2040, 680, 2720)]


# ------------------------------------------------------------------------------------------------ batches, references
@functools.lru_cache(maxsize=1)
def _state_dict():
    return synth.hot_state_dict(SD_SEED, "transformer_encoder", D, P, P, NLAY, DIMS)


@functools.lru_cache(maxsize=2)
def batch(geometry):
    """tokens [B, L] (ragged, right-padded, row 0 full), mask [B, P + L], prefix [B, D], flat keep-mask stream, its masks"""
    from oracle import capdec_oracle as O
    B, L = GEOMETRIES[geometry]
    g = torch.Generator().manual_seed(TOKEN_SEED + B)
    lens = [L] + torch.randint(L // 3, L + 1, (B - 1,), generator=g).tolist()
    tokens = torch.zeros(B, L, dtype=torch.int64)
    for r, n in enumerate(lens):
        tokens[r, :n] = torch.randint(1, DIMS.vocab, (n,), generator=g)
    mask = torch.cat((torch.ones(B, P), (tokens != 0).float()), dim=1)
    prefix = synth.synthetic_clip_embeddings(B, D, seed=EMBEDDING_SEED)
    sites = O.dropout_sites(DIMS.n_layer, B, P + L, DIMS.n_embd, DIMS.n_head)
    flat = (torch.rand(sum(int(np.prod(sh)) for _, sh in sites), generator=g) >= 0.1).to(torch.uint8)
    masks, o = [], 0
    for _, sh in sites:
        k = int(np.prod(sh))
        masks.append(flat[o:o + k].reshape(sh))
        o += k
    return tokens, mask, prefix, flat, masks


def oracle(geometry, scope, dtype):
    """(loss, gradients) of the oracle run in ``dtype``"""
    from oracle import capdec_oracle as O
    tokens, _, prefix, _, masks = batch(geometry)
    full = scope == "full_dropout"
    sd = {k: v.to(dtype) for k, v in _state_dict().items()}
    return O.train_step_loss_and_grads(sd, tokens, prefix.to(dtype), "transformer_encoder", P, n_head=DIMS.n_head, clip_length=P,
                                       num_layers=NLAY, train_gpt=full, drop=(0.1, masks) if full else None)


def _report(line):
    from tests.test_hip_parity import _report as report
    report(line)


def reference(geometry, scope, report=_report):
    """the float64 oracle -- after the float32 oracle has passed the comparison rule against it (the cap of the ReLU
    near-tie allowance is a condition on the inputs: the reference alone must stay inside it)"""
    loss64, want = oracle(geometry, scope, torch.float64)
    loss32, g32 = oracle(geometry, scope, torch.float32)
    assert abs(float(loss32) - float(loss64)) < 3e-4
    compare_gradients(g32, want, "", f"train rows {geometry} {scope}, the reference alone (fp32 oracle vs fp64 oracle)", report)
    return float(loss64), want


def device_step(geometry, scope):
    from capdec_amd import train as Tr
    from capdec_amd.gpt2_prefix import ClipCaptionModel, ClipCaptionPrefix, MappingType
    tokens, mask, prefix, flat, _ = batch(geometry)
    full = scope == "full_dropout"
    cls = ClipCaptionModel if full else ClipCaptionPrefix
    model = cls(P, clip_length=P, prefix_size=D, num_layers=NLAY, mapping_type=MappingType.TransformerEncoder, gpt2_dims=DIMS).to("cuda:0")
    try:
        model.load_state_dict(_state_dict())
        model.train()
        loss = Tr.train_step(model, Tr.AdamW(model.parameters(), lr=1e-3), tokens, mask, prefix, apply_update=False,
                             dropout_masks=flat if full else None)
        got = Tr.all_gradients(model) if full else Tr.mapper_gradients(model)
        return loss, {k: v.cpu() for k, v in got.items()}
    finally:
        model.release()


@pytest.mark.gpu
@pytest.mark.parametrize("geometry,scope", CASES, ids=[f"{g}-{s}" for g, s in CASES])
def test_train_step_rows_vs_fp64(geometry, scope):
    tokens = batch(geometry)[0]
    B, L = GEOMETRIES[geometry]
    assert tokens.shape == (B, L) and int((tokens[0] != 0).sum()) == L and int((tokens != 0).sum()) < B * L
    want_loss, want = reference(geometry, scope)
    loss, got = device_step(geometry, scope)
    native = os.environ.get("CAPDEC_TRAIN_F16X2") == "0"
    _report(f"[train rows {geometry} {scope}{', CAPDEC_TRAIN_F16X2=0' if native else ''}] loss {loss:.6f} vs fp64 oracle "
            f"{want_loss:.6f}: |difference| {abs(loss - want_loss):.2e} (bound 3e-4)")
    assert abs(loss - want_loss) < 3e-4, (loss, want_loss)
    compare_gradients(got, want, "" if scope == "full_dropout" else "clip_project.",
                      f"train rows {geometry} {scope}, device{' (CAPDEC_TRAIN_F16X2=0)' if native else ''}", _report)


@pytest.mark.gpu
def test_train_step_rows_on_the_native_fp32_gemm():
    """CAPDEC_TRAIN_F16X2=0 (and nothing else) in one child process: the four cases again with every backward GEMM on the
    native fp32 MFMA kernel -- transpose_pad with K padded to 32 and gemm_f32_kernel at K >= 2048 -- held to the same
    float64 numbers on identical inputs"""
    env = dict(os.environ, CAPDEC_TRAIN_F16X2="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "vs_fp64",
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:]
    assert r.returncode == 0 and f"{len(CASES)} passed" in tail and "failed" not in tail and "skipped" not in tail, tail


if __name__ == "__main__":            # the reference-alone condition of every case, on the CPU: python tests/test_train_rows.py
    for geometry, scope in CASES:
        reference(geometry, scope, report=print)
