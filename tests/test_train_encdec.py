"""Training the encoder-decoder mapper (MappingType.TransformerDecoder): capdec_train_set_encdec, the rectangular attention
backward, the saved forward / backward of ``kind == 3`` and its 3 + 36 L optimizer slots.

References: tests/golden/train_step_ed_tiny.npz (tools/gen_encdec_train_golden.py: the reference's own modules, fp32 and
float64) and, where no fixture exists, the float64 restatement tests/encdec_train_def.py.  Bounds are the project's own
(test_train_step_frozen_gpt2_vs_reference_golden): loss 3e-4; per tensor 3e-3 of the reference's largest entry on the
subsample; norm within 2e-3 -- measured against float64 values.  The reference's own fp32 run sits a factor of 400 inside
them (asserted below at a tenth).  Updated weights are judged by applying the restated AdamW (tests/adamw_def.py) to the
gradients the device itself reports, at the bar of tests/test_adamw_update.py: every slot is wired to the optimizer with the
right offset and size, and no sign-like first Adam step amplifies round-off into the comparison."""
from __future__ import annotations

import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import adamw_def as A                                     # noqa: E402
import encdec_train_def as R                              # noqa: E402
from capdec_amd import synth                              # noqa: E402

T = torch.from_numpy
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = synth.GPT2_TINY
LOSS_BOUND, GRAD_BOUND, NORM_BOUND = 3e-4, 3e-3, 2e-3
PFX = "clip_project."


# ----------------------------------------------------------------------------------------------- shared references
def _fixture_sd(g):
    P, C, L, D = (int(v) for v in g["geom"])
    sd = synth.hot_state_dict(42, "transformer_decoder", D, P, C, L, DIMS)
    assert synth.state_dict_checksum(sd) == int(g["sd_crc"]), "RNG drift"
    return sd, (P, C, L, D)


_CHAIN = {}


def _fixture_chain(golden):
    """the float64 restatement replayed over the fixture's three iterations, once per process: per iteration
    (loss, {name: float64 gradient}); the weights move as the generator moved them (float64 AdamW, rounded to fp32)"""
    if "chain" not in _CHAIN:
        from oracle import capdec_oracle as O
        g = golden("train_step_ed_tiny")
        sd, _ = _fixture_sd(g)
        keys = [str(k) for k in g["keys"]]
        state = {k: (torch.zeros_like(sd[k], dtype=torch.float64), torch.zeros_like(sd[k], dtype=torch.float64)) for k in keys}
        out = []
        for it in range(len(g["losses"])):
            loss, grads = R.loss_and_grads(sd, T(g[f"tokens_{it}"]), T(g[f"prefix_{it}"]), DIMS.n_head)
            out.append((loss, grads))
            for k in keys:
                p64 = sd[k].double()
                O.adamw_transformers(p64, grads[k], state[k][0], state[k][1], it + 1, float(g["lrs"][it]))
                sd[k] = p64.float()
        _CHAIN["chain"] = out
    return _CHAIN["chain"]


def _check_grads(got, want, sub, tag, norms=None):
    """``got`` {name: device gradient}, ``want`` {name: float64 reference}: full tensors, or (``norms`` given) subsamples"""
    worst = (0.0, 0.0, "")
    for k, ref in want.items():
        gk = got[k].detach().cpu()
        ref_sub = ref if norms is not None else R.subsample(ref, sub)
        ref_norm = float(norms[k]) if norms is not None else float(ref.double().norm())
        ref_sub = torch.as_tensor(ref_sub).double()
        scale = float(ref_sub.abs().max())
        err = float((R.subsample(gk, sub).double() - ref_sub).abs().max())
        gn = float(gk.double().norm())
        nrm = abs(gn / ref_norm - 1.0) if ref_norm > 0 else (0.0 if gn <= 1e-9 else float("inf"))
        frac = max(err / (GRAD_BOUND * scale + 1e-9), nrm / NORM_BOUND)
        if frac > worst[0]:
            worst = (frac, err / scale if scale else err, k)
        assert err <= GRAD_BOUND * scale + 1e-9, (tag, k, err, scale)
        assert nrm < NORM_BOUND, (tag, k, gn, ref_norm)
    print(f"[train encdec] {tag}: {len(want)} tensors, worst {worst[0]:.3f} of the bound ({worst[2]}, {worst[1]:.2e} of its largest entry)")


# ----------------------------------------------------------------------------------------------- CPU
def test_restatement_equals_fixture_float64_and_reference_fp32_is_well_inside_the_bound(golden):
    g = golden("train_step_ed_tiny")
    keys = [str(k) for k in g["keys"]]
    sub = int(g["sub"])
    assert len(keys) == 75 and len(g["losses"]) == 3 and float(g["lrs"][0]) == 0.0 and float(g["lrs"][1]) > 0.0
    for it, (loss, grads) in enumerate(_fixture_chain(golden)):
        assert abs(loss - float(g["losses"][it])) < 1e-5
        worst64 = worst32 = 0.0
        for k in keys:
            ref = g[f"grad64_{it}_{k}_sub"]
            scale = float(np.abs(ref).max())
            assert scale > 0
            worst64 = max(worst64, float(np.abs(R.subsample(grads[k], sub).numpy() - ref).max()) / scale,
                          abs(float(grads[k].norm()) / float(g[f"grad64_{it}_{k}_norm"]) - 1.0))
            worst32 = max(worst32, float(np.abs(g[f"grad_{it}_{k}_sub"] - ref).max()) / scale)
        print(f"[train encdec] iteration {it}: restatement vs fixture float64 {worst64:.2e}; the reference's fp32 vs float64 {worst32:.2e}")
        assert worst64 <= 1e-9, it
        assert worst32 <= GRAD_BOUND / 10, it


@pytest.mark.parametrize("geom", [(10, 10, 2, 512), (5, 7, 2, 640)], ids=["p10c10", "p5c7d640"])
def test_wrong_backwards_are_far_from_the_truth(geom):
    """keys / values of the odd layers detached from x; ``ref`` detached in all but the last cross layer: each differs from
    the true gradient by at least 10 bounds on every tensor it touches (and touches many)"""
    P, C, L, D = geom
    sd = synth.hot_state_dict(42, "transformer_decoder", D, P, C, L, DIMS)
    gen = torch.Generator().manual_seed(3)
    tokens = torch.randint(1, DIMS.vocab, (2, 6), generator=gen)
    x = synth.synthetic_clip_embeddings(2, D, seed=9)
    _, true = R.loss_and_grads(sd, tokens, x, DIMS.n_head)
    for wrong, at_least in zip(R.WRONG, (63, 26)):
        _, bad = R.loss_and_grads(sd, tokens, x, DIMS.n_head, wrong=wrong)
        diff = {k: float((bad[k] - true[k]).abs().max() / true[k].abs().max()) for k in true}
        touched = {k: v for k, v in diff.items() if v > 1e-9}          # (the others: the same sum in another order)
        print(f"[train encdec] {geom} {wrong}: {len(touched)} tensors differ, by {min(touched.values()):.2f} .. {max(touched.values()):.2f} of max|grad|")
        assert len(touched) >= at_least
        assert min(touched.values()) >= 10 * GRAD_BOUND, min(touched, key=touched.get)


def test_header_prototype_signature_and_abi_number():
    from capdec_amd import _capi
    import ctypes as C
    with open(os.path.join(ROOT, "include", "capdec.h")) as f:
        h = f.read()
    assert re.search(r"\bint\s+capdec_train_set_encdec\s*\(\s*capdec_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", h)
    assert re.search(r"#define\s+CAPDEC_ABI_VERSION\s+6\b", h) and _capi.ABI_VERSION == 6
    res, args = _capi.SIGNATURES["capdec_train_set_encdec"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int]


def test_tensor_names_follow_the_reference_state_dict(golden):
    from capdec_amd.engine import Engine
    g = golden("train_step_ed_tiny")
    L = int(g["geom"][2])
    assert Engine.train_tensor_names("transformer_decoder", L) == [str(k)[len(PFX):] for k in g["keys"]]
    for tag in ("512", "p5"):
        m = golden("mapper_encdec_" + tag)
        if "keys" in m.files:
            keys = [str(k) for k in m["keys"]]
            keys = [k[len(PFX):] if k.startswith(PFX) else k for k in keys]
            assert Engine.train_tensor_names("transformer_decoder", int(m["geom"][3])) == keys


def _train_h():
    with open(os.path.join(ROOT, "capdec_amd", "csrc", "train.h")) as f:
        src = f.read()
    nw = int(re.search(r"constexpr\s+int\s+ATTN_BLK_NW\s*=\s*(\d+)\s*;", src).group(1))
    mx = int(re.search(r"constexpr\s+size_t\s+ATTN_BLK_LDS_MAX\s*=\s*(\d+)\s*\*\s*1024\s*;", src).group(1)) * 1024
    ms = int(re.search(r"constexpr\s+int\s+ATTN_RECT_MAX_S\s*=\s*(\d+)\s*;", src).group(1))
    body = re.search(r"struct\s+AttnRect\s*\{.*?bwd_bytes\(int Sq, int Sk\)\s*\{\s*return\s*(.*?);\s*\}", src, re.S).group(1)
    assert re.sub(r"\s+", "", body) == ("((size_t)2*std::max(Sq,Sk)*LD+(size_t)2*Sq*(Sk+1)+ATTN_BLK_NW*(2*HD+Sk))*sizeof(float)"), body
    return nw, mx, ms


def rect_bytes(hd, sq, sk, nw=16):
    return (2 * max(sq, sk) * (hd + 1) + 2 * sq * (sk + 1) + nw * (2 * hd + sk)) * 4


def rect_fits(hd, sq, sk):
    nw, mx, ms = _train_h()
    return sq <= ms and sk <= ms and rect_bytes(hd, sq, sk, nw) <= mx


SQUARE_MAX = 90     # the largest P = C whose self layers (heads of 96) fit: checked against train.h below


def test_rectangular_lds_rule():
    nw, mx, ms = _train_h()
    assert (nw, mx, ms) == (16, 150 * 1024, 128)
    assert rect_fits(96, SQUARE_MAX, SQUARE_MAX) and not rect_fits(96, SQUARE_MAX + 1, SQUARE_MAX + 1)
    assert rect_bytes(96, 90, 90) == 153408
    for P in (10, 40, 80):      # the reference's own sizes: clip_length 10, prefix_length 10 .. 80
        assert rect_fits(64, 10, 10) and rect_fits(96, P, 10) and rect_fits(96, P, P)
    assert rect_fits(96, 128, 3) and rect_fits(96, 4, 128) and not rect_fits(96, 129, 3) and not rect_fits(96, 4, 129)


class _FakeEngine:
    """records what train_step asks of the engine"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def record(*a, **k):
            self.calls.append(name)
            return 1.25 if name == "train_step" else None
        return record


def test_requires_grad_gates_train_step_and_mapper_shapes(monkeypatch):
    from capdec_amd import train as TR
    from capdec_amd._capi import CapdecError
    from capdec_amd.gpt2_prefix import ClipCaptionPrefix, MappingType
    model = ClipCaptionPrefix(10, clip_length=10, prefix_dim=512, num_layers=2, mapping_type=MappingType.TransformerDecoder, gpt2_dims=DIMS)
    model.load_state_dict(synth.hot_state_dict(42, "transformer_decoder", 512, 10, 10, 2, DIMS))
    fake = _FakeEngine()
    model._engine, model._dirty = fake, False
    opt = TR.AdamW(lr=1e-4)
    tokens, x = torch.ones(2, 4, dtype=torch.int64), torch.zeros(2, 512)
    with pytest.raises(CapdecError, match="train_step: the encoder-decoder mapper is inference-only"):
        TR.train_step(model, opt, tokens, None, x)
    with pytest.raises(CapdecError, match="train_step: the encoder-decoder mapper is inference-only"):
        model._mapper_shapes()
    assert fake.calls == []
    assert model.clip_project.requires_grad_() is model.clip_project
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)      # (the token batch would move to a device this test does not need)
    assert TR.train_step(model, opt, tokens, None, x) == 1.25
    assert "train_set_encdec" in fake.calls and fake.calls.index("train_set_encdec") < fake.calls.index("train_step")
    shapes = model._mapper_shapes()
    assert len(shapes) == 75 and list(shapes)[0] == "prefix_const" and list(shapes)[-1] == "linear.bias"
    model._device_ahead = False             # (the fake engine holds no weights to read back)
    model.clip_project.requires_grad_(False)
    with pytest.raises(CapdecError, match="inference-only"):
        TR.train_step(model, opt, tokens, None, x)
    model._engine = None


# ----------------------------------------------------------------------------------------------- GPU
def _model(P, C, L, D, sd, full=False):
    from capdec_amd.gpt2_prefix import ClipCaptionModel, ClipCaptionPrefix, MappingType
    cls = ClipCaptionModel if full else ClipCaptionPrefix
    m = cls(P, clip_length=C, prefix_dim=D, num_layers=L, mapping_type=MappingType.TransformerDecoder, gpt2_dims=DIMS).to("cuda:0")
    m.load_state_dict(sd)
    m.train()
    m.gpt.config.resid_pdrop = m.gpt.config.embd_pdrop = m.gpt.config.attn_pdrop = 0.0
    m.clip_project.requires_grad_()
    return m


def _batch(B, D, seed, length=6):
    gen = torch.Generator().manual_seed(100 + seed)
    tokens = torch.zeros(B, length, dtype=torch.int64)
    for r in range(B):
        n = length if r == 0 else max(1, length - 1 - r)
        tokens[r, :n] = torch.randint(1, DIMS.vocab, (n,), generator=gen)
    return tokens, synth.synthetic_clip_embeddings(B, D, seed=60 + seed)


def _mask(P, tokens):
    return torch.cat((torch.ones(tokens.shape[0], P), (tokens != 0).float()), dim=1)


@pytest.mark.gpu
def test_fixture_parity_slot_wiring_and_inference_after_training(golden):
    """three iterations on train_step_ed_tiny.npz: loss, lr sequence and all 75 gradients against the reference's float64
    values; every update equals the restated AdamW applied to the device's own gradients; then inference runs the trained
    weights (the stacked cross GEMM, layer 0's shared queries, dropped operand planes)"""
    from capdec_amd import train as Tr
    g = golden("train_step_ed_tiny")
    sd, (P, C, L, D) = _fixture_sd(g)
    keys = [str(k) for k in g["keys"]]
    sub = int(g["sub"])
    model = _model(P, C, L, D, sd)
    try:
        opt = Tr.AdamW(model.parameters(), lr=float(g["lr"]))
        sched = Tr.get_linear_schedule_with_warmup(opt, int(g["warmup"]), int(g["total"]))
        m64 = v64 = m32 = v32 = None
        for it in range(len(g["losses"])):
            tokens, mask, prefix = T(g[f"tokens_{it}"]), T(g[f"mask_{it}"]), T(g[f"prefix_{it}"])
            lr_t = opt.param_groups[0]["lr"]
            assert abs(lr_t - float(g["lrs"][it])) < 1e-12
            before = model.engine.mapper_parameters(model._train_shapes())
            assert list(before) == keys
            loss = Tr.train_step(model, opt, tokens, mask, prefix)
            print(f"[train encdec] fixture iteration {it}: loss {loss:.6f} (reference {float(g['losses'][it]):.6f})")
            assert abs(loss - float(g["losses"][it])) < LOSS_BOUND, (it, loss)
            grads = Tr.all_gradients(model)
            assert list(grads) == keys
            _check_grads(grads, {k: g[f"grad64_{it}_{k}_sub"] for k in keys}, sub, f"fixture iteration {it}",
                         norms={k: g[f"grad64_{it}_{k}_norm"] for k in keys})
            # ---- slot wiring: the restated AdamW on the device's own gradients gives the device's new weights
            after = model.engine.mapper_parameters(model._train_shapes())
            if m64 is None:
                m64 = {k: torch.zeros(before[k].shape, dtype=torch.float64) for k in keys}
                v64 = {k: torch.zeros(before[k].shape, dtype=torch.float64) for k in keys}
                m32 = {k: torch.zeros(before[k].shape) for k in keys}
                v32 = {k: torch.zeros(before[k].shape) for k in keys}
            worst = 0.0
            for k in keys:
                b, gk, a = before[k].cpu(), grads[k].cpu(), after[k].cpu()
                want = A.adamw(b.double(), gk.double(), m64[k], v64[k], it + 1, lr_t)
                got32 = A.adamw(b, gk, m32[k], v32[k], it + 1, lr_t)
                e32, err = float(A.units_off(got32, want, lr_t).max()), float(A.units_off(a, want, lr_t).max())
                worst = max(worst, err / A.bar(e32))
                assert err <= A.bar(e32), (it, k, err, e32)
                if A.f32(lr_t) == 0.0:
                    assert torch.equal(a, b), (it, k)
                else:
                    assert float((a - b).abs().max()) > 0.25 * A.f32(lr_t), (it, k)
            print(f"[train encdec] fixture iteration {it}: updates of 75 slots, worst {worst:.3f} of the AdamW bar")
            sched.step()
        fin = model.state_dict()
        x = T(g["prefix_0"])
        with torch.no_grad():
            want = R.mapper({k[len(PFX):]: fin[k].double() for k in keys}, x.double())
        err = float((model.clip_project(x).double().cpu().reshape(want.shape) - want).abs().max())
        print(f"[train encdec] inference after training vs the restatement on the trained weights: {err:.2e}")
        assert err <= 2e-4
    finally:
        model.release()


SWEEP = {"p5c7d640": (5, 7, 2, 640, 3), "p12c3": (12, 3, 1, 512, 1), "one_key": (3, 1, 1, 512, 2), "p70": (70, 3, 1, 512, 2),
         "c66": (4, 66, 1, 512, 2), "square_max": (SQUARE_MAX, SQUARE_MAX, 1, 512, 2)}


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(SWEEP))
def test_geometry_sweep_against_the_restatement(tag):
    """one iteration per geometry against float64 autograd of the restatement; the same step twice is bit-identical"""
    from capdec_amd import train as Tr
    P, C, L, D, B = SWEEP[tag]
    assert rect_fits(64, C, C) and rect_fits(96, P, C) and rect_fits(96, P, P)
    sd = synth.hot_state_dict(31, "transformer_decoder", D, P, C, L, DIMS)
    tokens, x = _batch(B, D, seed=len(tag))
    want_loss, want = R.loss_and_grads(sd, tokens, x, DIMS.n_head)
    model = _model(P, C, L, D, sd)
    try:
        opt = Tr.AdamW(model.parameters(), lr=1e-4)
        loss = Tr.train_step(model, opt, tokens, _mask(P, tokens), x, apply_update=False)
        grads = Tr.all_gradients(model)
        print(f"[train encdec] {tag}: loss {loss:.6f} (float64 {want_loss:.6f})")
        assert abs(loss - want_loss) < LOSS_BOUND
        _check_grads(grads, want, 4096, tag)
        again = Tr.train_step(model, opt, tokens, _mask(P, tokens), x, apply_update=False)
        grads2 = Tr.all_gradients(model)
        assert again == loss
        differ = [k for k in grads if not torch.equal(grads[k], grads2[k])]
        assert not differ, differ[:5]
    finally:
        model.release()


@pytest.mark.gpu
def test_full_scope_composes():
    """scope 1 (a plain ClipCaptionModel, dropout 0): every mapper gradient and every GPT-2 gradient against float64"""
    from capdec_amd import train as Tr
    P, C, L, D, B = 5, 7, 2, 512, 2
    sd = synth.hot_state_dict(33, "transformer_decoder", D, P, C, L, DIMS)
    tokens, x = _batch(B, D, seed=4)
    want_loss, want = R.loss_and_grads(sd, tokens, x, DIMS.n_head, train_gpt=True)
    model = _model(P, C, L, D, sd, full=True)
    try:
        opt = Tr.AdamW(model.parameters(), lr=1e-4)
        loss = Tr.train_step(model, opt, tokens, _mask(P, tokens), x, apply_update=False)
        assert abs(loss - want_loss) < LOSS_BOUND
        grads = Tr.all_gradients(model)
        assert sorted(grads) == sorted(want) and len(grads) == 3 + 36 * L + 2 + 12 * DIMS.n_layer + 2
        _check_grads(grads, want, 4096, "full scope")
    finally:
        model.release()


@pytest.mark.gpu
def test_refusals_and_the_lds_limit(golden):
    from capdec_amd import train as Tr
    from capdec_amd._capi import CapdecError
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    OLD = "train_step: the encoder-decoder mapper is inference-only"
    g = golden("decode_encdec_tiny")
    model = ClipCaptionModel(10, clip_length=10, prefix_dim=512, num_layers=4, mapping_type=MappingType.TransformerDecoder,
                             gpt2_dims=DIMS).to("cuda:0").eval()
    model.load_state_dict(synth.hot_state_dict(42, "transformer_decoder", 512, 10, 10, 4, DIMS))
    try:
        x = T(g["greedy_x"])
        tokens = torch.tensor(g["greedy_ids_T12"][:, :6])
        opt = Tr.AdamW(model.parameters(), lr=1e-4)
        eng = model.engine

        def refused():
            with pytest.raises(CapdecError, match=OLD):
                Tr.train_step(model, opt, tokens, None, x)
            with pytest.raises(CapdecError, match=OLD):
                eng.train_step(x, tokens, 1e-4)
            y = eng.mapper_forward(x)
            assert float((y.double().cpu() - T(g["greedy_prefix_embed"]).double()).abs().max()) <= 2e-4

        refused()
        eng.train_set_encdec(True)
        assert np.isfinite(eng.train_step(x, tokens, 1e-4, apply_update=False))
        eng.train_set_encdec(False)
        refused()
        # ---- one past the square limit: refused on the host, with the limit in the message; the context goes on working
        big = SQUARE_MAX + 1
        eng.train_set_encdec(True)
        eng.load_mapper_encdec(synth.hot_encdec_mapper_state_dict(48, 512, big, big, 1))
        xb = synth.synthetic_clip_embeddings(2, 512, seed=1)
        tb = tokens[:2]
        with pytest.raises(CapdecError, match=r"LDS.*153600|153600.*LDS"):
            eng.train_step(xb, tb, 1e-4, apply_update=False)
        P, C, L, D = 5, 7, 1, 512
        sd = synth.hot_state_dict(42, "transformer_decoder", D, P, C, L, DIMS)      # (seed 42: the GPT-2 the context holds)
        eng.load_mapper_encdec(sd)         # (the switch survives the load)
        want_loss, _ = R.loss_and_grads(sd, tb, xb, DIMS.n_head)
        assert abs(eng.train_step(xb, tb, 1e-4, apply_update=False) - want_loss) < LOSS_BOUND
    finally:
        model._device_ahead = False
        model.release()


class _DS(torch.utils.data.Dataset):
    prefix_length = 10

    def __init__(self, n, seed):
        gen = torch.Generator().manual_seed(seed)
        x = synth.synthetic_clip_embeddings(n, 512, seed=seed)
        self.items = []
        for i in range(n):
            k = 3 + i % 6
            tok = torch.zeros(9, dtype=torch.int64)
            tok[:k] = torch.randint(1, DIMS.vocab, (k,), generator=gen)
            self.items.append((tok, torch.cat((torch.ones(10), (tok > 0).float())), x[i], i))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


@pytest.mark.gpu
def test_training_loop(tmp_path):
    """gpt2_prefix.train, two epochs over eight items: the reference's checkpoint names, the saved mapper equal to the same
    loop run step by step with waits, and a second epoch whose mean loss is below the first"""
    from torch.utils.data import DataLoader
    from capdec_amd import gpt2_prefix as GP
    from capdec_amd import train as Tr
    sd = synth.hot_state_dict(42, "transformer_decoder", 512, 10, 10, 2, DIMS)
    ds = _DS(8, 5)
    lr, bs, epochs, warm = 1e-3, 4, 2, 1

    def fresh():
        m = GP.ClipCaptionPrefix(10, clip_length=10, prefix_dim=512, num_layers=2, mapping_type=GP.MappingType.TransformerDecoder,
                                 gpt2_dims=DIMS).to("cuda:0")
        m.load_state_dict(sd)
        return m

    model = fresh()
    try:
        assert not model.clip_project._requires_grad
        torch.manual_seed(7)
        GP.train(ds, model, bs, epochs, lr=lr, warmup_steps=warm, output_dir=str(tmp_path), output_prefix="ed",
                 args=SimpleNamespace(save_every=5))
        assert model.clip_project._requires_grad
        assert sorted(os.listdir(tmp_path)) == ["ed-000.pt", "ed-001.pt"]
        saved = torch.load(os.path.join(tmp_path, "ed-001.pt"))
    finally:
        model.release()
    ref = fresh()
    try:
        ref.train()
        ref.clip_project.requires_grad_()
        opt = Tr.AdamW(ref.parameters(), lr=lr)
        torch.manual_seed(7)
        loader = DataLoader(ds, batch_size=bs, shuffle=True, drop_last=True)
        sched = Tr.get_linear_schedule_with_warmup(opt, warm, epochs * len(loader))
        means = []
        for _ in range(epochs):
            losses = []
            for tokens, mask, prefix, _idx in loader:
                losses.append(Tr.train_step(ref, opt, tokens, mask, prefix.to("cuda:0", dtype=torch.float32)))
                sched.step()
            means.append(sum(losses) / len(losses))
        fin = ref.state_dict()
    finally:
        ref.release()
    print(f"[train encdec] loop: epoch means {means}")
    assert means[1] < means[0]
    keys = [k for k in fin if k.startswith(PFX)]
    assert len(keys) == 75
    for k in keys:
        assert float((saved[k] - fin[k]).abs().max()) <= 1e-6, k
    assert float((fin[PFX + "prefix_const"] - sd[PFX + "prefix_const"]).abs().max()) > 1e-4


@pytest.mark.gpu
def test_fixture_parity_on_the_native_fp32_gemm():
    """CAPDEC_TRAIN_F16X2=0 puts the step's backward GEMMs on the native fp32 MFMA kernel: the fixture case once more, in a
    fresh child process"""
    import subprocess
    env = dict(os.environ, CAPDEC_TRAIN_F16X2="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "test_fixture_parity_slot_wiring", "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0 and "1 passed" in tail and "failed" not in tail, tail

