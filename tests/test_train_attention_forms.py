"""The train step's attention at every kernel form and on both sides of every switch between them.

``train_attn_fwd`` / ``train_attn_bwd`` (csrc/train_ops.hip) pick the block form (one block per (sample, head): K, V, P and dS
in LDS) while ``S <= 128`` and ``AttnBlk<HD>::fwd_bytes(S)`` / ``bwd_bytes(S)`` fit ``ATTN_BLK_LDS_MAX`` (csrc/train.h), the
wavefront form (one wavefront per query / key) otherwise; the TransformerMapper's forward falls back to the inference
kernel (``launch_attn_mapper``, csrc/attention.hip: 160 KiB of LDS).  The host-only test restates that arithmetic and
derives the boundary lengths; the GPU cases are built FROM those lengths, so a moved limit moves the cases with it.

Every GPU case is one ``capdec_amd.train.train_step(apply_update=False)`` of a two-layer model against
``oracle.capdec_oracle.train_step_loss_and_grads`` in float64: the loss, every gradient entry by entry and every norm.

The bar is taken from the reference, not from the kernels: the same oracle run in float32 gives, per tensor,
``e32 = max|g32 - g64| / max|g64|`` (about 4e-6 at these shapes) and the device must stay within ``32 * max(e32, 4e-6)`` of
the tensor's largest entry -- the factor 32 for what a correct fp32 pipeline may do differently from torch's CPU fp32:
summation order, atomics, the two-fp16-plane products, the loss scale.  Norms within 1e-4, the loss within 1e-4.  A
reference whose own ``e32`` would lift the bar past the 3e-3 of the older train tests is refused (a ReLU that switches
between the two oracle runs would do that).  Measured figures: profiles/train_attention_forms.txt."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from capdec_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------- the launchers' arithmetic
BLK_MAX_S = 128          # train_ops.hip: a lane of the block kernels owns the keys lane and lane + 64
TRAIN_MAX_S = 256        # train_step.hip: prefix_length + L <= 256
MAPPER_LDS_MAX = 160 * 1024          # attention.hip, launch_attn_mapper


def _train_h_constants():
    """(ATTN_BLK_NW, ATTN_BLK_LDS_MAX in bytes) as csrc/train.h spells them"""
    with open(os.path.join(ROOT, "capdec_amd", "csrc", "train.h")) as f:
        src = f.read()
    nw = re.search(r"constexpr\s+int\s+ATTN_BLK_NW\s*=\s*(\d+)\s*;", src)
    mx = re.search(r"constexpr\s+size_t\s+ATTN_BLK_LDS_MAX\s*=\s*(\d+)\s*\*\s*1024\s*;", src)
    assert nw and mx, "csrc/train.h no longer spells ATTN_BLK_NW / ATTN_BLK_LDS_MAX as this test reads them"
    return int(nw.group(1)), int(mx.group(1)) * 1024


ATTN_BLK_NW, ATTN_BLK_LDS_MAX = _train_h_constants()


def blk_fwd_bytes(hd, S):
    """AttnBlk<HD>::fwd_bytes: K and V tiles [S][HD + 1], a query [HD] and a score row [S] per wavefront"""
    return (2 * S * (hd + 1) + ATTN_BLK_NW * (hd + S)) * 4


def blk_bwd_bytes(hd, S):
    """AttnBlk<HD>::bwd_bytes: two tiles [S][HD + 1], P and dS [S][S + 1], (q, dO) [2 HD] and a row [S] per wavefront"""
    return (2 * S * (hd + 1) + 2 * S * (S + 1) + ATTN_BLK_NW * (2 * hd + S)) * 4


def mapper_fwd_bytes(hd, S):
    """launch_attn_mapper: K and V tiles [S][HD + 1], a query [HD] and a score row [S] for each of four wavefronts"""
    return (2 * S * (hd + 1) + 4 * hd + 4 * S) * 4


def _last_fit(nbytes, limit, cap):
    """the largest S <= cap whose request fits (the requests grow with S)"""
    return max(S for S in range(1, cap + 1) if nbytes(S) <= limit)


BLK_FWD_MAX = {hd: _last_fit(functools.partial(blk_fwd_bytes, hd), ATTN_BLK_LDS_MAX, BLK_MAX_S) for hd in (64, 96)}
BLK_BWD_MAX = {hd: _last_fit(functools.partial(blk_bwd_bytes, hd), ATTN_BLK_LDS_MAX, BLK_MAX_S) for hd in (64, 96)}
MAPPER_FWD_MAX = _last_fit(functools.partial(mapper_fwd_bytes, 96), MAPPER_LDS_MAX, 4096)


def attention_forms(hd, S, blk=True):
    """(forward, backward) kernel family of a (head size, sequence length); ``blk`` False: under CAPDEC_TRAIN_ATTN_BLK=0"""
    beyond = "wavefront" if hd == 64 else "inference"
    return (beyond if not blk or S > BLK_FWD_MAX[hd] else "block"), ("wavefront" if not blk or S > BLK_BWD_MAX[hd] else "block")


# ------------------------------------------------------------------------------------------- the cases
P_GPT, D_MLP, D_TM, VOCAB = 10, 512, 640, 1531
DIMS_256 = synth.GPT2Dims(n_layer=2, vocab=VOCAB, n_pos=TRAIN_MAX_S)

# GPT-2 side (HD 64, causal): (S, B) -- both sides of the backward's LDS boundary, both sides of the 128 / 129 switch, the
# longest sequence train_step takes; B = 1 at 128 / 129 puts R = B S on and one past the 128-row blocks of
# ln_param_grad_kernel and the 64-row blocks of colsum_kernel; (P + 1, 1) is the one-token batch
_B64 = BLK_BWD_MAX[64]
GPT_CASES = [(_B64, 2), (_B64 + 1, 2), (BLK_MAX_S, 2), (BLK_MAX_S, 1), (BLK_MAX_S + 1, 2), (BLK_MAX_S + 1, 1),
             (TRAIN_MAX_S, 2), (P_GPT + 1, 1)]
GPT_SCOPES = ["full_dropout", "frozen"]

# mapper side (HD 96, bidirectional): (clip_length, prefix_length, scope); sequence = clip_length + prefix_length
_B96 = BLK_BWD_MAX[96]


def _split(S):
    return S // 2, S - S // 2


MAPPER_LENGTHS = [_B96, _B96 + 1, BLK_MAX_S, BLK_MAX_S + 1, MAPPER_FWD_MAX]
MAPPER_CASES = [_split(S) + ("frozen",) for S in MAPPER_LENGTHS] + [_split(S) + ("full",) for S in (_B96 + 1, MAPPER_FWD_MAX)]
MAPPER_REFUSED = (MAPPER_FWD_MAX - MAPPER_FWD_MAX // 2 + 1, MAPPER_FWD_MAX // 2)          # one row more than fits


def test_attention_form_boundaries_from_the_launchers_arithmetic():
    """No GPU: the LDS formulas of csrc/train.h and of launch_attn_mapper, restated, give the boundary lengths the GPU
    cases are built from -- and those are the ones DESIGN.md ("Train step: which attention kernel runs") documents."""
    assert (ATTN_BLK_NW, ATTN_BLK_LDS_MAX) == (16, 150 * 1024)
    # block backward: GPT-2 through 102, the TransformerMapper through 90; block forward through 128 for both
    assert BLK_BWD_MAX == {64: 102, 96: 90} and BLK_FWD_MAX == {64: BLK_MAX_S, 96: BLK_MAX_S}
    for hd, S in ((64, 102), (96, 90)):
        assert blk_bwd_bytes(hd, S) <= ATTN_BLK_LDS_MAX < blk_bwd_bytes(hd, S + 1)
    assert (blk_bwd_bytes(64, 102), blk_bwd_bytes(64, 103)) == (151808, 154040)
    assert (blk_bwd_bytes(96, 90), blk_bwd_bytes(96, 91)) == (153408, 155704)
    assert max(blk_fwd_bytes(64, BLK_MAX_S), blk_fwd_bytes(96, BLK_MAX_S)) == 113664 <= ATTN_BLK_LDS_MAX
    # the mapper's forward beyond the block form: the inference kernel through 204
    assert MAPPER_FWD_MAX == 204 and mapper_fwd_bytes(96, 204) == 163104 <= MAPPER_LDS_MAX < mapper_fwd_bytes(96, 205)
    assert [attention_forms(64, S) for S in (102, 103, 128, 129, 256)] == [
        ("block", "block"), ("block", "wavefront"), ("block", "wavefront"), ("wavefront", "wavefront"), ("wavefront", "wavefront")]
    assert [attention_forms(96, S) for S in (90, 91, 128, 129, 204)] == [
        ("block", "block"), ("block", "wavefront"), ("block", "wavefront"), ("inference", "wavefront"), ("inference", "wavefront")]
    # the cases the GPU tests run
    assert GPT_CASES == [(102, 2), (103, 2), (128, 2), (128, 1), (129, 2), (129, 1), (256, 2), (11, 1)]
    assert [c[:2] for c in MAPPER_CASES] == [(45, 45), (45, 46), (64, 64), (64, 65), (102, 102), (45, 46), (102, 102)]
    assert MAPPER_REFUSED == (103, 102)
    # the row-blocked reductions meet R = B S on a block edge and one past it
    assert {B * S for S, B in GPT_CASES} >= {128, 129, 256, 258}


# ------------------------------------------------------------------------------------------- batches and references
FACTOR, E32_FLOOR, NORM_TOL, LOSS_TOL = 32.0, 4e-6, 1e-4, 1e-4
OLD_BAR = 3e-3           # the per-entry bar of the older train tests: no bar of this file may reach it


@functools.lru_cache(maxsize=2)
def _state_dict(mapping, D, P, clip_length, n_pos):
    dims = synth.GPT2_TINY if n_pos == synth.GPT2_TINY.n_pos else DIMS_256
    return synth.hot_state_dict(13, mapping, D, P, clip_length, 2, dims), dims


def _ragged(B, L, vocab, gen):
    """[B, L] right-padded captions: the first of length L, the others shorter"""
    lens = [L] + [max(1, (2 * L) // 3 - 3 * r) for r in range(B - 1)]
    tokens = torch.zeros(B, L, dtype=torch.int64)
    for r, n in enumerate(lens):
        tokens[r, :n] = torch.randint(1, vocab, (n,), generator=gen)
    return tokens


def _mask(P, tokens):
    return torch.cat((torch.ones(tokens.shape[0], P), (tokens != 0).float()), dim=1)


def _drop_masks(gen, dims, B, S):
    from oracle import capdec_oracle as O
    sites = O.dropout_sites(dims.n_layer, B, S, dims.n_embd, dims.n_head)
    flat = (torch.rand(sum(int(np.prod(sh)) for _, sh in sites), generator=gen) >= 0.1).to(torch.uint8)
    masks, o = [], 0
    for _, sh in sites:
        k = int(np.prod(sh))
        masks.append(flat[o:o + k].reshape(sh))
        o += k
    return flat, masks


def gpt_batch(S, B, scope):
    """tokens, mask, prefix, (flat, masks) or None, and the model's state dict / dims for one GPT-2-side case"""
    sd, dims = _state_dict("mlp", D_MLP, P_GPT, P_GPT, synth.GPT2_TINY.n_pos if S <= synth.GPT2_TINY.n_pos else TRAIN_MAX_S)
    gen = torch.Generator().manual_seed(1000 * S + B)
    tokens = _ragged(B, S - P_GPT, dims.vocab, gen)
    prefix = synth.synthetic_clip_embeddings(B, D_MLP, seed=S + B)
    drop = _drop_masks(gen, dims, B, S) if scope == "full_dropout" else None
    return tokens, _mask(P_GPT, tokens), prefix, drop, sd, dims


# The ReLU allowance of ``compare`` is a condition, not a measurement: with this seed no fc1 pre-activation of any mapper case
# switches sign between the float32 and the float64 oracle (every e32 <= 5e-6; the smallest |pre-activation| over the five
# geometries is 6.6e-7 in float64).  Seed base 0 had such a switch at 64 + 65 (e32 7e-3 on layers.0.mlp.fc1.weight).
MAPPER_PREFIX_SEED = 1000


def mapper_batch(clip_length, P):
    sd, dims = _state_dict("transformer_encoder", D_TM, P, clip_length, synth.GPT2_TINY.n_pos)
    gen = torch.Generator().manual_seed(1000 * clip_length + P)
    tokens = _ragged(2, 6, dims.vocab, gen)
    return tokens, _mask(P, tokens), synth.synthetic_clip_embeddings(2, D_TM, seed=MAPPER_PREFIX_SEED + clip_length + P), sd, dims


def references(sd, tokens, prefix, mapping, P, dims, clip_length, train_gpt, drop):
    """(loss64, grads64, e32 per tensor): the oracle in float64, and how far its own float32 run lies from that"""
    from oracle import capdec_oracle as O
    sd64 = {k: v.double() for k, v in sd.items()}
    kw = dict(n_head=dims.n_head, clip_length=clip_length, num_layers=2, train_gpt=train_gpt)
    loss64, g64 = O.train_step_loss_and_grads(sd64, tokens, prefix.double(), mapping, P, drop=drop, **kw)
    loss32, g32 = O.train_step_loss_and_grads(sd, tokens, prefix, mapping, P, drop=drop, **kw)
    del loss32              # (one label at logits of this size: torch's own fp32 loss is up to 2.5e-5 from the float64 one)
    e32 = {k: float((g32[k].double() - g64[k]).abs().max()) / float(g64[k].abs().max()) for k in g64}
    return float(loss64), g64, e32


def _report(line):
    from tests.test_hip_parity import _report as report
    report(line)


def compare(tag, loss, got, ref, strip="", relu_allowance=False):
    """loss within LOSS_TOL; every tensor entry by entry within 32 max(e32, 4e-6) of its largest entry; every norm within
    NORM_TOL.  ``relu_allowance`` (TransformerMapper cases, ``clip_project.*`` only): a ReLU whose pre-activation lies
    within fp32 round-off of zero switches between two correct fp32 pipelines; ONE such (token, unit) pair moves one row
    of that fc1's weight gradient and that token's share of everything upstream by a little (the reason documented in
    test_train_step_long_sequences_vs_oracle).  Allowed: at most max(8, 0.2 %) of a tensor's entries beyond the bar, each
    of them within 2e-2 -- the norm stays strict, and no GPT-2 tensor and no MLP-mapper case has the allowance.  (On the
    batches of this file no tensor has needed it: profiles/train_attention_forms.txt.)"""
    loss64, g64, e32 = ref
    name = lambda k: k[len(strip):] if strip and k.startswith(strip) else k      # noqa: E731
    assert sorted(name(k) for k in g64) == sorted(got)
    worst, worst_k, worst_norm, worst_e32, allowed = 0.0, "", 0.0, 0.0, []
    failures = []
    for k, want in g64.items():
        gk = got[name(k)].cpu().double()
        scale = float(want.abs().max())
        # (the reference itself: a bar beyond the older tests' 3e-3 would mean the two oracle runs disagree on a ReLU)
        assert scale > 0.0 and FACTOR * e32[k] < OLD_BAR, (tag, k, scale, e32[k])
        bar = FACTOR * max(e32[k], E32_FLOOR)
        dev = (gk - want).abs() / scale
        ratio = float(dev.max()) / bar
        over = int((dev > bar).sum())
        nrm = abs(float(gk.norm()) / float(want.norm()) - 1.0)
        worst_norm, worst_e32 = max(worst_norm, nrm), max(worst_e32, e32[k])
        if over and relu_allowance and k.startswith("clip_project.") and \
                over <= max(8, int(2e-3 * dev.numel())) and float(dev.max()) < 2e-2:
            allowed.append(f"{name(k)}: {over}/{dev.numel()} max {float(dev.max()):.2e}")
        else:
            if ratio > worst:
                worst, worst_k = ratio, name(k)
            if over:
                failures.append((k, over, dev.numel(), float(dev.max()), bar))
        if nrm >= NORM_TOL:
            failures.append((k, "norm", nrm))
    dl = abs(loss - loss64)
    knob = os.environ.get("CAPDEC_TRAIN_ATTN_BLK")
    _report(f"[train attention forms{', CAPDEC_TRAIN_ATTN_BLK=' + knob if knob else ''}] {tag}: {len(g64)} tensors, "
            f"worst entry deviation / bar {worst:.3f} ({worst_k}), worst e32 {worst_e32:.1e}, "
            f"worst |norm ratio - 1| {worst_norm:.1e}, |loss - fp64| {dl:.1e}"
            + (f"; ReLU near-tie allowance used by {len(allowed)}: " + "; ".join(allowed) if allowed else ""))
    assert dl < LOSS_TOL, (tag, loss, loss64)
    assert not failures, (tag, failures[:6])


# ------------------------------------------------------------------------------------------- GPU cases
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    for m in _MODELS.values():
        m.release()
    _MODELS.clear()


def _gpt_model(scope, sd, dims):
    """one model (and device context) per (scope, geometry): the cases differ in their batches only"""
    from capdec_amd.gpt2_prefix import ClipCaptionModel, ClipCaptionPrefix, MappingType
    key = (scope, dims.n_pos)
    if key not in _MODELS:
        cls = ClipCaptionPrefix if scope == "frozen" else ClipCaptionModel
        m = cls(P_GPT, clip_length=P_GPT, prefix_size=D_MLP, num_layers=2, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0")
        m.load_state_dict(sd)
        m.train()
        _MODELS[key] = m
    return _MODELS[key]


def _gpt_step(model, tokens, mask, prefix, drop):
    from capdec_amd import train as Tr
    opt = Tr.AdamW(model.parameters(), lr=1e-3)
    return Tr.train_step(model, opt, tokens, mask, prefix, apply_update=False, dropout_masks=drop[0] if drop else None)


@pytest.mark.gpu
@pytest.mark.parametrize("scope", GPT_SCOPES)
@pytest.mark.parametrize("S,B", GPT_CASES, ids=[f"S{S}-B{B}" for S, B in GPT_CASES])
def test_gpt2_side_vs_fp64(S, B, scope):
    """GPT-2's causal attention (HD 64) through the train step: MLP mapper (tanh: no ReLU ties), P = 10, ragged captions.
    full_dropout: GPT-2 trained, dropout 0.1 under injected keep-masks -- train_attn_fwd / train_attn_bwd with a mask;
    frozen: ClipCaptionPrefix -- the prefill kernel forward, train_attn_bwd without a mask.  No allowance anywhere."""
    from capdec_amd import train as Tr
    tokens, mask, prefix, drop, sd, dims = gpt_batch(S, B, scope)
    assert tokens.shape == (B, S - P_GPT) and int((tokens[0] != 0).sum()) == S - P_GPT
    full = scope == "full_dropout"
    ref = references(sd, tokens, prefix, "mlp", P_GPT, dims, P_GPT, full, (0.1, drop[1]) if drop else None)
    model = _gpt_model(scope, sd, dims)
    loss = _gpt_step(model, tokens, mask, prefix, drop)
    got = Tr.all_gradients(model) if full else Tr.mapper_gradients(model)
    fwd, bwd = attention_forms(64, S, os.environ.get("CAPDEC_TRAIN_ATTN_BLK") != "0")
    compare(f"GPT-2 S={S} B={B} {scope} (forward {fwd if full else 'prefill'}, backward {bwd})", loss, got, ref,
            strip="" if full else "clip_project.")


def _mapper_model(clip_length, P, scope, sd, dims):
    from capdec_amd.gpt2_prefix import ClipCaptionModel, ClipCaptionPrefix, MappingType
    cls = ClipCaptionPrefix if scope == "frozen" else ClipCaptionModel
    m = cls(P, clip_length=clip_length, prefix_size=D_TM, num_layers=2, mapping_type=MappingType.TransformerEncoder,
            gpt2_dims=dims).to("cuda:0")
    m.load_state_dict(sd)
    m.train()
    m.gpt.config.resid_pdrop = m.gpt.config.embd_pdrop = m.gpt.config.attn_pdrop = 0.0
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("clip_length,P,scope", MAPPER_CASES, ids=[f"{c}+{p}-{s}" for c, p, s in MAPPER_CASES])
def test_mapper_side_vs_fp64(clip_length, P, scope):
    """The TransformerMapper's bidirectional attention (HD 96) at clip_length + P positions: two layers, D = 640, two
    captions of at most 6 tokens on the tiny GPT-2.  frozen: the mapper's tensors; full: GPT-2 trained too, no dropout."""
    from capdec_amd import train as Tr
    tokens, mask, prefix, sd, dims = mapper_batch(clip_length, P)
    full = scope == "full"
    ref = references(sd, tokens, prefix, "transformer_encoder", P, dims, clip_length, full, None)
    model = _mapper_model(clip_length, P, scope, sd, dims)
    try:
        loss = Tr.train_step(model, Tr.AdamW(model.parameters(), lr=1e-3), tokens, mask, prefix, apply_update=False)
        got = Tr.all_gradients(model) if full else Tr.mapper_gradients(model)
        got = {k: v.cpu() for k, v in got.items()}
    finally:
        model.release()
    fwd, bwd = attention_forms(96, clip_length + P, os.environ.get("CAPDEC_TRAIN_ATTN_BLK") != "0")
    compare(f"mapper {clip_length}+{P} {scope} (forward {fwd}, backward {bwd})", loss, got, ref,
            strip="" if full else "clip_project.", relu_allowance=True)


N_FP64_CASES = len(GPT_CASES) * len(GPT_SCOPES) + len(MAPPER_CASES)


@pytest.mark.gpu
def test_the_wavefront_family_on_the_same_batches():
    """CAPDEC_TRAIN_ATTN_BLK=0 (and nothing else) in a child process: every case above again with the per-query / per-key
    wavefront kernels at EVERY length -- they meet S = 90 and S = 102 with their second 64-key slot -- held to the same
    float64 numbers on identical inputs"""
    env = dict(os.environ, CAPDEC_TRAIN_ATTN_BLK="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "vs_fp64",
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:]
    assert r.returncode == 0 and f"{N_FP64_CASES} passed" in tail and "failed" not in tail and "skipped" not in tail, tail


# ------------------------------------------------------------------------------------------- refusals
@pytest.mark.gpu
@pytest.mark.parametrize("n_pos", [TRAIN_MAX_S, synth.GPT2_TINY.n_pos])
def test_gpt2_sequence_past_the_limit_is_refused_and_the_context_lives_on(n_pos):
    """S = 257 on the n_pos = 256 model (train_step's own limit) and S = n_pos + 1 on the tiny model: CapdecError, and the
    same context then returns the loss of the valid step before, bit for bit"""
    from capdec_amd._capi import CapdecError
    tokens, mask, prefix, _, sd, dims = gpt_batch(n_pos, 2, "frozen")
    assert dims.n_pos == n_pos
    model = _gpt_model("frozen", sd, dims)
    before = _gpt_step(model, tokens, mask, prefix, None)
    longer = _ragged(2, n_pos + 1 - P_GPT, dims.vocab, torch.Generator().manual_seed(3))
    with pytest.raises(CapdecError, match="bad batch geometry"):
        _gpt_step(model, longer, _mask(P_GPT, longer), prefix, None)
    assert _gpt_step(model, tokens, mask, prefix, None) == before


@pytest.mark.gpu
def test_mapper_sequence_past_the_lds_is_refused_and_the_context_lives_on():
    """A TransformerMapper of 103 + 102 = 205 positions, loaded into the context of a 102 + 102 model: its forward needs
    more than 160 KiB of LDS and the step is refused (CapdecError, no launch); with the 204-position mapper loaded again
    the context returns the loss it returned before, bit for bit"""
    from capdec_amd import train as Tr
    from capdec_amd._capi import CapdecError
    clip_bad, P = MAPPER_REFUSED
    clip_length = MAPPER_FWD_MAX - P
    assert clip_length + P == MAPPER_FWD_MAX and clip_bad + P == MAPPER_FWD_MAX + 1 and mapper_fwd_bytes(96, clip_bad + P) > MAPPER_LDS_MAX
    tokens, mask, prefix, sd, dims = mapper_batch(clip_length, P)
    model = _mapper_model(clip_length, P, "frozen", sd, dims)
    try:
        opt = Tr.AdamW(model.parameters(), lr=1e-3)
        before = Tr.train_step(model, opt, tokens, mask, prefix, apply_update=False)
        bad = synth.hot_transformer_mapper_state_dict(14, D_TM, P, clip_bad, 2, dims.n_embd)
        model.engine.load_mapper_transformer(bad)
        with pytest.raises(CapdecError, match="sequence too long for LDS"):
            Tr.train_step(model, opt, tokens, mask, prefix, apply_update=False)
        model.engine.load_mapper_transformer({k: v for k, v in sd.items() if k.startswith("clip_project.")})
        assert Tr.train_step(model, opt, tokens, mask, prefix, apply_update=False) == before
    finally:
        model.release()
