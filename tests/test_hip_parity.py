"""Parity of the HIP path (through the C ABI / ctypes) against the CPU oracle and the golden
fixtures captured from the reference.  Needs an MI355X: ``pytest -m gpu``.

Tolerances (fp32 path): token ids / lengths / beam order bit-exact; beam mean-log-prob
scores 1e-4 (north_star); logits 2e-4 abs; mapper outputs 2e-4 abs."""
import os

import numpy as np
import pytest
import torch

from capdec_amd import synth

pytestmark = pytest.mark.gpu

T = torch.from_numpy


@pytest.fixture(scope="module")
def eng():
    from capdec_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _model(dims, mapping, D, seed=42, P=10, clip_length=10, num_layers=8):
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    mt = {"mlp": MappingType.MLP, "transformer_encoder": MappingType.TransformerEncoder}[mapping]
    m = ClipCaptionModel(P, clip_length=clip_length, prefix_dim=D, num_layers=num_layers, mapping_type=mt,
                         gpt2_dims=dims).to("cuda:0").eval()
    sd = synth.hot_state_dict(seed, mapping, D, P, clip_length, num_layers, dims)
    m.load_state_dict(sd)
    return m, sd


class FakeTok:
    def __init__(self, stop):
        self.stop = stop

    def encode(self, s):
        return [self.stop]

    def decode(self, ids):
        return " ".join(str(int(i)) for i in ids)


# ----------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,N,K", [(1, 8, 32), (5, 130, 64), (128, 128, 768), (257, 1531, 768), (300, 2304, 768),
                                   (77, 768, 3072), (1000, 50257, 768)])
def test_gemm_f32_vs_fp64(eng, M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N)
    a = torch.randn(M, K, generator=g)
    bt = torch.randn(N, K, generator=g) * 0.1
    # asymmetric operands: a transposed / row-col swapped result cannot pass
    ref = (a.double() @ bt.double().t())
    out = eng.gemm(a, bt).cpu()
    scale = (a.abs().double() @ bt.abs().double().t())
    assert float(((out.double() - ref).abs() / scale).max()) < 5e-7      # fp32 round-off class


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_gemm_epilogues(eng, act):
    from oracle import capdec_oracle as O
    g = torch.Generator().manual_seed(act)
    M, N, K = 193, 333, 96
    a, bt = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.3
    bias, resid = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    y = a @ bt.t() + bias
    y = [y, torch.tanh(y), torch.relu(y), O.gelu_new(y)][act] + resid
    out = eng.gemm(a, bt, bias=bias, resid=resid, act=act).cpu()
    np.testing.assert_allclose(out.numpy(), y.numpy(), atol=2e-5, rtol=1e-5)


# ----------------------------------------------------------------------------------- mappers
@pytest.mark.parametrize("D", [512, 640])
def test_mlp_mapper(eng, golden, D):
    g = golden("mappers")
    eng.load_mapper_mlp(synth.hot_mlp_mapper_state_dict(43, D, 10))
    y = eng.mapper_forward(T(g[f"x_{D}"])).cpu().reshape(4, -1)
    np.testing.assert_allclose(y.numpy(), g[f"mlp_{D}"], atol=2e-5)


@pytest.mark.parametrize("D", [512, 640])
def test_transformer_mapper(eng, golden, D):
    g = golden("mappers")
    eng.load_mapper_transformer(synth.hot_transformer_mapper_state_dict(43, D, 10, 10, 8))
    y = eng.mapper_forward(T(g[f"x_{D}"])).cpu()
    np.testing.assert_allclose(y.numpy(), g[f"tm_{D}"], atol=2e-4)


def test_transformer_mapper_ragged_geometry(eng, golden):
    g = golden("mappers")
    eng.load_mapper_transformer(synth.hot_transformer_mapper_state_dict(44, 512, 5, 7, 3))
    y = eng.mapper_forward(T(g["x_p5"])).cpu()
    assert y.shape == (3, 5, 768)
    np.testing.assert_allclose(y.numpy(), g["tm_p5"], atol=2e-4)


def test_mapper_long_sequence_vs_oracle(eng):
    """prefix_length 40 + clip_length 40 (the notebook's geometry): 80-token sequences"""
    from oracle import capdec_oracle as O
    sd = synth.hot_transformer_mapper_state_dict(9, 512, 40, 40, 2)
    x = synth.synthetic_clip_embeddings(3, 512, seed=3)
    eng.load_mapper_transformer(sd)
    y = eng.mapper_forward(x).cpu()
    np.testing.assert_allclose(y.numpy(), O.transformer_mapper(x, sd, 40, 2).numpy(), atol=3e-4)


def test_mapper_empty_batch(eng):
    eng.load_mapper_mlp(synth.hot_mlp_mapper_state_dict(43, 512, 10))
    assert eng.mapper_forward(torch.zeros(0, 512)).shape == (0, 10, 768)


# ----------------------------------------------------------------------------------- noise
def test_noise_injection(golden):
    from capdec_amd import train as ct
    g = golden("noise")
    x, noise, u = T(g["x"]).cuda(), T(g["noise"]), T(g["u"])
    off = T(g["offset_to_add_in_training"])
    assert ct.noise_injection(x, 0.0) is x
    np.testing.assert_allclose(ct.noise_injection(x, 0.016, noise=noise).cpu().numpy(), g["v016"], atol=1e-6)
    np.testing.assert_allclose(ct.noise_injection(x, 0.016, off, noise=noise).cpu().numpy(), g["v016_off"], atol=1e-6)
    np.testing.assert_allclose(ct.noise_injection(x, 0.016, dont_norm=True, noise=noise).cpu().numpy(),
                               g["v016_dontnorm"], atol=1e-6)
    np.testing.assert_allclose(ct.noise_injection(x, 0.016, uniform_noise=True, noise=noise, u=u).cpu().numpy(),
                               g["v016_uniform"], atol=1e-6)
    np.testing.assert_allclose(ct.get_uniform_ball_noise((6, 640), 0.3, noise=noise, u=u).cpu().numpy(), g["ball"],
                               atol=1e-6)


def test_noise_statistics_philox():
    """on-device Philox draw: RNG streams differ between back-ends, so pin the distribution:
    for unit rows and sigma^2 = 0.016 at D = 512 the pre-normalisation noise norm is
    sqrt(512 * 0.016) = 2.86 and outputs are unit-norm, seed-repeatable."""
    from capdec_amd import train as ct
    x = synth.synthetic_clip_embeddings(4096, 512, seed=0).cuda()
    a = ct.noise_injection(x, 0.016, seed=123)
    b = ct.noise_injection(x, 0.016, seed=123)
    c = ct.noise_injection(x, 0.016, seed=124)
    assert torch.equal(a, b) and not torch.equal(a, c)
    np.testing.assert_allclose(a.norm(dim=1).cpu().numpy(), 1.0, atol=1e-5)
    # zeros + N(0,1), normalised -> uniform direction: component mean 0, variance 1/512
    from capdec_amd.engine import get_engine
    v = get_engine(0).noise_inject(torch.zeros(20000, 512).cuda(), 1.0, None, False, True, seed=77).cpu().numpy()
    assert abs(v.mean()) < 1e-3 and abs(v.var() * 512 - 1.0) < 0.02
    cos = (a * x).sum(1).cpu().numpy()                               # E[cos] ~ 1 / sqrt(1 + 512 * 0.016)
    assert abs(cos.mean() - 1 / np.sqrt(1 + 512 * 0.016)) < 0.01


def test_normalize_prefix(eng, golden):
    g = golden("noise")
    x = T(g["x"])
    off = T(g["offset_to_add_in_inference"])
    y = eng.normalize_prefix(x, True, off).cpu()
    ref = x / x.norm(2, -1, keepdim=True) + off
    np.testing.assert_allclose(y.numpy(), ref.numpy(), atol=1e-6)
    np.testing.assert_array_equal(eng.normalize_prefix(x, False, None).cpu().numpy(), x.numpy())


# ----------------------------------------------------------------------------------- GPT-2 logits
def _check_logits(eng, g, dims):
    sd = synth.hot_gpt2_state_dict(42, dims)
    assert synth.state_dict_checksum(sd) == int(g["gpt_crc"]), "RNG drift: weights differ from fixture"
    eng.load_gpt2(sd)
    for L in (1, 10, 23, 77):
        x = T(g[f"x_L{L}"])
        full = eng.gpt2_logits(x, all_positions=True).cpu()
        last = eng.gpt2_logits(x, all_positions=False).cpu()
        np.testing.assert_array_equal(full[:, -1].numpy(), last.numpy())
        np.testing.assert_allclose(last[:, ::5].numpy(), g[f"last_sub_L{L}"], atol=2e-4)
        np.testing.assert_array_equal(last.topk(8, -1).indices.numpy(), g[f"top_i_L{L}"])
        np.testing.assert_allclose(torch.logsumexp(last, -1).numpy(), g[f"lse_L{L}"], atol=1e-4)
        step = max(1, dims.vocab // 64)
        np.testing.assert_allclose(full[:, :, ::step].numpy(), g[f"allpos_sub_L{L}"], atol=2e-4)


def test_gpt2_logits_tiny(eng, golden):
    _check_logits(eng, golden("gpt2_logits_tiny"), synth.GPT2_TINY)


def test_gpt2_logits_small(eng, golden):
    _check_logits(eng, golden("gpt2_logits_small"), synth.GPT2_SMALL)


def test_gpt2_logits_every_prefill_attention_form_vs_oracle(eng):
    """capdec_gpt2_logits over sequence lengths that take every form of the prefill attention: the per-row wavefront kernel
    (L = 10, 23; and L = 160, beyond the matrix-core kernel's four key tiles) and the matrix-core kernel with one to four
    key tiles (L = 24, 33, 64, 65, 96, 97, 128 -- the last ones need more than 64 KB of dynamic LDS), ragged batch of 3;
    causal masking across tile borders; every position's logits against the oracle"""
    from oracle import capdec_oracle as O
    dims = synth.GPT2Dims(n_layer=2, vocab=1531, n_pos=256)
    sd = synth.hot_gpt2_state_dict(42, dims)
    eng.load_gpt2(sd)
    gen = torch.Generator().manual_seed(5)
    for L in (10, 23, 24, 33, 64, 65, 96, 97, 128, 160):
        x = torch.randn(3, L, dims.n_embd, generator=gen) * 0.6
        got = eng.gpt2_logits(x, all_positions=True).cpu()
        want = O.gpt2_logits(x, sd, dims.n_head)
        np.testing.assert_allclose(got.numpy(), want.numpy(), atol=3e-4, err_msg=f"L = {L}")


def test_wte_lookup(eng):
    sd = synth.hot_gpt2_state_dict(42, synth.GPT2_TINY)
    eng.load_gpt2(sd)
    ids = torch.tensor([[0, 5, 1530], [7, 7, 3]])
    np.testing.assert_array_equal(eng.wte(ids).cpu().numpy(), sd["gpt.transformer.wte.weight"][ids].numpy())


# ----------------------------------------------------------------------------------- decode vs golden
def _check_decode(g, dims):
    from capdec_amd import gpt2_prefix_eval as E
    # greedy: config-1 shape (8 x 640-d, MLP mapper)
    model, sd = _model(dims, "mlp", 640)
    assert synth.state_dict_checksum(sd) == int(g["greedy_sd_crc"]), "RNG drift"
    pe = model.clip_project(T(g["greedy_x"])).reshape(8, 10, -1)
    np.testing.assert_allclose(pe.cpu().numpy(), g["greedy_prefix_embed"], atol=2e-5)
    pe = T(g["greedy_prefix_embed"])           # decode from the reference's own fp32 prefix
    stop = int(g["greedy_stop_id"])
    for el in (12, 67):
        ids, lens = E.decode_greedy_ids(model, pe, stop, el)
        np.testing.assert_array_equal(lens.cpu().numpy(), g[f"greedy_lens_T{el}"])
        np.testing.assert_array_equal(ids.cpu().numpy(), g[f"greedy_ids_T{el}"])
    ids, lens = E.decode_greedy_ids(model, pe, dims.vocab + 5, 67, alt_stop_id=-1)
    np.testing.assert_array_equal(ids.cpu().numpy(), g["greedy_ids_nostop"])
    # reference signature, one caption at a time
    for r in range(8):
        n = int(g["greedy_lens_T12"][r])
        want = " ".join(str(int(v)) for v in g["greedy_ids_T12"][r][:n])
        if n == 1:
            with pytest.raises(TypeError):      # reference :191 raises when the first token stops
                E.generate2(model, FakeTok(stop), embed=pe[r:r + 1], entry_length=12)
        else:
            assert E.generate2(model, FakeTok(stop), embed=pe[r:r + 1], entry_length=12) == want
    # beam: config-3 shape (512-d, TransformerMapper, beam 5)
    model, sd = _model(dims, "transformer_encoder", 512)
    assert synth.state_dict_checksum(sd) == int(g["beam_sd_crc"]), "RNG drift"
    nb = g["beam_x"].shape[0]
    pe = model.clip_project(T(g["beam_x"])).reshape(nb, 10, -1)
    np.testing.assert_allclose(pe.cpu().numpy(), g["beam_prefix_embed"], atol=2e-4)
    pe = T(g["beam_prefix_embed"])
    for el in (12, 67):
        for name, st in (("nostop", dims.vocab + 5), ("stop", int(g["beam_stop_id"]))):
            ids, lens, scores, order = E.decode_beam_ids(model, pe, st, 5, el)
            ids, lens, scores, order = (t.cpu().numpy() for t in (ids, lens, scores, order))
            gt, gl = g[f"beam_{name}_tokens_T{el}"], g[f"beam_{name}_seqlen_T{el}"]
            gs, go = g[f"beam_{name}_scores_T{el}"], g[f"beam_{name}_order_T{el}"]
            np.testing.assert_array_equal(order, go)                     # same beams, same ranking
            for r in range(nb):
                np.testing.assert_array_equal(ids[r], gt[r][go[r]])
                np.testing.assert_array_equal(lens[r], gl[r][go[r]].astype(np.int32))
                np.testing.assert_allclose(scores[r], gs[r][go[r]], atol=1e-4)
    st = int(g["beam_stop_id"])
    for r in range(nb):
        got = E.generate_beam(model, FakeTok(st), embed=pe[r:r + 1], entry_length=12)
        gt, gl, go = g["beam_stop_tokens_T12"][r], g["beam_stop_seqlen_T12"][r], g["beam_stop_order_T12"][r]
        want = [" ".join(str(int(v)) for v in gt[b][:int(gl[b])]) for b in go]
        assert got == want


def test_decode_tiny_vs_reference_golden(golden):
    _check_decode(golden("decode_tiny"), synth.GPT2_TINY)


@pytest.mark.parametrize("mode", ["f16x2", "bf16x3", "f32"])
def test_decode_small_vs_reference_golden(golden, mode, monkeypatch):
    """full GPT-2 small geometry (12 layers, V = 50257): greedy ids bit-identical to the reference, with the
    projections on the two-plane fp16 MFMA path (default, 3 MFMAs per product), on the three-plane bf16 path
    (6 MFMAs per product) and on the native fp32 MFMA path"""
    monkeypatch.setenv("CAPDEC_GEMM_MODE", mode)
    _check_decode(golden("decode_small"), synth.GPT2_SMALL)


class PromptTok(FakeTok):
    def encode(self, s):
        return [self.stop] if s == "." else [int(v) for v in s.split()]


@pytest.mark.parametrize("dims,tag", [(synth.GPT2_TINY, "tiny"), (synth.GPT2_SMALL, "small")], ids=["tiny", "small"])
def test_prompt_and_tokens_entry_vs_reference_golden(golden, dims, tag):
    """generate2(tokens=...), generate2(prompt=...), generate_beam(prompt=...) of the facade == strings captured from
    the reference (gpt2_prefix_eval.py:70-74,86-89,141-151): prompt ids stay in the output, generate_beam slices
    prompt + generated by the generated length"""
    from capdec_amd import gpt2_prefix_eval as E
    g = golden(f"prompt_{tag}")
    model, sd = _model(dims, "mlp", 512)
    assert synth.state_dict_checksum(sd) == int(g["sd_crc"]), "RNG drift"
    prompts = [list(map(int, row[:n])) for row, n in zip(g["prompts"], g["prompt_lens"])]
    for name, st in (("nostop", dims.vocab + 5), ("stop", int(g["stop_id"]))):
        for i, p in enumerate(prompts):
            want2, wantb = str(g[f"generate2_{name}"][i]), [str(t) for t in g[f"generate_beam_{name}"][i]]
            ptxt = " ".join(str(v) for v in p)
            assert E.generate2(model, PromptTok(st), tokens=torch.tensor([p]), entry_length=12) == want2
            assert E.generate2(model, PromptTok(st), prompt=ptxt, entry_length=12) == want2
            assert E.generate_beam(model, PromptTok(st), prompt=ptxt, entry_length=12) == wantb


@pytest.mark.parametrize("dims,tag", [(synth.GPT2_TINY, "tiny"), (synth.GPT2_SMALL, "small")], ids=["tiny", "small"])
def test_make_preds_driver_vs_reference_golden(golden, dims, tag, tmp_path):
    """A11: the batched driver (predictions_runner.caption_ids / make_preds = the reference's per-image loop
    :194-234,300-301) on the golden captions: embeddings -> clip_project -> decode -> ids / JSON must equal what the
    reference's generate2 / generate_beam(...)[0] produced one caption at a time -- as one batch (rank 0 of 1) and as
    the concatenation of a manual 2-way shard (the rank / world arithmetic without a process group)."""
    import json
    from capdec_amd import predictions_runner as PR, distributed as cdist
    g = golden(f"decode_{tag}")
    # ---- beam (config 3 shape): best beam per caption
    model, _ = _model(dims, "transformer_encoder", 512)
    x = T(g["beam_x"])
    nb = x.shape[0]
    for name, st, el in (("stop", int(g["beam_stop_id"]), 12), ("nostop", dims.vocab + 5, 67)):
        gt, gl = g[f"beam_{name}_tokens_T{el}"], g[f"beam_{name}_seqlen_T{el}"]
        go, gs = g[f"beam_{name}_order_T{el}"], g[f"beam_{name}_scores_T{el}"]
        want_ids = np.stack([gt[r][go[r][0]] for r in range(nb)])
        want_len = np.array([int(gl[r][go[r][0]]) for r in range(nb)])
        ids, lens, sc = PR.caption_ids(model, x, st, beam=True, entry_length=el, dont_normalize_prefix=True)
        np.testing.assert_array_equal(ids.cpu().numpy(), want_ids)
        np.testing.assert_array_equal(lens.cpu().numpy(), want_len)
        np.testing.assert_allclose(sc.cpu().numpy(), [gs[r][go[r][0]] for r in range(nb)], atol=1e-4)
        parts = [PR.caption_ids(model, x[slice(*cdist.shard_bounds(nb, r, 2))], st, beam=True, entry_length=el,
                                dont_normalize_prefix=True) for r in range(2)]
        np.testing.assert_array_equal(torch.cat([p[0] for p in parts]).cpu().numpy(), want_ids)
        np.testing.assert_array_equal(torch.cat([p[1] for p in parts]).cpu().numpy(), want_len)
    # the synthetic embeddings are unit-norm, so the reference's `prefix / prefix.norm()` (:222) moves them by <= 1 ulp:
    # the default (normalising) driver must produce the same captions
    st = int(g["beam_stop_id"])
    data = [{"image_id": 100 + r} for r in range(nb)]
    out = tmp_path / "preds.json"
    preds = PR.make_preds(data, x, model, FakeTok(st), str(out), beam=True, entry_length=12)
    gt, gl, go = g["beam_stop_tokens_T12"], g["beam_stop_seqlen_T12"], g["beam_stop_order_T12"]
    want = [{"caption": " ".join(str(int(v)) for v in gt[r][go[r][0]][:int(gl[r][go[r][0]])]), "image_id": 100 + r}
            for r in range(nb)]
    assert preds == want and json.load(open(out)) == want
    # the reference's Timer (predictions_runner.py:125-150) on the C ABI's hipEvent pair: one interval per batch
    timer = PR.Timer()
    for _ in range(2):
        assert PR.make_preds(data, x, model, FakeTok(st), None, beam=True, entry_length=12, timer=timer) == want
    assert timer.count == 2 and timer.items == 2 * nb and all(t > 0 for t in timer.timings)
    assert str(timer).startswith("mean: ") and " ms, std: " in str(timer)
    # ---- greedy (config 1 shape: 8 x 640-d, MLP mapper)
    model, _ = _model(dims, "mlp", 640)
    x = T(g["greedy_x"])
    st = int(g["greedy_stop_id"])
    for el in (12, 67):
        ids, lens, sc = PR.caption_ids(model, x, st, beam=False, entry_length=el, dont_normalize_prefix=True)
        assert sc is None
        np.testing.assert_array_equal(ids.cpu().numpy(), g[f"greedy_ids_T{el}"])
        np.testing.assert_array_equal(lens.cpu().numpy(), g[f"greedy_lens_T{el}"])
        parts = [PR.caption_ids(model, x, st, beam=False, entry_length=el, dont_normalize_prefix=True, rank=r, world=2)
                 for r in range(2)]                                  # rank / world arithmetic of the driver itself
        np.testing.assert_array_equal(torch.cat([p[0] for p in parts]).cpu().numpy(), g[f"greedy_ids_T{el}"])
    with pytest.raises(RuntimeError):                                # world > 1 without a process group is an error
        PR.make_preds([{"image_id": r} for r in range(8)], x, model, FakeTok(st), None, beam=False, rank=0, world=2)


@pytest.mark.parametrize("dims,tag", [(synth.GPT2_TINY, "tiny"), (synth.GPT2_SMALL, "small")], ids=["tiny", "small"])
def test_train_step_forward_vs_reference_golden(golden, dims, tag):
    """ClipCaptionModel.forward(tokens, prefix, mask) -- the forward of the reference's train step (train.py:251-260,348)
    on a right-padded batch built like train.ClipCocoDataset (:52-63): logits at every real position, their arg-max /
    logsumexp and the train loss (:349) equal the reference's; a mask that is not right padding is refused"""
    from capdec_amd._capi import CapdecError
    g = golden(f"train_forward_{tag}")
    model, sd = _model(dims, "mlp", 512)
    assert synth.state_dict_checksum(sd) == int(g["sd_crc"]), "RNG drift"
    tokens, prefix, mask = T(g["tokens"]), T(g["prefix"]), T(g["mask"])
    out = model(tokens, prefix, mask)
    logits = out.logits.cpu()
    assert logits.shape == (3, 10 + tokens.shape[1], dims.vocab) and out.loss is None
    ok = mask > 0
    step = max(1, dims.vocab // 97)
    np.testing.assert_allclose(logits[:, :, ::step][ok].numpy(), T(g["logits_sub"])[ok].numpy(), atol=2e-4)
    np.testing.assert_array_equal(logits.argmax(-1)[ok].numpy(), T(g["argmax"])[ok].numpy())
    np.testing.assert_allclose(torch.logsumexp(logits, -1)[ok].numpy(), T(g["lse"])[ok].numpy(), atol=1e-4)
    loss = torch.nn.functional.cross_entropy(logits[:, 9:-1].reshape(-1, logits.shape[-1]), tokens.flatten(), ignore_index=0)
    assert abs(float(loss) - float(g["train_loss"])) < 1e-4
    # rows without padding: GPT2LMHeadModel's own `labels=` loss is reproduced as well
    full = model(tokens[:1], prefix[:1], mask[:1], labels=tokens[:1])
    assert full.loss is not None and torch.isfinite(full.loss)
    lab = torch.cat((torch.zeros(1, 10, dtype=torch.int64), tokens[:1].long()), 1)[:, 1:]
    want = torch.nn.functional.cross_entropy(full.logits[:, :-1].reshape(-1, dims.vocab).cpu(), lab.reshape(-1))
    assert abs(float(full.loss) - float(want)) < 1e-4
    # the device cross-entropy is the train loss of train.py:349 (ignore_index = 0) when handed its slice and labels
    dl = model.engine.cross_entropy(out.logits[:, 9:-1], tokens, ignore_index=0)
    assert abs(float(dl) - float(g["train_loss"])) < 1e-4
    # a label outside the vocabulary (torch raises on it) must not be skipped like ignore_index: the loss turns NaN
    wrong = tokens.clone()
    wrong[0, 1] = dims.vocab + 3
    assert torch.isnan(model.engine.cross_entropy(out.logits[:, 9:-1], wrong, ignore_index=0)).item()
    bad = mask.clone()
    bad[1, 12] = 0                                               # a hole in the middle: not the dataset's mask
    with pytest.raises(CapdecError):
        model(tokens, prefix, bad)


@pytest.mark.parametrize("dims,tag,mapping,nlay", [(synth.GPT2_TINY, "tiny", "mlp", 8), (synth.GPT2_SMALL, "small", "mlp", 8),
                                                   (synth.GPT2_TINY, "tm_tiny", "transformer_encoder", 3)],
                         ids=["mlp_tiny", "mlp_small", "transformer_mapper_tiny"])
def test_train_step_frozen_gpt2_vs_reference_golden(golden, dims, tag, mapping, nlay):
    """The train step with a frozen GPT-2 (reference train.py:344-354 with --only_prefix; capdec_train_step): four
    consecutive iterations on the batches of tests/golden/train_step_*.npz -- the loss of every iteration, EVERY mapper
    gradient of every iteration (MLP: 4 tensors; TransformerMapper with three layers: 39) against what the reference's own
    loss.backward() left in .grad (each taken at the weights the previous updates produced), the lr sequence, and the
    weights after the four AdamW updates (the update rule itself is the restated transformers-4.24 AdamW:
    oracle/capdec_oracle.py adamw_transformers).  Then the trained mapper is what inference uses.  Tolerances: loss 3e-4;
    gradients 3e-3 of the tensor's largest entry on a 4096-entry subsample (TransformerMapper, last iteration: 5e-2 --
    fp32 round-off amplified by two Adam updates, see tests/test_oracle_vs_golden.py) + the norm within 2e-3; final
    weights 5e-5 abs."""
    from capdec_amd import train as Tr
    from capdec_amd.gpt2_prefix import ClipCaptionPrefix, MappingType
    from oracle import capdec_oracle as O
    g = golden(f"train_step_{tag}")
    sd = synth.hot_state_dict(42, mapping, 512, 10, 10, nlay, dims)
    assert synth.state_dict_checksum(sd) == int(g["sd_crc"]), "RNG drift"
    mt = MappingType.MLP if mapping == "mlp" else MappingType.TransformerEncoder
    model = ClipCaptionPrefix(10, clip_length=10, prefix_size=512, num_layers=nlay, mapping_type=mt, gpt2_dims=dims).to("cuda:0")
    model.load_state_dict(sd)
    model.train()
    opt = Tr.AdamW(model.parameters(), lr=float(g["lr"]))
    sched = Tr.get_linear_schedule_with_warmup(opt, int(g["warmup"]), int(g["total"]))
    names = [str(n) for n in g["names"]]
    for it in range(len(g["losses"])):
        tokens, mask, prefix = T(g[f"tokens_{it}"]), T(g[f"mask_{it}"]), T(g[f"prefix_{it}"])
        assert abs(opt.param_groups[0]["lr"] - float(g["lrs"][it])) < 1e-12
        loss = Tr.train_step(model, opt, tokens, mask, prefix)
        assert abs(loss - float(g["losses"][it])) < 3e-4, (it, loss, float(g["losses"][it]))
        grads = Tr.mapper_gradients(model)
        assert len(grads) == len(names)
        loose = mapping != "mlp" and it >= 3
        for k in names:
            gk = grads[k[len("clip_project."):]].cpu()
            flat = gk.flatten()
            sub = flat[::max(1, flat.numel() // 4096)].numpy()
            ref = g[f"grad_{it}_{k}_sub"]
            scale = float(np.abs(ref).max())
            np.testing.assert_allclose(sub, ref, atol=(5e-2 if loose else 3e-3) * scale + 1e-9, rtol=0, err_msg=f"iteration {it}, {k}")
            assert abs(float(gk.double().norm()) / float(g[f"grad_{it}_{k}_norm"]) - 1.0) < 2e-3, (it, k)
        sched.step()
    fin = model.state_dict()
    for k in names:
        flat = fin[k].flatten()
        np.testing.assert_allclose(flat[::max(1, flat.numel() // 4096)].numpy(), g[f"final_{k}_sub"], atol=5e-5, err_msg=k)
    # the trained mapper is the one inference runs
    x = T(g["prefix_0"])
    want = O.clip_project(x, {k: fin[k] for k in names}, mapping, 10, 10, nlay)
    np.testing.assert_allclose(model.clip_project(x).cpu().numpy().reshape(want.shape), want.numpy(), atol=2e-4)
    # a real token under a zero mask is refused (the reference's attention would hide what its loss reads)
    bad = T(g["mask_0"]).clone()
    bad[0, 10] = 0
    with pytest.raises(Exception):
        Tr.train_step(model, opt, T(g["tokens_0"]), bad, T(g["prefix_0"]))


def _full_model(dims, p_drop):
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    sd = synth.hot_state_dict(42, "mlp", 512, 10, dims=dims)
    model = ClipCaptionModel(10, clip_length=10, prefix_size=512, num_layers=8, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0")
    model.load_state_dict(sd)
    model.train()
    model.gpt.config.resid_pdrop = model.gpt.config.embd_pdrop = model.gpt.config.attn_pdrop = p_drop
    return model, sd


def _check_all_gradients(grads, g, names, key, sub=1024):
    assert sorted(grads) == sorted(names)
    for k in names:
        gk = grads[k].cpu()
        flat = gk.flatten()
        ref = g[key.format(k=k) + "_sub"]
        scale = float(np.abs(ref).max())
        np.testing.assert_allclose(flat[::max(1, flat.numel() // sub)].numpy(), ref, atol=3e-3 * scale + 1e-9, rtol=0, err_msg=k)
        assert abs(float(gk.double().norm()) / float(g[key.format(k=k) + "_norm"]) - 1.0) < 2e-3, k


def test_train_step_full_model_vs_reference_golden(golden):
    """capdec_train_set_scope(1), GPT2Config dropouts at 0: the reference's default train step without dropout.
    (a) gradients of all 32 tensors of the tiny model against the reference's loss.backward()
    (tests/golden/train_full_tiny.npz; Conv1D weights in the checkpoint's [in, out] layout); (b) three updates against the
    oracle's full-model loop: losses and every final tensor; (c) the scope survives a train_reset (state_dict() still pulls
    GPT-2's trained tensors); (d) an out-of-range token id raises and updates nothing."""
    from capdec_amd import train as Tr
    from oracle import capdec_oracle as O
    g = golden("train_full_tiny")
    dims = synth.GPT2_TINY
    model, sd = _full_model(dims, 0.0)
    assert synth.state_dict_checksum(sd) == int(g["sd_crc"]), "RNG drift"
    opt = Tr.AdamW(model.parameters(), lr=1e-3)
    loss = Tr.train_step(model, opt, T(g["tokens"]), T(g["mask"]), T(g["prefix"]), apply_update=False)
    assert abs(loss - float(g["loss"])) < 3e-4
    names = [str(n) for n in g["names"]]
    _check_all_gradients(Tr.all_gradients(model), g, names, "grad_{k}")
    # (b) three updates: oracle loop vs device
    batches = [(T(g["tokens"]), T(g["prefix"]))] * 3
    opt = Tr.AdamW(model.parameters(), lr=1e-4)
    model.engine.train_reset()
    want_losses, want_sd = O.train_steps(sd, batches, "mlp", 10, 1e-4, 0, 10, n_head=dims.n_head, train_gpt=True)
    sched = Tr.get_linear_schedule_with_warmup(opt, 0, 10)
    got = []
    for tok, pre in batches:
        got.append(Tr.train_step(model, opt, tok, T(g["mask"]), pre))
        sched.step()
    np.testing.assert_allclose(got, want_losses, atol=2e-2)
    assert got[2] < got[0]                                               # the same batch three times: the loss goes down
    last, total, n = model.engine.train_loss()
    assert n == 3 and abs(last - got[2]) < 1e-6 and abs(total - sum(got)) < 1e-3
    # (c) a fresh optimizer keeps the scope: the trained GPT-2 tensors can still be pulled back
    model.engine.train_reset()
    fin = model.state_dict()
    for k in names:        # (Adam's update of an entry whose gradient is of the order of eps is as sensitive as a sign: 3 lr at most)
        dev = np.abs(fin[k].numpy() - want_sd[k].numpy())
        assert float(dev.max()) <= 3.5e-4 and float((dev > 2e-5).mean()) < 0.01, (k, float(dev.max()), float((dev > 2e-5).mean()))
    # (d) an id outside the vocabulary: IndexError like the reference's embedding lookup, on a host or a device tensor,
    # and the device-side guard left every weight alone
    bad = T(g["tokens"]).clone()
    bad[1, 2] = dims.vocab + 7
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with pytest.raises(IndexError):
        Tr.train_step(model, opt, bad, T(g["mask"]), T(g["prefix"]))
    with pytest.raises(IndexError):
        Tr.train_step(model, opt, bad.cuda(), T(g["mask"]), T(g["prefix"]))
    model._device_ahead = True
    after = model.state_dict()
    for k in names:
        assert torch.equal(before[k], after[k]), k


def test_train_step_full_model_with_dropout_vs_reference_golden(golden):
    """The reference's default train step AS IT RUNS (train.py:344-350 on a ClipCaptionModel in train() mode: GPT-2's
    dropouts 0.1).  (a) injected masks -- the keep-masks recorded inside the reference's own F.dropout calls
    (tests/golden/train_full_dropout_tiny.npz): loss and the gradient of all 32 tensors equal the reference's
    loss.backward(), two batches; (b) the device's own mask stream (Philox): keep rate 1 - p on every site, a new stream
    every step, the same stream again after re-seeding, and the step it produced equals the oracle run with exactly those
    masks; (c) eval() mode turns dropout off like torch."""
    from capdec_amd import train as Tr
    from oracle import capdec_oracle as O
    from tests.test_oracle_vs_golden import unpack_dropout_masks
    g = golden("train_full_dropout_tiny")
    dims = synth.GPT2_TINY
    model, sd = _full_model(dims, float(g["p"]))
    assert synth.state_dict_checksum(sd) == int(g["sd_crc"]), "RNG drift"
    opt = Tr.AdamW(model.parameters(), lr=1e-3)
    names = [str(n) for n in g["names"]]
    for it in range(2):
        tokens, mask, prefix = T(g[f"tokens_{it}"]), T(g[f"mask_{it}"]), T(g[f"prefix_{it}"])
        flat, _ = unpack_dropout_masks(g, it, dims, tokens.shape[0], 10 + tokens.shape[1])
        loss = Tr.train_step(model, opt, tokens, mask, prefix, apply_update=False, dropout_masks=flat)
        assert abs(loss - float(g[f"loss_{it}"])) < 3e-4, (it, loss)
        _check_all_gradients(Tr.all_gradients(model), g, names, f"grad_{it}_" + "{k}")
    # (b) the Philox stream
    tokens, mask, prefix = T(g["tokens_0"]), T(g["mask_0"]), T(g["prefix_0"])
    B, S = tokens.shape[0], 10 + tokens.shape[1]
    n = model.engine.dropout_stream_size(B, S, dims.n_embd, dims.n_head, dims.n_layer)
    assert n == int(g["drop_n_0"])
    model.engine.train_set_dropout(0.1, 1234)
    l1 = Tr.train_step(model, opt, tokens, mask, prefix, apply_update=False)
    m1 = model.engine.train_get_dropout_masks(n).cpu()
    grads1 = Tr.all_gradients(model)
    l2 = Tr.train_step(model, opt, tokens, mask, prefix, apply_update=False)
    m2 = model.engine.train_get_dropout_masks(n).cpu()
    assert set(m1.unique().tolist()) <= {0, 1} and not torch.equal(m1, m2) and abs(l1 - l2) > 1e-4
    o = 0
    for name, shape in O.dropout_sites(dims.n_layer, B, S, dims.n_embd, dims.n_head):
        k = int(np.prod(shape))
        rate = float(m1[o:o + k].float().mean())
        assert abs(rate - 0.9) < 4.0 * (0.09 / k) ** 0.5 + 1e-3, (name, rate)
        o += k
    model.engine.train_set_dropout(0.1, 1234)
    l3 = Tr.train_step(model, opt, tokens, mask, prefix, apply_update=False)
    assert torch.equal(model.engine.train_get_dropout_masks(n).cpu(), m1) and l3 == l1
    masks, o = [], 0
    for _, shape in O.dropout_sites(dims.n_layer, B, S, dims.n_embd, dims.n_head):
        k = int(np.prod(shape))
        masks.append(m1[o:o + k].reshape(shape))
        o += k
    want_loss, want = O.train_step_loss_and_grads(sd, tokens, prefix, "mlp", 10, n_head=dims.n_head, train_gpt=True, drop=(0.1, masks))
    assert abs(l1 - float(want_loss)) < 3e-4
    for k in ("gpt.transformer.h.0.attn.c_attn.weight", "gpt.transformer.wte.weight", "clip_project.model.0.weight"):
        ref = want[k]
        np.testing.assert_allclose(grads1[k].cpu().numpy(), ref.numpy(), atol=3e-3 * float(ref.abs().max()), rtol=0, err_msg=k)
    # (c) eval(): no dropout -- the loss of the dropout-free step
    model.eval()
    l_eval = Tr.train_step(model, opt, tokens, mask, prefix, apply_update=False)
    want0, _ = O.train_step_loss_and_grads(sd, tokens, prefix, "mlp", 10, n_head=dims.n_head, train_gpt=True)
    assert abs(l_eval - float(want0)) < 3e-4 and abs(l_eval - l1) > 1e-3


def test_train_step_full_model_at_gpt2_small_geometry_vs_oracle():
    """The reference's default train step (train.py:344-354: GPT-2 trained too, dropouts 0.1) at the geometry it really runs
    at -- 12 layers, 768-d, V = 50 257: one step, batch 4, injected keep-masks.  The tied wte's gradient is the product the
    transposing packer feeds with the loss rows at a row stride of the PADDED vocabulary (50 304), a path the tiny
    geometry (V = 1531 -> 1536) cannot exercise.  Checker: the oracle's hand-written forward / backward, which is pinned to the
    reference's own loss.backward() at the tiny geometry (tests/golden/train_full*_tiny.npz).  Loss, every gradient's norm,
    and 4096-entry subsamples of wte, h.0.attn.c_attn.weight, h.11.mlp.c_proj.weight and ln_f.weight."""
    from capdec_amd import train as Tr
    from oracle import capdec_oracle as O
    dims = synth.GPT2_SMALL
    model, sd = _full_model(dims, 0.1)
    B, L, P = 4, 9, 10
    gen = torch.Generator().manual_seed(77)
    tokens = torch.randint(1, dims.vocab, (B, L), generator=gen)
    tokens[0, -1] = dims.vocab - 1                        # the last vocabulary row takes part (the padded tail must not)
    lens = torch.tensor([L, 7, 5, 8])
    tokens[torch.arange(L)[None, :] >= lens[:, None]] = 0
    mask = torch.cat((torch.ones(B, P), (tokens != 0).float()), dim=1)
    prefix = synth.synthetic_clip_embeddings(B, 512, seed=12)
    masks, flat = [], []
    for _, shape in O.dropout_sites(dims.n_layer, B, P + L, dims.n_embd, dims.n_head):
        m = (torch.rand(shape, generator=gen) >= 0.1).to(torch.uint8)
        masks.append(m)
        flat.append(m.flatten())
    flat = torch.cat(flat)
    assert flat.numel() == model.engine.dropout_stream_size(B, P + L, dims.n_embd, dims.n_head, dims.n_layer)
    want_loss, want = O.train_step_loss_and_grads(sd, tokens, prefix, "mlp", P, n_head=dims.n_head, train_gpt=True, drop=(0.1, masks))
    opt = Tr.AdamW(model.parameters(), lr=1e-3)
    loss = Tr.train_step(model, opt, tokens, mask, prefix, apply_update=False, dropout_masks=flat)
    assert abs(loss - float(want_loss)) < 3e-4, (loss, float(want_loss))
    grads = Tr.all_gradients(model)
    assert sorted(grads) == sorted(want)
    worst = 0.0
    for k, ref in want.items():
        r = float(grads[k].double().norm().cpu()) / max(float(ref.double().norm()), 1e-30)
        worst = max(worst, abs(r - 1.0))
        assert abs(r - 1.0) < 2e-3, (k, r)
    for k in ("gpt.transformer.wte.weight", "gpt.transformer.h.0.attn.c_attn.weight", "gpt.transformer.h.11.mlp.c_proj.weight",
              "gpt.transformer.ln_f.weight"):
        ref, got = want[k].flatten(), grads[k].cpu().flatten()
        step = max(1, ref.numel() // 4096)
        np.testing.assert_allclose(got[::step].numpy(), ref[::step].numpy(), atol=3e-3 * float(ref.abs().max()), rtol=0, err_msg=k)
    # the rows of wte the batch touched (token lookup + lm_head) and the LAST row, entry by entry
    gw, rw = grads["gpt.transformer.wte.weight"].cpu(), want["gpt.transformer.wte.weight"]
    rows = torch.unique(torch.cat((tokens.flatten(), torch.tensor([dims.vocab - 1, dims.vocab - 2, 0]))))
    np.testing.assert_allclose(gw[rows].numpy(), rw[rows].numpy(), atol=3e-3 * float(rw.abs().max()), rtol=0)
    _report("train step, full scope, GPT-2-small geometry (V = 50257): loss %.6f vs oracle %.6f; worst |gradient norm ratio - 1| over %d "
            "tensors %.2e" % (loss, float(want_loss), len(want), worst))


def test_train_step_long_sequences_vs_oracle():
    """Sequences beyond one wavefront's 64 lanes -- the reference's default geometry has prefix_length = clip_length = 40,
    i.e. 80-position TransformerMapper sequences and GPT-2 sequences of 40 + caption tokens -- where the block-form
    attention kernels run their second key slot per lane (the goldens above stop at 20 positions).  Tiny GPT-2, two mapper
    layers, batch of three ragged captions up to 30 tokens (GPT-2 sequences of 70): (a) frozen scope: loss and every mapper
    gradient against the oracle's hand-written backward (itself pinned against the reference's loss.backward() on the
    golden geometries); (b) full scope with dropout 0.1 under random injected keep-masks: every one of the tensors."""
    from capdec_amd import train as Tr
    from capdec_amd.gpt2_prefix import ClipCaptionModel, ClipCaptionPrefix, MappingType
    from oracle import capdec_oracle as O
    dims, P, D, nlay = synth.GPT2_TINY, 40, 640, 2
    sd = synth.hot_state_dict(13, "transformer_encoder", D, P, P, nlay, dims)
    g = torch.Generator().manual_seed(77)
    lens, L = [30, 17, 25], 30
    tokens = torch.zeros(3, L, dtype=torch.int64)
    mask = torch.zeros(3, P + L)
    mask[:, :P] = 1
    for r, n in enumerate(lens):
        tokens[r, :n] = torch.randint(1, dims.vocab, (n,), generator=g)
        mask[r, P:P + n] = 1
    prefix = synth.synthetic_clip_embeddings(3, D, seed=5)

    def compare(got, want, strip):
        # (the rule -- 3e-3 of the largest entry, norms within 2e-3, the ReLU near-tie allowance of the mapper's tensors -- is
        #  shared with test_train_rows.py: tests/train_compare_def.py)
        from tests.train_compare_def import compare_gradients
        compare_gradients(got, want, strip, "train long sequences", _report)

    # (a) frozen scope
    model = ClipCaptionPrefix(P, clip_length=P, prefix_size=D, num_layers=nlay, mapping_type=MappingType.TransformerEncoder,
                              gpt2_dims=dims).to("cuda:0")
    model.load_state_dict(sd)
    model.train()
    opt = Tr.AdamW(model.parameters(), lr=1e-3)
    loss = Tr.train_step(model, opt, tokens, mask, prefix, apply_update=False)
    want_loss, want = O.train_step_loss_and_grads(sd, tokens, prefix, "transformer_encoder", P, n_head=dims.n_head, clip_length=P,
                                                  num_layers=nlay)
    assert abs(loss - float(want_loss)) < 3e-4
    compare(Tr.mapper_gradients(model), want, "clip_project.")
    # (b) full scope, dropout 0.1 with injected masks
    full = ClipCaptionModel(P, clip_length=P, prefix_size=D, num_layers=nlay, mapping_type=MappingType.TransformerEncoder,
                            gpt2_dims=dims).to("cuda:0")
    full.load_state_dict(sd)
    full.train()
    sites = O.dropout_sites(dims.n_layer, 3, P + L, dims.n_embd, dims.n_head)
    n = sum(int(np.prod(sh)) for _, sh in sites)
    flat = (torch.rand(n, generator=g) >= 0.1).to(torch.uint8)
    masks, o = [], 0
    for _, sh in sites:
        k = int(np.prod(sh))
        masks.append(flat[o:o + k].reshape(sh))
        o += k
    loss2 = Tr.train_step(full, Tr.AdamW(full.parameters(), lr=1e-3), tokens, mask, prefix, apply_update=False, dropout_masks=flat)
    want_loss2, want2 = O.train_step_loss_and_grads(sd, tokens, prefix, "transformer_encoder", P, n_head=dims.n_head, clip_length=P,
                                                    num_layers=nlay, train_gpt=True, drop=(0.1, masks))
    assert abs(loss2 - float(want_loss2)) < 3e-4 and abs(loss2 - loss) > 1e-3
    compare(Tr.all_gradients(full), want2, "")


def test_train_step_on_the_native_fp32_gemm_and_the_wavefront_attention():
    """CAPDEC_TRAIN_F16X2=0 puts the backward GEMMs of the train step on the native fp32 MFMA kernel (the default is the
    fp32-accurate two-fp16-plane family) and CAPDEC_TRAIN_ATTN_BLK=0 its attention on the per-query wavefront kernels (the
    fallback of sequences beyond 128 positions; the default is one block per (sample, head)): the same goldens -- frozen
    scope with both mappers, full scope with and without dropout, the GPT-2-small-geometry case -- in a child process with
    both knobs"""
    import subprocess
    import sys
    env = dict(os.environ, CAPDEC_TRAIN_F16X2="0", CAPDEC_TRAIN_ATTN_BLK="0")
    sel = "(test_train_step_frozen_gpt2_vs_reference_golden and tiny) or test_train_step_full_model"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel,
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=900)
    tail = r.stdout[-1500:]
    assert r.returncode == 0 and "5 passed" in tail and "failed" not in tail, tail


def test_train_loop_with_validation_pass(tmp_path):
    """capdec_amd.train.train (reference train.py:317-392): two epochs of a ClipCaptionPrefix over an 8-item dataset with a
    validation dataset -- checkpoints under the reference's file names, loss_per_epoch.json = {'train': [...], 'val':
    [...]} with the epoch means (the train mean comes from the device's running sum: the steps are enqueued without a
    round trip), equal to the same loop run step by step with explicit waits"""
    import json
    from types import SimpleNamespace
    from capdec_amd import train as Tr
    from capdec_amd.gpt2_prefix import ClipCaptionPrefix, MappingType
    dims = synth.GPT2_TINY
    sd = synth.hot_state_dict(42, "mlp", 512, 10, dims=dims)
    gen = torch.Generator().manual_seed(5)

    class DS(torch.utils.data.Dataset):
        prefix_length = 10

        def __init__(self, n, seed):
            self.items = []
            x = synth.synthetic_clip_embeddings(n, 512, seed=seed)
            for i in range(n):
                L, k = 9, 3 + i % 6
                tok = torch.zeros(L, dtype=torch.int64)
                tok[:k] = torch.randint(1, dims.vocab, (k,), generator=gen)
                mask = torch.cat((torch.ones(10), (tok > 0).float()))
                self.items.append((tok, mask, x[i]))

        def __len__(self):
            return len(self.items)

        def __getitem__(self, i):
            return self.items[i]

    train_ds, val_ds = DS(8, 1), DS(4, 2)
    args = SimpleNamespace(bs=4, epochs=2, lr=1e-3, noise_variance=0.0, uniform_noise=False, dont_norm=False, save_every=1,
                           val_pt="")

    def fresh():
        m = ClipCaptionPrefix(10, clip_length=10, prefix_size=512, num_layers=8, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0")
        m.load_state_dict(sd)
        return m

    model = fresh()
    torch.manual_seed(11)
    Tr.train(train_ds, model, args, warmup_steps=1, output_dir=str(tmp_path), output_prefix="t", val_dataset=val_ds)
    rec = json.load(open(tmp_path / "loss_per_epoch.json"))
    assert sorted(rec) == ["train", "val"] and len(rec["train"]) == len(rec["val"]) == 2
    assert (tmp_path / "t-000.pt").exists() and (tmp_path / "t-001.pt").exists()
    # the same loop, step by step
    ref = fresh()
    ref.train()
    torch.manual_seed(11)
    opt = Tr.AdamW(ref.parameters(), lr=args.lr)
    loader = torch.utils.data.DataLoader(train_ds, batch_size=4, shuffle=True, drop_last=True)
    sched = Tr.get_linear_schedule_with_warmup(opt, 1, 2 * len(loader))
    for epoch in range(2):
        acc = 0.0
        for tok, mask, prefix in loader:
            acc += Tr.train_step(ref, opt, tok, mask, prefix.to("cuda:0"))
            sched.step()
        assert abs(acc / len(loader) - rec["train"][epoch]) < 1e-4, (epoch, acc / len(loader), rec["train"])
        v = Tr.validation_loss(ref, val_ds, 4)
        assert abs(v - rec["val"][epoch]) < 1e-4
    saved = torch.load(tmp_path / "t-001.pt")
    for k, v in ref.state_dict().items():
        if k.startswith("clip_project."):
            np.testing.assert_allclose(saved[k].numpy(), v.numpy(), atol=1e-6)
    assert rec["train"][1] < rec["train"][0]
    with pytest.raises(Exception):
        Tr.train(train_ds, model, SimpleNamespace(**dict(vars(args), val_pt="val.pkl")), output_dir=str(tmp_path))


@pytest.mark.parametrize("mode", ["f16x2", "bf16x3", "f32"])
def test_gemm_modes_vs_fp64(mode):
    """every fp32-accurate GEMM back-end stays in the fp32 round-off class (error relative to sum |a||b|)"""
    from capdec_amd.engine import Engine
    e = Engine(0)
    e.set_gemm_mode(mode)
    assert e.gemm_mode() == mode
    g = torch.Generator().manual_seed(5)
    for (M, N, K) in [(300, 1531, 768), (129, 257, 3072), (64, 64, 64), (1000, 768, 640)]:
        a = torch.randn(M, K, generator=g) * torch.logspace(-3, 3, K)       # wide dynamic range across k
        bt = torch.randn(N, K, generator=g) * 0.1
        ref = a.double() @ bt.double().t()
        scale = a.abs().double() @ bt.abs().double().t()
        out = e.gemm(a, bt).cpu().double()
        assert float(((out - ref).abs() / scale).max()) < 5e-7, (mode, M, N, K)
    e.close()


@pytest.mark.parametrize("mode", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("N", [1024, 1001, 130])
def test_gemm_packed_a_path(N, mode, monkeypatch):
    """the packed-A LDS-DMA kernels (both operands pre-split, transposed accumulator layout) through the test hook:
    float4 epilogue (N % 4 == 0) and the scalar tail path, bias + activation + residual, ragged M"""
    from capdec_amd.engine import Engine
    from oracle import capdec_oracle as O
    monkeypatch.setenv("CAPDEC_HOOK_PACKA", "1")
    eng = Engine(0)
    eng.set_gemm_mode(mode)
    g = torch.Generator().manual_seed(N)
    M, K = 333, 256
    a, bt = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.2
    bias, resid = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    ref = a.double() @ bt.double().t()
    scale = a.abs().double() @ bt.abs().double().t()
    out = eng.gemm(a, bt).cpu().double()
    assert float(((out - ref).abs() / scale).max()) < 5e-7
    y = O.gelu_new(a @ bt.t() + bias) + resid
    out = eng.gemm(a, bt, bias=bias, resid=resid, act=3).cpu()
    np.testing.assert_allclose(out.numpy(), y.numpy(), atol=2e-5, rtol=1e-5)
    eng.close()


def test_f16x2_split_edge_values():
    """the two-plane fp16 split at its edges: values below fp16's normal range (the high plane is dropped, the scaled
    low plane carries them: absolute error <= 2^-26 per element), around the 2^-14 switch, powers of two, and
    large-but-finite magnitudes (relative error <= 2^-23); magnitudes above 65504 saturate (documented limit)"""
    from capdec_amd.engine import Engine
    e = Engine(0)
    e.set_gemm_mode("f16x2")
    K = 64
    col = torch.tensor([2.0 ** -30, 2.0 ** -24, 2.0 ** -14, 2.0 ** -13, 2.0 ** -14 * 0.999, 1e-5, 3e-5, 6.1e-5, 1.0,
                        1.0 + 2.0 ** -11, 1.0 + 2.0 ** -12, 1.0 + 2.0 ** -23, 0.1, 1000.0, 60000.0, 65504.0])
    a = torch.zeros(16, K)
    a[torch.arange(16), torch.arange(16)] = col          # one value per row: the product isolates its split
    a[:, 32] = -col
    g = torch.Generator().manual_seed(2)
    bt = torch.randn(8, K, generator=g)
    ref = a.double() @ bt.double().t()
    out = e.gemm(a, bt).cpu().double()
    scale = a.abs().double() @ bt.abs().double().t()
    tiny = (a != 0).double() @ bt.abs().double().t() * 2.0 ** -25     # 2 elements per row, <= 2^-26 each
    assert bool(((out - ref).abs() <= 3e-7 * scale + tiny).all())
    big = torch.full((1, K), 0.0)
    big[0, 0] = 1e6                                        # above fp16's range: clamped to 65504
    out = e.gemm(big, torch.ones(1, K)).cpu()
    assert abs(float(out[0, 0]) - 65504.0) < 1.0
    e.close()


# ----------------------------------------------------------------------------------- bf16 GEMM-operand mode (configs[1])
def test_bf16_mode_gemm_is_bf16_operands_fp32_accumulate():
    """CAPDEC_GEMM_BF16: operands rounded to bf16 (RNE), fp32 accumulate -- equal, to fp32 round-off, to an fp64
    product of the bf16-rounded operands, and measurably NOT the fp32 product"""
    from capdec_amd.engine import Engine
    from oracle import capdec_oracle as O
    e = Engine(0)
    e.set_gemm_mode("bf16")
    assert e.gemm_mode() == "bf16"
    g = torch.Generator().manual_seed(11)
    for (M, N, K) in [(333, 1024, 768), (129, 1001, 3072), (64, 64, 64), (1000, 768, 128), (2, 130, 192)]:
        a, bt = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.2
        ar, br = a.bfloat16().double(), bt.bfloat16().double()
        ref, scale = ar @ br.t(), ar.abs() @ br.abs().t()
        out = e.gemm(a, bt).cpu().double()
        assert float(((out - ref).abs() / scale).max()) < 5e-7, (M, N, K)
        assert float(((out - a.double() @ bt.double().t()).abs() / scale).max()) > 1e-5      # really bf16 operands
    M, N, K = 193, 512, 256
    a, bt = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.2
    bias, resid = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    y = O.gelu_new(a.bfloat16().float() @ bt.bfloat16().float().t() + bias) + resid
    np.testing.assert_allclose(e.gemm(a, bt, bias=bias, resid=resid, act=3).cpu().numpy(), y.numpy(), atol=3e-5, rtol=1e-5)
    e.close()


@pytest.mark.parametrize("dims", [synth.GPT2_TINY, synth.GPT2_SMALL], ids=["tiny", "small"])
def test_bf16_mode_logits_and_decode_vs_bf16_oracle(dims):
    """bf16 mode end to end against the oracle run with bf16-rounded GEMM operands (oracle.bf16_gemm_operands).
    Bit-level agreement is impossible by construction: an fp32-round-off difference (1e-7) upstream flips a few bf16
    roundings, which decorrelates the roundings of every later layer (measured on the oracle itself: 1e-7 relative
    noise on the activations moves the logits by 0.03).  The exact statement about the arithmetic is the GEMM test
    above; here the mode must sit as close to the bf16 oracle as bf16 sits to fp32, and pick the same tokens wherever
    the margin is clear."""
    from capdec_amd.engine import Engine
    from oracle import capdec_oracle as O
    sd = synth.hot_gpt2_state_dict(42, dims)
    e = Engine(0)
    e.set_gemm_mode("bf16")
    e.load_gpt2(sd)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 23, dims.n_embd, generator=g) * 0.3
    got = e.gpt2_logits(x, all_positions=False).cpu()
    with O.bf16_gemm_operands():
        want = O.gpt2_logits(x, sd, dims.n_head)[:, -1]
    f32 = O.gpt2_logits(x, sd, dims.n_head)[:, -1]
    rms = lambda t: float(t.double().pow(2).mean().sqrt())
    gap = rms(want - f32)                                  # what bf16 operands cost against fp32
    assert gap > 3e-3                                      # the rounding is really there ...
    assert rms(got - want) < gap                           # ... and we are nearer to the bf16 oracle than fp32 is
    assert rms(got - f32) < 1.5 * gap                      # no extra error beyond the bf16 class
    assert rms(got - f32) > 0.3 * gap                      # and not silently running the fp32-accurate path
    top2 = want.topk(2, -1).values
    safe = (top2[:, 0] - top2[:, 1]) > 0.5
    assert bool((got.argmax(-1)[safe] == want.argmax(-1)[safe]).all())
    # decode under TEACHER FORCING: both pipelines are fed the same tokens (the fp32 oracle's greedy ids), so the
    # per-step logits stay comparable (free-running bf16 sequences diverge by construction).  Tolerance = 4 x the noise
    # the bf16 ORACLE ITSELF shows when its input moves by 1e-7 relative (the rounding chaos of the mode); wherever the
    # oracle's top-1 / top-2 margin clears that noise the arg-max must agree.  Covers the bf16 KV cache: K / V are
    # rounded when written (oracle: at production) and every later step reads the rounded values.
    n, Tn = 6, 12
    pe = torch.randn(n, 10, dims.n_embd, generator=g) * 0.3
    forced, _ = O.greedy_cached(sd, pe, dims.vocab + 5, Tn, alt_stop_id=-1, n_head=dims.n_head)       # fp32 ids
    got_ids, got_st = e.decode_greedy_forced(pe, forced)
    got_ids, got_st = got_ids.cpu(), got_st.cpu()
    with O.bf16_gemm_operands():
        want_ids, want_st = O.greedy_forced(sd, pe, forced, n_head=dims.n_head)
        noise = max(float((O.greedy_forced(sd, pe * (1 + eps), forced, n_head=dims.n_head)[1] - want_st).abs().max())
                    for eps in (1e-7, -3e-7, 1e-6))
    _, f32_st = O.greedy_forced(sd, pe, forced, n_head=dims.n_head)
    cls_gap = float((f32_st - want_st).abs().max())           # what the bf16 mode costs against fp32
    tol = max(4 * noise, 0.5 * cls_gap)
    assert cls_gap > 1e-3 and float((got_st - want_st).abs().max()) <= tol, (noise, cls_gap, float((got_st - want_st).abs().max()))
    assert float((got_st - f32_st).abs().max()) > 0.1 * cls_gap                  # really the bf16 path
    clear = (want_st[:, :, 0] - want_st[:, :, 1]) > 2 * tol
    assert int(clear.sum()) >= n * Tn // 4                     # the check is not vacuous
    assert bool((got_ids[clear] == want_ids[clear]).all())
    # free-running beam in bf16 mode: finite, full length, best score in the oracle's neighbourhood
    bi, bl, bs, _ = e.decode_beam(pe, dims.vocab + 5, 5, 12)
    with O.bf16_gemm_operands():
        ot, osl, osc = O.beam_cached(sd, pe, 5, dims.vocab + 5, 12, n_head=dims.n_head)
    order = O.beam_output_order(osc)
    best_sc = torch.stack([osc[r, order[r, 0]] for r in range(6)])
    np.testing.assert_allclose(bs[:, 0].cpu().numpy(), best_sc.numpy(), atol=0.05)    # best mean log-prob per caption
    assert bool((bl.cpu() == 12).all()) and bool(torch.isfinite(bs).all())
    e.close()


def test_bf16_mode_at_the_size_of_baseline_config_1():
    """BASELINE configs[1] at its own launch size: 5000 greedy rows through GPT-2 small in bf16 mode (the one-plane GEMM
    kernels' mid-size planner -- ping-pong tiles, split-K -- and the bf16 KV cache at 5000 rows, which the 6-caption test
    above never reaches).  32 seeded captions scattered through the batch are compared, TEACHER-FORCED on the fp32 oracle's
    greedy ids, with the oracle run on bf16-rounded GEMM operands: per-step (top-1, top-2, logsumexp) within the
    noise-derived tolerance of the small test (4 x what the bf16 oracle itself moves under a 1e-7 input perturbation, at
    least half the bf16-vs-fp32 class gap), arg-max equal wherever the oracle's margin clears it.  The filler rows carry
    random prefixes and random forced tokens."""
    from capdec_amd.engine import Engine
    from oracle import capdec_oracle as O
    dims = synth.GPT2_SMALL
    sd = synth.hot_gpt2_state_dict(42, dims)
    n, ncheck, Tn = 5000, 32, 10
    g = torch.Generator().manual_seed(19)
    pe = torch.randn(n, 10, dims.n_embd, generator=g) * 0.3
    forced = torch.randint(0, dims.vocab, (n, Tn), generator=g).to(torch.int32)
    rows = torch.arange(ncheck) * 157 + 3
    pe_c = pe[rows].clone()
    f_c, _ = O.greedy_cached(sd, pe_c, dims.vocab + 5, Tn, alt_stop_id=-1, n_head=dims.n_head)           # fp32 greedy ids
    forced[rows] = f_c.to(torch.int32)
    e = Engine(0)
    e.set_gemm_mode("bf16")
    e.load_gpt2(sd)
    got_ids, got_st = e.decode_greedy_forced(pe, forced)
    got_ids, got_st = got_ids.cpu()[rows], got_st.cpu()[rows]
    e.close()
    with O.bf16_gemm_operands():
        want_ids, want_st = O.greedy_forced(sd, pe_c, f_c, n_head=dims.n_head)
        noise = max(float((O.greedy_forced(sd, pe_c * (1 + eps), f_c, n_head=dims.n_head)[1] - want_st).abs().max())
                    for eps in (1e-7, -3e-7))
    _, f32_st = O.greedy_forced(sd, pe_c, f_c, n_head=dims.n_head)
    cls_gap = float((f32_st - want_st).abs().max())
    tol = max(4 * noise, 0.5 * cls_gap)
    err = float((got_st - want_st).abs().max())
    _report(f"[bf16 at 5000 rows] max |stat - bf16 oracle| {err:.4f}, tolerance {tol:.4f} (oracle noise {noise:.4f}, bf16-vs-fp32 gap {cls_gap:.4f})")
    assert cls_gap > 1e-3 and err <= tol, (noise, cls_gap, err)
    assert float((got_st - f32_st).abs().max()) > 0.1 * cls_gap                  # really the bf16 path
    clear = (want_st[:, :, 0] - want_st[:, :, 1]) > 2 * tol
    assert int(clear.sum()) >= ncheck * Tn // 4
    assert bool((got_ids[clear] == want_ids[clear]).all())


def test_bf16_kv_through_the_qkv_epilogue_matches_the_attention_append(monkeypatch):
    """bf16 mode, launches large enough for the unsplit qkv GEMM (round 5): K / V of the decoded token written by the
    one-plane GEMM's epilogue into the bf16 cache (CAPDEC_KV_DIRECT=1, default) against the attention kernel appending
    them itself (=0).  Both store the same bf16-rounded values; only the summation order of the own-token term differs --
    an fp32 round-off that the mode's rounding chaos turns into logit noise of a few hundredths (see the bf16 tests above).
    Greedy rows TEACHER-FORCED (2000 rows: per-step top-1 / top-2 / logsumexp within 0.15, mean deviation below 0.005),
    beam 5 free-running (700 captions: the best beam's mean log-prob within 0.05 for >= 95 % of them).  A wrong cache slot,
    head, position or beam row in the scatter moves these numbers by whole units."""
    from capdec_amd.engine import Engine
    dims = synth.GPT2_TINY
    sd = synth.hot_gpt2_state_dict(21, dims)
    g = torch.Generator().manual_seed(5)
    pe = torch.randn(2000, 10, dims.n_embd, generator=g) * 0.3
    forced = torch.randint(0, dims.vocab, (2000, 8), generator=g).to(torch.int32)
    outs = {}
    for kvd in ("1", "0"):
        monkeypatch.setenv("CAPDEC_GEMM_MODE", "bf16")
        monkeypatch.setenv("CAPDEC_KV_DIRECT", kvd)
        e = Engine(0)
        e.load_gpt2(sd)
        ids, st = e.decode_greedy_forced(pe, forced)
        _, _, bs, _ = e.decode_beam(pe[:700], dims.vocab + 5, 5, 9)
        outs[kvd] = (ids.cpu(), st.cpu(), bs.cpu())
        e.close()
    dst = (outs["1"][1] - outs["0"][1]).abs()
    agree = float((outs["1"][0] == outs["0"][0]).float().mean())
    dbs = (outs["1"][2][:, 0] - outs["0"][2][:, 0]).abs()
    _report(f"[bf16 K/V through the qkv epilogue vs attention append] teacher-forced stats: max {float(dst.max()):.4f} mean {float(dst.mean()):.5f}, "
            f"arg-max agreement {agree:.4f}; best-beam score |diff| < 0.05 for {float((dbs < 0.05).float().mean()):.4f} of 700")
    assert float(dst.max()) < 0.15 and float(dst.mean()) < 0.005 and agree > 0.99      # (observed: 0.039, 0.0003, 0.9998)
    assert float((dbs < 0.05).float().mean()) >= 0.95 and bool(torch.isfinite(outs["1"][2]).all())


def test_teacher_forced_decode_fp32_modes():
    """the teacher-forcing hook in the fp32-accurate default mode: arg-max ids and (top-1, top-2, logsumexp) of every step
    equal the fp32 oracle's (1e-4), with forced tokens that are NOT the arg-max (the hook really feeds them)"""
    from capdec_amd.engine import Engine
    from oracle import capdec_oracle as O
    dims = synth.GPT2_TINY
    sd = synth.hot_gpt2_state_dict(42, dims)
    e = Engine(0)
    e.load_gpt2(sd)
    g = torch.Generator().manual_seed(8)
    pe = torch.randn(5, 10, dims.n_embd, generator=g) * 0.3
    forced = torch.randint(0, dims.vocab, (5, 9), generator=g).to(torch.int32)
    ids, st = e.decode_greedy_forced(pe, forced)
    want_ids, want_st = O.greedy_forced(sd, pe, forced, n_head=dims.n_head)
    np.testing.assert_array_equal(ids.cpu().numpy(), want_ids.numpy())
    np.testing.assert_allclose(st.cpu().numpy(), want_st.numpy(), atol=1e-4)
    e.close()


# ----------------------------------------------------------------------------------- decode vs oracle, bigger batches
def test_batched_decode_vs_oracle_and_chunking():
    from capdec_amd import gpt2_prefix_eval as E
    from oracle import capdec_oracle as O
    dims = synth.GPT2_TINY
    model, sd = _model(dims, "mlp", 512, seed=7)
    x = synth.synthetic_clip_embeddings(37, 512, seed=11)          # ragged vs the 128-row GEMM tile
    pe = model.clip_project(x).reshape(37, 10, -1).cpu()
    ids_o, lens_o = O.greedy_cached(sd, pe, stop_id=443, entry_length=20)
    ids, lens = E.decode_greedy_ids(model, pe, 443, 20)
    np.testing.assert_array_equal(ids.cpu().numpy(), ids_o.numpy())
    np.testing.assert_array_equal(lens.cpu().numpy(), lens_o.numpy())
    mg = []
    tok_o, seq_o, sc_o = O.beam_cached(sd, pe, 5, 614, 20, margins=mg)
    order_o = O.beam_output_order(sc_o)
    # a caption whose selected / rejected candidate keys come within fp32 round-off of each other at some step is a
    # numerical tie (this 2-layer model has two at 4e-6): which beam survives then depends on the summation order
    clear = (mg[0] > 1e-4).numpy()
    assert clear.sum() >= 30
    def run():
        i, l, s, o = E.decode_beam_ids(model, pe, 614, 5, 20)
        return i.cpu().numpy(), l.cpu().numpy(), s.cpu().numpy(), o.cpu().numpy()
    i1, l1, s1, o1 = run()
    for r in range(37):
        if clear[r]:
            np.testing.assert_array_equal(o1[r], order_o[r].numpy())
            np.testing.assert_array_equal(i1[r], tok_o[r][order_o[r]].numpy())
            np.testing.assert_array_equal(l1[r], seq_o[r][order_o[r]].numpy())
            np.testing.assert_allclose(s1[r], sc_o[r][order_o[r]].numpy(), atol=1e-4)
        else:
            assert np.isfinite(s1[r]).all() and (np.diff(s1[r]) <= 0).all()      # a tie: any surviving beam set is valid
    # tiny KV budget -> many chunks; results must not change
    from capdec_amd import _capi
    _capi.check(model.engine.lib.capdec_set_kv_budget(model.engine._h, 3 * 5 * 29 * 768 * 2 * 4 * 2), "budget")
    i2, l2, s2, o2 = run()
    np.testing.assert_array_equal(i1, i2)
    np.testing.assert_array_equal(l1, l2)
    np.testing.assert_array_equal(s1, s2)
    # other beam widths
    for bw in (1, 3, 8):
        tok_o, seq_o, sc_o = O.beam_cached(sd, pe[:6], bw, 614, 9)
        od = O.beam_output_order(sc_o)
        i, l, s, o = E.decode_beam_ids(model, pe[:6], 614, bw, 9)
        for r in range(6):
            np.testing.assert_array_equal(i.cpu().numpy()[r], tok_o[r][od[r]].numpy())


def _report(line):
    """tie / match counts of the batched-vs-oracle tests: printed (visible with -s) and appended to
    gpurun_out/parity_counts.txt so a GPU run leaves them behind (profiles/r4_parity_counts.txt is a copy)"""
    print(line)
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "parity_counts.txt"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def _beam_rows_vs_oracle(got, sd, pe, rows, stop, T, n_head, what=""):
    """captions `rows` of a HIP beam-5 result (ids, lens, scores, order arrays) against O.beam_cached run on those
    captions alone (captions are independent).  EVERY caption is compared; a mismatch is tolerated only for a
    numerical tie -- the oracle's last selected and first rejected candidate keys within 1e-4 of each other at some
    step (with 66 steps x 5 beams about half of the captions have such a step, and nearly all of them still come out
    identical).  Returns (identical, tied_and_different); a clear caption that differs fails."""
    from oracle import capdec_oracle as O
    i1, l1, s1, o1 = got
    mg = []
    tok_o, seq_o, sc_o = O.beam_cached(sd, pe[rows], 5, stop, T, n_head=n_head, margins=mg)
    order_o = O.beam_output_order(sc_o)
    clear = (mg[0] > 1e-4).numpy()
    same = skipped = 0
    for j, r in enumerate(rows):
        eq = (np.array_equal(o1[r], order_o[j].numpy()) and np.array_equal(i1[r], tok_o[j][order_o[j]].numpy())
              and np.array_equal(l1[r], seq_o[j][order_o[j]].numpy())
              and np.allclose(s1[r], sc_o[j][order_o[j]].numpy(), atol=1e-4, rtol=0))
        if eq:
            same += 1
            continue
        if not clear[j]:
            assert np.isfinite(s1[r]).all() and (np.diff(s1[r]) <= 0).all()      # a tie: any surviving beam set is valid
            skipped += 1
            continue
        np.testing.assert_array_equal(o1[r], order_o[j].numpy())
        np.testing.assert_array_equal(i1[r], tok_o[j][order_o[j]].numpy())
        np.testing.assert_array_equal(l1[r], seq_o[j][order_o[j]].numpy())
        np.testing.assert_allclose(s1[r], sc_o[j][order_o[j]].numpy(), atol=1e-4)
    _report(f"[vs oracle] {what or 'beam'}: {len(rows)} captions compared, {same} identical "
            f"({int((~clear).sum())} had a step with a key gap < 1e-4), {skipped} differ on such a tie")
    return same, skipped


def _greedy_rows_vs_oracle(ids, lens, sd, pe, rows, stop, T, n_head, what=""):
    """captions `rows` of a HIP greedy result against O.greedy_cached: every caption is compared; a mismatch is tolerated
    only where the arg-max margin (top-1 minus top-2 logit of the oracle, teacher-forced on its own ids) drops below
    1e-4 at some step (a numerical tie).  Returns (identical, tied_and_different)."""
    from oracle import capdec_oracle as O
    gi, gl = O.greedy_cached(sd, pe[rows], stop_id=stop, entry_length=T, n_head=n_head)      # alt stop id 764: reference :187
    _, st = O.greedy_forced(sd, pe[rows], gi, n_head=n_head)
    live = torch.arange(T)[None, :] < gl[:, None]
    gap = torch.where(live, st[:, :, 0] - st[:, :, 1], torch.full((1, 1), 1e9))
    clear = (gap.min(dim=1).values > 1e-4).numpy()
    same = skipped = 0
    for j, r in enumerate(rows):
        if np.array_equal(ids[r], gi[j].numpy()) and int(lens[r]) == int(gl[j]):
            same += 1
        elif not clear[j]:
            skipped += 1
        else:
            np.testing.assert_array_equal(ids[r], gi[j].numpy())
            assert int(lens[r]) == int(gl[j])
    _report(f"[vs oracle] {what or 'greedy'}: {len(rows)} captions compared, {same} identical "
            f"({int((~clear).sum())} had a step with a top-2 gap < 1e-4), {skipped} differ on such a tie")
    return same, skipped


def test_midsize_batches_vs_oracle():
    """the regime one GPU of an 8-GPU run sits in (625 captions x beam 5 = 3125 rows): from 513 rows up the N = 768 /
    2304 projections take the mid-size split-K path (tiles <= 256, S from the tile count) and from 1024 rows the split-K
    reduce is fused with the LayerNorm that follows.  330 captions x beam 5 = 1650 rows and 1200 greedy rows, every
    caption against the KV-cached oracle (ties excluded by the margin mechanism)"""
    from capdec_amd import gpt2_prefix_eval as E
    from oracle import capdec_oracle as O
    dims = synth.GPT2_TINY
    model, sd = _model(dims, "mlp", 512, seed=7)
    n, T_ = 330, 16
    x = synth.synthetic_clip_embeddings(n, 512, seed=21)
    pe = O.clip_project(x, sd, "mlp", 10).reshape(n, 10, -1)
    assert 1024 <= n * 5 and (n * 5 + 127) // 128 * 6 <= 256            # mid-size split-K + fused reduce-LN
    i, l, s, o = E.decode_beam_ids(model, pe, 614, 5, T_)
    got = (i.cpu().numpy(), l.cpu().numpy(), s.cpu().numpy(), o.cpu().numpy())
    ok, ties = _beam_rows_vs_oracle(got, sd, pe, list(range(n)), 614, T_, dims.n_head, "mid-size: 330 captions x beam 5")
    assert ok >= 327 and ok + ties == n, (ok, ties)          # observed: 330 of 330 identical (11 with a near-tie step)
    n = 1200
    x = synth.synthetic_clip_embeddings(n, 512, seed=22)
    pe = O.clip_project(x, sd, "mlp", 10).reshape(n, 10, -1)
    ids, lens = E.decode_greedy_ids(model, pe, 443, T_)
    ok, ties = _greedy_rows_vs_oracle(ids.cpu().numpy(), lens.cpu().numpy(), sd, pe, list(range(n)), 443, T_, dims.n_head, "mid-size: 1200 greedy rows")
    assert ok >= 1188 and ok + ties == n, (ok, ties)        # observed: 1200 of 1200 identical


def test_large_launch_subset_vs_oracle():
    """the regime the 5000-caption bench runs in: 3400 captions x beam 5 = 17 000 rows in ONE launch (unsplit GEMM grids
    of several rounds of persistent blocks, the 4-rows-per-wavefront LayerNorm from 16 384 rows, the HBM-bound decode
    attention variant from 16 384 (caption, head) wavefronts); a random subset of 32 captions is compared with the
    oracle, and so are 32 of 17 000 greedy rows"""
    from capdec_amd import gpt2_prefix_eval as E
    from oracle import capdec_oracle as O
    dims = synth.GPT2_TINY
    model, sd = _model(dims, "mlp", 512, seed=7)
    n, T_ = 3400, 12
    assert n * 5 >= 16384 and n * dims.n_head > 16384
    x = synth.synthetic_clip_embeddings(n, 512, seed=31)
    pe = O.clip_project(x, sd, "mlp", 10).reshape(n, 10, -1)
    i, l, s, o = E.decode_beam_ids(model, pe, 614, 5, T_)
    got = (i.cpu().numpy(), l.cpu().numpy(), s.cpu().numpy(), o.cpu().numpy())
    rows = sorted(np.random.default_rng(5).choice(n, 32, replace=False).tolist() + [0, n - 1])
    ok, ties = _beam_rows_vs_oracle(got, sd, pe, rows, 614, T_, dims.n_head, "large launch: 34 of 3400 captions x beam 5")
    assert ok >= 33 and ok + ties == len(rows), (ok, ties)   # observed: 34 of 34 identical
    n = 17000
    x = synth.synthetic_clip_embeddings(n, 512, seed=32)
    pe = O.clip_project(x, sd, "mlp", 10).reshape(n, 10, -1)
    ids, lens = E.decode_greedy_ids(model, pe, 443, T_)
    rows = sorted(np.random.default_rng(6).choice(n, 32, replace=False).tolist() + [0, n - 1])
    ok, ties = _greedy_rows_vs_oracle(ids.cpu().numpy(), lens.cpu().numpy(), sd, pe, rows, 443, T_, dims.n_head, "large launch: 34 of 17000 greedy rows")
    assert ok >= 33 and ok + ties == len(rows), (ok, ties)   # observed: 34 of 34 identical


def test_headline_configuration_vs_oracle_at_its_own_size():
    """BASELINE metric configuration at the size bench.py times it: GPT-2 small (12 layers, V = 50 257 -> the 393-tile
    fused lm_head), 5000 x 512-d embeddings -> TransformerMapper(8) -> beam 5, P = 10, T = 67, DEFAULT mode, ONE launch of
    25 000 rows; 24 seeded captions of it against the KV-cached oracle (reference gpt2_prefix_eval.py:50-115), and 32 of
    a 25 000-row greedy batch against O.greedy_cached (reference :118-198).  The numbers of clear / tied captions are
    printed and asserted (observed: no ties on these seeds)"""
    from capdec_amd import gpt2_prefix_eval as E
    from oracle import capdec_oracle as O
    dims = synth.GPT2_SMALL
    model, sd = _model(dims, "transformer_encoder", 512, seed=42)
    n, T_, stop = 5000, 67, 13
    x = synth.synthetic_clip_embeddings(n, 512, seed=0)
    pe = model.clip_project(x).reshape(n, 10, -1)
    rows = sorted(np.random.default_rng(11).choice(n, 22, replace=False).tolist() + [0, n - 1])
    pe_rows = O.clip_project(x[rows], sd, "transformer_encoder", 10).reshape(len(rows), 10, -1)
    np.testing.assert_allclose(pe[rows].cpu().numpy(), pe_rows.numpy(), atol=2e-4, rtol=2e-4)
    i, l, s, o = E.decode_beam_ids(model, pe, stop, 5, T_)
    assert model.engine.decode_stats()["row_steps"] == n * 5 * (T_ - 1)           # one launch of 25 000 rows per step, all 67 steps
    got = (i.cpu().numpy(), l.cpu().numpy(), s.cpu().numpy(), o.cpu().numpy())
    pe_cpu = pe.cpu()
    ok, ties = _beam_rows_vs_oracle(got, sd, pe_cpu, rows, stop, T_, dims.n_head, "headline: beam 5, 5000 captions x T 67 in one launch, default mode")
    assert ok >= 23 and ok + ties == len(rows), (ok, ties)   # observed: 24 of 24 identical (12 with a near-tie step)
    del i, l, s, o
    # 25 000 greedy rows (the same 25 000-row launches, k = 1): 32 of them
    n = 25000
    x = synth.synthetic_clip_embeddings(n, 512, seed=1)
    pe = model.clip_project(x).reshape(n, 10, -1)
    ids, lens = E.decode_greedy_ids(model, pe, stop, T_)
    rows = sorted(np.random.default_rng(12).choice(n, 30, replace=False).tolist() + [0, n - 1])
    ok, ties = _greedy_rows_vs_oracle(ids.cpu().numpy(), lens.cpu().numpy(), sd, pe.cpu(), rows, stop, T_, dims.n_head,
                                      "headline: greedy, 25000 rows x T 67 in one launch, default mode")
    assert ok >= 31 and ok + ties == len(rows), (ok, ties)   # observed: 32 of 32 identical


def test_batch_invariant_mode_bit_identical_across_batch_sizes():
    """capdec_set_batch_invariant: no launch-size dependent summation order (no split-K, one GEMM geometry, pinned
    attention variant), so a caption's ids AND scores are bit-identical whether it is decoded alone, in a 330-caption
    shard (the mid-size split-K regime by default) or in a 1500-caption batch -- mapper included"""
    from capdec_amd import gpt2_prefix_eval as E
    dims = synth.GPT2_TINY
    model, sd = _model(dims, "transformer_encoder", 512, seed=7, num_layers=2)
    eng = model.engine
    n, T_ = 1500, 12
    assert n * 5 > 42 * 128 and n * dims.n_head > 16384
    x = synth.synthetic_clip_embeddings(n, 512, seed=41)

    def beams(xs):
        pe = model.clip_project(xs).reshape(xs.shape[0], 10, -1)
        i, l, s, _ = E.decode_beam_ids(model, pe, dims.vocab + 5, 5, T_)
        g, gl = E.decode_greedy_ids(model, pe, dims.vocab + 5, T_, alt_stop_id=-1)
        return i, l, s, g, gl
    default_big = beams(x)
    eng.set_batch_invariant(True)
    try:
        big, small, mid = beams(x), beams(x[:16]), beams(x[100:430])
    finally:
        eng.set_batch_invariant(False)
    # (the default mode may pick other kernel variants: same captions up to fp32 round-off -- near-ties aside)
    assert float((big[0] == default_big[0]).flatten(1).all(1).float().mean()) > 0.99
    np.testing.assert_allclose(big[2].cpu().numpy(), default_big[2].cpu().numpy(), atol=2e-5)
    for a, b in zip(big, small):
        assert torch.equal(a[:16], b)
    for a, b in zip(big, mid):
        assert torch.equal(a[100:430], b)


def test_operand_range_counter_and_nan_propagation():
    """GEMM operands beyond fp16's range are clamped AND counted (capdec_decode_counters resets the count); NaN is not
    clamped: it propagates to its output row like in an fp32 GEMM (round-2 review: a corrupt weight must not yield a
    plausible-looking caption)"""
    from capdec_amd.engine import Engine
    e = Engine(0)
    e.decode_counters()
    K = 64
    a = torch.ones(4, K)
    bt = torch.ones(8, K)
    e.gemm(a, bt)
    assert e.decode_counters()["saturated_quads"] == 0
    a[1, 3] = 1e6
    a[2, 5] = float("inf")
    a[3, 7] = float("nan")
    out = e.gemm(a, bt).cpu()
    c = e.decode_counters()
    assert c["saturated_quads"] >= 2, c
    assert e.decode_counters()["saturated_quads"] == 0                          # reset by the read
    assert torch.isfinite(out[:3]).all() and torch.isnan(out[3]).all()
    assert abs(float(out[0, 0]) - K) < 1e-3 and abs(float(out[1, 0]) - (65504.0 + K - 1)) < 1.0
    e.close()


def test_activation_range_probe_reports_saturation():
    """a checkpoint whose activations leave the fp16-plane range of the default GEMM mode must be REPORTED, not silently
    saturated: the hot-init weights stay far inside the range (counter 0 over a whole decode); the same model with
    mlp.c_fc blown up by 3e4 drives the GELU output past 65504 and the counter says so; bf16x3 mode (no such limit)
    counts nothing on the blown-up model"""
    from capdec_amd.engine import Engine
    dims = synth.GPT2_TINY
    sd = synth.hot_gpt2_state_dict(42, dims)
    g = torch.Generator().manual_seed(8)
    pe = torch.randn(3, 10, dims.n_embd, generator=g) * 0.3
    e = Engine(0)
    e.load_gpt2(sd)
    e.decode_counters()
    e.decode_greedy(pe, dims.vocab + 5, 6)
    assert e.decode_counters()["saturated_quads"] == 0
    big = {k: (v * 3e4 if k.endswith("mlp.c_fc.weight") else v) for k, v in sd.items()}
    e.load_gpt2(big)
    e.decode_greedy(pe, dims.vocab + 5, 6)
    assert e.decode_counters()["saturated_quads"] > 0
    e.set_gemm_mode("bf16x3")
    e.load_gpt2(big)
    e.decode_greedy(pe, dims.vocab + 5, 6)
    assert e.decode_counters()["saturated_quads"] == 0
    e.close()


def test_outlier_shaped_checkpoint_decodes_like_the_oracle():
    """weights shaped like a trained GPT-2 rather than like a fresh init: a few residual-stream channels carry values in
    the hundreds (fed by large c_proj columns / biases, with tiny LayerNorm gains on those channels, as in the published
    checkpoints), some LayerNorm gains are large, and mlp.c_fc holds entries beyond 16 (so that matrix leaves the
    single-accumulator GEMM kernels: GemmEpilogue::wide_ok).  Whole greedy and beam decodes in the default f16x2 mode
    must still equal the fp32 oracle token for token -- the fp16-plane operand format sees a 10^4 dynamic range per
    row here -- and nothing may be clamped (saturated_quads == 0)"""
    from capdec_amd import gpt2_prefix_eval as E
    from oracle import capdec_oracle as O
    dims = synth.GPT2_TINY
    model, sd = _model(dims, "mlp", 512, seed=11)
    g = torch.Generator().manual_seed(3)
    hot = [7, 138, 378]
    t = "gpt.transformer."
    for i in range(dims.n_layer):
        h = f"{t}h.{i}."
        sd[h + "mlp.c_proj.weight"][:, hot] *= 40.0                   # these channels of the residual stream run into the hundreds
        sd[h + "mlp.c_proj.bias"][hot] += torch.tensor([30.0, -25.0, 40.0])
        sd[h + "attn.c_proj.weight"][:, hot] *= 10.0
        for ln in ("ln_1", "ln_2"):
            sd[h + ln + ".weight"][hot] = 0.02                           # ... and the LayerNorms that read them look away
            big = torch.randint(0, dims.n_embd, (6,), generator=g)
            sd[h + ln + ".weight"][big] *= 8.0
        w = sd[h + "mlp.c_fc.weight"]
        idx = torch.randint(0, w.numel(), (40,), generator=g)
        w.view(-1)[idx] = torch.where(torch.rand(40, generator=g) > 0.5, 21.0, -19.0)      # max |w| >= 16
    sd[t + "ln_f.weight"][hot] = 0.02
    sd[t + "wpe.weight"][:, hot] *= 30.0
    model.load_state_dict(sd)
    eng = model.engine
    n, T_ = 96, 16
    x = synth.synthetic_clip_embeddings(n, 512, seed=77)
    pe = O.clip_project(x, sd, "mlp", 10).reshape(n, 10, -1)
    seen, orig = [], O.F.layer_norm                                    # what the LayerNorms of the oracle are fed
    O.F.layer_norm = lambda x_, *a, **k: (seen.append(float(x_.abs().max())), orig(x_, *a, **k))[1]
    try:
        O.gpt2_hidden(pe[:4], sd, dims.n_head)
    finally:
        O.F.layer_norm = orig
    assert max(seen) > 100.0, seen                                     # the residual stream really carries outliers
    eng.decode_counters()
    ids, lens = E.decode_greedy_ids(model, pe, 443, T_)
    ok, ties = _greedy_rows_vs_oracle(ids.cpu().numpy(), lens.cpu().numpy(), sd, pe, list(range(n)), 443, T_, dims.n_head,
                                      "outlier-shaped checkpoint: 96 greedy captions")
    assert ok >= n - 2 and ok + ties == n, (ok, ties)
    i, l, s_, o = E.decode_beam_ids(model, pe[:48], 614, 5, T_)
    got = (i.cpu().numpy(), l.cpu().numpy(), s_.cpu().numpy(), o.cpu().numpy())
    ok, ties = _beam_rows_vs_oracle(got, sd, pe[:48], list(range(48)), 614, T_, dims.n_head, "outlier-shaped checkpoint: 48 captions x beam 5")
    assert ok >= 46 and ok + ties == 48, (ok, ties)
    assert eng.decode_counters()["saturated_quads"] == 0


def test_kv_slot_statistic_and_diverged_beams():
    """capdec_decode_counters: distinct K/V slots per (caption, position) of a beam decode -- between 1 (all beams share
    their history) and the beam width; with the debug switch of the MEASUREMENT build (the shipped library has no such
    hook) that makes every beam continue itself it is exactly (P + 5 i) / (P + i) summed over the steps"""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd._capi import CapdecError
    dims = synth.GPT2_TINY
    model, sd = _model(dims, "mlp", 512, seed=7)
    eng = model.engine
    n, P, T_ = 40, 10, 14
    x = synth.synthetic_clip_embeddings(n, 512, seed=5)
    pe = model.clip_project(x).reshape(n, P, -1)
    i0, _, s0, _ = E.decode_beam_ids(model, pe, dims.vocab + 5, 5, T_)
    kv = eng.decode_counters()["kv_slots_per_position"]
    assert 1.0 <= kv <= 5.0
    assert not hasattr(eng.lib, "capdec_set_debug_diverge")                      # product library: no debug hook
    with pytest.raises(CapdecError, match="measurement build"):
        eng.set_debug_diverge(True)
    pe_host = pe.cpu()
    model.use_measurement_build(True)                 # a context of libcapdec_hip_measure.so (-DCAPDEC_MEASURE)
    engm = model.engine
    assert engm.measure and engm is not eng
    engm.set_debug_diverge(True)
    try:
        E.decode_beam_ids(model, pe_host, dims.vocab + 5, 5, T_)
        kvd = engm.decode_counters()["kv_slots_per_position"]
    finally:
        engm.set_debug_diverge(False)
    want = sum(P + 5 * i for i in range(1, T_)) / sum(P + i for i in range(1, T_))
    assert abs(kvd - want) < 1e-6 and kvd > kv
    i1, _, s1, _ = E.decode_beam_ids(model, pe_host, dims.vocab + 5, 5, T_)      # the switch is really off again, and the
    assert torch.equal(i0.cpu(), i1.cpu()) and torch.equal(s0.cpu(), s1.cpu())   # measurement build computes the same beams
    model.use_measurement_build(False)


def test_unknown_gemm_mode_is_an_error(monkeypatch):
    from capdec_amd.engine import Engine
    from capdec_amd._capi import CapdecError
    monkeypatch.setenv("CAPDEC_GEMM_MODE", "fp16")          # a typo of "f16"
    with pytest.raises(CapdecError, match="CAPDEC_GEMM_MODE"):
        Engine(0)
    monkeypatch.setenv("CAPDEC_GEMM_MODE", "f16")
    e = Engine(0)
    assert e.gemm_mode() == "f16"
    e.close()


@pytest.mark.parametrize("geometry", ["2", "8", "10", "14", "invariant"],
                         ids=["w256x128", "w128x192", "pingpong256x128", "pingpong256x192", "batch_invariant"])
def test_wide_single_accumulator_kernels_against_goldens(geometry):
    """the round-3 GEMM geometries (gemm_h2w.hip: one accumulator set, 256x128 / 128x192 block tiles, and the fused
    lm_head on the 256-row tile) and the round-4 ping-pong kernels (gemm_pp.hip: 256x128 with two accumulator sets,
    256x192 with one, their split-K, the K / V scatter and packed-output epilogues) are chosen by planners only
    for some launch sizes, so most parity tests never reach them: re-run the GEMM-vs-fp64, reference-golden (logits, greedy
    ids, beams) and batched oracle tests in a child process with CAPDEC_H2W forcing the geometry everywhere (the default
    precision mode's parametrisations only: the forced geometry is a property of those kernels)."""
    import subprocess, sys
    # ("invariant": the same tests with CAPDEC_BATCH_INVARIANT=1 -- unsplit 128x128 GEMMs at every size, which also puts
    #  the small reference goldens on the decode path of the big batches: K / V written by the qkv GEMM's epilogue)
    env = dict(os.environ, CAPDEC_BATCH_INVARIANT="1") if geometry == "invariant" else dict(os.environ, CAPDEC_H2W=geometry)
    sel = ("(test_gemm_packed_a_path or test_gpt2_logits or test_decode_small_vs_reference_golden or "
           "test_decode_tiny or test_batched_decode_vs_oracle_and_chunking or "
           "test_mlp_mapper or test_transformer_mapper or test_finished_caption_compaction or test_prompt_and_tokens) "
           "and not bf16x3 and not f32")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel,
                        "-p", "no:cacheprovider", "--durations=8"], env=env, capture_output=True, text=True, timeout=1500)
    tail = r.stdout[-2500:]
    _report(f"[forced geometry {geometry}] " + " | ".join(l.strip() for l in tail.splitlines() if " call " in l or " passed" in l)[:1200])
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, tail


@pytest.mark.parametrize("mode", ["f16x2", "bf16"])
def test_lm_head_three_candidates_with_exact_second_pass(monkeypatch, mode):
    """From 2048 rows the fused lm_head keeps 3 candidates per 128-column vocabulary tile of a k = 5 selection and
    re-runs, with 5 per tile, exactly the rows for which that can have dropped a candidate (select.hip:
    topk_merge_k3_kernel; decode.hip: lm_head_select).  The result must be the k = 5 result bit for bit: beam ids, lengths,
    scores and order with CAPDEC_LMHEAD_K3=0 (5 per tile everywhere) and with the default are compared in full -- on a
    12-tile vocabulary, where a few percent of the rows need the second pass (observed: 939 of 41 600), and on GPT-2's 393
    tiles, where almost none does -- and a subset goes against the oracle.  Same construction around the one-plane
    kernel of the bf16 mode (on/off equality only: that mode's oracle comparison is teacher-forced, see the bf16 tests)"""
    from capdec_amd.engine import Engine
    from oracle import capdec_oracle as O
    monkeypatch.setenv("CAPDEC_GEMM_MODE", mode)
    for dims, n, T_, stop, expect_many in ((synth.GPT2_TINY, 640, 14, 614, True), (synth.GPT2_SMALL, 440, 10, 13, False)):
        sd = synth.hot_state_dict(7, "mlp", 512, 10, dims=dims)
        x = synth.synthetic_clip_embeddings(n, 512, seed=77)
        pe = O.clip_project(x, sd, "mlp", 10).reshape(n, 10, -1)
        outs, second = {}, {}
        for k3 in ("1", "0", "fallback"):
            # ("fallback": a call whose second pass takes more than CAPDEC_LMHEAD_K3_MAX per mille of the rows goes back to
            #  5 per tile at the next poll point -- forced here with a threshold of 1 per mille)
            monkeypatch.setenv("CAPDEC_LMHEAD_K3", "0" if k3 == "0" else "1")
            monkeypatch.setenv("CAPDEC_LMHEAD_K3_MAX", "1" if k3 == "fallback" else "60")
            e = Engine(0)
            e.load_gpt2(sd)
            i, l, s_, o = e.decode_beam(pe, stop, 5, T_)
            outs[k3] = tuple(t.cpu().numpy() for t in (i, l, s_, o))
            second[k3] = e.second_pass_rows()
            rs = e.decode_stats()["row_steps"]
            e.close()
        _report(f"[lm_head second pass] {mode}, V = {dims.vocab}: {second['1']} of {rs} (row, step) pairs recomputed with 5 per tile")
        assert second["0"] == 0
        assert (second["1"] >= 200) if expect_many else (second["1"] < 0.02 * rs), (second, rs)
        for a, b, c_ in zip(outs["1"], outs["0"], outs["fallback"]):
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(a, c_)
        if expect_many:
            assert 0 < second["fallback"] < second["1"], second      # the call left the 3-per-tile path at its second poll
        if mode != "f16x2":
            continue
        rows = sorted(np.random.default_rng(3).choice(n, 10, replace=False).tolist())
        ok, ties = _beam_rows_vs_oracle(outs["1"], sd, pe, rows, stop, T_, dims.n_head, f"3 per tile + second pass, V = {dims.vocab}")
        assert ok + ties == len(rows) and ok >= len(rows) - 1, (ok, ties)


def test_finished_caption_compaction(monkeypatch):
    """captions that stop early leave the batch at the poll points (activation rows are compacted, KV / beam state stay
    in place): with a stop id that fires at staggered steps the results still equal the oracle token for token, the
    decode really ran on fewer rows, and CAPDEC_COMPACT=0 gives the same answer"""
    from capdec_amd.engine import Engine
    from oracle import capdec_oracle as O
    dims, stop, T, n = synth.GPT2_TINY, 1344, 34, 48
    sd = synth.hot_state_dict(7, "mlp", 512, 10, dims=dims)
    x = synth.synthetic_clip_embeddings(n, 512, seed=21)
    pe = O.clip_project(x, sd, "mlp", 10).reshape(n, 10, -1)
    gi, gl = O.greedy_cached(sd, pe, stop_id=stop, entry_length=T, alt_stop_id=-1, n_head=dims.n_head)
    assert int((gl < T - 8).sum()) >= 20 and int((gl == T).sum()) >= 5           # staggered finishing, some never stop
    bt, bq, bs_ = O.beam_cached(sd, pe, 5, stop, T, n_head=dims.n_head)
    order = O.beam_output_order(bs_)
    outs = {}
    for compact in ("1", "0"):
        monkeypatch.setenv("CAPDEC_COMPACT", compact)
        e = Engine(0)
        e.load_gpt2(sd)
        ids, lens = e.decode_greedy(pe, stop, T, alt_stop_id=-1)
        st = e.decode_stats()
        np.testing.assert_array_equal(ids.cpu().numpy(), gi.numpy())
        np.testing.assert_array_equal(lens.cpu().numpy(), gl.numpy())
        if compact == "1":
            assert st["compactions"] >= 2 and st["row_steps"] < 0.8 * n * (st["steps"] - 1), st
        else:
            assert st["compactions"] == 0 and st["row_steps"] == n * (st["steps"] - 1), st
        i, l, s_, o = e.decode_beam(pe, stop, 5, T)
        st = e.decode_stats()
        i, l, s_, o = (t.cpu().numpy() for t in (i, l, s_, o))
        np.testing.assert_array_equal(o, order.numpy())
        for r in range(n):
            np.testing.assert_array_equal(i[r], bt[r][order[r]].numpy())
            np.testing.assert_array_equal(l[r], bq[r][order[r]].numpy())
            np.testing.assert_allclose(s_[r], bs_[r][order[r]].numpy(), atol=1e-4)
        if compact == "1":
            assert st["compactions"] >= 1 and st["row_steps"] < 5 * n * (st["steps"] - 1), st
        outs[compact] = (ids.cpu().numpy(), i, s_)
        e.close()
    np.testing.assert_array_equal(outs["1"][1], outs["0"][1])
    np.testing.assert_array_equal(outs["1"][2], outs["0"][2])          # scores bit-identical with and without compaction


def test_captions_that_stop_at_the_headline_size():
    """The headline batch (5000 captions x beam 5 = 25 000-row launches, GPT-2 small, TransformerMapper) on weights whose
    captions STOP (synth.with_stop_bias: a constant on the stop token's logit; mean best-beam length ~11 tokens, a long
    tail): finished captions leave the batch at the poll points -- every step while a step is >= 8192 rows, then every
    2 / 4 / 8 -- so the launches shrink through every GEMM / attention / lm_head variant on the way down.  24 captions
    spread over the batch against the oracle (tokens, lengths, scores; numerical ties counted), compaction on against off
    (capdec_set_compact), the per-step row counts (capdec_decode_step_rows) against what the results say was still alive."""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd.predictions_runner import prefix_from_embeddings
    dims, n, T_ = synth.GPT2_SMALL, 5000, 67
    sd = synth.with_stop_bias(synth.hot_state_dict(42, "transformer_encoder", 512, 10), 13, 33.0)
    model, _ = _model(dims, "transformer_encoder", 512, seed=42)
    model.load_state_dict(sd)
    emb = synth.synthetic_clip_embeddings(n, 512, seed=0, normalize=False)
    pe = prefix_from_embeddings(model, emb)
    eng = model.engine
    eng.set_compact(True)
    i, l, s_, o = E.decode_beam_ids(model, pe, 13, 5, T_)
    st, rows = eng.decode_stats(), eng.decode_step_rows()
    lens = l.cpu().numpy()
    assert 6.0 < float(lens[:, 0].mean()) < 20.0 and int((lens[:, 0] == T_).sum()) >= 1, float(lens[:, 0].mean())
    assert len(rows) == st["steps"] - 1 and sum(rows) == st["row_steps"] and rows[0] == n * 5
    assert all(a >= b for a, b in zip(rows, rows[1:])) and rows[-1] < n * 5 // 4 and st["compactions"] >= 6, (rows, st)
    done_at = lens.max(axis=1)                                  # the step after which every beam of a caption has stopped
    for k, r in enumerate(rows):                                # never fewer rows than captions still generating
        assert r >= int((done_at > k + 1).sum()) * 5, (k, r)
    assert st["row_steps"] < 1.35 * sum(int((done_at > k + 1).sum()) * 5 for k in range(len(rows))), st
    pick = list(range(0, n, n // 24))[:24]
    got = tuple(t.cpu().numpy() for t in (i, l, s_, o))
    ok, ties = _beam_rows_vs_oracle(got, sd, pe.cpu(), pick, 13, T_, dims.n_head, "captions that stop: 24 of 5000 x beam 5")
    assert ok >= len(pick) - ties
    # observed: 24 of 24 identical (2 with a near-tie step); as at the headline size, at most one may flip on such a tie
    assert len(pick) == 24 and ok >= 23 and ok + ties == len(pick), (ok, ties)
    eng.set_compact(False)
    i2, l2, s2, _ = E.decode_beam_ids(model, pe[:1200], 13, 5, T_)
    eng.set_compact(True)
    assert eng.decode_stats()["compactions"] == 0 and len(set(eng.decode_step_rows())) == 1
    i1, l1, s1, _ = E.decode_beam_ids(model, pe[:1200], 13, 5, T_)
    same = ((i1 == i2).flatten(1).all(1) & (l1 == l2).all(1)).float().mean()
    assert float(same) >= 0.99, float(same)          # (other launch sizes: a numerical tie may flip; everything else is identical)


def test_capi_rccl_communicator_single_rank():
    """SURVEY section 8 B': capdec_comm_unique_id / capdec_comm_init / capdec_gather_rows / capdec_gather_ids over RCCL
    itself (dlopen'ed librccl, no torch.distributed): a one-rank communicator on the one GPU of this box -- ncclAllGather
    really runs -- plus the no-communicator copy path and the shard arithmetic"""
    import ctypes as C
    from capdec_amd.engine import Engine
    from capdec_amd._capi import CapdecError
    e = Engine(0)
    ids = torch.arange(7 * 12, dtype=torch.int32).view(7, 12).cuda()
    sc = torch.arange(7, dtype=torch.float32).cuda() * -0.25
    np.testing.assert_array_equal(e.gather_rows(ids, 7).cpu().numpy(), ids.cpu().numpy())       # no communicator: copy
    with pytest.raises(CapdecError):
        e.gather_rows(ids[:3], 7)                                    # partial shard without a communicator
    e.comm_init(0, 1, e.comm_unique_id())
    np.testing.assert_array_equal(e.gather_rows(ids, 7).cpu().numpy(), ids.cpu().numpy())       # ncclAllGather, 1 rank
    np.testing.assert_array_equal(e.gather_rows(sc, 7).cpu().numpy(), sc.cpu().numpy())
    assert e.gather_rows(ids[:0], 0).shape == (0, 12)
    with pytest.raises(CapdecError):
        e.gather_rows(ids[:3], 7)                                    # not this rank's shard of 7
    with pytest.raises(CapdecError):
        e.comm_init(0, 1, e.comm_unique_id())                        # one communicator per context
    e.comm_destroy()
    lo, hi = C.c_int(), C.c_int()
    for n, w in ((5, 4), (5000, 8), (0, 2)):
        spans = []
        for r in range(w):
            assert e.lib.capdec_shard_bounds(n, r, w, C.byref(lo), C.byref(hi)) == 0
            spans.append((lo.value, hi.value))
        from capdec_amd.distributed import shard_bounds
        assert spans == [shard_bounds(n, r, w) for r in range(w)]
    e.close()


def test_c_host_without_torch(tmp_path):
    """the C ABI from a plain C program (examples/c_host_demo.c: gcc, no Python, no torch in the process): same ids as
    the Python host on the same weights"""
    import os, shutil, struct, subprocess
    from capdec_amd.engine import Engine
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc on this machine")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "c_host_demo")
    lib_dir = os.path.join(root, "capdec_amd", "lib")
    subprocess.check_call([gcc, "-O2", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "c_host_demo.c"),
                           "-L" + lib_dir, "-lcapdec_hip", "-Wl,-rpath," + lib_dir, "-o", exe])
    dims = synth.GPT2_TINY
    sd = synth.hot_gpt2_state_dict(42, dims)
    g = torch.Generator().manual_seed(5)
    n, P, T = 5, 10, 12
    pe = torch.randn(n, P, dims.n_embd, generator=g) * 0.3
    path = str(tmp_path / "model.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<6if", 0x43415044, dims.n_layer, dims.n_head, dims.n_embd, dims.vocab, dims.n_pos, dims.ln_eps))
        t = "gpt.transformer."
        names = [t + "wte.weight", t + "wpe.weight"]
        for i in range(dims.n_layer):
            b = f"{t}h.{i}."
            names += [b + k for k in ("ln_1.weight", "ln_1.bias", "attn.c_attn.weight", "attn.c_attn.bias",
                                      "attn.c_proj.weight", "attn.c_proj.bias", "ln_2.weight", "ln_2.bias",
                                      "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")]
        names += [t + "ln_f.weight", t + "ln_f.bias"]
        for k in names:
            f.write(sd[k].contiguous().numpy().astype("<f4").tobytes())
        f.write(struct.pack("<2i", n, P))
        f.write(pe.numpy().astype("<f4").tobytes())
    env = dict(os.environ)
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe, path, str(T), "5"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith(("greedy", "beam"))]
    assert len(lines) == 2 * n
    e = Engine(0)
    e.load_gpt2(sd)
    ids, lens = e.decode_greedy(pe, 13, T)
    bi, bl, bs, _ = e.decode_beam(pe, 13, 5, T)
    for r in range(n):
        head, toks = lines[2 * r].split(":")
        assert int(head.split()[1]) == int(lens[r])
        assert [int(v) for v in toks.split()] == ids[r, :int(lens[r])].tolist()
        head, toks = lines[2 * r + 1].split(":")
        assert int(head.split()[1]) == int(bl[r, 0])
        assert abs(float(head.split()[2]) - float(bs[r, 0])) < 1e-5
        assert [int(v) for v in toks.split()] == bi[r, 0, :int(bl[r, 0])].tolist()
    # the same program as rank 0 of a one-rank RCCL job (communicator id through a file, capdec_gather_ids)
    out = subprocess.run([exe, path, str(T), "5", "0", "1", str(tmp_path / "rccl.id")], capture_output=True, text=True,
                         env=env, timeout=300)
    assert out.returncode == 0, out.stderr
    gathered = [ln for ln in out.stdout.splitlines() if ln.startswith("gathered")]
    assert len(gathered) == n
    for r in range(n):
        head, toks = gathered[r].split(":")
        assert int(head.split()[1]) == int(lens[r]) and [int(v) for v in toks.split()] == ids[r, :int(lens[r])].tolist()
    e.close()


def test_decode_edge_cases():
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd._capi import CapdecError
    model, sd = _model(synth.GPT2_TINY, "mlp", 512, seed=7)
    empty = torch.zeros(0, 10, 768)
    ids, lens = E.decode_greedy_ids(model, empty, 13, 5)
    assert ids.shape == (0, 5) and lens.shape == (0,)
    pe = torch.randn(2, 1, 768, generator=torch.Generator().manual_seed(0))       # prefix_length 1
    ids, lens = E.decode_greedy_ids(model, pe, 10 ** 6, 1)                       # entry_length 1
    assert ids.shape == (2, 1) and (lens.cpu() == 1).all()
    with pytest.raises(CapdecError):                                             # beyond n_positions (128)
        E.decode_greedy_ids(model, torch.zeros(1, 100, 768), 13, 67)
    with pytest.raises(CapdecError):
        E.decode_beam_ids(model, pe, 13, 9, 5)                                   # beam > 8


def test_decode_attention_launch_variants_agree():
    """the decode attention keeps 2 positions per 16-lane group in flight for large launches (> 16384 (caption, head)
    wavefronts: HBM-bound) and 4 for small ones (latency-bound); the oracle-checked tests above all sit in the small
    regime, so decode 1500 captions in one launch (large variant) and in chunks of 250 (small variant): same beams"""
    from capdec_amd import gpt2_prefix_eval as E
    dims = synth.GPT2_TINY
    model, _ = _model(dims, "mlp", 512)
    n = 1500
    assert n * dims.n_head > 16384 and 250 * dims.n_head <= 16384
    x = synth.synthetic_clip_embeddings(n, 512, seed=21)
    pe = model.clip_project(x).reshape(n, 10, -1)
    stop = dims.vocab + 5
    ids, lens, sc, _ = E.decode_beam_ids(model, pe, stop, 5, 24)
    parts = [E.decode_beam_ids(model, pe[i:i + 250], stop, 5, 24) for i in range(0, n, 250)]
    ids_c, sc_c = torch.cat([p[0] for p in parts]), torch.cat([p[2] for p in parts])
    np.testing.assert_allclose(sc.cpu().numpy(), sc_c.cpu().numpy(), atol=2e-5)
    same = (ids == ids_c).flatten(1).all(dim=1).float().mean()
    assert float(same) > 0.995, float(same)              # (a near-tie may fall the other way: different summation order)
    g, gl = E.decode_greedy_ids(model, pe, stop, 24)
    gp = torch.cat([E.decode_greedy_ids(model, pe[i:i + 250], stop, 24)[0] for i in range(0, n, 250)])
    assert float((g == gp).all(dim=1).float().mean()) > 0.995


def test_full_size_properties():
    """BASELINE geometry (GPT-2 small, P = 10, T = 67, beam 5) where the oracle is too slow:
    size-independent properties -- determinism, batch-composition invariance, beam-1 == greedy,
    scores sorted, lengths consistent with stop ids."""
    from capdec_amd import gpt2_prefix_eval as E
    model, sd = _model(synth.GPT2_SMALL, "transformer_encoder", 512)
    x = synth.synthetic_clip_embeddings(96, 512, seed=0)
    pe = model.clip_project(x).reshape(96, 10, -1)
    ids, lens = E.decode_greedy_ids(model, pe, 13, 67)
    ids2, lens2 = E.decode_greedy_ids(model, pe, 13, 67)
    assert torch.equal(ids, ids2) and torch.equal(lens, lens2)
    sub = torch.tensor([5, 90, 17, 3])
    ids_s, lens_s = E.decode_greedy_ids(model, pe[sub.cuda()], 13, 67)
    assert torch.equal(ids_s, ids[sub.cuda()]) and torch.equal(lens_s, lens[sub.cuda()])
    b_ids, b_lens, b_sc, _ = E.decode_beam_ids(model, pe[:16], 13, 1, 67)
    # beam-1 stops only on stop_id (generate_beam has no alt id 764): compare the common prefix
    n = torch.minimum(b_lens[:, 0], lens[:16]).cpu()
    for r in range(16):
        assert torch.equal(b_ids[r, 0, :n[r]].cpu(), ids[r, :n[r]].cpu())
    i5, l5, s5, _ = E.decode_beam_ids(model, pe[:32], 13, 5, 67)
    s5 = s5.cpu()
    assert bool((s5[:, :-1] >= s5[:, 1:]).all()) and bool(torch.isfinite(s5).all())
    assert int(l5.min()) >= 1 and int(l5.max()) <= 67
    # a stop id taken from the output must cut exactly there (greedy)
    first = int(ids[0, 3])
    ids_c, lens_c = E.decode_greedy_ids(model, pe[:1], first, 67)
    k = int((ids[0] == first).nonzero()[0])
    assert int(lens_c[0]) == k + 1 and torch.equal(ids_c[0, :k + 1], ids[0, :k + 1])


def test_contexts_up_to_gpt2_n_positions_vs_oracle():
    """The reference's only context limit is GPT-2's n_positions = 1024 (gpt2_prefix_eval.py:50-51,118-129 take any prefix and
    entry_length); until round 6 this library stopped at 256 / 128.  A prefix of 600 positions (prefill: the score rows of
    eight queries need 77 KB of LDS per block) and 120 decode steps (context 719: the decode attention's slot table of beam 3
    x 719 positions x four wavefronts, the beam step's history of 3 x 120 tokens + 3 x 719 ancestor bytes), greedy and beam 3,
    against the oracle; plus capdec_gpt2_logits at 700 positions."""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    from oracle import capdec_oracle as O
    dims = synth.GPT2Dims(n_layer=2, vocab=1531, n_pos=1024)
    sd = synth.hot_state_dict(5, "mlp", 512, 10, dims=dims)
    model = ClipCaptionModel(10, prefix_dim=512, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0").eval()
    model.load_state_dict(sd)
    gen = torch.Generator().manual_seed(2)
    pe = torch.randn(2, 600, 768, generator=gen) * 0.5
    ids_o, lens_o = O.greedy_cached(sd, pe, stop_id=10 ** 6, entry_length=120, alt_stop_id=-1, n_head=dims.n_head)
    ids, lens = E.decode_greedy_ids(model, pe, 10 ** 6, 120, alt_stop_id=-1)
    np.testing.assert_array_equal(ids.cpu().numpy(), ids_o.numpy())
    tok_o, seq_o, sc_o = O.beam_cached(sd, pe, 3, 10 ** 6, 120, n_head=dims.n_head)
    od = O.beam_output_order(sc_o)
    bi, bl, bs, bo = E.decode_beam_ids(model, pe, 10 ** 6, 3, 120)
    for r in range(2):
        np.testing.assert_array_equal(bi[r].cpu().numpy(), tok_o[r][od[r]].numpy())
        np.testing.assert_allclose(bs[r].cpu().numpy(), sc_o[r][od[r]].numpy(), atol=1e-4)
    x = torch.randn(1, 700, 768, generator=gen) * 0.5
    got = model.engine.gpt2_logits(x, all_positions=True).cpu()
    np.testing.assert_allclose(got.numpy(), O.gpt2_logits(x, sd, dims.n_head).numpy(), atol=4e-4)
    with pytest.raises(Exception):
        E.decode_greedy_ids(model, pe, 10 ** 6, 500)            # 600 + 500 - 1 positions: beyond n_positions


# ----------------------------------------------------------------------------------- CLIP ViT-B/32 towers
def _check_clip(g, dims):
    from capdec_amd import clip as cclip
    from oracle import capdec_oracle as O
    sd = synth.hot_clip_state_dict(43, dims)
    assert synth.state_dict_checksum(sd) == int(g["crc"]), "RNG drift"
    model, _ = cclip.load(sd, device=0)
    toks = T(g["tokens"])
    tf = model.encode_text(toks).cpu()
    np.testing.assert_allclose(tf.numpy(), g["text_features"], atol=5e-4)          # HF stand-in fixture
    np.testing.assert_allclose(tf.numpy(), O.clip_encode_text(toks, sd).numpy(), atol=5e-4)
    imgs = synth.synthetic_images(g["image_features"].shape[0], seed=int(g["image_seed"]))
    vf = model.encode_image(imgs).cpu()
    np.testing.assert_allclose(vf.numpy(), g["image_features"], atol=5e-4)
    return model, sd


def test_clip_tiny_towers(golden):
    model, sd = _check_clip(golden("clip_tiny"), synth.CLIP_TINY)
    from oracle import capdec_oracle as O
    # ragged batch (not a multiple of anything), every row a different EOT position
    toks = synth.synthetic_clip_tokens(37, seed=9, min_len=1, max_len=75)
    np.testing.assert_allclose(model.encode_text(toks).cpu().numpy(), O.clip_encode_text(toks, sd).numpy(), atol=5e-4)
    assert model.encode_text(toks[:0]).shape == (0, 512)


def test_clip_b32_towers(golden):
    _check_clip(golden("clip_b32"), synth.CLIP_VIT_B32)


def test_clip_b32_batches_and_shards(golden):
    """configs 4 / 5 beyond fixture size: ViT-B/32 towers on a few hundred texts / a hundred images -- still ONE internal
    chunk per call (batches past a chunk: tests/test_hip_chunks.py) -- must give every row what it gets alone or in
    another batch composition (a row's result may not depend on its neighbours), and the driver's rank / world shards
    must concatenate to the full batch"""
    from capdec_amd import embeddings_generator as EG
    model, sd = _check_clip(golden("clip_b32"), synth.CLIP_VIT_B32)
    toks = synth.synthetic_clip_tokens(301, seed=31, min_len=1, max_len=75).cuda()
    full = model.encode_text(toks)
    scale = float(full.abs().max())
    pick = torch.tensor([0, 7, 150, 299, 300]).cuda()
    sub = model.encode_text(toks[pick])
    assert float((sub - full[pick]).abs().max()) < 2e-5 * scale           # batch-composition independent (fp32 round-off)
    parts = [EG.encode_captions(model, toks, r, 3, gather=False) for r in range(3)]
    assert [p.shape[0] for p in parts] == [101, 101, 99]
    assert float((torch.cat(parts) - full).abs().max()) < 2e-5 * scale
    imgs = synth.synthetic_images(97, seed=32).cuda()
    fi = model.encode_image(imgs)
    si = float(fi.abs().max())
    assert float((model.encode_image(imgs[40:43]) - fi[40:43]).abs().max()) < 2e-5 * si
    parts = [EG.encode_images(model, imgs, r, 2, gather=False) for r in range(2)]
    assert float((torch.cat(parts) - fi).abs().max()) < 2e-5 * si
    # and the rows differ from one another (no broadcasting of one row's result)
    assert float((fi[0] - fi[1]).abs().max()) > 1e-3 * si and float((full[0] - full[1]).abs().max()) > 1e-3 * scale


def test_clip_text_tower_computes_only_up_to_the_eot(golden, monkeypatch):
    """Round 6: the text tower sorts a call's captions by EOT position and computes each chunk with as many positions as its
    longest caption needs (causal tower, feature read at the EOT row) instead of the 77 the reference pads to.  Same features
    as the full-length computation (CAPDEC_CLIP_TRUNC=0, a second context) and as the oracle, on a batch with every length
    from an EOT at position 1 to one at position 76, a row without any EOT-like maximum (all zeros: position 0) included,
    in the input order; fp32-accurate and fp16 towers."""
    from capdec_amd import clip as cclip
    from oracle import capdec_oracle as O
    sd = synth.hot_clip_state_dict(43, synth.CLIP_TINY)
    toks = synth.synthetic_clip_tokens(150, seed=77, min_len=0, max_len=75)
    toks[5] = 0                                                     # argmax of an all-zero row: position 0
    toks[6, :] = torch.arange(1, 78)                                # the maximum sits at the last position
    lens = toks.argmax(dim=-1)
    assert int(lens.min()) == 0 and int(lens.max()) == 76 and len(set(lens.tolist())) > 40
    want = O.clip_encode_text(toks, sd)
    for precision in ("fp32", "fp16"):
        monkeypatch.delenv("CAPDEC_CLIP_TRUNC", raising=False)
        m_t, _ = cclip.load(sd, device=0, precision=precision)
        got = m_t.encode_text(toks).cpu()
        monkeypatch.setenv("CAPDEC_CLIP_TRUNC", "0")
        m_f, _ = cclip.load(sd, device=0, precision=precision)
        full = m_f.encode_text(toks).cpu()
        monkeypatch.delenv("CAPDEC_CLIP_TRUNC", raising=False)
        scale = float(want.abs().max())
        if precision == "fp32":
            assert float((got - full).abs().max()) < 2e-5 * scale
            np.testing.assert_allclose(got.numpy(), want.numpy(), atol=5e-4)
        else:       # fp16 towers: the same arithmetic class either way (one fp16 plane per attention operand at every length)
            with O.bf16_gemm_operands(torch.float16):
                emu = O.clip_encode_text(toks, sd)
            gap = float((emu - want).abs().max())
            assert float((got - full).abs().max()) < 0.5 * gap + 2e-4 * scale
            assert float((got - emu).abs().max()) < 0.5 * gap + 2e-4 * scale
        np.testing.assert_array_equal(m_t.encode_text(toks[7:8]).cpu().numpy().shape, (1, want.shape[1]))


def _rn_check(model, sd, imgs, atol_rel, fixture=None):
    from oracle import capdec_oracle as O
    want = O.clip_encode_image_resnet(imgs, sd) if fixture is None else T(fixture)    # fixture: the torch.nn module witness
    got = model.encode_image(imgs).cpu()
    assert got.shape == want.shape
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    assert err < atol_rel * scale, (err, scale)
    return got, want


def test_clip_resnet_tiny_tower(golden):
    """ModifiedResNet image tower (the structure of RN50x4, the reference's default backbone: predictions_runner.py:158,
    220) at a small geometry vs the oracle restatement: stem with stride-2 convolution + average pool, bottlenecks with
    anti-aliased stride and downsample branches, attention pool.  Parity vs openai/CLIP itself is UNPINNED (package
    absent from the image; the oracle's attention pool is pinned against torch's multi_head_attention_forward in
    tests/test_oracle_vs_golden.py)."""
    from capdec_amd import clip as cclip
    from capdec_amd._capi import CapdecError
    sd = synth.hot_clip_resnet_state_dict(44, synth.CLIP_RN_TINY)
    model, pre = cclip.load(sd, device=0)
    assert model.input_resolution == 64 and pre.n_px == 64 and not model.has_text
    imgs = synth.synthetic_images(5, seed=12, size=64)                   # ragged: not a multiple of anything
    got, want = _rn_check(model, sd, imgs, 2e-5)
    g = golden("clip_resnet")
    assert synth.state_dict_checksum(sd) == int(g["crc_tiny"]), "RNG drift"
    _rn_check(model, sd, imgs, 3e-5, g["features_tiny"])                  # same images (seed 12): the module witness
    # every image its own answer, order preserved, batch-size independent
    assert float((want[0] - want[1]).abs().max()) > 1e-2 * float(want.abs().max())
    one = model.encode_image(imgs[3:4]).cpu()
    assert float((one - got[3:4]).abs().max()) < 1e-5 * float(want.abs().max())
    assert model.encode_image(imgs[:0]).shape == (0, 128)
    with pytest.raises(CapdecError):
        model.encode_text(torch.zeros(1, 77, dtype=torch.int64))
    with pytest.raises(CapdecError):
        model.encode_image(torch.zeros(1, 3, 32, 32))
    # a ViT tower loaded afterwards replaces the ResNet one in the same context (and vice versa)
    eng = model._engine
    vit = synth.hot_clip_state_dict(43, synth.CLIP_TINY)
    eng.load_clip(vit, text=False, vision=True)
    from oracle import capdec_oracle as O
    im2 = synth.synthetic_images(2, seed=3)
    np.testing.assert_allclose(eng.clip_encode_image(im2).cpu().numpy(), O.clip_encode_image(im2, vit).numpy(), atol=5e-4)
    eng.load_clip(sd, text=False, vision=True)
    assert float((eng.clip_encode_image(imgs).cpu() - got).abs().max()) == 0.0
    # the bf16x3 / f32 modes keep fp32 activations between the convolutions (im2col + GEMM): same answer
    for mode in ("bf16x3", "f32"):
        eng.set_gemm_mode(mode)
        alt = eng.clip_encode_image(imgs).cpu()
        assert float((alt - want).abs().max()) < 2e-5 * float(want.abs().max()), mode
    eng.set_gemm_mode("f16x2")


def test_clip_resnet_rn50x4_tower(golden):
    """the full RN50x4 geometry (layers 4/6/10/6, width 80, 288 x 288 pixels, 2560-channel attention pool with 40 heads
    over 82 tokens, 640-d output): channel counts that need padding (40, 80, 160) included"""
    from capdec_amd import clip as cclip
    sd = synth.hot_clip_resnet_state_dict(44, synth.CLIP_RN50X4)
    model, _ = cclip.load(sd, device=0)
    assert model.input_resolution == 288
    imgs = synth.synthetic_images(2, seed=13, size=288)
    g = golden("clip_resnet")
    assert synth.state_dict_checksum(sd) == int(g["crc_rn50x4"]), "RNG drift"
    _rn_check(model, sd, imgs, 5e-5, g["features_rn50x4"])                # fixture of the torch.nn module witness


def test_make_preds_from_images_rn_backbone(tmp_path):
    """the reference's image loop (predictions_runner.py:156-161, 207-234) end to end on the device: photos ->
    preprocess (PIL-exact) -> RN-tower encode_image -> normalise -> clip_project -> beam decode -> predictions JSON,
    against the oracle run one image at a time the way the reference does; a missing file (None) is skipped and
    `is_rn` forces beam search"""
    import json
    from capdec_amd import clip as cclip, predictions_runner as PR
    from oracle import capdec_oracle as O
    dims = synth.GPT2_TINY
    clip_sd = synth.hot_clip_resnet_state_dict(44, synth.CLIP_RN_TINY)
    clip_model, preprocess = cclip.load(clip_sd, device=0)
    model, sd = _model(dims, "mlp", synth.CLIP_RN_TINY.embed_dim)
    photos = [synth.synthetic_photo(h, w, 300 + i) for i, (h, w) in enumerate([(80, 100), (64, 64), (120, 70), (90, 91), (200, 150)])]
    images = photos[:2] + [None] + photos[2:]
    data = [{"image_id": 7 + i} for i in range(len(images))]
    stop = dims.vocab + 5                               # never emitted: all 12 steps run
    out = tmp_path / "p.json"
    preds = PR.make_preds_from_images(data, images, clip_model, preprocess, model, FakeTok(stop), str(out), beam=False,
                                      is_rn=True, entry_length=12, image_batch=2)
    assert [p["image_id"] for p in preds] == [7, 8, 10, 11, 12] and json.load(open(out)) == preds
    # the features: reference order of operations, one image at a time, on the oracle
    ref = torch.cat([O.clip_encode_image_resnet(O.clip_preprocess(im, 64).unsqueeze(0), clip_sd) for im in photos])
    feats = clip_model.encode_image(preprocess.batch(photos))
    assert float((feats.cpu() - ref).abs().max()) < 5e-5 * float(ref.abs().max())
    # the captions: the embedding driver (golden-tested above) on the same features; beam forced by is_rn
    kept = [d for d, im in zip(data, images) if im is not None]
    assert PR.make_preds(kept, feats, model, FakeTok(stop), None, beam=True, entry_length=12) == preds
    assert PR.make_preds(kept, feats, model, FakeTok(stop), None, beam=False, entry_length=12) != preds
    assert PR.make_preds_from_images([], [], clip_model, preprocess, model, FakeTok(stop)) == []


def test_config4_chain_images_vit_transformer_mapper_beam(tmp_path):
    """BASELINE configs[4] as ONE chain (reference predictions_runner.py:156-161, 207-234 with the ViT-B/32 backbone and a
    TransformerMapper): synthetic photos -> preprocess -> ViT encode_image (B/32 widths, two layers per tower) ->
    normalise -> + modality offset -> TransformerMapper -> beam 5 -> predictions JSON, against the oracle run ONE IMAGE AT
    A TIME the way the reference does (its own preprocess / encode_image / mapper restatements, then the reference-shaped
    generate_beam)."""
    import json
    from capdec_amd import clip as cclip, predictions_runner as PR
    from oracle import capdec_oracle as O
    dims, cdims = synth.GPT2_TINY, synth.CLIP_TINY
    csd = synth.hot_clip_state_dict(43, cdims)
    clip_model, preprocess = cclip.load(csd, device=0)
    model, sd = _model(dims, "transformer_encoder", cdims.embed_dim, seed=9, num_layers=2)
    photos = [synth.synthetic_photo(h, w, 500 + i) for i, (h, w) in enumerate([(240, 320), (224, 224), (300, 260), (231, 400)])]
    data = [{"image_id": 40 + i} for i in range(len(photos))]
    offset = torch.randn(cdims.embed_dim, generator=torch.Generator().manual_seed(4)) * 0.05
    stop, T_ = dims.vocab + 5, 9
    out = tmp_path / "c4.json"
    preds = PR.make_preds_from_images(data, photos, clip_model, preprocess, model, FakeTok(stop), str(out), beam=True,
                                      entry_length=T_, modality_offset=offset, image_batch=3)
    assert json.load(open(out)) == preds and [p["image_id"] for p in preds] == [40, 41, 42, 43]
    ok = 0
    for i, im in enumerate(photos):
        x = O.clip_encode_image(O.clip_preprocess(im, cdims.image_size).unsqueeze(0), csd, cdims.vision_heads)
        x = O.normalize_prefix(x, offset)
        pe = O.clip_project(x, sd, "transformer_encoder", 10, 10, 2).reshape(1, 10, -1)
        tok, sl, sc, order = O.generate_beam_ref(sd, pe, 5, stop, T_, n_head=dims.n_head)
        b = int(order[0])
        want = " ".join(str(int(v)) for v in tok[b][:int(sl[b])])
        ok += preds[i]["caption"] == want
        if preds[i]["caption"] != want:      # a numerical near-tie between two beams may swap them; nothing else may differ
            margin = float(sc[order[0]] - sc[order[1]])
            assert margin < 1e-4, (i, preds[i]["caption"], want, margin)
    assert ok >= len(photos) - 1


def test_make_preds_from_captions_text_branch(tmp_path):
    """the text-input branch of the reference loop (predictions_runner.py:215-218: `clip.tokenize(d['caption'])` ->
    `encode_text` -> the common tail) as a driver: captions -> token rows -> CLIP text tower -> normalise -> MLP mapper ->
    greedy -> JSON, against the oracle one caption at a time; sharded two ways it gives the same list"""
    import json
    from capdec_amd import clip as cclip, predictions_runner as PR
    from oracle import capdec_oracle as O
    dims, cdims = synth.GPT2_TINY, synth.CLIP_TINY
    csd = synth.hot_clip_state_dict(43, cdims)
    clip_model, _ = cclip.load(csd, device=0)
    model, sd = _model(dims, "mlp", cdims.embed_dim, seed=7)
    rows = synth.synthetic_clip_tokens(7, seed=21)
    data = [{"image_id": 900 + i, "caption": f"caption number {i}"} for i in range(7)]
    table = {d["caption"]: rows[i] for i, d in enumerate(data)}
    tokenize = lambda texts: torch.stack([table[t] for t in texts])       # noqa: E731  (stands for clip.tokenize: no BPE file here)
    stop, T_ = dims.vocab + 5, 11
    out = tmp_path / "t.json"
    preds = PR.make_preds_from_captions(data, clip_model, model, FakeTok(stop), tokenize, str(out), beam=False, entry_length=T_,
                                        text_batch=3)
    assert json.load(open(out)) == preds and [p["image_id"] for p in preds] == [900 + i for i in range(7)]
    for i in range(7):
        x = O.normalize_prefix(O.clip_encode_text(rows[i:i + 1], csd, cdims.text_heads))
        pe = O.clip_project(x, sd, "mlp", 10).reshape(1, 10, -1)
        want = O.generate2_ref(sd, pe, stop, T_, n_head=dims.n_head)
        assert preds[i]["caption"] == " ".join(str(v) for v in want), i
    # beam, and the default tokenizer without a vocabulary file is a clear error
    assert PR.make_preds_from_captions(data[:3], clip_model, model, FakeTok(stop), tokenize, beam=True, entry_length=T_) != preds[:3]
    with pytest.raises(Exception, match="CAPDEC_CLIP_BPE"):
        PR.make_preds_from_captions(data[:1], clip_model, model, FakeTok(stop))


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_clip_resnet_reduced_precision(precision):
    """`clip.load(..., precision="fp16")` on the ResNet tower: convolutions with ONE 16-bit operand plane (the reference's
    GPU precision class: clip.load converts the model to fp16, predictions_runner.py:218-220).  Close to the fp32 oracle at
    the precision's level, and really reduced precision (differs from the fp32-accurate run)."""
    from capdec_amd import clip as cclip
    from oracle import capdec_oracle as O
    sd = synth.hot_clip_resnet_state_dict(44, synth.CLIP_RN_TINY)
    imgs = synth.synthetic_images(6, seed=12, size=64)
    want = O.clip_encode_image_resnet(imgs, sd)
    scale = float(want.abs().max())
    full = cclip.load(sd, device=0)[0].encode_image(imgs).cpu()
    model, _ = cclip.load(sd, device=0, precision=precision)
    got = model.encode_image(imgs).cpu()
    tol = {"fp16": 1e-2, "bf16": 6e-2}[precision]
    err = float((got - want).abs().max())
    assert err < tol * scale, (err, scale)
    assert err > 20 * float((full - want).abs().max())
    # cosine similarity with the exact features: what the downstream normalise -> mapper consumes
    cos = torch.nn.functional.cosine_similarity(got, want, dim=1)
    assert float(cos.min()) > {"fp16": 0.9999, "bf16": 0.998}[precision]


@pytest.mark.parametrize("dims,tag", [(synth.CLIP_TINY, "tiny"), (synth.CLIP_VIT_B32, "b32")], ids=["tiny", "b32"])
def test_clip_fp16_tower_mode(golden, dims, tag):
    """`clip.load(..., precision="fp16")`: block GEMMs with fp16 operands (the reference's GPU precision class,
    predictions_runner.py:218,220).  (1) equals the oracle run with fp16-rounded GEMM operands up to the rounding
    chaos of the mode; (2) sits as close to the all-fp16 HF stand-in (tests/golden: model.half()) as that stand-in
    sits to fp32 -- parity vs openai/CLIP itself stays UNPINNED (package absent); (3) is really
    reduced precision (differs from the fp32 features) yet no worse than the fp16 class."""
    from capdec_amd import clip as cclip
    from oracle import capdec_oracle as O
    g = golden(f"clip_{tag}")
    sd = synth.hot_clip_state_dict(43, dims)
    assert synth.state_dict_checksum(sd) == int(g["crc"]), "RNG drift"
    model, _ = cclip.load(sd, device=0, precision="fp16")
    assert model._engine.gemm_mode() == "f16"
    toks = T(g["tokens"])
    imgs = synth.synthetic_images(g["image_features"].shape[0], seed=int(g["image_seed"]))
    for got, f32, hf16, want in (
            (model.encode_text(toks).cpu(), T(g["text_features"]), T(g["text_features_fp16"]),
             lambda: O.clip_encode_text(toks, sd)),
            (model.encode_image(imgs).cpu(), T(g["image_features"]), T(g["image_features_fp16"]),
             lambda: O.clip_encode_image(imgs, sd))):
        with O.bf16_gemm_operands(torch.float16):
            emu = want()
        scale = float(f32.abs().max())
        cls_gap = float((hf16 - f32).abs().max())             # what all-fp16 arithmetic costs (the reference's class)
        assert float((got - emu).abs().max()) < 0.5 * cls_gap + 2e-4 * scale
        assert float((got - hf16).abs().max()) < 2.0 * cls_gap
        assert 1e-5 * scale < float((got - f32).abs().max()) < 1.5 * cls_gap


def test_image_preprocess_bit_exact(eng, golden):
    """HIP preprocess (PIL-exact bicubic Resize + CenterCrop + ToTensor + Normalize) == oracle == PIL fixture, on a
    ragged batch in ONE call, both geometries; then the façade's `preprocess` feeding encode_image"""
    from oracle import capdec_oracle as O
    g = golden("preprocess")
    imgs = [synth.synthetic_photo(h, w, 100 + i) for i, (h, w) in enumerate(synth.PREPROCESS_SIZES)]
    for stretch in (False, True):
        out = eng.preprocess_images(imgs, 224, stretch).cpu()
        assert out.shape == (len(imgs), 3, 224, 224)
        for i, im in enumerate(imgs):
            want = O.clip_preprocess(im, 224, stretch)
            assert torch.equal(out[i], want), (i, stretch, float((out[i] - want).abs().max()))
            np.testing.assert_array_equal(out[i].reshape(-1)[::29].numpy(), g[f"sub_{i}_{int(stretch)}"])
    assert eng.preprocess_images([], 224).shape == (0, 3, 224, 224)
    small = eng.preprocess_images(imgs[:3], 64).cpu()                  # another n_px
    for i in range(3):
        assert torch.equal(small[i], O.clip_preprocess(imgs[i], 64))
    with pytest.raises(Exception):
        eng.preprocess_images([np.zeros((4, 4), np.uint8)])
    # drop-in surface: clip.load -> (model, preprocess); preprocess(image) -> [3, 224, 224] on the device
    from capdec_amd import clip
    model, preprocess = clip.load(synth.hot_clip_state_dict(43, synth.CLIP_TINY), device=0)
    x = preprocess(imgs[0])
    assert x.shape == (3, model.input_resolution, model.input_resolution) and x.is_cuda
    want = O.clip_preprocess(imgs[0], model.input_resolution)
    assert torch.equal(x.cpu(), want)
    emb = model.encode_image(preprocess.batch(imgs[:4]))
    ref = O.clip_encode_image(torch.stack([O.clip_preprocess(im, model.input_resolution) for im in imgs[:4]]),
                              synth.hot_clip_state_dict(43, synth.CLIP_TINY), synth.CLIP_TINY.vision_heads)
    np.testing.assert_allclose(emb.cpu().numpy(), ref.numpy(), atol=5e-4, rtol=1e-4)
    try:
        from PIL import Image
        assert torch.equal(preprocess(Image.fromarray(imgs[1])).cpu(), O.clip_preprocess(imgs[1], model.input_resolution))
    except ImportError:
        pass


def test_text_to_prefix_pipeline():
    """config-4 chain: encode_text -> noise_injection -> clip_project, vs the oracle with the same injected noise"""
    from capdec_amd import clip as cclip, embeddings_generator as eg
    from oracle import capdec_oracle as O
    dims = synth.CLIP_TINY
    csd = synth.hot_clip_state_dict(43, dims)
    cm, _ = cclip.load(csd, device=0)
    model, sd = _model(synth.GPT2_TINY, "mlp", 512, seed=7)
    toks = synth.synthetic_clip_tokens(9, seed=5)
    emb = eg.encode_captions(cm, toks)
    assert emb.shape == (9, 512)
    noise = torch.randn(9, 512, generator=torch.Generator().manual_seed(3))
    from capdec_amd import train as ct
    x = ct.noise_injection(emb, 0.016, noise=noise)
    pe = model.clip_project(x).reshape(9, 10, -1).cpu()
    ref = O.clip_project(O.noise_injection(O.clip_encode_text(toks, csd), 0.016, noise=noise), sd, "mlp", 10)
    np.testing.assert_allclose(pe.numpy(), ref.numpy(), atol=1e-3)
    assert eg.text_to_prefix(cm, model, toks, noise_variance=0.016, seed=1).shape == (9, 10, 768)


def test_decode_p40_notebook_geometry(golden):
    """prefix_length 40 / 640-d (others/CapDec_inference.ipynb): contexts up to 106 tokens, 80-token mapper sequences"""
    from capdec_amd import gpt2_prefix_eval as E
    g = golden("decode_p40_tiny")
    dims = synth.GPT2_TINY
    for mapping in ("mlp", "transformer_encoder"):
        model, sd = _model(dims, mapping, 640, seed=11, P=40, clip_length=40, num_layers=2)
        assert synth.state_dict_checksum(sd) == int(g[f"{mapping}_crc"]), "RNG drift"
        n = g[f"{mapping}_x"].shape[0]
        pe = model.clip_project(T(g[f"{mapping}_x"])).reshape(n, 40, -1)
        np.testing.assert_allclose(pe.cpu().numpy(), g[f"{mapping}_prefix_embed"], atol=3e-4)
        pe = T(g[f"{mapping}_prefix_embed"])
        ids, lens = E.decode_greedy_ids(model, pe, dims.vocab + 5, 67)
        np.testing.assert_array_equal(ids.cpu().numpy(), g[f"{mapping}_greedy_ids"])
        np.testing.assert_array_equal(lens.cpu().numpy(), g[f"{mapping}_greedy_lens"])
        bi, bl, bs, bo = (t.cpu().numpy() for t in E.decode_beam_ids(model, pe, int(g[f"{mapping}_beam_stop_id"]), 5, 67))
        go = g[f"{mapping}_beam_order"]
        np.testing.assert_array_equal(bo, go)
        for r in range(n):
            np.testing.assert_array_equal(bi[r], g[f"{mapping}_beam_tokens"][r][go[r]])
            np.testing.assert_array_equal(bl[r], g[f"{mapping}_beam_seqlen"][r][go[r]].astype(np.int32))
            np.testing.assert_allclose(bs[r], g[f"{mapping}_beam_scores"][r][go[r]], atol=1e-4)


def test_long_context_vs_oracle():
    """near the supported maxima (context 209 of 256, entry_length 120 of 128): softmax over > 3 x 64 positions,
    beam token history / ancestor tables at full length"""
    from capdec_amd import gpt2_prefix_eval as E
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    from oracle import capdec_oracle as O
    dims = synth.GPT2Dims(n_layer=2, vocab=1531, n_pos=256)
    sd = synth.hot_state_dict(5, "mlp", 512, 10, dims=dims)
    model = ClipCaptionModel(10, prefix_dim=512, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0").eval()
    model.load_state_dict(sd)
    pe = torch.randn(3, 90, 768, generator=torch.Generator().manual_seed(1)) * 0.5      # prefix of 90 positions
    ids_o, lens_o = O.greedy_cached(sd, pe, stop_id=10 ** 6, entry_length=120, alt_stop_id=-1)
    ids, lens = E.decode_greedy_ids(model, pe, 10 ** 6, 120, alt_stop_id=-1)
    np.testing.assert_array_equal(ids.cpu().numpy(), ids_o.numpy())
    tok_o, seq_o, sc_o = O.beam_cached(sd, pe, 3, 10 ** 6, 120)
    od = O.beam_output_order(sc_o)
    bi, bl, bs, bo = E.decode_beam_ids(model, pe, 10 ** 6, 3, 120)
    for r in range(3):
        np.testing.assert_array_equal(bi[r].cpu().numpy(), tok_o[r][od[r]].numpy())
        np.testing.assert_allclose(bs[r].cpu().numpy(), sc_o[r][od[r]].numpy(), atol=1e-4)
