"""The chunk loops of the CLIP towers and of the mapper, past one chunk, and the text tower at every short length.
Needs an MI355X: ``pytest -m gpu``.

``capdec_clip_encode_text`` sorts a call's captions by EOT position, cuts the sorted list into chunks (at most
4096 * 77 token rows and at most 65 536 captions each), computes a chunk with P = its largest EOT + 1 positions and
scatters the features back through the permutation; the image towers and ``capdec_mapper_forward`` walk their batch in
fixed-size chunks.  test_hip_parity.py only ever reaches the first iteration of these loops, and almost only P = 76 / 77.
Here every loop iterates, at the sizes bench.py's ``text_embed`` workload runs them, and the text tower runs at every
P from 1 up.

The checker is always the CPU oracle, which is per-row independent: evaluated on a subset of rows it is a full-strength
reference for those rows.  Every listed row is compared, none excluded.  Tolerances are the ones test_hip_parity.py
already uses: fp32-accurate ViT / text towers 5e-4 abs against the oracle; two GPU computations of the same row
2e-5 * max|features|; fp16 towers 0.5 * gap + 2e-4 * scale against the oracle with fp16 GEMM operands and
1.5 * gap + 2e-4 * scale against the fp32 oracle (gap = the distance of those two oracles); the RN50x4 tower
5e-5 * scale (at its feature scale of ~8 that is below 5e-4); mapper outputs 2e-4; the text -> noise -> mapper chain
1e-3."""
import numpy as np
import pytest
import torch

from capdec_amd import synth
from test_hip_parity import _report          # one line per comparison: printed and kept with the parity counts

pytestmark = pytest.mark.gpu

TEXT_ROW_BUDGET = 4096 * 77          # capdec_clip_encode_text (clip.hip) restated: token rows per chunk ...
TEXT_CAPTION_CAP = 65536             # ... and captions per chunk


def _err(a, b):
    return float((a - b).abs().max())


def _text_chunks(toks):
    """The chunk rule of capdec_clip_encode_text restated: -> (order, [(first sorted index, captions, P)]).
    order = the captions stably sorted by EOT position (argmax of the row: EOT is the highest id)."""
    pos = toks.argmax(dim=-1).numpy()
    order = np.argsort(pos, kind="stable")
    ps = pos[order] + 1
    n, chunks, i0 = len(ps), [], 0
    while i0 < n:
        m = 1
        while i0 + m < n and m < TEXT_CAPTION_CAP and (m + 1) * int(ps[i0 + m]) <= TEXT_ROW_BUDGET:
            m += 1
        chunks.append((i0, m, int(ps[i0 + m - 1])))
        i0 += m
    return order, chunks


def _text_rows(order, chunks, stride, ends=8):
    """every `stride`-th caption of the sorted order and its last 8 (the tail of the last chunk), 8 captions on each side of
    every chunk edge, the first and last `ends` of the input order"""
    n = len(order)
    rows = set(order[::stride].tolist()) | set(order[-8:].tolist())
    for i0, _, _ in chunks[1:]:
        rows.update(order[max(i0 - 8, 0):i0 + 8].tolist())
    rows.update(range(ends))
    rows.update(range(n - ends, n))
    return sorted(rows)


def _layout(chunks):
    return " + ".join(f"({m}, P {p})" for _, m, p in chunks)


def _oracles(toks, sd, fp16):
    from oracle import capdec_oracle as O
    want = O.clip_encode_text(toks, sd)
    if not fp16:
        return want, None
    with O.bf16_gemm_operands(torch.float16):
        return want, O.clip_encode_text(toks, sd)


def _check_text_rows(what, got, want, emu):
    """got / want / emu: the same rows from the GPU, the fp32 oracle and (fp16 towers) the fp16-operand oracle"""
    scale = float(want.abs().max())
    if emu is None:
        _report(f"{what}: {got.shape[0]} rows vs oracle, max err {_err(got, want):.3g} (bound 5e-4), scale {scale:.3g}")
        np.testing.assert_allclose(got.numpy(), want.numpy(), atol=5e-4, rtol=0, err_msg=what)
    else:
        gap = _err(emu, want)
        e_emu, e_f32 = _err(got, emu), _err(got, want)
        _report(f"{what}: {got.shape[0]} rows, fp16 tower vs fp16-operand oracle {e_emu:.3g} (bound "
                f"{0.5 * gap + 2e-4 * scale:.3g}), vs fp32 oracle {e_f32:.3g} (bound {1.5 * gap + 2e-4 * scale:.3g}), "
                f"gap {gap:.3g}, scale {scale:.3g}")
        assert e_emu < 0.5 * gap + 2e-4 * scale, (what, e_emu, gap, scale)
        assert e_f32 < 1.5 * gap + 2e-4 * scale, (what, e_f32, gap, scale)
    return scale


def _encode_text_sliced(model, toks, step):
    return torch.cat([model.encode_text(toks[i:i + step]) for i in range(0, toks.shape[0], step)])


# ----------------------------------------------------------------------------------- 1. every short chunk length
SHORT_P = [1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 76, 77]


def _tokens_at(P):
    """67 captions that all have their EOT at position P - 1: one chunk computed with exactly P positions"""
    if P == 1:
        return torch.zeros(67, 77, dtype=torch.int64)               # argmax of an all-zero row: position 0
    return synth.synthetic_clip_tokens(67, seed=P, min_len=P - 2, max_len=P - 2)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_text_tower_at_every_short_chunk_length(precision):
    """The truncated text tower at P = 1 .. 77 positions per caption, P not a multiple of the 16 / 32-row attention tiles
    included: 67 captions with the same EOT position are one chunk of exactly that P, all 67 against the oracle.  One
    context runs the lengths in descending and then ascending order, so the workspaces a longer chunk sized (K / V
    planes, packed operands) are reused by a shorter one and the reverse."""
    from capdec_amd import clip as cclip
    sd = synth.hot_clip_state_dict(43, synth.CLIP_TINY)
    cases = {}
    for P in SHORT_P:
        toks = _tokens_at(P)
        assert toks.argmax(dim=-1).tolist() == [P - 1] * 67
        cases[P] = (toks,) + _oracles(toks, sd, precision == "fp16")
    model, _ = cclip.load(sd, device=0, precision=precision)
    try:
        for leg, seq in (("descending", SHORT_P[::-1]), ("ascending", SHORT_P)):
            for P in seq:
                toks, want, emu = cases[P]
                got = model.encode_text(toks).cpu()
                _check_text_rows(f"short chunk P {P} ({leg}, {precision})", got, want, emu)
    finally:
        model._engine.close()


# ----------------------------------------------------------------------------------- 2. text_embed at its own size
def _check_chunked_text(what, sd, toks, precision, stride, min_chunks, expect=None, slices=2500):
    """encode `toks` in one call; the selected rows against the oracle, all rows against input-order slices that are one
    chunk each.  -> (features on the host, rows, oracle features of the rows)"""
    from capdec_amd import clip as cclip
    order, chunks = _text_chunks(toks)
    _report(f"{what}: {toks.shape[0]} captions, chunks {_layout(chunks)}")
    assert len(chunks) >= min_chunks, chunks             # a one-chunk call would not test the loop
    if expect is not None:
        assert [(m, p) for _, m, p in chunks] == expect, chunks
    rows = _text_rows(order, chunks, stride)
    want, emu = _oracles(toks[rows], sd, precision == "fp16")
    model, _ = cclip.load(sd, device=0, precision=precision)
    try:
        dev = toks.cuda()
        got = model.encode_text(dev)
        if slices:
            assert all(len(_text_chunks(toks[i:i + slices])[1]) == 1 for i in range(0, toks.shape[0], slices))
            part = _encode_text_sliced(model, dev, slices)
            again = model.encode_text(dev)                # after the small calls: same workspaces, same answer
        got_c = got.cpu()
        scale = _check_text_rows(f"{what} ({precision})", got_c[rows], want, emu)
        if slices:
            e_part, e_again = _err(got, part), _err(got, again)
            bound = 2e-5 * scale          # (fp16 towers too: the same operands are rounded the same way at every P)
            _report(f"{what} ({precision}): all {toks.shape[0]} rows vs slices of {slices}: {e_part:.3g}, vs the call "
                    f"repeated: {e_again:.3g} (bound {bound:.3g})")
            assert e_part < bound and e_again < bound, (e_part, e_again, bound)
    finally:
        model._engine.close()
    return got_c, rows, want


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_text_embed_at_its_own_size(precision):
    """bench.py's text_embed input (20 000 captions, lengths 8..20) through the 2-layer text tower: two chunks,
    (15 769, P 20) and (4 231, P 22).  ~1 300 rows against the oracle -- every 16th of the sorted order, 8 on each side
    of the chunk edge, the ends of the input order -- and all 20 000 against the same captions in slices of 2 500."""
    sd = synth.hot_clip_state_dict(43, synth.CLIP_TINY)
    toks = synth.synthetic_clip_tokens(20000, seed=2)
    _check_chunked_text("text_embed, tiny tower", sd, toks, precision, 16, 2, expect=[(15769, 20), (4231, 22)])


def test_text_embed_at_its_own_size_vit_b32_fp16():
    """the configuration the captions/s line of BASELINE configs[3] is quoted on: the 12-layer ViT-B/32 text tower with
    fp16 operands on the 20 000 captions, 256 of them against the oracle.  Measured: 0.0033 from the fp16-operand oracle
    against a bound of 0.0035 (gap 0.0052, scale 4.6) -- at 12 layers the bound that the 2-layer tower meets with a third
    to spare is nearly used up -- and 0.0052 from the fp32 oracle against 0.0086."""
    sd = synth.hot_clip_state_dict(43, synth.CLIP_VIT_B32)
    toks = synth.synthetic_clip_tokens(20000, seed=2)
    order, chunks = _text_chunks(toks)
    stride = -(-20000 // (256 - 40))       # 216 strided rows + 8 at the tail + 16 at the edge + 16 at the ends = 256
    rows = _text_rows(order, chunks, stride)
    assert 240 <= len(rows) <= 256, len(rows)
    _check_chunked_text("text_embed, ViT-B/32 tower", sd, toks, "fp16", stride, 2, expect=[(15769, 20), (4231, 22)],
                        slices=0)


# ----------------------------------------------------------------------------------- 3. many lengths, many chunks
def test_text_tower_many_lengths_many_chunks(monkeypatch):
    """24 000 captions with EOT positions 1..76: four chunks, each with its own P, and with CAPDEC_CLIP_TRUNC=0 (a second
    context) six chunks of 4096 full-length captions.  Both against the oracle rows and against each other on all rows."""
    from capdec_amd import clip as cclip
    sd = synth.hot_clip_state_dict(43, synth.CLIP_TINY)
    toks = synth.synthetic_clip_tokens(24000, seed=3, min_len=0, max_len=75)
    monkeypatch.delenv("CAPDEC_CLIP_TRUNC", raising=False)
    got, rows, want = _check_chunked_text("many lengths", sd, toks, "fp32", 16, 4,
                                          expect=[(9817, 32), (6065, 52), (4707, 67), (3411, 77)])
    monkeypatch.setenv("CAPDEC_CLIP_TRUNC", "0")
    model, _ = cclip.load(sd, device=0)
    try:
        full = model.encode_text(toks).cpu()
    finally:
        model._engine.close()
        monkeypatch.delenv("CAPDEC_CLIP_TRUNC", raising=False)
    scale = _check_text_rows("many lengths, CAPDEC_CLIP_TRUNC=0 (6 chunks of <= 4096)", full[rows], want, None)
    e = _err(got, full)
    _report(f"many lengths: all 24000 rows truncated vs full length {e:.3g} (bound {2e-5 * scale:.3g})")
    assert e < 2e-5 * scale, (e, scale)


# ----------------------------------------------------------------------------------- 4. the caption cap
def test_text_tower_caption_cap():
    """70 000 captions with their EOT at positions 1..3: P <= 4, so the row budget would admit 78 848 captions and the
    65 536-caption cap is what ends the first chunk: (65 536, P 4) + (4 464, P 4)."""
    from capdec_amd import clip as cclip
    sd = synth.hot_clip_state_dict(43, synth.CLIP_TINY)
    toks = synth.synthetic_clip_tokens(70000, seed=3, min_len=0, max_len=2)
    order, chunks = _text_chunks(toks)
    _report(f"caption cap: 70000 captions, chunks {_layout(chunks)}")
    assert [(m, p) for _, m, p in chunks] == [(65536, 4), (4464, 4)], chunks
    assert (TEXT_CAPTION_CAP + 1) * 4 <= TEXT_ROW_BUDGET             # the row budget is not what binds
    rows = sorted(set(order[::64].tolist()) | set(order[65536 - 8:65536 + 8].tolist()) | set(order[-8:].tolist()))
    want, _ = _oracles(toks[rows], sd, False)
    model, _ = cclip.load(sd, device=0)
    try:
        got = model.encode_text(toks).cpu()
    finally:
        model._engine.close()
    _check_text_rows("caption cap", got[rows], want, None)


# ----------------------------------------------------------------------------------- 5. image towers past one chunk
def test_vit_image_tower_past_one_chunk():
    """2 100 images through the 2-layer ViT image tower: chunks of 2048 + 52.  Every 32nd image, the 16 around the chunk
    edge and the last 4 against the oracle; all 2 100 against the same images 700 at a time."""
    from capdec_amd import clip as cclip
    from oracle import capdec_oracle as O
    sd = synth.hot_clip_state_dict(43, synth.CLIP_TINY)
    n = 2100
    imgs = synth.synthetic_images(n, seed=51)
    rows = sorted(set(range(0, n, 32)) | set(range(2040, 2057)) | set(range(n - 4, n)))
    want = O.clip_encode_image(imgs[rows], sd)
    model, _ = cclip.load(sd, device=0)
    try:
        dev = imgs.cuda()
        got = model.encode_image(dev)
        part = torch.cat([model.encode_image(dev[i:i + 700]) for i in range(0, n, 700)])
        e_part = _err(got, part)
        got = got.cpu()
        del dev, part
    finally:
        model._engine.close()
    scale = float(want.abs().max())
    _report(f"ViT image tower: 2100 images = chunks of 2048 + 52, {len(rows)} rows vs oracle {_err(got[rows], want):.3g} "
            f"(bound 5e-4), all rows vs 700 at a time {e_part:.3g} (bound {2e-5 * scale:.3g})")
    np.testing.assert_allclose(got[rows].numpy(), want.numpy(), atol=5e-4, rtol=0)
    assert e_part < 2e-5 * scale, (e_part, scale)


def test_rn50x4_image_tower_past_one_chunk():
    """200 images at 288 x 288 through the RN50x4 tower, whose chunk follows free memory (about 170 images, fewer on a
    fuller card): the edge is not known here, so every 8th image and the last 8 against the oracle and all 200 against
    the same images 8 at a time."""
    from capdec_amd import clip as cclip
    from oracle import capdec_oracle as O
    sd = synth.hot_clip_resnet_state_dict(44, synth.CLIP_RN50X4)
    n = 200
    imgs = synth.synthetic_images(n, seed=52, size=288)
    rows = sorted(set(range(0, n, 8)) | set(range(n - 8, n)))
    want = O.clip_encode_image_resnet(imgs[rows], sd)
    model, _ = cclip.load(sd, device=0)
    try:
        dev = imgs.cuda()
        got = model.encode_image(dev)
        part = torch.cat([model.encode_image(dev[i:i + 8]) for i in range(0, n, 8)])
        e_part = _err(got, part)
        got = got.cpu()
        del dev, part
    finally:
        model._engine.close()
    scale = float(want.abs().max())
    e = _err(got[rows], want)
    _report(f"RN50x4 image tower: 200 images, {len(rows)} rows vs oracle {e:.3g} (bound {5e-5 * scale:.3g}), all rows vs "
            f"8 at a time {e_part:.3g} (bound {2e-5 * scale:.3g}), scale {scale:.3g}")
    assert e < 5e-5 * scale, (e, scale)
    assert e_part < 2e-5 * scale, (e_part, scale)


# ----------------------------------------------------------------------------------- 6. mapper past one chunk, the chain
@pytest.mark.parametrize("mapping", ["mlp", "transformer_encoder"])
def test_mapper_past_one_chunk(mapping):
    """8 237 embeddings through capdec_mapper_forward: chunks of 8192 + 45.  Every 64th row, the 16 around the chunk edge
    and the last 8 against the oracle."""
    from capdec_amd.engine import Engine
    from oracle import capdec_oracle as O
    n = 8200 + 37
    x = synth.synthetic_clip_embeddings(n, 512, seed=61)
    rows = sorted(set(range(0, n, 64)) | set(range(8184, 8201)) | set(range(n - 8, n)))
    eng = Engine(0)
    try:
        if mapping == "mlp":
            sd = synth.hot_mlp_mapper_state_dict(43, 512, 10)
            eng.load_mapper_mlp(sd)
        else:
            sd = synth.hot_transformer_mapper_state_dict(43, 512, 10, 10, 8)
            eng.load_mapper_transformer(sd)
        got = eng.mapper_forward(x).cpu()
    finally:
        eng.close()
    want = O.clip_project(x[rows], sd, mapping, 10, 10, 8)
    assert got.shape == (n, 10, 768)
    _report(f"mapper {mapping}: 8237 rows = chunks of 8192 + 45, {len(rows)} rows vs oracle {_err(got[rows], want):.3g} "
            f"(bound 2e-4)")
    np.testing.assert_allclose(got[rows].numpy(), want.numpy(), atol=2e-4, rtol=0)


def test_text_to_prefix_at_the_size_of_text_embed():
    """The configs[3] chain on the 20 000 captions of text_embed: encode_text (two chunks) -> noise_injection ->
    clip_project (three mapper chunks).  With injected noise against the oracle chain on the oracle rows of
    test_text_embed_at_its_own_size; eg.text_to_prefix itself draws its noise on the device from a seed, which no
    oracle can restate, so it is compared on all rows with the same three steps called one by one with that seed."""
    from capdec_amd import clip as cclip, embeddings_generator as eg, train as ct
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    from oracle import capdec_oracle as O
    csd = synth.hot_clip_state_dict(43, synth.CLIP_TINY)
    toks = synth.synthetic_clip_tokens(20000, seed=2)
    n = toks.shape[0]
    order, chunks = _text_chunks(toks)
    assert len(chunks) >= 2 and n > 2 * 8192, chunks
    rows = _text_rows(order, chunks, 16)
    model = ClipCaptionModel(10, prefix_dim=512, mapping_type=MappingType.MLP, gpt2_dims=synth.GPT2_TINY).to("cuda:0").eval()
    sd = synth.hot_state_dict(7, "mlp", 512, 10, dims=synth.GPT2_TINY)
    model.load_state_dict(sd)
    noise = torch.randn(n, 512, generator=torch.Generator().manual_seed(3))
    cm, _ = cclip.load(csd, device=0)
    try:
        dev = toks.cuda()
        emb = eg.encode_captions(cm, dev)
        assert emb.shape == (n, 512)
        pe = model.clip_project(ct.noise_injection(emb, 0.016, noise=noise.cuda())).reshape(n, 10, -1)
        seeded = eg.text_to_prefix(cm, model, dev, noise_variance=0.016, seed=1)
        by_hand = model.clip_project(ct.noise_injection(eg.encode_captions(cm, dev), 0.016, seed=1)).reshape(n, 10, -1)
        assert seeded.shape == (n, 10, 768)
        e_seed, s_seed = _err(seeded, by_hand), float(by_hand.abs().max())
        differs = _err(seeded, pe)
        pe = pe.cpu()
    finally:
        cm._engine.close()
    ref = O.clip_project(O.noise_injection(O.clip_encode_text(toks[rows], csd), 0.016, noise=noise[rows]), sd, "mlp", 10)
    _report(f"text_to_prefix at 20000 captions: text chunks {_layout(chunks)}, 3 mapper chunks, {len(rows)} rows vs the "
            f"oracle chain {_err(pe[rows], ref):.3g} (bound 1e-3); seeded text_to_prefix vs its steps {e_seed:.3g} "
            f"(bound {2e-5 * s_seed:.3g})")
    np.testing.assert_allclose(pe[rows].numpy(), ref.numpy(), atol=1e-3, rtol=0)
    assert e_seed < 2e-5 * s_seed, (e_seed, s_seed)
    assert differs > 1e-3 * s_seed               # (another noise draw: the seeded call is not the injected one)
