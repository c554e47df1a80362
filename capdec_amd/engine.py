"""Host-side driver of one MI355X: owns a ``capdec_ctx`` and hands device pointers of torch
CUDA(HIP) tensors to the C ABI.  torch is plumbing only (device memory, streams); all
arithmetic happens in libcapdec_hip.so."""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses
import math
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _capi
from ._capi import CapdecError, check


def _f32(t: torch.Tensor) -> np.ndarray:
    """contiguous fp32 host array view of a (CPU) tensor; fp16 pickles are upcast like the
    reference's `.float()` (train.py:70)."""
    return np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())


def _fp(a: np.ndarray):
    return a.ctypes.data_as(_capi.c_float_p)


@dataclasses.dataclass(frozen=True, eq=False)
class LogitsProcessors:
    """What steers a decode (capdec_set_logits_processors / capdec_set_logit_bias; the contract: include/capdec.h).  The
    defaults switch everything off.  ``top_k`` acts in the sampling decode only; ``logit_bias`` is a HOST vector [vocab]
    (tensor, array or list) of finite or ``-inf`` entries."""
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    min_length: int = 0
    top_k: int = 0
    logit_bias: Optional[object] = None

    def __post_init__(self):
        t = self.repetition_penalty
        if not (isinstance(t, (int, float)) and t > 0 and math.isfinite(t)):
            raise CapdecError(f"LogitsProcessors: repetition_penalty must be a finite number > 0 (1 = off), got {t!r}")
        for name in ("no_repeat_ngram_size", "min_length", "top_k"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise CapdecError(f"LogitsProcessors: {name} must be an integer >= 0 (0 = off), got {v!r}")

    @property
    def active(self) -> bool:
        return (self.repetition_penalty != 1.0 or self.no_repeat_ngram_size > 0 or self.min_length > 0 or self.top_k > 0
                or self.logit_bias is not None)

    @classmethod
    def of(cls, base: Optional["LogitsProcessors"] = None, **kw) -> Optional["LogitsProcessors"]:
        """``base`` (may be None) with the keywords that are not None put on top; None when nothing is left switched on"""
        kw = {k: v for k, v in kw.items() if v is not None}
        if base is not None and not isinstance(base, cls):
            raise CapdecError(f"logits_processors must be a LogitsProcessors, got {type(base).__name__}")
        p = dataclasses.replace(base, **kw) if base is not None else cls(**kw)
        return p if p.active else None


MAX_PHRASES, MAX_PHRASE_TOKENS = 4, 4       # capdec_decode_beam_constrained's phrase table: [n, 4, 4]


def pack_phrases(phrases_per_caption) -> np.ndarray:
    """[[phrase, ...] per caption], a phrase a sequence of token ids -> the int32 [n, 4, 4] table of
    capdec_decode_beam_constrained, unused places -1.  More than 4 phrases for a caption, an empty phrase or one of more
    than 4 tokens is a CapdecError."""
    rows = [list(phs) for phs in phrases_per_caption]
    out = np.full((len(rows), MAX_PHRASES, MAX_PHRASE_TOKENS), -1, dtype=np.int32)
    for r, phs in enumerate(rows):
        if len(phs) > MAX_PHRASES:
            raise CapdecError(f"constrained beam search: caption {r} has {len(phs)} phrases, at most {MAX_PHRASES} are supported")
        for c, ph in enumerate(phs):
            ph = [int(t) for t in ph]
            if not 1 <= len(ph) <= MAX_PHRASE_TOKENS:
                raise CapdecError(f"constrained beam search: phrase {c} of caption {r} has {len(ph)} tokens, 1..{MAX_PHRASE_TOKENS} "
                                  f"are supported")
            out[r, c, :len(ph)] = ph
    return out


class Engine:
    """One context per GPU / rank."""

    def __init__(self, device: int = 0, kv_budget_bytes: int = 0, measure: bool = False):
        """measure=True: the context lives in libcapdec_hip_measure.so (the product library plus the diverged-beam hook)
        -- bench.py's untimed tail and one parity test only, never the product path"""
        if not torch.cuda.is_available():
            raise CapdecError("capdec_amd needs a HIP device (MI355X); none is visible and there is no CPU fallback")
        if measure:
            if not os.path.exists(_capi.MEASURE_LIB_PATH):
                raise CapdecError(f"{_capi.MEASURE_LIB_PATH} is missing: run `python -m capdec_amd.build --measure`")
            self.lib = _capi.load_library(_capi.MEASURE_LIB_PATH)
        else:
            self.lib = _capi.load_library()
        self.measure = bool(measure)
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        h = C.c_void_p()
        self._chk(self.lib.capdec_create(self.device_index, C.byref(h)), "capdec_create")
        self._h = h
        if kv_budget_bytes:
            self._chk(self.lib.capdec_set_kv_budget(self._h, kv_budget_bytes), "set_kv_budget")
        self.gpt_dims: Optional[Dict[str, int]] = None
        self.mapper: Optional[Dict[str, int]] = None
        self.comm: Optional[Tuple[int, int]] = None          # (rank, world) of the C-ABI RCCL communicator, if any

    def _chk(self, rc: int, what: str = ""):
        check(rc, what, self.lib)

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.capdec_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _sync_stream(self):
        """run on torch's current stream so torch copies and our kernels stay ordered"""
        s = torch.cuda.current_stream(self.device).cuda_stream
        self._chk(self.lib.capdec_set_stream(self._h, C.c_void_p(s)), "set_stream")

    def synchronize(self):
        self._chk(self.lib.capdec_synchronize(self._h), "synchronize")

    def _dev(self, t: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
        return t.to(device=self.device, dtype=dtype).contiguous()

    # ------------------------------------------------------------------ weights
    def load_gpt2(self, sd: Dict[str, torch.Tensor], prefix: str = "gpt.", n_head: int = 12, ln_eps: float = 1e-5):
        """Accepts the reference checkpoint layout (train.py:359-371): tied
        ``gpt.lm_head.weight`` is checked against wte; transformers-4.24 buffers
        ``h.{i}.attn.bias`` / ``.attn.masked_bias`` are ignored."""
        t = prefix + "transformer."
        wte = _f32(sd[t + "wte.weight"])
        lm = sd.get(prefix + "lm_head.weight")
        if lm is not None and lm.data_ptr() != sd[t + "wte.weight"].data_ptr():
            if not torch.equal(lm.float().cpu(), sd[t + "wte.weight"].float().cpu()):
                raise CapdecError("checkpoint lm_head.weight differs from wte.weight (untied heads are not supported)")
        wpe = _f32(sd[t + "wpe.weight"])
        n_layer = 0
        while f"{t}h.{n_layer}.ln_1.weight" in sd:
            n_layer += 1
        if n_layer == 0:
            raise CapdecError(f"no GPT-2 blocks under {t!r}")
        keep = [wte, wpe]
        layers = (_capi.Gpt2Layer * n_layer)()
        names = [("ln_1_w", "ln_1.weight"), ("ln_1_b", "ln_1.bias"), ("c_attn_w", "attn.c_attn.weight"),
                 ("c_attn_b", "attn.c_attn.bias"), ("c_proj_w", "attn.c_proj.weight"), ("c_proj_b", "attn.c_proj.bias"),
                 ("ln_2_w", "ln_2.weight"), ("ln_2_b", "ln_2.bias"), ("c_fc_w", "mlp.c_fc.weight"),
                 ("c_fc_b", "mlp.c_fc.bias"), ("mlp_c_proj_w", "mlp.c_proj.weight"), ("mlp_c_proj_b", "mlp.c_proj.bias")]
        for i in range(n_layer):
            for field, key in names:
                a = _f32(sd[f"{t}h.{i}.{key}"])
                keep.append(a)
                setattr(layers[i], field, _fp(a))
        d = wte.shape[1]
        if tuple(_f32(sd[f"{t}h.0.attn.c_attn.weight"]).shape) != (d, 3 * d):
            raise CapdecError("c_attn.weight must be Conv1D layout [d, 3d]")
        lnw, lnb = _f32(sd[t + "ln_f.weight"]), _f32(sd[t + "ln_f.bias"])
        keep += [lnw, lnb]
        w = _capi.Gpt2Weights(n_layer, n_head, d, wte.shape[0], wpe.shape[0], ln_eps, _fp(wte), _fp(wpe), layers,
                              _fp(lnw), _fp(lnb))
        self._chk(self.lib.capdec_load_gpt2(self._h, C.byref(w)), "capdec_load_gpt2")
        self.gpt_dims = dict(n_layer=n_layer, n_head=n_head, d=d, vocab=wte.shape[0], n_pos=wpe.shape[0])

    def load_mapper_mlp(self, sd: Dict[str, torch.Tensor], prefix: str = "clip_project."):
        w1, b1 = _f32(sd[prefix + "model.0.weight"]), _f32(sd[prefix + "model.0.bias"])
        w2, b2 = _f32(sd[prefix + "model.2.weight"]), _f32(sd[prefix + "model.2.bias"])
        d = self.gpt_dims["d"] if self.gpt_dims else 768
        hidden, D = w1.shape
        P = w2.shape[0] // d
        self._chk(self.lib.capdec_load_mapper_mlp(self._h, D, P, hidden, _fp(w1), _fp(b1), _fp(w2), _fp(b2)),
              "capdec_load_mapper_mlp")
        self.mapper = dict(kind="mlp", D=D, P=P, d=d)

    @staticmethod
    def _tmapper_layers(sd: Dict[str, torch.Tensor], stem: str, count: int, keep: list, shapes=None):
        """a ``TMapperLayer`` array from the tensors ``{stem}{i}.{key}``; the host copies go to ``keep`` (they must outlive
        the load call).  ``shapes(i)``: field -> the shape layer i's tensor must have (unchecked when None)"""
        layers = (_capi.TMapperLayer * count)()
        for i in range(count):
            want = shapes(i) if shapes else None
            for field, key in _capi.TMAPPER_LAYER:
                a = _f32(sd[f"{stem}{i}.{key}"])
                if want and tuple(a.shape) != want[field]:
                    raise CapdecError(f"mapper: {stem}{i}.{key} is {tuple(a.shape)}, expected {want[field]}")
                keep.append(a)
                setattr(layers[i], field, _fp(a))
        return layers

    def load_mapper_transformer(self, sd: Dict[str, torch.Tensor], prefix: str = "clip_project.", num_heads: int = 8):
        lw, lb = _f32(sd[prefix + "linear.weight"]), _f32(sd[prefix + "linear.bias"])
        pc = _f32(sd[prefix + "prefix_const"])
        P, d = pc.shape
        clip_len = lw.shape[0] // d
        stem = prefix + "transformer.layers."
        n_layers = 0
        while f"{stem}{n_layers}.norm1.weight" in sd:
            n_layers += 1
        keep = [lw, lb, pc]
        layers = self._tmapper_layers(sd, stem, n_layers, keep)
        hid = sd[f"{stem}0.mlp.fc1.weight"].shape[0]
        w = _capi.TMapperWeights(lw.shape[1], P, clip_len, n_layers, num_heads, d, hid, _fp(lw), _fp(lb), _fp(pc), layers)
        self._chk(self.lib.capdec_load_mapper_transformer(self._h, C.byref(w)), "capdec_load_mapper_transformer")
        self.mapper = dict(kind="transformer", D=lw.shape[1], P=P, d=d, clip_length=clip_len, num_layers=n_layers)

    def load_mapper_encdec(self, sd: Dict[str, torch.Tensor], prefix: str = "clip_project.", num_heads: int = 8):
        """TransformerEncoderDecoder (MappingType.TransformerDecoder): geometry from the tensors -- the encoder's width
        from ref_encoder's first norm (512 in the reference), its depth L from the keys; the decoder has 2 L layers."""
        lw, lb = _f32(sd[prefix + "linear.weight"]), _f32(sd[prefix + "linear.bias"])
        pc = _f32(sd[prefix + "prefix_const"])
        P, d = pc.shape
        n_layers = 0
        while f"{prefix}ref_encoder.layers.{n_layers}.norm1.weight" in sd:
            n_layers += 1
        if n_layers == 0 or f"{prefix}prefix_decoder.layers.{2 * n_layers - 1}.norm1.weight" not in sd or \
                f"{prefix}prefix_decoder.layers.{2 * n_layers}.norm1.weight" in sd:
            raise CapdecError(f"encoder-decoder mapper: {n_layers} ref_encoder layers need {2 * n_layers} prefix_decoder layers")
        enc = sd[f"{prefix}ref_encoder.layers.0.norm1.weight"].shape[0]
        clip_len = lw.shape[0] // enc
        keep = [lw, lb, pc]

        def stack(which: str, count: int, width: int):
            hid = sd[f"{prefix}{which}.layers.0.mlp.fc1.weight"].shape[0]

            def shapes(i: int):      # keys / values of an even (cross) decoder layer come from the encoder's rows
                ref = width if which == "ref_encoder" or i % 2 == 1 else enc
                return {"norm1_w": (width,), "norm1_b": (width,), "to_queries_w": (width, width),
                        "to_keys_values_w": (2 * width, ref), "project_w": (width, width), "project_b": (width,),
                        "norm2_w": (width,), "norm2_b": (width,), "fc1_w": (hid, width), "fc1_b": (hid,),
                        "fc2_w": (width, hid), "fc2_b": (width,)}
            return self._tmapper_layers(sd, f"{prefix}{which}.layers.", count, keep, shapes), hid

        if lw.shape[0] != clip_len * enc or tuple(lb.shape) != (clip_len * enc,):
            raise CapdecError(f"encoder-decoder mapper: linear.weight rows {lw.shape[0]} are not a multiple of the encoder width {enc}")
        enc_layers, enc_hid = stack("ref_encoder", n_layers, enc)
        dec_layers, dec_hid = stack("prefix_decoder", 2 * n_layers, d)
        w = _capi.EDMapperWeights(lw.shape[1], P, clip_len, n_layers, num_heads, d, enc, enc_hid, dec_hid, _fp(lw), _fp(lb),
                                  _fp(pc), enc_layers, dec_layers)
        self._chk(self.lib.capdec_load_mapper_encdec(self._h, C.byref(w)), "capdec_load_mapper_encdec")
        self.mapper = dict(kind="transformer_decoder", D=lw.shape[1], P=P, d=d, clip_length=clip_len, num_layers=n_layers,
                           enc_dim=enc)

    # ------------------------------------------------------------------ prefix stage
    def normalize_prefix(self, x: torch.Tensor, normalize: bool = True, offset: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = self._dev(x)
        n, dim = x.shape
        out = torch.empty_like(x)
        if n == 0:            # an empty shard (world > N): nothing to launch, no NULL pointer into the C ABI
            return out
        off = self._dev(offset).reshape(-1) if offset is not None else None
        self._sync_stream()
        self._chk(self.lib.capdec_normalize_prefix(self._h, x.data_ptr(), n, dim, int(normalize),
                                               off.data_ptr() if off is not None else None, out.data_ptr()),
              "capdec_normalize_prefix")
        return out

    def noise_inject(self, x: torch.Tensor, variance: float, offset: Optional[torch.Tensor] = None,
                     uniform: bool = False, dont_norm: bool = False, seed: int = 0,
                     noise: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = self._dev(x)
        n, dim = x.shape
        out = torch.empty_like(x)
        if n == 0:
            return out
        off = self._dev(offset).reshape(-1) if offset is not None else None
        nz = self._dev(noise) if noise is not None else None
        uu = self._dev(u) if u is not None else None
        self._sync_stream()
        self._chk(self.lib.capdec_noise_inject(self._h, x.data_ptr(), n, dim, float(variance),
                                           off.data_ptr() if off is not None else None, int(uniform), int(dont_norm),
                                           int(seed) & 0xFFFFFFFFFFFFFFFF, nz.data_ptr() if nz is not None else None,
                                           uu.data_ptr() if uu is not None else None, out.data_ptr()),
              "capdec_noise_inject")
        return out

    def mapper_forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.mapper is None:
            raise CapdecError("no mapper loaded")
        x = self._dev(x)
        n = x.shape[0]
        if x.shape[1] != self.mapper["D"]:
            raise CapdecError(f"mapper expects prefix_dim {self.mapper['D']}, got {x.shape[1]}")
        out = torch.empty(n, self.mapper["P"], self.mapper["d"], device=self.device, dtype=torch.float32)
        if n:
            self._sync_stream()
            self._chk(self.lib.capdec_mapper_forward(self._h, x.data_ptr(), n, out.data_ptr()), "capdec_mapper_forward")
        return out

    # ------------------------------------------------------------------ CLIP towers
    def _clip_blocks(self, sd, prefix: str, layers: int, keep: list):
        blocks = (_capi.ClipBlock * layers)()
        names = [("ln_1_w", "ln_1.weight"), ("ln_1_b", "ln_1.bias"), ("in_proj_w", "attn.in_proj_weight"),
                 ("in_proj_b", "attn.in_proj_bias"), ("out_proj_w", "attn.out_proj.weight"),
                 ("out_proj_b", "attn.out_proj.bias"), ("ln_2_w", "ln_2.weight"), ("ln_2_b", "ln_2.bias"),
                 ("c_fc_w", "mlp.c_fc.weight"), ("c_fc_b", "mlp.c_fc.bias"), ("c_proj_w", "mlp.c_proj.weight"),
                 ("c_proj_b", "mlp.c_proj.bias")]
        for i in range(layers):
            for field, key in names:
                a = _f32(sd[f"{prefix}transformer.resblocks.{i}.{key}"])
                keep.append(a)
                setattr(blocks[i], field, _fp(a))
        return blocks

    @staticmethod
    def _count_blocks(sd, prefix: str) -> int:
        n = 0
        while f"{prefix}transformer.resblocks.{n}.ln_1.weight" in sd:
            n += 1
        return n

    def load_clip(self, sd: Dict[str, torch.Tensor], text: bool = True, vision: bool = True):
        """OpenAI CLIP state dict (what `clip.load(...)[0].state_dict()` holds; fp16 weights are upcast).  The visual
        tower is a ViT (`visual.class_embedding` present) or a ModifiedResNet (`visual.layer1...`: RN50x4, the
        reference's default backbone)."""
        keep: list = []
        if text:
            te, pe = _f32(sd["token_embedding.weight"]), _f32(sd["positional_embedding"])
            proj = _f32(sd["text_projection"])
            lw, lb = _f32(sd["ln_final.weight"]), _f32(sd["ln_final.bias"])
            keep += [te, pe, proj, lw, lb]
            layers = self._count_blocks(sd, "")
            width = te.shape[1]
            w = _capi.ClipTextWeights(pe.shape[0], te.shape[0], width, width // 64, layers, proj.shape[1], _fp(te),
                                      _fp(pe), self._clip_blocks(sd, "", layers, keep), _fp(lw), _fp(lb), _fp(proj))
            self._chk(self.lib.capdec_load_clip_text(self._h, C.byref(w)), "capdec_load_clip_text")
            self.clip_text = dict(context_length=pe.shape[0], embed_dim=proj.shape[1], vocab=te.shape[0])
        if vision and "visual.layer1.0.conv1.weight" in sd:
            self._load_clip_resnet(sd)
        elif vision:
            if "visual.conv1.weight" not in sd or "visual.class_embedding" not in sd:
                raise CapdecError("no visual tower in the state dict (neither visual.class_embedding nor visual.layer1)")
            cw = _f32(sd["visual.conv1.weight"])
            ce, pe = _f32(sd["visual.class_embedding"]), _f32(sd["visual.positional_embedding"])
            l1w, l1b = _f32(sd["visual.ln_pre.weight"]), _f32(sd["visual.ln_pre.bias"])
            l2w, l2b = _f32(sd["visual.ln_post.weight"]), _f32(sd["visual.ln_post.bias"])
            proj = _f32(sd["visual.proj"])
            keep += [cw, ce, pe, l1w, l1b, l2w, l2b, proj]
            width, patch = cw.shape[0], cw.shape[-1]
            image = int(round((pe.shape[0] - 1) ** 0.5)) * patch
            layers = self._count_blocks(sd, "visual.")
            w = _capi.ClipVisionWeights(image, patch, width, width // 64, layers, proj.shape[1], _fp(cw), _fp(ce), _fp(pe),
                                        _fp(l1w), _fp(l1b), self._clip_blocks(sd, "visual.", layers, keep), _fp(l2w),
                                        _fp(l2b), _fp(proj))
            self._chk(self.lib.capdec_load_clip_vision(self._h, C.byref(w)), "capdec_load_clip_vision")
            self.clip_vision = dict(image_size=image, embed_dim=proj.shape[1])

    def _load_clip_resnet(self, sd: Dict[str, torch.Tensor]):
        """ModifiedResNet tower (`visual.conv1..3`, `visual.layer1..4`, `visual.attnpool`): every convolution goes
        over with its BatchNorm statistics; the library folds them at load time."""
        keep: list = []

        def conv_bn(conv: str, bn: str) -> _capi.ConvBn:
            if conv + ".weight" not in sd:
                return _capi.ConvBn()
            w = _f32(sd[conv + ".weight"])
            t = [w] + [_f32(sd[f"{bn}.{k}"]) for k in ("weight", "bias", "running_mean", "running_var")]
            keep.extend(t)
            if w.shape[2] != w.shape[3]:
                raise CapdecError(f"{conv}: square kernels only")
            return _capi.ConvBn(*[_fp(x) for x in t], w.shape[1], w.shape[0], w.shape[2])

        stem = (_capi.ConvBn * 3)(*[conv_bn(f"visual.conv{i}", f"visual.bn{i}") for i in (1, 2, 3)])
        layers = [len({k.split(".")[2] for k in sd if k.startswith(f"visual.layer{li}.")}) for li in (1, 2, 3, 4)]
        blocks = []
        for li, nb in enumerate(layers, start=1):
            for b in range(nb):
                p = f"visual.layer{li}.{b}."
                blocks += [conv_bn(p + f"conv{i}", p + f"bn{i}") for i in (1, 2, 3)]
                blocks.append(conv_bn(p + "downsample.0", p + "downsample.1"))
        barr = (_capi.ConvBn * len(blocks))(*blocks)
        a = "visual.attnpool."
        pos = _f32(sd[a + "positional_embedding"])
        names = ["q_proj", "k_proj", "v_proj", "c_proj"]
        proj = [(_f32(sd[a + n + ".weight"]), _f32(sd[a + n + ".bias"])) for n in names]
        keep += [pos] + [t for pr in proj for t in pr]
        width = sd["visual.layer1.0.conv1.weight"].shape[0]
        image = int(round((pos.shape[0] - 1) ** 0.5)) * 32
        embed = proj[3][0].shape[0]
        w = _capi.ClipResNetWeights(image, width, embed, (C.c_int * 4)(*layers), stem, barr, _fp(pos),
                                    *[_fp(t) for pr in proj for t in pr])
        self._chk(self.lib.capdec_load_clip_resnet(self._h, C.byref(w)), "capdec_load_clip_resnet")
        self.clip_vision = dict(image_size=image, embed_dim=embed, kind="resnet")

    def clip_encode_text(self, tokens: torch.Tensor) -> torch.Tensor:
        t = self._dev(tokens, torch.int32)
        n = t.shape[0]
        if t.shape[1] != self.clip_text["context_length"]:
            raise CapdecError(f"token rows must have context_length {self.clip_text['context_length']}")
        out = torch.empty(n, self.clip_text["embed_dim"], device=self.device, dtype=torch.float32)
        if n:
            self._sync_stream()
            self._chk(self.lib.capdec_clip_encode_text(self._h, t.data_ptr(), n, out.data_ptr()), "capdec_clip_encode_text")
        return out

    def clip_encode_image(self, pixels: torch.Tensor) -> torch.Tensor:
        x = self._dev(pixels)
        n, S = x.shape[0], self.clip_vision["image_size"]
        if tuple(x.shape[1:]) != (3, S, S):
            raise CapdecError(f"images must be [n, 3, {S}, {S}] (already preprocessed)")
        out = torch.empty(n, self.clip_vision["embed_dim"], device=self.device, dtype=torch.float32)
        if n:
            self._sync_stream()
            self._chk(self.lib.capdec_clip_encode_image(self._h, x.data_ptr(), n, out.data_ptr()), "capdec_clip_encode_image")
        return out

    # ------------------------------------------------------------------ GPT-2
    def gpt2_logits(self, embeds: torch.Tensor, all_positions: bool = True) -> torch.Tensor:
        e = self._dev(embeds)
        n, L, d = e.shape
        V = self.gpt_dims["vocab"]
        out = torch.empty((n, L, V) if all_positions else (n, V), device=self.device, dtype=torch.float32)
        self._sync_stream()
        self._chk(self.lib.capdec_gpt2_logits(self._h, e.data_ptr(), n, L, int(all_positions), out.data_ptr()),
              "capdec_gpt2_logits")
        return out

    def cross_entropy(self, logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100) -> torch.Tensor:
        """mean token cross-entropy of ``logits`` [..., V] against ``labels`` [...] on the device (capdec_cross_entropy);
        rows with ``labels == ignore_index`` are skipped -- what ``nnf.cross_entropy`` computes at train.py:349"""
        V = logits.shape[-1]
        lg = self._dev(logits).reshape(-1, V)
        lab = self._dev(labels.reshape(-1), torch.int32)
        out = torch.empty(1, device=self.device, dtype=torch.float32)
        self._sync_stream()
        self._chk(self.lib.capdec_cross_entropy(self._h, lg.data_ptr(), V, lab.data_ptr(), lg.shape[0], V, int(ignore_index),
                                            out.data_ptr()), "capdec_cross_entropy")
        return out[0]

    def wte(self, ids: torch.Tensor) -> torch.Tensor:
        shape = tuple(ids.shape)
        i = self._dev(ids.reshape(-1), torch.int32)
        out = torch.empty(i.numel(), self.gpt_dims["d"], device=self.device, dtype=torch.float32)
        self._sync_stream()
        self._chk(self.lib.capdec_wte_lookup(self._h, i.data_ptr(), i.numel(), out.data_ptr()), "capdec_wte_lookup")
        return out.view(*shape, -1)

    # ------------------------------------------------------------------ decode
    def set_logits_processors(self, processors: Optional[LogitsProcessors] = None):
        """the processors of the following decode calls (capdec_set_logits_processors; None: none).  The ``logit_bias`` of
        ``processors`` is NOT touched here: :meth:`set_logit_bias`"""
        if processors is None:
            self._chk(self.lib.capdec_set_logits_processors(self._h, None), "set_logits_processors")
            return
        if not isinstance(processors, LogitsProcessors):
            raise CapdecError(f"set_logits_processors takes a LogitsProcessors, got {type(processors).__name__}")
        st = _capi.LogitsProcessors(float(processors.repetition_penalty), int(processors.no_repeat_ngram_size),
                                    int(processors.min_length), int(processors.top_k))
        self._chk(self.lib.capdec_set_logits_processors(self._h, C.byref(st)), "set_logits_processors")

    def set_logit_bias(self, bias=None):
        """a constant added to every row's logits in the following decode calls (capdec_set_logit_bias): a host vector
        [vocab] of finite or ``-inf`` entries, validated by the library and uploaded once; None: none"""
        if bias is None:
            self._chk(self.lib.capdec_set_logit_bias(self._h, None, 0), "set_logit_bias")
            return
        b = bias.detach().to("cpu", torch.float32).numpy() if isinstance(bias, torch.Tensor) else np.asarray(bias, dtype=np.float32)
        b = np.ascontiguousarray(b.reshape(-1))
        self._chk(self.lib.capdec_set_logit_bias(self._h, _fp(b), int(b.shape[0])), "set_logit_bias")

    @contextlib.contextmanager
    def _processors(self, base=None, **kw):
        """set the processors (and the bias) for the one decode call inside, clear them afterwards -- also when the call
        raises.  With nothing switched on the context's state is left alone."""
        p = LogitsProcessors.of(base, **kw)
        if p is None:
            yield
            return
        try:
            self.set_logits_processors(p)
            if p.logit_bias is not None:
                self.set_logit_bias(p.logit_bias)
            yield
        finally:
            self.set_logits_processors(None)
            self.set_logit_bias(None)

    def decode_greedy(self, prefix_embed: torch.Tensor, stop_id: int, entry_length: int = 67,
                      alt_stop_id: int = 764, *, repetition_penalty: Optional[float] = None,
                      no_repeat_ngram_size: Optional[int] = None, min_length: Optional[int] = None,
                      logit_bias=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The keyword-only processors (None: off) are set for this call and cleared after it; without any, the call
        runs under whatever :meth:`set_logits_processors` / :meth:`set_logit_bias` left on the context."""
        with self._processors(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                              min_length=min_length, logit_bias=logit_bias):
            return self._decode_greedy(prefix_embed, stop_id, entry_length, alt_stop_id)

    def _decode_greedy(self, prefix_embed, stop_id, entry_length, alt_stop_id):
        p = self._dev(prefix_embed)
        n, P, _ = p.shape
        ids = torch.empty(n, entry_length, device=self.device, dtype=torch.int32)
        lens = torch.empty(n, device=self.device, dtype=torch.int32)
        self._sync_stream()
        self._chk(self.lib.capdec_decode_greedy(self._h, p.data_ptr(), n, P, int(stop_id), int(alt_stop_id),
                                            int(entry_length), ids.data_ptr(), lens.data_ptr()), "capdec_decode_greedy")
        return ids, lens

    def decode_sample(self, prefix_embed: torch.Tensor, stop_id: int, entry_length: int = 67, temperature: float = 1.0,
                      top_p: float = 0.8, seed: int = 0, u: Optional[torch.Tensor] = None, alt_stop_id: int = 764,
                      return_logp: bool = False, *, repetition_penalty: Optional[float] = None,
                      no_repeat_ngram_size: Optional[int] = None, min_length: Optional[int] = None, logit_bias=None,
                      top_k: Optional[int] = None):
        """nucleus-sampling decode (capdec_decode_sample): -> ids [n, T] (zero padded), lens [n] (including the stop
        token) and, with ``return_logp``, logp [n, T] of the chosen tokens under the unfiltered temperature-scaled
        distribution.  ``u`` [n, T] in [0, 1) injects the uniforms; None draws them from the device Philox keyed by
        (``seed``, caption index, step).  The keyword-only processors as in :meth:`decode_greedy`, plus ``top_k``"""
        with self._processors(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                              min_length=min_length, logit_bias=logit_bias, top_k=top_k):
            return self._decode_sample(prefix_embed, stop_id, entry_length, temperature, top_p, seed, u, alt_stop_id,
                                       return_logp)

    def _decode_sample(self, prefix_embed, stop_id, entry_length, temperature, top_p, seed, u, alt_stop_id, return_logp):
        top_p, temperature = float(top_p), float(temperature)
        if top_p != top_p or temperature != temperature:
            raise CapdecError("decode_sample: top_p or temperature is NaN")
        n, P = int(prefix_embed.shape[0]), int(prefix_embed.shape[1])
        if u is not None and tuple(u.shape) != (n, int(entry_length)):
            raise CapdecError(f"decode_sample: u must be [n, entry_length] = ({n}, {int(entry_length)}), got {tuple(u.shape)}")
        p = self._dev(prefix_embed)
        uu = self._dev(u) if u is not None else None
        ids = torch.empty(n, entry_length, device=self.device, dtype=torch.int32)
        lens = torch.empty(n, device=self.device, dtype=torch.int32)
        logp = torch.empty(n, entry_length, device=self.device, dtype=torch.float32) if return_logp else None
        self._sync_stream()
        self._chk(self.lib.capdec_decode_sample(self._h, p.data_ptr(), n, P, int(stop_id), int(alt_stop_id), int(entry_length),
                                                temperature, top_p, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                uu.data_ptr() if uu is not None else None, ids.data_ptr(), lens.data_ptr(),
                                                logp.data_ptr() if logp is not None else None), "capdec_decode_sample")
        return (ids, lens, logp) if return_logp else (ids, lens)

    def decode_greedy_forced(self, prefix_embed: torch.Tensor, forced_ids: torch.Tensor):
        """teacher-forced greedy decode: feeds ``forced_ids`` [n, T] and returns (arg-max ids [n, T], stats [n, T, 3] =
        (top-1 logit, top-2 logit, logsumexp) of every step)"""
        p = self._dev(prefix_embed)
        f = self._dev(forced_ids, torch.int32)
        n, P, _ = p.shape
        T = f.shape[1]
        ids = torch.empty(n, T, device=self.device, dtype=torch.int32)
        stats = torch.empty(n, T, 3, device=self.device, dtype=torch.float32)
        self._sync_stream()
        self._chk(self.lib.capdec_decode_greedy_forced(self._h, p.data_ptr(), n, P, T, f.data_ptr(), ids.data_ptr(),
                                                   stats.data_ptr()), "capdec_decode_greedy_forced")
        return ids, stats

    def decode_beam(self, prefix_embed: torch.Tensor, stop_id: int, beam_size: int = 5, entry_length: int = 67,
                    temperature: float = 1.0, *, repetition_penalty: Optional[float] = None,
                    no_repeat_ngram_size: Optional[int] = None, min_length: Optional[int] = None, logit_bias=None):
        """-> ids [n, beam, T], lens [n, beam], mean-log-prob scores [n, beam] (sorted by score
        descending, like the list generate_beam returns) and order [n, beam] (reference's
        internal beam index of each returned row).  The keyword-only processors as in :meth:`decode_greedy`."""
        with self._processors(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                              min_length=min_length, logit_bias=logit_bias):
            return self._decode_beam(prefix_embed, stop_id, beam_size, entry_length, temperature)

    def _decode_beam(self, prefix_embed, stop_id, beam_size, entry_length, temperature):
        p = self._dev(prefix_embed)
        n, P, _ = p.shape
        ids = torch.empty(n, beam_size, entry_length, device=self.device, dtype=torch.int32)
        lens = torch.empty(n, beam_size, device=self.device, dtype=torch.int32)
        scores = torch.empty(n, beam_size, device=self.device, dtype=torch.float32)
        order = torch.empty(n, beam_size, device=self.device, dtype=torch.int32)
        self._sync_stream()
        self._chk(self.lib.capdec_decode_beam(self._h, p.data_ptr(), n, P, int(beam_size), int(stop_id), int(entry_length),
                                          float(temperature), ids.data_ptr(), lens.data_ptr(), scores.data_ptr(),
                                          order.data_ptr()), "capdec_decode_beam")
        return ids, lens, scores, order

    def decode_beam_groups(self, prefix_embed: torch.Tensor, stop_id: int, beam_size: int = 6, num_beam_groups: int = 3,
                           diversity_penalty: float = 0.5, entry_length: int = 67, temperature: float = 1.0, *,
                           repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                           min_length: Optional[int] = None, logit_bias=None):
        """diverse (group) beam search (capdec_decode_beam_groups): the beam decode with its ``beam_size`` slots split into
        ``num_beam_groups`` groups that are advanced in order, a token that earlier groups took at the same step costing
        ``diversity_penalty`` per taker.  -> ids [n, beam, T], lens [n, beam], scores [n, beam] (the penalised mean
        log-probs, sorted descending over all slots), order [n, beam] (the slot of each returned row: its group is
        ``order // (beam_size // num_beam_groups)``) and logp [n, beam] (the unpenalised log-prob sums, same order).  One
        group is :meth:`decode_beam`.  The keyword-only processors as in :meth:`decode_greedy`."""
        for name, v in (("beam_size", beam_size), ("num_beam_groups", num_beam_groups)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise CapdecError(f"decode_beam_groups: {name} must be an integer, got {v!r}")
        if not 1 <= beam_size <= 8:
            raise CapdecError("decode_beam_groups: beam_size must be in 1..8")
        if num_beam_groups < 1 or num_beam_groups > beam_size or beam_size % num_beam_groups:
            raise CapdecError(f"decode_beam_groups: num_beam_groups must be >= 1 and divide beam_size, got {num_beam_groups} "
                              f"groups for {beam_size} beams")
        t = diversity_penalty
        if isinstance(t, bool) or not isinstance(t, (int, float, np.floating)) or not (t >= 0 and math.isfinite(t)):
            raise CapdecError(f"decode_beam_groups: diversity_penalty must be a finite number >= 0, got {t!r}")
        with self._processors(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                              min_length=min_length, logit_bias=logit_bias):
            return self._decode_beam_groups(prefix_embed, stop_id, beam_size, num_beam_groups, float(diversity_penalty),
                                            entry_length, temperature)

    def _decode_beam_groups(self, prefix_embed, stop_id, beam_size, groups, penalty, entry_length, temperature):
        p = self._dev(prefix_embed)
        n, P, _ = p.shape
        ids = torch.empty(n, beam_size, entry_length, device=self.device, dtype=torch.int32)
        lens = torch.empty(n, beam_size, device=self.device, dtype=torch.int32)
        scores = torch.empty(n, beam_size, device=self.device, dtype=torch.float32)
        order = torch.empty(n, beam_size, device=self.device, dtype=torch.int32)
        logp = torch.empty(n, beam_size, device=self.device, dtype=torch.float32)
        self._sync_stream()
        self._chk(self.lib.capdec_decode_beam_groups(self._h, p.data_ptr(), n, P, int(beam_size), int(groups), float(penalty),
                                                     int(stop_id), int(entry_length), float(temperature), ids.data_ptr(),
                                                     lens.data_ptr(), scores.data_ptr(), order.data_ptr(), logp.data_ptr()),
                  "capdec_decode_beam_groups")
        return ids, lens, scores, order, logp

    def decode_beam_constrained(self, prefix_embed: torch.Tensor, phrases, stop_id: int, beam_size: int = 5,
                                entry_length: int = 67, temperature: float = 1.0, *,
                                repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                                min_length: Optional[int] = None, logit_bias=None):
        """lexically constrained beam search (capdec_decode_beam_constrained): the beam decode in which every phrase of a
        caption must occur as a contiguous token run (dynamic beam allocation; ``force_words_ids`` of
        ``transformers.generate``).  ``phrases``: per caption a list of up to 4 phrases of 1..4 token ids (see
        :func:`pack_phrases`), or an int32 array / tensor [n, 4, 4] with -1 in the unused places.  -> ids [n, beam, T], lens
        [n, beam], scores [n, beam] (mean log-probs), order [n, beam] (the slot of each returned row) and met [n, beam] (the
        bitmask of the phrases each returned row holds); rows sorted by phrases met, then score, descending.  No phrases
        is :meth:`decode_beam` through materialised logits.  The keyword-only processors as in :meth:`decode_greedy`."""
        if isinstance(beam_size, bool) or not isinstance(beam_size, (int, np.integer)) or not 1 <= beam_size <= 8:
            raise CapdecError(f"decode_beam_constrained: beam_size must be an integer in 1..8, got {beam_size!r}")
        n = int(prefix_embed.shape[0])
        if isinstance(phrases, torch.Tensor):
            ph = phrases.detach().to("cpu", torch.int32).numpy()
        elif isinstance(phrases, np.ndarray):
            ph = phrases.astype(np.int32)
        else:
            ph = pack_phrases(phrases)
        if ph.shape != (n, 4, 4):
            raise CapdecError(f"decode_beam_constrained: phrases must be [n, 4, 4] = ({n}, 4, 4), got {tuple(ph.shape)}")
        with self._processors(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                              min_length=min_length, logit_bias=logit_bias):
            return self._decode_beam_constrained(prefix_embed, np.ascontiguousarray(ph), stop_id, beam_size, entry_length,
                                                 temperature)

    def _decode_beam_constrained(self, prefix_embed, phrases, stop_id, beam_size, entry_length, temperature):
        p = self._dev(prefix_embed)
        n, P, _ = p.shape
        ph = torch.from_numpy(phrases).to(self.device)
        ids = torch.empty(n, beam_size, entry_length, device=self.device, dtype=torch.int32)
        lens = torch.empty(n, beam_size, device=self.device, dtype=torch.int32)
        scores = torch.empty(n, beam_size, device=self.device, dtype=torch.float32)
        order = torch.empty(n, beam_size, device=self.device, dtype=torch.int32)
        met = torch.empty(n, beam_size, device=self.device, dtype=torch.int32)
        self._sync_stream()
        self._chk(self.lib.capdec_decode_beam_constrained(self._h, p.data_ptr(), ph.data_ptr(), n, P, int(beam_size),
                                                          int(stop_id), int(entry_length), float(temperature),
                                                          ids.data_ptr(), lens.data_ptr(), scores.data_ptr(),
                                                          order.data_ptr(), met.data_ptr()),
                  "capdec_decode_beam_constrained")
        return ids, lens, scores, order, met

    def decode_contrastive(self, prefix_embed: torch.Tensor, top_k: int = 4, penalty_alpha: float = 0.6, stop_id: int = 13,
                           alt_stop_id: int = -1, entry_length: int = 67, return_trace: bool = False, *,
                           repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                           min_length: Optional[int] = None, logit_bias=None):
        """contrastive search (capdec_decode_contrastive; Su et al. 2022): per step the ``top_k`` most probable tokens are
        each fed through the model, and the one with the best ``(1 - penalty_alpha) * p - penalty_alpha * max cosine`` of
        its ln_f hidden state against those of the whole context so far is emitted.  -> ids [n, T] (zero padded), lens
        [n] (including the stop token; ``stop_id`` defaults to GPT-2's '.') and, with ``return_trace``, trace [n, T, 2] =
        (p, sim) of every chosen candidate.  ``penalty_alpha=0`` or ``top_k=1`` is :meth:`decode_greedy`.  Needs
        ``P + entry_length <= n_positions``.  The keyword-only processors as in :meth:`decode_greedy`."""
        if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)):
            raise CapdecError(f"decode_contrastive: top_k must be an integer, got {top_k!r}")
        if not 1 <= top_k <= 8:
            raise CapdecError(f"decode_contrastive: top_k must be in 1..8, got {top_k}")
        a = penalty_alpha
        if isinstance(a, bool) or not isinstance(a, (int, float, np.floating)) or not 0 <= a <= 1:
            raise CapdecError(f"decode_contrastive: penalty_alpha must be a number in [0, 1], got {a!r}")
        if isinstance(entry_length, bool) or not isinstance(entry_length, (int, np.integer)) or entry_length < 1:
            raise CapdecError(f"decode_contrastive: entry_length must be a positive integer, got {entry_length!r}")
        with self._processors(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                              min_length=min_length, logit_bias=logit_bias):
            return self._decode_contrastive(prefix_embed, int(top_k), float(a), stop_id, alt_stop_id, int(entry_length),
                                            bool(return_trace))

    def _decode_contrastive(self, prefix_embed, top_k, alpha, stop_id, alt_stop_id, entry_length, return_trace):
        p = self._dev(prefix_embed)
        n, P, _ = p.shape
        ids = torch.empty(n, entry_length, device=self.device, dtype=torch.int32)
        lens = torch.empty(n, device=self.device, dtype=torch.int32)
        trace = torch.empty(n, entry_length, 2, device=self.device, dtype=torch.float32) if return_trace else None
        self._sync_stream()
        self._chk(self.lib.capdec_decode_contrastive(self._h, p.data_ptr(), n, P, top_k, alpha, int(stop_id), int(alt_stop_id),
                                                     entry_length, ids.data_ptr(), lens.data_ptr(),
                                                     trace.data_ptr() if trace is not None else None),
                  "capdec_decode_contrastive")
        return (ids, lens, trace) if return_trace else (ids, lens)

    def decode_guided(self, prefix_embed: torch.Tensor, negative_embed: torch.Tensor, guidance_scale: float, stop_id: int,
                      beam_size: int = 1, entry_length: int = 67, temperature: float = 1.0, alt_stop_id: int = 764, *,
                      repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                      min_length: Optional[int] = None, logit_bias=None, return_order: bool = False):
        """classifier-free guidance (capdec_decode_guided; ``guidance_scale`` of ``transformers.generate``): every caption is
        decoded from ``prefix_embed`` [n, P, d] and, in lock-step with the same tokens, from its negative prefix --
        ``negative_embed`` [P, d] or [1, P, d] (one for all) or [n, P, d] -- and the next token comes from
        ``guidance_scale * log_softmax(l_cond) + (1 - guidance_scale) * log_softmax(l_neg)``, which takes the place of the
        raw logits in front of the processors.  ``beam_size`` 1 -> (ids [n, T], lens [n]) as :meth:`decode_greedy`
        (``alt_stop_id`` counts there only); 2..8 -> (ids [n, beam, T], lens, scores [n, beam]) sorted like
        :meth:`decode_beam`'s, plus its order [n, beam] with ``return_order``.  ``guidance_scale`` must be finite and >= 1; 1 is off: the plain call, bit for bit.  The
        keyword-only processors as in :meth:`decode_greedy`; under guidance they see log-probabilities (all <= 0)."""
        g = guidance_scale
        if isinstance(g, bool) or not isinstance(g, (int, float, np.floating, np.integer)) or not (g >= 1 and math.isfinite(g)):
            raise CapdecError(f"decode_guided: guidance_scale must be a finite number >= 1, got {g!r}")
        if isinstance(beam_size, bool) or not isinstance(beam_size, (int, np.integer)) or not 1 <= beam_size <= 8:
            raise CapdecError(f"decode_guided: beam_size must be an integer in 1..8, got {beam_size!r}")
        if isinstance(entry_length, bool) or not isinstance(entry_length, (int, np.integer)) or entry_length < 1:
            raise CapdecError(f"decode_guided: entry_length must be a positive integer, got {entry_length!r}")
        for name, t in (("prefix_embed", prefix_embed), ("negative_embed", negative_embed)):
            if not isinstance(t, torch.Tensor) or not torch.is_floating_point(t):
                raise CapdecError(f"decode_guided: {name} must be a floating-point tensor")
        if prefix_embed.dim() != 3:
            raise CapdecError(f"decode_guided: prefix_embed must be [n, P, d], got {tuple(prefix_embed.shape)}")
        n, P, d = (int(s) for s in prefix_embed.shape)
        neg = negative_embed.unsqueeze(0) if negative_embed.dim() == 2 else negative_embed
        if neg.dim() != 3 or tuple(neg.shape[1:]) != (P, d) or int(neg.shape[0]) not in (1, n):
            raise CapdecError(f"decode_guided: negative_embed must be [P, d], [1, P, d] or [n, P, d] = [{n}, {P}, {d}], got "
                              f"{tuple(negative_embed.shape)}")
        with self._processors(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                              min_length=min_length, logit_bias=logit_bias):
            out = self._decode_guided(prefix_embed, neg, float(g), stop_id, int(beam_size), int(entry_length), temperature,
                                      alt_stop_id)
        return out if return_order or beam_size == 1 else out[:3]

    def _decode_guided(self, prefix_embed, neg, gamma, stop_id, beam, entry_length, temperature, alt_stop_id):
        p, q = self._dev(prefix_embed), self._dev(neg)
        n, P, _ = p.shape
        shape = (n,) if beam == 1 else (n, beam)
        ids = torch.empty(*shape, entry_length, device=self.device, dtype=torch.int32)
        lens = torch.empty(*shape, device=self.device, dtype=torch.int32)
        scores = torch.empty(n, beam, device=self.device, dtype=torch.float32) if beam > 1 else None
        order = torch.empty(n, beam, device=self.device, dtype=torch.int32) if beam > 1 else None
        self._sync_stream()
        self._chk(self.lib.capdec_decode_guided(self._h, p.data_ptr(), q.data_ptr(), int(q.shape[0]), n, P, beam, gamma,
                                                int(stop_id), int(alt_stop_id), entry_length, float(temperature),
                                                ids.data_ptr(), lens.data_ptr(),
                                                scores.data_ptr() if scores is not None else None,
                                                order.data_ptr() if order is not None else None), "capdec_decode_guided")
        return (ids, lens) if beam == 1 else (ids, lens, scores, order)

    # ------------------------------------------------------------------ scoring
    def score(self,prefix_embed: torch.Tensor, tokens: torch.Tensor, lens=None, ignore_id: int = -1,
              temperature: float = 1.0, return_top1: bool = False):
        """teacher-forced log-probabilities of given captions (capdec_score): ``prefix_embed`` [n, P, d], ``tokens``
        [n, L], ``lens`` [n] in 0..L (None: every caption has L tokens) -> device tensors logp [n, L] (0 past ``lens``
        and where the label is ``ignore_id``), sum [n], count [n] and, with ``return_top1``, the arg-max id [n, L] of
        every scored position.  ``lens`` is read on the host (the call plans its chunks from it): pass a list, a numpy
        array or a host tensor to avoid a device round trip."""
        temperature = float(temperature)
        if temperature != temperature:
            raise CapdecError("score: temperature is NaN")
        if prefix_embed.dim() != 3 or tokens.dim() != 2 or prefix_embed.shape[0] != tokens.shape[0]:
            raise CapdecError(f"score: prefix_embed [n, P, d] and tokens [n, L] expected, got {tuple(prefix_embed.shape)} "
                              f"and {tuple(tokens.shape)}")
        n, P, L = int(prefix_embed.shape[0]), int(prefix_embed.shape[1]), int(tokens.shape[1])
        hl = None
        if lens is not None:
            hl = np.ascontiguousarray((lens.detach().cpu().numpy() if isinstance(lens, torch.Tensor) else np.asarray(lens))
                                      .reshape(-1).astype(np.int32))
            if hl.shape[0] != n:
                raise CapdecError(f"score: lens must have one entry per caption ({n}), got {hl.shape[0]}")
        p = self._dev(prefix_embed)
        t = self._dev(tokens, torch.int32)
        logp = torch.empty(n, L, device=self.device, dtype=torch.float32)
        ssum = torch.empty(n, device=self.device, dtype=torch.float32)
        count = torch.empty(n, device=self.device, dtype=torch.int32)
        top1 = torch.empty(n, L, device=self.device, dtype=torch.int32) if return_top1 else None
        self._sync_stream()
        self._chk(self.lib.capdec_score(self._h, p.data_ptr(), t.data_ptr(),
                                        hl.ctypes.data_as(_capi.c_int_p) if hl is not None else None, n, P, L, int(ignore_id),
                                        temperature, logp.data_ptr(), ssum.data_ptr(), count.data_ptr(),
                                        top1.data_ptr() if top1 is not None else None), "capdec_score")
        return (logp, ssum, count, top1) if return_top1 else (logp, ssum, count)

    def score_chunks(self) -> int:
        """how many chunks the last :meth:`score` call split its captions into (capdec_score_chunks)"""
        n = C.c_int(0)
        self._chk(self.lib.capdec_score_chunks(self._h, C.byref(n)), "score_chunks")
        return n.value

    # ------------------------------------------------------------------ prefix interpretation
    def nearest_tokens(self, x: torch.Tensor, k: int = 1, table: Optional[torch.Tensor] = None, return_sims: bool = False):
        """the ``k`` rows of ``table`` [V, d] (None: the loaded GPT-2's wte, whose normalised copy the library caches)
        nearest to every row of ``x`` [..., d] under cosine similarity (capdec_nearest_tokens; the contract: include/capdec.h)
        -> ids int32 [..., k], descending similarity, equal similarities in ascending id order, and with ``return_sims`` the
        similarities fp32 [..., k].  A row of ``x`` holding a NaN or an inf gets ids -1 and sims NaN."""
        if x.dim() < 1:
            raise CapdecError("nearest_tokens: x must be [..., d]")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise CapdecError(f"nearest_tokens: k must be an integer, got {k!r}")
        lead, d = tuple(x.shape[:-1]), int(x.shape[-1])
        t = None
        if table is not None:
            if table.dim() != 2 or int(table.shape[1]) != d:
                raise CapdecError(f"nearest_tokens: table must be [V, {d}], got {tuple(table.shape)}")
            t = self._dev(table)
        xs = self._dev(x).reshape(-1, d)
        rows = int(xs.shape[0])
        k = int(k)
        if not 1 <= k <= 8:
            raise CapdecError(f"nearest_tokens: k must be in 1..8, got {k}")
        ids = torch.empty(rows, k, device=self.device, dtype=torch.int32)
        sims = torch.empty(rows, k, device=self.device, dtype=torch.float32) if return_sims else None
        self._sync_stream()
        self._chk(self.lib.capdec_nearest_tokens(self._h, xs.data_ptr() if rows else None, rows, d,
                                                 t.data_ptr() if t is not None else None, int(t.shape[0]) if t is not None else 0,
                                                 int(k), ids.data_ptr() if rows else None,
                                                 sims.data_ptr() if sims is not None and rows else None), "capdec_nearest_tokens")
        ids = ids.view(*lead, int(k))
        return (ids, sims.view(*lead, int(k))) if return_sims else ids

    # ------------------------------------------------------------------ noise variance and modality offset
    MOMENT_ROWS = ("mean_a", "mean_b", "mean_diff", "std_a", "std_b", "std_diff", "absmean_diff")

    def embed_moments(self, a: torch.Tensor, b: Optional[torch.Tensor] = None, normalize: bool = True,
                      return_pair: bool = False) -> Dict[str, torch.Tensor]:
        """column moments of the paired embeddings ``a`` (images) and ``b`` (texts), both [n, dim], every row first divided
        by its L2 norm unless ``normalize`` is off (capdec_embed_moments; the contract: include/capdec.h) -> fp32 [dim]
        tensors ``mean_a, mean_b, mean_diff`` (= mean of b - a), ``std_a, std_b, std_diff`` (unbiased), ``absmean_diff``,
        and with ``return_pair`` ``pair`` [n, 2] = (||b_i - a_i||_2, ||b_i - a_i||_inf).  Without ``b`` only ``mean_a`` and
        ``std_a`` are computed; the others are 0."""
        if a.dim() != 2 or (b is not None and tuple(b.shape) != tuple(a.shape)):
            raise CapdecError("embed_moments: a and b must both be [n, dim]")
        if return_pair and b is None:
            raise CapdecError("embed_moments: return_pair needs b")
        n, dim = int(a.shape[0]), int(a.shape[1])
        xa = self._dev(a)
        xb = self._dev(b) if b is not None else None
        stats = torch.empty(7, dim, device=self.device, dtype=torch.float32)
        pair = torch.empty(n, 2, device=self.device, dtype=torch.float32) if return_pair else None
        self._sync_stream()
        self._chk(self.lib.capdec_embed_moments(self._h, xa.data_ptr() if n else None, xb.data_ptr() if xb is not None and n else None,
                                                n, dim, int(bool(normalize)), stats.data_ptr(),
                                                pair.data_ptr() if pair is not None and n else None), "capdec_embed_moments")
        out = {name: stats[i] for i, name in enumerate(self.MOMENT_ROWS)}
        if return_pair:
            out["pair"] = pair
        return out

    def group_distances(self, x: torch.Tensor, offsets, index: Optional[torch.Tensor] = None) -> torch.Tensor:
        """distances inside groups of rows of ``x`` [rows, W] (capdec_group_distances; the contract: include/capdec.h): group
        k is the rows ``index[offsets[k]:offsets[k + 1]]`` (``index`` None: those row numbers themselves), 1 to 8 rows each;
        ``offsets`` is a host vector [groups + 1].  -> fp32 [groups, 8]: pair L1 / (W c), pair L2 / (W c), pair L-inf / c, max
        pair L2 / sqrt(W), mean L2 to the group's centre, mean L-inf to it, c = g (g - 1) / 2, g."""
        if x.dim() != 2:
            raise CapdecError("group_distances: x must be [rows, W]")
        raw = (offsets.detach().cpu().numpy() if isinstance(offsets, torch.Tensor) else np.asarray(offsets)).reshape(-1)
        if raw.shape[0] < 1:
            raise CapdecError("group_distances: offsets must have groups + 1 entries")
        if not np.issubdtype(raw.dtype, np.integer) or int(raw.min()) < -2 ** 31 or int(raw.max()) >= 2 ** 31:
            raise CapdecError("group_distances: offsets must be integers that fit 32 bits")      # (astype would wrap them)
        off = np.ascontiguousarray(raw.astype(np.int32))
        groups = int(off.shape[0]) - 1
        idx = None
        if index is not None:
            idx = self._dev(index.reshape(-1), torch.int32)
            if groups and int(idx.shape[0]) < int(off[-1]):
                raise CapdecError(f"group_distances: offsets end at {int(off[-1])} but index has {int(idx.shape[0])} entries")
        xs = self._dev(x)
        out = torch.empty(groups, 8, device=self.device, dtype=torch.float32)
        self._sync_stream()
        self._chk(self.lib.capdec_group_distances(self._h, xs.data_ptr() if xs.numel() else None, int(xs.shape[0]), int(xs.shape[1]),
                                                  idx.data_ptr() if idx is not None and idx.numel() else None,
                                                  off.ctypes.data_as(_capi.c_int_p), groups,
                                                  out.data_ptr() if groups else None), "capdec_group_distances")
        return out

    # ------------------------------------------------------------------ CLIPScore and candidate order (clipscore.hip)
    def _host_offsets(self, what: str, offsets) -> np.ndarray:
        raw = (offsets.detach().cpu().numpy() if isinstance(offsets, torch.Tensor) else np.asarray(offsets)).reshape(-1)
        if raw.shape[0] < 1:
            raise CapdecError(f"{what}: offsets must have groups + 1 entries")
        if not np.issubdtype(raw.dtype, np.integer) or int(raw.min()) < -2 ** 31 or int(raw.max()) >= 2 ** 31:
            raise CapdecError(f"{what}: offsets must be integers that fit 32 bits")      # (astype would wrap them)
        return np.ascontiguousarray(raw.astype(np.int32))

    def clip_score(self, cand: torch.Tensor, img: torch.Tensor, offsets, ref: Optional[torch.Tensor] = None, ref_offsets=None,
                   w: float = 2.5) -> Tuple[torch.Tensor, torch.Tensor]:
        """CLIPScore / RefCLIPScore of candidate captions and their order per image (capdec_clip_score; the contract:
        include/capdec.h).  Image g (row g of ``img`` [groups, d]) owns the rows ``offsets[g]:offsets[g + 1]`` of ``cand``
        [rows, d], 0 to 64 of them, and the rows ``ref_offsets[g]:ref_offsets[g + 1]`` of ``ref`` [ref_rows, d]; both offset
        vectors are host vectors [groups + 1].  All rows are raw tower outputs.  -> (scores fp32 [rows, 4] = cos, w max(cos, 0),
        max(0, best reference cosine), their harmonic mean -- the last two NaN without references; order int32 [rows]: the row
        numbers of every image's candidates, best first), both on the device.  Needs no loaded weights."""
        if cand.dim() != 2 or img.dim() != 2 or int(img.shape[1]) != int(cand.shape[1]):
            raise CapdecError("clip_score: cand must be [rows, d] and img [groups, d]")
        if ref is not None and (ref.dim() != 2 or int(ref.shape[1]) != int(cand.shape[1])):
            raise CapdecError("clip_score: ref must be [ref_rows, d]")
        off = self._host_offsets("clip_score", offsets)
        groups = int(off.shape[0]) - 1
        if int(img.shape[0]) != groups:
            raise CapdecError(f"clip_score: {groups} groups but {int(img.shape[0])} image rows")
        roff = None
        if ref_offsets is not None:
            roff = self._host_offsets("clip_score", ref_offsets)
            if int(roff.shape[0]) != groups + 1:
                raise CapdecError(f"clip_score: ref_offsets must have {groups + 1} entries, got {int(roff.shape[0])}")
        rows, d = int(cand.shape[0]), int(cand.shape[1])
        xc, xi = self._dev(cand), self._dev(img)
        xr = self._dev(ref) if ref is not None else None
        scores = torch.empty(rows, 4, device=self.device, dtype=torch.float32)
        order = torch.empty(rows, device=self.device, dtype=torch.int32)
        ptr = lambda t: t.data_ptr() if t.numel() else None      # noqa: E731
        ref_ptr = None
        if xr is not None:       # an empty reference array is still "given" (the library refuses half a pair): it gets a
            held = xr if xr.numel() else torch.zeros(4, device=self.device)      # pointer that is not NULL; none of it is read
            ref_ptr = held.data_ptr()
        self._sync_stream()
        self._chk(self.lib.capdec_clip_score(self._h, ptr(xc), rows, d, ptr(xi), off.ctypes.data_as(_capi.c_int_p), groups,
                                             ref_ptr, int(xr.shape[0]) if xr is not None else 0,
                                             roff.ctypes.data_as(_capi.c_int_p) if roff is not None else None, float(w),
                                             ptr(scores), ptr(order)), "capdec_clip_score")
        return scores, order

    # ------------------------------------------------------------------ projection onto a support memory (memory.hip)
    MEMORY_MAX_ROWS, MEMORY_MAX_D = 4194304, 640

    def memory_load(self, mem: torch.Tensor):
        """keep the rows of ``mem`` [M, d] (text embeddings), L2-normalised, as the context's support memory
        (capdec_memory_load; the contract: include/capdec.h).  One memory per engine: a second load replaces the first.  M in
        1..4 194 304, d a multiple of 32 in 32..640.  A row holding a NaN or an inf makes the load fail and leaves the memory
        that was loaded before in place."""
        if mem.dim() != 2:
            raise CapdecError(f"memory_load: mem must be [M, d], got {tuple(mem.shape)}")
        rows, d = int(mem.shape[0]), int(mem.shape[1])
        if not 1 <= rows <= self.MEMORY_MAX_ROWS or d % 32 or not 32 <= d <= self.MEMORY_MAX_D:
            raise CapdecError(f"memory_load: M must be in 1..{self.MEMORY_MAX_ROWS} and d a multiple of 32 in 32..{self.MEMORY_MAX_D}, "
                              f"got {tuple(mem.shape)}")
        ms = self._dev(mem)
        self._sync_stream()
        self._chk(self.lib.capdec_memory_load(self._h, ms.data_ptr(), rows, d), "capdec_memory_load")
        self.memory = (rows, d)
        self._memory_owner = None          # (a SupportMemory that loads itself writes its own name here afterwards)

    def memory_free(self):
        """drop the support memory (capdec_memory_free); :meth:`memory_project` raises until the next load"""
        self._chk(self.lib.capdec_memory_free(self._h), "capdec_memory_free")
        self.memory = None
        self._memory_owner = None

    def memory_project(self, x: torch.Tensor, temperature: float = 0.01, return_info: bool = False):
        """every row of ``x`` [..., d] replaced by the softmax-weighted combination of the memory's unit rows, weights
        ``softmax(cosine / temperature)``, L2-normalised (capdec_memory_project; DeCap's projection) -> fp32 [..., d] on the
        device.  With ``return_info`` also ``{"lse": logsumexp of the scaled similarities, "nearest": int32 index of the most
        similar memory row (the lowest among equals), "max_sim": its cosine}``, each [...].  A row holding a NaN or an inf
        comes back as NaN (``nearest`` -1).  A row's results do not depend on the other rows of the call."""
        if x.dim() < 1:
            raise CapdecError("memory_project: x must be [..., d]")
        lead, d = tuple(x.shape[:-1]), int(x.shape[-1])
        xs = self._dev(x).reshape(-1, d)
        rows = int(xs.shape[0])
        out = torch.empty(rows, d, device=self.device, dtype=torch.float32)
        info = None
        if return_info:
            info = {"lse": torch.empty(rows, device=self.device, dtype=torch.float32),
                    "nearest": torch.empty(rows, device=self.device, dtype=torch.int32),
                    "max_sim": torch.empty(rows, device=self.device, dtype=torch.float32)}
        ptr = lambda t: t.data_ptr() if t is not None and rows else None      # noqa: E731
        self._sync_stream()
        self._chk(self.lib.capdec_memory_project(self._h, ptr(xs), rows, d, float(temperature), ptr(out),
                                                 ptr(info["lse"]) if info else None, ptr(info["nearest"]) if info else None,
                                                 ptr(info["max_sim"]) if info else None), "capdec_memory_project")
        out = out.view(*lead, d)
        return (out, {k: v.view(*lead) for k, v in info.items()}) if return_info else out

    # ------------------------------------------------------------------ supervised modality bridger (bridger.hip)
    BRIDGER_MAX_LAYERS, BRIDGER_MAX_WIDTH, BRIDGER_MAX_BATCH = 16, 1024, 64

    def _bridger_dims(self, what: str) -> Tuple[int, ...]:
        dims = getattr(self, "bridger", None)
        if dims is None:
            raise CapdecError(f"{what}: no bridger is loaded (bridger_load)")
        return dims

    def _bridger_rows(self, what: str, x: torch.Tensor, y: Optional[torch.Tensor] = None) -> int:
        dims = self._bridger_dims(what)
        if x.dim() != 2 or int(x.shape[1]) != dims[0]:
            raise CapdecError(f"{what}: x must be [n, {dims[0]}], got {tuple(x.shape)}")
        if y is not None and tuple(y.shape) != (int(x.shape[0]), dims[-1]):
            raise CapdecError(f"{what}: y must be [{int(x.shape[0])}, {dims[-1]}], got {tuple(y.shape)}")
        return int(x.shape[0])

    def _bridger_batch(self, what: str, batch) -> int:
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or not 1 <= batch <= self.BRIDGER_MAX_BATCH:
            raise CapdecError(f"{what}: batch must be an integer in 1..{self.BRIDGER_MAX_BATCH}, got {batch!r}")
        return int(batch)

    def bridger_load(self, weights, biases):
        """load the supervised modality bridger (capdec_bridger_load; the contract: include/capdec.h): ``weights[l]`` is
        ``[dims[l + 1], dims[l]]`` (nn.Linear layout), ``biases[l]`` ``[dims[l + 1]]``; ReLU follows every layer but the last.
        1 to 16 layers, every width a multiple of 4 in 4..1024.  The momentum buffers and the loss scalars start at zero."""
        weights, biases = list(weights), list(biases)
        L = len(weights)
        if not 1 <= L <= self.BRIDGER_MAX_LAYERS or len(biases) != L:
            raise CapdecError(f"bridger_load: 1 to {self.BRIDGER_MAX_LAYERS} layers, one bias per weight (got {L} weights, "
                              f"{len(biases)} biases)")
        if any(w.dim() != 2 for w in weights):
            raise CapdecError("bridger_load: every weight must be [out, in]")
        dims = [int(weights[0].shape[1])] + [int(w.shape[0]) for w in weights]
        for l, (w, b) in enumerate(zip(weights, biases)):
            if int(w.shape[1]) != dims[l] or tuple(b.shape) != (dims[l + 1],):
                raise CapdecError(f"bridger_load: layer {l} must be a [{dims[l + 1]}, {dims[l]}] weight with a [{dims[l + 1]}] "
                                  f"bias, got {tuple(w.shape)} and {tuple(b.shape)}")
        for d in dims:
            if d % 4 or not 4 <= d <= self.BRIDGER_MAX_WIDTH:
                raise CapdecError(f"bridger_load: every width must be a multiple of 4 in 4..{self.BRIDGER_MAX_WIDTH}, got {d}")
        keep = [_f32(w) for w in weights] + [_f32(b) for b in biases]
        ptr = lambda ts: (_capi.c_float_p * L)(*[t.ctypes.data_as(_capi.c_float_p) for t in ts])      # noqa: E731
        self.bridger = None
        self._chk(self.lib.capdec_bridger_load(self._h, L, (C.c_int32 * (L + 1))(*dims), ptr(keep[:L]), ptr(keep[L:])),
                  "capdec_bridger_load")
        self.bridger = tuple(dims)

    def bridger_forward(self, x: torch.Tensor) -> torch.Tensor:
        """the bridger applied to ``x`` [n, dims[0]] -> fp32 [n, dims[L]] on the device; a row's result does not depend on n"""
        n = self._bridger_rows("bridger_forward", x)
        xs = self._dev(x)
        out = torch.empty(n, self.bridger[-1], device=self.device, dtype=torch.float32)
        if n:
            self._sync_stream()
            self._chk(self.lib.capdec_bridger_forward(self._h, xs.data_ptr(), n, out.data_ptr()), "capdec_bridger_forward")
        return out

    def bridger_train_step(self, x: torch.Tensor, y: torch.Tensor, lr: float = 0.001, momentum: float = 0.9,
                           return_loss: bool = True) -> Optional[float]:
        """one step of MSELoss + SGD with momentum on the batch (x [batch, dims[0]], y [batch, dims[L]], batch 1..64) ->
        the step's loss; ``return_loss=False`` only enqueues (read :meth:`bridger_loss` later)"""
        n = self._bridger_rows("bridger_train_step", x, y)
        self._bridger_batch("bridger_train_step", n)
        xs, ys = self._dev(x), self._dev(y)
        loss = C.c_float(0.0)
        self._sync_stream()
        self._chk(self.lib.capdec_bridger_train_step(self._h, xs.data_ptr(), ys.data_ptr(), n, float(lr), float(momentum),
                                                     C.byref(loss) if return_loss else None), "capdec_bridger_train_step")
        if not return_loss:
            self._bridger_keep = (xs, ys)                # the enqueued kernels still read them
            return None
        return float(loss.value)

    def bridger_train_epoch(self, x: torch.Tensor, y: torch.Tensor, batch: int = 32, lr: float = 0.001, momentum: float = 0.9):
        """one pass over the rows in consecutive batches of ``batch`` (the last may be short), every step enqueued from C;
        the epoch's loss is ``sum / steps`` of :meth:`bridger_loss`"""
        n = self._bridger_rows("bridger_train_epoch", x, y)
        batch = self._bridger_batch("bridger_train_epoch", batch)
        if n == 0:
            return
        xs, ys = self._dev(x), self._dev(y)
        self._sync_stream()
        self._chk(self.lib.capdec_bridger_train_epoch(self._h, xs.data_ptr(), ys.data_ptr(), n, batch, float(lr), float(momentum)),
                  "capdec_bridger_train_epoch")
        self._bridger_keep = (xs, ys)                    # the enqueued kernels still read them

    def bridger_eval(self, x: torch.Tensor, y: torch.Tensor, batch: int = 32) -> Tuple[float, int]:
        """(sum of the MSE losses of the consecutive batches of ``batch`` rows, number of batches) without an update"""
        n = self._bridger_rows("bridger_eval", x, y)
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
            raise CapdecError(f"bridger_eval: batch must be an integer >= 1, got {batch!r}")
        total, count = C.c_double(0.0), C.c_longlong(0)
        if n:
            xs, ys = self._dev(x), self._dev(y)
            self._sync_stream()
            self._chk(self.lib.capdec_bridger_eval(self._h, xs.data_ptr(), ys.data_ptr(), n, int(batch), C.byref(total),
                                                   C.byref(count)), "capdec_bridger_eval")
        return float(total.value), int(count.value)

    def bridger_loss(self, reset: bool = False) -> Tuple[float, float, int]:
        """(loss of the last step, fp64 sum of the steps' losses since the load or the last reset, number of those steps)"""
        self._bridger_dims("bridger_loss")
        last, total, n = C.c_float(0.0), C.c_double(0.0), C.c_longlong(0)
        self._chk(self.lib.capdec_bridger_loss(self._h, C.byref(last), C.byref(total), C.byref(n), int(bool(reset))),
                  "capdec_bridger_loss")
        return float(last.value), float(total.value), int(n.value)

    def bridger_get(self, kind: int, which: int, batch: Optional[int] = None) -> torch.Tensor:
        """kind 0: parameter ``which`` (2 l = weight of layer l, 2 l + 1 = its bias); kind 1: its momentum buffer; kind 2:
        activation ``which`` of the last train step, [batch, dims[which + 1]] (post-ReLU for hidden layers, L - 1 = the
        output) -- ``batch`` is that step's row count"""
        dims = self._bridger_dims("bridger_get")
        L = len(dims) - 1
        if kind in (0, 1):
            if not 0 <= which < 2 * L:
                raise CapdecError(f"bridger_get: which must be in [0, {2 * L}), got {which}")
            l = which // 2
            shape = (dims[l + 1], dims[l]) if which % 2 == 0 else (dims[l + 1],)
        elif kind == 2:
            if not 0 <= which < L:
                raise CapdecError(f"bridger_get: activation must be in [0, {L}), got {which}")
            shape = (self._bridger_batch("bridger_get", batch), dims[which + 1])
        else:
            raise CapdecError(f"bridger_get: kind must be 0 (parameter), 1 (momentum buffer) or 2 (activation), got {kind!r}")
        out = torch.empty(*shape, device=self.device, dtype=torch.float32)
        self._sync_stream()
        self._chk(self.lib.capdec_bridger_get(self._h, int(kind), int(which), out.data_ptr(), out.numel()), "capdec_bridger_get")
        return out

    # ------------------------------------------------------------------ caption-shard communicator (RCCL through the C ABI)
    def comm_unique_id(self) -> bytes:
        """rank 0: the 128-byte communicator id every rank passes to :meth:`comm_init`"""
        buf = C.create_string_buffer(128)
        self._chk(self.lib.capdec_comm_unique_id(buf), "capdec_comm_unique_id")
        return buf.raw

    def comm_init(self, rank: int, world: int, comm_id: bytes):
        if len(comm_id) != 128:
            raise CapdecError("comm_init: the communicator id is 128 bytes")
        self._chk(self.lib.capdec_comm_init(self._h, int(rank), int(world), comm_id), "capdec_comm_init")
        self.comm = (int(rank), int(world))

    def comm_info(self) -> Tuple[int, int]:
        """(rank, ranks) as RCCL itself reports them for the C-ABI communicator (ncclCommUserRank / ncclCommCount);
        (0, 1) without one"""
        r, n = C.c_int(0), C.c_int(1)
        self._chk(self.lib.capdec_comm_info(self._h, C.byref(r), C.byref(n)), "capdec_comm_info")
        return r.value, n.value

    def comm_destroy(self):
        self._chk(self.lib.capdec_comm_destroy(self._h), "capdec_comm_destroy")
        self.comm = None

    def gather_rows(self, local: torch.Tensor, n_total: int) -> torch.Tensor:
        """all-gather of this rank's row block (int32 or fp32, [n_local, ...]) in rank order -> [n_total, ...]"""
        if local.dtype not in (torch.int32, torch.float32):
            raise CapdecError("gather_rows: int32 or float32 rows")
        t = local.to(self.device).contiguous()
        row = int(np.prod(t.shape[1:])) if t.dim() > 1 else 1
        out = torch.empty((n_total,) + tuple(t.shape[1:]), dtype=t.dtype, device=self.device)
        self._sync_stream()
        self._chk(self.lib.capdec_gather_rows(self._h, t.data_ptr() if t.numel() else None, t.shape[0], max(row, 1),
                                          int(n_total), out.data_ptr() if out.numel() else None), "capdec_gather_rows")
        return out

    # ------------------------------------------------------------------ image preprocessing
    def preprocess_images(self, images, n_px: int = 224, stretch: bool = False,
                          mean=(0.48145466, 0.4578275, 0.40821073), std=(0.26862954, 0.26130258, 0.27577711)) -> torch.Tensor:
        """uint8 RGB images (list of [H, W, 3] numpy arrays / torch tensors, any sizes) -> fp32 [n, 3, n_px, n_px] on the
        device: PIL-exact bicubic Resize(n_px) + CenterCrop(n_px) (or stretch to n_px x n_px) + ToTensor + Normalize
        (reference predictions_runner.py:116-122,212; embeddings_generator.py:72), one HIP launch pair per batch."""
        arrs = []
        for im in images:
            a = im.detach().cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
            if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
                raise CapdecError(f"preprocess_images: expected uint8 [H, W, 3], got {a.dtype} {a.shape}")
            arrs.append(np.ascontiguousarray(a))
        n = len(arrs)
        out = torch.empty(n, 3, n_px, n_px, device=self.device, dtype=torch.float32)
        if n == 0:
            return out
        sizes = np.array([a.size for a in arrs], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        flat = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])).to(self.device)
        hs = np.array([a.shape[0] for a in arrs], dtype=np.int32)
        ws = np.array([a.shape[1] for a in arrs], dtype=np.int32)
        m = np.asarray(mean, dtype=np.float32)
        sd = np.asarray(std, dtype=np.float32)
        self._sync_stream()
        self._chk(self.lib.capdec_preprocess_images(
            self._h, flat.data_ptr(), offs.ctypes.data_as(C.POINTER(C.c_int64)), hs.ctypes.data_as(C.POINTER(C.c_int32)),
            ws.ctypes.data_as(C.POINTER(C.c_int32)), n, int(n_px), int(bool(stretch)), _fp(m), _fp(sd), out.data_ptr()),
            "capdec_preprocess_images")
        return out

    def timer_start(self):
        """hipEvent on the engine's stream (capdec_timer_start): the reference Timer's ``starter.record()``"""
        self._sync_stream()
        self._chk(self.lib.capdec_timer_start(self._h), "timer_start")

    def timer_stop_ms(self) -> float:
        """records the end event, synchronises, returns the elapsed milliseconds (capdec_timer_stop_ms)"""
        ms = C.c_float(0.0)
        self._chk(self.lib.capdec_timer_stop_ms(self._h, C.byref(ms)), "timer_stop_ms")
        return float(ms.value)

    def decode_stats(self) -> Dict[str, int]:
        """steps run / compactions / activation row-steps of the last decode call"""
        a, b, r = C.c_int(0), C.c_int(0), C.c_longlong(0)
        self._chk(self.lib.capdec_decode_stats(self._h, C.byref(a), C.byref(b), C.byref(r)), "decode_stats")
        return dict(steps=a.value, compactions=b.value, row_steps=r.value)

    def set_compact(self, on: bool = True):
        """finished-caption compaction at the decode loop's poll points on / off (capdec_set_compact; default on)"""
        self._chk(self.lib.capdec_set_compact(self._h, int(bool(on))), "set_compact")

    def decode_step_rows(self):
        """activation rows of every decode step (after the prefill) of the last decode call (capdec_decode_step_rows)"""
        buf, n = (C.c_int * 1024)(), C.c_int(0)
        self._chk(self.lib.capdec_decode_step_rows(self._h, buf, 1024, C.byref(n)), "decode_step_rows")
        return [int(buf[i]) for i in range(min(n.value, 1024))]

    def decode_chunks(self) -> int:
        """how many chunks the KV budget split the captions of the last decode call into (capdec_decode_chunks)"""
        n = C.c_int(0)
        self._chk(self.lib.capdec_decode_chunks(self._h, C.byref(n)), "decode_chunks")
        return n.value

    def decode_counters(self) -> Dict[str, float]:
        """kv_slots_per_position: mean number of distinct K/V slots a (caption, position) of the last beam decode read
        (1 = beams share their whole history, beam = nothing); saturated_quads: GEMM-operand quads clamped to the fp16
        range since the last call (the call resets the counter)"""
        kv, sat = C.c_double(0.0), C.c_longlong(0)
        self._chk(self.lib.capdec_decode_counters(self._h, C.byref(kv), C.byref(sat)), "decode_counters")
        return dict(kv_slots_per_position=kv.value, saturated_quads=sat.value)

    # ---- the train step (reference train.py:344-354): scope 0 = --only_prefix, scope 1 = the default run
    @staticmethod
    def train_tensor_names(mapping: str, num_layers: int = 8):
        """the mapper's trainable tensors in the order capdec_train_get indexes them (names as in ``clip_project.state_dict()``)"""
        if mapping == "mlp":
            return ["model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias"]
        if mapping == "transformer_decoder":      # the key order of the reference module's state_dict()
            names = ["prefix_const"]
            for stack, count in (("ref_encoder", num_layers), ("prefix_decoder", 2 * num_layers)):
                for i in range(count):
                    names += [f"{stack}.layers.{i}.{key}" for key in _capi.TMAPPER_LAYER_KEYS]
            return names + ["linear.weight", "linear.bias"]
        names = ["linear.weight", "linear.bias", "prefix_const"]
        for i in range(num_layers):
            names += [f"transformer.layers.{i}.{key}" for key in _capi.TMAPPER_LAYER_KEYS]
        return names

    def train_step(self, prefix: torch.Tensor, tokens: torch.Tensor, lr: float, betas=(0.9, 0.999), eps: float = 1e-6,
                   weight_decay: float = 0.0, apply_update: bool = True, wait: bool = True) -> Optional[float]:
        """one iteration on the device-resident weights (capdec_train_step): ``prefix`` [B, D] AFTER noise injection,
        ``tokens`` [B, L] right-padded with 0; returns the loss of train.py:349.  ``wait=False`` only enqueues the step and
        returns None (``train_loss`` reads the loss, and the running sum, later: no device round trip per step)"""
        self._sync_stream()
        x = prefix.to(self.device, torch.float32).contiguous()
        tok = tokens.to(self.device, torch.int32).contiguous()
        if x.dim() != 2 or tok.dim() != 2 or x.shape[0] != tok.shape[0]:
            raise CapdecError("train_step: prefix [B, D] and tokens [B, L] expected")
        loss = C.c_float(0.0)
        self._chk(self.lib.capdec_train_step(self._h, x.data_ptr(), tok.data_ptr(), tok.shape[0], tok.shape[1], float(lr),
                                             float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                             int(bool(apply_update)), C.byref(loss) if wait else None), "train_step")
        if not wait:
            x.record_stream(torch.cuda.current_stream(self.device))      # (no-ops on the stream they were made on: kept
            tok.record_stream(torch.cuda.current_stream(self.device))    #  for callers that build batches on a side stream)
            return None
        return float(loss.value)

    def train_loss(self, reset: bool = False):
        """(loss of the last step, sum of the losses since the last reset, number of those steps) -- capdec_train_loss"""
        last, total, n = C.c_float(0.0), C.c_double(0.0), C.c_longlong(0)
        self._chk(self.lib.capdec_train_loss(self._h, C.byref(last), C.byref(total), C.byref(n), int(bool(reset))), "train_loss")
        return float(last.value), float(total.value), int(n.value)

    def train_set_dropout(self, p: float, seed: int = 0):
        """GPT-2's dropouts in scope 1 (transformers' default 0.1); keep-masks from the Philox stream keyed by ``seed``"""
        self._chk(self.lib.capdec_train_set_dropout(self._h, float(p), int(seed) & 0xFFFFFFFFFFFFFFFF), "train_set_dropout")

    def train_set_dropout_masks(self, masks: torch.Tensor):
        """keep-masks (uint8, 1 = keep) of the NEXT train step, all sites concatenated in call order (capdec.h)"""
        self._sync_stream()
        m = masks.to(self.device, torch.uint8).contiguous().flatten()
        self._chk(self.lib.capdec_train_set_dropout_masks(self._h, m.data_ptr(), m.numel()), "train_set_dropout_masks")

    def train_get_dropout_masks(self, n: int) -> torch.Tensor:
        """the mask stream the last train step used (uint8 [n])"""
        self._sync_stream()
        out = torch.empty(n, device=self.device, dtype=torch.uint8)
        self._chk(self.lib.capdec_train_get_dropout_masks(self._h, out.data_ptr(), n), "train_get_dropout_masks")
        return out

    @staticmethod
    def dropout_stream_size(B: int, S: int, d: int, n_head: int, n_layer: int) -> int:
        """bytes of one step's mask stream: embd [B, S, d] + per block attn [B, H, S, S], resid [B, S, d], mlp [B, S, d]"""
        return B * S * d + n_layer * (B * n_head * S * S + 2 * B * S * d)

    def _train_get(self, kind: int, shapes) -> Dict[str, torch.Tensor]:
        """``shapes``: ordered {name: shape} in the order of train_tensor_names"""
        out = {}
        for i, name in enumerate(shapes):
            t = torch.empty(shapes[name], device=self.device, dtype=torch.float32)
            self._chk(self.lib.capdec_train_get(self._h, kind, i, t.data_ptr(), t.numel()), "train_get")
            out[name] = t
        return out

    def mapper_parameters(self, shapes) -> Dict[str, torch.Tensor]:
        """the mapper's current tensors on the device (after train steps: the updated values), keyed like MLP.state_dict"""
        return self._train_get(0, shapes)

    def mapper_gradients(self, shapes) -> Dict[str, torch.Tensor]:
        """d loss / d tensor of the last train_step (what loss.backward() leaves in .grad, train.py:350)"""
        return self._train_get(1, shapes)

    @staticmethod
    def train_gpt2_tensor_names(n_layer: int):
        """the GPT-2 tensors that follow the mapper's in capdec_train_get when the scope includes GPT-2 (state-dict names
        without the ``gpt.`` prefix)"""
        names = ["transformer.wte.weight", "transformer.wpe.weight"]
        for i in range(n_layer):
            names += [f"transformer.h.{i}.{n}" for n in (
                "ln_1.weight", "ln_1.bias", "attn.c_attn.weight", "attn.c_attn.bias", "attn.c_proj.weight", "attn.c_proj.bias",
                "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")]
        return names + ["transformer.ln_f.weight", "transformer.ln_f.bias"]

    def train_set_scope(self, train_gpt: bool):
        """False: the mapper only, GPT-2 frozen and in eval mode (--only_prefix); True: GPT-2 as well (the reference's
        default run; dropout per train_set_dropout)"""
        self._chk(self.lib.capdec_train_set_scope(self._h, int(bool(train_gpt))), "train_set_scope")

    def train_set_encdec(self, on: bool):
        """True: the encoder-decoder mapper trains (capdec_train_set_encdec); False, the default: train_step refuses it.  A
        context setting like the scope; without effect on the other two mappers"""
        self._chk(self.lib.capdec_train_set_encdec(self._h, int(bool(on))), "train_set_encdec")

    def train_reset(self):
        """a fresh optimizer: drops the AdamW moments and the step count (scope and dropout setting stay)"""
        self._chk(self.lib.capdec_train_reset(self._h), "train_reset")

    def second_pass_rows(self) -> int:
        """(row, step) pairs of the last decode call whose lm_head top 5 went through the exact second pass (capdec.h)"""
        n = C.c_longlong(0)
        self._chk(self.lib.capdec_decode_second_pass_rows(self._h, C.byref(n)), "decode_second_pass_rows")
        return n.value

    def set_batch_invariant(self, on: bool = True):
        """results independent of batch size / chunking / sharding (no split-K, pinned kernel variants); see capdec.h"""
        self._chk(self.lib.capdec_set_batch_invariant(self._h, int(bool(on))), "set_batch_invariant")

    def set_debug_diverge(self, on: bool = True):
        """measurement builds only (Engine(measure=True)): beams never share history -- the worst-case decode-attention
        traffic; the shipped library does not export the hook"""
        if not hasattr(self.lib, "capdec_set_debug_diverge") or not self.measure:
            raise CapdecError("capdec_set_debug_diverge exists only in the measurement build: Engine(measure=True)")
        self._chk(self.lib.capdec_set_debug_diverge(self._h, int(bool(on))), "set_debug_diverge")

    # ------------------------------------------------------------------ hooks
    def _rows(self, t: torch.Tensor, what: str) -> torch.Tensor:
        """a 2-D fp32 operand on the device as it is when its rows are contiguous (a column slice of a wider tensor keeps
        its row stride: the product call sites pass lda = T * C, ldc = Vp); anything else is copied to a dense tensor"""
        if (t.device == self.device and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and
                t.stride(0) >= t.shape[1]):
            return t
        if what == "out":
            raise CapdecError("gemm: out= must be a 2-D fp32 tensor on the engine's device with contiguous rows")
        return self._dev(t)

    def gemm(self, a: torch.Tensor, bt: torch.Tensor, bias=None, resid=None, act: int = 0, out=None) -> torch.Tensor:
        """out = act(a . bt^T + bias) + resid.  ``a`` [M, K] and ``resid`` [M, N] may be row-strided views (their real row
        strides are passed as lda / ldr); ``out=`` is an [M, N] view with row stride ldc >= N, written in place and
        returned; ``resid is out`` accumulates onto the output as the block stack does (h += ...)."""
        a, bt = self._rows(a, "a"), self._dev(bt)
        if a.stride(0) % 4 or a.data_ptr() % 16:      # (the kernels read 16-byte pieces of a row)
            a = a.clone(memory_format=torch.contiguous_format)
        M, K = a.shape
        N = bt.shape[0]
        if bt.shape[1] != K:
            raise CapdecError(f"gemm: a is [{M}, {K}] but bt is {list(bt.shape)}")
        if out is None:
            out = torch.empty(M, N, device=self.device, dtype=torch.float32)
        else:
            out = self._rows(out, "out")
            if tuple(out.shape) != (M, N):
                raise CapdecError(f"gemm: out= must be [{M}, {N}], got {list(out.shape)}")
        b = self._dev(bias) if bias is not None else None
        r = None
        if resid is not None:
            r = out if resid is out else self._rows(resid, "resid")
            if tuple(r.shape) != (M, N):
                raise CapdecError(f"gemm: resid must be [{M}, {N}], got {list(r.shape)}")
        self._sync_stream()
        self._chk(self.lib.capdec_gemm_f32(self._h, a.data_ptr(), a.stride(0), bt.data_ptr(), K, out.data_ptr(), out.stride(0),
                                       M, N, K, b.data_ptr() if b is not None else None,
                                       r.data_ptr() if r is not None else None, r.stride(0) if r is not None else N, act),
                  "capdec_gemm_f32")
        return out

    def gemm_tn(self, xa: torch.Tensor, xb: torch.Tensor, out=None) -> torch.Tensor:
        """out [N1, N2] = xa^T . xb for xa [rows, N1], xb [rows, N2]: the weight-gradient product of the train step
        (dW = dY^T X) through the launch the train step uses.  Both operands and ``out=`` may be row-strided views (their
        real row strides are passed as lda / ldb / ldc)."""
        xa, xb = self._rows(xa, "xa"), self._rows(xb, "xb")
        rows, N1 = xa.shape
        N2 = xb.shape[1]
        if xb.shape[0] != rows:
            raise CapdecError(f"gemm_tn: xa is [{rows}, {N1}] but xb is {list(xb.shape)}")
        if out is None:
            out = torch.empty(N1, N2, device=self.device, dtype=torch.float32)
        else:
            out = self._rows(out, "out")
            if tuple(out.shape) != (N1, N2):
                raise CapdecError(f"gemm_tn: out= must be [{N1}, {N2}], got {list(out.shape)}")
        self._sync_stream()
        self._chk(self.lib.capdec_gemm_tn_f32(self._h, xa.data_ptr(), xa.stride(0), xb.data_ptr(), xb.stride(0), rows, N1, N2,
                                              out.data_ptr(), out.stride(0)), "capdec_gemm_tn_f32")
        return out

    def set_gemm_mode(self, mode: str):
        """'f16x2' (default: fp32-accurate, operands as two fp16 planes, 3 MFMAs per product), 'bf16x3' (fp32-accurate,
        three bf16 planes, 6 MFMAs per product), 'f32' (native fp32 MFMA), 'bf16' (bf16 GEMM operands and KV cache, fp32
        accumulate: BASELINE configs[1]) or 'f16' (fp16 GEMM operands: the reference's CLIP-tower arithmetic on a GPU)"""
        self._chk(self.lib.capdec_set_gemm_mode(self._h, {"f32": 0, "bf16x3": 1, "bf16": 2, "f16x2": 3, "f16": 4}[mode]), "set_gemm_mode")

    def gemm_mode(self) -> str:
        return ["f32", "bf16x3", "bf16", "f16x2", "f16"][self.lib.capdec_get_gemm_mode(self._h)]

    def profile_enable(self, on=True):
        """True / 1: time every launch; N > 1: every N-th launch of each kernel family (sampling); False: off"""
        self._chk(self.lib.capdec_profile_enable(self._h, int(on)), "profile_enable")

    def profile_reset(self):
        self._chk(self.lib.capdec_profile_reset(self._h), "profile_reset")

    def profile_get(self) -> Dict[str, Dict[str, float]]:
        cnt = C.c_int(24)                 # in: capacity of the arrays below, out: families filled
        names = (C.c_char_p * 24)()
        ms = (C.c_float * 24)()
        launches = (C.c_int64 * 24)()
        flops = (C.c_double * 24)()
        calls = (C.c_int64 * 24)()
        self._chk(self.lib.capdec_profile_get(self._h, C.byref(cnt), names, ms, launches, flops, calls), "profile_get")
        return {names[i].decode(): dict(ms=float(ms[i]), launches=int(launches[i]), flops=float(flops[i]),
                                        calls=int(calls[i]))
                for i in range(cnt.value)}


_engines: Dict[int, Engine] = {}


def get_engine(device: int = 0) -> Engine:
    """process-wide engine per device index"""
    if device not in _engines:
        _engines[device] = Engine(device)
    return _engines[device]
