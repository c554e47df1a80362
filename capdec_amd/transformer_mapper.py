"""Drop-in surface of reference ``transformer_mapper.py``: ``TransformerMapper`` (:113-127) and
``TransformerEncoderDecoder`` (:130-145, MappingType.TransformerDecoder; trained once ``requires_grad_()`` asks for it).
The layer stack (Mlp :4-19, MultiHeadAttention :22-51, TransformerLayer :54-73, Transformer
:76-110) runs as HIP kernels inside ``capdec_mapper_forward``."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Optional

import torch

from ._capi import TMAPPER_LAYER_KEYS
from .engine import Engine
from .gpt2_prefix import _HipModule


class _TransformerMapperBase(_HipModule):
    """what the two classes share; a subclass names its state-dict keys (``_keys``), the width of ``linear``'s output rows
    (``_linear_width``) and the engine loader (``_LOADER``)"""

    def __init__(self, dim_clip: int, dim_embedding: int, prefix_length: int, clip_length: int, num_layers: int,
                 _owner: Optional[_HipModule] = None):
        super().__init__()
        self.dim_clip, self.dim_embedding = dim_clip, dim_embedding
        self.prefix_length, self.clip_length, self.num_layers = prefix_length, clip_length, num_layers
        self._owner = _owner

    def _layer_keys(self, stack: str, count: int):
        return [f"{stack}.layers.{i}.{key}" for i in range(count) for key in TMAPPER_LAYER_KEYS]

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        need = self._keys()
        missing = [k for k in need if k not in sd]
        if missing and strict:
            raise RuntimeError(f"Missing key(s) in state_dict: {missing}")
        for k in need:
            if k in sd:
                self._sd[k] = sd[k].detach().float().cpu()
        if tuple(self._sd["prefix_const"].shape) != (self.prefix_length, self.dim_embedding):
            raise RuntimeError("size mismatch for prefix_const")
        if tuple(self._sd["linear.weight"].shape) != (self.clip_length * self._linear_width(), self.dim_clip):
            raise RuntimeError("size mismatch for linear.weight")
        self._dirty = True
        return SimpleNamespace(missing_keys=missing, unexpected_keys=[k for k in sd if k not in need])

    def _upload(self, eng: Engine):
        getattr(eng, self._LOADER)({"clip_project." + k: v for k, v in self._sd.items()})

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        eng = self._owner.engine if self._owner is not None else self.engine
        return eng.mapper_forward(x)   # [B, P, dim_embedding]


class TransformerMapper(_TransformerMapperBase):
    _LOADER = "load_mapper_transformer"

    def __init__(self, dim_clip: int, dim_embedding: int, prefix_length: int, clip_length: int, num_layers: int = 8,
                 _owner: Optional[_HipModule] = None):
        super().__init__(dim_clip, dim_embedding, prefix_length, clip_length, num_layers, _owner)

    def _keys(self):
        return ["linear.weight", "linear.bias", "prefix_const"] + self._layer_keys("transformer", self.num_layers)

    def _linear_width(self):
        return self.dim_embedding


class TransformerEncoderDecoder(_TransformerMapperBase):
    """reference transformer_mapper.py:130-145: ``num_layers`` encoder layers at width 512 over ``linear(x)`` viewed as
    [clip_length, 512], then ``2 * num_layers`` decoder layers at width ``dim_embedding`` that carry ``prefix_const``,
    alternately attending to the encoder's output and to their own residual stream."""

    ENC_DIM = 512       # hard-coded in the reference (:142-144), whatever dim_clip and dim_embedding are
    _LOADER = "load_mapper_encdec"

    def __init__(self, dim_clip: int, dim_embedding: int, prefix_length: int, clip_length: int, num_layers: int = 4,
                 _owner: Optional[_HipModule] = None):
        super().__init__(dim_clip, dim_embedding, prefix_length, clip_length, num_layers, _owner)
        self._requires_grad = False

    def requires_grad_(self, flag: bool = True):
        """torch's own name: ask for (or give up) the training of this mapper.  Off by default -- a model that was merely
        built and loaded is refused by ``train.train_step``; ``gpt2_prefix.train`` turns it on itself"""
        if not flag and self._requires_grad and self._owner is not None:
            self._owner._pull_mapper()          # weights that only the device holds are read back while the switch is on
        self._requires_grad = bool(flag)
        if self._owner is not None and self._owner._engine is not None:
            self._owner._engine.train_set_encdec(self._requires_grad)
        return self

    def _keys(self):
        """the reference class's ``state_dict()`` keys, in its order"""
        return (["prefix_const"] + self._layer_keys("ref_encoder", self.num_layers)
                + self._layer_keys("prefix_decoder", 2 * self.num_layers) + ["linear.weight", "linear.bias"])

    def _linear_width(self):
        return self.ENC_DIM
