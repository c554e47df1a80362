"""Projection of image embeddings onto a support memory of text embeddings: the training-free way across the modality gap
(DeCap, Li et al., ICLR 2023; not in the reference).  The memory is the ``clip_embedding_text_dave`` tensor that
``embeddings_generator.py`` writes and ``train()`` reads -- the text embeddings the decoder was trained on -- and an image
embedding is replaced by the softmax-weighted combination of its rows (``Engine.memory_project``, capdec_memory_project: one
fused HIP pass, the similarity matrix never in HBM).  ``predictions_runner``'s ``support_memory=`` takes a
:class:`SupportMemory`."""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from . import formats
from ._capi import CapdecError
from .engine import Engine, get_engine


class SupportMemory:
    """``text_embeddings`` [M, d] (normalised or not: the engine normalises every row), optionally the M caption strings
    (or the reference's caption dicts, whose ``"caption"`` is taken).  The device copy lives in an Engine's memory slot (one
    per context): the object loads itself there on first use and again whenever the engine holds another memory."""

    def __init__(self, text_embeddings: torch.Tensor, captions: Optional[Sequence] = None, engine: Optional[Engine] = None):
        if text_embeddings.dim() != 2 or text_embeddings.shape[0] < 1:
            raise CapdecError(f"SupportMemory: text_embeddings must be [M, d] with M >= 1, got {tuple(text_embeddings.shape)}")
        self.text_embeddings = text_embeddings
        self.captions: Optional[List[str]] = None
        if captions is not None:
            caps = [c["caption"] if isinstance(c, dict) else c for c in captions]
            if len(caps) != int(text_embeddings.shape[0]):
                raise CapdecError(f"SupportMemory: {len(caps)} captions for {int(text_embeddings.shape[0])} embeddings")
            self.captions = caps
        self._engine = engine

    @classmethod
    def from_pickle(cls, path: str, engine: Optional[Engine] = None) -> "SupportMemory":
        """the text side and the caption strings of the reference's embeddings pickle (``formats.load_embeddings_pickle``)"""
        _, txt, caps = formats.load_embeddings_pickle(path)
        if txt.shape[0] < 1:
            raise CapdecError(f"SupportMemory.from_pickle: {path} holds no text embeddings (clip_embedding_text_dave)")
        return cls(txt, caps if len(caps) == int(txt.shape[0]) else None, engine=engine)

    def __len__(self) -> int:
        return int(self.text_embeddings.shape[0])

    @property
    def dim(self) -> int:
        return int(self.text_embeddings.shape[1])

    @property
    def engine(self) -> Engine:
        if self._engine is None:
            self._engine = get_engine()
        if getattr(self._engine, "_memory_owner", None) is not self:
            self._engine.memory_load(self.text_embeddings)
            self._engine._memory_owner = self
        return self._engine

    def project(self, x: torch.Tensor, temperature: float = 0.01, return_info: bool = False):
        """``x`` [..., d] -> its projection, unit rows fp32 [..., d] on the device; with ``return_info`` also the dict of
        ``Engine.memory_project`` (``lse``, ``nearest``, ``max_sim``)"""
        if x.dim() < 1 or int(x.shape[-1]) != self.dim:
            raise CapdecError(f"SupportMemory: the input must be [..., {self.dim}], got {tuple(x.shape)}")
        return self.engine.memory_project(x, temperature=temperature, return_info=return_info)

    __call__ = project

    def nearest(self, x: torch.Tensor) -> torch.Tensor:
        """index of the memory row most similar to every row of ``x`` (int32 [...]; -1 for a row holding a NaN or an inf)"""
        return self.project(x, return_info=True)[1]["nearest"]

    def nearest_captions(self, x: torch.Tensor) -> List[Optional[str]]:
        """the caption of that row for every row of ``x`` (flattened): the retrieval baseline"""
        if self.captions is None:
            raise CapdecError("SupportMemory.nearest_captions: the memory was built without captions")
        return [self.captions[i] if i >= 0 else None for i in self.nearest(x).reshape(-1).tolist()]
