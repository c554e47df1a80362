"""Which candidate caption fits the image: CLIPScore / RefCLIPScore (Hessel et al., EMNLP 2021) and reranking by CLIP
similarity.  The decoders return several captions per image -- the beams, diverse-beam groups, constrained beams,
``entry_count`` samples -- ordered by the language model alone; a CapDec decoder is trained on text, so its most probable
beam is often the most generic one.  Here the candidates go through the CLIP text tower (``ClipModel.encode_text``) and are
compared with the image embedding the prefix was made from, in ``Engine.clip_score`` (capdec_clip_score: one block per
image; cosines, scores and the order come back, the similarity block never exists in memory).  Not in the reference, which
leaves the metric to outside tools; the contract is include/capdec.h.

``clip_score``        the four values per candidate, the order per image and the paper's two corpus numbers
``rerank_by_clip``    what ``generate_*_batch`` returned, every image's list best first
``score_predictions`` the corpus numbers of a predictions list as ``make_preds`` writes it
(``predictions_runner.make_preds(..., clip_rerank=clip_model)`` writes the CLIP-best beam instead of the LM-best one.)"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from ._capi import CapdecError

COLUMNS = ("cos", "clip_s", "ref_sim", "refclip_s")


def _default_tokenize(texts):
    from .clip import tokenize
    return tokenize(texts, truncate=True)       # an over-long caption is scored on its first 77 tokens, not raised on


def _lists(what: str, texts, n: int):
    """``texts`` as one list of strings per image -> (lists, flat: it was one string per image)"""
    texts = list(texts)
    if len(texts) != n:
        raise CapdecError(f"{what}: {len(texts)} entries for {n} images")
    flat = n > 0 and all(isinstance(t, str) for t in texts)
    if not flat and any(isinstance(t, str) for t in texts):
        raise CapdecError(f"{what}: either one string per image or one list of strings per image")
    return ([[t] for t in texts] if flat else [list(t) for t in texts]), flat


def _offsets(lists) -> np.ndarray:
    return np.concatenate([[0], np.cumsum([len(t) for t in lists], dtype=np.int64)]).astype(np.int64)


def _encode(clip_model, lists, tokenize, text_batch: int, d: int, device) -> torch.Tensor:
    texts = [t for ts in lists for t in ts]
    step = max(1, int(text_batch))
    feats = [clip_model.encode_text(tokenize(texts[b0:b0 + step])).float() for b0 in range(0, len(texts), step)]
    return torch.cat(feats) if feats else torch.zeros(0, d, dtype=torch.float32, device=device)


def clip_score(clip_model, image_features: torch.Tensor, candidates, references=None, *, tokenize=None, w: float = 2.5,
               text_batch: int = 2048) -> Dict:
    """``image_features`` [N, d] (``clip_model.encode_image``, raw); ``candidates``: one string per image, or one list of
    strings per image (0 to 64, ragged allowed); ``references``: one list of strings per image, or None.  The texts go
    through ``tokenize`` (default ``capdec_amd.clip.tokenize`` with truncation; any ``list[str] -> int [N, 77]``) in batches
    of ``text_batch``, then ``clip_model.encode_text``, then ``Engine.clip_score``.  -> a dict of host values:
    ``cos``, ``clip_s`` (= w max(cos, 0)), ``ref_sim``, ``refclip_s`` fp32, shaped like ``candidates`` (an array [N], or a list
    of N arrays; the last two NaN for an image without references); ``order``: per image the indices of its candidates, best
    first; ``CLIPScore`` / ``RefCLIPScore``: the fp64 means of ``clip_s`` / ``refclip_s`` over every image's FIRST listed
    candidate -- the paper's corpus numbers (NaN when a value they average is NaN; an image without candidates is left
    out)."""
    if image_features.dim() != 2:
        raise CapdecError("clip_score: image_features must be [N, d]")
    if tokenize is None:
        tokenize = _default_tokenize
    n, d = int(image_features.shape[0]), int(image_features.shape[1])
    eng = clip_model._engine
    cands, flat = _lists("clip_score: candidates", candidates, n)
    off = _offsets(cands)
    cand = _encode(clip_model, cands, tokenize, text_batch, d, eng.device)
    ref = roff = None
    if references is not None:
        refs, was_flat = _lists("clip_score: references", references, n)
        if was_flat:
            raise CapdecError("clip_score: references is one LIST of strings per image")
        roff = _offsets(refs)
        ref = _encode(clip_model, refs, tokenize, text_batch, d, eng.device)
    scores, order = eng.clip_score(cand, image_features, off, ref, roff, w)
    scores, order = scores.cpu().numpy(), order.cpu().numpy()
    out: Dict = {}
    for k, name in enumerate(COLUMNS):
        out[name] = scores[:, k].copy() if flat else [scores[off[g]:off[g + 1], k].copy() for g in range(n)]
    out["order"] = [(order[off[g]:off[g + 1]] - off[g]).astype(np.int64) for g in range(n)]
    first = off[:-1][off[1:] > off[:-1]]
    for name, col in (("CLIPScore", 1), ("RefCLIPScore", 3)):
        vals = scores[first, col].astype(np.float64)
        out[name] = float(vals.mean()) if len(vals) and (col == 1 or references is not None) else float("nan")
    return out


def rerank_by_clip(clip_model, image_features: torch.Tensor, texts, *, tokenize=None, return_scores: bool = False):
    """``texts``: one list of candidate strings per image -- exactly what ``generate_beam_batch``,
    ``generate_diverse_beam_batch``, ``generate_constrained_beam_batch`` and ``generate_samples_batch`` return -- and
    ``image_features`` [N, d] the CLIP image embeddings they were decoded from.  -> ``texts`` with every image's list
    reordered by descending cosine to its image (equal cosines keep their order); with ``return_scores`` also the cosines,
    one fp32 array per image in the new order."""
    lists, flat = _lists("rerank_by_clip: texts", texts, int(image_features.shape[0]))
    if flat:
        raise CapdecError("rerank_by_clip: texts is one LIST of candidate strings per image")
    res = clip_score(clip_model, image_features, lists, tokenize=tokenize)
    ranked = [[ts[int(i)] for i in o] for ts, o in zip(lists, res["order"])]
    if not return_scores:
        return ranked
    return ranked, [c[o] for c, o in zip(res["cos"], res["order"])]


def score_predictions(preds: Sequence[Dict], image_features: torch.Tensor, clip_model, references: Optional[Dict] = None, *,
                      tokenize=None, w: float = 2.5) -> Dict:
    """``preds``: the list ``make_preds`` writes, ``[{"caption", "image_id"}]``; ``image_features`` [N, d] in the same order;
    ``references``: ``image_id -> list[str]``, or None.  -> ``CLIPScore``, ``RefCLIPScore`` (fp64 means over the images) and the
    per-image ``cos``, ``clip_s``, ``ref_sim``, ``refclip_s`` (fp32 [N]) with their ``image_id`` list."""
    preds = list(preds)
    refs = None
    if references is not None:
        missing = [p["image_id"] for p in preds if p["image_id"] not in references]
        if missing:
            raise CapdecError(f"score_predictions: no references for image_id {missing[0]!r} ({len(missing)} missing)")
        refs = [list(references[p["image_id"]]) for p in preds]
    res = clip_score(clip_model, image_features, [p["caption"] for p in preds], refs, tokenize=tokenize, w=w)
    out = {k: res[k] for k in ("CLIPScore", "RefCLIPScore") + COLUMNS}
    out["image_id"] = [p["image_id"] for p in preds]
    return out
