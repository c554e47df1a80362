"""Batched counterpart of the per-image loop of reference ``predictions_runner.make_preds``
(:194-234,300-301): embeddings -> normalise (+ modality offset) -> ``clip_project`` ->
``generate_beam`` / ``generate2`` -> ``{"caption": text.lower(), "image_id": ...}``.
``generate_beam`` / ``generate2`` are re-exported here because the reference imports them
into this module (:13) and BASELINE.json's north_star names them under it.

The distance ablations of the reference (``--ablation_dist``: :18-95 and :235-251; ``--ablation_image_dist``: :240-247) are here
too, under its names: ``count_ready_parphrased_embeddings``, ``calc_distances_of_ready_embeddings``, and their batched forms
``paraphrase_distances``, ``paraphrase_distance_ablation``, ``image_text_distance`` and ``estimate_noise_variance``.  The
pair loops run in ``Engine.group_distances`` (capdec_group_distances: one block per image); host numpy only sees the
[groups, 8] result."""
from __future__ import annotations

import json
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import distributed as cdist
from ._capi import CapdecError
from .engine import Engine, get_engine
from .gpt2_prefix import ClipCaptionModel, MappingType  # noqa: F401
from .gpt2_prefix_eval import (_phrases_of, decode_beam_ids, decode_constrained_beam_ids, decode_greedy_ids,  # noqa: F401
                               generate2, generate2_batch, generate_beam, generate_beam_batch)


class Timer:
    """reference predictions_runner.py:125-150 (``with timer: ...`` around the work of one image, ``print(timer)`` every 99
    images, :214,:233,:253): here the events are the C ABI's hipEvent pair on the engine's stream (capdec_timer_start /
    capdec_timer_stop_ms) and one interval covers one BATCH; ``per_item`` divides by the batch size so that the printed
    mean / std stay "ms per image" like the reference's."""

    def __init__(self, model: Optional[ClipCaptionModel] = None):
        self.sum = 0.0
        self.count = 0
        self.timings: List[float] = []
        self.items = 0
        self._model = model

    def bind(self, model: ClipCaptionModel):
        self._model = model
        return self

    def __enter__(self):
        self._model.engine.timer_start()
        return self

    def __exit__(self, *args):
        interval = self._model.engine.timer_stop_ms()
        self.timings.append(interval)
        self.sum += interval
        self.count += 1

    def add_items(self, n: int):
        self.items += int(n)

    def __str__(self):
        import numpy as np
        if self.count == 0:
            return "mean: nan ms, std: nan ms"
        s = f"mean: {self.sum / self.count:.2f} ms, std: {float(np.std(self.timings)):.2f} ms"
        if self.items:
            s += f" per batch; {self.sum / self.items:.4f} ms per image over {self.items} images"
        return s


def _given(**kw) -> Dict:
    """the logits-processor keywords a caller did give (None = not given: ``model.logits_processors`` decides)"""
    return {k: v for k, v in kw.items() if v is not None}


def _memory_kw(support_memory, projection_temperature) -> Dict:
    """the projection keywords, only when a support memory was given: without one every call runs what it always ran"""
    return {} if support_memory is None else {"support_memory": support_memory, "projection_temperature": projection_temperature}


def prefix_from_embeddings(model: ClipCaptionModel, embeddings: torch.Tensor, dont_normalize_prefix: bool = False,
                           modality_offset: Optional[torch.Tensor] = None, *, modality_bridger=None, support_memory=None,
                           projection_temperature: float = 0.01) -> torch.Tensor:
    """reference :221-228 for a batch: ``prefix / prefix.norm(2,-1)``; ``+ offset``; with ``modality_bridger`` (the callable
    of ``supervised_embedding_bridger.get_map_to_text_space_using_modality_bridger`` or its ``MLP``; --modality_bridger)
    ``prefix = modality_bridger(prefix)``, NOT normalised again (:227 computes the quotient and drops it);
    ``clip_project(prefix).reshape(N, P, -1)``.  With ``support_memory`` (a ``support_memory.SupportMemory``; not in the
    reference) the prefix is instead replaced, at the same place, by its projection onto the memory of text embeddings at
    ``projection_temperature`` -- a unit vector, which goes to ``clip_project`` as it is.  Both at once is an error."""
    if support_memory is not None and modality_bridger is not None:
        raise CapdecError("prefix_from_embeddings: support_memory and modality_bridger are two ways across the same gap: "
                          "pass one of them")
    eng = model.engine
    x = eng.normalize_prefix(embeddings, normalize=not dont_normalize_prefix, offset=modality_offset)
    if modality_bridger is not None:
        x = modality_bridger(x)
    if support_memory is not None:
        x = support_memory.project(x, temperature=projection_temperature)
    return model.clip_project(x).reshape(x.shape[0], model.prefix_length, -1)


def caption_ids(model: ClipCaptionModel, embeddings: torch.Tensor, stop_token_index: int, beam: bool = True,
                beam_size: int = 5, entry_length: int = 67, dont_normalize_prefix: bool = False,
                modality_offset: Optional[torch.Tensor] = None, rank: int = 0, world: int = 1, *,
                repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                min_length: Optional[int] = None, logit_bias=None, modality_bridger=None, phrases=None, support_memory=None,
                projection_temperature: float = 0.01, pick=None):
    """The whole device-side path for this rank's shard of ``embeddings`` [N, D].
    Returns (ids [n_local, T] int32 of the best caption, lens [n_local]) and, for beam, the
    mean-log-prob score of the best beam.  The keyword-only logits processors (None: ``model.logits_processors``'s) are
    those of ``decode_beam_ids`` / ``decode_greedy_ids``.  ``phrases`` (int32 [N, 4, 4], beam only; None: the plain beam):
    the phrases every caption must contain (``decode_constrained_beam_ids``).  ``support_memory``,
    ``projection_temperature``: see ``prefix_from_embeddings``.  ``pick`` (beam only; None: beam 0, the best under the language
    model): a callable ``(ids [n_local, beam, T], lens [n_local, beam], lo, hi) -> int64 [n_local]``, the beam to return for
    every caption of the shard ``embeddings[lo:hi]`` (``make_preds``'s ``clip_rerank``)."""
    pk = _given(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, logit_bias=logit_bias)
    lo, hi = cdist.shard_bounds(embeddings.shape[0], rank, world)
    pe = prefix_from_embeddings(model, embeddings[lo:hi], dont_normalize_prefix, modality_offset,
                                **_given(modality_bridger=modality_bridger), **_memory_kw(support_memory, projection_temperature))
    if pick is not None and not beam:
        raise CapdecError("caption_ids: picking among the beams needs the beam decode (beam=True)")

    def best(ids, lens, scores):
        if pick is None:
            return ids[:, 0].contiguous(), lens[:, 0].contiguous(), scores[:, 0].contiguous()
        b = pick(ids, lens, lo, hi).to(ids.device)
        r = torch.arange(ids.shape[0], device=ids.device)
        return ids[r, b].contiguous(), lens[r, b].contiguous(), scores[r, b].contiguous()

    if phrases is not None:
        if not beam:
            raise CapdecError("caption_ids: forced words need the beam decode (beam=True)")
        ids, lens, scores = decode_constrained_beam_ids(model, pe, np.asarray(phrases)[lo:hi], stop_token_index, beam_size,
                                                        entry_length, **pk)[:3]
        return best(ids, lens, scores)
    if beam:
        ids, lens, scores, _ = decode_beam_ids(model, pe, stop_token_index, beam_size, entry_length, **pk)
        return best(ids, lens, scores)
    ids, lens = decode_greedy_ids(model, pe, stop_token_index, entry_length, **pk)
    return ids, lens, None


def _clip_pick(clip_model, clip_tokenize, tokenizer, embeddings: torch.Tensor):
    """``caption_ids``'s ``pick``: the beam whose text, as ``make_preds`` would write it, has the largest CLIP cosine to the
    caption's own embedding -- the tensor its prefix was made from"""
    from .clip_score import clip_score

    def pick(ids, lens, lo, hi):
        ids_h, lens_h = ids.cpu().numpy(), lens.cpu().numpy()
        texts = [[tokenizer.decode(list(ids_h[r, b, :int(lens_h[r, b])])).lower() for b in range(ids_h.shape[1])]
                 for r in range(ids_h.shape[0])]
        order = clip_score(clip_model, embeddings[lo:hi], texts, tokenize=clip_tokenize)["order"]
        return torch.tensor([int(o[0]) for o in order], dtype=torch.int64)

    return pick


def make_preds(data: Sequence[Dict], embeddings: torch.Tensor, model: ClipCaptionModel, tokenizer,
               out_path: Optional[str] = None, beam: bool = True, entry_length: int = 67,
               dont_normalize_prefix: bool = False, modality_offset: Optional[torch.Tensor] = None,
               rank: int = 0, world: int = 1, timer: Optional[Timer] = None, *,
               repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
               min_length: Optional[int] = None, logit_bias=None, modality_bridger=None, force_words=None,
               support_memory=None, projection_temperature: float = 0.01, clip_rerank=None, clip_tokenize=None) -> List[Dict]:
    """``data[i]`` = {"image_id": ...}; ``embeddings[i]`` its CLIP embedding.  ``modality_bridger`` (--modality_bridger),
    ``support_memory`` and ``projection_temperature``: see ``prefix_from_embeddings``.  ``force_words`` (beam only; None: the plain beam): per caption a list of up to 4 words its
    caption must contain (``generate_constrained_beam_batch``).  ``clip_rerank`` (beam only; None: the beam the language model
    scores best, as ever): a ``ClipModel`` with a text tower -- all five beams of this rank's captions (with the forced words,
    when given) go through its text tower (``clip_tokenize``: ``list[str] -> int [N, 77]``, default ``clip.tokenize`` with
    truncation) and the beam closest to ``embeddings[i]`` is written (``capdec_amd.clip_score``).  Writes the
    reference's predictions JSON (``[{"caption": lower-cased text, "image_id": id}]``, :260-261,
    :301) -- the whole list, not only every 99th flush."""
    pk = _given(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, logit_bias=logit_bias,
                modality_bridger=modality_bridger)
    pk.update(_memory_kw(support_memory, projection_temperature))
    cdist.check_world(rank, world)
    if len(data) != embeddings.shape[0]:
        raise ValueError(f"make_preds: {len(data)} data entries but {embeddings.shape[0]} embeddings")
    stop = tokenizer.encode('.')[0]
    if force_words is not None:
        pk["phrases"] = _phrases_of(tokenizer, len(data), force_words, None)
    if clip_rerank is not None:
        if not beam:
            raise CapdecError("make_preds: clip_rerank needs the beam decode (beam=True): one candidate is nothing to rerank")
        pk["pick"] = _clip_pick(clip_rerank, clip_tokenize, tokenizer, embeddings)
    if timer is not None:           # the reference's `with timer:` (:214-233) around this rank's share of the batch
        with timer.bind(model):
            ids, lens, _ = caption_ids(model, embeddings, stop, beam, 5, entry_length, dont_normalize_prefix,
                                       modality_offset, rank, world, **pk)
        lo, hi = cdist.shard_bounds(embeddings.shape[0], rank, world)
        timer.add_items(hi - lo)
        print(timer)                # (:253)
    else:
        ids, lens, _ = caption_ids(model, embeddings, stop, beam, 5, entry_length, dont_normalize_prefix,
                                   modality_offset, rank, world, **pk)
    ids, lens, _ = cdist.gather_ids(ids, lens, embeddings.shape[0])
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    new_data = [{"caption": tokenizer.decode(list(ids[i, :int(lens[i])])).lower(), "image_id": d["image_id"]}
                for i, d in enumerate(data)]
    if out_path and rank == 0:
        with open(out_path, 'w') as outfile:
            json.dump(new_data, outfile)
    return new_data


def make_preds_from_images(data: Sequence[Dict], images: Sequence, clip_model, preprocess, model: ClipCaptionModel,
                           tokenizer, out_path: Optional[str] = None, beam: bool = True, is_rn: bool = False,
                           entry_length: int = 67, dont_normalize_prefix: bool = False,
                           modality_offset: Optional[torch.Tensor] = None, rank: int = 0, world: int = 1,
                           image_batch: int = 256, *, repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                           min_length: Optional[int] = None, logit_bias=None, modality_bridger=None, support_memory=None,
                           projection_temperature: float = 0.01) -> List[Dict]:
    """The image half of the reference loop in front of ``make_preds`` (:156-161, :207-220): ``images[i]`` is what
    ``Image.open(filename).convert("RGB")`` gave for ``data[i]`` (a PIL image or a uint8 [H, W, 3] array), or ``None``
    for a file the reference would skip (:207-210: the entry is left out of the output).  ``preprocess`` and
    ``clip_model.encode_image`` (``capdec_amd.clip.load``) run on the device in batches of ``image_batch``;
    ``is_rn`` (the RN50x4 backbone) forces ``beam=True`` exactly as the reference does (:157-159)."""
    if len(data) != len(images):
        raise ValueError(f"make_preds_from_images: {len(data)} data entries but {len(images)} images")
    if is_rn:
        beam = True
    keep = [i for i, im in enumerate(images) if im is not None]
    if not keep:                       # nothing to caption: the reference writes an empty list
        if out_path and rank == 0:
            with open(out_path, 'w') as outfile:
                json.dump([], outfile)
        return []
    # the image tower is the expensive half of this path (RN50x4: ~10x a caption's decode), so it is sharded like the
    # decode: rank r preprocesses / encodes / decodes only ITS block of the kept images; the ids are gathered at the end
    cdist.check_world(rank, world)
    lo, hi = cdist.shard_bounds(len(keep), rank, world)
    mine = keep[lo:hi]
    feats = []
    for b0 in range(0, len(mine), max(1, image_batch)):
        batch = [images[i] for i in mine[b0:b0 + max(1, image_batch)]]
        feats.append(clip_model.encode_image(preprocess.batch(batch)).float())
    stop = tokenizer.encode('.')[0]
    T = entry_length
    if feats:
        ids, lens, _ = caption_ids(model, torch.cat(feats), stop, beam, 5, T, dont_normalize_prefix, modality_offset,
                                   **_given(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, logit_bias=logit_bias,
                                            modality_bridger=modality_bridger),
                                   **_memory_kw(support_memory, projection_temperature))
    else:                              # an empty shard (more ranks than images) still takes part in the gather
        dev = next(model.parameters()).device
        ids, lens = torch.zeros(0, T, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    ids, lens, _ = cdist.gather_ids(ids, lens, len(keep))
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    new_data = [{"caption": tokenizer.decode(list(ids[j, :int(lens[j])])).lower(), "image_id": data[i]["image_id"]}
                for j, i in enumerate(keep)]
    if out_path and rank == 0:
        with open(out_path, 'w') as outfile:
            json.dump(new_data, outfile)
    return new_data


def make_preds_from_captions(data: Sequence[Dict], clip_model, model: ClipCaptionModel, tokenizer, tokenize=None,
                             out_path: Optional[str] = None, beam: bool = True, entry_length: int = 67,
                             dont_normalize_prefix: bool = False, modality_offset: Optional[torch.Tensor] = None,
                             rank: int = 0, world: int = 1, text_batch: int = 2048, *,
                             repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                             min_length: Optional[int] = None, logit_bias=None) -> List[Dict]:
    """The TEXT-input branch of the reference loop (:215-218: ``args.text_autoencoder`` or ``dataset_mode == 5`` -- "the
    image is actually text input"): ``caption_tokens = clip.tokenize(d['caption'])``; ``prefix =
    clip_model.encode_text(caption_tokens).float()``; then the common tail (:221-234) -- normalise, modality offset,
    ``clip_project``, ``generate_beam`` / ``generate2`` -- and the predictions JSON of :260-261.  ``tokenize`` defaults to
    ``capdec_amd.clip.tokenize`` (needs the CLIP BPE vocabulary file); any callable ``list[str] -> int [N, 77]`` does.
    This rank tokenises / encodes / decodes only its block of ``data``; the ids are gathered in caption order."""
    if tokenize is None:
        from .clip import tokenize
    cdist.check_world(rank, world)
    n = len(data)
    lo, hi = cdist.shard_bounds(n, rank, world)
    feats = []
    for b0 in range(lo, hi, max(1, text_batch)):
        toks = tokenize([d["caption"] for d in data[b0:min(hi, b0 + max(1, text_batch))]])
        feats.append(clip_model.encode_text(toks).float())
    stop = tokenizer.encode('.')[0]
    if feats:
        ids, lens, _ = caption_ids(model, torch.cat(feats), stop, beam, 5, entry_length, dont_normalize_prefix, modality_offset,
                                   **_given(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, logit_bias=logit_bias))
    else:                              # an empty shard (more ranks than captions) still takes part in the gather
        dev = next(model.parameters()).device
        ids = torch.zeros(0, entry_length, dtype=torch.int32, device=dev)
        lens = torch.zeros(0, dtype=torch.int32, device=dev)
    ids, lens, _ = cdist.gather_ids(ids, lens, n)
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    new_data = [{"caption": tokenizer.decode(list(ids[i, :int(lens[i])])).lower(), "image_id": d["image_id"]}
                for i, d in enumerate(data)]
    if out_path and rank == 0:
        with open(out_path, 'w') as outfile:
            json.dump(new_data, outfile)
    return new_data


# ---------------------------------------------------------------------------- distance ablations
def count_ready_parphrased_embeddings(embeddings_dict):
    """reference :18-24: how many images have all five of their captions' embeddings"""
    ready = 0
    for img_id in embeddings_dict.keys():
        if embeddings_dict[img_id] is not None:
            if len(embeddings_dict[img_id]) == 5:
                ready += 1
    return ready


def _group_by_image(image_ids):
    """rows grouped by image id in order of first appearance (the insertion order of the reference's dict), a group's rows
    in input order -> (index int32 [N], offsets int32 [groups + 1], the ids)"""
    if hasattr(image_ids, "tolist"):        # a tensor or an array: its elements would hash by identity, one group per row
        image_ids = image_ids.tolist()
    rows: Dict = {}
    for r, i in enumerate(image_ids):
        rows.setdefault(i, []).append(r)
    index = np.array([r for v in rows.values() for r in v], np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(v) for v in rows.values()])]).astype(np.int32)
    return index, offsets, list(rows)


def paraphrase_distances(prefix_embed: torch.Tensor, clip_embed: torch.Tensor, image_ids: Sequence,
                         engine: Optional[Engine] = None):
    """The batched ``--ablation_dist``: row r of ``prefix_embed`` [N, W1] (a caption's mapped prefix, flattened) and of
    ``clip_embed`` [N, W2] (its CLIP embedding) belongs to image ``image_ids[r]``.  -> (prefix [groups, 8], clip [groups, 8],
    ids): per image, in order of first appearance, the columns of ``Engine.group_distances`` as host numpy.  The rows are
    grouped through an index, never gathered."""
    if len(image_ids) != prefix_embed.shape[0] or len(image_ids) != clip_embed.shape[0]:
        raise ValueError(f"paraphrase_distances: {len(image_ids)} image ids but {prefix_embed.shape[0]} prefix rows and "
                         f"{clip_embed.shape[0]} CLIP rows")
    eng = engine or get_engine()
    index, offsets, ids = _group_by_image(image_ids)
    idx = torch.tensor(index, dtype=torch.int32, device=eng.device)
    pre = eng.group_distances(prefix_embed.reshape(prefix_embed.shape[0], -1), offsets, idx).cpu().numpy()
    clp = eng.group_distances(clip_embed.reshape(clip_embed.shape[0], -1), offsets, idx).cpu().numpy()
    return pre, clp, ids


def _print_distances(pre: np.ndarray, clp: np.ndarray):
    """reference :59-88 on the per-image columns: the pair statistics over the images with exactly five captions, the
    to-centre statistics over every image"""
    five = clp[:, 7] == 5
    distances, distances_l2 = pre[five, 0].astype(np.float64), pre[five, 1].astype(np.float64)
    distances_clip, distances_l2_clip = clp[five, 0].astype(np.float64), clp[five, 1].astype(np.float64)
    max_distances_l1, maxoutof5 = clp[five, 2].astype(np.float64), clp[five, 3].astype(np.float64)
    distances_l2_from_center, max_distances_l1_from_center = clp[:, 4].astype(np.float64), clp[:, 5].astype(np.float64)
    print(
        f"\n\n\n Average noremlised L1 between 5 annotations of same image MAPPER: {np.array(distances).mean()}, STD: {np.array(distances).std()}")
    print(
        f"\n\n\n Average noremlised L2 between 5 annotations of same image MAPPER: {np.array(distances_l2).mean()}, STD: {np.array(distances_l2).std()}")
    print(
        f"\n\n\n Average noremlised L1 between 5 annotations of same image CLIP: {np.array(distances_clip).mean()}, STD: {np.array(distances_clip).std()}")
    print(
        f"\n\n\n Average noremlised L2 between 5 annotations of same image CLIP: {np.array(distances_l2_clip).mean()}, STD: {np.array(distances_l2_clip).std()}")
    print(
        f"\n\n\n Mean L2 between 5 annotations of same image CLIP to their center: {np.array(distances_l2_from_center).mean()}, STD: {np.array(distances_l2_from_center).std()}")
    print(
        f"\n\n\n Max (per-entry) L1 between 5 annotations of same image CLIP to their center: {np.array(max_distances_l1_from_center).mean()}, STD: {np.array(max_distances_l1_from_center).std()}")
    print(
        f"\n\n\n Max (per-entry) L1 between 5 annotations of same image CLIP: {np.array(max_distances_l1).mean()}, STD: {np.array(max_distances_l1).std()}")
    print(
        f"\n\n\n Taking max out of the 10 L2 between 5 annotations of same image CLIP: {np.array(maxoutof5).mean()}")
    return (list(distances), list(distances_l2), list(distances_clip), list(distances_l2_clip), list(max_distances_l1))


def calc_distances_of_ready_embeddings(embeddings_dict, out_file='embeddings_distances.pkl'):
    """reference :32-95.  ``embeddings_dict``: image id -> list of ``(prefix_embed, clip_embed)`` arrays, one per caption
    (at most eight per image).  Prints the reference's eight lines and returns its ``(distances, distances_l2,
    distances_clip, distances_l2_clip, data_size)``; with an ``out_file`` it also writes the reference's pickle
    (``distances_clip``, ``distances_l2_clip``, ``max_distances_l1``).  One deviation: it then RETURNS -- the reference calls
    ``exit(0)`` there."""
    ids = [i for i in embeddings_dict.keys() for _ in embeddings_dict[i]]
    pairs = [p for i in embeddings_dict.keys() for p in embeddings_dict[i]]
    if not pairs:
        raise ValueError("calc_distances_of_ready_embeddings: no embeddings")
    prefix = torch.tensor(np.stack([np.asarray(p[0], np.float32).reshape(-1) for p in pairs]))
    clip_e = torch.tensor(np.stack([np.asarray(p[1], np.float32).reshape(-1) for p in pairs]))
    pre, clp, groups = paraphrase_distances(prefix, clip_e, ids)
    distances, distances_l2, distances_clip, distances_l2_clip, max_distances_l1 = _print_distances(pre, clp)
    data_size = len(groups)
    if out_file is not None:
        import pickle
        with open(out_file, 'wb') as f:
            pickle.dump(({"distances_clip": distances_clip, "distances_l2_clip": distances_l2_clip, "max_distances_l1": max_distances_l1}), f)
        print(f"Saved distances to {out_file} and finished")
    return distances, distances_l2, distances_clip, distances_l2_clip, data_size


def paraphrase_distance_ablation(data: Sequence[Dict], clip_model, model: ClipCaptionModel, tokenize=None,
                                 dont_normalize_prefix: bool = False, modality_offset: Optional[torch.Tensor] = None,
                                 text_batch: int = 2048):
    """The ``--ablation_dist`` run of the reference on its text-input data (``dataset_mode`` 5; :215-228, :235-239) as one
    batch: ``data[i]`` = {"image_id", "caption"}; captions -> ``clip_model.encode_text`` -> normalise (+ modality offset) ->
    ``model.clip_project`` -> the distances among each image's prefixes and among its CLIP embeddings.  Nothing passes
    through the host in between.  -> what ``paraphrase_distances`` returns."""
    if tokenize is None:
        from .clip import tokenize
    feats = []
    for b0 in range(0, len(data), max(1, text_batch)):
        feats.append(clip_model.encode_text(tokenize([d["caption"] for d in data[b0:b0 + max(1, text_batch)]])).float())
    if not feats:
        raise ValueError("paraphrase_distance_ablation: no captions")
    eng = model.engine
    prefix = eng.normalize_prefix(torch.cat(feats), normalize=not dont_normalize_prefix, offset=modality_offset)
    prefix_embed = model.clip_project(prefix).reshape(prefix.shape[0], -1)
    return paraphrase_distances(prefix_embed, prefix, [d["image_id"] for d in data], eng)


def image_text_distance(image_embeddings: torch.Tensor, text_embeddings: torch.Tensor, engine: Optional[Engine] = None) -> float:
    """the ``--ablation_image_dist`` number (reference :240-247 and its final average): the mean over the rows of the L2
    distance between the normalised image embedding and the normalised embedding of its caption"""
    pair = (engine or get_engine()).embed_moments(image_embeddings, text_embeddings, normalize=True, return_pair=True)["pair"]
    return float(pair.cpu().numpy()[:, 0].astype(np.float64).mean())


def estimate_noise_variance(text_embeddings: torch.Tensor, image_ids: Sequence, normalize: bool = True,
                            engine: Optional[Engine] = None) -> float:
    """The quantity ``--noise_variance 0.016`` of the reference's README stands for: over the images with at least two
    captions, the mean of the per-entry maximum distance between the CLIP text embeddings of captions that describe the same
    image, averaged over the image's pairs -- the reference's "Max (per-entry) L1 between 5 annotations of same image CLIP"
    (:55, :65, :86), here for any 2 to 8 captions per image.  ``text_embeddings`` [N, D]; ``image_ids[r]`` the image of row
    r; ``normalize``: divide every row by its L2 norm first, as the reference's inference path does (:221-222)."""
    eng = engine or get_engine()
    x = eng.normalize_prefix(text_embeddings, normalize=True) if normalize else text_embeddings
    index, offsets, _ = _group_by_image(image_ids)
    out = eng.group_distances(x, offsets, torch.tensor(index, dtype=torch.int32, device=eng.device)).cpu().numpy()
    many = out[:, 7] >= 2
    if not many.any():
        raise ValueError("estimate_noise_variance: no image has two captions")
    return float(out[many, 2].astype(np.float64).mean())
