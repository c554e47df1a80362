"""Reference ``others/modality_offset_calculator.py`` under its own names: the centres of the image and the text embeddings,
the modality offset between them (``--add_modality_offset``) and the spread of their difference, from an
``embeddings_generator`` pickle or from a pair of tensors.

The reference normalises 20 000 (``get_centers_info``) or 200 000 (``get_variance_info``) rows of each side with fp32 torch
on the host and reduces them there.  Here both are one ``Engine.embed_moments`` call (capdec_embed_moments: every sum in fp64;
its memory traffic: include/capdec.h); what is left for the host is numpy on the [7, D] result -- the norms, means and
extrema over the D columns that the print lines show.  The lines have the reference's text and format.

``path_or_data``: the path of a pickle in the ``embeddings_generator`` layout (``formats.load_embeddings_pickle``; the
reference hard-codes ``coco_clip_embeddings/oscar_split_RN50x4_train_with_text_embeddings.pkl``) or a pair
``(image_embeddings, text_embeddings)`` of [N, D] tensors, fp16 or fp32, host or device.  Row i of one side belongs to row i
of the other, as in the reference's parallel slices."""
from __future__ import annotations

import pickle
from typing import Optional, Tuple

import numpy as np
import torch

from . import formats
from ._capi import CapdecError
from .engine import Engine, get_engine

DEFAULT_EMBEDDINGS = 'coco_clip_embeddings/oscar_split_RN50x4_train_with_text_embeddings.pkl'
DEFAULT_CENTERS = 'CLIP_embeddings_centers_info.pkl'


def _sides(path_or_data, limit: int) -> Tuple[torch.Tensor, torch.Tensor]:
    if isinstance(path_or_data, (str, bytes)) or hasattr(path_or_data, "__fspath__"):
        images, texts, _ = formats.load_embeddings_pickle(path_or_data)
    else:
        images, texts = path_or_data
    images, texts = images[:limit], texts[:limit]
    if images.dim() != 2 or tuple(images.shape) != tuple(texts.shape) or images.shape[0] < 1:
        raise CapdecError(f"modality offset: image and text embeddings must both be [N >= 1, D], got {tuple(images.shape)} "
                          f"and {tuple(texts.shape)}")
    return images, texts


def _moments(path_or_data, limit: int, engine: Optional[Engine]):
    images, texts = _sides(path_or_data, limit)
    m = (engine or get_engine()).embed_moments(images, texts, normalize=True)
    return {k: v.cpu().numpy().astype(np.float64) for k, v in m.items()}


def _norm(v: np.ndarray) -> float:
    return float(np.sqrt((v * v).sum()))


def _row(v: np.ndarray) -> torch.Tensor:
    return torch.tensor(v.astype(np.float32)).reshape(1, -1)


def get_centers_info(path_or_data=DEFAULT_EMBEDDINGS, limit: int = 20000, engine: Optional[Engine] = None):
    """-> (center_text, center_image, offset_to_add_in_training, offset_to_add_in_inference), each fp32 [1, D] on the host,
    over the first ``limit`` rows; prints the reference's two 'Offset analysis' lines (:22-24)."""
    m = _moments(path_or_data, limit, engine)
    md, sd = m["mean_diff"], m["std_diff"]
    print(f'Offset analysis: L2 norm={_norm(md):.2f}, Mean={m["absmean_diff"].mean():.2f}, Max={np.abs(md).max():.2f}, Min={np.abs(md).min():.2f}')
    print(f'STD of Offset analysis: L2 norm={_norm(sd):.2f}, Mean={sd.mean():.2f}, Max={sd.max():.2f}, Min={sd.min():.2f}')
    return _row(m["mean_b"]), _row(m["mean_a"]), _row(-md), _row(md)


def get_variance_info(path_or_data=DEFAULT_EMBEDDINGS, limit: int = 200000, engine: Optional[Engine] = None):
    """prints the reference's three 'STD norm' lines (:36-44) and returns the three norms: of the column standard deviations
    of the difference, of the image embeddings and of the text embeddings"""
    m = _moments(path_or_data, limit, engine)
    out = tuple(float(np.float32(_norm(m[k]))) for k in ("std_diff", "std_a", "std_b"))
    print(f'STD norm of diff ={out[0]}')
    print(f'STD norm of image embeddings ={out[1]}')
    print(f'STD norm of text embeddings ={out[2]}')
    return out


def save_centers_info_to_pickle(out_path=DEFAULT_CENTERS, path_or_data=DEFAULT_EMBEDDINGS, limit: int = 20000,
                                engine: Optional[Engine] = None):
    """writes the reference's four keys (:47-57) as fp32 [1, D] tensors: the file ``formats.load_modality_offset`` and the
    reference's ``get_precalculated_centers`` read"""
    center_text, center_image, offset_to_add_in_training, offset_to_add_in_inference = get_centers_info(path_or_data, limit, engine)
    with open(out_path, 'wb') as f:
        pickle.dump({
            'center_text': center_text,
            'center_image': center_image,
            'offset_to_add_in_training': offset_to_add_in_training,
            'offset_to_add_in_inference': offset_to_add_in_inference,
        }, f)
    print(f'norm of diff ={float(np.float32(_norm(offset_to_add_in_inference.numpy().astype(np.float64))))}')
    print('saved centers info to pickle successfully')


def get_precalculated_centers(path=DEFAULT_CENTERS):
    with open(path, 'rb') as f:
        return pickle.load(f)
