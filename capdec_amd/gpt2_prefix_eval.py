"""Drop-in surface of reference ``gpt2_prefix_eval.py``: ``generate_beam`` (:50-115) and
``generate2`` (:118-198) with the reference signatures, plus batched variants
(``embed`` [N, P, 768]) that the throughput path uses.  The per-token Python loop, the
no-cache re-forward and the per-token host syncs of the reference are replaced by one call
into the KV-cached HIP decode (``capdec_decode_greedy`` / ``capdec_decode_beam``).  ``generate_diverse_beam`` /
``generate_diverse_beam_batch`` are ``generate_beam`` with diverse (group) beam search (``capdec_decode_beam_groups``:
``num_beam_groups`` / ``diversity_penalty``), for callers who want beams that differ.  ``generate_constrained_beam`` /
``generate_constrained_beam_batch`` are ``generate_beam`` with words that must occur in the caption
(``capdec_decode_beam_constrained``: ``force_words_ids`` of ``transformers.generate``).  ``generate_samples`` /
``generate_samples_batch`` make ``top_p``, ``temperature`` and ``entry_count`` live: nucleus sampling
(``capdec_decode_sample``), the multinomial line the reference leaves commented out (:178).  ``generate_guided`` /
``generate_guided_batch`` decode under classifier-free guidance against a negative prefix (``capdec_decode_guided``:
``guidance_scale`` of ``transformers.generate``), greedy or beam.

Logits processors (``engine.LogitsProcessors``; the contract: include/capdec.h).  The batched functions take them as
keyword-only arguments (None: not given); ``generate2`` / ``generate_beam`` keep the reference's signatures and read
``model.logits_processors`` instead, which is also what a batched function starts from before its own keywords go on top.
Whatever is switched on is set on the engine for the one decode call and cleared after it.

Prefix interpretation and editing (reference :201-251): ``get_prefix_tokens`` reads each prefix vector as its nearest
vocabulary token under cosine similarity (``capdec_nearest_tokens``: the [rows, vocab] similarity matrix never exists);
``add_embedding_from_text`` / ``generate_text`` / ``re_caption`` / ``remove_token`` / ``try_all_places`` are the probes built
on it, with the reference's names and signatures.  ``prefix_token_ids`` / ``get_prefix_tokens_batch`` are the batched forms;
``try_all_places`` decodes its P edited prefixes as one batch."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._capi import CapdecError
from .engine import MAX_PHRASE_TOKENS, MAX_PHRASES, LogitsProcessors, get_engine, pack_phrases
from .gpt2_prefix import ClipCaptionModel
from .train import _next_seed

ALT_STOP_ID = 764   # hard-coded second stop id of generate2 (reference gpt2_prefix_eval.py:187)


def _prefix_from(model, tokenizer, tokens, prompt, embed) -> Tuple[torch.Tensor, Optional[List[int]]]:
    """reference :70-74 / :141-151: use ``embed`` if given, else wte(tokens or encode(prompt))."""
    if embed is not None:
        return embed, None
    if tokens is None:
        tokens = torch.tensor(tokenizer.encode(prompt))
        tokens = tokens.unsqueeze(0)
    tokens = tokens.reshape(1, -1)
    return model.gpt.transformer.wte(tokens), [int(t) for t in tokens.reshape(-1).tolist()]


def _processor_kw(model, sampling: bool = False, **kw) -> dict:
    """the processor keywords of the engine's decode call: ``model.logits_processors`` with the given (not None) keywords
    on top; only what is switched on is passed, so a call without processors is the call it always was.  ``top_k`` goes
    to the sampling decode only."""
    p = LogitsProcessors.of(getattr(model, "logits_processors", None), **kw)
    if p is None:
        return {}
    out = {}
    if p.repetition_penalty != 1.0:
        out["repetition_penalty"] = p.repetition_penalty
    if p.no_repeat_ngram_size:
        out["no_repeat_ngram_size"] = p.no_repeat_ngram_size
    if p.min_length:
        out["min_length"] = p.min_length
    if p.logit_bias is not None:
        out["logit_bias"] = p.logit_bias
    if sampling and p.top_k:
        out["top_k"] = p.top_k
    return out


# --------------------------------------------------------------------------- batched id-level API
def decode_greedy_ids(model: ClipCaptionModel, embed: torch.Tensor, stop_token_index: int, entry_length: int = 67,
                      alt_stop_id: int = ALT_STOP_ID, *, repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                      min_length: Optional[int] = None, logit_bias=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """embed [N, P, d] -> ids int32 [N, entry_length] (zero padded), lens int32 [N] (tokens
    emitted INCLUDING the stop token) -- device tensors."""
    kw = _processor_kw(model, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, logit_bias=logit_bias)
    return model.engine.decode_greedy(embed, stop_token_index, entry_length, alt_stop_id, **kw)


def decode_beam_ids(model: ClipCaptionModel, embed: torch.Tensor, stop_token_index: int, beam_size: int = 5,
                    entry_length: int = 67, temperature: float = 1.0, *, repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                    min_length: Optional[int] = None, logit_bias=None):
    """embed [N, P, d] -> (ids [N, beam, T], lens [N, beam], scores [N, beam], order [N, beam]),
    beams sorted by mean log-prob descending (the order generate_beam returns)."""
    kw = _processor_kw(model, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, logit_bias=logit_bias)
    return model.engine.decode_beam(embed, stop_token_index, beam_size, entry_length, temperature, **kw)


def decode_diverse_beam_ids(model: ClipCaptionModel, embed: torch.Tensor, stop_token_index: int, beam_size: int = 6,
                            num_beam_groups: int = 3, diversity_penalty: float = 0.5, entry_length: int = 67,
                            temperature: float = 1.0, *, repetition_penalty: Optional[float] = None,
                            no_repeat_ngram_size: Optional[int] = None, min_length: Optional[int] = None, logit_bias=None):
    """embed [N, P, d] -> (ids [N, beam, T], lens [N, beam], scores [N, beam], order [N, beam], logp [N, beam]) of the
    diverse (group) beam search (``capdec_decode_beam_groups``): rows sorted by their penalised mean log-prob descending;
    ``order // (beam_size // num_beam_groups)`` is a row's group, ``logp`` its unpenalised log-prob sum."""
    kw = _processor_kw(model, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, logit_bias=logit_bias)
    return model.engine.decode_beam_groups(embed, stop_token_index, beam_size, num_beam_groups, diversity_penalty, entry_length,
                                           temperature, **kw)


def encode_force_words(tokenizer, words: Sequence[str]) -> List[List[int]]:
    """the phrases of one caption from its words: ``tokenizer.encode(" " + word)`` each (GPT-2's BPE marks the leading
    space, so this is the word as it stands inside a sentence).  More than 4 words, or a word of more than 4 tokens (or of
    none), is a CapdecError that names the word."""
    words = list(words)
    if len(words) > MAX_PHRASES:
        raise CapdecError(f"force_words: at most {MAX_PHRASES} words per caption, got {len(words)}: {words!r} (first one too many: "
                          f"{words[MAX_PHRASES]!r})")
    out = []
    for w in words:
        if not isinstance(w, str):
            raise CapdecError(f"force_words: a word must be a string, got {w!r}")
        ids = [int(t) for t in tokenizer.encode(" " + w)]
        if not 1 <= len(ids) <= MAX_PHRASE_TOKENS:
            raise CapdecError(f"force_words: the word {w!r} encodes to {len(ids)} tokens, 1..{MAX_PHRASE_TOKENS} are supported")
        out.append(ids)
    return out


def _phrases_of(tokenizer, n: int, force_words, force_words_ids) -> np.ndarray:
    """the [n, 4, 4] phrase table from per-caption words or per-caption id lists (both None: no phrases)"""
    if force_words is not None and force_words_ids is not None:
        raise CapdecError("give force_words or force_words_ids, not both")
    if force_words is not None:
        per_caption = [encode_force_words(tokenizer, ws) for ws in force_words]
    elif force_words_ids is not None:
        per_caption = [list(p) for p in force_words_ids]
    else:
        per_caption = [[] for _ in range(n)]
    if len(per_caption) != n:
        raise CapdecError(f"constrained beam search: {len(per_caption)} lists of forced words for {n} captions")
    return pack_phrases(per_caption)


def decode_constrained_beam_ids(model: ClipCaptionModel, embed: torch.Tensor, phrases, stop_token_index: int,
                                beam_size: int = 5, entry_length: int = 67, temperature: float = 1.0, *,
                                repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                                min_length: Optional[int] = None, logit_bias=None):
    """embed [N, P, d], phrases (per caption a list of up to 4 id lists of 1..4 tokens, or int32 [N, 4, 4] with -1 in the
    unused places) -> (ids [N, beam, T], lens [N, beam], scores [N, beam], order [N, beam], met [N, beam]) of the lexically
    constrained beam search (``capdec_decode_beam_constrained``): rows sorted by the number of phrases they hold, then by
    mean log-prob, descending; ``met`` is the bitmask of the phrases a row holds."""
    kw = _processor_kw(model, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, logit_bias=logit_bias)
    return model.engine.decode_beam_constrained(embed, phrases, stop_token_index, beam_size, entry_length, temperature, **kw)


def sample_ids(model: ClipCaptionModel, embed: torch.Tensor, stop_token_index: int, entry_length: int = 67,
               top_p: float = 0.8, temperature: float = 1., seed: Optional[int] = None, u: Optional[torch.Tensor] = None,
               alt_stop_id: int = ALT_STOP_ID, return_logp: bool = False, *, repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
               min_length: Optional[int] = None, logit_bias=None,
               top_k: Optional[int] = None):
    """embed [N, P, d] -> ids int32 [N, entry_length] (zero padded), lens int32 [N] (including the stop token), drawn
    by nucleus sampling: one uniform per (caption, step), from ``u`` [N, entry_length] or from the device Philox keyed by
    (``seed``, caption index, step); ``seed=None`` takes the process's next key
    (``train._next_seed``: torch's global seed and the number of keys drawn so far), so successive calls differ and a
    program that seeds torch and makes the same calls in the same order repeats its captions."""
    kw = _processor_kw(model, True, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, logit_bias=logit_bias, top_k=top_k)
    return model.engine.decode_sample(embed, stop_token_index, entry_length, temperature, top_p,
                                      _next_seed() if seed is None else seed, u, alt_stop_id, return_logp, **kw)


def generate_samples_batch(model, tokenizer, embed: torch.Tensor, entry_count: int = 1, entry_length: int = 67,
                           top_p: float = 0.8, temperature: float = 1., stop_token: str = '.',
                           seed: Optional[int] = None, *, repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                           min_length: Optional[int] = None, logit_bias=None,
                           top_k: Optional[int] = None) -> List[List[str]]:
    """embed [N, P, d] -> ``entry_count`` sampled texts per caption.  Every prefix row is repeated ``entry_count``
    times; each repeat is a caption index of its own (caption r, entry e -> index r * entry_count + e) and so has its
    own draws."""
    if entry_count < 1:
        raise CapdecError("generate_samples_batch: entry_count must be >= 1")
    stop = tokenizer.encode(stop_token)[0]
    ids, lens = sample_ids(model, embed.repeat_interleave(entry_count, dim=0), stop, entry_length, top_p, temperature, seed,
                           repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, logit_bias=logit_bias, top_k=top_k)
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    return [[tokenizer.decode(list(ids[r * entry_count + e, :lens[r * entry_count + e]])) for e in range(entry_count)]
            for r in range(embed.shape[0])]


def score_ids(model: ClipCaptionModel, embed: torch.Tensor, tokens: torch.Tensor, lens=None, ignore_id: int = -1,
              temperature: float = 1., return_top1: bool = False):
    """embed [N, P, d], tokens [N, L], lens [N] (None: all L) -> (logp [N, L], sum [N], count [N][, top1 [N, L]]) device
    tensors: the log-probability the model gives every token of the given captions (capdec_score; the logits are never
    materialised)."""
    return model.engine.score(embed, tokens, lens, ignore_id, temperature, return_top1)


def score_captions(model, tokenizer, embed: torch.Tensor, texts, temperature: float = 1.):
    """embed [N, P, d] and ``texts`` -- one string per prefix row, or a list of K strings per row (K candidates repeat
    their prefix row, like ``generate_samples_batch``'s entries) -> ``(sum logp, token count)`` per text, shaped like
    ``texts``.  A text is scored as ``tokenizer.encode`` gives it: include the stop token to score the caption as the
    decoders emit it."""
    n = int(embed.shape[0])
    texts = list(texts)
    if len(texts) != n:
        raise CapdecError(f"score_captions: {len(texts)} texts for {n} prefix rows")
    flat = all(isinstance(t, str) for t in texts)
    rows = [[t] for t in texts] if flat else [list(t) for t in texts]
    if any(isinstance(t, str) for t in texts) and not flat:
        raise CapdecError("score_captions: texts is either one string per row or one list of strings per row")
    K = len(rows[0]) if rows else 0
    if K < 1 or any(len(r) != K for r in rows):
        raise CapdecError("score_captions: every prefix row needs the same number (>= 1) of candidate texts")
    enc = [[int(t) for t in tokenizer.encode(s)] for r in rows for s in r]
    lens = [len(e) for e in enc]
    L = max(max(lens), 1)
    tokens = torch.zeros(n * K, L, dtype=torch.int32)
    for i, e in enumerate(enc):
        tokens[i, :len(e)] = torch.tensor(e, dtype=torch.int32)
    _, s, c = score_ids(model, embed.repeat_interleave(K, dim=0) if K > 1 else embed, tokens, lens, -1, temperature)
    s, c = s.cpu().tolist(), c.cpu().tolist()
    out = [(float(a), int(b)) for a, b in zip(s, c)]
    return out if flat else [out[r * K:(r + 1) * K] for r in range(n)]


def generate2_batch(model, tokenizer, embed: torch.Tensor, entry_length: int = 67, stop_token: str = '.', *,
                    repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                    min_length: Optional[int] = None, logit_bias=None) -> List[str]:
    stop = tokenizer.encode(stop_token)[0]
    ids, lens = decode_greedy_ids(model, embed, stop, entry_length, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, logit_bias=logit_bias)
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    return [tokenizer.decode(list(ids[r, :lens[r]])) for r in range(ids.shape[0])]


def generate_beam_batch(model, tokenizer, embed: torch.Tensor, beam_size: int = 5, entry_length: int = 67,
                        temperature: float = 1., stop_token: str = '.', *, repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                        min_length: Optional[int] = None, logit_bias=None) -> List[List[str]]:
    stop = tokenizer.encode(stop_token)[0]
    ids, lens, _, _ = decode_beam_ids(model, embed, stop, beam_size, entry_length, temperature, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, logit_bias=logit_bias)
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    return [[tokenizer.decode(ids[r, b, :int(lens[r, b])]) for b in range(ids.shape[1])] for r in range(ids.shape[0])]


def generate_diverse_beam_batch(model, tokenizer, embed: torch.Tensor, beam_size: int = 6, num_beam_groups: int = 3,
                                diversity_penalty: float = 0.5, entry_length: int = 67, temperature: float = 1.,
                                stop_token: str = '.', per_group: bool = False, *, repetition_penalty: Optional[float] = None,
                                no_repeat_ngram_size: Optional[int] = None, min_length: Optional[int] = None,
                                logit_bias=None) -> List[List[str]]:
    """embed [N, P, d] -> per caption the ``beam_size`` texts of the diverse beam search, best first; with ``per_group`` the
    best text of each group, in group order (``num_beam_groups`` texts)"""
    stop = tokenizer.encode(stop_token)[0]
    ids, lens, _, order, _ = decode_diverse_beam_ids(model, embed, stop, beam_size, num_beam_groups, diversity_penalty, entry_length,
                                                     temperature, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                                     min_length=min_length, logit_bias=logit_bias)
    ids, lens, order = ids.cpu().numpy(), lens.cpu().numpy(), order.cpu().numpy()
    out = []
    for r in range(ids.shape[0]):
        rows = list(range(ids.shape[1]))
        if per_group:       # rows are sorted best first: the first row of every group is its best
            group = order[r] // (beam_size // num_beam_groups)
            rows = [int(np.nonzero(group == g)[0][0]) for g in range(num_beam_groups)]
        out.append([tokenizer.decode(ids[r, b, :int(lens[r, b])]) for b in rows])
    return out


def generate_constrained_beam_batch(model, tokenizer, embed: torch.Tensor, beam_size: int = 5, force_words=None,
                                    force_words_ids=None, entry_length: int = 67, temperature: float = 1.,
                                    stop_token: str = '.', return_met: bool = False, *,
                                    repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                                    min_length: Optional[int] = None, logit_bias=None):
    """``generate_beam_batch`` with words every caption must contain: ``force_words`` is one list of up to 4 words per
    caption (each encoded as ``" " + word``, up to 4 tokens), ``force_words_ids`` one list of up to 4 token-id lists per
    caption.  -> per caption the ``beam_size`` texts, the rows that hold the most words first, then by score; with
    ``return_met`` also the int array [N, beam] of the bitmasks of the words each row holds (a row lacks a word only when
    ``entry_length`` ran out first)."""
    stop = tokenizer.encode(stop_token)[0]
    phrases = _phrases_of(tokenizer, int(embed.shape[0]), force_words, force_words_ids)
    ids, lens, _, _, met = decode_constrained_beam_ids(model, embed, phrases, stop, beam_size, entry_length, temperature,
                                                       repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                                       min_length=min_length, logit_bias=logit_bias)
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    texts = [[tokenizer.decode(ids[r, b, :int(lens[r, b])]) for b in range(ids.shape[1])] for r in range(ids.shape[0])]
    return (texts, met.cpu().numpy()) if return_met else texts


# --------------------------------------------------------------------------- reference signatures
def generate_beam(model: ClipCaptionModel, tokenizer, beam_size: int = 5, prompt=None, embed=None,
                  entry_length=67, temperature=1., stop_token: str = '.'):
    """reference gpt2_prefix_eval.py:50-115 -> List[str] of ``beam_size`` texts, best first.  (Logits processors:
    ``model.logits_processors``.)"""
    model.eval()
    prefix, prompt_ids = _prefix_from(model, tokenizer, None, prompt, embed)
    if prefix.shape[0] != 1:
        raise CapdecError("generate_beam takes one caption ([1, P, d]); use generate_beam_batch for [N, P, d]")
    stop = tokenizer.encode(stop_token)[0]
    ids, lens, _, _ = decode_beam_ids(model, prefix, stop, beam_size, entry_length, temperature)
    ids, lens = ids.cpu().numpy()[0], lens.cpu().numpy()[0]
    out = []
    for b in range(beam_size):
        toks = ids[b, :int(lens[b])]
        if prompt_ids is not None:   # reference :86-87: prompt tokens stay in the output
            # seq_lengths counts generated tokens only (+ the reference slices the concatenated row)
            toks = np.concatenate([np.asarray(prompt_ids, dtype=toks.dtype), ids[b]])[:int(lens[b])]
        out.append(tokenizer.decode(toks))
    return out


def generate_constrained_beam(model: ClipCaptionModel, tokenizer, beam_size: int = 5, prompt=None, embed=None,
                              force_words=None, force_words_ids=None, entry_length=67, temperature=1.,
                              stop_token: str = '.'):
    """``generate_beam`` with words the caption must contain: one caption ([1, P, d], or a prompt), ``force_words`` a list
    of up to 4 words (each encoded as ``" " + word``, up to 4 tokens) or ``force_words_ids`` a list of up to 4 token-id
    lists -> ``beam_size`` texts ordered like ``generate_beam``'s, the rows that hold the most words in front.  Prompt
    tokens stay in front as in ``generate_beam``.  (Logits processors: ``model.logits_processors``.)"""
    model.eval()
    prefix, prompt_ids = _prefix_from(model, tokenizer, None, prompt, embed)
    if prefix.shape[0] != 1:
        raise CapdecError("generate_constrained_beam takes one caption ([1, P, d]); use generate_constrained_beam_batch for [N, P, d]")
    stop = tokenizer.encode(stop_token)[0]
    phrases = _phrases_of(tokenizer, 1, None if force_words is None else [force_words],
                          None if force_words_ids is None else [force_words_ids])
    ids, lens = decode_constrained_beam_ids(model, prefix, phrases, stop, beam_size, entry_length, temperature)[:2]
    ids, lens = ids.cpu().numpy()[0], lens.cpu().numpy()[0]
    out = []
    for b in range(beam_size):
        toks = ids[b, :int(lens[b])]
        if prompt_ids is not None:   # as generate_beam: the prompt tokens stay in the output, the row is cut at seq_lengths
            toks = np.concatenate([np.asarray(prompt_ids, dtype=toks.dtype), ids[b]])[:int(lens[b])]
        out.append(tokenizer.decode(toks))
    return out


def generate_diverse_beam(model: ClipCaptionModel, tokenizer, beam_size: int = 6, num_beam_groups: int = 3,
                          diversity_penalty: float = 0.5, prompt=None, embed=None, entry_length=67, temperature=1.,
                          stop_token: str = '.', per_group: bool = False):
    """``generate_beam`` with diverse (group) beam search: one caption ([1, P, d], or a prompt) -> ``beam_size`` texts, best
    first (``per_group``: the best text of each group, in group order).  Prompt tokens stay in front as in
    ``generate_beam``.  (Logits processors: ``model.logits_processors``.)"""
    model.eval()
    prefix, prompt_ids = _prefix_from(model, tokenizer, None, prompt, embed)
    if prefix.shape[0] != 1:
        raise CapdecError("generate_diverse_beam takes one caption ([1, P, d]); use generate_diverse_beam_batch for [N, P, d]")
    stop = tokenizer.encode(stop_token)[0]
    ids, lens, _, order, _ = decode_diverse_beam_ids(model, prefix, stop, beam_size, num_beam_groups, diversity_penalty,
                                                     entry_length, temperature)
    ids, lens, order = ids.cpu().numpy()[0], lens.cpu().numpy()[0], order.cpu().numpy()[0]
    rows = list(range(beam_size))
    if per_group:
        group = order // (beam_size // num_beam_groups)
        rows = [int(np.nonzero(group == g)[0][0]) for g in range(num_beam_groups)]
    out = []
    for b in rows:
        toks = ids[b, :int(lens[b])]
        if prompt_ids is not None:   # as generate_beam: the prompt tokens stay in the output, the row is cut at seq_lengths
            toks = np.concatenate([np.asarray(prompt_ids, dtype=toks.dtype), ids[b]])[:int(lens[b])]
        out.append(tokenizer.decode(toks))
    return out


def generate2(model, tokenizer, tokens=None, prompt=None, embed=None, entry_count=1, entry_length=67,
              top_p=0.8, temperature=1., stop_token: str = '.'):
    """reference gpt2_prefix_eval.py:118-198 -> str.  ``top_p`` is accepted and has no effect,
    exactly as in the reference: the filter never removes the arg-max (:172), and the next
    token is ``argmax`` (:177); ``temperature`` > 0 does not change an arg-max either.  ``generate_samples`` /
    ``generate_samples_batch`` are the entry points where the three parameters act.  (Logits processors:
    ``model.logits_processors``.)"""
    model.eval()
    prefix, prompt_ids = _prefix_from(model, tokenizer, tokens, prompt, embed)
    if prefix.shape[0] != 1:
        raise CapdecError("generate2 takes one caption ([1, P, d]); use generate2_batch for [N, P, d]")
    stop = tokenizer.encode(stop_token)[0]
    ids, lens = decode_greedy_ids(model, prefix, stop, entry_length)
    n = int(lens.cpu()[0])
    out = [int(t) for t in ids.cpu().numpy()[0, :n]]
    if prompt_ids is not None:
        out = prompt_ids + out
    if len(out) == 1:
        # reference :191 does list(tokens.squeeze().cpu().numpy()) -- a 0-d array when the very
        # first token stops -- and raises; keep the error behaviour
        raise TypeError("iteration over a 0-d array")
    return tokenizer.decode(out)


def generate_samples(model, tokenizer, tokens=None, prompt=None, embed=None, entry_count=1, entry_length=67,
                     top_p=0.8, temperature=1., stop_token: str = '.', seed: Optional[int] = None, *,
                     repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                     min_length: Optional[int] = None, logit_bias=None, top_k: Optional[int] = None) -> List[str]:
    """``generate2``'s signature plus ``seed`` -> ``entry_count`` texts drawn by nucleus sampling from one caption
    ([1, P, d]); prompt tokens stay in front of every text, as in ``generate2``."""
    model.eval()
    prefix, prompt_ids = _prefix_from(model, tokenizer, tokens, prompt, embed)
    if prefix.shape[0] != 1:
        raise CapdecError("generate_samples takes one caption ([1, P, d]); use generate_samples_batch for [N, P, d]")
    if entry_count < 1:
        raise CapdecError("generate_samples: entry_count must be >= 1")
    stop = tokenizer.encode(stop_token)[0]
    ids, lens = sample_ids(model, prefix.repeat_interleave(entry_count, dim=0), stop, entry_length, top_p, temperature, seed,
                           repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, logit_bias=logit_bias, top_k=top_k)
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    return [tokenizer.decode((prompt_ids or []) + [int(t) for t in ids[e, :lens[e]]]) for e in range(entry_count)]


# --------------------------------------------------------------------------- contrastive search
def decode_contrastive_ids(model: ClipCaptionModel, embed: torch.Tensor, stop_token_index: int, top_k: int = 4,
                           penalty_alpha: float = 0.6, entry_length: int = 67, alt_stop_id: int = ALT_STOP_ID,
                           return_trace: bool = False, *, repetition_penalty: Optional[float] = None,
                           no_repeat_ngram_size: Optional[int] = None, min_length: Optional[int] = None, logit_bias=None):
    """embed [N, P, d] -> ids int32 [N, entry_length] (zero padded), lens int32 [N] (including the stop token) of the
    contrastive search (``capdec_decode_contrastive``: ``top_k`` / ``penalty_alpha`` of ``transformers.generate``) and,
    with ``return_trace``, trace [N, entry_length, 2] = (probability, max cosine) of every chosen candidate."""
    kw = _processor_kw(model, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, logit_bias=logit_bias)
    return model.engine.decode_contrastive(embed, top_k, penalty_alpha, stop_token_index, alt_stop_id, entry_length,
                                           return_trace, **kw)


def generate_contrastive_batch(model, tokenizer, embed: torch.Tensor, entry_length: int = 67, top_k: int = 4,
                               penalty_alpha: float = 0.6, stop_token: str = '.', *,
                               repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                               min_length: Optional[int] = None, logit_bias=None) -> List[str]:
    """``generate2_batch`` with contrastive search: embed [N, P, d] -> one text per caption"""
    stop = tokenizer.encode(stop_token)[0]
    ids, lens = decode_contrastive_ids(model, embed, stop, top_k, penalty_alpha, entry_length,
                                       repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                       min_length=min_length, logit_bias=logit_bias)
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    return [tokenizer.decode(list(ids[r, :lens[r]])) for r in range(ids.shape[0])]


def generate_contrastive(model, tokenizer, tokens=None, prompt=None, embed=None, entry_length=67, top_k: int = 4,
                         penalty_alpha: float = 0.6, stop_token: str = '.') -> str:
    """``generate2`` with contrastive search instead of the arg-max: one caption ([1, P, d], tokens or a prompt) -> str.
    Prompt tokens stay in front and 764 is the second stop id, as in ``generate2``; ``penalty_alpha=0`` or ``top_k=1``
    gives ``generate2``'s tokens.  (Logits processors: ``model.logits_processors``.)"""
    model.eval()
    prefix, prompt_ids = _prefix_from(model, tokenizer, tokens, prompt, embed)
    if prefix.shape[0] != 1:
        raise CapdecError("generate_contrastive takes one caption ([1, P, d]); use generate_contrastive_batch for [N, P, d]")
    stop = tokenizer.encode(stop_token)[0]
    ids, lens = decode_contrastive_ids(model, prefix, stop, top_k, penalty_alpha, entry_length)
    n = int(lens.cpu()[0])
    out = [int(t) for t in ids.cpu().numpy()[0, :n]]
    return tokenizer.decode((prompt_ids or []) + out)


# --------------------------------------------------------------------------- classifier-free guidance
def _negative_prefix(model, embed: torch.Tensor, negative_embed) -> torch.Tensor:
    """the negative prefix of the guided decode: ``negative_embed`` if given, else the documented default -- the mapper's
    output for the all-zero CLIP embedding, ``model.clip_project(zeros)``, computed once per call and shared by all captions"""
    if negative_embed is not None:
        return negative_embed
    zeros = torch.zeros(1, model.prefix_dim, device=embed.device, dtype=torch.float32)
    return model.clip_project(zeros).reshape(1, model.prefix_length, -1)


def decode_guided_ids(model: ClipCaptionModel, embed: torch.Tensor, negative_embed, stop_token_index: int,
                      guidance_scale: float = 1.5, beam_size: int = 1, entry_length: int = 67, temperature: float = 1.,
                      alt_stop_id: int = ALT_STOP_ID, *, repetition_penalty: Optional[float] = None,
                      no_repeat_ngram_size: Optional[int] = None, min_length: Optional[int] = None, logit_bias=None):
    """embed [N, P, d], negative_embed [P, d] / [1, P, d] / [N, P, d] (None: ``model.clip_project(zeros)``) -> the
    classifier-free-guided decode (``capdec_decode_guided``): (ids [N, T], lens [N]) for ``beam_size`` 1, (ids [N, beam, T],
    lens [N, beam], scores [N, beam]) best first otherwise"""
    kw = _processor_kw(model, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, logit_bias=logit_bias)
    return model.engine.decode_guided(embed, _negative_prefix(model, embed, negative_embed), guidance_scale, stop_token_index,
                                      beam_size, entry_length, temperature, alt_stop_id, **kw)


def generate_guided_batch(model, tokenizer, embed: torch.Tensor, negative_embed=None, guidance_scale: float = 1.5,
                          beam_size: int = 1, entry_length: int = 67, stop_token: str = '.', temperature: float = 1., *,
                          repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                          min_length: Optional[int] = None, logit_bias=None):
    """``generate2_batch`` (``beam_size`` 1: one text per caption) / ``generate_beam_batch`` (the ``beam_size`` texts per
    caption, best first) under classifier-free guidance against ``negative_embed`` (None: the mapper's output for the
    all-zero CLIP embedding)"""
    stop = tokenizer.encode(stop_token)[0]
    out = decode_guided_ids(model, embed, negative_embed, stop, guidance_scale, beam_size, entry_length, temperature,
                            repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                            min_length=min_length, logit_bias=logit_bias)
    ids, lens = out[0].cpu().numpy(), out[1].cpu().numpy()
    if ids.ndim == 2:
        return [tokenizer.decode(list(ids[r, :lens[r]])) for r in range(ids.shape[0])]
    return [[tokenizer.decode(ids[r, b, :int(lens[r, b])]) for b in range(ids.shape[1])] for r in range(ids.shape[0])]


def generate_guided(model, tokenizer, tokens=None, prompt=None, embed=None, negative_embed=None, guidance_scale: float = 1.5,
                    beam_size: int = 1, entry_length=67, temperature=1., stop_token: str = '.'):
    """``generate2`` (``beam_size`` 1 -> str) / ``generate_beam`` (-> the list of ``beam_size`` texts, best first) under
    classifier-free guidance: one caption ([1, P, d], tokens or a prompt) against ``negative_embed`` ([P, d] or [1, P, d]; None:
    the mapper's output for the all-zero CLIP embedding).  Prompt tokens stay in front as in those functions.  (Logits
    processors: ``model.logits_processors``.)"""
    model.eval()
    prefix, prompt_ids = _prefix_from(model, tokenizer, tokens, prompt, embed)
    if prefix.shape[0] != 1:
        raise CapdecError("generate_guided takes one caption ([1, P, d]); use generate_guided_batch for [N, P, d]")
    stop = tokenizer.encode(stop_token)[0]
    out = decode_guided_ids(model, prefix, negative_embed, stop, guidance_scale, beam_size, entry_length, temperature)
    ids, lens = out[0].cpu().numpy()[0], out[1].cpu().numpy()[0]
    if ids.ndim == 1:
        return tokenizer.decode((prompt_ids or []) + [int(t) for t in ids[:int(lens)]])
    texts = []
    for b in range(ids.shape[0]):
        toks = ids[b, :int(lens[b])]
        if prompt_ids is not None:      # as generate_beam: the prompt tokens stay in the output, the row is cut at seq_lengths
            toks = np.concatenate([np.asarray(prompt_ids, dtype=toks.dtype), ids[b]])[:int(lens[b])]
        texts.append(tokenizer.decode(toks))
    return texts


# --------------------------------------------------------------------------- prefix interpretation and editing
def _nearest(embeddings, x: torch.Tensor, k: int = 1, model=None):
    """(ids, sims) of the rows of ``x`` [..., d] against ``embeddings``: a ClipCaptionModel (its wte, normalised once and
    cached by the library) or a [V, d] tensor as the reference passes it (given to the library as ``table``; normalising an
    already normalised table again is harmless)"""
    if isinstance(embeddings, torch.Tensor):
        if model is not None:
            eng = model.engine
        else:
            dev = x.device if x.device.type == "cuda" else embeddings.device
            eng = get_engine(dev.index or 0)
        return eng.nearest_tokens(x, k, table=embeddings, return_sims=True)
    return embeddings.engine.nearest_tokens(x, k, return_sims=True)


def prefix_token_ids(model: ClipCaptionModel, embed: torch.Tensor, k: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """embed [N, P, d] -> (ids int32 [N, P, k], sims fp32 [N, P, k]): the ``k`` vocabulary tokens nearest to every prefix
    vector, best first -- device tensors"""
    return _nearest(model, embed, k)


def get_prefix_tokens_batch(model: ClipCaptionModel, tokenizer, embed: torch.Tensor) -> List[str]:
    """embed [N, P, d] -> one "prefix sentence" per caption (``get_prefix_tokens`` of each row, one device call)"""
    ids, _ = prefix_token_ids(model, embed, 1)
    ids = ids[..., 0].to(torch.int64).cpu()
    return [tokenizer.decode(ids[r]) for r in range(ids.shape[0])]


def get_prefix_tokens(prefix_embed, embeddings, tokenizer) -> str:
    """reference gpt2_prefix_eval.py:247-251.  ``embeddings``: the ClipCaptionModel, or the (normalised) embedding table
    [V, d] the reference passes"""
    ids, _ = _nearest(embeddings, prefix_embed[0], 1)
    return tokenizer.decode(ids[:, 0].to(torch.int64).cpu())


def add_embedding_from_text(add_in: str, prefix_embed: torch.Tensor, tokenizer, model: ClipCaptionModel, where: int):
    """the prefix [1, P, d] with the embedding rows of ``add_in``'s tokens spliced in before position ``where`` (0: in
    front; P or -1: appended) -> [1, P + m, d].  Name, signature and ``where`` rules of reference :201-212."""
    ids = torch.as_tensor(tokenizer.encode(add_in), device=prefix_embed.device)
    rows = model.get_embedding(ids).to(prefix_embed.device)[None]
    at = prefix_embed.shape[1] if where == -1 else where
    return torch.cat((prefix_embed[:, :at], rows, prefix_embed[:, at:]), 1)


def _decode_texts(embed: torch.Tensor, tokenizer, model: ClipCaptionModel, use_beam: bool) -> List[str]:
    """embed [N, P, d] -> one text per row from ONE decode call, as ``generate_beam(..., beam_size=5)[0]`` /
    ``generate2`` give it with their defaults (entry_length 67, stop token '.', the model's logits processors)"""
    model.eval()
    stop = tokenizer.encode('.')[0]
    if use_beam:
        ids, lens, _, _ = decode_beam_ids(model, embed, stop, 5)
        ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
        return [tokenizer.decode(ids[r, 0, :int(lens[r, 0])]) for r in range(ids.shape[0])]
    ids, lens = decode_greedy_ids(model, embed, stop)
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    first = [r for r in range(ids.shape[0]) if lens[r] == 1]
    if first:      # generate2 raises a TypeError for such a caption (the reference's squeeze() to a 0-d array, :191)
        raise TypeError(f"iteration over a 0-d array: the first token stops the greedy decode of row(s) {first}")
    return [tokenizer.decode([int(t) for t in ids[r, :lens[r]]]) for r in range(ids.shape[0])]


def generate_text(prefix_embed: torch.Tensor, tokenizer, model: ClipCaptionModel, use_beam: bool) -> str:
    """the caption of one prefix [1, P, d]: the best of 5 beams, or the greedy text (reference :215-220)"""
    if prefix_embed.shape[0] != 1:
        raise CapdecError("generate_text takes one caption ([1, P, d])")
    return _decode_texts(prefix_embed, tokenizer, model, use_beam)[0]


def re_caption(add_in: str, prefix_embed: torch.Tensor, tokenizer, model: ClipCaptionModel, where: int,
               use_beam: bool = True) -> str:
    """the caption after ``add_in`` was spliced into the prefix at ``where`` (reference :223-226)"""
    return generate_text(add_embedding_from_text(add_in, prefix_embed, tokenizer, model, where), tokenizer, model, use_beam)


def remove_token(prefix_embed: torch.Tensor, tokenizer, model: ClipCaptionModel, embeddings, where: List[int],
                 use_beam: bool = True):
    """reference :229-237 -> (text generated from the prefix without the positions ``where``, its prefix sentence)"""
    keep = [i for i in range(prefix_embed.shape[1]) if i not in where]
    shorter = prefix_embed[:, keep]
    ids, _ = _nearest(embeddings, shorter[0], 1, model)
    return generate_text(shorter, tokenizer, model, use_beam), tokenizer.decode(ids[:, 0].to(torch.int64).cpu())


def try_all_places(add_in: str, prefix_embed: torch.Tensor, tokenizer, model: ClipCaptionModel,
                   use_beam: bool = True) -> List[str]:
    """``re_caption`` at every position 0..P-1 (reference :240-244): the P edited prefixes form one [P, P + m, d] batch
    that ONE decode call serves.  Greedy: a TypeError naming the places whose first token stops, where ``re_caption``
    would raise for that place alone."""
    P = int(prefix_embed.shape[1])
    if P == 0:
        return []
    batch = torch.cat([add_embedding_from_text(add_in, prefix_embed, tokenizer, model, i) for i in range(P)], 0)
    return _decode_texts(batch, tokenizer, model, use_beam)
