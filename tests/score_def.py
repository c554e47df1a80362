"""The scoring contract of ``capdec_score``, restated in fp64 numpy -- what tests/test_score.py checks the HIP path against.

Caption r has prefix rows ``prefix[r]`` [P, d], token ids ``tok[r, 0..L)`` and a length ``len[r]`` in 0..L.  The model input
is ``cat(prefix[r], wte(tok[r, :len[r]-1])) + wpe``, and for ``i < len[r]``

    logp[r, i] = s[tok[r, i]] - logsumexp(s),   s = logits at position P-1+i, divided by the temperature

(``logits[:, P-1:-1]`` against ``tokens`` of reference train.py:349).  Positions ``i >= len[r]`` get 0.  A label equal to
``ignore_id`` gets 0 and is not counted (``ignore_id = -1``: none).  ``sum[r]`` / ``count[r]`` run over the counted
positions.  An id outside [0, V) is never looked up: as a label it gives NaN at its position; as an input (``i < len[r]-1``)
it makes every later position of the caption NaN.

The functions take the logits of the scored positions, ``logits[r, i]`` = the model's logits at position ``P-1+i``
(``O.train_forward(...)[:, P-1:]``), so they restate the definition and nothing of the model.
"""
import numpy as np


def log_softmax(logits, temperature=1.0):
    s = np.asarray(logits, dtype=np.float64) / (temperature if temperature > 0 else 1.0)
    m = s.max(axis=-1, keepdims=True)
    return s - (m + np.log(np.exp(s - m).sum(axis=-1, keepdims=True)))


def score(logits, tokens, lens=None, ignore_id=-1, temperature=1.0):
    """logits [n, >= L, V] (position P-1+i at index i), tokens [n, L], lens [n] or None (all L) ->
    (logp fp64 [n, L], sum fp64 [n], count int64 [n], top1 int64 [n, L] -- 0 past lens)"""
    tokens = np.asarray(tokens).astype(np.int64)
    n, L = tokens.shape
    V = logits.shape[-1]
    lens = np.full(n, L, dtype=np.int64) if lens is None else np.asarray(lens).astype(np.int64)
    assert ((lens >= 0) & (lens <= L)).all()
    logp = np.zeros((n, L), dtype=np.float64)
    top1 = np.zeros((n, L), dtype=np.int64)
    ssum = np.zeros(n, dtype=np.float64)
    count = np.zeros(n, dtype=np.int64)
    for r in range(n):
        tainted = False                                  # an input id outside the vocabulary fed an earlier position
        for i in range(int(lens[r])):
            row = np.asarray(logits[r, i], dtype=np.float64)
            top1[r, i] = int(row.argmax())
            t = int(tokens[r, i])
            outside = t < 0 or t >= V
            if not (ignore_id != -1 and t == ignore_id):
                logp[r, i] = np.nan if (tainted or outside) else log_softmax(row, temperature)[t]
                ssum[r] += logp[r, i]
                count[r] += 1
            tainted = tainted or outside                 # (it is the input of position i + 1)
    return logp, ssum, count, top1


def mean_nll(ssum, count):
    """-sum(logp) / count over all captions: the train loss of reference train.py:349 when ignore_id = 0 and lens = L"""
    return -float(np.sum(ssum)) / float(np.sum(count))
