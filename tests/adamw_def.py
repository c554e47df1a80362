"""The AdamW update of the train step, restated in float64 -- what tests/test_adamw_update.py checks
``adam_prepare_kernel`` / ``adamw_multi_kernel`` (csrc/train_optim.hip) against.

The rule is transformers-4.24 ``AdamW.step`` (``oracle.capdec_oracle.adamw_transformers``, run here on float64 tensors):

    m <- b1 m + (1 - b1) g          v <- b2 v + (1 - b2) g g
    p <- p - lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps)
    p <- p - lr wd p                (only when wd > 0: after the update, with the uncorrected lr)

with ``t`` = 1 for the first update, and the learning rate of update k (k = 0, 1, ...) is
``lr * linear_schedule_with_warmup(k, warmup, total)`` (reference train.py:329-331,351-352: the optimizer steps before the
scheduler, so the first update of a run with a warm-up has lr = 0: it moves no weight, but it advances m, v and t).

Hyper-parameters as the C ABI receives them.  ``capdec_train_step`` takes ``lr``, ``beta1``, ``beta2``, ``eps`` and
``weight_decay`` as C floats, so the restatement rounds each of them to float32 FIRST and then uses the rounded value as a
double (``abi``).  With the exact doubles instead (0.9 for 0.899999976..., 1e-6 for 9.99999997e-7) an entry whose gradient
is near eps / sqrt(1 - b2) -- where neither sqrt(v) nor eps dominates the denominator -- differs by up to about 70 of the
units below (measured on the CPU; about 4e-6 lr: harmless for training, but it would swamp the bar).

The unit of every comparison is ``unit = ulp32(p') / 2 + 2^-24 lr`` per entry, p' the float64 result: half a float32
spacing at the result (the one rounding no float32 update can avoid) plus the rounding of the float32 step size.

``e32`` is what the SAME rule costs in float32: torch CPU float32 ops, float32 moments, from the same ``p`` (teacher
forced), against the float64 run, in those units.  A device result passes when ``err <= 4 max(e32, 4)``; a reference run
whose own e32 exceeds 64 units is refused.
"""
import numpy as np
import torch

from oracle import capdec_oracle as O

FACTOR, E32_FLOOR, E32_REFUSE = 4.0, 4.0, 64.0


def f32(x):
    """a Python float as the C ABI hands it to the kernels: rounded to float32, then widened again"""
    return float(np.float32(x))


def abi(lr, betas, eps, weight_decay):
    return f32(lr), (f32(betas[0]), f32(betas[1])), f32(eps), f32(weight_decay)


def schedule_lr(lr, k, warmup, total):
    """the learning rate of update k (0-based) under get_linear_schedule_with_warmup"""
    return lr * O.linear_schedule_with_warmup(k, warmup, total)


def adamw(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0):
    """one update at the tensors' own dtype (float64: the definition; float32: the e32 run): returns p', updates m and v in
    place.  ``t`` counts from 1."""
    lr, betas, eps, weight_decay = abi(lr, betas, eps, weight_decay)
    out = p.clone()
    O.adamw_transformers(out, g.to(p.dtype), m, v, t, lr, betas, eps, weight_decay)
    return out


def ulp32(x):
    """float32 spacing at |x| (x a float64 tensor): 2^(exponent - 23), the subnormal spacing 2^-149 at and near 0"""
    _, e = torch.frexp(x)                                  # |x| = m 2^e, m in [0.5, 1): floor(log2 |x|) = e - 1
    return torch.ldexp(torch.ones_like(x), (e - 24).clamp(min=-149))


def unit(p64_new, lr):
    return 0.5 * ulp32(p64_new) + 2.0 ** -24 * f32(lr)


def units_off(got, p64_new, lr):
    """|got - p64'| / unit, entry by entry (got: a float32 or float64 tensor)"""
    return (got.double() - p64_new).abs() / unit(p64_new, lr)


def bar(e32):
    assert e32 <= E32_REFUSE, f"the float32 run of the reference is itself {e32:.1f} units from float64: not a bar"
    return FACTOR * max(e32, E32_FLOOR)


# ---- the slot / chunk table of build_slots (csrc/train_optim.hip), restated
def chunk_table(sizes, chunk):
    """[(slot, chunk within the slot, first element, one past the last)] for the tensors' element counts, in slot order"""
    table = []
    for s, n in enumerate(sizes):
        k = 0
        while k * chunk < n:
            table.append((s, k, k * chunk, min(n, (k + 1) * chunk)))
            k += 1
    return table


def slot_kind(n, chunk):
    """'short' (less than one chunk), 'whole' (exactly k chunks) or 'ragged' (k chunks and a shorter last one)"""
    return "short" if n < chunk else ("whole" if n % chunk == 0 else "ragged")
