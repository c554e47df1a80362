"""The AdamW update of the train step (``adam_prepare_kernel`` / ``adamw_multi_kernel``, csrc/train_optim.hip) and every
piece of state that has to follow it, against the float64 restatement in tests/adamw_def.py.

Protocol of one update (``Trajectory.step``).  The moments cannot be read from the device, so the test carries them:

  1. every tensor of the scope is read (``engine.mapper_parameters(model._train_shapes())``, every element);
  2. a probe ``train_step(apply_update=False)`` on the batch, every gradient read;
  3. the same batch with ``apply_update=True`` at ``lr_t``, every gradient read again: the arena the update consumed (the
     update does not write it, and ``capdec_train_get`` scales it by the same float32 product the kernel does).  The
     expectation is built from THESE gradients -- an entry whose gradient is smaller than the atomics noise between two
     runs has a probe gradient of the other sign now and then, and Adam turns a sign into 2 lr -- and the probe's
     gradients must lie within 1e-6 of the tensor's largest entry of them, at every step;
  4. every tensor is read again;
  5. ``p64' = adamw64(p_before, g_dev, m64, v64, t, lr_t, ...)`` with m64, v64 carried from the device's own gradients and
     ``t`` counting good updates only.

Bar: ``err_dev = max |p_dev' - p64'| / unit <= 4 max(e32, 4)`` per tensor and step, ``unit = ulp32(p64') / 2 + 2^-24 lr_t``,
``e32`` the same figure of the float32 run of the restatement (adamw_def.py).  Where ``lr_t == 0`` the tensors are
bit-identical.  The factor 4: FMA contraction, the step size applied after the division, float32 ``1 - beta``.
GPT-2's dropouts are 0 throughout.  Case E runs WITHOUT probes, so that the device's loss counter counts exactly the
good updates.

Geometry: d = 768 always (the train step refuses another width); one-layer GPT-2 of 1531 tokens and 32 positions, MLP mapper
at prefix_length 4 (full and frozen scope), one-layer TransformerMapper (clip_length 4, P 4, D 640; frozen scope), B = 2,
L = 5, ragged.  The host-only test restates the slot / chunk table and shows which kinds of slot the cases hold.

Measured figures: profiles/adamw_update.txt."""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import adamw_def as D                                     # noqa: E402
from capdec_amd import synth                              # noqa: E402
from capdec_amd.engine import Engine                      # noqa: E402


def _adamw_chunk():
    with open(os.path.join(ROOT, "capdec_amd", "csrc", "train.h")) as f:
        m = re.search(r"constexpr\s+int\s+ADAMW_CHUNK\s*=\s*(\d+)\s*;", f.read())
    assert m, "csrc/train.h no longer spells ADAMW_CHUNK as this test reads it"
    return int(m.group(1))


ADAMW_CHUNK = _adamw_chunk()
DIMS = synth.GPT2Dims(n_layer=1, vocab=1531, n_pos=32)
P, CLIP_LEN, D_MLP, D_TM, B, L = 4, 4, 512, 640, 2, 5
DEFAULTS = dict(betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0)
GRAD_REPEAT_TOL = 1e-6          # probe-to-update gradient difference, of the tensor's largest entry


def _shapes(mapping, full, prefix_length=P, dims=DIMS):
    """ordered {state-dict name: shape} of a scope, in the device's slot order (what ``model._train_shapes()`` returns)"""
    sd = _state_dict(mapping, prefix_length, dims)
    if mapping == "mlp":
        names = ["clip_project." + n for n in Engine.train_tensor_names("mlp")]
    else:
        names = ["clip_project." + n for n in Engine.train_tensor_names("transformer", 1)]
    if full:
        names += ["gpt." + n for n in Engine.train_gpt2_tensor_names(dims.n_layer)]
    return {n: tuple(sd[n].shape) for n in names}


@functools.lru_cache(maxsize=None)
def _state_dict(mapping, prefix_length=P, dims=DIMS):
    return synth.hot_state_dict(17, mapping, D_MLP if mapping == "mlp" else D_TM, prefix_length, CLIP_LEN, 1, dims)


# ------------------------------------------------------------------------------------------- host only
def test_slot_and_chunk_table_of_the_cases():
    """No GPU: the slot / chunk arithmetic of build_slots restated (one block per 16 384-element chunk of every tensor).
    The full-scope case holds all three kinds of slot -- shorter than a chunk, exactly k chunks, k chunks and a ragged
    last one -- and every chunk table covers every element exactly once.  Every trainable tensor of the cases is a
    multiple of 256 elements, so the kernel's 256-thread loop always ends on a whole pass there; with an ODD prefix_length
    the MLP mapper's first bias has 384 P elements -- whole wavefronts still (a partial wavefront cannot be reached at
    d = 768), but half a block in the last pass: the P = 3 case of test_case_a_frozen covers it."""
    assert ADAMW_CHUNK == 16384
    full = {k: int(np.prod(s)) for k, s in _shapes("mlp", True).items()}
    kinds = {k: D.slot_kind(n, ADAMW_CHUNK) for k, n in full.items()}
    assert kinds["gpt.transformer.h.0.ln_1.weight"] == "short" and full["gpt.transformer.h.0.ln_1.weight"] == 768
    assert kinds["gpt.transformer.h.0.attn.c_attn.bias"] == "short" and kinds["gpt.transformer.h.0.mlp.c_fc.bias"] == "short"
    assert kinds["gpt.transformer.h.0.attn.c_proj.weight"] == "whole" and full["gpt.transformer.h.0.attn.c_proj.weight"] == 36 * ADAMW_CHUNK
    assert kinds["gpt.transformer.wpe.weight"] == "ragged" and full["gpt.transformer.wpe.weight"] == ADAMW_CHUNK + ADAMW_CHUNK // 2
    assert kinds["gpt.transformer.wte.weight"] == "ragged" and full["gpt.transformer.wte.weight"] == 71 * ADAMW_CHUNK + 12544
    assert (full["clip_project.model.0.weight"], full["clip_project.model.2.weight"]) == (1536 * 512, 3072 * 1536)
    assert set(kinds.values()) == {"short", "whole", "ragged"}
    assert 13.5e6 < sum(full.values()) < 14.5e6
    for mapping, scope_full, pl in (("mlp", True, P), ("mlp", False, P), ("transformer_encoder", False, P), ("mlp", False, 3)):
        sizes = [int(np.prod(s)) for s in _shapes(mapping, scope_full, pl).values()]
        table = D.chunk_table(sizes, ADAMW_CHUNK)
        assert len(table) == sum(-(-n // ADAMW_CHUNK) for n in sizes)
        covered = [0] * len(sizes)
        for s, k, i0, i1 in table:
            assert i0 == k * ADAMW_CHUNK and i0 < i1 <= sizes[s] and i1 - i0 <= ADAMW_CHUNK
            covered[s] += i1 - i0
        assert covered == sizes
        assert all(n % 128 == 0 for n in sizes)                      # whole wavefronts at d = 768, whatever the geometry
        if pl % 2 == 0:
            assert all(n % 256 == 0 for n in sizes), (mapping, scope_full)
    frozen_tm = {D.slot_kind(int(np.prod(s)), ADAMW_CHUNK) for s in _shapes("transformer_encoder", False).values()}
    assert frozen_tm == {"short", "whole"}
    odd = {k: int(np.prod(s)) for k, s in _shapes("mlp", False, 3).items()}
    assert odd["clip_project.model.0.bias"] == 1152 and odd["clip_project.model.0.bias"] % 256 == 128


def test_definition_float32_run_stays_within_its_own_bar():
    """No GPU: the float32 run of the restatement against its float64 run over 24 steps of gradients spanning
    e^(-8 +- 4), four hyper-parameter sets -- every e32 below the refusal threshold, and a second float32 restatement in
    the kernel's operation order (numpy) within the bar the first one sets.  A wrong step count, decay before the update
    and a skipped entry are each far outside it."""
    gen = torch.Generator().manual_seed(3)
    n = 1 << 15
    sets = [dict(DEFAULTS, lr=1e-3), dict(betas=(0.9, 0.999), eps=1e-6, weight_decay=0.5, lr=1e-2),
            dict(betas=(0.5, 0.9), eps=1e-3, weight_decay=0.0, lr=1e-3), dict(betas=(0.0, 0.999), eps=1e-6, weight_decay=0.0, lr=1e-3)]
    for hp in sets:
        lr = hp["lr"]
        kw = {k: v for k, v in hp.items() if k != "lr"}
        p = torch.randn(n, generator=gen) * 0.1
        m64, v64 = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        m32, v32 = torch.zeros(n), torch.zeros(n)
        mk, vk = np.zeros(n, np.float32), np.zeros(n, np.float32)
        worst32 = worstk = 0.0
        for t in range(1, 25):
            g = torch.randn(n, generator=gen) * torch.exp(-8.0 + 4.0 * torch.randn(n, generator=gen))
            want = D.adamw(p.double(), g.double(), m64, v64, t, lr, **kw)
            got32 = D.adamw(p, g, m32, v32, t, lr, **kw)
            gotk = torch.from_numpy(_kernel_order_f32(p.numpy(), g.numpy(), mk, vk, t, lr, **kw))
            e32, ek = float(D.units_off(got32, want, lr).max()), float(D.units_off(gotk, want, lr).max())
            assert ek <= D.bar(e32), (hp, t, ek, e32)
            worst32, worstk = max(worst32, e32), max(worstk, ek)
            if t == 3:          # what the bar has to catch
                m_prev = (m64 - (1.0 - D.f32(kw["betas"][0])) * g.double()) / max(D.f32(kw["betas"][0]), 1e-30)
                v_prev = (v64 - (1.0 - D.f32(kw["betas"][1])) * g.double() ** 2) / D.f32(kw["betas"][1])
                if kw["betas"][0] > 0:                                                                           # a step count off by one
                    wrong = D.adamw(p.double(), g.double(), m_prev.clone(), v_prev.clone(), t + 1, lr, **kw)
                    assert float(D.units_off(wrong, want, lr).max()) > 1000.0, hp
                    if kw["weight_decay"] > 0:                                                                   # decay before the update
                        wrong = _decay_first(p.double(), g.double(), m_prev, v_prev, t, lr, **kw)
                        assert float(D.units_off(wrong, want, lr).max()) > 1000.0, hp
                assert float(D.units_off(p.double(), want, lr).max()) > 1000.0                                 # a skipped entry
            p = got32
        print(f"[adamw definition] {hp}: worst e32 {worst32:.2f} units, kernel-order float32 {worstk:.2f} units over 24 steps")
        assert worst32 <= 16.0 and worstk <= 16.0


def _kernel_order_f32(p, g, m, v, t, lr, betas, eps, weight_decay):
    """adamw_multi_kernel's arithmetic in numpy float32, operation by operation (m, v in place)"""
    lr, (b1, b2), eps, wd = D.abi(lr, betas, eps, weight_decay)
    f = np.float32
    step_size = f(lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))
    m[:] = m * f(b1) + g * (f(1.0) - f(b1))
    v[:] = v * f(b2) + g * g * (f(1.0) - f(b2))
    out = p - step_size * (m / (np.sqrt(v) + f(eps)))
    decay = f(lr) * f(wd)
    if decay > 0:
        out = out - decay * out
    return out.astype(np.float32)


def _decay_first(p, g, m, v, t, lr, betas, eps, weight_decay):
    """the misplaced decay: p shrinks BEFORE the Adam term is subtracted"""
    lr_, _, _, wd_ = D.abi(lr, betas, eps, weight_decay)
    return D.adamw(p - lr_ * wd_ * p, g, m.clone(), v.clone(), t, lr, betas, eps, 0.0)


# ------------------------------------------------------------------------------------------- batches, models
@functools.lru_cache(maxsize=None)
def _batch(seed, dim, vocab=DIMS.vocab, batch=B, length=L):
    """[batch, length] right-padded ragged captions (the first full, the others shorter), their mask and a prefix batch"""
    gen = torch.Generator().manual_seed(1000 + seed)
    tokens = torch.zeros(batch, length, dtype=torch.int64)
    for r in range(batch):
        n = length if r == 0 else max(1, length - 1 - r)
        tokens[r, :n] = torch.randint(1, vocab, (n,), generator=gen)
    return tokens, synth.synthetic_clip_embeddings(batch, dim, seed=50 + seed)


def _mask(prefix_length, tokens):
    return torch.cat((torch.ones(tokens.shape[0], prefix_length), (tokens != 0).float()), dim=1)


def _model(mapping, full, prefix_length=P, dims=DIMS, num_layers=1):
    from capdec_amd.gpt2_prefix import ClipCaptionModel, ClipCaptionPrefix, MappingType
    cls = ClipCaptionModel if full else ClipCaptionPrefix
    mt = MappingType.MLP if mapping == "mlp" else MappingType.TransformerEncoder
    m = cls(prefix_length, clip_length=CLIP_LEN if mapping != "mlp" else prefix_length, prefix_size=D_MLP if mapping == "mlp" else D_TM,
            num_layers=num_layers, mapping_type=mt, gpt2_dims=dims).to("cuda:0")
    m.load_state_dict(_state_dict(mapping, prefix_length, dims))
    m.train()
    m.gpt.config.resid_pdrop = m.gpt.config.embd_pdrop = m.gpt.config.attn_pdrop = 0.0
    m._train_gpt = full
    m.engine.train_set_scope(full)
    return m


def _report(line):
    from tests.test_hip_parity import _report as report
    report(line)


class Trajectory:
    """the test's own copy of the optimizer state of one model: float64 (and float32) moments from the device's gradients,
    and the count of good updates"""

    def __init__(self, tag, model, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, probes=True):
        from capdec_amd import train as Tr
        self.tag, self.model, self.probes = tag, model, probes
        self.hp = dict(betas=betas, eps=eps, weight_decay=weight_decay)
        self.opt = Tr.AdamW(model.parameters(), lr=lr, **self.hp)
        self.prefix_length = model.prefix_length
        self.dim = model.prefix_dim
        self.worst = {}                 # slot kind -> (err_dev, e32, bar) of the entry nearest its bar
        self.grad_repeat = 0.0
        self.losses = []                # of the updates, in order (the length counts them across fresh())
        self.fresh()

    def fresh(self):
        """a new optimizer: zero moments, no update yet"""
        self.t, self.m64, self.v64, self.m32, self.v32 = 0, None, None, None, None

    def read(self):
        """every tensor of the scope, every element, as one flat float32 host vector (+ the names and sizes)"""
        got = self.model.engine.mapper_parameters(self.model._train_shapes())
        names = list(got)
        return names, [got[k].numel() for k in names], torch.cat([got[k].flatten() for k in names]).cpu()

    def _grads(self, names):
        from capdec_amd import train as Tr
        got = Tr.all_gradients(self.model)
        assert list(got) == names
        return torch.cat([got[k].flatten() for k in names]).cpu()

    def step(self, seed, lr_t, expect_t=None):
        from capdec_amd import train as Tr
        tokens, prefix = _batch(seed, self.dim)
        mask = _mask(self.prefix_length, tokens)
        names, sizes, before = self.read()
        self.opt.param_groups[0]["lr"] = lr_t
        if self.probes:
            Tr.train_step(self.model, self.opt, tokens, mask, prefix, apply_update=False)
            g_probe = self._grads(names)
        self.losses.append(Tr.train_step(self.model, self.opt, tokens, mask, prefix, apply_update=True))
        g = self._grads(names)
        _, _, after = self.read()
        if self.m64 is None:
            n = before.numel()
            self.m64, self.v64 = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
            self.m32, self.v32 = torch.zeros(n), torch.zeros(n)
        self.t += 1
        assert expect_t is None or self.t == expect_t
        want = D.adamw(before.double(), g.double(), self.m64, self.v64, self.t, lr_t, **self.hp)
        got32 = D.adamw(before, g, self.m32, self.v32, self.t, lr_t, **self.hp)
        u32, udev = D.units_off(got32, want, lr_t), D.units_off(after, want, lr_t)
        failures, o = [], 0
        for k, n in zip(names, sizes):
            sl = slice(o, o + n)
            o += n
            e32, err = float(u32[sl].max()), float(udev[sl].max())
            bar = D.bar(e32)
            kind = D.slot_kind(n, ADAMW_CHUNK)
            if kind not in self.worst or err / bar > self.worst[kind][0] / self.worst[kind][2]:
                self.worst[kind] = (err, e32, bar, k, self.t)
            if self.probes:
                scale = float(g[sl].abs().max())
                rep = float((g_probe[sl] - g[sl]).abs().max()) / scale if scale > 0 else 0.0
                self.grad_repeat = max(self.grad_repeat, rep)
                if rep >= GRAD_REPEAT_TOL:
                    failures.append((k, "probe gradient", rep))
            if D.f32(lr_t) == 0.0 and not torch.equal(before[sl], after[sl]):
                failures.append((k, "moved at lr = 0", float((before[sl] - after[sl]).abs().max())))
            if not err <= bar:
                bad = int((udev[sl] > bar).sum())
                failures.append((k, f"t={self.t} lr={lr_t:g}", f"err_dev {err:.1f} units > bar {bar:.1f} (e32 {e32:.1f}); {bad}/{n} entries"))
        assert not failures, (self.tag, failures[:8])
        if D.f32(lr_t) != 0.0:          # the update really moved the weights (nothing of the above holds trivially)
            assert float((after - before).abs().max()) > 0.25 * D.f32(lr_t), (self.tag, self.t)
        return before, after

    def report(self):
        for kind in ("short", "whole", "ragged"):
            if kind in self.worst:
                err, e32, bar, k, t = self.worst[kind]
                _report(f"[adamw update] {self.tag}: {kind:6s} slots: worst err_dev {err:6.2f} units, e32 {e32:5.2f}, bar {bar:5.1f} "
                        f"({k}, t = {t})")
        if self.probes:
            _report(f"[adamw update] {self.tag}: {len(self.losses)} updates; probe-to-update gradient difference <= {self.grad_repeat:.2e} "
                    f"of the tensor's largest entry")


def _run_schedule(traj, lr, warmup, total, steps, seed0=0):
    for k in range(steps):
        traj.step(seed0 + k, D.schedule_lr(lr, k, warmup, total), expect_t=k + 1)


# ------------------------------------------------------------------------------------------- A .. F
@pytest.mark.gpu
def test_gradient_reads_repeat():
    """Once per file: the same probe twice, every gradient of the full scope -- the largest difference between the two reads
    (the order of the atomics) stays below 1e-6 of the tensor's largest entry"""
    from capdec_amd import train as Tr
    model = _model("mlp", True)
    try:
        tokens, prefix = _batch(0, D_MLP)
        opt = Tr.AdamW(model.parameters(), lr=1e-3)
        reads = []
        for _ in range(2):
            Tr.train_step(model, opt, tokens, _mask(P, tokens), prefix, apply_update=False)
            reads.append({k: v.cpu() for k, v in Tr.all_gradients(model).items()})
        worst, worst_k = 0.0, ""
        for k in reads[0]:
            rel = float((reads[0][k] - reads[1][k]).abs().max()) / float(reads[0][k].abs().max())
            if rel > worst:
                worst, worst_k = rel, k
        _report(f"[adamw update] probe-to-probe gradient difference, full scope, {len(reads[0])} tensors: {worst:.2e} of the tensor's "
                f"largest entry ({worst_k or 'bit-identical'})")
        assert worst < GRAD_REPEAT_TOL
    finally:
        model.release()


@pytest.mark.gpu
def test_case_a_full_scope_defaults_with_the_reference_schedule():
    """A: full scope (about 14 M parameters: slots shorter than a chunk, of exactly k chunks, with a ragged last chunk),
    lr 1e-3, warm-up 2 of 8 steps, 6 steps; step 0 has lr = 0: no weight moves, the moments and t advance"""
    model = _model("mlp", True)
    try:
        kinds = {D.slot_kind(int(np.prod(s)), ADAMW_CHUNK) for s in model._train_shapes().values()}
        assert kinds == {"short", "whole", "ragged"} and list(model._train_shapes()) == list(_shapes("mlp", True))
        traj = Trajectory("A full scope, lr 1e-3, warm-up 2 of 8", model, 1e-3)
        assert D.schedule_lr(1e-3, 0, 2, 8) == 0.0
        _run_schedule(traj, 1e-3, 2, 8, 6)
        traj.report()
    finally:
        model.release()


@pytest.mark.gpu
@pytest.mark.parametrize("mapping,prefix_length", [("mlp", P), ("transformer_encoder", P), ("mlp", 3)],
                         ids=["mlp", "transformer_mapper", "mlp_P3"])
def test_case_a_frozen(mapping, prefix_length):
    """A: frozen scope with both mappers, the same schedule, 6 steps.  mlp_P3: the odd prefix_length whose first bias (1152
    elements) ends the kernel's loop on half a block"""
    model = _model(mapping, False, prefix_length)
    try:
        traj = Trajectory(f"A frozen scope, {mapping} P = {prefix_length}, lr 1e-3, warm-up 2 of 8", model, 1e-3)
        _run_schedule(traj, 1e-3, 2, 8, 6)
        traj.report()
    finally:
        model.release()


@pytest.mark.gpu
def test_case_b_weight_decay():
    """B: lr 1e-2, weight_decay 0.5, 4 steps, full scope, an lr = 0 step in the middle (decay = lr wd: nothing moves).
    Decay before the update instead of after it differs by lr^2 wd = 5e-5 per step: more than 1e4 units.  The decay is also
    what moves the rows of wpe no batch reaches (S = 9 of 32 positions: their gradient is 0) -- the ragged last chunk of
    that slot is checked here; wte's ragged chunk moves in every full-scope case (the lm_head reaches every row)."""
    model = _model("mlp", True)
    try:
        traj = Trajectory("B full scope, lr 1e-2, weight_decay 0.5", model, 1e-2, weight_decay=0.5)
        for k, lr_t in enumerate((1e-2, 1e-2, 0.0, 1e-2)):
            traj.step(10 + k, lr_t, expect_t=k + 1)
        traj.report()
    finally:
        model.release()


@pytest.mark.gpu
@pytest.mark.parametrize("betas,eps", [((0.5, 0.9), 1e-3), ((0.0, 0.999), 1e-6)], ids=["b0.5-0.9-eps1e-3", "b0-0.999-eps1e-6"])
def test_case_c_other_moments(betas, eps):
    """C: frozen scope (MLP mapper), 4 steps at lr 1e-3: (0.5, 0.9, 1e-3), where eps dominates small gradients, and
    (0.0, 0.999, 1e-6), where the bias correction meets pow(0, t)"""
    model = _model("mlp", False)
    try:
        traj = Trajectory(f"C frozen scope, betas {betas}, eps {eps:g}", model, 1e-3, betas=betas, eps=eps)
        for k in range(4):
            traj.step(20 + k, 1e-3, expect_t=k + 1)
        traj.report()
    finally:
        model.release()


@pytest.mark.gpu
def test_case_d_long_run():
    """D: frozen scope, TransformerMapper, 24 steps, defaults, warm-up 2 of 24: the device's counter against the test's t,
    and the drift of the float32 moments against the float64 ones"""
    model = _model("transformer_encoder", False)
    try:
        traj = Trajectory("D frozen scope, TransformerMapper, 24 steps, warm-up 2 of 24", model, 1e-3)
        _run_schedule(traj, 1e-3, 2, 24, 24, seed0=30)
        traj.report()
    finally:
        model.release()


@pytest.mark.gpu
def test_case_e_bad_step_in_the_middle():
    """E: full scope, 5 good updates; between the second and the third a step whose device-resident tokens hold an id
    >= vocab: IndexError, every tensor bit-identical; updates 3 to 5 meet the bar with t = 3, 4, 5 and the moments carried
    over -- the bad step added nothing to them; the loss counter counts 5 and its sum is the sum of the 5 good losses.
    No probes here: every train_step of this case is an update."""
    from capdec_amd import train as Tr
    model = _model("mlp", True)
    try:
        traj = Trajectory("E full scope, a bad step after update 2", model, 1e-3, probes=False)
        for k in range(2):
            traj.step(40 + k, 1e-3, expect_t=k + 1)
        tokens, prefix = _batch(47, D_MLP)
        bad = tokens.clone()
        bad[1, 1] = DIMS.vocab + 7
        _, _, before = traj.read()
        with pytest.raises(IndexError):
            Tr.train_step(model, traj.opt, bad.cuda(), _mask(P, tokens), prefix)
        _, _, after = traj.read()
        assert torch.equal(before, after)
        for k in range(2, 5):
            traj.step(40 + k, 1e-3, expect_t=k + 1)
        last, total, n = model.engine.train_loss()
        want = float(np.sum(np.asarray(traj.losses, dtype=np.float64)))
        # (four float32 additions, each within half a float32 spacing of the running sum)
        assert n == 5 and len(traj.losses) == 5 and abs(last - traj.losses[-1]) == 0.0 and np.isfinite(total)
        assert abs(total - want) <= 4 * float(np.spacing(np.float32(want))), (total, want)
        traj.report()
        _report(f"[adamw update] E: loss counter {n} steps, sum {total:.6f} (the 5 good losses: {want:.6f})")
    finally:
        model.release()


@pytest.mark.gpu
def test_case_f_fresh_state():
    """F: frozen scope (TransformerMapper).  Two updates; the same scope set again: update 3 meets the bar with t = 3
    (nothing was reset); after train_reset(): t = 1 and zero moments from the current weights; after a scope switch
    frozen -> full (one full-scope update) -> frozen: t = 1 and zero moments again."""
    model = _model("transformer_encoder", False)
    try:
        eng = model.engine
        traj = Trajectory("F frozen scope, TransformerMapper", model, 1e-3)
        traj.step(60, 1e-3, expect_t=1)
        traj.step(61, 1e-3, expect_t=2)
        eng.train_set_scope(False)
        traj.step(62, 1e-3, expect_t=3)
        eng.train_reset()
        traj.fresh()
        traj.step(63, 1e-3, expect_t=1)
        traj.step(64, 1e-3, expect_t=2)
        tokens, prefix = _batch(65, D_TM)
        eng.train_set_scope(True)
        loss = eng.train_step(prefix, tokens, 1e-3)             # one full-scope update: moments of another parameter set
        assert np.isfinite(loss)
        eng.train_set_scope(False)
        traj.fresh()
        traj.step(66, 1e-3, expect_t=1)
        traj.step(67, 1e-3, expect_t=2)
        traj.report()
    finally:
        model.release()


# ------------------------------------------------------------------------------------------- G
G_DIMS, G_P, G_LR, G_UPDATES = synth.GPT2_TINY, 10, 1e-2, 3
G_STOP, G_T, G_BEAM = G_DIMS.vocab + 5, 8, 5
LOGITS_TOL, SCORE_TOL, TIE = 2e-4, 3e-4, 1e-4
G_SEED = 5


@functools.lru_cache(maxsize=None)
def _g_inputs():
    gen = torch.Generator().manual_seed(G_SEED)
    embeds = torch.randn(3, 14, G_DIMS.n_embd, generator=gen) * 0.3                  # gpt2_logits: fixed embeddings
    x = synth.synthetic_clip_embeddings(4, D_MLP, seed=G_SEED)                       # mapper_forward, and the decodes' prefixes
    cap = torch.randint(1, G_DIMS.vocab, (4, 6), generator=gen)                      # score: 4 short captions
    cap_lens = np.array([6, 3, 5, 1])
    train = [_batch(70 + k, D_MLP, G_DIMS.vocab, 4, 8) for k in range(G_UPDATES + 1)]
    return embeds, x, cap, cap_lens, train


def _g_oracle(sd):
    """everything step 1 / step 4 calls, from the oracle at the weights ``sd``"""
    import score_def
    from oracle import capdec_oracle as O
    embeds, x, cap, cap_lens, _ = _g_inputs()
    nh = G_DIMS.n_head
    out = {"logits": O.gpt2_logits(embeds, sd, nh)}
    with O.bf16_gemm_operands():
        out["logits_bf16"] = O.gpt2_logits(embeds, sd, nh)
    pe = O.clip_project(x, sd, "mlp", G_P).reshape(4, G_P, -1)
    out["pe"] = pe
    out["greedy"], out["greedy_margin"] = [], []
    for r in range(4):
        mg = []
        out["greedy"].append(O.generate2_ref(sd, pe[r:r + 1], G_STOP, G_T, n_head=nh, margins=mg))
        out["greedy_margin"].append(min(mg))
    out["beam"] = [O.generate_beam_ref(sd, pe[r:r + 1], G_BEAM, G_STOP, G_T, n_head=nh) for r in range(4)]
    mg = []
    O.beam_cached(sd, pe, G_BEAM, G_STOP, G_T, n_head=nh, margins=mg)
    out["beam_margin"] = mg[0]
    lg = O.gpt2_logits(torch.cat((pe, O.wte(cap[:, :-1], sd)), dim=1), sd, nh)[:, G_P - 1:].numpy()
    out["logp"] = score_def.score(lg, cap.numpy(), cap_lens)[0]
    return out


def _g_device(model):
    """the calls of step 1 / step 4 on the device: f16x2 logits, greedy, beam, score, mapper; bf16 logits; back to f16x2"""
    embeds, x, cap, cap_lens, _ = _g_inputs()
    eng = model.engine
    assert eng.gemm_mode() == "f16x2"
    out = {"logits": eng.gpt2_logits(embeds).cpu()}
    pe = eng.mapper_forward(x).reshape(4, G_P, -1)
    out["pe"] = pe.cpu()
    ids, lens = eng.decode_greedy(pe, G_STOP, G_T)
    out["greedy"] = [ids[r, :int(lens[r])].cpu().tolist() for r in range(4)]
    out["beam"] = tuple(t.cpu() for t in eng.decode_beam(pe, G_STOP, G_BEAM, G_T))
    out["logp"] = eng.score(pe, cap, cap_lens)[0].cpu().numpy()
    eng.set_gemm_mode("bf16")
    try:
        out["logits_bf16"] = eng.gpt2_logits(embeds).cpu()
    finally:
        eng.set_gemm_mode("f16x2")
    return out


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


def _g_compare(tag, got, want):
    """the bars each path already has in this suite; returns the figures.  Ids are compared with the suite's near-tie
    allowance: a caption may differ only where the oracle's own margin drops below 1e-4 at some step"""
    fig = {"logits": float((got["logits"] - want["logits"]).abs().max()), "mapper": float((got["pe"] - want["pe"]).abs().max())}
    assert fig["logits"] <= LOGITS_TOL and fig["mapper"] <= 2e-4, (tag, fig)
    gap = _rms(want["logits_bf16"] - want["logits"])                        # what bf16 operands cost against fp32
    fig["bf16_gap"], fig["bf16"], fig["bf16_vs_f32"] = gap, _rms(got["logits_bf16"] - want["logits_bf16"]), _rms(got["logits_bf16"] - want["logits"])
    assert gap > 3e-3 and fig["bf16"] < gap and 0.3 * gap < fig["bf16_vs_f32"] < 1.5 * gap, (tag, fig)
    tied = 0
    for r in range(4):
        if got["greedy"][r] != want["greedy"][r]:
            assert want["greedy_margin"][r] < TIE, (tag, r, got["greedy"][r], want["greedy"][r])
            tied += 1
        tok, sl, sc, order = want["beam"][r]
        ids, lens, scores, ordr = (t[r] for t in got["beam"])
        same = (torch.equal(ordr.long(), order) and torch.equal(ids.long(), tok[order]) and torch.equal(lens.float(), sl[order])
                and float((scores - sc[order]).abs().max()) <= 1e-4)
        if not same:
            assert float(want["beam_margin"][r]) < TIE, (tag, r, ids, tok[order])
            tied += 1
    fig["tied"] = tied
    ok = np.isfinite(want["logp"])
    fig["logp"] = float(np.abs(got["logp"] - want["logp"])[ok].max())
    assert fig["logp"] <= SCORE_TOL, (tag, fig)
    return fig


@pytest.mark.gpu
def test_case_g_nothing_stale_after_full_scope_updates():
    """G: the tiny GPT-2 (2 layers) with an MLP mapper at P = 10.  Every cache is warmed at the initial weights W0 -- f16x2
    planes (logits, greedy, beam, score, mapper), bf16 planes (logits) -- then three full-scope updates at lr 1e-2 move every
    matrix by at least 2 % of its largest entry, and every call is repeated WITHOUT reloading anything and compared with
    the oracle at W1 under the bar that path already has.  The oracle alone shows that a stale answer could not pass: its
    logits at W0 and W1 are at least 100 bars apart and its greedy ids differ for at least 3 of 4 captions.  Then the next
    gradient at W1 against the float64 oracle, entry by entry, under the bar of tests/test_train_attention_forms.py --
    and the oracle's gradients at W0 and W1 are at least 100 bars apart for every mapper tensor, so dX through a 2 % stale
    transposed copy could not pass either."""
    from capdec_amd import train as Tr
    from oracle import capdec_oracle as O
    from tests import test_train_attention_forms as TA
    model = _model("mlp", True, G_P, G_DIMS, num_layers=8)
    try:
        *_, train = _g_inputs()
        W0 = {k: v.clone() for k, v in model.state_dict().items()}
        ref0 = _g_oracle(W0)
        f0 = _g_compare("W0", _g_device(model), ref0)                                         # (1) every cache is warm, and right
        opt = Tr.AdamW(model.parameters(), lr=G_LR)
        for k in range(G_UPDATES):                                                            # (2)
            tokens, prefix = train[k]
            Tr.train_step(model, opt, tokens, _mask(G_P, tokens), prefix)
        W1 = model.state_dict()                                                               # (3)
        moved = {}
        for k, w0 in W0.items():
            if w0.dim() == 2 and k != "gpt.lm_head.weight":
                moved[k] = float((W1[k] - w0).abs().max()) / float(w0.abs().max())
        assert len(moved) == 2 + 4 * G_DIMS.n_layer + 2 and min(moved.values()) >= 0.02, sorted(moved.items(), key=lambda kv: kv[1])[:3]
        ref1 = _g_oracle(W1)                                                                  # (5) from the oracle alone
        sep_logits = float((ref1["logits"] - ref0["logits"]).abs().max())
        sep_bf16 = _rms(ref1["logits_bf16"] - ref0["logits_bf16"]) / _rms(ref1["logits_bf16"] - ref1["logits"])
        sep_ids = sum(a != b for a, b in zip(ref0["greedy"], ref1["greedy"]))
        sep_logp = float(np.nanmax(np.abs(ref1["logp"] - ref0["logp"])))
        sep_pe = float((ref1["pe"] - ref0["pe"]).abs().max())
        assert sep_logits >= 100 * LOGITS_TOL and sep_ids >= 3 and sep_bf16 >= 10.0 and sep_logp >= 100 * SCORE_TOL and sep_pe >= 100 * 2e-4, \
            (sep_logits, sep_ids, sep_bf16, sep_logp, sep_pe)
        f1 = _g_compare("W1", _g_device(model), ref1)                                         # (4) nothing reloaded
        _report(f"[adamw update] G: weight movement over {len(moved)} matrices: min {min(moved.values()):.3f}, max {max(moved.values()):.3f} "
                f"of the largest entry; oracle W0/W1 separation: logits {sep_logits:.3f} ({sep_logits / LOGITS_TOL:.0f} bars), greedy ids "
                f"{sep_ids} of 4 captions, bf16 logits {sep_bf16:.1f} class gaps, logp {sep_logp:.3f}, mapper {sep_pe:.3f}")
        for tag, f in (("W0", f0), ("W1", f1)):
            _report(f"[adamw update] G at {tag}: logits {f['logits']:.2e} (bar {LOGITS_TOL:g}), mapper {f['mapper']:.2e}, bf16 logits rms "
                    f"{f['bf16']:.2e} (class gap {f['bf16_gap']:.2e}), logp {f['logp']:.2e} (bar {SCORE_TOL:g}), "
                    f"{f['tied']} of 8 decodes differ on a near-tie")
        # (6) the next gradient, at W1
        tokens, prefix = train[G_UPDATES]
        kw = dict(n_head=G_DIMS.n_head, train_gpt=True)
        ref = TA.references(W1, tokens, prefix, "mlp", G_P, G_DIMS, G_P, True, None)
        _, g0 = O.train_step_loss_and_grads({k: v.double() for k, v in W0.items()}, tokens, prefix.double(), "mlp", G_P, **kw)
        loss64, g64, e32 = ref
        seps = {}
        for k in g64:
            if k.startswith("clip_project."):
                bar = TA.FACTOR * max(e32[k], TA.E32_FLOOR)
                seps[k] = float((g0[k] - g64[k]).abs().max()) / float(g64[k].abs().max()) / bar
        assert len(seps) == 4 and min(seps.values()) >= 100.0, seps
        loss = Tr.train_step(model, opt, tokens, _mask(G_P, tokens), prefix, apply_update=False)
        TA.compare("adamw update G: the gradient at W1", loss, Tr.all_gradients(model), ref)
        _report(f"[adamw update] G: oracle gradient W0/W1 separation of the mapper's tensors: {min(seps.values()):.0f} to "
                f"{max(seps.values()):.0f} bars")
    finally:
        model.release()
