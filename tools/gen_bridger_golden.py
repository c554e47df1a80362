#!/usr/bin/env python
"""Generate tests/golden/bridger.npz: what the REFERENCE's ``others/supervised_embedding_bridger.py`` returns, logs and saves
on seeded synthetic embeddings (build container only: the reference is imported from its checkout with an empty ``wandb``
stand-in, as tools/gen_gap_golden.py does).  Only inputs and results are written -- numbers, never reference source.

  (a) ``a_*``  its ``get_dataloader()`` on a pickle of 61 captions over 20 image ids in scrambled order: the raw rows, the
               image ids, the captions' row indices, and the four tensors it returns.
  (b) ``b_*``  two epochs of 13 rows in batches of 5 with its own ``MLP(36, 44, 28, 4)`` (seeded random weights), its
               ``get_torch_dataloader_from_list``, ``MSELoss`` and ``SGD(lr=0.05, momentum=0.9)``: the state dict before the
               first and after every step, every loss, the outputs in eval mode and the eval losses per batch.
  (c) ``c_*``  its ``train_modal()`` itself (wandb.init / wandb.log recorded) on a pickle of 101 rows at width 640: the
               train_loss and val_loss of all 100 epochs, the initial and the final biases, the first 8 rows of every final
               weight matrix.

``floor_*`` = max |reference - fp64 definition| (tests/bridger_def.py) with the definition advanced in lock-step on the same
inputs and with torch's own ReLU masks (read by forward hooks).  The generator also runs the definition with its OWN masks
and asserts that it stays inside 4 floor + 2.4e-7 max |value|: the CPU tests do that run.

usage: python tools/gen_bridger_golden.py
"""
from __future__ import annotations

import contextlib
import importlib.util
import io
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bridger_def as D       # noqa: E402

REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "bridger.npz")
PICKLE = 'coco_clip_embeddings/oscar_split_RN50x4_train_with_text_embeddings.pkl'


def import_reference():
    wandb = types.ModuleType("wandb")
    wandb.records = []
    wandb.init = lambda *a, **k: None
    wandb.log = lambda d: wandb.records.append(dict(d))
    sys.modules["wandb"] = wandb
    spec = importlib.util.spec_from_file_location("ref_supervised_embedding_bridger",
                                                  os.path.join(REF, "others", "supervised_embedding_bridger.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref, wandb


def make_pickle(rng, n, dim, ids):
    """n + 1 captions and rows (the reference drops the last of each): scrambled image ids and row indices"""
    images = (rng.normal(0.0, 1.0, (n + 1, dim)) * rng.uniform(2.0, 9.0, (n + 1, 1))).astype(np.float16)
    texts = (images.astype(np.float64) * 0.3 + rng.normal(0.0, 1.0, (n + 1, dim))).astype(np.float16)
    image_ids = rng.integers(1000, 1000 + ids, n + 1)
    index = rng.permutation(n)                           # caption i -> row index[i]; the dropped caption points at row 0
    index = np.concatenate([index, [0]])
    captions = [{"image_id": int(image_ids[i]), "clip_embedding": int(index[i]), "caption": f"c{i}"} for i in range(n + 1)]
    return {"captions": captions, "clip_embedding": torch.from_numpy(images), "clip_embedding_text_dave": torch.from_numpy(texts)}, \
        images, texts, image_ids, index


@contextlib.contextmanager
def in_temp_dir(data):
    old = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, os.path.dirname(PICKLE)))
        with open(os.path.join(tmp, PICKLE), "wb") as f:
            pickle.dump(data, f)
        os.chdir(tmp)
        try:
            yield tmp
        finally:
            os.chdir(old)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def params_of(model):
    return [p.detach().numpy().copy() for p in model.parameters()]          # w0, b0, w1, b1, ...


def def_params(d):
    return [t for l in range(d.L) for t in (d.w[l], d.b[l])]


class MaskReader:
    """forward hooks on the reference model's Linear layers: the pre-activations of the last forward -> torch's own masks"""

    def __init__(self, model):
        self.z = [None] * len(model.layers)
        for i, layer in enumerate(model.layers):
            layer.register_forward_hook(lambda m, inp, out, i=i: self.z.__setitem__(i, out.detach().numpy().copy()))

    def masks(self):
        return [z > 0 for z in self.z[:-1]]


def part_a(ref, out):
    rng = np.random.default_rng(20240701)
    data, images, texts, image_ids, index = make_pickle(rng, 60, 16, 20)
    with in_temp_dir(data):
        dl_train, dl_test = quiet(ref.get_dataloader)
    out.update(a_images=images, a_texts=texts, a_image_ids=image_ids.astype(np.int64), a_index=index.astype(np.int64),
               a_x_train=dl_train.dataset.tensors[0].numpy(), a_y_train=dl_train.dataset.tensors[1].numpy(),
               a_x_test=dl_test.dataset.tensors[0].numpy(), a_y_test=dl_test.dataset.tensors[1].numpy(),
               a_batch=np.int64(dl_train.batch_size))
    print("(a) train", out["a_x_train"].shape, "test", out["a_x_test"].shape)


def part_b(ref, out):
    rng = np.random.default_rng(20240702)
    dims, n, batch, lr, mom = [36, 44, 44, 44, 28], 13, 5, 0.05, 0.9
    x = rng.normal(0.0, 1.0, (n, dims[0])).astype(np.float32)
    y = rng.normal(0.0, 1.0, (n, dims[-1])).astype(np.float32)
    torch.manual_seed(1234)
    model = ref.MLP(36, 44, 28, 4)
    with torch.no_grad():
        for l, layer in enumerate(model.layers):
            layer.weight.copy_(torch.from_numpy((rng.normal(0.0, 1.0, (dims[l + 1], dims[l])) / np.sqrt(dims[l])).astype(np.float32)))
    reader = MaskReader(model)
    loader = ref.get_torch_dataloader_from_list(torch.from_numpy(x), torch.from_numpy(y), batch_size_train=batch)
    criterion = torch.nn.MSELoss()
    optimizer = torch.optim.SGD(model.parameters(), lr=lr, momentum=mom)
    states, losses = [params_of(model)], []
    d = D.Bridger(states[0][0::2], states[0][1::2])
    floor_p, floor_l = 0.0, 0.0
    own = d.copy()
    model.train()
    for epoch in range(2):
        for inputs, labels in loader:
            optimizer.zero_grad()
            loss = criterion(model(inputs).view(-1), labels.view(-1))
            loss.backward()
            optimizer.step()
            losses.append(loss.item())
            states.append(params_of(model))
            ld = d.train_step(inputs.numpy(), labels.numpy(), lr, mom, reader.masks())
            own.train_step(inputs.numpy(), labels.numpy(), lr, mom)
            floor_l = max(floor_l, abs(losses[-1] - ld))
            floor_p = max(floor_p, max(D.deviation(a, b) for a, b in zip(states[-1], def_params(d))))
    model.eval()
    with torch.no_grad():
        ev = model(torch.from_numpy(x)).numpy()
        ev_losses = [criterion(model(torch.from_numpy(x[r:r + batch])).view(-1), torch.from_numpy(y[r:r + batch]).view(-1)).item()
                     for r in range(0, n, batch)]
    floor_o = D.deviation(ev, d.forward(x))
    floor_e = abs(float(np.sum(ev_losses)) - d.evaluate(x, y, batch)[0])
    scale = max(float(np.abs(p).max()) for p in def_params(d))
    dev_own = max(D.deviation(a, b) for a, b in zip(states[-1], def_params(own)))
    assert dev_own <= 4 * floor_p + D.ULP2 * scale, ("(b): the definition with its own masks leaves the bound", dev_own, floor_p)
    out.update(b_dims=np.array(dims, dtype=np.int64), b_x=x, b_y=y, b_batch=np.int64(batch), b_lr=np.float64(lr), b_momentum=np.float64(mom),
               b_losses=np.array(losses, dtype=np.float64), b_eval_out=ev, b_eval_losses=np.array(ev_losses, dtype=np.float64),
               floor_b_params=np.float64(floor_p), floor_b_loss=np.float64(floor_l), floor_b_out=np.float64(floor_o),
               floor_b_eval=np.float64(floor_e))
    for s, st in enumerate(states):
        for k, p in enumerate(st):
            out[f"b_state{s}_{k}"] = p
    print("(b) steps", len(losses), "floors: params %.3g loss %.3g out %.3g eval %.3g; own-mask run %.3g" %
          (floor_p, floor_l, floor_o, floor_e, dev_own))


def part_c(ref, wandb, out):
    rng = np.random.default_rng(20240703)
    data, images, texts, image_ids, index = make_pickle(rng, 100, 640, 30)
    made = []
    real_mlp = ref.MLP

    def recording_mlp(*a, **k):
        m = real_mlp(*a, **k)
        made.append(m)
        m.initial = params_of(m)
        m.reader = MaskReader(m)
        return m

    with in_temp_dir(data):
        dl_train, dl_test = quiet(ref.get_dataloader)
        xt, yt = (t.numpy() for t in dl_train.dataset.tensors)
        xv, yv = (t.numpy() for t in dl_test.dataset.tensors)
        batch = dl_train.batch_size
        # the definition in lock-step: a hook on the last layer sees every training forward
        state = {"step": 0, "d": None, "floor_p": 0.0, "losses": [], "val": []}
        steps_per_epoch = (len(xt) + batch - 1) // batch

        def val_of(d):
            s, k = d.evaluate(xv, yv, batch)
            return s / k

        def after_forward(m, inp, o):
            model = made[0]
            if not model.training:
                return
            if state["d"] is None:
                state["d"] = D.Bridger(model.initial[0::2], model.initial[1::2])
            else:                                        # the parameters before this step = after the one before
                state["floor_p"] = max(state["floor_p"], max(D.deviation(a, b) for a, b in zip(params_of(model), def_params(state["d"]))))
                if state["step"] % steps_per_epoch == 0:
                    state["val"].append(val_of(state["d"]))
            r0 = (state["step"] % steps_per_epoch) * batch
            state["d"].train_step(xt[r0:r0 + batch], yt[r0:r0 + batch], 0.001, 0.9, model.reader.masks())
            state["losses"].append(state["d"].last)
            state["step"] += 1

        ref.MLP = recording_mlp
        torch.manual_seed(4321)
        try:
            wandb.records.clear()
            # train_modal calls wandb.init right after it has built the model: the lock-step hook goes on there, behind the
            # mask hooks that recording_mlp registered
            wandb.init = lambda *a, **k: made[0].layers[-1].register_forward_hook(after_forward)
            assert quiet(ref.train_modal) == -1
            final = torch.load(ref.PATH, map_location="cpu")
        finally:
            ref.MLP = real_mlp
    model, d = made[0], state["d"]
    state["val"].append(val_of(d))
    train_loss = np.array([r["train_loss"] for r in wandb.records if "train_loss" in r])
    val_loss = np.array([r["val_loss"] for r in wandb.records if "val_loss" in r])
    assert len(train_loss) == 100 and len(val_loss) == 100 and state["step"] == 100 * steps_per_epoch
    final_p = [final[f"layers.{i}.{p}"].numpy() for i in range(8) for p in ("weight", "bias")]
    floor_p = max(state["floor_p"], max(D.deviation(a, b) for a, b in zip(final_p, def_params(d))))
    tl_def = np.array(state["losses"]).reshape(100, steps_per_epoch).mean(1)
    floor_t, floor_v = float(np.abs(train_loss - tl_def).max()), float(np.abs(val_loss - np.array(state["val"])).max())

    # the definition with its OWN masks, as the CPU test runs it
    own = D.Bridger(model.initial[0::2], model.initial[1::2])
    tl_own, vl_own = [], []
    for e in range(100):
        own.read_loss(reset=True)
        own.train_epoch(xt, yt, batch, 0.001, 0.9)
        _, s, k = own.read_loss(reset=True)
        tl_own.append(s / k)
        vl_own.append(val_of(own))
    scale = max(float(np.abs(p).max()) for p in def_params(d))
    dev_own = max(D.deviation(a, b) for a, b in zip(final_p, def_params(own)))
    assert dev_own <= 4 * floor_p + D.ULP2 * scale, ("(c): the definition with its own masks leaves the bound", dev_own, floor_p)
    assert np.abs(train_loss - tl_own).max() <= 4 * floor_t + D.ULP2 * train_loss.max()
    assert np.abs(val_loss - vl_own).max() <= 4 * floor_v + D.ULP2 * val_loss.max()
    out.update(c_images=images, c_texts=texts, c_image_ids=image_ids.astype(np.int64), c_index=index.astype(np.int64),
               c_train_loss=train_loss, c_val_loss=val_loss, c_batch=np.int64(batch),
               floor_c_params=np.float64(floor_p), floor_c_train_loss=np.float64(floor_t), floor_c_val_loss=np.float64(floor_v))
    for i in range(8):
        out[f"c_bias0_{i}"] = model.initial[2 * i + 1]
        out[f"c_bias_{i}"] = final_p[2 * i + 1]
        out[f"c_weight8_{i}"] = final_p[2 * i][:8].copy()
    print("(c) train_loss %.6g -> %.6g, val_loss %.6g -> %.6g; floors: params %.3g train %.3g val %.3g; own-mask run %.3g" %
          (train_loss[0], train_loss[-1], val_loss[0], val_loss[-1], floor_p, floor_t, floor_v, dev_own))


def main():
    ref, wandb = import_reference()
    torch.set_num_threads(8)
    out = {}
    part_a(ref, out)
    part_b(ref, out)
    part_c(ref, wandb, out)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT}: {size} bytes, {len(out)} arrays")
    assert size < 1000000


if __name__ == "__main__":
    main()
