"""The supervised modality bridger: ``capdec_bridger_*`` (bridger.hip), their Engine methods, the reference's
``others/supervised_embedding_bridger.py`` under its names and ``predictions_runner``'s ``modality_bridger=``, against the fp64
restatement of the contract in tests/bridger_def.py, against torch fp32 on the CPU (the reference's arithmetic: an nn.Linear
stack, F.relu, nn.MSELoss, torch.optim.SGD, restated here) and against what the reference itself returned, logged and saved
(tests/golden/bridger.npz, tools/gen_bridger_golden.py).

Bounds.  For every compared tensor q (output, activations, loss, momentum buffers, parameters, per step):
``4 floor_q + 2.4e-7 max |def_q|`` with ``floor_q = max |torch fp32 - definition|`` on the same inputs, measured in the test
(bridger_def.bound).  No element is excluded anywhere.  A hidden pre-activation within rounding of 0 can fall on either side
in fp32, which changes the gradient by a whole term; so the tests read the device's activations, hold them to the
definition's forward, require the device's masks ``h > 0`` to differ from the definition's only at units with ``|z_def|``
inside that layer's forward bound, and run the definition's backward with the device's masks (the torch floor is taken
with torch's own masks in the same way).  Through the facade, against the recorded reference runs: 4 floor (reference vs
definition, stored with the fixture) + the bound above.  Every test prints its largest deviation as a fraction of its bound.

Measured on the MI355X (max deviation / bound; ReLU units whose mask differed from the definition's):
  forward vs definition        0.191 ([640] * 9), 0.129 ([36, 44, 28]), 0.170 ([1024, 8, 1024]), 0.182 ([640, 640]),
                               0.276 ([1024, 1024]), 0.130 (widths 12, 16, 20 around the column tile); rows bit-identical for every n
  three train steps            0.261 (reference shape, identity), 0.274 (random), 0.256 / 0.239 / 0.338 / 0.393 / 0.318
                               (batch 1 / 2 / 31 / 33 / 64), 0.401 ([1024, 1024] batch 64), 0.392 ([1024, 8, 1024]),
                               0.429 (widths 4, 8, 12, 20, 132, 124, 8 around the backward tile), 0.204 (one step at lr 0.001),
                               0.338 (lr 0); mask units that differed: 0 in every case
  epoch = steps, eval          bit for bit; eval 0.030 at most
  facade vs the fixture        (b) 0.149; (c) train_loss 0.064, val_loss 0.060, final tensors 0.001
"""
import contextlib
import ctypes as C
import inspect
import io
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bridger_def as D                                   # noqa: E402
from capdec_amd import synth                              # noqa: E402

T = torch.from_numpy
SRC = open(os.path.join(ROOT, "capdec_amd", "csrc", "bridger.hip")).read()
FWD_COLS = int(re.search(r"BRIDGER_FWD_COLS\s*=\s*(\d+)", SRC).group(1))       # the forward kernel's column tile
BWD_COLS = int(re.search(r"BRIDGER_BWD_COLS\s*=\s*(\d+)", SRC).group(1))       # the columns of W a backward block owns
NAMES = ("capdec_bridger_load", "capdec_bridger_forward", "capdec_bridger_train_step", "capdec_bridger_train_epoch",
         "capdec_bridger_eval", "capdec_bridger_loss", "capdec_bridger_get")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "bridger.npz"))


def make(dims, batch, seed, identity=False):
    """(weights, biases, x, y): seeded random weights of scale 1 / sqrt(fan_in) or the reference's identity initialisation,
    biases within 1 / sqrt(fan_in), unit rows"""
    rng = np.random.default_rng(seed)
    L = len(dims) - 1
    ws = [np.eye(dims[l + 1], dims[l], dtype=np.float32) if identity else
          (rng.normal(0.0, 1.0, (dims[l + 1], dims[l])) / np.sqrt(dims[l])).astype(np.float32) for l in range(L)]
    bs = [rng.uniform(-1.0, 1.0, dims[l + 1]).astype(np.float32) / np.float32(np.sqrt(dims[l])) for l in range(L)]
    x = rng.normal(0.0, 1.0, (batch, dims[0]))
    y = rng.normal(0.0, 1.0, (batch, dims[-1]))
    if identity:
        x, y = np.abs(x), np.abs(y) * 0.7 + 0.3 * np.abs(x[:, :1])       # the identity stack passes what is positive
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)      # noqa: E731
    return ws, bs, unit(x), unit(y)


def params(d):
    return [t for l in range(d.L) for t in (d.w[l], d.b[l])]


def buffers(d):
    return [t for l in range(d.L) for t in (d.vw[l], d.vb[l])]


def torch_forward(layers, x):
    h, acts = x, []
    for i, layer in enumerate(layers):
        h = F.relu(layer(h)) if i < len(layers) - 1 else layer(h)
        acts.append(h)
    return acts


def torch_layers(ws, bs):
    layers = [torch.nn.Linear(w.shape[1], w.shape[0]) for w in ws]
    with torch.no_grad():
        for layer, w, b in zip(layers, ws, bs):
            layer.weight.copy_(T(np.asarray(w, dtype=np.float32)))
            layer.bias.copy_(T(np.asarray(b, dtype=np.float32)))
    return layers


def torch_floors(ws, bs, x, y, steps, lr, momentum):
    """the reference arithmetic (torch fp32, CPU) beside the definition run with torch's own masks -> per step
    {'act': [L], 'loss', 'v': [2 L], 'p': [2 L]} = max |torch - definition|"""
    layers = torch_layers(ws, bs)
    ps = [p for layer in layers for p in (layer.weight, layer.bias)]
    opt = torch.optim.SGD(ps, lr=lr, momentum=momentum)
    d, out = D.Bridger(ws, bs), []
    for _ in range(steps):
        opt.zero_grad()
        acts = torch_forward(layers, T(x))
        loss = torch.nn.MSELoss()(acts[-1].view(-1), T(y).view(-1))
        loss.backward()
        opt.step()
        ld = d.train_step(x, y, lr, momentum, [a.detach().numpy() > 0 for a in acts[:-1]])
        out.append({"act": [D.deviation(a.detach().numpy(), h) for a, h in zip(acts, d.acts)], "loss": abs(loss.item() - ld),
                    "v": [D.deviation(opt.state[p]["momentum_buffer"].numpy(), v) for p, v in zip(ps, buffers(d))],
                    "p": [D.deviation(p.detach().numpy(), q) for p, q in zip(ps, params(d))]})
    return out


def ratio(dev, bound):
    return dev / bound if bound > 0 else (0.0 if dev == 0 else float("inf"))


class DefEngine:
    """stands for the Engine where there is no GPU: the bridger calls answered by the definition"""
    device = torch.device("cpu")

    def normalize_prefix(self, x, normalize=True, offset=None):
        x = x.double()
        return (x / x.norm(2, -1, keepdim=True)).float()

    def bridger_load(self, weights, biases):
        self.d = D.Bridger([w.numpy() for w in weights], [b.numpy() for b in biases])
        self.calls = []

    def bridger_train_epoch(self, x, y, batch=32, lr=0.001, momentum=0.9):
        self.calls.append("epoch")
        self.d.train_epoch(x.numpy(), y.numpy(), batch, lr, momentum)

    def bridger_eval(self, x, y, batch=32):
        self.calls.append("eval")
        return self.d.evaluate(x.numpy(), y.numpy(), batch)

    def bridger_loss(self, reset=False):
        return self.d.read_loss(reset)

    def bridger_get(self, kind, which, batch=None):
        return T(params(self.d)[which].astype(np.float32))

    def bridger_forward(self, x):
        return T(self.d.forward(x.numpy()).astype(np.float32))


def _prototype(header, name):
    bare = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", bare, flags=re.S)
    assert m, f"include/capdec.h does not declare {name}"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _pickle_of(g, part):
    idx, ids = g[part + "_index"], g[part + "_image_ids"]
    return {"captions": [{"image_id": int(ids[i]), "clip_embedding": int(idx[i]), "caption": f"c{i}"} for i in range(len(ids))],
            "clip_embedding": T(g[part + "_images"]), "clip_embedding_text_dave": T(g[part + "_texts"])}


# ===================================================================================== CPU
def test_abi_surface():
    """the seven prototypes are in the header, _capi.SIGNATURES agrees with them, bridger.hip is built, the library exports the
    symbols and the ABI number stays 6"""
    from capdec_amd import _capi, build
    header = open(os.path.join(ROOT, "include", "capdec.h")).read()
    for name, count in zip(NAMES, (5, 4, 7, 7, 7, 5, 5)):
        ps = _prototype(header, name)
        res, args = _capi.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(ps) == count, name
        for p, a in zip(ps, args):
            assert (a is C.c_int) == (p.startswith("int ") and "*" not in p), (p, a)
            assert (a is C.c_float) == (p.startswith("float ") and "*" not in p), (p, a)
    assert re.search(r"#define\s+CAPDEC_ABI_VERSION\s+6\b", header) and _capi.ABI_VERSION == 6
    assert "bridger.hip" in build.SOURCES
    assert "capdec::Bridger bridger" in open(os.path.join(ROOT, "capdec_amd", "csrc", "context.h")).read()
    lib = _capi.load_library()
    assert all(hasattr(lib, n) for n in NAMES) and lib.capdec_abi_version() == 6
    assert FWD_COLS % 4 == 0 and BWD_COLS % 4 == 0


def test_reference_names_and_parameters(tmp_path):
    """the reference's names, its parameters first; MLP(640, 640, 640, 8) is identity weights and nn.Linear biases"""
    from capdec_amd import predictions_runner as PR, supervised_embedding_bridger as B
    from capdec_amd.engine import Engine
    P = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert B.BTCH_SIZE == 32 and B.PATH == 'weights_modality_mapper.pt' and B.DBG is False
    assert P(B.MLP.__init__)[:5] == ["self", "input_dim", "hidden_dim", "output_dim", "num_layers"]
    assert P(B.noise_augmentation) == ["x", "variance"] and inspect.signature(B.noise_augmentation).parameters["variance"].default == 0.001
    assert P(B.get_torch_dataloader_from_list) == ["list_x", "list_y", "list_x_test", "list_y_test", "batch_size_train",
                                                   "batch_size_test", "split"]
    assert P(B.get_dataloader)[0] == "path_or_data"
    assert P(B.train_modal) == ["data", "epochs", "lr", "momentum", "batch_size", "out_path", "log", "engine"]
    sig = inspect.signature(B.train_modal).parameters
    assert [sig[k].default for k in P(B.train_modal)] == [None, 100, 0.001, 0.9, 32, B.PATH, None, None]
    assert "returns -1" in " ".join(B.train_modal.__doc__.split())
    assert P(B.get_map_to_text_space_using_modality_bridger) == ["path", "engine"]
    assert inspect.signature(B.get_map_to_text_space_using_modality_bridger).parameters["path"].default == 'others/' + B.PATH
    assert not hasattr(B, "check_results")
    for f in (PR.prefix_from_embeddings, PR.caption_ids, PR.make_preds, PR.make_preds_from_images):
        p = inspect.signature(f).parameters["modality_bridger"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert "modality_bridger" not in inspect.signature(PR.paraphrase_distance_ablation).parameters
    for name in ("bridger_load", "bridger_forward", "bridger_train_step", "bridger_train_epoch", "bridger_eval", "bridger_loss",
                 "bridger_get"):
        assert callable(getattr(Engine, name))
    torch.manual_seed(5)
    m = B.MLP(640, 640, 640, 8)
    sd = m.state_dict()
    assert list(sd) == [f"layers.{i}.{p}" for i in range(8) for p in ("weight", "bias")]
    for i in range(8):
        assert torch.equal(sd[f"layers.{i}.weight"], torch.eye(640)) and sd[f"layers.{i}.bias"].shape == (640,)
        assert float(sd[f"layers.{i}.bias"].abs().max()) <= 1 / np.sqrt(640) and float(sd[f"layers.{i}.bias"].abs().max()) > 0
    torch.manual_seed(5)                                    # nn.Linear's own initialisation, in the reference's draw order
    want = [torch.nn.Linear(640, 640).bias.detach() for _ in range(8)]
    assert all(torch.equal(sd[f"layers.{i}.bias"], want[i]) for i in range(8))
    torch.save(sd, tmp_path / "w.pt")
    m2 = B.MLP(640, 640, 640, 8)
    m2.load_state_dict(torch.load(tmp_path / "w.pt"))
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), sd.values()))
    with pytest.raises(RuntimeError):
        m2.load_state_dict({"layers.0.weight": torch.eye(640)})
    small = B.MLP(36, 44, 28, 4).state_dict()
    assert [tuple(v.shape) for v in small.values()] == [(44, 36), (44,), (44, 44), (44,), (44, 44), (44,), (28, 44), (28,)]


def test_definition_vs_reference_fixture(golden):
    """the definition, with its own masks, against the reference's recorded runs (b) and (c), within 4 floor + two ulps"""
    g = golden
    # ---- (b): every state, every loss, the eval outputs
    x, y, batch, lr, mom = g["b_x"], g["b_y"], int(g["b_batch"]), float(g["b_lr"]), float(g["b_momentum"])
    state = lambda s: [g[f"b_state{s}_{k}"] for k in range(8)]      # noqa: E731
    d = D.Bridger(state(0)[0::2], state(0)[1::2])
    worst, s = 0.0, 0
    for _ in range(2):
        for r0 in range(0, len(x), batch):
            ld = d.train_step(x[r0:r0 + batch], y[r0:r0 + batch], lr, mom)
            s += 1
            worst = max(worst, ratio(abs(ld - g["b_losses"][s - 1]), D.bound(g["floor_b_loss"], ld)))
            for got, want in zip(params(d), state(s)):
                worst = max(worst, ratio(D.deviation(want, got), D.bound(g["floor_b_params"], got)))
    assert s == 6 == len(g["b_losses"])
    out = d.forward(x)
    worst = max(worst, ratio(D.deviation(g["b_eval_out"], out), D.bound(g["floor_b_out"], out)))
    ev, k = d.evaluate(x, y, batch)
    assert k == len(g["b_eval_losses"]) == 3
    worst = max(worst, ratio(abs(ev - g["b_eval_losses"].sum()), D.bound(g["floor_b_eval"], ev)))
    print(f"(b) definition vs the reference's run: max deviation / bound {worst:.3f}")
    assert worst <= 1.0
    # ---- (a) + (c): the split, then train_modal's 100 epochs
    for part in ("a", "c"):
        test, train = D.split_rows(list(g[part + "_image_ids"][:-1]), list(g[part + "_index"][:-1]))
        unit = lambda a: a.astype(np.float64) / np.linalg.norm(a.astype(np.float64), axis=1, keepdims=True)      # noqa: E731
        if part == "a":
            xi, xt = unit(g["a_images"][:-1]), unit(g["a_texts"][:-1])
            for rows, src, name in ((train, xi, "a_x_train"), (train, xt, "a_y_train"), (test, xi, "a_x_test"), (test, xt, "a_y_test")):
                assert g[name].shape == (len(rows), src.shape[1]) and float(np.abs(g[name] - src[rows]).max()) <= 2.4e-7
    xi, xt = unit(g["c_images"][:-1]).astype(np.float32), unit(g["c_texts"][:-1]).astype(np.float32)
    batch = int(g["c_batch"])
    d = D.Bridger([np.eye(640)] * 8, [g[f"c_bias0_{i}"] for i in range(8)])
    worst = 0.0
    for e in range(100):
        d.read_loss(reset=True)
        d.train_epoch(xi[train], xt[train], batch, 0.001, 0.9)
        _, tot, k = d.read_loss(reset=True)
        worst = max(worst, ratio(abs(tot / k - g["c_train_loss"][e]), D.bound(g["floor_c_train_loss"], tot / k)))
        tot, k = d.evaluate(xi[test], xt[test], batch)
        worst = max(worst, ratio(abs(tot / k - g["c_val_loss"][e]), D.bound(g["floor_c_val_loss"], tot / k)))
    scale = max(float(np.abs(p).max()) for p in params(d))
    for i in range(8):
        for got, want in ((d.b[i], g[f"c_bias_{i}"]), (d.w[i][:8], g[f"c_weight8_{i}"])):
            worst = max(worst, D.deviation(want, got) / (4 * float(g["floor_c_params"]) + D.ULP2 * scale))
    print(f"(c) definition vs the reference's train_modal: max deviation / bound {worst:.3f}")
    assert worst <= 1.0


def test_a_wrong_term_does_not_fit_the_bound():
    """one batch row left out of dW, and momentum applied wrongly on the first step (v = g (1 - momentum)), each deviate from
    the definition by more than 10 bounds on the tests' inputs"""
    for dims, batch, identity in (([36, 44, 28], 31, False), ([640] * 9, 32, True), ([640] * 9, 32, False)):
        ws, bs, x, y = make(dims, batch, 11, identity)
        floors = torch_floors(ws, bs, x, y, 1, 0.05, 0.9)[0]
        good = D.Bridger(ws, bs)
        good.train_step(x, y, 0.05, 0.9)
        for wrong in ("drop_row", "first_step_momentum"):
            bad = D.Bridger(ws, bs)
            bad.train_step(x, y, 0.05, 0.9, wrong=wrong)
            worst = max(ratio(D.deviation(a, b), D.bound(f, b))
                        for f, a, b in list(zip(floors["v"], buffers(bad), buffers(good))) + list(zip(floors["p"], params(bad), params(good))))
            print(f"{dims[:3]} batch {batch} identity {identity}: '{wrong}' deviates by {worst:.0f} bounds")
            assert worst > 10.0


def test_engine_argument_checks():
    """what the Engine methods refuse before they reach the library"""
    from capdec_amd._capi import CapdecError
    from capdec_amd.engine import Engine
    e = Engine.__new__(Engine)
    z = torch.zeros
    for call in (lambda: Engine.bridger_forward(e, z(2, 8)), lambda: Engine.bridger_train_step(e, z(2, 8), z(2, 8)),
                 lambda: Engine.bridger_train_epoch(e, z(2, 8), z(2, 8)), lambda: Engine.bridger_eval(e, z(2, 8), z(2, 8)),
                 lambda: Engine.bridger_loss(e), lambda: Engine.bridger_get(e, 0, 0)):
        with pytest.raises(CapdecError, match="no bridger is loaded"):
            call()
    with pytest.raises(CapdecError, match="multiple of 4"):
        Engine.bridger_load(e, [z(8, 6), z(8, 8)], [z(8), z(8)])
    with pytest.raises(CapdecError, match="multiple of 4"):
        Engine.bridger_load(e, [z(1028, 8)], [z(1028)])
    with pytest.raises(CapdecError, match="1 to 16 layers"):
        Engine.bridger_load(e, [], [])
    with pytest.raises(CapdecError, match="1 to 16 layers"):
        Engine.bridger_load(e, [z(8, 8)] * 17, [z(8)] * 17)
    with pytest.raises(CapdecError, match="layer 1 must be"):
        Engine.bridger_load(e, [z(12, 8), z(8, 16)], [z(12), z(8)])
    with pytest.raises(CapdecError, match="layer 0 must be"):
        Engine.bridger_load(e, [z(12, 8)], [z(8)])
    e.bridger = (8, 12, 4)                                 # as after a load
    with pytest.raises(CapdecError, match=r"x must be \[n, 8\]"):
        Engine.bridger_forward(e, z(2, 12))
    with pytest.raises(CapdecError, match=r"y must be \[2, 4\]"):
        Engine.bridger_train_step(e, z(2, 8), z(2, 8))
    with pytest.raises(CapdecError, match="batch must be"):
        Engine.bridger_train_step(e, z(0, 8), z(0, 4))
    with pytest.raises(CapdecError, match="batch must be"):
        Engine.bridger_train_step(e, z(65, 8), z(65, 4))
    for batch in (0, 65, 2.5, True):
        with pytest.raises(CapdecError, match="batch must be"):
            Engine.bridger_train_epoch(e, z(70, 8), z(70, 4), batch)
    with pytest.raises(CapdecError, match="batch must be"):
        Engine.bridger_eval(e, z(70, 8), z(70, 4), 0)
    with pytest.raises(CapdecError, match="which must be"):
        Engine.bridger_get(e, 1, 4)
    with pytest.raises(CapdecError, match="activation must be"):
        Engine.bridger_get(e, 2, 2, 8)
    with pytest.raises(CapdecError, match="kind must be"):
        Engine.bridger_get(e, 3, 0)


def test_train_modal_logs_and_prints(golden, tmp_path, capsys):
    """train_modal with the definition standing for the engine: the dicts the reference gives wandb.log, in its order, one
    epoch call and one eval call per epoch, the printed text, the saved state dict; get_dataloader's split (fixture (a))"""
    from capdec_amd import supervised_embedding_bridger as B
    g, eng = golden, DefEngine()
    dl_train, dl_test = B.get_dataloader(_pickle_of(g, "a"), engine=eng)
    text = capsys.readouterr().out
    assert text.splitlines() == ["images_embeddings torch.Size([60, 16])", "sample...", "indexs...", "indexs..."]
    assert dl_train.batch_size == dl_test.batch_size == 32 == int(g["a_batch"])
    got = [t.numpy() for dl in (dl_train, dl_test) for t in dl.dataset.tensors]
    test, train = D.split_rows(list(g["a_image_ids"][:-1]), list(g["a_index"][:-1]))
    xi, xt = eng.normalize_prefix(T(g["a_images"][:-1]).float()).numpy(), eng.normalize_prefix(T(g["a_texts"][:-1]).float()).numpy()
    for have, rows, src, name in zip(got, (train, train, test, test), (xi, xt, xi, xt), ("a_x_train", "a_y_train", "a_x_test", "a_y_test")):
        np.testing.assert_array_equal(have, src[rows])     # the same rows in the same order, exactly
        assert float(np.abs(have - g[name]).max()) <= 2.4e-7
    logged = []
    torch.manual_seed(3)
    model = B.train_modal((dl_train, dl_test), epochs=3, lr=0.05, batch_size=5, out_path=str(tmp_path / "m.pt"), log=logged.append,
                          engine=eng)
    assert capsys.readouterr().out == "Finished Training\n"
    assert [sorted(d) for d in logged] == [["epoch", "train_loss"], ["epoch", "val_loss"]] * 3
    assert [d["epoch"] for d in logged] == [0, 0, 1, 1, 2, 2] and eng.calls == ["epoch", "eval"] * 3
    torch.manual_seed(3)
    d = D.Bridger([np.eye(16)] * 8, [torch.nn.Linear(16, 16).bias.detach().numpy() for _ in range(8)])
    for e in range(3):
        d.read_loss(reset=True)
        d.train_epoch(got[0], got[1], 5, 0.05, 0.9)
        _, tot, k = d.read_loss(reset=True)
        assert k == 10 and logged[2 * e]["train_loss"] == tot / k
        tot, k = d.evaluate(got[2], got[3], 5)
        assert k == 3 and logged[2 * e + 1]["val_loss"] == tot / k
    saved = torch.load(tmp_path / "m.pt")
    assert isinstance(model, B.MLP) and list(saved) == list(model.state_dict())
    for a, b in zip(saved.values(), params(d)):
        np.testing.assert_array_equal(a.numpy(), b.astype(np.float32))
    # four tensors, an empty test set: no val_loss; the default log prints the dicts
    B.train_modal((T(got[0]), T(got[1]), torch.zeros(0, 16), torch.zeros(0, 16)), epochs=2, batch_size=7,
                  out_path=str(tmp_path / "m2.pt"), engine=eng)
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 3 and lines[2] == "Finished Training" and lines[0].startswith("{'epoch': 0, 'train_loss': ")
    with pytest.raises(B.CapdecError, match="four tensors"):
        B.train_modal([1, 2, 3], engine=eng)


def test_no_bridger_leaves_the_prefix_path_alone():
    """modality_bridger=None: prefix_from_embeddings makes exactly the calls it made before; with one, it is applied between
    the normalisation and clip_project and nothing is normalised again"""
    from capdec_amd import predictions_runner as PR
    calls = []

    class Eng:
        def normalize_prefix(self, x, normalize=True, offset=None):
            calls.append(("normalize_prefix", normalize, offset))
            return x * 2

    class Model:
        engine, prefix_length = Eng(), 2

        def clip_project(self, x):
            calls.append(("clip_project", x.clone()))
            return x.repeat(1, 2)

    x = torch.arange(8.0).reshape(2, 4)
    out = PR.prefix_from_embeddings(Model(), x, True, None)
    assert [c[0] for c in calls] == ["normalize_prefix", "clip_project"] and calls[0][1:] == (False, None)
    assert torch.equal(calls[1][1], x * 2) and out.shape == (2, 2, 4)
    calls.clear()
    PR.prefix_from_embeddings(Model(), x, modality_bridger=lambda v: calls.append(("bridger", v.clone())) or v + 1)
    assert [c[0] for c in calls] == ["normalize_prefix", "bridger", "clip_project"]
    assert torch.equal(calls[1][1], x * 2) and torch.equal(calls[2][1], x * 2 + 1)
    seen = {}
    real = PR.prefix_from_embeddings

    class Reached(Exception):
        pass

    def stand_in(*a, **k):
        seen.update(k)
        raise Reached

    PR.prefix_from_embeddings = stand_in
    try:
        with pytest.raises(Reached):
            PR.caption_ids(Model(), x, 0)
        assert seen == {}                                   # no new keyword reaches the call when no bridger is given
    finally:
        PR.prefix_from_embeddings = real


# ===================================================================================== GPU
@pytest.fixture(scope="module")
def eng():
    from capdec_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _load(eng, ws, bs):
    eng.bridger_load([T(np.asarray(w, dtype=np.float32)) for w in ws], [T(np.asarray(b, dtype=np.float32)) for b in bs])


FORWARD_DIMS = [[640] * 9, [36, 44, 28], [1024, 8, 1024], [640, 640], [1024, 1024],
                [40, FWD_COLS - 4, FWD_COLS, FWD_COLS + 4, 8]]


@pytest.mark.gpu
@pytest.mark.parametrize("dims", FORWARD_DIMS, ids=lambda d: "x".join(map(str, d[:5])))
def test_forward_vs_definition(eng, dims):
    """n = 1, 63, 64, 65, 200: every row within the bound of the definition, and the same bits for every n that contains it"""
    ws, bs, x, _ = make(dims, 200, 21)
    _load(eng, ws, bs)
    want = D.Bridger(ws, bs).forward(x)
    with torch.no_grad():
        floor = D.deviation(torch_forward(torch_layers(ws, bs), T(x))[-1].numpy(), want)
    full = eng.bridger_forward(T(x)).cpu().numpy()
    assert full.dtype == np.float32 and full.shape == want.shape
    w = ratio(D.deviation(full, want), D.bound(floor, want))
    for n in (1, 63, 64, 65):
        np.testing.assert_array_equal(eng.bridger_forward(T(x[:n])).cpu().numpy(), full[:n])
    np.testing.assert_array_equal(eng.bridger_forward(T(x[137:])).cpu().numpy(), full[137:])      # wherever the row sits
    assert eng.bridger_forward(T(x[:0])).shape == (0, dims[-1])
    print(f"forward {dims[:3]} x{len(dims) - 1}: max deviation / bound {w:.3f} (floor {floor:.2e})")
    assert w <= 1.0


def _steps_vs_definition(eng, ws, bs, x, y, steps, lr, momentum=0.9):
    """`steps` train steps on the device beside the definition advanced in lock-step with the device's masks -> (largest
    deviation / bound over activations, loss, momentum buffers and parameters of every step; mask units that differed)"""
    floors = torch_floors(ws, bs, x, y, steps, lr, momentum)
    _load(eng, ws, bs)
    d, B, L = D.Bridger(ws, bs), len(x), len(ws)
    worst, flips = 0.0, 0
    for s in range(steps):
        loss = eng.bridger_train_step(T(x), T(y), lr, momentum)
        acts = [eng.bridger_get(2, l, B).cpu().numpy() for l in range(L)]
        zs, hs = d.forward_all(x)
        for l in range(L):
            b = D.bound(floors[s]["act"][l], hs[l])
            w = ratio(D.deviation(acts[l], hs[l]), b)
            assert w <= 1.0, f"step {s}: activation {l} deviates by {w:.2f} bounds"
            worst = max(worst, w)
            if l < L - 1:
                flips += D.masks_agree(acts[l], zs[l], b)
        ld = d.train_step(x, y, lr, momentum, [a > 0 for a in acts[:-1]])
        w = ratio(abs(loss - ld), D.bound(floors[s]["loss"], ld))
        assert w <= 1.0, f"step {s}: the loss deviates by {w:.2f} bounds"
        worst = max(worst, w)
        assert eng.bridger_loss()[0] == loss
        for kind, key, want in ((1, "v", buffers(d)), (0, "p", params(d))):
            for k in range(2 * L):
                got = eng.bridger_get(kind, k).cpu().numpy()
                w = ratio(D.deviation(got, want[k]), D.bound(floors[s][key][k], want[k]))
                assert w <= 1.0, f"step {s}: {'momentum buffer' if kind else 'parameter'} {k} deviates by {w:.2f} bounds"
                worst = max(worst, w)
    return worst, flips


TRAIN_CASES = [("reference shape, identity", [640] * 9, 32, True, 0.05), ("reference shape, random", [640] * 9, 32, False, 0.05)] + \
    [(f"batch {b}", [36, 44, 28], b, False, 0.05) for b in (1, 2, 31, 33, 64)] + \
    [("one layer, LDS chunks", [1024, 1024], 64, False, 0.05), ("narrow waist", [1024, 8, 1024], 64, False, 0.05),
     ("backward tile edges", [BWD_COLS - 4, BWD_COLS, BWD_COLS + 4, 2 * BWD_COLS + 4, 132, 124, BWD_COLS], 33, False, 0.05),
     ("reference lr", [640] * 9, 32, True, 0.001), ("lr 0", [36, 44, 28], 31, False, 0.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("what,dims,batch,identity,lr", TRAIN_CASES, ids=[c[0].replace(" ", "_").replace(",", "") for c in TRAIN_CASES])
def test_train_steps_vs_definition(eng, what, dims, batch, identity, lr):
    """three train steps (one at the reference's lr and at lr 0): activations, loss, every momentum buffer and every parameter
    after every step"""
    ws, bs, x, y = make(dims, batch, 31, identity)
    steps = 3 if lr == 0.05 else 1
    worst, flips = _steps_vs_definition(eng, ws, bs, x, y, steps, lr)
    if lr == 0.0:                                           # the weights stay, the momentum buffers move
        for k in range(2 * (len(dims) - 1)):
            np.testing.assert_array_equal(eng.bridger_get(0, k).cpu().numpy(), (ws + bs)[(k % 2) * len(ws) + k // 2])
            assert float(eng.bridger_get(1, k).abs().max()) > 0
    print(f"{what} {dims[:3]} batch {batch} lr {lr}: max deviation / bound {worst:.3f}; mask units that differ {flips}")


@pytest.mark.gpu
def test_epoch_equals_steps_and_is_deterministic(eng):
    """an epoch over 3 * 32 + 5 rows = the four step calls, bit for bit; bridger_loss gives their sum and count; the same epoch
    twice from the same load gives the same bits; bridger_eval agrees with the definition"""
    for dims in ([36, 44, 28], [640] * 4):
        ws, bs, x, y = make(dims, 3 * 32 + 5, 41)
        L = len(ws)
        state = lambda: [eng.bridger_get(kind, k).cpu().numpy() for kind in (0, 1) for k in range(2 * L)]      # noqa: E731
        _load(eng, ws, bs)
        losses = [eng.bridger_train_step(T(x[r:r + 32]), T(y[r:r + 32]), 0.05, 0.9) for r in range(0, len(x), 32)]
        assert len(losses) == 4
        last, total, count = eng.bridger_loss(reset=True)
        assert (last, total, count) == (losses[-1], float(np.sum(np.array(losses, dtype=np.float64))), 4)
        assert eng.bridger_loss()[1:] == (0.0, 0)
        by_steps = state()
        runs = []
        for _ in range(2):
            _load(eng, ws, bs)
            eng.bridger_train_epoch(T(x), T(y), 32, 0.05, 0.9)
            assert eng.bridger_loss() == (last, total, count)
            runs.append(state())
        for a, b, c in zip(by_steps, runs[0], runs[1]):
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(b, c)
        d = D.Bridger([a.astype(np.float64) for a in runs[0][0:2 * L:2]], [a.astype(np.float64) for a in runs[0][1:2 * L:2]])
        for batch in (32, 7, 200):
            got, k = eng.bridger_eval(T(x), T(y), batch)
            want, kd = d.evaluate(x, y, batch)
            with torch.no_grad():
                layers = torch_layers(d.w, d.b)
                ref = sum(float(np.float32(torch.nn.MSELoss()(torch_forward(layers, T(x[r:r + batch]))[-1].view(-1), T(y[r:r + batch]).view(-1)).item()))
                          for r in range(0, len(x), batch))
            w = ratio(abs(got - want), D.bound(abs(ref - want), want))
            print(f"eval {dims[:3]} batch {batch}: {k} batches, deviation / bound {w:.3f}")
            assert k == kd and w <= 1.0
        assert eng.bridger_eval(T(x[:0]), T(y[:0]), 32) == (0.0, 0)


@pytest.mark.gpu
def test_refusals_leave_the_engine_usable(eng):
    """every refusal -- by the Engine and by the library itself -- and a correct call after them"""
    from capdec_amd._capi import CapdecError
    ws, bs, x, y = make([36, 44, 28], 8, 51)
    _load(eng, ws, bs)
    want = eng.bridger_forward(T(x)).cpu().numpy()
    h, lib = eng._h, eng.lib
    xd, yd = T(x).to(eng.device), T(y).to(eng.device)
    assert lib.capdec_bridger_train_step(h, xd.data_ptr(), yd.data_ptr(), 0, 0.1, 0.9, None) != 0
    assert lib.capdec_bridger_train_step(h, xd.data_ptr(), yd.data_ptr(), 65, 0.1, 0.9, None) != 0
    assert lib.capdec_bridger_train_epoch(h, xd.data_ptr(), yd.data_ptr(), 8, 65, 0.1, 0.9) != 0
    assert lib.capdec_bridger_train_step(h, xd.data_ptr() + 4, yd.data_ptr(), 4, 0.1, 0.9, None) != 0      # not 16-byte aligned
    assert lib.capdec_bridger_get(h, 0, 0, yd.data_ptr(), 5) != 0 and lib.capdec_bridger_get(h, 3, 0, yd.data_ptr(), 5) != 0
    assert lib.capdec_bridger_get(h, 2, 0, yd.data_ptr(), 8 * 44) != 0                                   # no train step yet
    dims = (C.c_int32 * 2)(6, 8)
    assert lib.capdec_bridger_load(h, 1, dims, None, None) != 0 and lib.capdec_bridger_load(h, 0, dims, None, None) != 0
    with pytest.raises(CapdecError):
        eng.bridger_train_step(T(x), T(y[:, :24]))
    np.testing.assert_array_equal(eng.bridger_forward(T(x)).cpu().numpy(), want)      # the bridger loaded before is still there
    assert eng.bridger_train_step(T(x), T(y), 0.05, 0.9) > 0 and eng.bridger_get(2, 1, 8).shape == (8, 28)
    from capdec_amd.engine import Engine
    fresh = Engine(0)
    try:
        assert fresh.lib.capdec_bridger_forward(fresh._h, xd.data_ptr(), 8, yd.data_ptr()) != 0
        assert b"no bridger is loaded" in fresh.lib.capdec_last_error()
    finally:
        fresh.close()


@pytest.mark.gpu
def test_facade_vs_reference_fixture(eng, golden, tmp_path):
    """fixture (b) step by step through an MLP on the engine, fixture (c) through train_modal: the reference's losses, its
    100-epoch curves and its final tensors, within 4 floor (reference vs definition) + the bound of the device"""
    from capdec_amd import supervised_embedding_bridger as B
    g = golden
    two = lambda floor, q: 4 * float(floor) + D.bound(floor, q)      # noqa: E731
    # ---- (b)
    x, y, batch, lr, mom = g["b_x"], g["b_y"], int(g["b_batch"]), float(g["b_lr"]), float(g["b_momentum"])
    model = B.MLP(36, 44, 28, 4, engine=eng)
    keys = list(model.state_dict())
    model.load_state_dict({k: T(g[f"b_state0_{i}"]) for i, k in enumerate(keys)})
    worst, s = 0.0, 0
    for _ in range(2):
        for r0 in range(0, len(x), batch):
            loss = model.engine.bridger_train_step(T(x[r0:r0 + batch]), T(y[r0:r0 + batch]), lr, mom)
            model._device_newer = True
            s += 1
            worst = max(worst, ratio(abs(loss - g["b_losses"][s - 1]), two(g["floor_b_loss"], loss)))
            for i, k in enumerate(keys):
                want = g[f"b_state{s}_{i}"]
                worst = max(worst, ratio(D.deviation(model.state_dict()[k].numpy(), want), two(g["floor_b_params"], want)))
                model._device_newer = True
    out = model(T(x)).cpu().numpy()
    worst = max(worst, ratio(D.deviation(out, g["b_eval_out"]), two(g["floor_b_out"], out)))
    ev, k = model.engine.bridger_eval(T(x), T(y), batch)
    worst = max(worst, ratio(abs(ev - g["b_eval_losses"].sum()), two(g["floor_b_eval"], ev)))
    print(f"(b) through the engine: max deviation / bound {worst:.3f}")
    assert worst <= 1.0 and k == 3
    # ---- (a): the reference's split -- the same rows in the same order (exactly the normalised input's), its values
    with contextlib.redirect_stdout(io.StringIO()):
        dl = B.get_dataloader(_pickle_of(g, "a"), engine=eng)
    test, train = D.split_rows(list(g["a_image_ids"][:-1]), list(g["a_index"][:-1]))
    xi, xt = (eng.normalize_prefix(T(g[k][:-1]).float()).cpu().numpy() for k in ("a_images", "a_texts"))
    got = [t.numpy() for loader in dl for t in loader.dataset.tensors]
    for have, rows, src, name in zip(got, (train, train, test, test), (xi, xt, xi, xt), ("a_x_train", "a_y_train", "a_x_test", "a_y_test")):
        np.testing.assert_array_equal(have, src[rows])
        assert float(np.abs(have - g[name]).max()) <= 2.4e-7
    # ---- (c)
    with contextlib.redirect_stdout(io.StringIO()):
        loaders = B.get_dataloader(_pickle_of(g, "c"), engine=eng)
    logged = []
    torch.manual_seed(4321)                                 # the generator's seed: nn.Linear's biases are the reference's
    with contextlib.redirect_stdout(io.StringIO()) as text:
        trained = B.train_modal(loaders, out_path=str(tmp_path / B.PATH), log=logged.append, engine=eng)
    assert text.getvalue() == "Finished Training\n" and len(logged) == 200
    tl = np.array([d["train_loss"] for d in logged[0::2]])
    vl = np.array([d["val_loss"] for d in logged[1::2]])
    wt = float(np.max(np.abs(tl - g["c_train_loss"]) / (8 * float(g["floor_c_train_loss"]) + D.ULP2 * g["c_train_loss"])))
    wv = float(np.max(np.abs(vl - g["c_val_loss"]) / (8 * float(g["floor_c_val_loss"]) + D.ULP2 * g["c_val_loss"])))
    sd = torch.load(tmp_path / B.PATH)
    assert list(sd) == list(trained.state_dict())
    wp = 0.0
    for i in range(8):
        wp = max(wp, D.deviation(sd[f"layers.{i}.bias"].numpy(), g[f"c_bias_{i}"]), D.deviation(sd[f"layers.{i}.weight"].numpy()[:8], g[f"c_weight8_{i}"]))
    wp /= 8 * float(g["floor_c_params"]) + D.ULP2 * 1.0
    print(f"(c) train_modal: train_loss {tl[0]:.6f} -> {tl[-1]:.6f} (reference {g['c_train_loss'][-1]:.6f}); max deviation / bound: "
          f"train_loss {wt:.3f}, val_loss {wv:.3f}, final tensors {wp:.3f}")
    assert max(wt, wv, wp) <= 1.0
    fn = B.get_map_to_text_space_using_modality_bridger(str(tmp_path / B.PATH), engine=eng)
    probe = loaders[1].dataset.tensors[0]
    np.testing.assert_array_equal(fn(probe).cpu().numpy(), trained(probe).cpu().numpy())


class FakeTok:
    def __init__(self, stop):
        self.stop = stop

    def encode(self, s):
        return [self.stop]

    def decode(self, ids):
        return " ".join(str(int(v)) for v in ids)


@pytest.mark.gpu
def test_end_to_end_make_preds(eng):
    """make_preds with an identity bridger (zero biases, non-negative inputs) gives the tokens of the plain call; with a trained
    one, the tokens of decoding clip_project(bridger(x)) prepared by hand"""
    from capdec_amd import predictions_runner as PR, supervised_embedding_bridger as B
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    from capdec_amd.gpt2_prefix_eval import decode_greedy_ids
    dims, P, W = synth.GPT2_TINY, 10, 64
    model = ClipCaptionModel(P, clip_length=10, prefix_dim=W, num_layers=8, mapping_type=MappingType.MLP, gpt2_dims=dims).to("cuda:0").eval()
    model.load_state_dict(synth.hot_state_dict(7, "mlp", W, P, 10, 8, dims))
    x = synth.synthetic_clip_embeddings(6, W, seed=5, normalize=False).abs() + 0.01
    data = [{"image_id": 40 + i} for i in range(6)]
    tok = FakeTok(dims.vocab + 5)                          # never emitted: every step runs
    plain = PR.make_preds(data, x, model, tok, None, beam=False, entry_length=8)
    ident = B.MLP(W, W, W, 8, engine=eng)
    ident.load_state_dict({k: (v if k.endswith("weight") else torch.zeros_like(v)) for k, v in ident.state_dict().items()})
    assert PR.make_preds(data, x, model, tok, None, beam=False, entry_length=8, modality_bridger=ident) == plain
    assert PR.make_preds(data, x, model, tok, None, beam=True, entry_length=8, modality_bridger=ident) == \
        PR.make_preds(data, x, model, tok, None, beam=True, entry_length=8)
    trained = B.MLP(W, W, W, 8, engine=eng)
    e = trained.engine
    y = synth.synthetic_clip_embeddings(6, W, seed=9, normalize=True)
    for _ in range(20):
        e.bridger_train_step(e.normalize_prefix(x), y, 0.5, 0.9)
    trained._device_newer = True
    bridged = trained(model.engine.normalize_prefix(x))
    assert float((bridged - model.engine.normalize_prefix(x)).abs().max()) > 1e-3      # it does something
    ids, lens = decode_greedy_ids(model, model.clip_project(bridged).reshape(6, P, -1), tok.stop, 8)
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    want = [{"caption": tok.decode(list(ids[i, :int(lens[i])])).lower(), "image_id": 40 + i} for i in range(6)]
    got = PR.make_preds(data, x, model, tok, None, beam=False, entry_length=8, modality_bridger=trained)
    assert got == want and got != plain
    model.release()
