"""Reference ``others/supervised_embedding_bridger.py`` under its own names: a fully supervised mapper from the image
embeddings to the text embeddings -- ``MLP(640, 640, 640, 8)``, ReLU between its Linear layers, identity-initialised weights,
trained with ``MSELoss`` and ``SGD(lr=0.001, momentum=0.9)`` -- that bridges the modality gap in ``predictions_runner``
(``--modality_bridger``).  The reference's trained weights are not distributed, so this module can make them.

The model, the loss, the backward pass and the optimizer run in ``bridger.hip`` (capdec_bridger_*; the contract:
include/capdec.h): an epoch is ONE ``Engine.bridger_train_epoch`` call over rows resident on the device, the validation pass
one ``Engine.bridger_eval``.  What stays on the host is what the reference does there too: reading the pickle, the split by
image id, ``TensorDataset`` / ``DataLoader`` objects, the log lines and ``torch.save``.

The reference's functions take no arguments and read hard-coded paths; here its parameters come first under its names and
the paths, the hyper-parameters and an optional ``engine`` follow.  ``check_results`` is not rebuilt; wandb is not a
dependency (``train_modal(log=wandb.log)`` passes exactly the dicts the reference logs)."""
from __future__ import annotations

import pickle
from collections import OrderedDict
from types import SimpleNamespace
from typing import Dict, Optional

import torch

from ._capi import CapdecError
from .engine import Engine, get_engine
from .gpt2_prefix import _HipModule

DBG = False
BTCH_SIZE = 32 if not DBG else 1
PATH = 'weights_modality_mapper.pt'
DEFAULT_EMBEDDINGS = 'coco_clip_embeddings/oscar_split_RN50x4_train_with_text_embeddings.pkl'


class MLP(_HipModule):
    """reference :87-108 -- "Very simple multi-layer perceptron (also called FFN)": ``num_layers`` Linear layers,
    ``input_dim -> hidden_dim -> ... -> output_dim``, ReLU after every layer but the last.  Weights are ``nn.init.eye_``;
    biases keep ``nn.Linear``'s own initialisation, drawn from torch's generator in the reference's order.  State-dict keys
    ``layers.{i}.weight`` / ``layers.{i}.bias``.  The device copy lives in an Engine's bridger slot (one per context);
    ``state_dict()`` pulls the parameters back after training."""

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers, engine: Optional[Engine] = None):
        super().__init__()
        if num_layers < 1:
            raise CapdecError(f"MLP: num_layers must be at least 1, got {num_layers}")
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.dims = [input_dim] + h + [output_dim]
        for i, (n, k) in enumerate(zip([input_dim] + h, h + [output_dim])):
            layer = torch.nn.Linear(n, k)               # draws the weight, then the bias, like the reference's constructor
            torch.nn.init.eye_(layer.weight)
            self._sd[f"layers.{i}.weight"] = layer.weight.detach().clone()
            self._sd[f"layers.{i}.bias"] = layer.bias.detach().clone()
        self._device_newer = False                      # train steps have run since the host copy was taken
        if engine is not None:
            self._engine = engine

    # --- host copy <-> the engine's bridger slot
    def _keys(self):
        return [f"layers.{i}.{p}" for i in range(self.num_layers) for p in ("weight", "bias")]

    def _upload(self, eng):
        other = getattr(eng, "_bridger_owner", None)
        if other is not None and other is not self:
            other._pull()                               # a context holds one bridger: the one that leaves keeps its values
            other._dirty = True
        eng.bridger_load([self._sd[f"layers.{i}.weight"] for i in range(self.num_layers)],
                         [self._sd[f"layers.{i}.bias"] for i in range(self.num_layers)])
        eng._bridger_owner = self
        self._device_newer = False

    @property
    def engine(self):
        if self._engine is None:
            self._engine = Engine(self._device_index, measure=self._measure)
            self._dirty = True
        if self._dirty or getattr(self._engine, "_bridger_owner", None) is not self:
            self._upload(self._engine)
            self._dirty = False
        return self._engine

    def _pull(self):
        if self._device_newer and self._engine is not None and getattr(self._engine, "_bridger_owner", None) is self:
            for k, name in enumerate(self._keys()):
                self._sd[name] = self._engine.bridger_get(0, k).detach().cpu()
        self._device_newer = False

    def _before_engine_close(self):
        self._pull()

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        self._pull()
        return OrderedDict(self._sd)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        need = self._keys()
        missing = [k for k in need if k not in sd]
        unexpected = [k for k in sd if k not in need]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for MLP: Missing key(s): {missing}; unexpected key(s): {unexpected}")
        for k in need:
            if k in sd:
                if tuple(sd[k].shape) != tuple(self._sd[k].shape):
                    raise RuntimeError(f"size mismatch for {k}: {tuple(sd[k].shape)} in the checkpoint, {tuple(self._sd[k].shape)} in the model")
                self._sd[k] = sd[k].detach().float().cpu().clone()
        self._device_newer = False
        self._dirty = True
        return SimpleNamespace(missing_keys=missing, unexpected_keys=unexpected)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """``x`` [..., input_dim] -> fp32 [..., output_dim] on the device"""
        if x.dim() < 1 or int(x.shape[-1]) != self.dims[0]:
            raise CapdecError(f"MLP: the input must be [..., {self.dims[0]}], got {tuple(x.shape)}")
        out = self.engine.bridger_forward(x.reshape(-1, self.dims[0]))
        return out.reshape(*x.shape[:-1], self.dims[-1])


def get_map_to_text_space_using_modality_bridger(path='others/' + PATH, engine: Optional[Engine] = None):
    """reference :21-30: load the trained ``MLP(640, 640, 640, 8)`` from ``path`` and return the callable that
    ``predictions_runner``'s ``modality_bridger=`` takes"""
    model = MLP(640, 640, 640, 8, engine=engine)
    model.load_state_dict(torch.load(path, map_location="cpu"))
    model.eval()

    def map_to_text_space_using_modality_bridger(image_embedding):
        return model(image_embedding)

    return map_to_text_space_using_modality_bridger


def get_torch_dataloader_from_list(list_x, list_y, list_x_test=None, list_y_test=None, batch_size_train=1, batch_size_test=1, split=None):
    """reference :70-84, host code over torch's ``TensorDataset`` / ``DataLoader`` (unshuffled, not ``drop_last``)"""
    my_dataset = torch.utils.data.TensorDataset(torch.Tensor(list_x.float()), torch.Tensor(list_y).float())
    my_dataloader = torch.utils.data.DataLoader(my_dataset, batch_size=batch_size_train)
    if split is not None:
        assert list_x_test is None and list_y_test is None
        split[0] += (len(list_x) - (split[0] + split[1]))
        train_set, val_set = torch.utils.data.random_split(my_dataset, split)
        return torch.utils.data.DataLoader(train_set, batch_size=batch_size_train), torch.utils.data.DataLoader(val_set, batch_size=batch_size_test)

    if list_x_test is not None and list_y_test is not None:
        my_dataset_test = torch.utils.data.TensorDataset(torch.Tensor(list_x_test), torch.Tensor(list_y_test))
        my_dataloader_test = torch.utils.data.DataLoader(my_dataset_test, batch_size=batch_size_test)
        return my_dataloader, my_dataloader_test

    return my_dataloader


def get_dataloader(path_or_data=DEFAULT_EMBEDDINGS, engine: Optional[Engine] = None):
    """reference :33-67 -> (train loader, test loader), batches of ``BTCH_SIZE``.  ``path_or_data``: the path of the pickle
    (keys ``captions``, ``clip_embedding``, ``clip_embedding_text_dave``) or that dict.  As in the reference the LAST caption
    and the last row of either side are dropped, the rows are L2-normalised (``Engine.normalize_prefix``), the captions are
    sorted by ``image_id`` (stably), the first ``int(0.2 * len)`` of them form the test set, and both sides are gathered
    through each caption's ``clip_embedding`` index."""
    if isinstance(path_or_data, (str, bytes)) or hasattr(path_or_data, "__fspath__"):
        with open(path_or_data, 'rb') as f:
            data = pickle.load(f)
    else:
        data = path_or_data
    captions = list(data['captions'])[:10 if DBG else -1]
    eng = engine or get_engine()
    images_embeddings = eng.normalize_prefix(torch.as_tensor(data['clip_embedding'])[:10 if DBG else -1].float()).cpu()
    text_embeddings = eng.normalize_prefix(torch.as_tensor(data['clip_embedding_text_dave'])[:10 if DBG else -1].float()).cpu()
    print('images_embeddings', images_embeddings.shape)
    print('sample...')
    print('indexs...')
    captions.sort(key=lambda x: x['image_id'])          # split to test and train by image id
    cut = int(len(captions) * 0.2)
    test_embeddings_indexs = [s['clip_embedding'] for s in captions[:cut]]
    train_embeddings_indexs = [s['clip_embedding'] for s in captions[cut:]]
    print('indexs...')
    return get_torch_dataloader_from_list(images_embeddings[train_embeddings_indexs], text_embeddings[train_embeddings_indexs],
                                          images_embeddings[test_embeddings_indexs], text_embeddings[test_embeddings_indexs],
                                          batch_size_train=BTCH_SIZE, batch_size_test=BTCH_SIZE)


def noise_augmentation(x, variance=0.001):
    """reference :121-126: normalise, add N(0, variance), normalise -- ``train.noise_injection`` without an offset"""
    from .train import noise_injection
    return noise_injection(x, variance)


def _tensors_of(data):
    """-> (x_train, y_train, x_test, y_test) from a pair of loaders over ``TensorDataset``s or from four tensors"""
    data = tuple(data)
    if len(data) == 4:
        return tuple(torch.as_tensor(t).float() for t in data)
    if len(data) == 2:
        sets = [getattr(dl, "dataset", None) for dl in data]
        if all(isinstance(s, torch.utils.data.TensorDataset) and len(s.tensors) == 2 for s in sets):
            return tuple(t.float() for s in sets for t in s.tensors)
    raise CapdecError("train_modal: data must be None, a pair of DataLoaders whose datasets are TensorDatasets of (x, y), or "
                      "four tensors (x_train, y_train, x_test, y_test)")


def train_modal(data=None, epochs=100, lr=0.001, momentum=0.9, batch_size=BTCH_SIZE, out_path=PATH, log=None, engine=None):
    """reference :129-181: train ``MLP(input, input, output, 8)`` (640 wide on the reference's data) with MSELoss and SGD with
    momentum for ``epochs`` passes over the train rows in consecutive batches of ``batch_size`` (at most 64), the validation
    loss after every pass.  One ``capdec_bridger_train_epoch`` and one ``capdec_bridger_eval`` per epoch; the rows stay on
    the device.  ``data``: None (``get_dataloader()``), a pair of loaders over ``TensorDataset``s, or four tensors.  ``log``
    receives exactly the dicts the reference gives ``wandb.log`` -- ``{'epoch', 'train_loss'}`` then ``{'epoch',
    'val_loss'}``, the latter skipped when the test set is empty -- and defaults to ``print``.  Ends with the reference's
    ``print('Finished Training')`` and ``torch.save(model.state_dict(), out_path)``.

    Returns the trained model.  (The reference returns -1.)"""
    x_train, y_train, x_test, y_test = _tensors_of(get_dataloader(engine=engine) if data is None else data)
    if x_train.dim() != 2 or y_train.dim() != 2 or x_train.shape[0] != y_train.shape[0] or x_train.shape[0] < 1:
        raise CapdecError(f"train_modal: the train set must be x [n >= 1, D] and y [n, D'], got {tuple(x_train.shape)} and "
                          f"{tuple(y_train.shape)}")
    if log is None:
        log = print
    model = MLP(int(x_train.shape[1]), int(x_train.shape[1]), int(y_train.shape[1]), 8, engine=engine)
    model.train()
    eng = model.engine
    dev = eng.device
    x_train, y_train, x_test, y_test = (t.to(dev).contiguous() for t in (x_train, y_train, x_test, y_test))
    for epoch in range(epochs):  # loop over the dataset multiple times
        model._device_newer = True
        eng.bridger_train_epoch(x_train, y_train, batch_size, lr, momentum)
        _, running_loss, steps = eng.bridger_loss(reset=True)
        log({'epoch': epoch, 'train_loss': running_loss / steps})

        # valid set
        if x_test.shape[0] == 0:
            continue
        running_loss, batches = eng.bridger_eval(x_test, y_test, batch_size)
        log({'epoch': epoch, 'val_loss': running_loss / batches})

    print('Finished Training')
    torch.save(model.state_dict(), out_path)
    return model


if "__main__" == __name__:
    train_modal()
