"""The supervised modality bridger's contract (include/capdec.h: capdec_bridger_*) restated in fp64 numpy, in this project's
words: an MLP of L Linear layers in nn.Linear layout with ReLU after every layer but the last, the mean-squared-error loss,
its gradient, and SGD with momentum (dampening 0, no Nesterov, no weight decay; the momentum buffer starts at zero, which
is torch's ``buf = grad`` on the first step).  The tests compare the HIP kernels, the torch-fp32 arithmetic of the reference
and the recorded reference runs against this.

The bound for a compared tensor q: ``4 * floor_q + 2.4e-7 * max |def_q|`` with ``floor_q = max |torch fp32 - definition|`` on
the same inputs -- another fp32 summation order deviates by the same order of magnitude as the reference's own, and the second
term is two fp32 ulps at the tensor's scale for entries the reference happens to get exactly.
"""
import numpy as np

ULP2 = 2.4e-7


def f64(a):
    return np.asarray(a, dtype=np.float64)


class Bridger:
    """parameters ``w[l]`` [dims[l + 1], dims[l]], ``b[l]`` [dims[l + 1]], momentum buffers ``vw``, ``vb`` (zero at the start),
    the loss scalars of capdec_bridger_loss"""

    def __init__(self, weights, biases):
        self.w = [f64(w).copy() for w in weights]
        self.b = [f64(b).copy() for b in biases]
        self.vw = [np.zeros_like(w) for w in self.w]
        self.vb = [np.zeros_like(b) for b in self.b]
        self.L = len(self.w)
        self.dims = [self.w[0].shape[1]] + [w.shape[0] for w in self.w]
        self.last, self.sum, self.steps = 0.0, 0.0, 0
        self.steps_since_load = 0
        self.acts = None

    def copy(self):
        c = Bridger(self.w, self.b)
        c.vw = [v.copy() for v in self.vw]
        c.vb = [v.copy() for v in self.vb]
        c.last, c.sum, c.steps = self.last, self.sum, self.steps
        c.steps_since_load = self.steps_since_load
        return c

    # ---- forward: (pre-activations z_l, post-activations h_l); h_{L-1} = z_{L-1} is the output
    def forward_all(self, x):
        h, zs, hs = f64(x), [], []
        for l in range(self.L):
            z = h @ self.w[l].T + self.b[l]
            h = np.maximum(z, 0.0) if l < self.L - 1 else z
            zs.append(z)
            hs.append(h)
        return zs, hs

    def forward(self, x):
        return self.forward_all(x)[1][-1]

    @staticmethod
    def loss(out, y):
        d = f64(out) - f64(y)
        return float(np.mean(d * d))

    # ---- backward: gradients of the loss; masks[l] (bool [batch, dims[l + 1]], l < L - 1) stands for relu'(z_l); default z_l > 0
    def backward(self, x, y, masks=None, drop_row_from_dw=None):
        zs, hs = self.forward_all(x)
        out = hs[-1]
        d = 2.0 * (out - f64(y)) / out.size
        gw, gb = [None] * self.L, [None] * self.L
        for l in range(self.L - 1, -1, -1):
            inp = hs[l - 1] if l else f64(x)
            if drop_row_from_dw is None:
                gw[l] = d.T @ inp
            else:                                   # a WRONG gradient, for the sensitivity test: one batch row left out
                keep = np.arange(d.shape[0]) != drop_row_from_dw
                gw[l] = d[keep].T @ inp[keep]
            gb[l] = d.sum(0)
            if l:
                m = (zs[l - 1] > 0.0) if masks is None else np.asarray(masks[l - 1], dtype=bool)
                d = (d @ self.w[l]) * m
        return gw, gb, zs, hs

    # ---- one train step (capdec_bridger_train_step) -> the loss before the update
    def train_step(self, x, y, lr, momentum, masks=None, wrong=None):
        gw, gb, zs, hs = self.backward(x, y, masks, drop_row_from_dw=0 if wrong == "drop_row" else None)
        loss = self.loss(hs[-1], y)
        first = self.steps_since_load == 0
        for l in range(self.L):
            for v, g, p in ((self.vw, gw, self.w), (self.vb, gb, self.b)):
                if wrong == "first_step_momentum" and first:      # a WRONG first step: v = g (1 - momentum)
                    v[l] = g[l] * (1.0 - momentum)
                else:
                    v[l] = momentum * v[l] + g[l]
                p[l] = p[l] - lr * v[l]
        self.steps_since_load += 1
        self.acts, self.zs = hs, zs
        self.last = float(np.float32(loss))         # the loss leaves the device as fp32 ...
        self.sum += self.last                       # ... and the running sum adds those in fp64
        self.steps += 1
        return loss

    def train_epoch(self, x, y, batch, lr, momentum):
        for r0 in range(0, len(x), batch):          # consecutive slices, the last one possibly short
            self.train_step(x[r0:r0 + batch], y[r0:r0 + batch], lr, momentum)

    def evaluate(self, x, y, batch):
        """(sum of the fp32-rounded batch losses, number of batches) -- capdec_bridger_eval"""
        out = self.forward(x)
        losses = [float(np.float32(self.loss(out[r0:r0 + batch], y[r0:r0 + batch]))) for r0 in range(0, len(x), batch)]
        return float(np.sum(losses)), len(losses)

    def read_loss(self, reset=False):
        r = (self.last, self.sum, self.steps)
        if reset:
            self.sum, self.steps = 0.0, 0
        return r


def bound(floor, def_q):
    """4 floor + two fp32 ulps at the tensor's scale"""
    return 4.0 * float(floor) + ULP2 * float(np.max(np.abs(def_q))) if np.size(def_q) else 4.0 * float(floor)


def deviation(got, want):
    got, want = f64(got), f64(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want))) if got.size else 0.0


def masks_agree(h_got, z_def, fwd_bound):
    """the device's ReLU masks (h > 0) may differ from the definition's (z > 0) only where |z_def| <= that layer's forward
    bound -> the number of such units; anything else is an assertion"""
    mg, md = f64(h_got) > 0.0, f64(z_def) > 0.0
    diff = mg != md
    assert np.all(np.abs(f64(z_def))[diff] <= fwd_bound), "a ReLU mask differs at a unit that is not within rounding of zero"
    return int(diff.sum())


# ---- the reference's data split (others/supervised_embedding_bridger.py:33-67) on rows that are already normalised
def split_rows(image_ids, clip_index):
    """captions = the pickle's list WITHOUT its last entry: (test row numbers, train row numbers) -- a stable sort by image id,
    the first int(0.2 * len) captions are the test set, rows picked through each caption's ``clip_embedding`` index"""
    order = sorted(range(len(image_ids)), key=lambda i: image_ids[i])
    cut = int(len(image_ids) * 0.2)
    pick = [int(clip_index[i]) for i in order]
    return pick[:cut], pick[cut:]
