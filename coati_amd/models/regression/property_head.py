"""Property heads on embeddings: an FC-ResNet (first Linear, `depth` residual blocks h + relu(Linear(h)), last Linear) that maps an
embedding to a few properties, the way the reference's regressors (coati.models.regression.basic_due) do before their GP head.

    model, (y_true, y_pred, _) = fit_property_head(records, x_field="emb_smiles", y_field="logp")
    model.predict(vectors)                      # [n, P] f32: the fused kernel (include/coati_screen.h, csrc/screen.hip)
    index.screen(model, k=10)                   # the k best rows of an EmbeddingIndex (coati_amd/search.py)

    values, grad = model.value_and_grad(vectors)   # the same values and d values / d vectors: one kernel (include/coati_guide.h, csrc/guide.hip)
    model.fused(x)                              # predict() as a differentiable function of x (torch.autograd.Function over the two kernels)

forward() is plain f32 torch and differentiable: it is what fitting uses (it is the only path that gives gradients to the parameters).
predict() / predict_rows() run one kernel that carries a tile of rows through all layers on the matrix cores; value_and_grad() /
grad_rows() / fused() run its twin, which goes back through the layers for the gradient with respect to the rows; there is no CPU fallback.
reference() / reference_grad() restate the kernels' arithmetic, rounding points included, in torch: the yardstick of the tests."""
import ctypes

import numpy as np
import torch

from ... import _lib

E_MAX = 512
FEATURES = (64, 128, 256)
DEPTH_MAX = 16
OUTPUTS_MAX = 8


def _padded(dim):
    return (dim + 31) // 32 * 32


def _normalised(x):
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-30)


def unit_input_chain(g_u, x):
    """The gradient with respect to x of a function of u = x / |x|, given its gradient g_u with respect to u:
    g_x = (g_u - (g_u . u) u) / |x|, per row, in g_u's dtype."""
    x = x.to(g_u.dtype)
    norm = x.norm(dim=1, keepdim=True).clamp_min(1e-30)
    u = x / norm
    return (g_u - (g_u * u).sum(dim=1, keepdim=True) * u) / norm


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


class PropertyHead(torch.nn.Module):
    def __init__(self, input_dim, features=256, depth=4, num_outputs=1, unit_input=False, dropout_rate=0.0):
        super().__init__()
        input_dim, features, depth, num_outputs = int(input_dim), int(features), int(depth), int(num_outputs)
        if input_dim < 1 or input_dim > E_MAX:
            raise ValueError(f"PropertyHead: input_dim={input_dim} outside 1 .. {E_MAX}")
        if features not in FEATURES:
            raise ValueError(f"PropertyHead: features={features} is not one of {FEATURES}")
        if depth < 0 or depth > DEPTH_MAX:
            raise ValueError(f"PropertyHead: depth={depth} outside 0 .. {DEPTH_MAX}")
        if num_outputs < 1 or num_outputs > OUTPUTS_MAX:
            raise ValueError(f"PropertyHead: num_outputs={num_outputs} outside 1 .. {OUTPUTS_MAX}")
        if not 0.0 <= float(dropout_rate) < 1.0:
            raise ValueError(f"PropertyHead: dropout_rate={dropout_rate} outside [0, 1)")
        self.input_dim, self.features, self.depth, self.num_outputs = input_dim, features, depth, num_outputs
        self.unit_input, self.dropout_rate = bool(unit_input), float(dropout_rate)
        self.first = torch.nn.Linear(input_dim, features)
        self.residuals = torch.nn.ModuleList([torch.nn.Linear(features, features) for _ in range(depth)])
        self.last = torch.nn.Linear(features, num_outputs)
        self.dropout = torch.nn.Dropout(self.dropout_rate)
        self._packed = None             # (key, device tensors) of the kernel's operands

    @property
    def input_dim_padded(self):
        """the width of prepared rows: input_dim up to the next multiple of 32 (zero columns against zero weights)"""
        return _padded(self.input_dim)

    @property
    def device(self):
        return self.first.weight.device

    def hyper(self):
        return dict(input_dim=self.input_dim, features=self.features, depth=self.depth, num_outputs=self.num_outputs,
                    unit_input=self.unit_input, dropout_rate=self.dropout_rate)

    def forward(self, x):
        if self.unit_input:
            x = _normalised(x)
        h = self.first(x)
        for res in self.residuals:
            h = h + self.dropout(torch.relu(res(h)))
        return self.last(h)

    # ---- the kernel's arithmetic ---------------------------------------------------------------------------------------------
    def reference(self, x16, dtype=torch.float64):
        """The kernel's result on prepared bf16 rows x16 [n, input_dim or input_dim_padded], computed in `dtype` with the kernel's
        rounding points: bf16 weights of first and of the residual blocks, the f32 stream rounded to bf16 as the operand of a block's
        product only, everything else (biases, the stream itself, the last layer) unrounded."""
        if x16.dtype != torch.bfloat16 or x16.dim() != 2 or x16.shape[1] not in (self.input_dim, self.input_dim_padded):
            raise ValueError(f"PropertyHead.reference: rows must be bf16 [n, {self.input_dim} or {self.input_dim_padded}], "
                             f"got {x16.dtype} {tuple(x16.shape)}")

        def rb(t):
            return t.detach().to(torch.float32).to(torch.bfloat16).to(dtype)

        with torch.no_grad():
            h = x16[:, :self.input_dim].to(dtype) @ rb(self.first.weight).T + self.first.bias.to(dtype)
            for res in self.residuals:
                h = h + torch.relu(rb(h) @ rb(res.weight).T + res.bias.to(dtype))
            return h @ self.last.weight.to(dtype).T + self.last.bias.to(dtype)

    def reference_grad(self, x16, cot, dtype=torch.float64, round_fn=None):
        """(out [n, P], g [n, width of x16]) of coati_head_grad on prepared bf16 rows, computed in `dtype` with the kernel's rounding points:
        the forward of reference(), whose pre-activations give the masks m[l] = (z_l > 0); then d = cot . wl, d = d + rb(m[l] (.) d) . rb(wr[l])
        for l = D - 1 .. 0 (d itself unrounded) and g = rb(d) . rb(w0).  round_fn (tensor -> tensor of `dtype`) replaces rb, the rounding to
        bf16, everywhere: with a plain cast this is the gradient of forward() in `dtype`."""
        if x16.dtype != torch.bfloat16 or x16.dim() != 2 or x16.shape[1] not in (self.input_dim, self.input_dim_padded):
            raise ValueError(f"PropertyHead.reference_grad: rows must be bf16 [n, {self.input_dim} or {self.input_dim_padded}], "
                             f"got {x16.dtype} {tuple(x16.shape)}")
        if cot.dim() != 2 or tuple(cot.shape) != (x16.shape[0], self.num_outputs):
            raise ValueError(f"PropertyHead.reference_grad: the cotangent must be [{x16.shape[0]}, {self.num_outputs}], got {tuple(cot.shape)}")

        def rb(t):
            return t.detach().to(torch.float32).to(torch.bfloat16).to(dtype)

        rb = round_fn if round_fn is not None else rb
        with torch.no_grad():
            w0 = rb(self.first.weight)
            wr = [rb(res.weight) for res in self.residuals]
            wl = self.last.weight.to(dtype)
            h = x16[:, :self.input_dim].to(dtype) @ w0.T + self.first.bias.to(dtype)
            masks = []
            for res, w in zip(self.residuals, wr):
                z = rb(h) @ w.T + res.bias.to(dtype)
                masks.append(z > 0)
                h = h + torch.relu(z)
            out = h @ wl.T + self.last.bias.to(dtype)
            d = cot.to(dtype) @ wl
            for m, w in zip(reversed(masks), reversed(wr)):
                d = d + rb(torch.where(m, d, torch.zeros_like(d))) @ w
            g = rb(d) @ w0
            return out, torch.nn.functional.pad(g, (0, x16.shape[1] - self.input_dim))

    def prepare(self, vectors):
        """vectors [n, input_dim] (any float dtype, any device) as the kernel reads them: on the head's device, normalised in f32 if
        unit_input, rounded to bf16, zero-padded to input_dim_padded columns"""
        x = torch.as_tensor(vectors)
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2 or x.shape[1] != self.input_dim:
            raise ValueError(f"PropertyHead: vectors must be [n, {self.input_dim}], got {tuple(x.shape)}")
        x = x.detach().to(device=self.device, dtype=torch.float32)
        if self.unit_input:
            x = _normalised(x)
        x16 = x.to(torch.bfloat16)
        pad = self.input_dim_padded - self.input_dim
        return (torch.nn.functional.pad(x16, (0, pad)) if pad else x16).contiguous()

    def _operands(self):
        params = list(self.parameters())
        key = tuple((p.data_ptr(), p._version) for p in params)
        if self._packed is None or self._packed[0] != key:
            with torch.no_grad():
                w0 = torch.nn.functional.pad(self.first.weight.to(torch.bfloat16), (0, self.input_dim_padded - self.input_dim)).contiguous()
                b0 = self.first.bias.float().contiguous().clone()
                if self.depth:
                    wr = torch.stack([r.weight.to(torch.bfloat16) for r in self.residuals]).contiguous()
                    br = torch.stack([r.bias.float() for r in self.residuals]).contiguous()
                else:
                    wr = br = None
                wl = self.last.weight.float().contiguous().clone()
                bl = self.last.bias.float().contiguous().clone()
                w0t = w0.T.contiguous()                                      # the backward's operands: [E, F] and [D, F, F], transposed
                wrt = wr.transpose(1, 2).contiguous() if self.depth else None
            self._packed = (key, (w0, b0, wr, br, wl, bl), (w0t, wrt))
        return self._packed[1]

    def _grad_operands(self):
        """(w0t, wrt): w0 and every wr[l] transposed, packed with _operands() under the same cache key"""
        self._operands()
        return self._packed[2]

    def _kernel_rows(self, x16, what):
        """x16 as the kernels read it (predict_rows' stride rules), and its row stride"""
        E = self.input_dim_padded
        if not isinstance(x16, torch.Tensor) or x16.dtype != torch.bfloat16 or x16.dim() != 2 or x16.shape[1] != E:
            raise ValueError(f"PropertyHead.{what}: rows must be a bf16 tensor [n, {E}]")
        if x16.device != self.device:
            raise ValueError(f"PropertyHead.{what}: rows on {x16.device}, the head on {self.device}")
        n = x16.shape[0]
        if n > 1 and (x16.stride(1) != 1 or x16.stride(0) < E or x16.stride(0) % 8 or x16.data_ptr() % 16):
            x16 = x16.contiguous()
        elif n == 1 and (x16.stride(1) != 1 or x16.data_ptr() % 16):
            x16 = x16.contiguous()
        return x16, (x16.stride(0) if n > 1 else E)

    def grad_rows(self, x16, cot):
        """(out [n, P], g [n, input_dim_padded]) f32 of prepared rows: out as predict_rows gives it, bit for bit, and g the gradient of
        sum_p cot[:, p] * out[:, p] with respect to the rows as the kernel reads them -- one launch of coati_head_grad.  x16 under
        predict_rows' stride rules; cot [n, P] (made f32 and contiguous).  There is no CPU fallback."""
        x16, ldx = self._kernel_rows(x16, "grad_rows")
        n, E, P = x16.shape[0], self.input_dim_padded, self.num_outputs
        if not isinstance(cot, torch.Tensor) or cot.dim() != 2 or tuple(cot.shape) != (n, P):
            raise ValueError(f"PropertyHead.grad_rows: the cotangent must be a tensor [{n}, {P}]")
        if cot.device != self.device:
            raise ValueError(f"PropertyHead.grad_rows: the cotangent on {cot.device}, the head on {self.device}")
        out = torch.empty(n, P, dtype=torch.float32, device=self.device)
        g = torch.empty(n, E, dtype=torch.float32, device=self.device)
        if n == 0:
            return out, g
        if self.device.type != "cuda":
            raise RuntimeError("PropertyHead.grad_rows: the head is not on a GPU; there is no CPU fallback (forward() is plain torch)")
        cot = cot.detach().to(torch.float32).contiguous()
        w0, b0, wr, br, wl, bl = self._operands()
        w0t, wrt = self._grad_operands()
        with torch.cuda.device(self.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.call("coati_head_grad", _ptr(x16), ldx, n, E, _ptr(w0), _ptr(b0), _ptr(wr), _ptr(br), self.depth, _ptr(wl), _ptr(bl), P,
                      self.features, _ptr(w0t), _ptr(wrt), _ptr(cot), P, _ptr(out), P, _ptr(g), E, stream)
        return out, g

    def _cotangent(self, cotangent, n):
        """None (ones), [P] weights or [n, P] -> [n, P] f32 on the head's device"""
        P = self.num_outputs
        if cotangent is None:
            return torch.ones(n, P, dtype=torch.float32, device=self.device)
        c = torch.as_tensor(cotangent).detach().to(device=self.device, dtype=torch.float32)
        if c.dim() == 1 and c.shape[0] == P:
            return c[None].expand(n, P).contiguous()
        if c.dim() == 2 and tuple(c.shape) == (n, P):
            return c.contiguous()
        raise ValueError(f"PropertyHead: the cotangent must be None, [{P}] or [{n}, {P}], got {tuple(c.shape)}")

    def value_and_grad(self, vectors, cotangent=None):
        """(values [n, P], grad [n, input_dim]) f32 on the head's device: predict(vectors) and the gradient of sum_p c[p] * values[:, p]
        with respect to the vectors, one kernel call (coati_head_grad on prepare(vectors)).  cotangent: None (ones), a [P] vector of
        weights, or [n, P].  The gradient is that of the function predict() computes on the prepared rows -- it does not see the rounding
        of the input to bf16; with unit_input the chain through the normalisation is unit_input_chain, in f32 torch."""
        x = torch.as_tensor(vectors)
        if x.dim() == 1:
            x = x[None]
        with torch.no_grad():
            x16 = self.prepare(x)
            cot = self._cotangent(cotangent, x16.shape[0])
            out, g = self.grad_rows(x16, cot)
            g = g[:, :self.input_dim]
            if self.unit_input:
                g = unit_input_chain(g, x.detach().to(device=self.device, dtype=torch.float32))
            return out, g.contiguous()

    def fused(self, x):
        """predict(x) [n, P] as a differentiable function of x [n, input_dim] (models/autograd_funs/property.py): the forward is
        coati_head_eval, the backward one coati_head_grad call with grad_output as the cotangent plus the chain of unit_input.  Gradients
        flow to x ONLY: the head's parameters are constants here and receive none (fit with forward()).  What lets a property term and
        hclip_likelihood / hcoati_likelihood stand in one torch objective."""
        from ..autograd_funs.property import head_fused
        return head_fused(x, self)

    def predict_rows(self, x16):
        """[n, P] f32 of prepared rows: x16 [n, input_dim_padded] bf16 on the head's device (e.g. EmbeddingIndex.vectors).  Rows may be
        strided (a multiple of 8 elements); anything else is made contiguous first."""
        x16, ldx = self._kernel_rows(x16, "predict_rows")
        n, E = x16.shape[0], self.input_dim_padded
        out = torch.empty(n, self.num_outputs, dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        if self.device.type != "cuda":
            raise RuntimeError("PropertyHead.predict_rows: the head is not on a GPU; there is no CPU fallback (forward() is plain torch)")
        w0, b0, wr, br, wl, bl = self._operands()
        with torch.cuda.device(self.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.call("coati_head_eval", _ptr(x16), ldx, n, E, _ptr(w0), _ptr(b0), _ptr(wr), _ptr(br), self.depth, _ptr(wl), _ptr(bl),
                      self.num_outputs, self.features, _ptr(out), self.num_outputs, stream)
        return out

    def predict(self, vectors):
        """[n, P] f32 on the head's device: the kernel on prepare(vectors).  Inference only (no dropout, no gradient)."""
        with torch.no_grad():
            return self.predict_rows(self.prepare(vectors))

    # ---- files -----------------------------------------------------------------------------------------------------------------
    def save(self, path):
        torch.save({"hyper": self.hyper(), "state_dict": {k: v.detach().cpu() for k, v in self.state_dict().items()}}, path)

    @classmethod
    def load(cls, path, device="cpu"):
        d = torch.load(path, map_location="cpu")
        model = cls(**d["hyper"])
        model.load_state_dict(d["state_dict"])
        return model.to(device).eval()


def fit_property_head(dataset, x_field="emb_smiles", y_field="pic50", steps=1e5, depth=4, batch_size=512, test_frac=0.03, random_seed=510,
                      lr=1e-3, features=256, unit_input=False, device=None):
    """Fits a PropertyHead to records: x = record[x_field] (an embedding), y = record[y_field] (y_field may be a list of fields: one
    output each).  basic_due's arguments where they still mean something, and its split: np.random.seed(random_seed), one permutation,
    the first int(test_frac * n) records are the test set.  Adam on the mean squared error for `steps` steps of shuffled batches.

    Returns (model, (Xs, Ys, None)): the test targets, the model's predictions on the test set, and None where basic_due returns
    standard deviations: fit_gp_head (gp_head.py) puts a GP head on this extractor and fills that slot.  What is NOT here: spectral
    normalisation of the feature extractor."""
    np.random.seed(seed=random_seed)
    x = np.stack([np.asarray(r[x_field]) for r in dataset], 0)
    if isinstance(y_field, (list, tuple)):
        y = np.stack([np.stack([np.asarray(r[f]) for f in y_field], -1) for r in dataset], 0)
    else:
        y = np.stack([np.asarray(r[y_field]) for r in dataset], 0)
    n = x.shape[0]
    perm = np.random.permutation(n)
    n_test = int(test_frac * n)
    test_idx, train_idx = perm[:n_test], perm[n_test:]
    device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
    X = torch.tensor(x, dtype=torch.float32).reshape(n, -1)
    Y = torch.tensor(y, dtype=torch.float32).reshape(n, -1)
    train_x, train_y = X[train_idx].to(device), Y[train_idx].to(device)
    gen = torch.Generator().manual_seed(int(random_seed))
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(random_seed))
        model = PropertyHead(X.shape[1], features=features, depth=depth, num_outputs=Y.shape[1], unit_input=unit_input).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    model.train()
    step, steps = 0, int(steps)
    while step < steps:
        order = torch.randperm(train_x.shape[0], generator=gen).to(device)
        for lo in range(0, order.numel(), batch_size):
            if step >= steps:
                break
            idx = order[lo:lo + batch_size]
            opt.zero_grad()
            loss = torch.nn.functional.mse_loss(model(train_x[idx]), train_y[idx])
            loss.backward()
            opt.step()
            step += 1
    model.eval()
    with torch.no_grad():
        pred = model(X[test_idx].to(device)).cpu().numpy()
    return model, (y[test_idx], pred.reshape(y[test_idx].shape), None)
