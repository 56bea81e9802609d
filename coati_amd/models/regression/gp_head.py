"""A Gaussian-process head on inducing points over a PropertyHead's features: predictions WITH standard deviations, what the reference's
DUE regressors (coati.models.regression.basic_due) return as (Xs, Ys, dYs).

    gp, (y_true, y_pred, y_std) = fit_gp_head(records, x_field="emb_smiles", y_field="logp")
    mean, std = gp.predict_with_std(vectors)    # [n, P] f32 each: one fused kernel (include/coati_gp.h, csrc/gp.hip)
    index.screen(gp, k=10, acquisition="ucb", beta=2.0)     # an EmbeddingIndex ranked by mean + 2 std (coati_amd/search.py)

The model: phi(x) = the extractor's last stream rounded to bf16, an RBF kernel k(a, b) = s2 exp(-|a - b|^2 / (2 l^2)) on phi, M <= 64
inducing points Z shared by all P outputs, a constant mean, one Gaussian noise on standardised targets.  For a Gaussian likelihood the
optimal variational distribution over the inducing values has a closed form (Titsias' collapsed bound), so fitting needs neither gpytorch
nor a variational training loop: three hyper-parameters are optimised on the bound, the posterior follows from linear algebra.  Prediction
is

    mean_p = c_p + sum_j alpha[p, j] k(phi, z_j)        var = s2 - sum_ij k(phi, z_i) q[i, j] k(phi, z_j)

with alpha = Kzz^-1 m and q = Kzz^-1 - Kzz^-1 S Kzz^-1 for an inducing distribution N(m, S).  predict*() run the kernel, there is no
CPU fallback; reference() restates the kernel's arithmetic in torch, rounding points included: the yardstick of the tests."""
import copy
import ctypes
import math
import warnings

import numpy as np
import torch

from ... import _lib
from .property_head import PropertyHead, _ptr, fit_property_head

INDUCING_MAX = 64
ACQUISITIONS = ("mean", "ucb", "lcb", "ei")


def rbf_kernel(a, b, lengthscale, signal_var):
    """[n, m] = signal_var * exp(-|a_i - b_j|^2 / (2 lengthscale^2)), in a's dtype"""
    d2 = ((a * a).sum(dim=1)[:, None] + (b * b).sum(dim=1)[None, :] - 2.0 * a @ b.T).clamp_min(0.0)
    return signal_var * torch.exp(-d2 / (2.0 * lengthscale ** 2))


def collapsed_bound(phi, y, z, lengthscale, signal_var, noise_var, jitter=1e-6):
    """Titsias' collapsed evidence lower bound of a sparse GP with inducing points z on (phi [n, F], y [n, P]): the P outputs share the
    kernel and the noise.  sum_p log N(y_p | 0, Qff + noise I) - P / (2 noise) tr(Kff - Qff), Qff = Kfz Kzz^-1 Kzf; differentiable in
    the three hyper-parameters (tensors or floats).  jitter * signal_var is added to Kzz's diagonal."""
    n, P, M = phi.shape[0], y.shape[1], z.shape[0]
    Kzz = rbf_kernel(z, z, lengthscale, signal_var) + jitter * signal_var * torch.eye(M, dtype=phi.dtype, device=phi.device)
    Kzf = rbf_kernel(z, phi, lengthscale, signal_var)
    L = torch.linalg.cholesky(Kzz)
    A = torch.linalg.solve_triangular(L, Kzf, upper=False) / noise_var ** 0.5
    AAT = A @ A.T
    LB = torch.linalg.cholesky(AAT + torch.eye(M, dtype=phi.dtype, device=phi.device))
    c = torch.linalg.solve_triangular(LB, A @ y, upper=False) / noise_var ** 0.5
    log_noise = torch.log(noise_var) if isinstance(noise_var, torch.Tensor) else math.log(noise_var)
    bound = -0.5 * n * P * math.log(2.0 * math.pi) - P * torch.log(torch.diagonal(LB)).sum() - 0.5 * n * P * log_noise
    bound = bound - 0.5 * (y * y).sum() / noise_var + 0.5 * (c * c).sum()
    return bound - 0.5 * P * n * signal_var / noise_var + 0.5 * P * torch.diagonal(AAT).sum()


def collapsed_posterior(phi, y, z, lengthscale, signal_var, noise_var, jitter=1e-6):
    """The optimal inducing distribution of the collapsed bound, packed for prediction: Sigma = (Kzz + Kzf Kfz / noise)^-1,
    alpha [P, M] = Sigma Kzf y / noise, q [M, M] = Kzz^-1 - Sigma.  In phi's dtype (use float64).  Returns (alpha, q, Sigma, Kzz)."""
    M = z.shape[0]
    Kzz = rbf_kernel(z, z, lengthscale, signal_var) + jitter * signal_var * torch.eye(M, dtype=phi.dtype, device=phi.device)
    Kzf = rbf_kernel(z, phi, lengthscale, signal_var)
    inner = Kzz + Kzf @ Kzf.T / noise_var
    Sigma = torch.linalg.inv(0.5 * (inner + inner.T))
    Sigma = 0.5 * (Sigma + Sigma.T)
    Kinv = torch.linalg.inv(Kzz)
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha = (Sigma @ (Kzf @ y)).T / noise_var
    return alpha, Kinv - Sigma, Sigma, Kzz


def acquisition_values(mean, std, acquisition, beta=1.0, best=None):
    """The acquisition of a screen from a mean and a standard deviation (tensors of one shape): "mean"; "ucb" = mean + beta std; "lcb" =
    mean - beta std; "ei" = the expected improvement over `best`, (mean - best) Phi(u) + std phi(u) with u = (mean - best) / std, and
    max(mean - best, 0) where std == 0."""
    if acquisition is None or acquisition == "mean":
        return mean
    if acquisition == "ucb":
        return mean + float(beta) * std
    if acquisition == "lcb":
        return mean - float(beta) * std
    if acquisition == "ei":
        if best is None:
            raise ValueError("acquisition 'ei' needs best=, the value to improve on")
        d = mean - float(best)
        safe = torch.where(std > 0, std, torch.ones_like(std))
        u = d / safe
        ei = d * 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + std * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
        return torch.where(std > 0, ei, d.clamp_min(0.0))
    raise ValueError(f"acquisition={acquisition!r} is not one of {ACQUISITIONS}")


def extractor_features(ex, x16, dtype=torch.float64):
    """phi [n, F] in `dtype` of prepared bf16 rows: PropertyHead.reference's stream after the residual blocks (its rounding points),
    rounded to bf16"""
    if x16.dtype != torch.bfloat16 or x16.dim() != 2 or x16.shape[1] not in (ex.input_dim, ex.input_dim_padded):
        raise ValueError(f"GPHead.features_reference: rows must be bf16 [n, {ex.input_dim} or {ex.input_dim_padded}], "
                         f"got {x16.dtype} {tuple(x16.shape)}")

    def rb(t):
        return t.detach().to(torch.float32).to(torch.bfloat16).to(dtype)

    with torch.no_grad():
        h = x16[:, :ex.input_dim].to(dtype) @ rb(ex.first.weight).T + ex.first.bias.to(dtype)
        for res in ex.residuals:
            h = h + torch.relu(rb(h) @ rb(res.weight).T + res.bias.to(dtype))
        return rb(h)


class GPHead(torch.nn.Module):
    """extractor: a PropertyHead (copied and frozen; its last layer is not part of the GP).  z [M, F] inducing points (rounded to bf16: the
    model's Z is the kernel's Z), alpha [P, M], q [M, M] (any matrix), const [P], on STANDARDISED targets; lengthscale, signal_var,
    noise_var floats; y_mean, y_scale [P] (default 0 and 1) undo the standardisation: mean = y_mean + y_scale * (const + alpha . k),
    std = y_scale * sqrt(var).  1 <= M <= 64.  Everything is a buffer: nothing is trained through this class."""

    has_input_gradient = False

    def __init__(self, extractor, z, alpha, q, const, lengthscale, signal_var, noise_var, y_mean=None, y_scale=None):
        super().__init__()
        if not isinstance(extractor, PropertyHead):
            raise TypeError("GPHead: extractor must be a PropertyHead")
        z, alpha, q = torch.as_tensor(z), torch.as_tensor(alpha), torch.as_tensor(q)
        if z.dim() != 2 or z.shape[1] != extractor.features or not 1 <= z.shape[0] <= INDUCING_MAX:
            raise ValueError(f"GPHead: z must be [M, {extractor.features}] with 1 <= M <= {INDUCING_MAX}, got {tuple(z.shape)}")
        M = z.shape[0]
        if alpha.dim() != 2 or alpha.shape[1] != M or not 1 <= alpha.shape[0] <= 8:
            raise ValueError(f"GPHead: alpha must be [P, {M}] with 1 <= P <= 8, got {tuple(alpha.shape)}")
        P = alpha.shape[0]
        if tuple(q.shape) != (M, M):
            raise ValueError(f"GPHead: q must be [{M}, {M}], got {tuple(q.shape)}")
        if not (float(lengthscale) > 0 and float(signal_var) > 0 and float(noise_var) >= 0):
            raise ValueError(f"GPHead: lengthscale={lengthscale} and signal_var={signal_var} must be positive, noise_var={noise_var} not negative")

        def vec(t, default, name):
            t = torch.full((P,), default, dtype=torch.float64) if t is None else torch.as_tensor(t, dtype=torch.float64).reshape(-1)
            if t.shape[0] != P:
                raise ValueError(f"GPHead: {name} must be [{P}], got {tuple(t.shape)}")
            return t.detach().clone()

        self.extractor = copy.deepcopy(extractor).eval().requires_grad_(False)
        self.extractor._packed = None
        dev = self.extractor.device
        self.register_buffer("z", z.detach().to(torch.float32).to(torch.bfloat16).to(dev))
        self.register_buffer("alpha", alpha.detach().to(torch.float64).clone().to(dev))
        self.register_buffer("q", q.detach().to(torch.float64).clone().to(dev))
        self.register_buffer("const", vec(const, 0.0, "const").to(dev))
        self.register_buffer("y_mean", vec(y_mean, 0.0, "y_mean").to(dev))
        self.register_buffer("y_scale", vec(y_scale, 1.0, "y_scale").to(dev))
        self.lengthscale, self.signal_var, self.noise_var = float(lengthscale), float(signal_var), float(noise_var)
        self.fit_info = {}
        self._gp_packed = None

    # ---- what callers of a PropertyHead ask for -----------------------------------------------------------------------------------
    input_dim = property(lambda self: self.extractor.input_dim)
    input_dim_padded = property(lambda self: self.extractor.input_dim_padded)
    features = property(lambda self: self.extractor.features)
    depth = property(lambda self: self.extractor.depth)
    unit_input = property(lambda self: self.extractor.unit_input)
    num_outputs = property(lambda self: self.alpha.shape[0])
    num_inducing = property(lambda self: self.z.shape[0])
    device = property(lambda self: self.extractor.device)

    def prepare(self, vectors):
        return self.extractor.prepare(vectors)

    def gp_hyper(self):
        return dict(lengthscale=self.lengthscale, signal_var=self.signal_var, noise_var=self.noise_var)

    # ---- the kernel's arithmetic ----------------------------------------------------------------------------------------------------
    def features_reference(self, x16, dtype=torch.float64):
        """phi [n, F] in `dtype`: the extractor's stream after its residual blocks, with PropertyHead.reference's rounding points, rounded
        to bf16 -- the point the GP is defined on."""
        return extractor_features(self.extractor, x16, dtype)

    def _folded(self):
        """(alpha, const) with the standardisation folded in, float64: what the kernel's alpha and c are rounded from"""
        return self.alpha * self.y_scale[:, None], self.y_mean + self.y_scale * self.const

    def reference(self, x16, dtype=torch.float64, f32_operands=True):
        """(mean [n, P], var [n]) of coati_head_gp on prepared bf16 rows, computed in `dtype` with the kernel's rounding points: phi as
        features_reference gives it, d2 = max(0, |phi|^2 + zn - 2 phi . z), k = s2 exp(-d2 / (2 l^2)) unrounded, mean = c + alpha . k,
        var = max(0, s2 - k q k).  f32_operands (default): alpha, c, q, zn and the two scalars are the f32 values the kernel is given --
        rounding them is a rounding point like the bf16 weights are.  False: the stored float64 values, the model before it is packed."""
        phi = self.features_reference(x16, dtype)
        with torch.no_grad():
            z = self.z.to(dtype)
            alpha, c = self._folded()
            q, zn = self.q, (self.z.double() ** 2).sum(dim=1)
            inv2l2, s2 = 1.0 / (2.0 * self.lengthscale ** 2), self.signal_var
            if f32_operands:
                alpha, c, q, zn = alpha.float(), c.float(), q.float(), zn.float()
                inv2l2, s2 = float(np.float32(inv2l2)), float(np.float32(s2))
            alpha, c, q, zn = alpha.to(dtype), c.to(dtype), q.to(dtype), zn.to(dtype)
            d2 = ((phi * phi).sum(dim=1)[:, None] + zn[None, :] - 2.0 * (phi @ z.T)).clamp_min(0.0)
            k = s2 * torch.exp(-d2 * inv2l2)
            mean = c[None, :] + k @ alpha.T
            var = (s2 - ((k @ q.T) * k).sum(dim=1)).clamp_min(0.0)
            return mean, var

    def std_from_var(self, var, include_noise=False):
        """[n, P]: y_scale * sqrt(var (+ noise_var)), in var's dtype"""
        v = var + self.noise_var if include_noise else var
        return self.y_scale.to(var.dtype)[None, :] * v.clamp_min(0.0).sqrt()[:, None]

    # ---- the kernel -----------------------------------------------------------------------------------------------------------------
    def _gp_operands(self):
        """(z [Mp, F] bf16, zn [Mp], alpha [P, Mp], q [Mp, Mp], c [P]) f32 on the device, padded to Mp = 32 or 64 with zeros: a padded
        point has zero alpha and a zero row and column of q"""
        key = tuple((b.data_ptr(), b._version) for b in (self.z, self.alpha, self.q, self.const, self.y_mean, self.y_scale))
        if self._gp_packed is None or self._gp_packed[0] != key:
            M = self.z.shape[0]
            Mp = 32 if M <= 32 else 64
            with torch.no_grad():
                alpha, c = self._folded()
                z = torch.nn.functional.pad(self.z.to(torch.bfloat16), (0, 0, 0, Mp - M)).contiguous()
                zn = torch.nn.functional.pad((self.z.double() ** 2).sum(dim=1).float(), (0, Mp - M)).contiguous()
                alpha = torch.nn.functional.pad(alpha.float(), (0, Mp - M)).contiguous()
                q = torch.nn.functional.pad(self.q.float(), (0, Mp - M, 0, Mp - M)).contiguous()
                c = c.float().contiguous()
                zt = z.T.contiguous()                                        # the acquisition gradient's operands: z transposed [F, Mp] and
                qs = torch.nn.functional.pad((0.5 * (self.q.double() + self.q.double().T)).float(), (0, Mp - M, 0, Mp - M)).contiguous()
            self._gp_packed = (key, (z, zn, alpha, q, c, Mp), (zt, qs))     # the symmetric part of q, formed in float64
        return self._gp_packed[1]

    def _gp_grad_operands(self):
        """(zt [F, Mp] bf16, qs [Mp, Mp] f32): z transposed and the symmetric part of q, packed with _gp_operands() under the same cache key"""
        self._gp_operands()
        return self._gp_packed[2]

    def gp_rows(self, x16, linear=False):
        """(mean [n, P], var [n]) f32 of prepared rows, one launch of coati_head_gp; linear=True: (mean, var, out) with out [n, P_lin] the
        extractor's own linear prediction from the same pass (coati_head_eval's numbers, bit for bit).  x16 under PropertyHead.predict_rows'
        stride rules.  There is no CPU fallback."""
        ex = self.extractor
        x16, ldx = ex._kernel_rows(x16, "gp_rows")
        n, E, P = x16.shape[0], ex.input_dim_padded, self.num_outputs
        mean = torch.empty(n, P, dtype=torch.float32, device=self.device)
        var = torch.empty(n, dtype=torch.float32, device=self.device)
        out = torch.empty(n, ex.num_outputs, dtype=torch.float32, device=self.device) if linear else None
        if n > 0:
            if self.device.type != "cuda":
                raise RuntimeError("GPHead.gp_rows: the head is not on a GPU; there is no CPU fallback (reference() is plain torch)")
            w0, b0, wr, br, wl, bl = ex._operands()
            z, zn, alpha, q, c, Mp = self._gp_operands()
            with torch.cuda.device(self.device):
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                _lib.call("coati_head_gp", _ptr(x16), ldx, n, E, _ptr(w0), _ptr(b0), _ptr(wr), _ptr(br), ex.depth, ex.features,
                          _ptr(wl if linear else None), _ptr(bl if linear else None), ex.num_outputs, _ptr(out), ex.num_outputs,
                          _ptr(z), _ptr(zn), _ptr(alpha), _ptr(q), _ptr(c), 1.0 / (2.0 * self.lengthscale ** 2), self.signal_var, P, Mp,
                          _ptr(mean), P, _ptr(var), stream)
        return (mean, var, out) if linear else (mean, var)

    def predict_rows(self, x16):
        """mean [n, P] f32 of prepared rows: PropertyHead.predict_rows' contract"""
        return self.gp_rows(x16)[0]

    def predict_rows_with_std(self, x16, include_noise=False):
        """(mean, std), both [n, P] f32: std[:, p] = y_scale[p] * sqrt(var), the latent standard deviation (the reference's pred.stddev);
        include_noise=True adds noise_var under the root"""
        mean, var = self.gp_rows(x16)
        return mean, self.std_from_var(var, include_noise)

    def predict(self, vectors):
        """mean [n, P] f32 on the head's device: PropertyHead.predict's contract, so callers that index [:, output] work unchanged"""
        with torch.no_grad():
            return self.predict_rows(self.prepare(vectors))

    def predict_with_std(self, vectors, include_noise=False):
        with torch.no_grad():
            return self.predict_rows_with_std(self.prepare(vectors), include_noise)

    # ---- acquisitions and their gradient with respect to the rows -----------------------------------------------------------------------
    def reference_acq_grad(self, x16, wm, kappa, var_add=0.0, mode=0, best=0.0, row_scale=None, dtype=torch.float64, round_fn=None,
                           f32_operands=True):
        """(mean [n, P], var [n], acq [n], g [n, width of x16]) of coati_head_gp_grad (include/coati_acq.h) on prepared bf16 rows, computed in
        `dtype` with the kernel's rounding points: reference()'s forward with qs = (q + q^T) / 2 in place of q; the acquisition of mode 0
        (wm . mean + kappa sqrt(var + var_add)) or 1 (expected improvement over `best`) with its derivatives A and B (B = 0 where var was
        clamped or var + var_add <= 1e-6 s2); t = rs (A wm . alpha - 2 B w) k, tb = rb(t), S = sum tb, dphi = 2 inv2l2 (tb . z - phi S); the
        rounding h -> phi passed straight through; then PropertyHead.reference_grad's backward from d = dphi.  round_fn (tensor -> tensor
        of `dtype`) replaces rb, the rounding to bf16, everywhere: with a plain cast this is the exact gradient of the unrounded model.
        f32_operands as in reference(), for wm and the four scalars too."""
        ex = self.extractor
        if x16.dtype != torch.bfloat16 or x16.dim() != 2 or x16.shape[1] not in (ex.input_dim, ex.input_dim_padded):
            raise ValueError(f"GPHead.reference_acq_grad: rows must be bf16 [n, {ex.input_dim} or {ex.input_dim_padded}], "
                             f"got {x16.dtype} {tuple(x16.shape)}")
        if int(mode) not in (0, 1) or (int(mode) == 1 and not float(kappa) > 0):
            raise ValueError(f"GPHead.reference_acq_grad: mode={mode} must be 0 or 1, and kappa={kappa} positive with mode 1")

        def rb(t):
            return t.detach().to(torch.float32).to(torch.bfloat16).to(dtype)

        rb = round_fn if round_fn is not None else rb
        n = x16.shape[0]
        with torch.no_grad():
            w0 = rb(ex.first.weight)
            wr = [rb(res.weight) for res in ex.residuals]
            h = x16[:, :ex.input_dim].to(dtype) @ w0.T + ex.first.bias.to(dtype)
            masks = []
            for res, w in zip(ex.residuals, wr):
                pre = rb(h) @ w.T + res.bias.to(dtype)
                masks.append(pre > 0)
                h = h + torch.relu(pre)
            phi = rb(h)
            # the operands padded to Mp = 32 or 64 inducing points as the kernel reads them: every sum over the points then has the kernel's
            # terms, and a head that carries its padding explicitly (zero alpha, zero rows and columns of q, any z) gives the same bits
            M = self.z.shape[0]
            pad = (32 if M <= 32 else 64) - M
            z = torch.nn.functional.pad(self.z.to(dtype), (0, 0, 0, pad))
            alpha, c = self._folded()
            alpha = torch.nn.functional.pad(alpha, (0, pad))
            qs = torch.nn.functional.pad(0.5 * (self.q.double() + self.q.double().T), (0, pad, 0, pad))
            zn = torch.nn.functional.pad((self.z.double() ** 2).sum(dim=1), (0, pad))
            wm = torch.as_tensor(wm, dtype=torch.float64, device=alpha.device).reshape(-1)
            if wm.shape[0] != self.num_outputs:
                raise ValueError(f"GPHead.reference_acq_grad: wm must be [{self.num_outputs}], got {tuple(wm.shape)}")
            inv2l2, s2 = 1.0 / (2.0 * self.lengthscale ** 2), self.signal_var
            kappa, var_add, best = float(kappa), float(var_add), float(best)
            if f32_operands:
                alpha, c, qs, zn, wm = alpha.float(), c.float(), qs.float(), zn.float(), wm.float()
                inv2l2, s2, kappa, var_add, best = (float(np.float32(v)) for v in (inv2l2, s2, kappa, var_add, best))
            alpha, c, qs, zn, wm = alpha.to(dtype), c.to(dtype), qs.to(dtype), zn.to(dtype), wm.to(dtype)
            d2 = ((phi * phi).sum(dim=1)[:, None] + zn[None, :] - 2.0 * (phi @ z.T)).clamp_min(0.0)
            k = s2 * torch.exp(-d2 * inv2l2)
            mean = c[None, :] + k @ alpha.T
            w = k @ qs.T
            var = (s2 - (w * k).sum(dim=1)).clamp_min(0.0)
            m = mean @ wm
            va = var + var_add
            sd = va.sqrt()
            dead = (var <= 0) | (va <= 1e-6 * s2)
            hb = torch.where(dead, torch.zeros_like(sd), kappa / (2.0 * torch.where(dead, torch.ones_like(sd), sd)))
            if int(mode) == 0:
                acq, A, B = m + kappa * sd, torch.ones_like(m), hb
            else:
                mu, s = m - best, kappa * sd
                pos = s > 0
                u = mu / torch.where(pos, s, torch.ones_like(s))
                Phi = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))
                ph = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
                acq = torch.where(pos, mu * Phi + s * ph, mu.clamp_min(0.0))
                A = torch.where(pos, Phi, (mu > 0).to(dtype))
                B = torch.where(pos, ph * hb, torch.zeros_like(hb))
            rs = torch.ones(n, dtype=dtype, device=k.device) if row_scale is None else torch.as_tensor(row_scale).detach().to(k).reshape(n)
            ca = wm @ alpha
            tb = rb(rs[:, None] * (A[:, None] * ca[None, :] - 2.0 * B[:, None] * w) * k)
            S = tb.sum(dim=1)
            d = 2.0 * inv2l2 * (tb @ z - phi * S[:, None])
            for msk, wl in zip(reversed(masks), reversed(wr)):
                d = d + rb(torch.where(msk, d, torch.zeros_like(d))) @ wl
            g = rb(d) @ w0
            return mean, var, acq, torch.nn.functional.pad(g, (0, x16.shape[1] - ex.input_dim))

    def acq_rows(self, x16, wm, kappa, var_add=0.0, mode=0, best=0.0, row_scale=None):
        """(mean [n, P], var [n], acq [n], g [n, input_dim_padded]) f32 of prepared rows, one launch of coati_head_gp_grad: mean as gp_rows
        gives it, bit for bit, acq the acquisition (reference_acq_grad names the two modes) and g the gradient of row_scale * acq with respect
        to the rows as the kernel reads them.  x16 under PropertyHead.predict_rows' stride rules; wm [P] weights on the means; row_scale
        [n] or None.  There is no CPU fallback."""
        ex = self.extractor
        x16, ldx = ex._kernel_rows(x16, "acq_rows")
        n, E, P = x16.shape[0], ex.input_dim_padded, self.num_outputs
        wm = torch.as_tensor(wm).detach().to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        if wm.shape[0] != P:
            raise ValueError(f"GPHead.acq_rows: wm must be [{P}], got {tuple(wm.shape)}")
        if int(mode) not in (0, 1) or (int(mode) == 1 and not float(kappa) > 0):
            raise ValueError(f"GPHead.acq_rows: mode={mode} must be 0 or 1, and kappa={kappa} positive with mode 1")
        if row_scale is not None:
            if not isinstance(row_scale, torch.Tensor) or row_scale.numel() != n:
                raise ValueError(f"GPHead.acq_rows: row_scale must be a tensor of {n} elements")
            if row_scale.device != self.device:
                raise ValueError(f"GPHead.acq_rows: row_scale on {row_scale.device}, the head on {self.device}")
            row_scale = row_scale.detach().to(torch.float32).reshape(n).contiguous()
        mean = torch.empty(n, P, dtype=torch.float32, device=self.device)
        var = torch.empty(n, dtype=torch.float32, device=self.device)
        acq = torch.empty(n, dtype=torch.float32, device=self.device)
        g = torch.empty(n, E, dtype=torch.float32, device=self.device)
        if n == 0:
            return mean, var, acq, g
        if self.device.type != "cuda":
            raise RuntimeError("GPHead.acq_rows: the head is not on a GPU; there is no CPU fallback (reference_acq_grad() is plain torch)")
        w0, b0, wr, br, _, _ = ex._operands()
        w0t, wrt = ex._grad_operands()
        z, zn, alpha, _, c, Mp = self._gp_operands()
        zt, qs = self._gp_grad_operands()
        with torch.cuda.device(self.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.call("coati_head_gp_grad", _ptr(x16), ldx, n, E, _ptr(w0), _ptr(b0), _ptr(wr), _ptr(br), ex.depth, ex.features, _ptr(w0t),
                      _ptr(wrt), _ptr(z), _ptr(zt), _ptr(zn), _ptr(alpha), _ptr(qs), _ptr(c), 1.0 / (2.0 * self.lengthscale ** 2),
                      self.signal_var, P, Mp, _ptr(wm), float(kappa), float(var_add), int(mode), float(best), _ptr(row_scale), _ptr(mean), P,
                      _ptr(var), _ptr(acq), _ptr(g), E, stream)
        return mean, var, acq, g

    def acquisition(self, kind="ucb", beta=1.0, best=None, output=0, include_noise=False):
        """An AcquisitionObjective (acquisition.py) on this head: the scalar that guided_ascent, guided_generation and torch autograd climb.
        guided_ascent(start, gp.acquisition("lcb", beta=2.0), steps=..., anchor=...)"""
        from .acquisition import AcquisitionObjective
        return AcquisitionObjective(self, kind=kind, beta=beta, best=best, output=output, include_noise=include_noise)

    def value_and_grad(self, vectors, cotangent=None):
        raise NotImplementedError("GPHead.value_and_grad: the gradient of the GP's mean or std with respect to the embedding is not "
                                  "implemented; gradients are those of the extractor (GPHead.extractor.value_and_grad)")

    def fused(self, x):
        raise NotImplementedError("GPHead.fused: the gradient of the GP's mean or std with respect to the embedding is not implemented; "
                                  "gradients are those of the extractor (GPHead.extractor.fused)")

    # ---- construction and files -------------------------------------------------------------------------------------------------------
    @classmethod
    def from_variational(cls, extractor, z, m, S, const=None, lengthscale=1.0, signal_var=1.0, noise_var=0.0, y_mean=None, y_scale=None,
                         jitter=0.0):
        """A GPHead from any unwhitened inducing distribution u ~ N(m [P, M], S [M, M]) at z: alpha = Kzz^-1 m, q = Kzz^-1 - Kzz^-1 S
        Kzz^-1, in float64, Kzz on the bf16-rounded z with jitter * signal_var on its diagonal."""
        z16 = torch.as_tensor(z).detach().to(torch.float32).to(torch.bfloat16)
        zd = z16.double().cpu()
        m, S = torch.as_tensor(m).detach().double().cpu(), torch.as_tensor(S).detach().double().cpu()
        if m.dim() == 1:
            m = m[None]
        M = zd.shape[0]
        Kzz = rbf_kernel(zd, zd, float(lengthscale), float(signal_var)) + float(jitter) * float(signal_var) * torch.eye(M, dtype=torch.float64)
        Kinv = torch.linalg.inv(Kzz)
        Kinv = 0.5 * (Kinv + Kinv.T)
        return cls(extractor, z16, (Kinv @ m.T).T, Kinv - Kinv @ S @ Kinv, const, lengthscale, signal_var, noise_var, y_mean, y_scale)

    def save(self, path):
        torch.save({"hyper": self.extractor.hyper(), "gp": self.gp_hyper(), "fit_info": dict(self.fit_info),
                    "state_dict": {k: v.detach().cpu() for k, v in self.state_dict().items()}}, path)

    @classmethod
    def load(cls, path, device="cpu"):
        d = torch.load(path, map_location="cpu")
        sd = d["state_dict"]
        ex = PropertyHead(**d["hyper"])
        ex.load_state_dict({k[len("extractor."):]: v for k, v in sd.items() if k.startswith("extractor.")})
        model = cls(ex, sd["z"], sd["alpha"], sd["q"], sd["const"], y_mean=sd["y_mean"], y_scale=sd["y_scale"], **d["gp"])
        model.fit_info = dict(d.get("fit_info", {}))
        return model.to(device).eval()


def _kmeans(x, k, iters, gen):
    """seeded Lloyd: the centres start at k distinct rows of x, `iters` rounds, an empty cluster keeps its centre"""
    centres = x[torch.randperm(x.shape[0], generator=gen)[:k]].clone()
    for _ in range(int(iters)):
        assign = torch.cdist(x, centres).argmin(dim=1)
        sums = torch.zeros_like(centres).index_add_(0, assign, x)
        counts = torch.zeros(centres.shape[0], dtype=x.dtype).index_add_(0, assign, torch.ones(x.shape[0], dtype=x.dtype))
        centres = torch.where(counts[:, None] > 0, sums / counts.clamp_min(1.0)[:, None], centres)
    return centres


def fit_gp_head(dataset, x_field="emb_smiles", y_field="pic50", n_inducing=60, head=None, gp_steps=200, jitter=1e-6, gp_lr=0.05,
                kmeans_iters=10, steps=1e5, depth=4, batch_size=512, test_frac=0.03, random_seed=510, lr=1e-3, features=256, unit_input=False,
                device=None):
    """Fits a GPHead to records; fit_property_head's arguments, split and seed.  head=None: the extractor is fitted first with
    fit_property_head (steps, depth, ... go there); a given PropertyHead is used frozen.  Then, in float64 on the training rows: phi from
    features_reference (fitting sees the kernel's features), targets standardised per output, inducing points from a seeded Lloyd k-means
    over at most 1000 sampled feature rows, rounded to bf16; log l (from the sample's mean pairwise distance), log s2 and log noise
    optimised with Adam on the negative collapsed bound for gp_steps steps, the best bound seen kept; the posterior in closed form
    (collapsed_posterior).  All outputs share Z, the kernel and the noise: one variance per row serves every output.

    Returns (gp_head, (Xs, Ys, dYs)): the test targets, the GP's mean and its latent standard deviation on the test set -- from the kernel
    when the head is on a GPU, from reference() on a CPU-only host.  gp_head.fit_info holds the bound, the initial bound and
    f32_var_error, the largest change of var (in units of s2) on the training rows from rounding the GP's operands to f32, as the kernel
    reads them; above 1e-2 a warning names it."""
    n_inducing = int(n_inducing)
    if not 1 <= n_inducing <= INDUCING_MAX:
        raise ValueError(f"fit_gp_head: n_inducing={n_inducing} outside 1 .. {INDUCING_MAX}")
    device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
    if head is None:
        head, _ = fit_property_head(dataset, x_field=x_field, y_field=y_field, steps=steps, depth=depth, batch_size=batch_size,
                                    test_frac=test_frac, random_seed=random_seed, lr=lr, features=features, unit_input=unit_input,
                                    device=device)
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
    X = torch.tensor(x, dtype=torch.float32).reshape(n, -1)
    Y = torch.tensor(y, dtype=torch.float64).reshape(n, -1)
    P = Y.shape[1]

    cpu_head = copy.deepcopy(head).cpu()
    phi = extractor_features(cpu_head, cpu_head.prepare(X[train_idx]), torch.float64)
    y_mean = Y[train_idx].mean(dim=0)
    y_scale = Y[train_idx].std(dim=0, unbiased=False).clamp_min(1e-12)
    ys = (Y[train_idx] - y_mean) / y_scale

    gen = torch.Generator().manual_seed(int(random_seed))
    sample = phi[torch.randperm(phi.shape[0], generator=gen)[:1000]]
    M = min(n_inducing, sample.shape[0])
    z = _kmeans(sample, M, kmeans_iters, gen).to(torch.float32).to(torch.bfloat16).double()
    m = sample.shape[0]
    l0 = max(float(torch.cdist(sample, sample).sum() / max(m * (m - 1), 1)), 1e-6)

    logs = torch.tensor([math.log(l0), 0.0, math.log(0.1)], dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([logs], lr=gp_lr)

    def bound_of(p):
        return collapsed_bound(phi, ys, z, torch.exp(p[0]), torch.exp(p[1]), torch.exp(p[2]), jitter)

    with torch.no_grad():
        initial = float(bound_of(logs))
    best, best_logs = initial, logs.detach().clone()
    for _ in range(int(gp_steps)):
        opt.zero_grad()
        try:
            loss = -bound_of(logs)
        except RuntimeError:            # (a Cholesky factor failed: stay with the best parameters seen)
            break
        if not bool(torch.isfinite(loss)):
            break
        loss.backward()
        opt.step()
        with torch.no_grad():
            try:
                b = float(bound_of(logs))
            except RuntimeError:
                break
        if math.isfinite(b) and b > best:
            best, best_logs = b, logs.detach().clone()
    l, s2, noise = (float(v) for v in torch.exp(best_logs))
    alpha, q, _, _ = collapsed_posterior(phi, ys, z, l, s2, noise, jitter)
    gp = GPHead(cpu_head, z, alpha, q, None, l, s2, noise, y_mean, y_scale).eval()
    # what handing q, alpha and zn to the kernel in f32 costs on (at most 1000 of) the training rows: the quadratic form cancels, and an
    # ill-conditioned Kzz (a tiny jitter under a long lengthscale) amplifies the rounding of q by its condition number
    rows = cpu_head.prepare(X[train_idx[:1000]])
    f32_var_error = float((gp.reference(rows)[1] - gp.reference(rows, f32_operands=False)[1]).abs().max()) / s2
    if f32_var_error > 1e-2:
        warnings.warn(f"fit_gp_head: rounding the GP's operands to f32 moves the variance by {f32_var_error:.2g} of s2 on the training rows "
                      f"(Kzz is ill-conditioned at lengthscale {l:.3g}); a larger jitter= conditions it")
    gp = gp.to(device)
    gp.fit_info = {"bound": best, "initial_bound": initial, "n_train": int(phi.shape[0]), "jitter": float(jitter),
                   "f32_var_error": f32_var_error}

    shape = y[test_idx].shape
    if n_test == 0:
        return gp, (y[test_idx], np.zeros(shape, dtype=np.float32), np.zeros(shape, dtype=np.float32))
    if device.type == "cuda":
        mean, std = gp.predict_with_std(X[test_idx])
    else:
        mean, var = gp.reference(gp.prepare(X[test_idx]))
        std = gp.std_from_var(var)
    return gp, (y[test_idx], mean.float().cpu().numpy().reshape(shape), std.float().cpu().numpy().reshape(shape))
