"""A mixture of K diagonal Gaussians over a library of embeddings held in device memory as bf16 rows (include/coati_gmm.h, csrc/gmm.hip).

    gmm = index.gmm(64)                                  # an EmbeddingIndex (coati_amd.search), "cosine" or "l2"
    index.log_density(gmm), index.outliers(gmm, 100)     # log p of every stored row; the 100 live rows of lowest density
    gmm.log_prob(vectors), gmm.predict(vectors)          # any vectors
    sampled_virtual_screen(index.gmm(64), head, model, tokenizer, hit_thresh)      # gmm.rsample is the call the screen makes

An EM iteration is two kernels and a float64 finish on [K, E] tensors: coati_gmm_estep streams the library once and writes every row's
log sum_k w_k N(x | mu_k, diag var_k) by an online log-sum-exp (no [N, K] matrix exists), coati_gmm_mstep recomputes the responsibilities
from it and adds the weighted moments in a fixed order (no atomics).  log N + log w is linear in [x | x^2]: prepare_params turns (weights,
means, variances) into the kernels' parameter rows.  The operands are f32 on the f32 matrix cores: the terms cancel by two orders of
magnitude, which bf16 parameter rows would not survive.  Both kernels are bitwise reproducible and do not depend on their launch geometry,
so neither does a fit.  reference_estep / reference_mstep / reference_fit are the same arithmetic in float64 torch on the CPU, what the
tests pin the kernels to.  The reference has no counterpart (its density is one full-covariance Gaussian fitted by SGD)."""
import math

import torch

from . import _lib
from .ops import ptr, stream

K_MAX = 256


def prepare_params(weights, means, variances, width, dtype=torch.float32):
    """(par f32 [K, 2 width], cst f32 [K]) of the kernels: par[k, :width] = mu / var, par[k, width:] = -0.5 / var and cst[k] = log w_k -
    0.5 sum_{d < dim} (mu^2 / var + log(2 pi var)), computed in float64 and rounded once to `dtype`.  Columns dim .. width - 1 (the zero padding of
    padded_dim) get par = 0 and take no part in cst."""
    w, mu, var = (torch.as_tensor(t).detach().double() for t in (weights, means, variances))
    if mu.dim() != 2 or var.shape != mu.shape or w.shape != mu.shape[:1] or not 1 <= mu.shape[0] <= K_MAX or mu.shape[1] > width:
        raise ValueError(f"gmm: weights [K], means and variances [K, dim <= {width}] with 1 <= K <= {K_MAX}, got {tuple(w.shape)}, "
                         f"{tuple(mu.shape)}, {tuple(var.shape)}")
    K, dim = mu.shape
    par = torch.zeros(K, 2 * width, dtype=torch.float64, device=mu.device)
    par[:, :dim] = mu / var
    par[:, width:width + dim] = -0.5 / var
    cst = w.log() - 0.5 * (mu * mu / var + (2.0 * math.pi * var).log()).sum(dim=1)
    return par.to(dtype).contiguous(), cst.to(dtype).contiguous()


def _check_operands(x16, row_bias, par, cst, what):
    from .cluster import _check_rows
    _check_rows(x16, row_bias, what)
    E = x16.shape[1]
    if par.dtype != torch.float32 or par.dim() != 2 or par.shape[1] != 2 * E or not 1 <= par.shape[0] <= K_MAX or not par.is_contiguous():
        raise ValueError(f"{what}: par must be contiguous f32 [1 .. {K_MAX}, {2 * E}]")
    if cst.dtype != torch.float32 or tuple(cst.shape) != (par.shape[0],) or par.device != x16.device or cst.device != x16.device:
        raise ValueError(f"{what}: cst must be f32 [{par.shape[0]}] on the rows' device, as par")


def estep_call(x16, row_bias, par, cst, want_assign=True, blocks=0):
    """coati_gmm_estep on prepared operands: (lse f32 [N], assign int32 [N] or None)"""
    _check_operands(x16, row_bias, par, cst, "estep_call")
    N, E = x16.shape
    lse = torch.empty(N, dtype=torch.float32, device=x16.device)
    assign = torch.empty(N, dtype=torch.int32, device=x16.device) if want_assign else None
    if N:
        with torch.cuda.device(x16.device):
            _lib.call("coati_gmm_estep", ptr(x16), N, E, ptr(row_bias), ptr(par), par.shape[0], ptr(cst), ptr(lse), ptr(assign), int(blocks),
                      stream())
    return lse, assign


def mstep_call(x16, row_bias, par, cst, lse, part=None, blocks=0):
    """coati_gmm_mstep: (w f32 [K], s1 f32 [K, E], s2 f32 [K, E]) from the E-step's lse; part: scratch kept by the caller between calls"""
    _check_operands(x16, row_bias, par, cst, "mstep_call")
    N, E = x16.shape
    K = par.shape[0]
    if lse.dtype != torch.float32 or tuple(lse.shape) != (N,) or lse.device != x16.device:
        raise ValueError(f"mstep_call: lse must be f32 [{N}] on the rows' device")
    w = torch.zeros(K, dtype=torch.float32, device=x16.device)
    s1 = torch.zeros(K, E, dtype=torch.float32, device=x16.device)
    s2 = torch.zeros(K, E, dtype=torch.float32, device=x16.device)
    if N:
        lib = _lib.lib()
        need = int(lib.coati_gmm_part_floats(N, E, K))
        if need < 0:
            raise RuntimeError(f"coati_gmm_part_floats({N}, {E}, {K}): {lib.coati_last_error().decode('utf-8', 'replace')}")
        if part is None or part.numel() < need:
            part = torch.empty(need, dtype=torch.float32, device=x16.device)
        with torch.cuda.device(x16.device):
            _lib.call("coati_gmm_mstep", ptr(x16), N, E, ptr(row_bias), ptr(par), K, ptr(cst), ptr(lse), ptr(part), part.numel(), ptr(w),
                      ptr(s1), ptr(s2), int(blocks), stream())
    return w, s1, s2


def _live(x, row_bias):
    return torch.ones(x.shape[0], dtype=torch.bool, device=x.device) if row_bias is None else row_bias > float("-inf")


def reference_logits(x16, par, cst):
    """[N, K] float64: the kernels' logit, restated"""
    x = x16.double()
    return torch.cat([x, x * x], dim=1) @ par.double().T + cst.double()


def reference_estep(x16, row_bias, par, cst):
    """(lse float64 [N], assign int64 [N]) as coati_gmm_estep defines them, in float64 torch"""
    logit = reference_logits(x16, par, cst)
    live = _live(x16, row_bias)
    lse = torch.where(live, torch.logsumexp(logit, dim=1), torch.full_like(logit[:, 0], float("-inf")))
    return lse, torch.where(live, logit.argmax(dim=1), torch.full_like(live, -1, dtype=torch.int64))


def reference_mstep(x16, row_bias, par, cst, lse):
    """(w [K], s1 [K, E], s2 [K, E]) float64 as coati_gmm_mstep defines them, from the given lse"""
    live = _live(x16, row_bias)
    x = x16.double()
    r = (reference_logits(x16, par, cst) - torch.where(live, lse.double(), torch.zeros_like(lse, dtype=torch.float64))[:, None]).exp()
    r = torch.where(live[:, None], r, torch.zeros_like(r))                     # (not `* live`: an excluded row's exp(logit) may be inf)
    return r.sum(dim=0), r.T @ x, r.T @ (x * x)


def _finish(w, s1, s2, weights, means, variances, n_live, reg_covar):
    """the float64 finish of an iteration on [K, E] tensors; a component with w < 10 eps N keeps its parameters"""
    w, s1, s2 = w.double(), s1.double(), s2.double()
    keep = w < 10.0 * torch.finfo(torch.float64).eps * n_live
    ws = torch.where(keep, torch.ones_like(w), w)[:, None]
    mu = s1 / ws
    var = s2 / ws - mu * mu + reg_covar
    means = torch.where(keep[:, None], means, mu)
    variances = torch.where(keep[:, None], variances, var)
    return w / w.sum(), means, variances


def reference_fit(x16, row_bias, weights, means, variances, iters, reg_covar=1e-6, dtype=torch.float64):
    """`iters` EM iterations in `dtype` torch on the CPU from the given parameters: (weights, means, variances, trace), trace[i] = the mean
    log-likelihood of the live rows under the parameters BEFORE update i.  dtype=float32 rounds the operands and sums as the kernels do
    (par, cst, logits, lse, moments in f32; the finish in float64): the f32 restatement the GPU fit is measured against."""
    x16 = x16.cpu()
    row_bias = None if row_bias is None else row_bias.cpu()
    live = _live(x16, row_bias)
    xl = x16[live]
    E, n = x16.shape[1], int(live.sum())
    weights, means, variances = (torch.as_tensor(t).double().cpu() for t in (weights, means, variances))
    dim = means.shape[1]
    x = xl.to(dtype)
    xx = torch.cat([x, x * x], dim=1)
    trace = []
    for _ in range(int(iters)):
        par, cst = (prepare_params_f64 if dtype == torch.float64 else prepare_params)(weights, means, variances, E)
        logit = xx @ par.to(dtype).T + cst.to(dtype)
        lse = torch.logsumexp(logit, dim=1)
        trace.append(float(lse.double().mean()))
        r = (logit - lse[:, None]).exp()
        w, s1, s2 = r.sum(dim=0), r.T @ x, r.T @ (x * x)
        weights, means, variances = _finish(w, s1[:, :dim], s2[:, :dim], weights, means, variances, n, reg_covar)
    return weights, means, variances, trace


def prepare_params_f64(weights, means, variances, width):
    """prepare_params without the rounding to f32 (reference_fit in float64)"""
    return prepare_params(weights, means, variances, width, dtype=torch.float64)


def _column_variance(x16, live, block=1 << 18):
    """[E] float64: the per-column variance of the live rows, from float64 sums taken in row blocks (no [N, E] temporary)"""
    E = x16.shape[1]
    s1, s2 = (torch.zeros(E, dtype=torch.float64, device=x16.device) for _ in range(2))
    for lo in range(0, x16.shape[0], block):
        x = x16[lo:lo + block].double() * live[lo:lo + block, None]
        s1 += x.sum(dim=0)
        s2 += (x * x).sum(dim=0)
    n = live.sum().double()
    return (s2 / n - (s1 / n) ** 2).clamp_min(0.0)


def fit_rows(x16, row_bias, k, iters=50, seed=0, init="kmeans", reg_covar=1e-6, tol=1e-4, dim=None, metric="cosine", check_every=5):
    """EM on prepared rows x16 [N, E] bf16 (row_bias [N] f32 or None: -inf excludes a row) -> GaussianMixture over the first `dim` columns
    (default: all E).  One iteration: coati_gmm_estep, coati_gmm_mstep, then in float64 on the device mu = s1 / w, var = s2 / w - mu^2 +
    reg_covar, weights = w / sum w; a component with w < 10 eps N keeps its parameters.  The mean of lse over the live rows is the trace,
    summed in float64 on the device and read every check_every iterations; the loop ends when an iteration gained less than tol.
    init="kmeans": cluster.kmeans_rows(x16, row_bias, metric, k, seed=seed) gives the means and, by its cluster sizes, the weights, and
    every component starts from the global per-dimension variance.  init=(weights, means, variances): the given start.  The same inputs
    give the same bits."""
    from .cluster import _check_rows, kmeans_rows
    _check_rows(x16, row_bias, "fit_rows")
    k, iters = int(k), int(iters)
    if not 1 <= k <= K_MAX:
        raise ValueError(f"fit_rows: k={k} outside 1 .. {K_MAX}")
    if iters < 0:
        raise ValueError(f"fit_rows: iters={iters} < 0")
    N, E = x16.shape
    dim = E if dim is None else int(dim)
    live = _live(x16, row_bias)
    n_live = int(live.sum())
    if n_live < 1:
        raise ValueError("fit_rows: no live row")
    if isinstance(init, str):
        if init != "kmeans":
            raise ValueError(f"fit_rows: init={init!r} is neither 'kmeans' nor (weights, means, variances)")
        cl = kmeans_rows(x16, row_bias, metric, k, seed=seed)
        means = cl.centres.double()[:, :dim]
        variances = (_column_variance(x16, live)[:dim] + reg_covar).expand(k, dim).clone()
        weights = cl.sizes.double().clamp_min(1.0)
        weights = weights / weights.sum()
    else:
        weights, means, variances = (torch.as_tensor(t).detach().to(device=x16.device, dtype=torch.float64) for t in init)
        if means.shape != (k, dim) or variances.shape != (k, dim) or weights.shape != (k,):
            raise ValueError(f"fit_rows: init must be ([{k}], [{k}, {dim}], [{k}, {dim}])")
    sums, trace, converged, it = [], [], False, 0
    need = int(_lib.lib().coati_gmm_part_floats(N, E, k))
    part = torch.empty(max(need, 1), dtype=torch.float32, device=x16.device)

    def flush():
        if sums:
            trace.extend(float(v) / n_live for v in torch.stack(sums).cpu())
            sums.clear()

    def gained_little():
        return len(trace) >= 2 and any(b - a < tol for a, b in zip(trace[-check_every - 1:-1], trace[-check_every:]))

    while it < iters:
        par, cst = prepare_params(weights, means, variances, E)
        lse, _ = estep_call(x16, row_bias, par, cst, want_assign=False)
        sums.append(torch.where(live, lse, torch.zeros_like(lse)).sum(dtype=torch.float64))
        w, s1, s2 = mstep_call(x16, row_bias, par, cst, lse, part)
        weights, means, variances = _finish(w, s1[:, :dim], s2[:, :dim], weights, means, variances, n_live, reg_covar)
        it += 1
        if it % check_every == 0 or it == iters:
            flush()
            if tol is not None and tol > 0 and gained_little():
                converged = True
                break
    flush()
    out = GaussianMixture(weights.float(), means.float(), variances.float(), metric=metric)
    out.float64 = (weights, means, variances)
    out.trace, out.iterations, out.converged = trace, it, converged
    out.log_likelihood = trace[-1] if trace else None
    return out


class GaussianMixture:
    """weights [K], means [K, dim], variances [K, dim] f32.  log_likelihood: the mean log-density of the fitted rows at the last E-step;
    trace: one such value per iteration; iterations; converged; metric: how vectors are prepared ("cosine": normalised, as the index
    stores its rows); float64: the fit's (weights, means, variances) before their rounding to f32, None unless fitted here."""

    def __init__(self, weights, means, variances, metric="cosine"):
        self.weights, self.means, self.variances = (torch.as_tensor(t).detach().float() for t in (weights, means, variances))
        if self.means.dim() != 2 or self.variances.shape != self.means.shape or self.weights.shape != self.means.shape[:1]:
            raise ValueError("GaussianMixture: weights [K], means [K, dim], variances [K, dim]")
        self.metric, self.log_likelihood, self.trace, self.iterations, self.converged, self.float64 = metric, None, [], 0, False, None

    @property
    def k(self):
        return self.means.shape[0]

    @property
    def dim(self):
        return self.means.shape[1]

    def _rows(self, vectors):
        from .search import padded_dim, prepare_rows
        if isinstance(vectors, torch.Tensor) and vectors.dtype == torch.bfloat16 and vectors.dim() == 2 and vectors.shape[1] == padded_dim(self.dim):
            return vectors.contiguous(), vectors.shape[1]                      # rows as an index stores them: taken as they are
        _, x16, _ = prepare_rows(vectors, self.metric, self.dim, torch.as_tensor(vectors).device)
        return x16.contiguous(), padded_dim(self.dim)

    def _estep(self, vectors):
        x16, E = self._rows(vectors)
        par, cst = prepare_params(self.weights, self.means, self.variances, E)
        if x16.device.type == "cuda":
            return estep_call(x16, None, par.to(x16.device), cst.to(x16.device))
        lse, assign = reference_estep(x16, None, par.to(x16.device), cst.to(x16.device))
        return lse.float(), assign.to(torch.int32)

    def log_prob(self, vectors):
        """[n] f32: log p of vectors [n, dim], prepared as the index prepares its rows (bf16 [n, dim_padded] rows, an index's .vectors,
        are taken as they are) -- the E-step kernel on a GPU, its float64
        restatement on the CPU"""
        return self._estep(vectors)[0]

    def predict(self, vectors):
        """[n] int32: the most responsible component"""
        return self._estep(vectors)[1]

    def responsibilities(self, vectors):
        """[n, K] f32 in torch (the [n, K] matrix is the caller's choice)"""
        x16, E = self._rows(vectors)
        par, cst = prepare_params(self.weights, self.means, self.variances, E)
        return torch.softmax(reference_logits(x16, par.to(x16.device), cst.to(x16.device)), dim=1).float()

    def rsample(self, shape, generator=None):
        """[*shape, dim] f32 draws: the component by torch.multinomial, then mu + sqrt(var) randn (what sampled_virtual_screen calls).
        The draws live where the mixture was fitted: the index's PREPARED rows, so on a "cosine" index they are of about unit norm, not at
        the model's own embedding scale -- rescale them before decoding with a model that minds the norm."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        n = int(math.prod(shape))
        comp = torch.multinomial(self.weights.cpu().double(), n, replacement=True, generator=generator)
        noise = torch.randn(n, self.dim, generator=generator)
        comp, noise = comp.to(self.means.device), noise.to(self.means.device)
        return (self.means[comp] + self.variances[comp].sqrt() * noise).reshape(*shape, self.dim)

    sample = rsample

    def to_torch(self, dtype=torch.float64):
        """torch.distributions.MixtureSameFamily of Independent(Normal)"""
        D = torch.distributions
        return D.MixtureSameFamily(D.Categorical(probs=self.weights.to(dtype)),
                                   D.Independent(D.Normal(self.means.to(dtype), self.variances.to(dtype).sqrt()), 1))

    def bic(self, n):
        """the Bayesian information criterion at n rows of mean log-likelihood self.log_likelihood"""
        if self.log_likelihood is None:
            raise ValueError("GaussianMixture.bic: no log_likelihood (a fitted mixture carries it)")
        return -2.0 * self.log_likelihood * n + (self.k * (2 * self.dim + 1) - 1) * math.log(n)

    def to(self, device):
        self.weights, self.means, self.variances = (t.to(device) for t in (self.weights, self.means, self.variances))
        return self

    def save(self, path):
        torch.save({"weights": self.weights.cpu(), "means": self.means.cpu(), "variances": self.variances.cpu(), "metric": self.metric,
                    "log_likelihood": self.log_likelihood, "trace": list(self.trace), "iterations": self.iterations,
                    "converged": self.converged}, path)

    @classmethod
    def load(cls, path, device=None):
        d = torch.load(path, map_location="cpu")
        out = cls(d["weights"], d["means"], d["variances"], metric=d["metric"])
        out.log_likelihood, out.trace, out.iterations, out.converged = d["log_likelihood"], list(d["trace"]), d["iterations"], d["converged"]
        return out if device is None else out.to(device)
