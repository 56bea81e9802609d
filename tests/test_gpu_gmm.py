"""Library density on the GPU (include/coati_gmm.h, coati_amd/gmm.py, EmbeddingIndex.gmm / log_density / outliers) against the float64
restatement of coati_amd.gmm (reference_estep, reference_mstep, reference_fit) on the libraries of tests/gmm_util.py.  The kernels are held
to the forward error bound of an f32 dot product of their length, valid in any summation order; nothing here is a measured tolerance
except the fit's, which is four times what the same arithmetic in f32 on the CPU loses on the day."""
import functools
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import gmm_util as U  # noqa: E402
from tests.gpu_util import log  # noqa: E402

DEV = "cuda:0"
NEG_INF = float("-inf")
ROW_TILE = 128            # the E-step's rows per workgroup pass


def _dev(t):
    return None if t is None else t.to(DEV)


LIB_ROWS = 8000


@functools.lru_cache(maxsize=None)
def _case(E, K, far=True):
    """(x16 [LIB_ROWS, E], par, cst) on the CPU: reference_fit's parameters after 5 iterations, the last component then moved 50 sigma
    away so that its exponentials underflow.  The library has max(K - 1, 3) clusters and the start is their means (by the generator's own
    labels), the global variance and equal weights; for K >= 4 the last component starts as cluster 0's second one (the mean of its odd
    rows against the even rows' for component 0) and shares that cluster, so that moving it away orphans no row: every row keeps a
    component of its own cluster, and the margins of the assign check are those between clusters."""
    from coati_amd import gmm
    C = max(3, K - 1)
    x16 = U.library(LIB_ROWS, E, C, 0.5)
    x, lab = x16.double(), U.labels(LIB_ROWS, E, C)
    means = torch.stack([x[lab == c].mean(dim=0) for c in range(min(K, C))])
    if K > C:
        own = torch.nonzero(lab == 0).reshape(-1)
        means = torch.cat([means, x[own[1::2]].mean(dim=0, keepdim=True)])
        means[0] = x[own[0::2]].mean(dim=0)
    start = (torch.full((K,), 1.0 / K, dtype=torch.float64), means, (x.var(dim=0, unbiased=False) + 1e-6).expand(K, E).clone())
    w, m, v, _ = gmm.reference_fit(x16, None, *start, 5)
    if far:
        m = m.clone()
        m[K - 1] += 50.0 * v[K - 1].sqrt()
    par, cst = gmm.prepare_params(w, m, v, E)
    return x16, par, cst


def _estep(x16, bias, par, cst, blocks=0):
    from coati_amd import gmm
    lse, assign = gmm.estep_call(_dev(x16.contiguous()), _dev(bias), _dev(par), _dev(cst), blocks=blocks)
    torch.cuda.synchronize()
    assert lse.dtype == torch.float32 and assign.dtype == torch.int32 and lse.shape == assign.shape == (x16.shape[0],)
    return lse.cpu(), assign.cpu()


def _mstep(x16, bias, par, cst, lse, blocks=0):
    from coati_amd import gmm
    out = gmm.mstep_call(_dev(x16.contiguous()), _dev(bias), _dev(par), _dev(cst), _dev(lse), blocks=blocks)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)


# the issue's grid, whole: E x K x N, N also at the E-step's row tile +- 1
ESTEP = [(E, K, N) for E in (32, 64, 256, 288, 512) for K in (1, 15, 16, 17, 33, 256) for N in (1, 63, 64, 65, 1000, ROW_TILE - 1, ROW_TILE, ROW_TILE + 1)]


@pytest.mark.parametrize("E,K,N", ESTEP)
def test_estep_is_the_restatement_within_the_f32_bound(E, K, N):
    from coati_amd import gmm
    x16, par, cst = _case(E, K)
    x16 = x16[:N]
    lse, assign = _estep(x16, None, par, cst)
    want, _ = gmm.reference_estep(x16, None, par, cst)
    bound = U.logit_bound(x16, par, cst)
    err = (lse.double() - want).abs()
    log(f"gmm estep E={E} K={K} N={N}: worst |lse - ref| / bound = {float((err / bound).max()):.3f}, bound <= {float(bound.max()):.2e}")
    assert torch.isfinite(lse).all() and (err <= bound).all()
    top = gmm.reference_logits(x16, par, cst).topk(min(2, K), dim=1)
    clear = torch.ones(N, dtype=torch.bool) if K == 1 else (top.values[:, 0] - top.values[:, 1]) > 2 * bound
    log(f"gmm estep E={E} K={K} N={N}: {int((~clear).sum())} of {N} rows left out of the assign check")
    assert int((~clear).sum()) <= 0.02 * N and torch.equal(assign[clear].long(), top.indices[clear, 0])
    for blocks in (1, 3):
        l2, a2 = _estep(x16, None, par, cst, blocks)
        assert torch.equal(l2, lse) and torch.equal(a2, assign), blocks


def test_estep_far_rows_duplicates_and_excluded_rows():
    from coati_amd import gmm
    x16, par, cst = _case(64, 17, far=False)
    x16 = x16[:1000]
    far = (x16[:200].float() * 1000.0).to(torch.bfloat16)                       # 1000 norms away: every logit is hugely negative
    lse, assign = _estep(far, None, par, cst)
    want, wa = gmm.reference_estep(far, None, par, cst)
    assert torch.isfinite(lse).all() and ((lse.double() - want).abs() <= U.logit_bound(far, par, cst)).all()
    p2, c2 = par.clone(), cst.clone()
    p2[9], c2[9], p2[16], c2[16] = par[3], cst[3], par[3], cst[3]              # components 3, 9 and 16 identical: the lowest wins
    lse, assign = _estep(x16, None, p2, c2)
    _, first = gmm.reference_estep(x16, None, par, cst)
    assert not ((assign == 9) | (assign == 16)).any() and int((assign == 3).sum()) >= int((first == 3).sum()) > 0
    bias = torch.zeros(1000)
    gone = torch.tensor([0, 1, 63, 64, 500, 998, 999])
    bias[gone] = NEG_INF
    bias[5] = 7.0                                                               # any other value is ignored
    l3, a3 = _estep(x16, bias, p2, c2)
    keep = torch.ones(1000, dtype=torch.bool)
    keep[gone] = False
    assert (l3[gone] == NEG_INF).all() and (a3[gone] == -1).all() and torch.equal(l3[keep], lse[keep]) and torch.equal(a3[keep], assign[keep])


def _chain(N):
    """L: the longest addition chain of the M-step's order -- a range's rows enter one accumulator four at a time, each MFMA adding its
    four products one after the other (CH ceil(chunks / R) additions), then the R ranges are added in turn"""
    from coati_amd import _lib
    ch, R = _lib.lib().coati_gmm_chunk(), _lib.lib().coati_gmm_ranges(N)
    return ch * math.ceil(math.ceil(N / ch) / R) + R


CH = 64
MSTEP = [(32, 1, 1), (64, 17, 63), (256, 33, 65), (288, 16, 129), (512, 256, 1000), (32, 15, CH - 1), (64, 16, CH), (32, 17, CH + 1),
         (32, 8, 512 * 2 * CH + 5)]


@pytest.mark.parametrize("E,K,N", MSTEP)
def test_mstep_is_the_restatement_fed_the_kernel_s_lse(E, K, N):
    """per entry |got - ref| <= (expm1(2 beta) + L 2^-24) sum_n r |x| (x^2 for s2, 1 for w): beta the largest E-step bound of the call (r
    = exp of a difference of two quantities each within beta), L = _chain(N) = 64 ceil(chunks / ranges) + ranges, the longest chain of
    f32 additions; the last case puts two chunks into every range"""
    from coati_amd import _lib, gmm
    assert _lib.lib().coati_gmm_chunk() == CH
    if N <= 1000:
        x16, par, cst = _case(E, K)
        x16 = x16[:N]
    else:
        _, par, cst = _case(E, K)
        x16 = U.library(N, E, max(3, K - 1), 0.5)
    bias = None
    if N >= 129:
        bias = torch.zeros(N)
        bias[torch.tensor([0, 70, N - 1])] = NEG_INF
    lse, _ = _estep(x16, bias, par, cst)
    w, s1, s2 = _mstep(x16, bias, par, cst, lse)
    assert w.shape == (K,) and s1.shape == s2.shape == (K, E) and w.dtype == s1.dtype == s2.dtype == torch.float32
    rw, r1, r2 = gmm.reference_mstep(x16, bias, par, cst, lse)
    x = x16.double()
    live = torch.ones(N, dtype=torch.bool) if bias is None else bias > NEG_INF
    r = (gmm.reference_logits(x16, par, cst) - torch.where(live, lse.double(), torch.zeros(N, dtype=torch.float64))[:, None]).exp()
    r = torch.where(live[:, None], r, torch.zeros_like(r))
    beta = float(U.logit_bound(x16, par, cst).max())
    L = _chain(N)
    rel = math.expm1(2 * beta) + L * 2.0 ** -24
    worst, ok = [], []
    for got, ref, mag in ((w, rw, r.sum(dim=0)), (s1, r1, r.T @ x.abs()), (s2, r2, r.T @ (x * x))):
        err, tol = (got.double() - ref).abs(), rel * mag + N * 2.0 ** -126   # (an r below the smallest normal f32 is flushed to zero; |x| <= 1)
        worst.append(float((err / tol.clamp_min(1e-300)).max()))
        ok.append(bool((err <= tol).all()) and bool(torch.isfinite(got).all()))
    log(f"gmm mstep E={E} K={K} N={N}: L={L}, beta={beta:.2e}, worst error / tolerance (w, s1, s2) = " + ", ".join(f"{v:.3g}" for v in worst))
    assert all(ok), worst
    assert abs(float(w.double().sum()) - int(live.sum())) <= N * 2.0 ** -20
    for blocks in (0, 1, 3):
        again = _mstep(x16, bias, par, cst, lse, blocks)
        assert all(torch.equal(a, b) for a, b in zip(again, (w, s1, s2))), blocks


def test_mstep_excluded_rows_contribute_nothing():
    """Excluded rows add exact zeros.  The summation order hangs on the chunk a row falls in, so the bit-equal comparison removes rows
    that leave every other row among the same chunk-mates -- the library's tail within its last chunk, and one whole chunk in the middle
    (one chunk per range here, so a range of exact zeros drops out); single rows excluded in the middle are compared with the rows zeroed
    out of the restatement, in test_mstep_is_the_restatement_fed_the_kernel_s_lse"""
    x16, par, cst = _case(64, 17)
    x16 = x16[:1000]
    bias = torch.zeros(1000)
    bias[990:] = NEG_INF                                                        # chunks of 64: 1000 and 990 rows both make 16
    lse, _ = _estep(x16, bias, par, cst)
    with_them = _mstep(x16, bias, par, cst, lse)
    without = _mstep(x16[:990], None, par, cst, lse[:990].contiguous())
    assert all(torch.equal(a, b) for a, b in zip(with_them, without))
    bias = torch.zeros(1000)
    bias[128:192] = NEG_INF                                                     # a whole chunk in the middle: its range adds exact zeros
    lse, _ = _estep(x16, bias, par, cst)
    keep = bias > NEG_INF
    with_them = _mstep(x16, bias, par, cst, lse)
    without = _mstep(x16[keep].contiguous(), None, par, cst, lse[keep].contiguous())
    assert all(torch.equal(a, b) for a, b in zip(with_them, without))


def _fit_diffs(got, ref):
    (w, m, v, t), (rw, rm, rv, rt) = got, ref
    return {"means (sigma)": float(((m.double() - rm) / rv.sqrt()).abs().max()), "variances (relative)": float(((v.double() - rv) / rv).abs().max()),
            "weights": float((w.double() - rw).abs().max()), "mean log-likelihood": abs(t[-1] - rt[-1])}


@pytest.mark.parametrize("name", ["a", "c"])
def test_fit_rows_follows_reference_fit(name):
    """20 iterations from the common start: fit_rows may differ from the float64 EM by four times what the same EM with f32 operands and
    sums on the CPU differs by (the factor covers the other accumulation order); both are logged"""
    from coati_amd import gmm
    N, dim, C, K, noise = U.LIBRARIES[name]
    x16 = U.library(N, dim, C, noise)
    start = U.common_start(N, dim, C, noise, K)
    ref = gmm.reference_fit(x16, None, *start, 20)
    cpu32 = _fit_diffs(gmm.reference_fit(x16, None, *start, 20, dtype=torch.float32), ref)
    fits = [gmm.fit_rows(_dev(x16), None, K, iters=20, init=start, tol=0) for _ in range(2)]
    g = fits[0]
    assert g.iterations == 20 and len(g.trace) == 20
    assert all(torch.equal(getattr(fits[0], n), getattr(fits[1], n)) for n in ("weights", "means", "variances")) and fits[0].trace == fits[1].trace
    gpu = _fit_diffs(tuple(t.cpu() for t in g.float64) + (g.trace,), ref)      # the parameters before their rounding to f32
    for what in gpu:
        log(f"gmm fit {name}, {what}: f32 on the CPU {cpu32[what]:.3e}, fit_rows {gpu[what]:.3e}")
    for what in gpu:
        assert gpu[what] <= 4 * cpu32[what], what
    lim = 4 * cpu32["mean log-likelihood"]
    assert all(b - a >= -lim for a, b in zip(g.trace, g.trace[1:]))


def _index(planted=0):
    from coati_amd.search import EmbeddingIndex
    N, dim, C, K, noise = U.LIBRARIES["a"]
    x = U.library(N, dim, C, noise).float()
    if planted:
        u = torch.randn(planted, dim, generator=torch.Generator().manual_seed(7))
        x = torch.cat([x, u / u.norm(dim=1, keepdim=True)])
    index = EmbeddingIndex(dim, "cosine", device=DEV)
    index.add(x)
    return index


def test_index_gmm_log_density_and_outliers():
    from coati_amd import gmm
    index = _index()
    index.remove([3, 77, 19999])
    live = (index.bias > NEG_INF).cpu()
    g = index.gmm(8)
    cl = index.kmeans(8, seed=0)
    x16 = index.vectors.cpu()
    xl = x16[live]
    w0 = cl.sizes.double().cpu().clamp_min(1)
    ref = gmm.reference_fit(xl, None, w0 / w0.sum(), cl.centres.double().cpu(),
                            (xl.double().var(dim=0, unbiased=False) + 1e-6).expand(8, 64).clone(), 50)
    log(f"gmm index.gmm(8): mean log-likelihood {g.log_likelihood:.4f} after {g.iterations} iterations, reference_fit {ref[3][-1]:.4f} after 50")
    assert abs(g.log_likelihood - ref[3][-1]) <= 0.01 * abs(ref[3][-1])
    dens = index.log_density(g)
    assert dens.dtype == torch.float32 and dens.shape == (20000,) and (dens.cpu()[~live] == NEG_INF).all()
    assert torch.equal(dens[live.to(DEV)], g.log_prob(index.vectors[live.to(DEV)]))
    vals, rows = index.outliers(g, 10)
    order = torch.where(live, dens.cpu(), torch.full((20000,), float("inf"))).sort(stable=True)
    assert torch.equal(vals.cpu(), order.values[:10]) and sorted(rows.cpu().tolist()) == sorted(order.indices[:10].tolist())


def test_planted_uniform_rows_are_the_outliers():
    """20 rows drawn uniformly on the sphere among 20000 clustered ones: at least 18 are among the 40 rows of lowest density (the float64
    reference_fit from the same k-means start finds all 20 there)"""
    index = _index(planted=20)
    g = index.gmm(8)
    _, rows = index.outliers(g, 40)
    found = int((rows >= 20000).sum())
    log(f"gmm outliers: {found} of 20 planted rows among the 40 of lowest density")
    assert found >= 18


def test_fit_library_density_from_a_tensor():
    from coati_amd.generative import fit_library_density
    N, dim, C, K, noise = U.LIBRARIES["c"]
    x = U.library(N, dim, C, noise).float()
    g = fit_library_density(x, 3, iters=10)
    index = _index_of(x)
    h = fit_library_density(index, 3, iters=10)
    assert g.metric == "cosine" and g.k == 3 and g.dim == dim and all(torch.equal(getattr(g, n), getattr(h, n)) for n in ("weights", "means", "variances"))
    assert g.means.device.type == "cuda" and torch.isfinite(g.log_prob(x.to(DEV))).all()


def _index_of(x):
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(x.shape[1], "cosine", device=DEV)
    index.add(x)
    return index
