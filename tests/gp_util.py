"""Shared by the GP-head tests (test_gp_cpu.py, test_gpu_gp.py): random GP heads whose every inducing index carries distinct values, f32
restatements of the kernel's arithmetic in two summation orders, and the C entry called on raw tensors."""
import ctypes
import math

import torch

from coati_amd.models.regression import GPHead, PropertyHead
from coati_amd.models.regression.gp_head import extractor_features, rbf_kernel

LOG2E = 1.4426950408889634


def unit_rows(n, E, gen):
    x = torch.randn(n, E, generator=gen)
    return (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)


def random_gp(E, F, D, P, M, seed, n=2000, unit_input=False):
    """(gp, x16 [n, E]): a random extractor; z = the features of M other unit rows; l = half the median distance between the rows' features
    and z (feature distances are concentrated: a shorter l spreads k, and with it var, over the rows); random alpha; a random NON-symmetric positive q scaled so that k q k reaches 0.95 s2 on these rows, so var spans (0.05 s2, s2).
    alpha and q are f32-representable: the kernel reads exactly the model's numbers."""
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    ex = PropertyHead(E, features=F, depth=D, num_outputs=P, unit_input=unit_input)
    rows = unit_rows(n + M, E, gen)
    x16, other = rows[:n], rows[n:]
    z = extractor_features(ex, other).to(torch.bfloat16)
    phi = extractor_features(ex, x16)
    zd = z.double()
    dist = torch.cdist(phi, zd)
    l = 0.5 * float(dist.median())
    s2 = 1.7
    alpha = torch.randn(P, M, generator=gen).float().double()
    u = (0.2 + 0.8 * torch.rand(M, M, generator=gen)).double()
    k = rbf_kernel(phi, zd, l, s2)
    scale = 0.95 * s2 / float(((k @ u.T) * k).sum(dim=1).max())
    q = (u * scale).float().double()
    const = torch.randn(P, generator=gen).float().double()
    gp = GPHead(ex, z, alpha, q, const, l, s2, 0.01)
    return gp, x16


def restate_gp_f32(gp, x16, chunks=1):
    """(mean, var) of GPHead.reference in f32: every product's K sum taken in `chunks` pieces that are then added in f32, |phi|^2 summed
    in f32, the exponential as exp2(x * log2 e) in f32, the way the device's fast exponential is evaluated"""
    ex = gp.extractor

    def rb(t):
        return t.detach().to(torch.bfloat16).float()

    def mm(a, w):
        K = a.shape[1]
        step = max(1, K // chunks)
        acc = None
        for lo in range(0, K, step):
            part = a[:, lo:lo + step] @ w[:, lo:lo + step].T
            acc = part if acc is None else acc + part
        return acc

    with torch.no_grad():
        h = mm(x16[:, :ex.input_dim].float(), rb(ex.first.weight)) + ex.first.bias
        for res in ex.residuals:
            h = h + torch.relu(mm(rb(h), rb(res.weight)) + res.bias)
        phi = rb(h)
        z = gp.z.float()
        zn = (gp.z.double() ** 2).sum(dim=1).float()
        alpha, c = gp._folded()
        alpha, c, q = alpha.float(), c.float(), gp.q.float()
        inv2l2 = torch.tensor(1.0 / (2.0 * gp.lengthscale ** 2), dtype=torch.float32)
        s2 = torch.tensor(gp.signal_var, dtype=torch.float32)
        nl = -inv2l2 * torch.tensor(LOG2E, dtype=torch.float32)
        d2 = ((phi * phi).sum(dim=1)[:, None] + zn[None, :] - 2.0 * mm(phi, z)).clamp_min(0.0)
        k = s2 * torch.exp2(d2 * nl)
        mean = c[None, :] + mm(k, alpha)
        var = (s2 - (mm(k, q) * k).sum(dim=1)).clamp_min(0.0)
        return mean, var


def errors(gp, mean, var, ref_mean, ref_var):
    """(largest error of mean relative to max |ref mean|, largest error of var relative to s2)"""
    em = float((mean.double() - ref_mean).abs().max()) / float(ref_mean.abs().max())
    ev = float((var.double() - ref_var).abs().max()) / gp.signal_var
    return em, ev


def restatement_errors(gp, x16, ref_mean, ref_var):
    """the worst (mean, var) error of the one-piece and the 8-chunk f32 restatement"""
    pairs = [errors(gp, *restate_gp_f32(gp, x16, chunks), ref_mean, ref_var) for chunks in (1, 8)]
    return max(p[0] for p in pairs), max(p[1] for p in pairs), pairs


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def head_gp_raw(gp, x16, mean, var, n, ldx=None, ldm=None, out=None, ldo=None, z=None):
    """coati_head_gp on tensors as they lie: x16's first n rows at stride ldx, mean at row stride ldm; out given: the linear layer too;
    z given: these (padded) inducing points instead of the head's"""
    from coati_amd import _lib
    ex = gp.extractor
    w0, b0, wr, br, wl, bl = ex._operands()
    zz, zn, alpha, q, c, Mp = gp._gp_operands()
    if z is not None:
        zz = z
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lin = out is not None
    _lib.call("coati_head_gp", _ptr(x16), x16.stride(0) if ldx is None else ldx, n, ex.input_dim_padded, _ptr(w0), _ptr(b0), _ptr(wr),
              _ptr(br), ex.depth, ex.features, _ptr(wl if lin else None), _ptr(bl if lin else None), ex.num_outputs, _ptr(out),
              (out.stride(0) if ldo is None else ldo) if lin else 0, _ptr(zz), _ptr(zn), _ptr(alpha), _ptr(q), _ptr(c),
              1.0 / (2.0 * gp.lengthscale ** 2), gp.signal_var, gp.num_outputs, Mp, _ptr(mean), mean.stride(0) if ldm is None else ldm,
              _ptr(var), stream)


def synthetic_records(n, dim, seed, noise=0.1, w=3.0):
    """records with a smooth property of a unit-scale embedding plus noise: sin(w x.a) + cos(w x.b) / 2 along two unit directions"""
    import numpy as np
    rng = np.random.RandomState(seed)
    x = rng.randn(n, dim).astype(np.float32)
    a, b = rng.randn(dim), rng.randn(dim)
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    y = (np.sin(w * (x @ a)) + 0.5 * np.cos(w * (x @ b)) + noise * rng.randn(n)).astype(np.float32)
    return [{"emb": x[i], "prop": y[i]} for i in range(n)], x, y
