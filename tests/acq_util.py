"""Shared by the acquisition-gradient tests (test_acq_cpu.py, test_gpu_acq.py): GP heads over a given extractor, f32 restatements of
coati_head_gp_grad's arithmetic (include/coati_acq.h) in two summation orders, an autograd model of the same function whose roundings are
straight-through (or absent), reference-backed value_and_grad callables, and the C entry called on raw tensors.  Builds on gp_util and
guide_util, which stay as they are."""
import ctypes
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import gp_util as GP  # noqa: E402

from coati_amd.models.regression import GPHead  # noqa: E402
from coati_amd.models.regression.gp_head import extractor_features, rbf_kernel  # noqa: E402
from coati_amd.models.regression.property_head import unit_input_chain  # noqa: E402

# (E, F, D, P, M): E % 64 == 32 with Mp = 32 exactly; the first M with Mp = 64; the bench shape; the largest LDS footprint
SHAPES = [(32, 64, 1, 1, 8), (96, 128, 2, 2, 32), (64, 128, 3, 8, 33), (256, 256, 4, 1, 60), (512, 256, 16, 3, 64)]
LOG2E = GP.LOG2E


def ids(s):
    return "x".join(map(str, s))


def gp_over(ex, x16, other, P, M, seed):
    """gp_util.random_gp's GP over a GIVEN extractor: z = the features of `other` [M, E], l = half the median feature distance, random
    alpha, a random non-symmetric positive q scaled so that k q k reaches 0.95 s2 on x16"""
    gen = torch.Generator().manual_seed(seed)
    z = extractor_features(ex, other).to(torch.bfloat16)
    phi = extractor_features(ex, x16)
    zd = z.double()
    l = 0.5 * float(torch.cdist(phi, zd).median())
    s2 = 1.7
    alpha = torch.randn(P, M, generator=gen).float().double()
    u = (0.2 + 0.8 * torch.rand(M, M, generator=gen)).double()
    k = rbf_kernel(phi, zd, l, s2)
    scale = 0.95 * s2 / float(((k @ u.T) * k).sum(dim=1).max())
    const = torch.randn(P, generator=gen).float().double()
    return GPHead(ex, z, alpha, (u * scale).float().double(), const, l, s2, 0.01)


def acq_cases(gp, x16, seed=0):
    """[(name, wm, kappa, var_add, mode, best, rs)]: both modes, var_add = 0 and noise_var, with and without rs; for ei `best` is the
    median of the reference's weighted mean, so that Phi(u) is not saturated"""
    gen = torch.Generator().manual_seed(1000 + seed)
    P, n = gp.num_outputs, x16.shape[0]
    wm = torch.zeros(P)
    wm[P - 1] = 1.0
    best = float((gp.reference(x16)[0] @ wm.double()).median())
    rs = (0.5 + torch.rand(n, generator=gen)).float()
    return [("ucb", wm, 1.5, 0.0, 0, 0.0, None), ("lcb+noise+rs", wm, -0.75, gp.noise_var, 0, 0.0, rs),
            ("ei", wm, 1.0, 0.0, 1, best, None), ("ei+noise+rs", wm, 2.0, gp.noise_var, 1, best, rs)]


def restate_acq_f32(gp, x16, wm, kappa, var_add, mode, best, rs=None, chunks=1):
    """(mean, var, acq, g, masks) of GPHead.reference_acq_grad in f32: every product's K sum taken in `chunks` pieces that are then added in
    f32, the exponential as exp2(x * log2 e) as in gp_util.restate_gp_f32; masks [D, n, F] are the ReLU decisions"""
    ex = gp.extractor
    f32 = torch.float32

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

    def t32(v):
        return torch.tensor(v, dtype=f32)

    with torch.no_grad():
        n = x16.shape[0]
        w0 = rb(ex.first.weight)
        wr = [rb(res.weight) for res in ex.residuals]
        h = mm(x16[:, :ex.input_dim].float(), w0) + ex.first.bias
        masks = []
        for res, w in zip(ex.residuals, wr):
            pre = mm(rb(h), w) + res.bias
            masks.append(pre > 0)
            h = h + torch.relu(pre)
        phi = rb(h)
        z = gp.z.float()
        zn = (gp.z.double() ** 2).sum(dim=1).float()
        alpha, c = gp._folded()
        alpha, c = alpha.float(), c.float()
        qs = (0.5 * (gp.q.double() + gp.q.double().T)).float()
        inv2l2, s2 = t32(1.0 / (2.0 * gp.lengthscale ** 2)), t32(gp.signal_var)
        kappa, var_add, best, wm = t32(kappa), t32(var_add), t32(best), torch.as_tensor(wm).float()
        d2 = ((phi * phi).sum(dim=1)[:, None] + zn[None, :] - 2.0 * mm(phi, z)).clamp_min(0.0)
        k = s2 * torch.exp2(d2 * (-inv2l2 * t32(LOG2E)))
        mean = c[None, :] + mm(k, alpha)
        w = mm(k, qs)
        var = (s2 - (w * k).sum(dim=1)).clamp_min(0.0)
        m = mm(mean, wm[None])[:, 0]
        va = var + var_add
        sd = va.sqrt()
        dead = (var <= 0) | (va <= t32(1e-6) * s2)
        hb = torch.where(dead, torch.zeros_like(sd), kappa / (2.0 * torch.where(dead, torch.ones_like(sd), sd)))
        if mode == 0:
            acq, A, B = m + kappa * sd, torch.ones_like(m), hb
        else:
            mu, s = m - best, kappa * sd
            pos = s > 0
            u = mu / torch.where(pos, s, torch.ones_like(s))
            Phi = 0.5 * (1.0 + torch.erf(u * t32(math.sqrt(0.5))))
            ph = torch.exp(-0.5 * u * u) * t32(1.0 / math.sqrt(2.0 * math.pi))
            acq = torch.where(pos, mu * Phi + s * ph, mu.clamp_min(0.0))
            A = torch.where(pos, Phi, (mu > 0).float())
            B = torch.where(pos, ph * hb, torch.zeros_like(hb))
        r = torch.ones(n) if rs is None else torch.as_tensor(rs).float()
        ca = mm(wm[None], alpha.T.contiguous())[0]
        tb = rb(r[:, None] * (A[:, None] * ca[None, :] - 2.0 * B[:, None] * w) * k)
        S = tb.sum(dim=1)
        d = 2.0 * inv2l2 * (mm(tb, z.T.contiguous()) - phi * S[:, None])
        for msk, wl in zip(reversed(masks), reversed(wr)):
            d = d + mm(rb(torch.where(msk, d, torch.zeros_like(d))), wl.T.contiguous())
        g = torch.nn.functional.pad(mm(rb(d), w0.T.contiguous()), (0, x16.shape[1] - ex.input_dim))
        assert all(t.dtype == f32 for t in (mean, var, acq, g))
        return mean, var, acq, g, (torch.stack(masks) if masks else torch.zeros(0, n, ex.features, dtype=torch.bool))


def row_error(g, ref):
    """per row: max |g - ref| / max |ref| over the whole of ref"""
    return (g.double() - ref).abs().max(dim=1).values / float(ref.abs().max())


def shares(gp, x16, case, ref_g, threshold):
    """[(share of rows within `threshold` of scale, largest row error)] of the one-piece and the 8-chunk f32 restatement"""
    _, wm, kappa, var_add, mode, best, rs = case
    out = []
    for chunks in (1, 8):
        err = row_error(restate_acq_f32(gp, x16, wm, kappa, var_add, mode, best, rs, chunks)[3], ref_g)
        out.append((float((err <= threshold).float().mean()), float(err.max())))
    return out


# ---- an autograd model of the same function ------------------------------------------------------------------------------------------
def _rb64(t):
    return t.detach().to(torch.float32).to(torch.bfloat16).to(torch.float64)


class _RoundForward(torch.autograd.Function):
    """rb(t) forward, the gradient passed straight through"""

    @staticmethod
    def forward(ctx, t):
        return _rb64(t)

    @staticmethod
    def backward(ctx, grad):
        return grad


class _RoundBackward(torch.autograd.Function):
    """t forward, rb(gradient) backward: where the kernel rounds a backward operand"""

    @staticmethod
    def forward(ctx, t):
        return t.clone()

    @staticmethod
    def backward(ctx, grad):
        return _rb64(grad)


def autograd_acq(gp, vectors, wm, kappa, var_add, mode, best, rs=None, rounded=False):
    """(acq [n], grad [n, dim]) in float64 from torch.autograd on the model written forward only, on the STORED float64 operands and the
    model's own (non-symmetric) q.  vectors [n, input_dim] float64; with unit_input they are normalised, and the prepared bf16 row stands in
    for them straight-through (the gradient does not see that rounding).  rounded=False: no rounding anywhere else (weights and streams as
    they are).  rounded=True: the kernel's roundings, forward ones straight-through, backward ones (the three operands rb(m (.) d), rb(d)
    and tb) applied to the gradient where it passes."""
    ex = gp.extractor
    f64 = torch.float64
    rf = _RoundForward.apply if rounded else (lambda t: t)
    rbk = _RoundBackward.apply if rounded else (lambda t: t)
    wt = _rb64 if rounded else (lambda t: t.detach().to(f64))
    with torch.enable_grad():
        x = vectors.detach().to(f64).clone().requires_grad_(True)
        u = x / x.norm(dim=1, keepdim=True).clamp_min(1e-30) if ex.unit_input else x
        x16 = gp.prepare(vectors)[:, :ex.input_dim].to(f64)
        u = u + (x16 - u).detach()                       # the prepared row forward, the identity backward
        h = rbk(u @ wt(ex.first.weight).T) + ex.first.bias.detach().to(f64)
        for res in ex.residuals:
            pre = rf(h) @ wt(res.weight).T + res.bias.detach().to(f64)
            h = h + rbk(torch.relu(pre))
        phi = rf(h)
        z = gp.z.to(f64)
        alpha, c = gp._folded()
        zn = (gp.z.double() ** 2).sum(dim=1)
        inv2l2, s2 = 1.0 / (2.0 * gp.lengthscale ** 2), gp.signal_var
        d2 = ((phi * phi).sum(dim=1)[:, None] + zn[None, :] - 2.0 * (phi @ z.T)).clamp_min(0.0)
        k = s2 * torch.exp(rbk(-d2 * inv2l2))
        mean = c[None, :] + k @ alpha.T
        var = (s2 - ((k @ gp.q.T) * k).sum(dim=1)).clamp_min(0.0)
        m = mean @ torch.as_tensor(wm).to(f64)
        sd = (var + var_add).sqrt()
        if mode == 0:
            acq = m + kappa * sd
        else:
            mu, s = m - best, kappa * sd
            uu = mu / s
            acq = mu * 0.5 * (1.0 + torch.erf(uu / math.sqrt(2.0))) + s * torch.exp(-0.5 * uu * uu) / math.sqrt(2.0 * math.pi)
        scale = torch.ones_like(acq) if rs is None else torch.as_tensor(rs).to(f64)
        (grad,) = torch.autograd.grad((acq * scale).sum(), x)
    return acq.detach(), grad


def reference_value_and_grad(objective, round_fn=None, f32_operands=True):
    """AcquisitionObjective.value_and_grad's contract from GPHead.reference_acq_grad in float64, on the CPU: what runs guided_ascent without
    a GPU.  round_fn as in reference_acq_grad."""
    gp = objective.gp

    def fn(v, cot=None):
        wm, kappa, var_add, mode, best = objective.operands()
        rs = None if cot is None else torch.as_tensor(cot).double().reshape(-1).expand(v.shape[0])
        _, _, acq, g = gp.reference_acq_grad(gp.prepare(v), wm, kappa, var_add, mode, best, rs, torch.float64, round_fn, f32_operands)
        g = g[:, :gp.input_dim]
        if gp.unit_input:
            g = unit_input_chain(g, v.detach().double())
        return acq[:, None], g
    return fn


def autograd_value_and_grad(objective):
    """the same contract from autograd_acq on the unrounded float64 model"""
    def fn(v, cot=None):
        wm, kappa, var_add, mode, best = objective.operands()
        rs = None if cot is None else torch.as_tensor(cot).double().reshape(-1).expand(v.shape[0])
        acq, grad = autograd_acq(objective.gp, v, wm, kappa, var_add, mode, best, rs, rounded=False)
        return acq[:, None], grad
    return fn


# ---- the C entry on raw tensors --------------------------------------------------------------------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def head_gp_grad_raw(gp, x16, case, mean, var, acq, g, n, ldx=None, ldm=None, ldg=None, rs=None, z=None):
    """coati_head_gp_grad on tensors as they lie: x16's first n rows at stride ldx, mean and g at their own row strides; rs given: this
    device tensor instead of the case's; z given: these padded inducing points [Mp, F] (and their transpose) instead of the head's"""
    from coati_amd import _lib
    _, wm, kappa, var_add, mode, best, case_rs = case
    ex = gp.extractor
    w0, b0, wr, br, _, _ = ex._operands()
    w0t, wrt = ex._grad_operands()
    zz, zn, alpha, _, c, Mp = gp._gp_operands()
    zt, qs = gp._gp_grad_operands()
    if z is not None:
        zz, zt = z, z.T.contiguous()
    if rs is None and case_rs is not None:
        rs = case_rs.to(x16.device).contiguous()
    keep = wm.to(device=x16.device, dtype=torch.float32).contiguous()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.call("coati_head_gp_grad", _ptr(x16), x16.stride(0) if ldx is None else ldx, n, ex.input_dim_padded, _ptr(w0), _ptr(b0), _ptr(wr),
              _ptr(br), ex.depth, ex.features, _ptr(w0t), _ptr(wrt), _ptr(zz), _ptr(zt), _ptr(zn), _ptr(alpha), _ptr(qs), _ptr(c),
              1.0 / (2.0 * gp.lengthscale ** 2), gp.signal_var, gp.num_outputs, Mp, _ptr(keep), float(kappa), float(var_add), int(mode),
              float(best), _ptr(rs), _ptr(mean), mean.stride(0) if ldm is None else ldm, _ptr(var), _ptr(acq), _ptr(g),
              g.stride(0) if ldg is None else ldg, stream)
    torch.cuda.synchronize()


def run_case(gp, x16_d, case):
    """GPHead.acq_rows with a case's operands on device rows"""
    _, wm, kappa, var_add, mode, best, rs = case
    return gp.acq_rows(x16_d, wm, kappa, var_add, mode, best, None if rs is None else rs[:x16_d.shape[0]].to(x16_d.device))


def f32_scalar(v):
    return float(np.float32(v))


# ---- the cases of test_gpu_acq.py, built once on the CPU -------------------------------------------------------------------------------
THRESHOLD = 1e-5    # a row is "close" when max |g - ref64| <= THRESHOLD * max |ref64| (test_gpu_guide.py's threshold)
# ... except where the two CPU f32 restatements themselves keep fewer than 0.9 of the rows within it: 17 masked bf16 operands of 256 values per
# row (D = 16) leave only 0.22 .. 0.60 of their rows within 1e-5 and 0.78 .. 0.86 within 1e-3; the first decade at which both reach 0.9 is 1e-2
THRESHOLDS = {(512, 256, 16, 3, 64): 1e-2}


def threshold(shape):
    return THRESHOLDS.get(tuple(shape), THRESHOLD)


def random_case(shape, i, n=2000):
    """a gp_util.random_gp head with its n unit rows, and per acquisition case the float64 reference and the two f32 restatements' (share of
    close rows, largest error)"""
    E, F, D, P, M = shape
    gp, x16 = GP.random_gp(E, F, D, P, M, seed=500 + i, n=n)
    per = []
    for case in acq_cases(gp, x16, seed=i):
        _, wm, kappa, var_add, mode, best, rs = case
        ref = gp.reference_acq_grad(x16, wm, kappa, var_add, mode, best, rs)
        per.append((case, ref, shares(gp, x16, case, ref[3], threshold(shape))))
    return gp, x16, per


def ternary_case(shape, i, n=2000):
    """a GP over a guide_util.ternary_head extractor on screen_util.exact_rows: the ReLU decisions and phi are the same in any arithmetic
    (asserted), so every difference of g is rounding behind phi"""
    from tests import guide_util, screen_util
    E, F, D, P, M = shape
    ex = guide_util.ternary_head(E, F, D, P, seed=640 + i)
    rows = screen_util.exact_rows(n + M, E, seed=650 + i)
    gp = gp_over(ex, rows[:n], rows[n:], P, M, seed=660 + i)
    x16 = rows[:n].contiguous()
    per = []
    m64 = None
    for case in acq_cases(gp, x16, seed=i):
        _, wm, kappa, var_add, mode, best, rs = case
        ref = gp.reference_acq_grad(x16, wm, kappa, var_add, mode, best, rs)
        cpu = []
        for chunks in (1, 8):
            r = restate_acq_f32(gp, x16, wm, kappa, var_add, mode, best, rs, chunks)
            if m64 is None:
                m64 = restate_masks64(gp, x16)
            assert torch.equal(r[4], m64), (shape, "masks differ between arithmetics")
            err = row_error(r[3], ref[3])
            cpu.append((float((err <= threshold(shape)).float().mean()), float(err.max())))
        per.append((case, ref, cpu))
    return gp, x16, per


def restate_masks64(gp, x16):
    """the ReLU decisions [D, n, F] of the float64 reference forward"""
    ex = gp.extractor

    def rb(t):
        return t.detach().to(torch.float32).to(torch.bfloat16).double()

    with torch.no_grad():
        h = x16[:, :ex.input_dim].double() @ rb(ex.first.weight).T + ex.first.bias.double()
        masks = []
        for res in ex.residuals:
            pre = rb(h) @ rb(res.weight).T + res.bias.double()
            masks.append(pre > 0)
            h = h + torch.relu(pre)
    return torch.stack(masks) if masks else torch.zeros(0, x16.shape[0], ex.features, dtype=torch.bool)
