"""Embedding maps restated in float64 torch (CPU): the bisection of coati_tsne_affinities, the all-pairs sums of coati_tsne_repulsion, the
attraction / gradient / update of coati_tsne_step, coati_amd.tsne.joint and the loop of coati_amd.tsne.layout.  Nothing here calls the
library: these are the definitions the kernels are tested against, and kl_and_grad is what ties them to sklearn's exact method."""
import math

import torch

F64 = torch.float64
FLT_MAX = 3.4028234663852886e38
U = 2.0 ** -24          # half an ulp of f32, relative: one rounding


def affinities(d2, nbr, perplexity, steps=100):
    """(p float64 [n, k], beta [n], H [n]) by the header's rule, all rows at once; H = the entropy reached (nats)"""
    d2, valid = d2.to(F64), nbr >= 0
    n, k = d2.shape
    some = valid.any(dim=1)
    dmin = torch.where(valid, d2, torch.full_like(d2, math.inf)).min(dim=1).values
    d = torch.where(valid, d2 - torch.where(some, dmin, torch.zeros_like(dmin))[:, None], torch.zeros_like(d2))
    target = math.log(perplexity)

    def evaluate(b):
        p = torch.where(valid, torch.exp(-b[:, None] * d), torch.zeros_like(d))
        S = p.sum(dim=1).clamp_min(1e-300)
        return p, S, torch.log(S) + b * (p * d).sum(dim=1) / S

    b, lo, hi = torch.ones(n, dtype=F64), torch.zeros(n, dtype=F64), torch.full((n,), math.inf, dtype=F64)
    for _ in range(steps):
        _, _, H = evaluate(b)
        up = H > target
        lo, hi = torch.where(up, b, lo), torch.where(up, hi, b)
        b = torch.where(up, torch.where(torch.isinf(hi), (2 * b).clamp_max(FLT_MAX), 0.5 * (b + hi)), 0.5 * (b + lo))
    p, S, H = evaluate(b)
    p = torch.where(some[:, None], p / S[:, None], torch.zeros_like(p))
    return p, torch.where(some, b, torch.zeros_like(b)), H


def repulsion(y):
    """(rep [n, 2], z [n], |rep| terms summed [n, 2], the pairs' q [n, n] with a zero diagonal) in float64 from y as given (f32 values)"""
    y = y.to(F64)
    diff = y[:, None, :] - y[None, :, :]
    q = 1.0 / (1.0 + (diff ** 2).sum(dim=2))
    q.fill_diagonal_(0.0)
    terms = (q ** 2)[:, :, None] * diff
    return terms.sum(dim=1), q.sum(dim=1), terms.abs().sum(dim=1), q


def joint_dense(nbr, p):
    """float64 [n, n]: (P + P^T) / (2 n) of the conditional p over the graph nbr"""
    n, k = nbr.shape
    P = torch.zeros(n, n, dtype=F64)
    there = nbr >= 0
    r = torch.arange(n)[:, None].expand(n, k)[there]
    P.index_put_((r, nbr[there].long()), p[there].to(F64), accumulate=True)
    return (P + P.T) / (2 * n)


def csr_rows(offsets):
    """the row of every CSR entry"""
    counts = offsets[1:] - offsets[:-1]
    return torch.repeat_interleave(torch.arange(counts.shape[0]), counts)


def step(y, rep, Z, offsets, cols, vals, update, gains, exaggeration, momentum, lr, min_gain):
    """float64 dict of coati_tsne_step on CPU operands (update / gains are not changed): att, att_abs (the sum of |terms|), g, gains,
    update, y_out, kl_rows, kl_abs (sum of v |log v| + v |log q|: two terms an entry)"""
    y, rep, vals, update, gains = (t.to(F64) for t in (y, rep, vals, update, gains))
    n = y.shape[0]
    r, c = csr_rows(offsets), cols.long()
    diff = y[r] - y[c]
    d = 1.0 + (diff ** 2).sum(dim=1)
    terms = (vals / d)[:, None] * diff
    att = torch.zeros(n, 2, dtype=F64).index_add_(0, r, terms)
    att_abs = torch.zeros(n, 2, dtype=F64).index_add_(0, r, terms.abs())
    pos = vals > 0
    lv = torch.where(pos, vals.clamp_min(1e-300).log(), torch.zeros_like(vals))
    kl = torch.zeros(n, dtype=F64).index_add_(0, r, torch.where(pos, vals * (lv + d.log()), torch.zeros_like(vals)))
    kl_abs = torch.zeros(n, dtype=F64).index_add_(0, r, torch.where(pos, vals * (lv.abs() + d.log()), torch.zeros_like(vals)))
    Z = float(Z)
    g = 4.0 * (exaggeration * att - (rep / Z if Z > 0 else torch.zeros_like(rep)))
    new_gains = torch.where(update * g < 0, gains + 0.2, gains * 0.8).clamp_min(min_gain)
    new_update = momentum * update - lr * new_gains * g
    return dict(att=att, att_abs=att_abs, g=g, gains=new_gains, update=new_update, y_out=y + new_update, kl_rows=kl, kl_abs=kl_abs)


def kl_and_grad(y, P):
    """(KL(P | Q), its gradient [n, 2]) of the exact method on a dense symmetric joint P [n, n] (zero diagonal, sums to 1), float64:
    KL = sum P (log P - log q) + log Z, grad_i = 4 (sum_j P_ij q_ij (y_i - y_j) - rep_i / Z) -- what the three kernels compute"""
    y, P = y.to(F64), P.to(F64)
    rep, z, _, q = repulsion(y)
    Z = z.sum()
    diff = y[:, None, :] - y[None, :, :]
    att = ((P * q)[:, :, None] * diff).sum(dim=1)
    off = P > 0
    kl = (P[off] * (P[off].log() - q[off].log())).sum() + Z.log()
    return kl, 4.0 * (att - rep / Z)


def kl_csr(y, offsets, cols, vals):
    """KL(P | Q) in float64 of the map y under the CSR joint P"""
    _, z, _, _ = repulsion(y)
    out = step(y, torch.zeros_like(y, dtype=F64), 1.0, offsets, cols, vals, torch.zeros_like(y, dtype=F64), torch.ones_like(y, dtype=F64), 1.0, 0.0, 0.0, 0.0)
    return float(out["kl_rows"].sum() + z.sum().log())


def layout(y0, offsets, cols, vals, iters, exaggeration=12.0, exaggeration_iters=250, lr=None, momentum=(0.5, 0.8), min_gain=0.01, keep=()):
    """(y float64 [n, 2], {iteration: y after it} for the iterations in `keep`): coati_amd.tsne.layout's loop from the start y0"""
    y = y0.to(F64).clone()
    n = y.shape[0]
    lr = max(n / exaggeration / 4.0, 50.0) if lr is None else lr
    update, gains, kept = torch.zeros_like(y), torch.ones_like(y), {}
    for it in range(1, iters + 1):
        early = it <= exaggeration_iters
        rep, z, _, _ = repulsion(y)
        out = step(y, rep, z.sum(), offsets, cols, vals, update, gains, exaggeration if early else 1.0, momentum[0] if early else momentum[1], lr, min_gain)
        y, update, gains = out["y_out"], out["update"], out["gains"]
        if it in keep:
            kept[it] = y.clone()
    return y, kept


def clustered_rows(n=512, E=64, clusters=8, noise=0.5, seed=0):
    """(unit rows f32 [n, E], labels [n]): lab = i % clusters, normal centres, noise, rows normalised"""
    g = torch.Generator().manual_seed(seed)
    lab = torch.arange(n) % clusters
    x = torch.randn(clusters, E, generator=g)[lab] + noise * torch.randn(n, E, generator=g)
    return x / x.norm(dim=1, keepdim=True), lab


def neighbour_purity(y, lab, k=10):
    """the share of (point, one of its k nearest map neighbours) pairs with one label"""
    d = torch.cdist(y.to(F64), y.to(F64))
    d.fill_diagonal_(math.inf)
    near = d.topk(k, largest=False).indices
    return float((lab[near] == lab[:, None]).double().mean())
