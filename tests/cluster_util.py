"""Library clustering restated in float64 torch (CPU): the scores of stored bf16 rows against bf16 centres, the argmax with the lowest
index among equal scores, excluded rows, per-cluster sums, one Lloyd round and the loop of coati_amd.cluster.kmeans_rows.  Nothing here
calls the library."""
import torch

NEG_INF = float("-inf")


def ints(shape, seed, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).to(torch.float32)


def scores(x16, c16, cbias=None):
    """float64 [N, K]: dot(x_n, c_k) + cbias[k] of the stored values"""
    s = x16.double().cpu() @ c16.double().cpu().T
    return s if cbias is None else s + cbias.double().cpu()[None]


def argmax_low(s):
    """(index, value) of every row's maximum, the LOWEST index among equal values"""
    top = s.max(dim=1, keepdim=True).values
    K = s.shape[1]
    idx = torch.where(s == top, torch.arange(K)[None].expand_as(s), torch.full_like(s, K, dtype=torch.int64)).min(dim=1).values
    return idx, top[:, 0]


def assign(x16, row_bias, c16, cbias=None):
    """(assign int32 [N], best float64 [N]) as coati_cluster_assign defines them; (-1, -inf) where row_bias is -inf"""
    idx, top = argmax_low(scores(x16, c16, cbias))
    if row_bias is not None:
        out = row_bias.cpu() == NEG_INF
        idx, top = torch.where(out, torch.full_like(idx, -1), idx), torch.where(out, torch.full_like(top, NEG_INF), top)
    return idx.to(torch.int32), top


def sums(x16, assign_, k):
    """float64 [k, E]: the sum of the stored rows of every cluster; rows with assign < 0 nowhere"""
    keep = assign_ >= 0
    return torch.zeros(k, x16.shape[1], dtype=torch.float64).index_add_(0, assign_[keep].long().cpu(), x16.double().cpu()[keep.cpu()])


def prepare_centres(c, metric):
    """(float64 centres after the metric's preparation as float32 does it, their bf16 rounding, cbias f32 or None)"""
    c = c.float().cpu()
    if metric == "cosine":
        c = c / c.norm(dim=1, keepdim=True).clamp_min(1e-30)
    c16 = c.to(torch.bfloat16)
    cbias = (-0.5 * (c16.double() ** 2).sum(dim=1)).float() if metric == "l2" else None
    return c, c16, cbias


def lloyd_round(x16, row_bias, centres, metric):
    """one round from f32 centres [k, E]: (assign, best, sizes int64, new centres f32).  The sums are exact in float64; the mean and the
    renormalisation are float32 operations on them, as in coati_amd.cluster."""
    k = centres.shape[0]
    _, c16, cbias = prepare_centres(centres, metric)
    a, best = assign(x16, row_bias, c16, cbias)
    sizes = torch.bincount(a[a >= 0].long(), minlength=k)
    mean = sums(x16, a, k).float() / sizes.clamp_min(1).float()[:, None]
    if metric == "cosine":
        mean = mean / mean.norm(dim=1, keepdim=True).clamp_min(1e-30)
    return a, best, sizes, torch.where((sizes > 0)[:, None], mean, centres.float().cpu())


def kmeans(x16, row_bias, metric, init, iters=20):
    """the loop of kmeans_rows from given initial centres: dict(centres, assign, sizes, iterations, converged)"""
    centres, _, _ = prepare_centres(init, metric)
    prev, iterations = None, 0
    while True:
        a, _, sizes, new = lloyd_round(x16, row_bias, centres, metric)
        converged = prev is not None and torch.equal(a, prev)
        if converged or iterations == iters:
            break
        centres, prev, iterations = new, a, iterations + 1
    return dict(centres=centres, assign=a, sizes=sizes, iterations=iterations, converged=converged)


def representatives(assign_, values, k):
    """[k] int64: per cluster the member with the largest value, the lowest row among equal values; -1 for an empty cluster"""
    out = []
    for c in range(k):
        rows = torch.nonzero(assign_.cpu() == c).reshape(-1)
        if rows.numel() == 0:
            out.append(-1)
            continue
        v = values.cpu()[rows]
        out.append(int(rows[torch.nonzero(v == v.max()).reshape(-1)[0]]))
    return torch.tensor(out, dtype=torch.int64)
