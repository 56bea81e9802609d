"""What the mixture tests share (no GPU): the one generator of clustered test libraries, the common start of every EM run, and the
kernels' forward error bound."""
import functools

import torch

LIBRARIES = {"a": (20000, 64, 12, 8, 0.5), "b": (20000, 256, 40, 16, 0.5), "c": (3000, 32, 3, 17, 0.4)}      # (N, dim, C, K, noise)


@functools.lru_cache(maxsize=None)
def library(N, dim, C, noise):
    """unit rows around C centres with per-centre, per-dimension scales, rounded to bf16: [N, dim] bf16"""
    g = torch.Generator().manual_seed(1)
    cent = torch.randn(C, dim, generator=g)
    lab = torch.randint(0, C, (N,), generator=g)
    scale = 0.5 + torch.rand(C, dim, generator=g)
    x = cent[lab] + noise * scale[lab] * torch.randn(N, dim, generator=g)
    return (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)


def labels(N, dim, C):
    """[N] int64: the cluster each row of library(N, dim, C, noise) was drawn around (the generator's own draws, repeated)"""
    g = torch.Generator().manual_seed(1)
    torch.randn(C, dim, generator=g)
    return torch.randint(0, C, (N,), generator=g)


@functools.lru_cache(maxsize=None)
def common_start(N, dim, C, noise, K):
    """(weights, means, variances) float64: the rows randperm(N, seed 2)[:K] improved by 5 Lloyd rounds in float64 (an empty cluster keeps
    its centre), every variance the global per-dimension variance + 1e-6, weights 1 / K"""
    x = library(N, dim, C, noise).double()
    c = x[torch.randperm(N, generator=torch.Generator().manual_seed(2))[:K]].clone()
    for _ in range(5):
        a = torch.cdist(x, c).argmin(dim=1)
        for k in range(K):
            if bool((a == k).any()):
                c[k] = x[a == k].mean(dim=0)
    var = (x.var(dim=0, unbiased=False) + 1e-6).expand(K, dim).clone()
    return torch.full((K,), 1.0 / K, dtype=torch.float64), c, var


def padded(x16, E):
    return x16 if x16.shape[1] == E else torch.nn.functional.pad(x16, (0, E - x16.shape[1]))


def logit_bound(x16, par, cst):
    """[N] float64: (2E + 8) 2^-24 max_k (sum_d |x p1| + |x^2 p2| + |cst|), the forward error bound of an f32 dot product of that length
    in any order"""
    x = x16.double()
    E = x16.shape[1]
    mag = torch.cat([x.abs(), x * x], dim=1) @ par.double().abs().T + cst.double().abs()
    return (2 * E + 8) * 2.0 ** -24 * mag.max(dim=1).values
