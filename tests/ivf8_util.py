"""Helpers of tests/test_ivf8_cpu.py and tests/test_gpu_ivf8.py: the float64 restatement of stage 1 of the IVF search over fp8 lists
(include/coati_ivf8.h) -- tests/search8_util.py's arithmetic (dequantised rows, dequantised queries) under tests/ivf_util.py's masking
(only the probed lists, ties by ORIGINAL row) -- and a hand-put-together Ivf8Index for the host-side tests."""
import torch

from tests import ivf_util, search_util

NEG_INF = float("-inf")


def dequantised_queries(ivf8, queries):
    """f32 [Q, dim_padded]: the queries as stage 1 sees them -- prepared for the metric, rounded to bf16, quantised, dequantised"""
    from coati_amd import fp8_index as F, search as S
    _, q16 = S.prepare_queries(queries, ivf8.metric, ivf8.dim, "cpu")
    return F.dequantise(*F.quantise_rows(q16))


def score_matrix8(ivf8, queries, extra=None):
    """([Q, M] float64 by POSITION, q_hat): stage 1's score under the metric for every stored position -- alpha q_hat . x_hat + bias
    (+ extra [N] by original row), for l2 minus |q_hat|^2 and at most 0; a removed row is -inf.  search8_util.stage1_scores' arithmetic."""
    from coati_amd import search as S
    q_hat = dequantised_queries(ivf8, queries)
    bias = ivf8.bias.cpu()
    if extra is not None:
        bias = bias + extra.cpu()[ivf8.ids.long().cpu()]
    s = search_util.score_matrix(ivf8.dequantised().cpu(), bias, q_hat, S.metric_alpha(ivf8.metric))
    if ivf8.metric == "l2":
        s = (s - (q_hat.double() ** 2).sum(dim=1, keepdim=True)).clamp_max(0.0)
    return s, q_hat


def probed_mask(ivf8, probes):
    """bool [Q, M]: the positions of every query's probed lists (ivf_util.scan's masking)"""
    probes = torch.as_tensor(probes).long().cpu()
    list_off = ivf8.list_offsets.long().cpu()
    M, L = int(list_off[-1]), list_off.shape[0] - 1
    list_of = torch.bucketize(torch.arange(M), list_off[1:], right=True)
    probed = torch.zeros(probes.shape[0], L + 1, dtype=torch.bool)
    probed.scatter_(1, torch.where(probes < 0, torch.full_like(probes, L), probes), True)
    return probed[:, :L][:, list_of]


def scan8(ivf8, queries, probes, k, extra=None):
    """the oracle of Ivf8Index.search(queries, k, probes=probes, rescore=False, bias=extra): (scores [Q, k] float64, rows [Q, k] int64
    ORIGINAL rows, the masked score matrix [Q, M] by position)"""
    s, _ = score_matrix8(ivf8, queries, extra)
    s = torch.where(probed_mask(ivf8, probes), s, torch.full_like(s, NEG_INF))
    ids = ivf8.ids.long().cpu()
    order = torch.argsort(ids, stable=True)                                  # positions in original-row order: ties by original row
    val, idx = search_util.topk(s[:, order], k)
    return val, torch.where(idx >= 0, ids[order][idx.clamp_min(0)], idx), s


def by_hand(x, assign, metric="l2", keep_rows=True, nlist=None, device="cpu"):
    """(Ivf8Index, EmbeddingIndex) put together without a kernel: rows x [N, dim], lists assign [N] (-1 = left out), centres = the
    lists' means (zeros for an empty list), the bytes by quantise_rows -- Ivf8Index.build's layout rules restated"""
    from coati_amd import fp8_index as F
    from coati_amd.ivf8 import Ivf8Index, stage1_bias
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(x.shape[1], metric=metric, device=device)
    index.add(x)
    assign = torch.as_tensor(assign)
    L = int(assign.max()) + 1 if nlist is None else nlist
    ids, off = ivf_util.inverted(assign, L)
    centres = torch.stack([x[assign == l].mean(dim=0) if bool((assign == l).any()) else torch.zeros(x.shape[1]) for l in range(L)])
    rows16 = index.vectors[ids.to(index.device)]
    vec8, scale = F.quantise_rows(rows16)
    bias = stage1_bias(metric, vec8, scale, index.bias[ids.to(index.device)])
    ivf8 = Ivf8Index(index.dim, index.dim_padded, metric, len(index), centres, vec8, scale, ids, bias, off[1:] - off[:-1],
                     index.vectors if keep_rows else None, index.bias.clone() if keep_rows else None, device)
    return ivf8, index
