"""Helpers of tests/test_ivfpq_cpu.py and tests/test_gpu_ivfpq.py: float64 restatements of the IVF-PQ storage rule (residuals, x_hat) and
of its two stages -- tests/pq_util.py's arithmetic on x_hat = centre + entry under tests/ivf_util.py's masking (only the probed lists,
ties by ORIGINAL row) -- and an IvfPqIndex put together through the constructor for the host-side tests."""
import torch

from tests import ivf8_util, ivf_util, search_util

NEG_INF = float("-inf")


def position_lists(list_off):
    """int64 [M]: the list of every position, from list_off [L + 1]"""
    list_off = torch.as_tensor(list_off).long().cpu()
    return torch.bucketize(torch.arange(int(list_off[-1])), list_off[1:], right=True)


def residuals(x16, ids, list_off, c16):
    """bf16 [M, E]: the storage rule restated -- the exact difference of the bf16 row and its list's bf16 centre (float64), rounded to f32
    and then to bf16"""
    lists = position_lists(list_off)
    return (x16.cpu()[torch.as_tensor(ids).long().cpu()].double() - c16.cpu()[lists].double()).float().to(torch.bfloat16)


def x_hat(ivfpq):
    """float64 [M, E] by position: the list's bf16 centre plus the code-book entries the codes name, exact"""
    cb, codes = ivfpq.codebooks.cpu(), ivfpq.codes.cpu().long()
    entry = cb[torch.arange(cb.shape[0])[None, :], codes].reshape(codes.shape[0], -1)
    return ivfpq.centres16.cpu()[position_lists(ivfpq.list_offsets)].double() + entry.double()


def score_matrix(ivfpq, queries, extra=None):
    """([Q, M] float64 by POSITION, q16): stage 1's score under the metric -- alpha q . x_hat + bias (+ extra [N] by original row), for
    l2 minus |q|^2 and at most 0; a removed row is -inf"""
    from coati_amd import search as S
    _, q16 = S.prepare_queries(queries, ivfpq.metric, ivfpq.dim, "cpu")
    bias = ivfpq.bias.cpu()
    if extra is not None:
        bias = bias + extra.cpu()[ivfpq.ids.long().cpu()]
    s = S.metric_alpha(ivfpq.metric) * (q16.double() @ x_hat(ivfpq).T) + bias.double()[None, :] + 0.0
    if ivfpq.metric == "l2":
        s = (s - (q16.double() ** 2).sum(dim=1, keepdim=True)).clamp_max(0.0)
    return s, q16


def scan(ivfpq, queries, probes, k, extra=None):
    """the oracle of IvfPqIndex.search(queries, k, probes=probes, rescore=False, bias=extra): (scores [Q, k] float64, rows [Q, k] int64
    ORIGINAL rows, the masked score matrix [Q, M] by position)"""
    s, _ = score_matrix(ivfpq, queries, extra)
    s = torch.where(ivf8_util.probed_mask(ivfpq, probes), s, torch.full_like(s, NEG_INF))
    ids = ivfpq.ids.long().cpu()
    order = torch.argsort(ids, stable=True)                                  # positions in original-row order: ties by original row
    val, idx = search_util.topk(s[:, order], k)
    return val, torch.where(idx >= 0, ids[order][idx.clamp_min(0)], idx), s


def two_stage(ivfpq, index, queries, probes, k, R):
    """the oracle of the two stages: the best k by index's exact float64 score among stage 1's best R rows of the probed lists"""
    _, cand, _ = scan(ivfpq, queries, probes, R)
    exact = search_util.index_scores(index, queries).cpu()
    picked = torch.full_like(exact, NEG_INF)
    ok = cand >= 0
    picked.scatter_(1, cand.clamp_min(0), torch.where(ok, exact.gather(1, cand.clamp_min(0)), torch.full_like(exact[:, :1], NEG_INF).expand_as(cand)))
    return search_util.topk(picked, k)


def by_hand(x, assign, centres, metric="l2", keep_rows=True, codebooks=None, device="cpu", **fit):
    """(IvfPqIndex, EmbeddingIndex) put together through the constructor, without make_lists: rows x [N, dim], lists assign [N] (-1 = left
    out), centres [L, dim]; the codes and the bias by the package's encode_lists, the code books given or by its fit_residual_codebooks"""
    from coati_amd import cluster, ivfpq as P
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(x.shape[1], metric=metric, device=device)
    index.add(x)
    L = centres.shape[0]
    ids, off = ivf_util.inverted(torch.as_tensor(assign), L)
    ids, sizes = ids.to(index.device), (off[1:] - off[:-1]).to(index.device)
    c16 = cluster.prepare_centres(centres, metric, index.dim_padded, index.device)[1]
    x16, bias16 = index.vectors, index.bias
    if codebooks is None:
        codebooks = P.fit_residual_codebooks(lambda pos: x16[ids[pos]], ids.shape[0], sizes, c16, **fit)
    codes, bias = P.encode_lists(metric, lambda pos: x16[ids[pos]], lambda pos: bias16[ids[pos]], ids.shape[0], sizes, c16, codebooks.to(index.device))
    return P.IvfPqIndex(index.dim, index.dim_padded, metric, len(index), centres, codes, codebooks, ids, bias, sizes,
                        x16 if keep_rows else None, bias16.clone() if keep_rows else None, device), index
