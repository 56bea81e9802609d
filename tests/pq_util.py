"""Helpers of tests/test_pq_cpu.py and tests/test_gpu_pq.py: float64 restatements of the product-quantised search's encoder and of its
two stages on top of tests/search_util.py (whose oracle and tie rule they reuse), and the hand-made code books that make a library
lossless."""
import torch

from tests import search_util
from tests.search_util import clustered, recall  # noqa: F401  (the tests reach both through this module)

NEG_INF = float("-inf")


def distances64(x16, codebooks):
    """[n, M, 256] float64: the squared distance of every sub-vector of bf16 rows [n, E] to every entry of code books [M, 256, 8]"""
    M = codebooks.shape[0]
    x = x16.to(torch.float64).reshape(-1, M, 1, 8)
    return ((x - codebooks.to(torch.float64)[None]) ** 2).sum(dim=3)


def encode64(x16, codebooks):
    """uint8 [n, M]: the brute force in float64, the lowest index among equal distances"""
    d = distances64(x16, codebooks)
    idx = torch.arange(256)
    return torch.where(d == d.amin(dim=2, keepdim=True), idx, 256).amin(dim=2).to(torch.uint8)


def int_codebooks(M, seed, duplicates=False):
    """bf16 [M, 256, 8] of integers of magnitude <= 15 whose entries are distinct within a sub-space: the first two values spell the
    entry's index.  duplicates: entries 128 .. 255 repeat entries 0 .. 127, so that the lowest index has to win."""
    cb = search_util.ints((M, 256, 8), seed, -15, 15)
    e = torch.arange(256)
    cb[:, :, 0], cb[:, :, 1] = (e // 16 - 8)[None, :], (e % 16 - 8)[None, :]
    if duplicates:
        cb[:, 128:] = cb[:, :128]
    return cb.to(torch.bfloat16)


def composed_rows(codebooks, N, seed, distinct=256):
    """(rows f32 [N, E], codes uint8 [N, M]): rows put together from random entries (of the first `distinct`) of the code books --
    a library that product quantisation holds without loss"""
    M = codebooks.shape[0]
    codes = torch.randint(0, distinct, (N, M), generator=torch.Generator().manual_seed(seed))
    rows = codebooks[torch.arange(M)[None, :], codes].reshape(N, M * 8).to(torch.float32)
    return rows, codes.to(torch.uint8)


def stage1_scores(pq, queries, extra=None):
    """([Q, N] float64, q16): stage 1's score under the metric, from the RECONSTRUCTED rows and the bf16 queries
    (search_util.stage1_scores)"""
    from coati_amd import search as S
    _, q16 = S.prepare_queries(queries, pq.metric, pq.dim, "cpu")
    return search_util.stage1_scores(pq, q16, extra), q16


def stage1_search(pq, queries, k, extra=None):
    """the oracle of PQIndex.search(queries, k, rescore=False): (scores [Q, k] float64, rows [Q, k] int64, the score matrix)"""
    from coati_amd import search as S
    return search_util.stage1_search(pq, S.prepare_queries(queries, pq.metric, pq.dim, "cpu")[1], k, extra)


def two_stage_search(pq, index, queries, k, R):
    """the oracle of the two stages: the best k by index's exact float64 score among stage 1's best R rows"""
    return search_util.two_stage_search(stage1_search(pq, queries, R)[1], index, queries, k)
