"""Helpers of tests/test_search8_cpu.py and tests/test_gpu_search8.py: float64 restatements of the quantised search's two stages on
top of tests/search_util.py (whose oracle, data and tie rule they reuse), and the hand-made rows that pin the quantiser."""
import torch

from tests import search_util
from tests.search_util import clustered  # noqa: F401  (the tests reach the clustered generator through this module)

NEG_INF = float("-inf")


def query_hat(fp8, queries):
    """f32 [Q, E]: the dequantised e4m3 queries of Fp8Index.search, computed on the CPU with torch's float8_e4m3fn"""
    from coati_amd import fp8_index as F, search as S
    _, q16 = S.prepare_queries(queries, fp8.metric, fp8.dim, "cpu")
    return F.dequantise(*F.quantise_rows(q16))


def stage1_scores(fp8, queries, extra=None):
    """([Q, N] float64, q_hat): stage 1's score under the metric, from the DEQUANTISED rows and the dequantised queries
    (search_util.stage1_scores)"""
    q_hat = query_hat(fp8, queries)
    return search_util.stage1_scores(fp8, q_hat, extra), q_hat


def stage1_search(fp8, queries, k, extra=None):
    """the oracle of Fp8Index.search(queries, k, rescore=False): (scores [Q, k] float64, rows [Q, k] int64, the score matrix)"""
    return search_util.stage1_search(fp8, query_hat(fp8, queries), k, extra)


def quantiser_rows(n, E, seed):
    """bf16 rows [n, E]: Gaussian ones and, as far as n allows, the hand-made ones -- a row of zeros, rows whose largest magnitude is
    exactly 448 * 2^j and the next bf16 value above it (the scale steps between the two), a row with entries so far below its largest
    that they land in e4m3's subnormals (below 2^-6 after scaling) or round to zero, and negative zeros."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, E, generator=g) * torch.exp(3 * torch.randn(n, 1, generator=g))).to(torch.bfloat16)
    special = []
    special.append(torch.zeros(E))
    for j in (-9, 0, 5):
        edge = torch.full((E,), 0.25 * 2.0 ** j)
        edge[E // 2] = -448.0 * 2.0 ** j                                   # bf16 holds 448 = 1.75 * 2^8 exactly
        special.append(edge)
        above = edge.clone()
        above[E // 2] = 450.0 * 2.0 ** j                                   # the next bf16 value: 1.7578125 * 2^8
        special.append(above)
    small = torch.zeros(E)
    small[0] = 300.0
    small[1:9] = torch.tensor([2.0 ** -7, 3 * 2.0 ** -9, -(2.0 ** -9), 2.0 ** -10, -(2.0 ** -11), 5 * 2.0 ** -9, 2.0 ** -6, -7 * 2.0 ** -9])
    special.append(small)
    negz = torch.randn(E, generator=g)
    negz[::3] = -0.0
    special.append(negz)
    allneg = torch.full((E,), -0.0)
    special.append(allneg)
    for i, row in enumerate(special[:n]):
        x[n - 1 - i] = row.to(torch.bfloat16)
    return x


def hex_library(kind, N=4096):
    """one query q = (256, 16, 1, 0, ...) and rows (a, b, c, 0, ...) with hex digits a, b, c: score = 256 a + 16 b + c, exact in e4m3 and
    f32.  ascending / descending: the digits of n / of N - 1 - n; constant: (1, 2, 3); blocks: c = (n // 100) % 2 under a = 9.  The rows'
    largest digits differ, and so do their scales."""
    n = torch.arange(N)
    x = torch.zeros(N, 32)
    if kind == "ascending":
        v = n
    elif kind == "descending":
        v = N - 1 - n
    if kind in ("ascending", "descending"):
        x[:, 0], x[:, 1], x[:, 2] = v // 256, (v // 16) % 16, v % 16
    elif kind == "constant":
        x[:, 0], x[:, 1], x[:, 2] = 1, 2, 3
    else:
        x[:, 0], x[:, 2] = 9, (n // 100) % 2
    q = torch.zeros(1, 32)
    q[0, 0], q[0, 1], q[0, 2] = 256, 16, 1
    return x, q
