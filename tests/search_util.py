"""A pure-torch restatement of the embedding-library search of include/coati_search.h, in float64, for the tests: scores from the
STORED bf16 rows and the bf16-rounded queries, a stable descending sort (row index ascending among equal scores), rows whose score is
-inf never returned, padding with (-inf, -1).  And the synthetic data test_gpu_search.py and test_gpu_ivf.py share."""
import torch

NEG_INF = float("-inf")


def score_matrix(rows16, bias, q16, alpha=1.0):
    """[Q, N] float64: alpha * q . x + bias of bf16 (or any exactly representable) operands; a zero is +0"""
    s = alpha * (q16.to(torch.float64) @ rows16.to(torch.float64).T)
    if bias is not None:
        s = s + bias.to(torch.float64)[None, :]
    return s + 0.0


def topk(s, k):
    """(scores [Q, k] float64, rows [Q, k] int64) of a score matrix [Q, N]: score descending, row ascending among equal scores; what is
    -inf is not a result, and what is missing is (-inf, -1)"""
    Q, N = s.shape
    val, idx = torch.sort(s, dim=1, descending=True, stable=True)
    val, idx = val[:, :k], idx[:, :k]
    idx = torch.where(val == NEG_INF, torch.full_like(idx, -1), idx)
    if k > N:
        val = torch.cat([val, torch.full((Q, k - N), NEG_INF, dtype=val.dtype, device=val.device)], dim=1)
        idx = torch.cat([idx, torch.full((Q, k - N), -1, dtype=idx.dtype, device=idx.device)], dim=1)
    return val, idx


def search(rows16, bias, q16, k, alpha=1.0):
    return topk(score_matrix(rows16, bias, q16, alpha), k)


def index_scores(index, queries):
    """The metric's scores [Q, N] float64 of an EmbeddingIndex's stored rows for `queries` as the index prepares them (normalised for
    cosine, rounded to bf16): dot / cosine = q . x, l2 = min(2 q . x - |x|^2 - |q|^2, 0) with a removed row at -inf."""
    from coati_amd import search as S
    _, q16 = S.prepare_queries(queries, index.metric, index.dim, index.vectors.device)
    s = score_matrix(index.vectors, index.bias, q16, S.metric_alpha(index.metric))
    if index.metric == "l2":
        s = (s - (q16.to(torch.float64) ** 2).sum(dim=1, keepdim=True)).clamp_max(0.0)
    return s


def index_search(index, queries, k):
    """the oracle of EmbeddingIndex.search(queries, k): (scores [Q, k] float64, rows [Q, k] int64, the score matrix)"""
    s = index_scores(index, queries)
    val, idx = topk(s, k)
    return val, idx, s


def stage1_scores(index, q_hat, extra=None):
    """[Q, N] float64: stage 1's score of a two-stage index (Fp8Index, Fp4Index, PQIndex) under its metric for the queries q_hat as its
    stage 1 sees them -- alpha q_hat . x_hat + bias (+ extra) from index.dequantised(), for l2 minus |q_hat|^2 and at most 0; a removed
    row is -inf.  On the CPU."""
    from coati_amd import search as S
    bias = index.bias.cpu() if extra is None else index.bias.cpu() + extra.cpu()
    s = score_matrix(index.dequantised().cpu(), bias, q_hat, S.metric_alpha(index.metric))
    if index.metric == "l2":
        s = (s - (q_hat.double() ** 2).sum(dim=1, keepdim=True)).clamp_max(0.0)
    return s


def stage1_search(index, q_hat, k, extra=None):
    """the oracle of index.search(queries, k, rescore=False): (scores [Q, k] float64, rows [Q, k] int64, the score matrix)"""
    s = stage1_scores(index, q_hat, extra)
    val, idx = topk(s, k)
    return val, idx, s


def two_stage_search(cand, index, queries, k):
    """the oracle of the two stages: the best k by index's exact float64 score among stage 1's candidates cand [Q, R] (-1 = none)"""
    exact = index_scores(index, queries)
    picked = torch.full_like(exact, NEG_INF)
    ok = cand >= 0
    picked.scatter_(1, cand.clamp_min(0), torch.where(ok, exact.gather(1, cand.clamp_min(0)), torch.full_like(exact[:, :1], NEG_INF).expand_as(cand)))
    return topk(picked, k)


def recall(rows, exact_rows):
    """the fraction of the exact result's rows (>= 0) that `rows` holds, over all queries"""
    rows, exact_rows = rows.cpu(), exact_rows.cpu()
    want = exact_rows >= 0
    hit = (exact_rows[:, :, None] == rows[:, None, :]).any(dim=2) & want
    return float(hit.sum()) / max(int(want.sum()), 1)


def clustered(N, E, seed, centres=200, noise=0.5):
    """rows [N, E] and queries from the same law: `centres` Gaussian centres plus noise-sigma Gaussian noise"""
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(centres, E, generator=g)
    return lambda n: c[torch.randint(0, centres, (n,), generator=g)] + noise * torch.randn(n, E, generator=g)


def ints(shape, seed, lo=-4, hi=4):
    """integer-valued f32 in lo .. hi: every score is exact, and ties abound"""
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).to(torch.float32)


def canon(s):
    if not s or "X" in s:
        return None
    return min(s, s[::-1])


def strings(tokens, n, seed):
    """n distinct strings of 2 .. 6 tokens that are their own canonical form"""
    g = torch.Generator().manual_seed(seed)
    out, seen = [], set()
    while len(out) < n:
        s = "".join(tokens[int(i)] for i in torch.randint(0, len(tokens), (int(torch.randint(2, 7, (1,), generator=g)),), generator=g))
        if canon(s) == s and s not in seen:
            seen.add(s)
            out.append(s)
    return out
