"""A pure-torch restatement of the radius search of include/coati_radius.h, in float64, for the tests, on top of
search_util.index_scores: the hits of a query are the live rows with score >= threshold and row < row_below, row-ascending, in CSR form.
And the greedy leader rule of EmbeddingIndex.dedup, restated over such a CSR."""
import torch

from tests import search_util

NEG_INF = float("-inf")


def csr_of(s, thr, row_below=None):
    """(offsets int64 [Q + 1], scores float64 [T], rows int64 [T]) of a score matrix [Q, N] (a removed row is -inf there): per query
    the rows with -inf < s, s >= thr[q] and row < row_below[q], in ascending row order"""
    Q, N = s.shape
    thr = torch.as_tensor(thr).to(device=s.device, dtype=torch.float64)        # (an f32 threshold is exact in float64)
    thr = thr.expand(Q) if thr.dim() == 0 else thr
    hit = (s > NEG_INF) & (s >= thr[:, None])
    if row_below is not None:
        hit &= torch.arange(N, device=s.device)[None, :] < torch.as_tensor(row_below).to(s.device)[:, None]
    offsets = torch.zeros(Q + 1, dtype=torch.int64, device=s.device)
    offsets[1:] = hit.sum(dim=1).cumsum(0)
    qi, rows = hit.nonzero(as_tuple=True)               # row-major: query ascending, then row ascending
    return offsets, s[qi, rows], rows


def index_radius(index, queries, thr, row_below=None):
    """the oracle of EmbeddingIndex.radius_search(queries, thr, order="row", row_below=row_below), and the score matrix"""
    s = search_util.index_scores(index, queries)
    return csr_of(s, thr, row_below) + (s,)


def by_score(offsets, scores, rows):
    """every segment by score descending, row ascending among equal scores (two stable sorts, segment by segment)"""
    s_out, r_out = [], []
    for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist()):
        order = torch.sort(scores[a:b], descending=True, stable=True).indices          # the segment arrives row-ascending
        s_out.append(scores[a:b][order])
        r_out.append(rows[a:b][order])
    return (torch.cat(s_out), torch.cat(r_out)) if s_out else (scores, rows)


def self_scores(index):
    """[N, N] float64: the metric's scores of the STORED bf16 rows against themselves (not prepared again), removed columns at -inf"""
    from coati_amd import search as S
    x = index.vectors
    s = search_util.score_matrix(x, index.bias, x, S.metric_alpha(index.metric))
    if index.metric == "l2":
        s = (s - (x.to(torch.float64) ** 2).sum(dim=1, keepdim=True)).clamp_max(0.0)
    return s


def index_near_duplicates(index, thr):
    """the oracle of EmbeddingIndex.near_duplicates(thr): for every live row the earlier live rows with score >= thr"""
    s = self_scores(index)
    N = s.shape[0]
    live = index.bias > NEG_INF
    t = torch.where(live, torch.full((N,), float(thr), dtype=torch.float64, device=s.device),
                    torch.full((N,), float("inf"), dtype=torch.float64, device=s.device))
    return csr_of(s, t, torch.arange(N, device=s.device))


def greedy(offsets, rows, live):
    """keep mask [N] (a list of bool): in row order, a live row is kept iff none of its earlier neighbours is kept"""
    offsets, rows = [int(v) for v in offsets], [int(v) for v in rows]
    keep = []
    for i, alive in enumerate(bool(v) for v in live):
        keep.append(alive and not any(keep[j] for j in rows[offsets[i]:offsets[i + 1]]))
    return keep
