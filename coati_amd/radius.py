"""Radius search over an EmbeddingIndex (include/coati_radius.h, csrc/radius.hip): every library row within a threshold of each query, in
CSR form, and what is built on it -- local densities, the near-duplicate self-join and greedy deduplication.

    offsets, scores, rows = index.radius_search(queries, 0.9)       # query i's hits are [offsets[i], offsets[i + 1]), row ascending
    counts = index.radius_count(queries, 0.9)                       # int64 [Q], the count pass alone
    keep = index.dedup(0.999)                                       # bool [N]: the first of every group of near-duplicates

The answer has no k: a count pass over the library's slices, a prefix sum, ONE .item() for the total, an allocation, and a fill pass that
computes the scores again and writes the hits in ascending row order.  A (query, row) score has the bits EmbeddingIndex.search returns
for it, the l2 score included (the same single f32 subtraction of |q|^2 and the same clamp at 0), and no result depends on the slices.
The host logic here works on prepared operands (bf16 queries, f32 thresholds); the EmbeddingIndex methods are thin wrappers.  There is no
CPU fallback.  The reference has no counterpart."""
import torch

from . import _lib
from .ops import ptr, stream
from .search import metric_alpha, prepare_queries

ORDERS = ("row", "score")
MAX_RESULTS = 1 << 28
S_MAX = 65535                    # the grid's y limit
SELF_JOIN_SLICE_ROWS = 2048      # near_duplicates: slices about this long, so that the triangle's workgroups are many and even
SELF_JOIN_S_MAX = 4096


def thresholds(threshold, Q, device, what):
    """f32 [Q] on `device` from a float or a [Q] tensor"""
    if isinstance(threshold, torch.Tensor):
        if threshold.dim() == 0:
            threshold = threshold.reshape(1).expand(Q)
        if tuple(threshold.shape) != (Q,):
            raise ValueError(f"{what}: threshold must be a float or a [{Q}] tensor, got {tuple(threshold.shape)}")
        return threshold.detach().to(device=device, dtype=torch.float32).contiguous()
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)):
        raise ValueError(f"{what}: threshold must be a float or a [{Q}] tensor, got {type(threshold).__name__}")
    return torch.full((Q,), float(threshold), dtype=torch.float32, device=device)


def row_bounds(row_below, Q, device, what):
    """int32 [Q] on `device`, or None"""
    if row_below is None:
        return None
    r = torch.as_tensor(row_below)
    if r.dtype.is_floating_point or r.dtype == torch.bool or tuple(r.shape) != (Q,):
        raise ValueError(f"{what}: row_below must be an integer [{Q}] tensor")
    return r.detach().to(device=device, dtype=torch.int64).clamp(0, 2 ** 31 - 1).to(torch.int32).contiguous()


def check_slices(slices, what):
    if slices is not None and (int(slices) < 1 or int(slices) > S_MAX):
        raise ValueError(f"{what}: slices={slices} outside 1 .. {S_MAX}")


def default_slices(n, Q):
    S = _lib.lib().coati_radius_slices(n, Q)
    if S < 1:
        raise RuntimeError(f"coati_radius_slices({n}, {Q}) = {S}: {_lib.lib().coati_last_error().decode('utf-8', 'replace')}")
    return S


def self_join_slices(n, Q):
    return min(max(default_slices(n, Q), -(-n // SELF_JOIN_SLICE_ROWS)), SELF_JOIN_S_MAX)


class Operands:
    """the kernel's operands for one set of prepared queries: lib [n, E] bf16 and bias [>= n] f32 on a GPU, q16 [Q, E] bf16, thr [Q] f32,
    sub [Q] f32 or None, row_hi [Q] int32 or None, S slices"""

    def __init__(self, vec, n, bias, q16, alpha, sub, clamp0, thr, row_hi, S):
        self.vec, self.n, self.bias, self.q16, self.alpha, self.sub, self.clamp0 = vec, int(n), bias, q16.contiguous(), float(alpha), sub, int(clamp0)
        self.thr, self.row_hi, self.S = thr, row_hi, int(S)

    def _common(self):
        return (ptr(self.vec), self.n, self.vec.shape[1], ptr(self.bias), ptr(self.q16), self.q16.shape[0], self.alpha, ptr(self.sub), self.clamp0,
                ptr(self.thr), ptr(self.row_hi), self.S)

    def count(self):
        """counts [Q, S] int32"""
        counts = torch.empty(self.q16.shape[0], self.S, dtype=torch.int32, device=self.vec.device)
        with torch.cuda.device(self.vec.device):
            _lib.call("coati_radius_count", *self._common(), ptr(counts), stream())
        return counts

    def search(self, max_results, what):
        """(offsets int64 [Q + 1], scores f32 [T], rows int64 [T]): count, prefix sum, one .item(), allocate, fill"""
        Q, dev = self.q16.shape[0], self.vec.device
        counts = self.count().view(-1)
        incl = counts.cumsum(0, dtype=torch.int64)
        total = int(incl[-1].item())                                        # the only synchronisation
        if total > max_results:
            raise ValueError(f"{what}: {total} results exceed max_results={max_results}")
        offsets = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
        offsets[1:] = incl.view(Q, self.S)[:, -1]
        scores = torch.empty(total, dtype=torch.float32, device=dev)
        rows = torch.empty(total, dtype=torch.int64, device=dev)
        if total > 0:
            excl = (incl - counts).contiguous()
            with torch.cuda.device(dev):
                _lib.call("coati_radius_fill", *self._common(), ptr(counts), ptr(excl), ptr(scores), ptr(rows), stream())
        return offsets, scores, rows


def sort_segments_by_score(offsets, scores, rows):
    """every CSR segment by score descending, row ascending among equal scores (the segments arrive row-ascending): ONE stable sort on
    the key (segment, order-reversed score bits)"""
    T = scores.numel()
    if T == 0:
        return scores, rows
    seg = torch.repeat_interleave(torch.arange(offsets.numel() - 1, device=scores.device), offsets[1:] - offsets[:-1], output_size=T)
    b = (scores + 0.0).view(torch.int32).to(torch.int64) & 0xFFFFFFFF        # the f32 bits, -0 as +0
    up = torch.where(b >= 2 ** 31, 0xFFFFFFFF - b, b + 2 ** 31)              # ascending with the score
    order = ((seg << 32) | (0xFFFFFFFF - up)).sort(stable=True).indices
    return scores[order], rows[order]


def greedy_leaders(offsets, rows, live):
    """bool [N] keep mask of the greedy leader rule in row order over a CSR of EARLIER neighbours (rows[offsets[i] : offsets[i + 1]] < i): a
    live row is kept iff none of its earlier neighbours is kept.  CPU tensors; only the rows that have a neighbour are visited."""
    offsets, rows = offsets.cpu().numpy(), rows.cpu().numpy()
    keep = live.cpu().clone().numpy()
    for i in (offsets[1:] > offsets[:-1]).nonzero()[0]:
        if keep[i] and keep[rows[offsets[i]:offsets[i + 1]]].any():
            keep[i] = False
    return torch.from_numpy(keep)


# ---- on an EmbeddingIndex ------------------------------------------------------------------------------------------------------------
def _need_gpu(index, what):
    if index.device.type != "cuda":
        raise RuntimeError(f"EmbeddingIndex.{what}: the index is not on a GPU; there is no CPU fallback")


def _empty(index, Q):
    dev = index.device
    return (torch.zeros(Q + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.float32, device=dev),
            torch.empty(0, dtype=torch.int64, device=dev))


def _query_operands(index, queries, threshold, row_below, slices, what):
    """validated arguments -> Operands (None when there is nothing to search), Q"""
    check_slices(slices, what)
    _, q16 = prepare_queries(queries, index.metric, index.dim, index.device)
    Q = q16.shape[0]
    thr = thresholds(threshold, Q, index.device, what)
    row_hi = row_bounds(row_below, Q, index.device, what)
    if Q == 0 or len(index) == 0:
        return None, Q
    _need_gpu(index, what.split(".")[-1])
    l2 = index.metric == "l2"
    sub = (q16.float() ** 2).sum(dim=1).contiguous() if l2 else None          # finish_scores' |q|^2, the same reduction
    S = int(slices) if slices is not None else default_slices(len(index), Q)
    return Operands(index._vec, len(index), index._bias, q16, metric_alpha(index.metric), sub, l2, thr, row_hi, S), Q


def radius_count(index, queries, threshold, row_below=None):
    ops, Q = _query_operands(index, queries, threshold, row_below, None, "EmbeddingIndex.radius_count")
    if ops is None:
        return torch.zeros(Q, dtype=torch.int64, device=index.device)
    return ops.count().sum(dim=1, dtype=torch.int64)


def radius_search(index, queries, threshold, order="row", row_below=None, slices=None, max_results=MAX_RESULTS):
    what = "EmbeddingIndex.radius_search"
    if order not in ORDERS:
        raise ValueError(f"{what}: order {order!r} is not one of {ORDERS}")
    if isinstance(max_results, bool) or not isinstance(max_results, int) or max_results < 0:
        raise ValueError(f"{what}: max_results={max_results!r} is not a non-negative int")
    ops, Q = _query_operands(index, queries, threshold, row_below, slices, what)
    if ops is None:
        return _empty(index, Q)
    offsets, scores, rows = ops.search(max_results, what)
    if order == "score":
        scores, rows = sort_segments_by_score(offsets, scores, rows)
    return offsets, scores, rows


def near_duplicates(index, threshold, chunk=4096):
    what = "EmbeddingIndex.near_duplicates"
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"{what}: chunk={chunk} < 1")
    n = len(index)
    thr_all = thresholds(threshold, 1, index.device, what)[0]
    if n == 0:
        return _empty(index, 0)
    _need_gpu(index, "near_duplicates")
    l2 = index.metric == "l2"
    vec, bias = index.vectors, index.bias
    inf = torch.full((), float("inf"), dtype=torch.float32, device=index.device)
    offsets, scores, rows, base = [torch.zeros(1, dtype=torch.int64, device=index.device)], [], [], 0
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        q16 = vec[lo:hi]                                                       # the stored bits themselves, not re-prepared
        sub = (q16.float() ** 2).sum(dim=1).contiguous() if l2 else None
        thr = torch.where(bias[lo:hi] > float("-inf"), thr_all, inf).contiguous()
        row_hi = torch.arange(lo, hi, dtype=torch.int32, device=index.device)
        ops = Operands(index._vec, n, index._bias, q16, metric_alpha(index.metric), sub, l2, thr, row_hi, self_join_slices(n, hi - lo))
        o, s, r = ops.search(MAX_RESULTS, what)
        offsets.append(o[1:] + base)
        scores.append(s)
        rows.append(r)
        base += s.numel()
    return torch.cat(offsets), torch.cat(scores), torch.cat(rows)


def dedup(index, threshold):
    offsets, _, rows = near_duplicates(index, threshold)
    return greedy_leaders(offsets, rows, index.bias > float("-inf")).to(index.device)
