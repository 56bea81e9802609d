"""Clustering of a library of embeddings held in device memory as bf16 rows (include/coati_cluster.h, csrc/cluster.hip).

    clustering = index.kmeans(64)                       # an EmbeddingIndex (coati_amd.search), "cosine" or "l2"
    clustering.assign, clustering.centres               # [N] int32 (-1 = removed row), [64, dim] f32
    rows = clustering.representatives(scores)           # [64] int64: every cluster's best-scored member

A Lloyd round is two kernels and a little torch between them: coati_cluster_assign streams the library once and writes every row's
nearest centre (no [N, K] score matrix exists), a stable torch sort turns the assignment into an inverted index, coati_cluster_sums adds
every cluster's rows in a fixed order (no atomics), and the mean is taken in f32.  Both kernels are bitwise reproducible and do not depend on
their launch geometry, so neither does a whole run from one seed.  "cosine" is spherical k-means (unit rows, the mean renormalised), "l2"
plain k-means (the centre's -|c|^2 / 2 goes in as the kernel's per-centre bias); "dot" has no nearest centre and raises.  There is no CPU
fallback: off a GPU these raise RuntimeError, like EmbeddingIndex.search.  The reference has no counterpart."""
import torch

from . import _lib
from .ops import ptr, stream

K_MAX = 4096
CLUSTER_METRICS = ("cosine", "l2")




def _check_metric(metric):
    if metric not in CLUSTER_METRICS:
        raise ValueError(f"cluster: metric {metric!r} is not one of {CLUSTER_METRICS} (a dot product has no nearest centre)")


def _check_rows(x16, row_bias, what):
    if not isinstance(x16, torch.Tensor) or x16.dtype != torch.bfloat16 or x16.dim() != 2 or x16.shape[1] % 32 or not 32 <= x16.shape[1] <= 512:
        raise ValueError(f"{what}: rows must be prepared bf16 [N, E], E a multiple of 32 in 32 .. 512")
    if row_bias is not None and (row_bias.dtype != torch.float32 or tuple(row_bias.shape) != (x16.shape[0],) or row_bias.device != x16.device):
        raise ValueError(f"{what}: row_bias must be f32 [{x16.shape[0]}] on the rows' device")
    if x16.device.type != "cuda":
        raise RuntimeError(f"{what}: the rows are not on a GPU; there is no CPU fallback")


def chunk_rows():
    """CH of coati_cluster_sums: the rows of one work item"""
    return int(_lib.lib().coati_cluster_chunk())


def prepare_centres(centres, metric, width, device=None):
    """centres as the kernel takes them: (f32 [K, width] after the metric's preparation, its bf16 rounding, cbias [K] f32 or None).
    Narrower centres are padded with zero columns, as the rows are."""
    _check_metric(metric)
    c = torch.as_tensor(centres)
    if c.dim() != 2 or c.shape[1] > width or not 1 <= c.shape[0] <= K_MAX:
        raise ValueError(f"cluster: centres must be [1 .. {K_MAX}, <= {width}], got {tuple(c.shape)}")
    c = c.detach().to(device=device, dtype=torch.float32)
    if c.shape[1] < width:
        c = torch.nn.functional.pad(c, (0, width - c.shape[1]))
    if metric == "cosine":
        c = c / c.norm(dim=1, keepdim=True).clamp_min(1e-30)
    c16 = c.to(torch.bfloat16).contiguous()
    cbias = (-0.5 * (c16.double() ** 2).sum(dim=1)).float() if metric == "l2" else None   # one rounding, as the rows' -|x|^2
    return c, c16, cbias


def assign_call(x16, row_bias, c16, cbias=None, blocks=0):
    """coati_cluster_assign on prepared operands: (assign int32 [N], best f32 [N]), best = dot + cbias"""
    N, E = x16.shape
    assign = torch.empty(N, dtype=torch.int32, device=x16.device)
    best = torch.empty(N, dtype=torch.float32, device=x16.device)
    if N:
        with torch.cuda.device(x16.device):
            _lib.call("coati_cluster_assign", ptr(x16), N, E, ptr(row_bias), ptr(c16), c16.shape[0], ptr(cbias), ptr(assign), ptr(best),
                      int(blocks), stream())
    return assign, best


def sorted_order(assign, k):
    """the inverted index of an assignment: (order int64 [M]: the rows with assign >= 0 sorted by (cluster, row), sizes int64 [k])"""
    key = torch.where(assign < 0, torch.full_like(assign, k), assign)
    sizes = torch.bincount(key, minlength=k + 1)[:k]
    order = torch.sort(key.to(torch.int16) if k < 2 ** 15 else key, stable=True).indices      # k <= 4096: 16-bit keys, fewer radix passes
    return order, sizes


def item_table(sizes, ch):
    """(offsets int32 [k + 1], item_off int32 [k + 1]) of coati_cluster_sums from the cluster sizes"""
    zero = torch.zeros(1, dtype=torch.int64, device=sizes.device)
    offsets = torch.cat([zero, sizes.cumsum(0)]).to(torch.int32)
    item_off = torch.cat([zero, ((sizes + ch - 1) // ch).cumsum(0)]).to(torch.int32)
    return offsets, item_off


def sums_call(x16, order32, offsets, item_off, part=None, blocks=0):
    """coati_cluster_sums: sums f32 [K, E] of the rows listed in order32 [M] int32 (cluster by cluster: offsets, item_off [K + 1] int32)"""
    N, E = x16.shape
    M, K = order32.shape[0], offsets.shape[0] - 1
    sums = torch.zeros(K, E, dtype=torch.float32, device=x16.device)
    if M:
        lib = _lib.lib()
        items_max = int(lib.coati_cluster_items_max(M, K))
        if items_max < 0:
            raise RuntimeError(f"coati_cluster_items_max({M}, {K}): {lib.coati_last_error().decode('utf-8', 'replace')}")
        if part is None or part.numel() < items_max * E:
            part = torch.empty(items_max * E, dtype=torch.float32, device=x16.device)
        with torch.cuda.device(x16.device):
            _lib.call("coati_cluster_sums", ptr(x16), N, E, ptr(order32), M, ptr(offsets), ptr(item_off), K, ptr(part), items_max,
                      ptr(sums), int(blocks), stream())
    return sums


def finish_assign_scores(best, metric, row_bias, x16):
    """the kernel's dot + cbias as the metric's score: the cosine, or for l2 2 (x.c - |c|^2 / 2) - |x|^2 = -|x - c|^2 (at most 0), the
    rows' -|x|^2 taken from row_bias (an index's stored bias) when given; -inf (excluded) stays"""
    if metric != "l2":
        return best
    xn = row_bias if row_bias is not None else -(x16.double() ** 2).sum(dim=1).float()
    return (2.0 * best + xn).clamp_max(0.0)


def assign_rows(x16, row_bias, centres, metric, blocks=0):
    """(assign int32 [N], score f32 [N]) of prepared rows x16 [N, E] bf16: the nearest of centres [K, <= E] (prepared as queries are:
    normalised for cosine, rounded to bf16), the lowest index among equally near ones, and the metric's score to it (the cosine; the
    negated squared distance for l2).  row_bias [N] f32 or None: -inf excludes a row (assign -1, score -inf); for l2 it carries the rows'
    -|x|^2, as an EmbeddingIndex stores it."""
    _check_metric(metric)
    _check_rows(x16, row_bias, "assign_rows")
    _, c16, cbias = prepare_centres(centres, metric, x16.shape[1], x16.device)
    assign, best = assign_call(x16, row_bias, c16, cbias, blocks)
    return assign, finish_assign_scores(best, metric, row_bias, x16)


class Clustering:
    """centres [k, dim] f32; assign [N] int32 (-1: a removed row); score [N] f32, every row's metric score to its centre (-inf: removed);
    sizes [k] int64; inertia: per assignment pass, the sum over the rows of the squared distance (l2) or of 1 - cosine; iterations: the
    centre updates made; converged: whether the last pass changed no assignment.  rows: None, or the library rows [N] int64 that were
    clustered (kmeans(rows=...)): assign and score are in their order, members() and representatives() answer in library rows."""

    def __init__(self, centres, assign, score=None, inertia=(), iterations=0, converged=False, rows=None, metric=None):
        self.centres, self.assign, self.score = centres, assign, score
        self.inertia, self.iterations, self.converged, self.rows, self.metric = list(inertia), int(iterations), bool(converged), rows, metric
        self.k = centres.shape[0]
        self._order, self.sizes = sorted_order(assign, self.k)
        self._order = self._order[:int(self.sizes.sum())]
        self._offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.sizes.device), self.sizes.cumsum(0)])

    def _library(self, positions):
        return positions if self.rows is None else torch.where(positions >= 0, self.rows[positions.clamp_min(0)], positions)

    def members(self, c):
        """the rows of cluster c, ascending"""
        if not 0 <= int(c) < self.k:
            raise IndexError(f"Clustering.members: cluster {c} outside 0 .. {self.k - 1}")
        lo, hi = int(self._offsets[int(c)]), int(self._offsets[int(c) + 1])
        return self._library(self._order[lo:hi])

    def representatives(self, scores=None):
        """[k] int64: every cluster's member with the largest scores[i] (scores [N], aligned with assign), the lowest row among equal
        scores; without scores the member nearest its centre; -1 for an empty cluster.  A segmented argmax over the sorted order."""
        values = self.score if scores is None else torch.as_tensor(scores).to(self.assign.device)
        if values is None or tuple(values.shape) != tuple(self.assign.shape):
            raise ValueError(f"Clustering.representatives: scores must be [{self.assign.shape[0]}]")
        order, M = self._order, self._order.shape[0]
        seg, vals = self.assign[order].long(), values[order]
        top = torch.full((self.k,), float("-inf"), dtype=vals.dtype, device=vals.device).scatter_reduce(0, seg, vals, "amax", include_self=True)
        pos = torch.where(vals == top[seg], torch.arange(M, device=vals.device), torch.full((M,), M, device=vals.device))
        first = torch.full((self.k,), M, dtype=torch.int64, device=vals.device).scatter_reduce(0, seg, pos, "amin", include_self=True)
        none = torch.full((self.k,), -1, dtype=torch.int64, device=vals.device)
        return self._library(torch.where(first < M, order[first.clamp_max(max(M - 1, 0))], none) if M else none)


def kmeans_rows(x16, row_bias, metric, k, iters=20, seed=0, init=None, dim=None):
    """Lloyd's k-means on prepared rows x16 [N, E] bf16 (row_bias as in assign_rows) -> Clustering.  init: None = k distinct included rows
    drawn by a CPU torch.randperm seeded with `seed`, or a [k, <= E] tensor.  A round: assign; a stable sort and the counts; the sums; the
    mean in f32 (renormalised for cosine), an empty cluster keeping its centre.  The loop ends with the first pass that changes no
    assignment, or after `iters` centre updates (one more pass then assigns the rows to the last centres).  dim: the columns of the
    centres returned (default: all E)."""
    _check_metric(metric)
    _check_rows(x16, row_bias, "kmeans_rows")
    k, iters = int(k), int(iters)
    if not 1 <= k <= K_MAX:
        raise ValueError(f"kmeans_rows: k={k} outside 1 .. {K_MAX}")
    if iters < 0:
        raise ValueError(f"kmeans_rows: iters={iters} < 0")
    N, E = x16.shape
    live = torch.arange(N, device=x16.device) if row_bias is None else torch.nonzero(row_bias > float("-inf")).reshape(-1)
    M = live.shape[0]
    if init is None:
        if k > M:
            raise ValueError(f"kmeans_rows: k={k} centres from {M} rows")
        pick = torch.randperm(M, generator=torch.Generator().manual_seed(int(seed)))[:k]
        centres = x16[live[pick.to(x16.device)]].float()
    else:
        centres = torch.as_tensor(init)
        if centres.dim() != 2 or centres.shape[0] != k:
            raise ValueError(f"kmeans_rows: init must be [{k}, dim], got {tuple(centres.shape)}")
    centres, c16, cbias = prepare_centres(centres, metric, E, x16.device)
    ch = chunk_rows()
    part = torch.empty((M // ch + k) * E, dtype=torch.float32, device=x16.device)
    inertia, prev, iterations, converged = [], None, 0, False

    def one_pass():
        assign, best = assign_call(x16, row_bias, c16, cbias)
        score = finish_assign_scores(best, metric, row_bias, x16)
        kept = score[live].double()
        inertia.append((-kept).sum() if metric == "l2" else (1.0 - kept).sum())
        return assign, score

    while True:
        assign, score = one_pass()
        converged = prev is not None and torch.equal(assign, prev)
        if converged or iterations == iters:
            break
        order, sizes = sorted_order(assign, k)
        offsets, item_off = item_table(sizes, ch)
        sums = sums_call(x16, order[:M].to(torch.int32), offsets, item_off, part)
        mean = sums / sizes.clamp_min(1).to(torch.float32)[:, None]
        if metric == "cosine":
            mean = mean / mean.norm(dim=1, keepdim=True).clamp_min(1e-30)
        centres = torch.where((sizes > 0)[:, None], mean, centres)
        c16 = centres.to(torch.bfloat16).contiguous()
        cbias = (-0.5 * (c16.double() ** 2).sum(dim=1)).float() if metric == "l2" else None
        prev, iterations = assign, iterations + 1
    out = centres if dim is None else centres[:, :dim].contiguous()
    return Clustering(out, assign, score, [float(v) for v in torch.stack(inertia).cpu()], iterations, converged, metric=metric)
