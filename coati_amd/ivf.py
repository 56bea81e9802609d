"""Approximate nearest-neighbour search over an embedding library: an inverted file (IVF) on top of an EmbeddingIndex
(include/coati_ivf.h, csrc/ivf.hip).

    ivf = index.ivf(1024)                                # k-means centres as the coarse quantiser; "cosine" or "l2"
    scores, rows = ivf.search(queries, k=10, nprobe=8)   # EmbeddingIndex.search's contract over the rows of the 8 nearest lists

Building runs index.kmeans (or index.assign on given centres), stable-sorts the live rows by list and gathers vectors and bias into list
order; every list is then a contiguous run of rows whose original indices ascend.  A search is three steps: the coarse step is
coati_search_topk on the centres (no new kernel); torch inverts the probe table [Q, nprobe] on the device into (list, query) pairs; then
coati_ivf_scan scores the rows of every pair's list on the matrix cores -- no score matrix exists -- and coati_ivf_merge merges a query's
partial lists.  The scores are the exact kernel's bits, the rows returned are original rows, and with nprobe >= the number of non-empty
lists the result IS EmbeddingIndex.search's.  Nothing depends on the launch geometry; building is reproducible bit for bit from the seed.
"dot" has no nearest centre and raises.  There is no CPU fallback.  Lists of e4m3 bytes with an exact bf16 re-scoring are
coati_amd.ivf8.Ivf8Index (index.ivf(nlist, fp8=True), ivf.fp8(index)): the same lists, probe tables and merge, built on the helpers
below (make_lists, ListIndex).  Radius search over the lists -- IVFIndex.radius_search / radius_count / near_duplicates / dedup -- is
coati_amd.ivf_radius (include/coati_ivf_radius.h).  Lists of PQ codes of the rows' residuals are
coati_amd.ivfpq.IvfPqIndex (index.ivfpq(nlist), ivf.pq(index)), on the same helpers.  Out of scope: add() after build (rebuild instead),
more than 4096 lists, fp8 centres, several GPUs.  The reference has no counterpart."""
import torch

from . import _lib, cluster
from .ops import ptr, stream
from .search import K_MAX, SCRATCH_BYTES, check_bias, check_rows, finish_scores, metric_alpha, prepare_queries, scratch_pair

NLIST_MAX = 4096
NPROBE_MAX = 128
MERGE_MAX = 16384                # nprobe * segs * k: one query's partial lists are one row of the merge's select
PAIR_GROUP = 16                  # the pairs of one work item


def invert_probes(probes, sizes, seg_rows, cache=None):
    """The scan's operands from a probe table: probes [Q, nprobe] int32 on the device (list, or -1), sizes [L] int64 (rows per list) ->
    (pair_q [Q * nprobe] int32, pair_off [L + 1] int32, item_off [L + 1] int32, pair_slot [Q, nprobe] int32).  The pairs are the entries
    that are not -1, sorted by (list, query) with a stable sort; the -1 entries sort behind them and belong to no list.  Device work
    only: nothing here waits for the GPU.  cache: a dict that keeps the tensors that depend on the shapes alone between calls (the list
    numbers, the slot numbers, the segments per list)."""
    Q, nprobe = probes.shape
    L, dev, P = sizes.shape[0], probes.device, probes.shape[0] * probes.shape[1]
    cache = {} if cache is None else cache
    if len(cache) > 64:                                                          # (a caller that varies Q or seg_rows without end)
        cache.clear()
    if ("lists", L) not in cache:
        cache["lists", L] = torch.arange(L + 1, dtype=torch.int16 if L < 2 ** 15 else torch.int32, device=dev)
    if ("slots", P) not in cache:
        cache["slots", P] = torch.arange(P, dtype=torch.int32, device=dev)
    if ("segments", seg_rows) not in cache:
        cache["segments", seg_rows] = (sizes + seg_rows - 1) // seg_rows
    lists, slots, segments = cache["lists", L], cache["slots", P], cache["segments", seg_rows]
    flat = probes.reshape(-1).clamp(-1, L)
    none = flat < 0
    key = torch.where(none, L, flat).to(lists.dtype)                             # L <= 4096: 16-bit keys, fewer radix passes
    key, order = torch.sort(key, stable=True)
    pair_q = torch.div(order, nprobe, rounding_mode="floor").to(torch.int32)
    pair_off = torch.searchsorted(key, lists)                                    # the first pair of every list, and of "no list"
    counts = pair_off[1:] - pair_off[:-1]
    item_off = torch.zeros(L + 1, dtype=torch.int32, device=dev)
    torch.cumsum(((counts + PAIR_GROUP - 1) // PAIR_GROUP) * segments, 0, dtype=torch.int32, out=item_off[1:])
    pair_slot = torch.empty(P, dtype=torch.int32, device=dev)
    pair_slot[order] = slots
    pair_slot.masked_fill_(none, -1)
    return pair_q, pair_off.to(torch.int32), item_off, pair_slot.reshape(Q, nprobe)


def make_lists(what, index, nlist, iters=20, seed=0, centres=None, assign=None):
    """The inverted lists of an EmbeddingIndex ("cosine" or "l2") on a GPU: (centres [nlist, dim], order int64 [M], sizes int64 [nlist]).
    The lists are index.kmeans(nlist, iters, seed)'s clusters, or, with centres, every live row's nearest of them (index.assign), or
    assign [N] int32 given by hand (-1 leaving a row out).  order lists the rows list by list, ascending inside every list; removed
    rows of the index are left out.  Reproducible bit for bit from the seed."""
    cluster._check_metric(index.metric)
    nlist = int(nlist)
    if not 1 <= nlist <= NLIST_MAX:
        raise ValueError(f"{what}: nlist={nlist} outside 1 .. {NLIST_MAX}")
    if index.device.type != "cuda":
        raise RuntimeError(f"{what}: the index is not on a GPU; there is no CPU fallback")
    if centres is None:
        if assign is not None:
            raise ValueError(f"{what}: assign= needs centres=")
        clustering = index.kmeans(nlist, iters=iters, seed=seed)
        centres, assign = clustering.centres, clustering.assign
    else:
        centres = torch.as_tensor(centres)
        if tuple(centres.shape) != (nlist, index.dim):
            raise ValueError(f"{what}: centres must be [{nlist}, {index.dim}], got {tuple(centres.shape)}")
        if assign is None:
            assign, _ = index.assign(centres)
        else:
            assign = torch.as_tensor(assign).to(index.device, torch.int32)
            if tuple(assign.shape) != (len(index),) or int(assign.max()) >= nlist:
                raise ValueError(f"{what}: assign must be [{len(index)}] with entries below {nlist}")
            assign = torch.where(index.bias > float("-inf"), assign, torch.full_like(assign, -1))
    order, sizes = cluster.sorted_order(assign, nlist)
    return centres, order[:int(sizes.sum())], sizes


class ListIndex:
    """What IVFIndex, coati_amd.ivf8.Ivf8Index and coati_amd.ivfpq.IvfPqIndex share: the lists (centres, ids, sizes, offsets), the coarse step, the checks of a
    search's arguments and the scan + merge loop over chunks of queries.  A subclass stores the rows and supplies the scan call."""

    def _init_lists(self, dim, dim_padded, metric, n, centres, ids, sizes, device):
        cluster._check_metric(metric)
        self._name = type(self).__name__
        self.dim, self.dim_padded, self.metric, self.device = int(dim), int(dim_padded), metric, torch.device(device)
        self._n = int(n)
        self.centres = centres.to(self.device, torch.float32)
        self._ids = ids.to(self.device, torch.int32).contiguous()
        self._sizes = sizes.to(self.device, torch.int64)
        self.nlist = int(self._sizes.shape[0])
        if not 1 <= self.nlist <= NLIST_MAX or self.centres.shape[0] != self.nlist:
            raise ValueError(f"{self._name}: {self.nlist} lists for {self.centres.shape[0]} centres, outside 1 .. {NLIST_MAX}")
        host = self._sizes.cpu()
        self._m, self._max_rows = int(host.sum()), int(host.max())
        if self._ids.shape != (self._m,):
            raise ValueError(f"{self._name}: vectors, ids and bias do not match the list sizes")
        self._list_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), self._sizes.cumsum(0)]).to(torch.int32)
        self._inverse = torch.full((self._n,), -1, dtype=torch.int64, device=self.device)
        self._inverse[self._ids.long()] = torch.arange(self._m, device=self.device)
        # the coarse step's library: the centres as queries are prepared, the metric's per-centre bias, -inf for an empty list
        _, self._c16, cbias = cluster.prepare_centres(self.centres, metric, self.dim_padded, self.device)
        cb = 2.0 * cbias if cbias is not None else torch.zeros(self.nlist, dtype=torch.float32, device=self.device)
        self._cbias = torch.where(self._sizes > 0, cb, torch.full_like(cb, float("-inf"))).contiguous()
        self._scratch = None         # the scan's partial lists, kept between searches
        self._tables = {}            # invert_probes' shape-only tensors
        self._coarse = None          # the coarse step's

    def __len__(self):
        return self._n

    @property
    def sizes(self):
        """[L] int64: the rows of every list (removed rows stay counted)"""
        return self._sizes

    @property
    def ids(self):
        """[M] int32: the original row of every stored position, ascending inside every list"""
        return self._ids

    @property
    def list_offsets(self):
        """[L + 1] int32: list l owns positions list_offsets[l] .. list_offsets[l + 1] - 1"""
        return self._list_off

    def list_rows(self, l):
        """the original rows of list l, ascending"""
        if not 0 <= int(l) < self.nlist:
            raise IndexError(f"{self._name}.list_rows: list {l} outside 0 .. {self.nlist - 1}")
        lo, hi = int(self._list_off[int(l)]), int(self._list_off[int(l) + 1])
        return self._ids[lo:hi].long()

    def _positions(self, rows):
        """the stored positions of original rows (those that have one), for remove()"""
        rows = check_rows(f"{self._name}.remove", rows, self._n).to(self.device)
        pos = self._inverse[rows]
        return rows, pos[pos >= 0]

    # ---- searching -----------------------------------------------------------------------------------------------------------------
    def _check_nprobe(self, nprobe):
        nprobe = int(nprobe)
        if not 1 <= nprobe <= NPROBE_MAX:
            raise ValueError(f"{self._name}: nprobe={nprobe} outside 1 .. {NPROBE_MAX}")
        return nprobe

    def _probe16(self, q16, nprobe):
        """the coarse step on prepared queries: [Q, nprobe] int64, the nearest non-empty lists, nearest first, -1 padded"""
        Q = q16.shape[0]
        if Q == 0:
            return torch.full((Q, nprobe), -1, dtype=torch.int64, device=self.device)
        lists = torch.empty(Q, nprobe, dtype=torch.int64, device=self.device)      # (the kernel writes every entry, -1 padding included)
        if self.device.type != "cuda":
            raise RuntimeError(f"{self._name}.probe: the index is not on a GPU; there is no CPU fallback")
        lib = _lib.lib()
        S = lib.coati_search_slices(self.nlist, Q, nprobe)
        if S < 1:
            raise RuntimeError(f"coati_search_slices({self.nlist}, {Q}, {nprobe}) = {S}: {lib.coati_last_error().decode('utf-8', 'replace')}")
        self._coarse = scratch_pair(self._coarse, Q * S * nprobe, self.device)
        scores = torch.empty(Q, nprobe, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.call("coati_search_topk", ptr(self._c16), self.nlist, self.dim_padded, ptr(self._cbias), ptr(q16), Q, nprobe,
                      metric_alpha(self.metric), S, ptr(self._coarse[0]), ptr(self._coarse[1]), ptr(scores), ptr(lists), stream())
        return lists

    def probe(self, queries, nprobe):
        """[Q, nprobe] int64: every query's nprobe nearest non-empty lists under the metric, nearest first, the lower list among equally
        near ones; -1 where fewer lists have rows"""
        nprobe = self._check_nprobe(nprobe)
        _, q16 = prepare_queries(queries, self.metric, self.dim, self.device)
        return self._probe16(q16, nprobe)

    def plan(self, Q, nprobe, k):
        """the default seg_rows (coati_ivf_plan)"""
        lib = _lib.lib()
        seg_rows = int(lib.coati_ivf_plan(max(self._max_rows, 1), int(Q), int(nprobe), int(k)))
        if seg_rows < 1:
            raise ValueError(f"{self._name}: coati_ivf_plan: {lib.coati_last_error().decode('utf-8', 'replace')}")
        return seg_rows

    def _given_probes(self, probes, nprobe, Q, what):
        """(the caller's probe table [Q, n] on the device, n), or (None, the checked nprobe) where the coarse step is to decide"""
        if probes is None:
            return None, self._check_nprobe(nprobe)
        table = torch.as_tensor(probes).to(self.device)
        if table.dim() != 2 or table.shape[0] != Q or table.dtype not in (torch.int32, torch.int64) or not 1 <= table.shape[1] <= NPROBE_MAX:
            raise ValueError(f"{self._name}.{what}: probes must be an integer table [{Q}, 1 .. {NPROBE_MAX}]")
        return table, table.shape[1]

    def _search_args(self, queries, kk, nprobe, probes, seg_rows):
        """The checks of a search that keeps kk entries per partial list: (q16, table [Q, nprobe] on the device, nprobe, seg_rows, segs)"""
        _, q16 = prepare_queries(queries, self.metric, self.dim, self.device)
        Q = q16.shape[0]
        table, nprobe = self._given_probes(probes, nprobe, Q, "search")
        if table is None:
            table = self._probe16(q16, nprobe)
        if nprobe * kk > MERGE_MAX:
            raise ValueError(f"{self._name}.search: nprobe={nprobe} times k={kk} exceeds {MERGE_MAX}")
        if seg_rows is None:
            seg_rows = self.plan(max(Q, 1), nprobe, kk)
        seg_rows = int(seg_rows)
        if seg_rows < 64 or seg_rows % 64:
            raise ValueError(f"{self._name}.search: seg_rows={seg_rows} is not a positive multiple of 64")
        segs = max(1, -(-self._max_rows // seg_rows))
        if nprobe * segs * kk > MERGE_MAX:
            raise ValueError(f"{self._name}.search: nprobe={nprobe} lists of {segs} segments of k={kk} exceed nprobe * segs * k <= {MERGE_MAX}; "
                             "pass a larger seg_rows, or none")
        return q16, table, nprobe, seg_rows, segs

    def _scan_merge(self, scan, Q, table, nprobe, kk, seg_rows, segs):
        """(scores [Q, kk] f32, rows [Q, kk] int64): per chunk of queries (the partial lists of a chunk stay within SCRATCH_BYTES) the
        probe table inverted, scan(lo, n, pair_q, pair_off, item_off, P, seg_rows, segs, part_score, part_row, stream) and coati_ivf_merge"""
        if Q == 0 or self._m == 0:
            return (torch.full((Q, kk), float("-inf"), dtype=torch.float32, device=self.device),
                    torch.full((Q, kk), -1, dtype=torch.int64, device=self.device))
        if self.device.type != "cuda":
            raise RuntimeError(f"{self._name}.search: the index is not on a GPU; there is no CPU fallback")
        scores = torch.empty(Q, kk, dtype=torch.float32, device=self.device)      # (the merge writes every entry, padding included)
        rows = torch.empty(Q, kk, dtype=torch.int64, device=self.device)
        table32 = table.to(torch.int32).contiguous()
        per_query = nprobe * segs * kk * 8
        qc = max(1, min(Q, SCRATCH_BYTES // per_query))
        self._scratch = scratch_pair(self._scratch, qc * nprobe * segs * kk, self.device)
        with torch.cuda.device(self.device):
            s = stream()
            for lo in range(0, Q, qc):
                n = min(qc, Q - lo)
                pair_q, pair_off, item_off, pair_slot = invert_probes(table32[lo:lo + n], self._sizes, seg_rows, self._tables)
                P = n * nprobe
                scan(lo, n, pair_q, pair_off, item_off, P, seg_rows, segs, self._scratch[0], self._scratch[1], s)
                _lib.call("coati_ivf_merge", ptr(self._scratch[0]), ptr(self._scratch[1]), ptr(table32[lo:lo + n]), ptr(pair_slot),
                          P, ptr(self._list_off), self.nlist, n, nprobe, kk, seg_rows, segs, ptr(scores[lo:lo + n]),
                          ptr(rows[lo:lo + n]), s)
        return scores, rows


class IVFIndex(ListIndex):
    """An inverted-file index over the live rows of an EmbeddingIndex at the time of build().  len() is the source's; rows returned by
    search are the source's rows.  Attributes: centres [L, dim] f32, nlist, metric, dim, dim_padded, device."""

    def __init__(self, dim, dim_padded, metric, n, centres, vectors, ids, bias, sizes, device):
        self._init_lists(dim, dim_padded, metric, n, centres, ids, sizes, device)
        self._vec, self._bias = vectors.to(self.device).contiguous(), bias.to(self.device, torch.float32).contiguous()
        if self._vec.shape != (self._m, self.dim_padded) or self._bias.shape != (self._m,):
            raise ValueError("IVFIndex: vectors, ids and bias do not match the list sizes")

    # ---- building ----------------------------------------------------------------------------------------------------------------
    @classmethod
    def build(cls, index, nlist, iters=20, seed=0, centres=None, assign=None):
        """index: an EmbeddingIndex ("cosine" or "l2") on a GPU.  The lists are index.kmeans(nlist, iters, seed)'s clusters, or, with
        centres [nlist, dim], every live row's nearest of them (index.assign).  assign [N] int32 (with centres): the lists given by hand,
        -1 leaving a row out.  Removed rows of the index are left out.  Reproducible bit for bit from the seed."""
        centres, order, sizes = make_lists("IVFIndex.build", index, nlist, iters, seed, centres, assign)
        return cls(index.dim, index.dim_padded, index.metric, len(index), centres, index.vectors[order], order, index.bias[order], sizes,
                   index.device)

    def fp8(self, index=None):
        """A coati_amd.ivf8.Ivf8Index of these lists: the stored rows as e4m3 bytes.  index: the source EmbeddingIndex, whose bf16 rows
        the second stage then re-scores the candidates from (a view); without it the result is stage 1's."""
        from .ivf8 import Ivf8Index
        return Ivf8Index.from_ivf(self, index)

    def pq(self, index=None, pq_seed=0, pq_iters=20, sample=65536, codebooks=None):
        """A coati_amd.ivfpq.IvfPqIndex of these lists: the stored rows as PQ codes of their residuals against the lists' centres, under
        code books fitted on a seeded sample of the residuals or given.  index: the source EmbeddingIndex, whose bf16 rows the second stage
        then re-scores the candidates from (a view); without it the result is stage 1's."""
        from .ivfpq import IvfPqIndex
        return IvfPqIndex.from_ivf(self, index, pq_seed=pq_seed, pq_iters=pq_iters, sample=sample, codebooks=codebooks)

    @property
    def vectors(self):
        """the stored bf16 rows [M, dim_padded] in list order"""
        return self._vec

    @property
    def bias(self):
        """[M] f32: the positions' bias (0, -|x|^2 for l2, -inf once removed)"""
        return self._bias

    def remove(self, rows):
        """the rows (original indices) are never returned again; len() and the other rows' indices do not change"""
        _, pos = self._positions(rows)
        self._bias[pos] = float("-inf")

    def search(self, queries, k, nprobe=8, probes=None, seg_rows=None, bias=None, return_probes=False, blocks=0):
        """(scores [Q, k] f32, rows [Q, k] int64) of the k nearest rows among every query's probed lists: EmbeddingIndex.search's contract
        -- the metric's score, descending, original row ascending among equal scores, (-inf, -1) where fewer rows qualify.
        nprobe: the lists probed per query (probe()).  probes: a table [Q, n] of lists instead (-1 = none; a list at most once per
        query).  seg_rows: the rows of a work item's segment, a multiple of 64 (default: coati_ivf_plan), blocks: the scan's workgroups
        (default 0: the kernel's); the result depends on neither.  bias: f32 [N] over ORIGINAL rows, added to every row's score, -inf
        excluding a row.  return_probes: also return the probe table used, int64."""
        k = int(k)
        if k < 1 or k > K_MAX:
            raise ValueError(f"IVFIndex.search: k={k} outside 1 .. {K_MAX}")
        check_bias("IVFIndex.search", bias, self._n)
        q16, table, nprobe, seg_rows, segs = self._search_args(queries, k, nprobe, probes, seg_rows)
        pos_bias = self._bias if bias is None else (self._bias + bias.to(self.device)[self._ids.long()]).contiguous()

        def scan(lo, n, pair_q, pair_off, item_off, P, seg_rows, segs, part_score, part_row, s):
            _lib.call("coati_ivf_scan", ptr(self._vec), ptr(self._ids), ptr(pos_bias), ptr(self._list_off), self._m, self.dim_padded,
                      self.nlist, ptr(q16[lo:lo + n]), n, ptr(pair_q), ptr(pair_off), ptr(item_off), P, k, metric_alpha(self.metric),
                      seg_rows, segs, ptr(part_score), ptr(part_row), int(blocks), s)

        scores, rows = self._scan_merge(scan, q16.shape[0], table, nprobe, k, seg_rows, segs)
        scores = finish_scores(scores, self.metric, q16)
        return (scores, rows, table.long()) if return_probes else (scores, rows)

    # ---- radius search (coati_amd.ivf_radius) -----------------------------------------------------------------------------------------
    def radius_search(self, queries, threshold, nprobe=8, probes=None, order="row", row_below=None, seg_rows=None, max_results=1 << 28,
                      blocks=0, return_probes=False):
        """(offsets int64 [Q + 1], scores f32 [T], rows int64 [T]): EmbeddingIndex.radius_search's contract restricted to the rows of every
        query's probed lists -- every such live row whose score reaches the threshold (a float or a [Q] tensor, in the units search()
        returns; +inf nothing, -inf every live probed row), original rows, the score bits EmbeddingIndex.search gives the pair.  With
        nprobe >= the number of non-empty lists the result IS EmbeddingIndex.radius_search's.
        nprobe / probes / seg_rows / blocks / return_probes: as in search(); the result depends on neither seg_rows nor blocks.
        order: "row" = ascending row, "score" = score descending and row ascending among equal scores, "probe" = as the kernel writes:
        list by list in the probe table's order, row ascending inside a list.  row_below: int [Q], only rows < row_below[i] are hits of
        query i.  The total is known after the count pass (one synchronisation per chunk of queries); above max_results a ValueError
        names it before the result is allocated."""
        from . import ivf_radius
        return ivf_radius.radius_search(self, queries, threshold, nprobe, probes, order, row_below, seg_rows, max_results, blocks, return_probes)

    def radius_count(self, queries, threshold, nprobe=8, probes=None, row_below=None):
        """int64 [Q]: how many live rows of each query's probed lists reach the threshold -- the count pass alone, nothing is allocated
        per hit"""
        from . import ivf_radius
        return ivf_radius.radius_count(self, queries, threshold, nprobe, probes, row_below)

    def near_duplicates(self, threshold, nprobe=8, chunk=4096):
        """(offsets int64 [len + 1], scores f32 [T], rows int64 [T]) in ORIGINAL row order: for every live stored row i the EARLIER live
        rows j < i within the threshold AMONG THE LISTS ROW i PROBES (its own list always, then its nearest by the coarse step), row
        ascending -- a subset of EmbeddingIndex.near_duplicates with the same score bits, and equal to it once nprobe >= the number of
        non-empty lists.  The queries are the stored bf16 rows themselves, taken `chunk` positions at a time in list order, so a chunk
        probes a few neighbouring lists.  Rows without a position (left out at build) and removed rows have empty segments."""
        from . import ivf_radius
        return ivf_radius.near_duplicates(self, threshold, nprobe, chunk)

    def dedup(self, threshold, nprobe=8):
        """bool [len] keep mask: the greedy leader rule in row order (coati_amd.radius.greedy_leaders) over near_duplicates(threshold,
        nprobe); removed rows and rows without a position are False.  What survives the approximation: every dropped row is within
        the threshold of a KEPT one.  What does not: "no two kept rows within the threshold" holds only for pairs in which the later
        row probed the earlier one's list.  Exact -- EmbeddingIndex.dedup's mask -- at nprobe >= the number of non-empty lists."""
        from . import ivf_radius
        return ivf_radius.dedup(self, threshold, nprobe)

    # ---- persistence ---------------------------------------------------------------------------------------------------------------
    def save(self, path):
        torch.save({"dim": self.dim, "dim_padded": self.dim_padded, "metric": self.metric, "n": self._n, "centres": self.centres.cpu(),
                    "vectors": self._vec.cpu(), "ids": self._ids.cpu(), "bias": self._bias.cpu(), "sizes": self._sizes.cpu()}, path)

    @classmethod
    def load(cls, path, device="cuda:0"):
        d = torch.load(path, map_location="cpu")
        return cls(d["dim"], d["dim_padded"], d["metric"], d["n"], d["centres"], d["vectors"], d["ids"], d["bias"], d["sizes"], device)
