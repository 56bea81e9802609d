"""Nearest-neighbour search over a library of embeddings held in device memory as bf16 rows (include/coati_search.h, csrc/search.hip).

    index = EmbeddingIndex(256, metric="cosine")
    index.add(library_vectors)                       # [N, 256] float, any device
    scores, rows = index.search(queries, k=10)       # [Q, 10] f32 / int64: score descending, row ascending among equal scores

One streaming kernel computes alpha * dot(q, row) + bias[row] on the matrix cores and keeps every query's k best in LDS -- no [Q, N]
score matrix exists -- and a second one merges the library slices' lists.  The three metrics are host-side preparation (torch) on
top of that one kernel: "dot" (alpha 1, no bias), "cosine" (rows and queries normalised in f32, then rounded to bf16) and "l2" (alpha 2,
bias = -|x|^2 of the STORED bf16 values; the score returned is the negated squared distance).  Removing a row sets its bias to -inf.
There is no CPU fallback: search() on an index that is not on a GPU raises.  The reference has no counterpart."""
import torch

from . import _lib
from .ops import ptr, stream

METRICS = ("dot", "cosine", "l2")
DIM_MAX = 512
K_MAX = 128                      # TOPK_MAX of the radix select (csrc/decode_dev.h)
MERGE_MAX = 30720                # S * k: one query's partial lists are one row of the merge's select
SCRATCH_BYTES = 64 << 20         # the [Q, S, k] partial lists of one chunk of queries (f32 score + int32 row)
MIN_CAPACITY = 1024


def padded_dim(dim):
    """the stored width of a `dim`-wide embedding: the next multiple of 32 (the zero columns change no metric)"""
    if dim < 1 or dim > DIM_MAX:
        raise ValueError(f"EmbeddingIndex: dim={dim} outside 1 .. {DIM_MAX}")
    return (dim + 31) // 32 * 32


def _check_metric(metric):
    if metric not in METRICS:
        raise ValueError(f"EmbeddingIndex: metric {metric!r} is not one of {METRICS}")


def metric_alpha(metric):
    _check_metric(metric)
    return 2.0 if metric == "l2" else 1.0


def _as_f32(x, dim, device, what):
    x = torch.as_tensor(x)
    if x.dim() == 1:
        x = x[None]
    if x.dim() != 2 or x.shape[1] != dim:
        raise ValueError(f"EmbeddingIndex: {what} must be [n, {dim}], got {tuple(x.shape)}")
    x = x.detach().to(device=device, dtype=torch.float32)
    ep = padded_dim(dim)
    return x if ep == dim else torch.nn.functional.pad(x, (0, ep - dim))


def _normalised(x):
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-30)


def prepare_rows(x, metric, dim, device=None):
    """library rows as stored: (f32 [n, dim_padded] after the metric's preparation, its bf16 rounding, bias [n] f32)"""
    _check_metric(metric)
    x = _as_f32(x, dim, device, "vectors")
    if metric == "cosine":
        x = _normalised(x)
    x16 = x.to(torch.bfloat16)
    if metric == "l2":
        bias = -(x16.double() ** 2).sum(dim=1).float()      # one rounding: the squares' sum in float64, stored as f32
    else:
        bias = torch.zeros(x.shape[0], dtype=torch.float32, device=x.device)
    return x, x16, bias


def prepare_queries(q, metric, dim, device=None):
    """queries as searched: (f32 [Q, dim_padded] after the metric's preparation, its bf16 rounding)"""
    _check_metric(metric)
    q = _as_f32(q, dim, device, "queries")
    if metric == "cosine":
        q = _normalised(q)
    return q, q.to(torch.bfloat16).contiguous()


def finish_scores(scores, metric, q16):
    """the kernel's alpha * dot + bias as the metric's score: l2 = 2 q.x - |x|^2 - |q|^2 = -|q - x|^2 (at most 0); -inf padding stays"""
    if metric != "l2":
        return scores
    return (scores - (q16.float() ** 2).sum(dim=1, keepdim=True)).clamp_max(0.0)


def scratch_pair(pair, need, device):
    """`pair` if it is an (f32, int32) pair of at least `need` elements each, else a new one: a kernel's partial lists, kept between calls"""
    if pair is None or pair[0].numel() < need:
        pair = (torch.empty(need, dtype=torch.float32, device=device), torch.empty(need, dtype=torch.int32, device=device))
    return pair


def check_rows(what, rows, n):
    """`rows` as a flat int64 tensor; an IndexError naming `what` unless every one is a row of 0 .. n - 1"""
    rows = torch.as_tensor(rows, dtype=torch.int64).reshape(-1)
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n):
        raise IndexError(f"{what}: rows outside 0 .. {n - 1}")
    return rows


def check_bias(what, bias, n):
    """a search's extra bias: None, or an f32 tensor [n]"""
    if bias is not None and (not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or tuple(bias.shape) != (n,)):
        raise ValueError(f"{what}: bias must be an f32 tensor [{n}]")


def plan_chunks(entry, default_slices, Q, kk, slices):
    """(queries per call, slices): the [Q, S, kk] partial lists of a call stay within SCRATCH_BYTES.  S is `slices`, or else
    default_slices(qc, kk), the C entry `entry`'s answer for a call of qc queries."""
    qc = Q
    while True:
        S = int(slices) if slices is not None else default_slices(qc, kk)
        if S < 1:
            raise RuntimeError(f"{entry} at Q={qc}, k={kk} = {S}: {_lib.lib().coati_last_error().decode('utf-8', 'replace')}")
        if qc * S * kk * 8 <= SCRATCH_BYTES or qc == 1:
            return qc, S
        qc = max(1, min(qc // 2, SCRATCH_BYTES // (S * kk * 8)))


def sliced_topk(index, what, Q, kk, slices, call):
    """The flat indices' stage over all N rows: (scores [Q, kk] f32, rows [Q, kk] int64) of Q prepared queries, written chunk by chunk
    (index._plan) by call(lo, n, S, part_score, part_row, scores, rows, stream) -- one C entry on queries lo .. lo + n - 1 and their
    slices of the outputs.  No queries or no rows: the padding (-inf, -1).  index keeps the partial lists between calls (_scratch)."""
    if Q == 0 or len(index) == 0:
        return (torch.full((Q, kk), float("-inf"), dtype=torch.float32, device=index.device),
                torch.full((Q, kk), -1, dtype=torch.int64, device=index.device))
    if index.device.type != "cuda":
        raise RuntimeError(f"{what}: the index is not on a GPU; there is no CPU fallback")
    scores = torch.empty(Q, kk, dtype=torch.float32, device=index.device)          # (the merge writes every entry, padding included)
    rows = torch.empty(Q, kk, dtype=torch.int64, device=index.device)
    qc, S = index._plan(Q, kk, slices)
    index._scratch = scratch_pair(index._scratch, qc * S * kk, index.device)
    with torch.cuda.device(index.device):
        s = stream()
        for lo in range(0, Q, qc):
            n = min(qc, Q - lo)
            call(lo, n, S, index._scratch[0], index._scratch[1], scores[lo:lo + n], rows[lo:lo + n], s)
    return scores, rows


class EmbeddingIndex:
    def __init__(self, dim, metric="cosine", device="cuda:0", keep_f32=False):
        _check_metric(metric)
        self.dim, self.dim_padded = int(dim), padded_dim(int(dim))
        self.metric, self.device, self.keep_f32 = metric, torch.device(device), bool(keep_f32)
        self._n = 0
        self._vec = self._bias = self._f32 = None      # [capacity, dim_padded] bf16, [capacity] f32, [capacity, dim_padded] f32 (keep_f32)
        self._scratch = None                           # the partial lists, kept between searches

    def __len__(self):
        return self._n

    @property
    def vectors(self):
        """the stored bf16 rows [N, dim_padded] (a view)"""
        return self._empty(torch.bfloat16) if self._vec is None else self._vec[:self._n]

    @property
    def bias(self):
        """the rows' f32 bias [N] (a view): 0, -|x|^2 for l2, -inf once removed"""
        return torch.empty(0, dtype=torch.float32, device=self.device) if self._bias is None else self._bias[:self._n]

    def _empty(self, dtype):
        return torch.empty(0, self.dim_padded, dtype=dtype, device=self.device)

    def _reserve(self, n):
        cap = 0 if self._vec is None else self._vec.shape[0]
        if n <= cap:
            return
        new = max(MIN_CAPACITY, cap)
        while new < n:
            new *= 2

        def grown(old, shape, dtype):
            t = torch.empty(shape, dtype=dtype, device=self.device)
            if old is not None:
                t[:self._n] = old[:self._n]
            return t

        self._vec = grown(self._vec, (new, self.dim_padded), torch.bfloat16)
        self._bias = grown(self._bias, (new,), torch.float32)
        if self.keep_f32:
            self._f32 = grown(self._f32, (new, self.dim_padded), torch.float32)

    def add(self, vectors):
        """appends the rows of vectors [n, dim] (any float dtype, any device); returns their row indices"""
        x, x16, bias = prepare_rows(vectors, self.metric, self.dim, self.device)
        if self._n + x.shape[0] >= 2 ** 31:
            raise ValueError("EmbeddingIndex: more than 2^31 - 1 rows")
        lo, hi = self._n, self._n + x.shape[0]
        self._reserve(hi)
        self._vec[lo:hi], self._bias[lo:hi] = x16, bias
        if self.keep_f32:
            self._f32[lo:hi] = x
        self._n = hi
        return range(lo, hi)

    def remove(self, rows):
        """the rows are never returned again; len() and the other rows' indices do not change"""
        rows = check_rows("EmbeddingIndex.remove", rows, self._n)
        if rows.numel():
            self._bias[rows.to(self.device)] = float("-inf")

    def _plan(self, Q, k, slices):
        """(queries per call, slices) of a search: plan_chunks with coati_search_slices' default"""
        return plan_chunks("coati_search_slices", lambda qc, k: _lib.lib().coati_search_slices(self._n, qc, k), Q, k, slices)

    def search(self, queries, k, rescore=1, slices=None, bias=None):
        """(scores [Q, k] f32, rows [Q, k] int64) of the k nearest rows per query, score descending, row ascending among equal scores;
        fewer than k rows left: the tail is (-inf, -1).  rescore = m > 1 (needs keep_f32): the best min(m * k, 128) rows of the bf16
        search are scored again from the f32 copies and the best k of those returned.  slices: the library slices of the kernel's
        grid (default: coati_search_slices); the result does not depend on it.  bias: f32 [N], added to every row's score under the
        metric (for l2: to the negated squared distance), e.g. a multiple of property_scores(head)[:, 0] for "near q and high property";
        -inf entries exclude rows.  Not with rescore > 1."""
        k, rescore = int(k), int(rescore)
        if k < 1 or k > K_MAX:
            raise ValueError(f"EmbeddingIndex.search: k={k} outside 1 .. {K_MAX}")
        if rescore < 1:
            raise ValueError(f"EmbeddingIndex.search: rescore={rescore} < 1")
        if rescore > 1 and not self.keep_f32:
            raise ValueError("EmbeddingIndex.search: rescore > 1 needs the f32 copies (keep_f32=True)")
        kk = min(rescore * k, K_MAX) if rescore > 1 else k
        if slices is not None and (int(slices) < 1 or int(slices) * kk > MERGE_MAX):
            raise ValueError(f"EmbeddingIndex.search: slices={slices} outside 1 .. {MERGE_MAX // kk} at k={kk}")
        if bias is not None:
            if rescore > 1:
                raise ValueError("EmbeddingIndex.search: bias is not compatible with rescore > 1")
            check_bias("EmbeddingIndex.search", bias, self._n)
        q32, q16 = prepare_queries(queries, self.metric, self.dim, self.device)
        scores, rows = self._topk(q16, kk, slices, self._bias if bias is None else self.bias + bias.to(self.device))
        if rescore > 1:
            return self._rescore(q32, scores, rows, k)
        return finish_scores(scores, self.metric, q16), rows

    def _topk(self, q16, kk, slices, bias):
        """the kernel on prepared queries: (alpha * dot + bias[row] [Q, kk], rows [Q, kk]); bias f32, at least N entries on the device"""
        def call(lo, n, S, part_score, part_row, scores, rows, s):
            _lib.call("coati_search_topk", ptr(self._vec), self._n, self.dim_padded, ptr(bias), ptr(q16[lo:lo + n]), n, kk,
                      metric_alpha(self.metric), S, ptr(part_score), ptr(part_row), ptr(scores), ptr(rows), s)

        return sliced_topk(self, "EmbeddingIndex.search", q16.shape[0], kk, slices, call)

    def _check_head(self, head, what):
        if head.input_dim != self.dim:
            raise ValueError(f"EmbeddingIndex.{what}: the head's input_dim={head.input_dim}, the index's dim={self.dim}")
        if bool(head.unit_input) != (self.metric == "cosine"):
            raise ValueError(f"EmbeddingIndex.{what}: a head with unit_input={bool(head.unit_input)} on a {self.metric!r} index "
                             "(cosine indices store unit rows, the others rows as given)")

    def property_scores(self, head):
        """[N, P] f32: head (coati_amd.models.regression.PropertyHead, or a GPHead: its mean; on the index's device) on every stored
        row -- one fused kernel over the bf16 rows, removed rows included.  A cosine index stores unit rows, so the head must be one of
        unit inputs (unit_input=True), and only then."""
        self._check_head(head, "property_scores")
        return head.predict_rows(self.vectors)

    def property_uncertainty(self, head):
        """(mean [N, P], std [N, P]) f32 of a coati_amd.models.regression.GPHead on every stored row: one fused kernel
        (GPHead.predict_rows_with_std), under property_scores' rules."""
        self._check_head(head, "property_uncertainty")
        if not hasattr(head, "predict_rows_with_std"):
            raise ValueError("EmbeddingIndex.property_uncertainty: the head gives no standard deviation (a GPHead does)")
        return head.predict_rows_with_std(self.vectors)

    def screen(self, head, k, output=0, largest=True, acquisition=None, beta=1.0, best=None):
        """(scores [k] f32, rows [k] int64): the k best live rows by the head's output `output` -- the largest values first (the smallest
        first for largest=False; the scores returned are the head's own values either way), row index ascending among equal values.
        Removed rows are never returned; fewer than k live rows: the tail is (-inf, -1).  The selection is one call of the search
        kernel, so 1 <= k <= 128: for larger selections sort property_scores(head) yourself.

        acquisition: None or "mean" rank by the head's value.  With a GPHead, "ucb" = mean + beta std, "lcb" = mean - beta std and "ei" =
        the expected improvement over `best` (regression.acquisition_values) rank by that value, computed in torch from the GP kernel's
        two outputs; the scores returned are the acquisition values."""
        k, output = int(k), int(output)
        if k < 1 or k > K_MAX:
            raise ValueError(f"EmbeddingIndex.screen: k={k} outside 1 .. {K_MAX} (for more, sort property_scores)")
        if output < 0 or output >= head.num_outputs:
            raise ValueError(f"EmbeddingIndex.screen: output={output} outside 0 .. {head.num_outputs - 1}")
        if acquisition not in (None, "mean"):
            from .models.regression.gp_head import ACQUISITIONS, acquisition_values
            if acquisition not in ACQUISITIONS:
                raise ValueError(f"EmbeddingIndex.screen: acquisition={acquisition!r} is not one of {ACQUISITIONS}")
            if not hasattr(head, "predict_rows_with_std"):
                raise ValueError(f"EmbeddingIndex.screen: acquisition={acquisition!r} needs a head with a standard deviation (a GPHead)")
            if acquisition == "ei" and best is None:
                raise ValueError("EmbeddingIndex.screen: acquisition='ei' needs best=, the value to improve on")
            mean, std = self.property_uncertainty(head)
            values = acquisition_values(mean[:, output], std[:, output], acquisition, beta, best).to(torch.float32).contiguous()
        else:
            values = self.property_scores(head)[:, output]
        if self._n == 0:
            return (torch.full((k,), float("-inf"), dtype=torch.float32, device=self.device),
                    torch.full((k,), -1, dtype=torch.int64, device=self.device))
        live = self.bias > float("-inf")                     # (not `+ self.bias`: an l2 index keeps -|x|^2 there)
        key = torch.where(live, values if largest else -values, torch.full_like(values, float("-inf"))).contiguous()
        q16 = torch.zeros(1, self.dim_padded, dtype=torch.bfloat16, device=self.device)      # alpha * dot(0, row) + key[row]
        _, rows = self._topk(q16, k, None, key)
        rows = rows[0]
        scores = torch.where(rows >= 0, values[rows.clamp_min(0)], torch.full((k,), float("-inf"), dtype=torch.float32, device=self.device))
        return scores, rows

    def _cluster_operands(self, what, rows=None):
        """(x16, row_bias, rows) for coati_amd.cluster: the stored rows and their bias (-inf = removed), or a gathered subset of them"""
        from .cluster import _check_metric as check_cluster_metric
        check_cluster_metric(self.metric)
        if self.device.type != "cuda":
            raise RuntimeError(f"EmbeddingIndex.{what}: the index is not on a GPU; there is no CPU fallback")
        if rows is None:
            return self.vectors, self.bias, None
        rows = check_rows(f"EmbeddingIndex.{what}", rows, self._n).to(self.device)
        return self.vectors[rows].contiguous(), self.bias[rows].contiguous(), rows

    def assign(self, centres):
        """(assign [N] int32, score [N] f32): every stored row's nearest of centres [K, dim] (K <= 4096) under the index's metric ("cosine"
        or "l2"; "dot" raises ValueError), the lowest index among equally near ones, and the cosine / negated squared distance to it.
        A removed row gets (-1, -inf).  One streaming kernel (coati_amd.cluster.assign_rows); no [N, K] scores exist."""
        from . import cluster
        x16, bias, _ = self._cluster_operands("assign")
        centres = torch.as_tensor(centres)
        if centres.dim() != 2 or centres.shape[1] != self.dim:
            raise ValueError(f"EmbeddingIndex.assign: centres must be [K, {self.dim}], got {tuple(centres.shape)}")
        return cluster.assign_rows(x16, bias, centres, self.metric)

    def kmeans(self, k, iters=20, seed=0, init=None, rows=None):
        """A coati_amd.cluster.Clustering of the live rows into k clusters (spherical k-means on a "cosine" index, plain k-means on an "l2"
        one), reproducible bit for bit from `seed`.  init: a [k, dim] tensor instead of k seeded rows.  rows: cluster this subset only (a
        gathered temporary); the Clustering then carries it as .rows and answers members() / representatives() in library rows."""
        from . import cluster
        x16, bias, rows = self._cluster_operands("kmeans", rows)
        if init is not None and (torch.as_tensor(init).dim() != 2 or torch.as_tensor(init).shape[1] != self.dim):
            raise ValueError(f"EmbeddingIndex.kmeans: init must be [{int(k)}, {self.dim}]")
        out = cluster.kmeans_rows(x16, bias, self.metric, k, iters, seed, init, dim=self.dim)
        out.rows = rows
        return out

    def gmm(self, k, iters=50, seed=0, init="kmeans", rows=None, reg_covar=1e-6, tol=1e-4):
        """A coati_amd.gmm.GaussianMixture of k diagonal Gaussians fitted to the live rows by EM on two fused kernels (an online
        log-sum-exp E-step and a moment-accumulating M-step on the f32 matrix cores; no [N, K] matrix), reproducible bit for bit from
        `seed`.  "cosine" or "l2" index; "dot" raises ValueError.  init: "kmeans" (kmeans(k, seed=seed)'s centres, the global variance)
        or (weights, means, variances).  rows: fit this subset only.  The mixture answers log_prob / predict for any vectors and its
        rsample is what a virtual screen draws from: sampled_virtual_screen(index.gmm(64), head, model, tokenizer, hit_thresh); its
        draws are in the index's prepared space (of about unit norm on a "cosine" index)."""
        from . import gmm
        x16, bias, _ = self._cluster_operands("gmm", rows)
        return gmm.fit_rows(x16, bias, k, iters=iters, seed=seed, init=init, reg_covar=reg_covar, tol=tol, dim=self.dim, metric=self.metric)

    def log_density(self, gmm):
        """[N] f32: log p of every stored row under a GaussianMixture, -inf for removed rows -- one pass of the E-step kernel over the
        stored rows, nothing else allocated"""
        from . import gmm as G
        x16, bias, _ = self._cluster_operands("log_density")
        if gmm.dim != self.dim:
            raise ValueError(f"EmbeddingIndex.log_density: the mixture's dim={gmm.dim}, the index's dim={self.dim}")
        par, cst = G.prepare_params(gmm.weights, gmm.means, gmm.variances, self.dim_padded)
        return G.estep_call(x16, bias, par.to(self.device), cst.to(self.device), want_assign=False)[0]

    def outliers(self, gmm, n):
        """(log_density [n] f32, rows [n] int64): the n live rows of lowest density under the mixture, lowest first (torch.topk)"""
        dens = self.log_density(gmm)
        live = self.bias > float("-inf")
        n = min(int(n), int(live.sum()))
        vals, rows = torch.topk(torch.where(live, dens, torch.full_like(dens, float("inf"))), n, largest=False)
        return vals, rows

    def ivf(self, nlist, iters=20, seed=0, centres=None, fp8=False, keep_rows=True):
        """A coati_amd.ivf.IVFIndex over the live rows: kmeans(nlist, iters, seed)'s clusters (or the nearest of `centres`) as inverted
        lists, for approximate search over the nprobe nearest lists of every query.  fp8=True: a coati_amd.ivf8.Ivf8Index instead -- the
        same lists stored as e4m3 bytes, the candidates re-scored from these bf16 rows (keep_rows=True: a view of them) or stage 1 alone
        (keep_rows=False).  Rows added or removed afterwards are not seen by it."""
        if fp8:
            from .ivf8 import Ivf8Index
            return Ivf8Index.build(self, nlist, iters=iters, seed=seed, centres=centres, keep_rows=keep_rows)
        from .ivf import IVFIndex
        return IVFIndex.build(self, nlist, iters=iters, seed=seed, centres=centres)

    def ivfpq(self, nlist, iters=20, seed=0, centres=None, keep_rows=True, pq_seed=0, pq_iters=20, sample=65536, codebooks=None):
        """A coati_amd.ivfpq.IvfPqIndex over the live rows: ivf(nlist, iters, seed, centres)'s lists, every row stored as one code byte
        per 8 dimensions of its RESIDUAL (row minus its list's centre) under one set of code books fitted on the residuals of at most
        `sample` rows (pq_seed, pq_iters) or given as `codebooks`; the candidates re-scored from these bf16 rows (keep_rows=True: a view of
        them) or stage 1 alone (keep_rows=False).  Rows added or removed afterwards are not seen by it.  dim_padded <= 256."""
        from .ivfpq import IvfPqIndex
        return IvfPqIndex.build(self, nlist, iters=iters, seed=seed, centres=centres, keep_rows=keep_rows, pq_seed=pq_seed, pq_iters=pq_iters,
                                sample=sample, codebooks=codebooks)

    def fp8(self, keep_rows=True):
        """A coati_amd.fp8_index.Fp8Index over the rows present now: every row as e4m3 bytes plus one scale (half the bytes), searched in
        two stages -- a stream over the bytes keeps oversample * k candidates, their exact scores from the bf16 rows decide.
        keep_rows=True holds a view of these bf16 rows; keep_rows=False nothing but bytes, scales and bias (stage 1 alone).  Rows
        added or removed afterwards are not seen by it."""
        from .fp8_index import Fp8Index
        return Fp8Index.build(self, keep_rows=keep_rows)

    def fp4(self, keep_rows=True):
        """A coati_amd.fp4_index.Fp4Index over the rows present now: every row as e2m1 nibbles plus one scale byte per 32 elements (a
        quarter of the bytes and one in 32; dim_padded <= 512, stored in multiples of 128), searched in two stages -- a stream over
        the nibbles keeps oversample * k candidates, their exact scores from the bf16 rows decide.  keep_rows=True holds a view of these
        bf16 rows; keep_rows=False nothing but codes, scales and bias (stage 1 alone).  Rows added or removed afterwards are not seen
        by it."""
        from .fp4_index import Fp4Index
        return Fp4Index.build(self, keep_rows=keep_rows)

    def pq(self, keep_rows=True, seed=0, iters=20, sample=65536, codebooks=None):
        """A coati_amd.pq.PQIndex over the rows present now: every row as one code byte per 8 dimensions (16 times fewer bytes) under code
        books fitted on these rows (seeded k-means per sub-space over at most `sample` of them) or given as `codebooks`, searched in two
        stages -- a stream over the codes keeps oversample * k candidates, their exact scores from the bf16 rows decide.  keep_rows=True
        holds a view of these bf16 rows; keep_rows=False nothing but codes and bias (stage 1 alone).  Rows added or removed afterwards
        are not seen by it.  dim_padded <= 256."""
        from .pq import PQIndex
        return PQIndex.build(self, keep_rows=keep_rows, seed=seed, iters=iters, sample=sample, codebooks=codebooks)

    def radius_count(self, queries, threshold, row_below=None):
        """int64 [Q]: how many live rows score >= threshold for each query (threshold, row_below: as in radius_search) -- the count pass
        of coati_amd.radius alone; nothing is allocated per hit."""
        from . import radius
        return radius.radius_count(self, queries, threshold, row_below)

    def radius_search(self, queries, threshold, order="row", row_below=None, slices=None, max_results=1 << 28):
        """(offsets int64 [Q + 1], scores f32 [T], rows int64 [T]): EVERY live row within the threshold of each query, in CSR form -- query
        i's hits are scores / rows [offsets[i] : offsets[i + 1]].  threshold (a float, or a [Q] tensor) is in the units search() returns:
        cosine or dot score >= threshold; for "l2" the NEGATED squared distance >= threshold, so pass -r * r for "within r".  +inf matches
        nothing, -inf every live row.  A score has the bits search() returns for the same (query, row).
        order: "row" = ascending row (the kernel's order); "score" = score descending, row ascending among equal scores, so that a
        segment begins with what search() returns.  row_below: int [Q], only rows < row_below[i] are hits of query i.  slices: the
        library slices of the kernel's grid (default: coati_radius_slices); the result does not depend on it.  The total is known after the
        count pass (the one synchronisation); above max_results a ValueError names it before anything is allocated."""
        from . import radius
        return radius.radius_search(self, queries, threshold, order, row_below, slices, max_results)

    def near_duplicates(self, threshold, chunk=4096):
        """(offsets int64 [N + 1], scores f32 [T], rows int64 [T]): for every live row i the EARLIER live rows j < i whose score with it is
        >= threshold (units as in radius_search), row ascending -- the self-join, `chunk` rows at a time, of which only the triangle
        j < i is computed.  The queries are the stored bf16 rows themselves, so a copy of a row scores exactly what the stored bits
        give.  A removed row has no neighbours and is nobody's neighbour."""
        from . import radius
        return radius.near_duplicates(self, threshold, chunk)

    def dedup(self, threshold):
        """bool [N] keep mask of the greedy leader rule in row order over near_duplicates(threshold): a live row is kept iff none of its
        earlier neighbours is kept; removed rows are False.  No two kept rows are within the threshold of each other, and every dropped
        live row is within the threshold of a kept one.  The sequential pass runs on the CPU over the rows that have a neighbour."""
        from . import radius
        return radius.dedup(self, threshold)

    def knn_graph(self, k, chunk=4096):
        """(rows int64 [n], nbr int32 [n, k], d2 f32 [n, k]): every live row's k nearest other live rows as positions in `rows`, and the
        squared distances to them (coati_amd.tsne.knn_graph); "cosine" or "l2", 1 <= k <= 127."""
        from . import tsne
        return tsne.knn_graph(self, k, chunk)

    def tsne(self, perplexity=30.0, iters=1000, seed=0, k=None, **layout):
        """A coati_amd.tsne.TSNEResult: the exact t-SNE map of the live rows in two dimensions, reproducible bit for bit from `seed`.
        y [len(index), 2] f32 by row, NaN for removed rows.  k: the neighbours P is held on, default min(n - 1, int(3 perplexity), 127);
        **layout: coati_amd.tsne.layout's arguments (lr, exaggeration, momentum, init, kl_every, ...)."""
        from . import tsne
        return tsne.tsne_index(self, perplexity, iters, seed, k, **layout)

    def _rescore(self, q32, scores, rows, k):
        """the candidates' scores from the f32 copies (a gather and a bmm over [Q, m k, E]), re-sorted: score descending, row ascending"""
        pad = rows < 0
        order = torch.where(pad, torch.full_like(rows, 2 ** 62), rows).argsort(dim=1, stable=True)
        rows, pad = rows.gather(1, order), pad.gather(1, order)
        cand = self._f32[rows.clamp_min(0)]                                   # [Q, kk, E]
        s = torch.bmm(cand, q32.unsqueeze(2)).squeeze(2)
        if self.metric == "l2":
            s = -(cand - q32.unsqueeze(1)).pow(2).sum(dim=2)
        s = torch.where(pad, torch.full_like(s, float("-inf")), s)
        s, order = s.sort(dim=1, descending=True, stable=True)
        return s[:, :k].contiguous(), rows.gather(1, order)[:, :k].contiguous()

    def save(self, path):
        torch.save({"dim": self.dim, "metric": self.metric, "vectors": self.vectors.cpu(), "bias": self.bias.cpu(),
                    "f32": self._f32[:self._n].cpu() if self.keep_f32 and self._f32 is not None else None}, path)

    @classmethod
    def load(cls, path, device="cuda:0"):
        d = torch.load(path, map_location="cpu")
        index = cls(d["dim"], metric=d["metric"], device=device, keep_f32=d["f32"] is not None)
        n = d["vectors"].shape[0]
        index._reserve(n)
        if n:
            index._vec[:n], index._bias[:n] = d["vectors"].to(index.device), d["bias"].to(index.device)
            if index.keep_f32:
                index._f32[:n] = d["f32"].to(index.device)
        index._n = n
        return index
