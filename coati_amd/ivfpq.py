"""IVF-PQ search: an inverted file whose lists hold product-quantisation codes of the RESIDUAL, row minus its list's centre, and an exact
re-scoring of its candidates from the source index's bf16 rows (include/coati_ivfpq.h, csrc/ivfpq.hip).

    ivfpq = index.ivfpq(2048)                              # IVFIndex.build's lists, 1 byte per 8 dimensions; or ivf.pq(index)
    scores, rows = ivfpq.search(queries, k=10, nprobe=8)   # EmbeddingIndex.search's contract over the rows of the 8 nearest lists

The lists, the coarse step (bf16 centres, bf16 queries) and so the probe table are IVFIndex's (coati_amd.ivf.make_lists, ListIndex); the
encoder and the code-book fit are PQIndex's (coati_amd.pq.encode_rows / coati_pq_encode, fit_codebooks), used unchanged; the second stage
is Fp8Index's (coati_amd.fp8_index.rescore_candidates), used as Ivf8Index uses it.

Storage (fixed, so that it can be tested byte for byte), per stored position p of list l:
    centre    c16[l]: the prepared bf16 centre the coarse step uses, [L, dim_padded]
    residual  r16[p] = bf16(f32(x16[ids[p]]) - f32(c16[l])): one subtraction in f32, one rounding to bf16
    codes     codes[p] = encode_rows(r16[p]) under ONE set of residual code books [dim_padded / 8, 256, 8] bf16 shared by all lists,
              fit_codebooks of the residuals of a seeded sample of at most `sample` stored rows (the rows are drawn first, only their
              residuals are formed), or given as codebooks=
    x_hat[p] = c16[l] + entry(codes[p]): the row the position stands for; it exists only in oracles and in dequantised()
    bias      stage 1's: 0 for "cosine"; for "l2" -|x_hat[p]|^2, summed in float64 and stored as f32; -inf once removed
Held per row: dim_padded / 8 code bytes, 4 bytes of ids and 4 of bias -- 40 bytes at dim 256 where Ivf8Index holds 268 and IVFIndex 520.

A search scans the probed lists (coati_ivfpq_scan: the code books in LDS once per workgroup, the centre's share of a score computed once
per work item) keeping R = min(oversample * k, coati_ivfpq_k_max(dim_padded), 128) candidates per query after coati_ivf_merge, and
re-scores those R original rows from the EmbeddingIndex's bf16 rows IN PLACE (coati_search_rescore).  When every row of IVFIndex.search's
top k is among the R candidates the result IS IVFIndex.search's, bit for bit; otherwise every returned score is still the exact score of
its row.  Without the bf16 rows (keep_rows=False, or rescore=False) the result is stage 1's: the metric's score of the query against
x_hat.

Residual codes spend their bytes on what differs INSIDE a list, so they pay once there are at least as many lists as the data has
clusters, and not before: with fewer lists than clusters a list's residuals are as spread as the rows themselves and the flat PQIndex,
which codes the raw row, is as good or better ("Quantised inverted lists").

"dot" has no nearest centre and raises.  There is no CPU fallback for search().  Out of scope: add() after build, per-list or rotated
code books, sub-vectors other than 8 dimensions, dim_padded > 256, more than 4096 lists, radius search, clustering or property heads
over codes, several GPUs, re-scoring from rows in host memory.  The reference has no counterpart."""
import torch

from . import _lib, cluster, pq
from .ivf import make_lists
from .ops import ptr
from .two_stage import ListTwoStage

BUILD_CHUNK = 1 << 20            # rows gathered, subtracted and encoded at a time by build()
DIM_MAX = pq.DIM_MAX             # the code books of a wider row do not fit a CU's LDS


def k_max(E):
    """coati_ivfpq_k_max(E): the largest k of stage 1 at this stored width"""
    lib = _lib.lib()
    km = lib.coati_ivfpq_k_max(int(E))
    if km < 1:
        raise ValueError(f"coati_ivfpq_k_max({E}) = {km}: {lib.coati_last_error().decode('utf-8', 'replace')}")
    return km


def _check_dim(what, dim_padded):
    if dim_padded > DIM_MAX:
        raise ValueError(f"{what}: the rows are stored {dim_padded} wide, above {DIM_MAX}")


def residuals(x16, lists, c16):
    """r16 [n, E] bf16 of bf16 rows x16 [n, E] in the lists `lists` [n] with centres c16 [L, E] bf16: the storage rule's subtraction"""
    return (x16.to(torch.float32) - c16[lists].to(torch.float32)).to(torch.bfloat16)


def list_of(pos, sizes):
    """int64: the list of every stored position pos, from the list sizes [L]"""
    return torch.bucketize(pos, sizes.cumsum(0), right=True)


def fit_residual_codebooks(rows_at, M, sizes, c16, seed=0, iters=20, sample=65536):
    """bf16 [E / 8, 256, 8]: pq.fit_codebooks of the residuals of at most `sample` of the M stored positions, drawn with a CPU generator
    from `seed` (pq._draw).  rows_at(pos) gives the bf16 rows of positions pos: only the drawn rows are gathered."""
    if M < 1:
        raise ValueError("IvfPqIndex: no rows to fit code books on; pass codebooks=")
    pos = pq._draw(M, int(sample), torch.Generator().manual_seed(int(seed))).to(c16.device)
    r16 = residuals(rows_at(pos), list_of(pos, sizes), c16)
    return pq.fit_codebooks(r16, seed=seed, iters=iters, sample=r16.shape[0])


def x_hat64(codes, lists, c16, codebooks):
    """float64 [n, E]: centre plus entry, exact"""
    return c16[lists].double() + pq.reconstruct(codes, codebooks).double()


def stage1_bias(metric, codes, lists, c16, codebooks, bias16):
    """stage 1's bias of positions with these codes in these lists and the bf16 rows' bias bias16 (whose l2 term is not used): 0 for
    "cosine", for "l2" -|x_hat|^2 (summed in float64, stored f32); -inf where bias16 is"""
    if metric != "l2":
        return torch.where(bias16 > float("-inf"), torch.zeros_like(bias16), bias16)
    out = torch.empty_like(bias16)
    step = pq._BIAS_CHUNK
    for lo in range(0, codes.shape[0], step):
        norm = -(x_hat64(codes[lo:lo + step], lists[lo:lo + step], c16, codebooks) ** 2).sum(dim=1).float()
        out[lo:lo + step] = torch.where(bias16[lo:lo + step] > float("-inf"), norm, bias16[lo:lo + step])
    return out


def encode_lists(metric, rows_at, bias_at, M, sizes, c16, codebooks):
    """(codes uint8 [M, E / 8], bias f32 [M]) of the M stored positions in chunks of at most BUILD_CHUNK: a chunk is gathered
    (rows_at(pos), bias_at(pos)), subtracted, encoded (coati_pq_encode on a GPU, pq.encode_rows elsewhere: the same bytes) and given its
    bias.  No bf16 copy of the library or of its residuals exists at any time."""
    dev, E = c16.device, c16.shape[1]
    codes = torch.empty(M, E // pq.SUB, dtype=torch.uint8, device=dev)
    bias = torch.empty(M, dtype=torch.float32, device=dev)
    for lo in range(0, M, BUILD_CHUNK):
        pos = torch.arange(lo, min(lo + BUILD_CHUNK, M), device=dev)
        lists = list_of(pos, sizes)
        r16 = residuals(rows_at(pos), lists, c16).contiguous()
        chunk = pq.encode_device(r16, codebooks) if dev.type == "cuda" else pq.encode_rows(r16, codebooks)
        codes[lo:lo + BUILD_CHUNK] = chunk
        bias[lo:lo + BUILD_CHUNK] = stage1_bias(metric, chunk, lists, c16, codebooks, bias_at(pos))
    return codes, bias


class IvfPqIndex(ListTwoStage):
    """An inverted-file index over the live rows of an EmbeddingIndex at the time of build(), the rows stored as PQ codes of their
    residuals in list order.  len() is the source's; rows returned by search are the source's rows.  Attributes: centres [L, dim] f32,
    nlist, metric, dim, dim_padded, device, keep_rows."""

    def __init__(self, dim, dim_padded, metric, n, centres, codes, codebooks, ids, bias, sizes, rows16=None, bias16=None, device="cuda:0"):
        cluster._check_metric(metric)
        _check_dim("IvfPqIndex", int(dim_padded))
        pq._check_codebooks(codebooks, int(dim_padded))
        self._init_lists(dim, dim_padded, metric, n, centres, ids, sizes, device)
        self._codes = codes.to(self.device).contiguous()
        self._cb = codebooks.to(self.device).contiguous()
        self._bias = bias.to(self.device, torch.float32).contiguous()
        if self._codes.dtype != torch.uint8 or self._codes.shape != (self._m, self.dim_padded // pq.SUB) or self._bias.shape != (self._m,):
            raise ValueError("IvfPqIndex: codes, ids and bias do not match the list sizes")
        self._adopt_rows(rows16, bias16)

    # ---- building ----------------------------------------------------------------------------------------------------------------
    @classmethod
    def _from_lists(cls, metric, dim, dim_padded, n, centres, order, sizes, rows_at, bias_at, rows16, bias16, device, pq_seed, pq_iters,
                    sample, codebooks):
        M = int(order.shape[0])
        c16 = cluster.prepare_centres(centres, metric, dim_padded, device)[1]      # (what ListIndex holds as _c16)
        sizes = sizes.to(c16.device)
        if codebooks is None:
            codebooks = fit_residual_codebooks(rows_at, M, sizes, c16, pq_seed, pq_iters, sample)
        pq._check_codebooks(codebooks, dim_padded)
        codebooks = codebooks.to(c16.device).contiguous()
        codes, bias = encode_lists(metric, rows_at, bias_at, M, sizes, c16, codebooks)
        return cls(dim, dim_padded, metric, n, centres, codes, codebooks, order, bias, sizes, rows16, bias16, device)

    @classmethod
    def build(cls, index, nlist, iters=20, seed=0, centres=None, assign=None, keep_rows=True, pq_seed=0, pq_iters=20, sample=65536,
              codebooks=None):
        """index: an EmbeddingIndex ("cosine" or "l2") on a GPU; nlist, iters, seed, centres, assign: IVFIndex.build's, and the same lists
        for the same arguments.  pq_seed, pq_iters, sample: the fit of the residual code books (fit_residual_codebooks), or codebooks=
        [dim_padded / 8, 256, 8] bf16 given.  The rows are gathered into list order, subtracted and encoded in chunks of at most 2^20.
        keep_rows=True holds a VIEW of the index's bf16 rows and a clone of its bias, by original row, for stage 2; keep_rows=False holds
        codes and bias only and search() is stage 1 alone."""
        cluster._check_metric(index.metric)
        _check_dim("IvfPqIndex.build", index.dim_padded)
        centres, order, sizes = make_lists("IvfPqIndex.build", index, nlist, iters, seed, centres, assign)
        x16, bias16 = index.vectors, index.bias
        return cls._from_lists(index.metric, index.dim, index.dim_padded, len(index), centres, order, sizes,
                               lambda pos: x16[order[pos]], lambda pos: bias16[order[pos]], x16 if keep_rows else None,
                               bias16.clone() if keep_rows else None, index.device, pq_seed, pq_iters, sample, codebooks)

    @classmethod
    def from_ivf(cls, ivf, index=None, pq_seed=0, pq_iters=20, sample=65536, codebooks=None):
        """The lists of an IVFIndex with its stored rows coded: what build() gives for the same lists and the same pq_seed, pq_iters,
        sample, codebooks.  index: the source EmbeddingIndex (same length, dim and metric); its bf16 rows (a view) and a clone of its
        bias serve stage 2.  Without it keep_rows is False."""
        if index is not None and (len(index) != len(ivf) or index.dim != ivf.dim or index.metric != ivf.metric):
            raise ValueError(f"IvfPqIndex.from_ivf: the index ({len(index)} rows, dim {index.dim}, {index.metric!r}) is not the IVFIndex's source "
                             f"({len(ivf)} rows, dim {ivf.dim}, {ivf.metric!r})")
        _check_dim("IvfPqIndex.from_ivf", ivf.dim_padded)
        vec, bias = ivf.vectors, ivf.bias
        return cls._from_lists(ivf.metric, ivf.dim, ivf.dim_padded, len(ivf), ivf.centres, ivf.ids.long(), ivf.sizes,
                               lambda pos: vec[pos], lambda pos: bias[pos], None if index is None else index.vectors,
                               None if index is None else index.bias.clone(), ivf.device, pq_seed, pq_iters, sample, codebooks)

    @property
    def codes(self):
        """the stored code bytes [M, dim_padded / 8] uint8 in list order"""
        return self._codes

    @property
    def codebooks(self):
        """the residual code books [dim_padded / 8, 256, 8] bf16, shared by all lists"""
        return self._cb

    @property
    def centres16(self):
        """the prepared bf16 centres [L, dim_padded]: the coarse step's library and the constant part of every list's rows"""
        return self._c16

    @property
    def bias(self):
        """stage 1's f32 bias [M] by position: 0, -|x_hat|^2 for l2, -inf once removed"""
        return self._bias

    def dequantised(self):
        """f32 [M, dim_padded]: the rows the codes stand for, centre plus entry (one f32 addition), in list order"""
        lists = list_of(torch.arange(self._m, device=self.device), self._sizes)
        return self._c16[lists].float() + pq.reconstruct(self._codes, self._cb).float()

    def bytes_per_row(self):
        """what stage 1 holds per row: the code bytes, the int32 id and the f32 bias"""
        return self.dim_padded // pq.SUB + 8

    # ---- searching (ListTwoStage) ----------------------------------------------------------------------------------------------------
    def _stage1_queries(self, q16, rescore):
        return q16, q16

    def _scan(self, q16, pos_bias, kk, alpha, blocks):
        def scan(lo, n, pair_q, pair_off, item_off, P, seg_rows, segs, part_score, part_row, s):
            _lib.call("coati_ivfpq_scan", ptr(self._codes), ptr(self._ids), ptr(pos_bias), ptr(self._list_off), self._m, self.dim_padded,
                      self.nlist, ptr(self._c16), ptr(self._cb), ptr(q16[lo:lo + n]), n, ptr(pair_q), ptr(pair_off), ptr(item_off), P, kk,
                      alpha, seg_rows, segs, ptr(part_score), ptr(part_row), int(blocks), s)
        return scan

    def search(self, queries, k, nprobe=8, oversample=4, rescore=None, probes=None, seg_rows=None, bias=None, return_probes=False, blocks=0):
        """(scores [Q, k] f32, rows [Q, k] int64): EmbeddingIndex.search's contract over every query's probed lists -- the metric's score,
        descending, original row ascending among equal scores, (-inf, -1) where fewer rows qualify.  Stage 1 keeps
        R = min(oversample * k, coati_ivfpq_k_max(dim_padded), 128) candidates per query, stage 2 returns the best k of them by their
        exact scores.  rescore: default keep_rows; False: stage 1's k best with stage 1's scores (of x_hat); True without the bf16 rows
        raises.  nprobe, probes, seg_rows, blocks, return_probes: IVFIndex.search's (seg_rows defaults to coati_ivf_plan at R).  bias:
        f32 [N] over ORIGINAL rows, added to every row's score in both stages, -inf excluding a row.  oversample=4 is Ivf8Index's
        default, kept: see DESIGN.md section 6 for what was and was not measured."""
        return self._search(queries, k, nprobe, oversample, rescore, probes, seg_rows, bias, return_probes, blocks, k_max(self.dim_padded),
                            f", the limit of coati_ivfpq_k_max({self.dim_padded})")

    # ---- persistence ---------------------------------------------------------------------------------------------------------------
    def save(self, path):
        """centres, code books, codes, ids, bias and sizes; with the bf16 rows kept, those and their bias too"""
        d = {"dim": self.dim, "dim_padded": self.dim_padded, "metric": self.metric, "n": self._n, "centres": self.centres.cpu(),
             "codes": self._codes.cpu(), "codebooks": self._cb.cpu(), "ids": self._ids.cpu(), "bias": self._bias.cpu(),
             "sizes": self._sizes.cpu()}
        if self.keep_rows:
            d.update(rows16=self._rows16.cpu(), bias16=self._bias16.cpu())
        torch.save(d, path)

    @classmethod
    def load(cls, path, device="cuda:0"):
        d = torch.load(path, map_location="cpu")
        rows16 = d["rows16"].to(device) if "rows16" in d else None
        return cls(d["dim"], d["dim_padded"], d["metric"], d["n"], d["centres"], d["codes"], d["codebooks"], d["ids"], d["bias"], d["sizes"],
                   rows16, d.get("bias16"), device)
