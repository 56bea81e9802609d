"""Quantised approximate search: an inverted file whose lists are stored as OCP e4m3 bytes plus one power-of-two scale per row, and an
exact re-scoring of its candidates from the source index's bf16 rows (include/coati_ivf8.h, csrc/ivf8.hip).

    ivf8 = index.ivf(2048, fp8=True)                      # IVFIndex.build's lists, half the bytes; or ivf.fp8(index) of an existing IVFIndex
    scores, rows = ivf8.search(queries, k=10, nprobe=8)   # EmbeddingIndex.search's contract over the rows of the 8 nearest lists

The lists, the coarse step (bf16 centres, bf16 queries) and so the probe table are IVFIndex's (coati_amd.ivf.make_lists, ListIndex); the
storage rule, the quantiser and the second stage are Fp8Index's (coati_amd.fp8_index).  A search quantises the queries, scans the probed
lists on the fp8 matrix cores (coati_ivf8_scan) keeping R = min(oversample * k, 128) candidates per query after coati_ivf_merge, and
re-scores those R original rows from the EmbeddingIndex's bf16 rows IN PLACE (coati_search_rescore): no bf16 copy of the library in list
order is ever made, so the index costs half the library's bytes on top of it where IVFIndex costs all of them again, and with
keep_rows=False half the bytes are the whole searchable library.  When every row of IVFIndex.search's top k is among the R candidates
the result IS IVFIndex.search's, bit for bit; otherwise every returned score is still the exact score of its row.  Without the bf16 rows
(keep_rows=False, or rescore=False) the result is stage 1's: the metric's score of the DEQUANTISED operands.  Stage 1's bias is the
index's for "cosine"; for "l2" it is -|x_hat|^2 of the dequantised row (summed in float64, stored as f32).

"dot" has no nearest centre and raises.  There is no CPU fallback for search().  Out of scope: fp8 centres or an fp8 coarse step,
re-scoring from bf16 rows in list order or in host memory, add() after build, R > 128, radius search, clustering or property heads over
fp8 lists, per-block scales, fp6 / fp4, more than 4096 lists, several GPUs.  Product quantisation inside the lists is coati_amd.ivfpq.IvfPqIndex.  The reference has no counterpart."""
import torch

from . import _lib
from .fp8_index import dequantise, quantise_device, quantise_rows, stage1_bias
from .ivf import make_lists
from .ops import ptr
from .two_stage import ListTwoStage

BUILD_CHUNK = 1 << 20            # rows gathered and quantised at a time by build()


def _quantise(x16):
    return quantise_device(x16) if x16.device.type == "cuda" else quantise_rows(x16)


class Ivf8Index(ListTwoStage):
    """An inverted-file index over the live rows of an EmbeddingIndex at the time of build(), the rows stored as e4m3 bytes and scales
    in list order.  len() is the source's; rows returned by search are the source's rows.  Attributes: centres [L, dim] f32, nlist, metric,
    dim, dim_padded, device, keep_rows."""

    def __init__(self, dim, dim_padded, metric, n, centres, vectors8, scales, ids, bias, sizes, rows16=None, bias16=None, device="cuda:0"):
        self._init_lists(dim, dim_padded, metric, n, centres, ids, sizes, device)
        self._vec8 = vectors8.to(self.device).contiguous()
        self._scale = scales.to(self.device, torch.float32).contiguous()
        self._bias = bias.to(self.device, torch.float32).contiguous()
        if self._vec8.dtype != torch.uint8 or self._vec8.shape != (self._m, self.dim_padded) or self._scale.shape != (self._m,) \
                or self._bias.shape != (self._m,):
            raise ValueError("Ivf8Index: bytes, scales, ids and bias do not match the list sizes")
        self._adopt_rows(rows16, bias16)

    # ---- building ----------------------------------------------------------------------------------------------------------------
    @classmethod
    def build(cls, index, nlist, iters=20, seed=0, centres=None, assign=None, keep_rows=True):
        """index: an EmbeddingIndex ("cosine" or "l2") on a GPU; nlist, iters, seed, centres, assign: IVFIndex.build's, and the same lists
        for the same arguments.  The rows are gathered into list order and quantised in chunks of at most 2^20: no bf16 copy of the
        library exists at any time.  keep_rows=True holds a VIEW of the index's bf16 rows and a clone of its bias, by original row, for
        stage 2; keep_rows=False holds bytes, scales and bias only and search() is stage 1 alone."""
        centres, order, sizes = make_lists("Ivf8Index.build", index, nlist, iters, seed, centres, assign)
        x16, bias16 = index.vectors, index.bias
        M = order.shape[0]
        vec8 = torch.empty(M, index.dim_padded, dtype=torch.uint8, device=index.device)
        scale = torch.empty(M, dtype=torch.float32, device=index.device)
        bias = torch.empty(M, dtype=torch.float32, device=index.device)
        for lo in range(0, M, BUILD_CHUNK):
            rows = order[lo:lo + BUILD_CHUNK]
            vec8[lo:lo + BUILD_CHUNK], scale[lo:lo + BUILD_CHUNK] = _quantise(x16[rows])
            bias[lo:lo + BUILD_CHUNK] = stage1_bias(index.metric, vec8[lo:lo + BUILD_CHUNK], scale[lo:lo + BUILD_CHUNK], bias16[rows])
        return cls(index.dim, index.dim_padded, index.metric, len(index), centres, vec8, scale, order, bias, sizes,
                   x16 if keep_rows else None, bias16.clone() if keep_rows else None, index.device)

    @classmethod
    def from_ivf(cls, ivf, index=None):
        """The lists of an IVFIndex with its stored rows quantised.  index: the source EmbeddingIndex (same length, dim and metric); its
        bf16 rows (a view) and a clone of its bias serve stage 2.  Without it keep_rows is False."""
        if index is not None and (len(index) != len(ivf) or index.dim != ivf.dim or index.metric != ivf.metric):
            raise ValueError(f"Ivf8Index.from_ivf: the index ({len(index)} rows, dim {index.dim}, {index.metric!r}) is not the IVFIndex's source "
                             f"({len(ivf)} rows, dim {ivf.dim}, {ivf.metric!r})")
        M = ivf.vectors.shape[0]
        vec8 = torch.empty(M, ivf.dim_padded, dtype=torch.uint8, device=ivf.device)
        scale = torch.empty(M, dtype=torch.float32, device=ivf.device)
        bias = torch.empty(M, dtype=torch.float32, device=ivf.device)
        for lo in range(0, M, BUILD_CHUNK):
            hi = lo + BUILD_CHUNK
            vec8[lo:hi], scale[lo:hi] = _quantise(ivf.vectors[lo:hi])
            bias[lo:hi] = stage1_bias(ivf.metric, vec8[lo:hi], scale[lo:hi], ivf.bias[lo:hi])
        return cls(ivf.dim, ivf.dim_padded, ivf.metric, len(ivf), ivf.centres, vec8, scale, ivf.ids, bias, ivf.sizes,
                   None if index is None else index.vectors, None if index is None else index.bias.clone(), ivf.device)

    @property
    def vectors8(self):
        """the stored e4m3 bytes [M, dim_padded] uint8 in list order"""
        return self._vec8

    @property
    def scales(self):
        """the positions' f32 scales [M]: powers of two"""
        return self._scale

    @property
    def bias(self):
        """stage 1's f32 bias [M] by position: the index's, -|x_hat|^2 for l2, -inf once removed"""
        return self._bias

    def dequantised(self):
        """f32 [M, dim_padded]: the rows the bytes and scales stand for, in list order"""
        return dequantise(self._vec8, self._scale)

    # ---- searching (ListTwoStage) ----------------------------------------------------------------------------------------------------
    def _stage1_queries(self, q16, rescore):
        q8, qscale = quantise_device(q16)
        return (q8, qscale), None if rescore else dequantise(q8, qscale)

    def _scan(self, qs, pos_bias, kk, alpha, blocks):
        def scan(lo, n, pair_q, pair_off, item_off, P, seg_rows, segs, part_score, part_row, s):
            _lib.call("coati_ivf8_scan", ptr(self._vec8), ptr(self._scale), ptr(self._ids), ptr(pos_bias), ptr(self._list_off), self._m,
                      self.dim_padded, self.nlist, ptr(qs[0][lo:lo + n]), ptr(qs[1][lo:lo + n]), n, ptr(pair_q), ptr(pair_off), ptr(item_off),
                      P, kk, alpha, seg_rows, segs, ptr(part_score), ptr(part_row), int(blocks), s)
        return scan

    def search(self, queries, k, nprobe=8, oversample=4, rescore=None, probes=None, seg_rows=None, bias=None, return_probes=False, blocks=0):
        """(scores [Q, k] f32, rows [Q, k] int64): EmbeddingIndex.search's contract over every query's probed lists -- the metric's score,
        descending, original row ascending among equal scores, (-inf, -1) where fewer rows qualify.  Stage 1 keeps
        R = min(oversample * k, 128) candidates per query, stage 2 returns the best k of them by their exact scores.  rescore: default
        keep_rows; False: stage 1's k best with stage 1's scores (of the dequantised operands); True without the bf16 rows raises.
        nprobe, probes, seg_rows, blocks, return_probes: IVFIndex.search's (seg_rows defaults to coati_ivf_plan at R).  bias: f32 [N]
        over ORIGINAL rows, added to every row's score in both stages, -inf excluding a row."""
        return self._search(queries, k, nprobe, oversample, rescore, probes, seg_rows, bias, return_probes, blocks)

    # ---- persistence ---------------------------------------------------------------------------------------------------------------
    def save(self, path):
        """With the bf16 rows kept they are what is saved (load() quantises them again: the same bytes), else bytes and scales."""
        d = {"dim": self.dim, "dim_padded": self.dim_padded, "metric": self.metric, "n": self._n, "centres": self.centres.cpu(),
             "ids": self._ids.cpu(), "bias": self._bias.cpu(), "sizes": self._sizes.cpu()}
        if self.keep_rows:
            d.update(rows16=self._rows16.cpu(), bias16=self._bias16.cpu())
        else:
            d.update(vectors8=self._vec8.cpu(), scales=self._scale.cpu())
        torch.save(d, path)

    @classmethod
    def load(cls, path, device="cuda:0"):
        d = torch.load(path, map_location="cpu")
        rows16 = bias16 = None
        if "rows16" in d:
            vec8, scale = quantise_rows(d["rows16"][d["ids"].long()])
            rows16, bias16 = d["rows16"].to(device), d["bias16"]
        else:
            vec8, scale = d["vectors8"], d["scales"]
        return cls(d["dim"], d["dim_padded"], d["metric"], d["n"], d["centres"], vec8, scale, d["ids"], d["bias"], d["sizes"], rows16, bias16,
                   device)
