"""Quantised search over an embedding library: the rows as OCP e4m3 bytes plus one power-of-two scale each, half the bytes of the bf16
rows, and a two-stage search on top of them (include/coati_search8.h, csrc/search8.hip).

    fp8 = index.fp8()                                    # a snapshot of an EmbeddingIndex's rows; keep_rows=False: bytes and scales only
    scores, rows = fp8.search(queries, k=10)             # EmbeddingIndex.search's contract

Stage 1 streams the fp8 rows against fp8 queries on the matrix cores (coati_search8_topk) and keeps the R = min(oversample * k, 128) best
per query; stage 2 (coati_search_rescore) scores those R rows again from the bf16 rows with the exact search's arithmetic and returns the
best k.  When every row of the exact top k is among the R candidates the result IS EmbeddingIndex.search's, bit for bit; otherwise
every returned score is still the exact score of its row.  Without the bf16 rows (keep_rows=False, or rescore=False) the result is
stage 1's: the metric's score of the DEQUANTISED operands.

Storage (fixed, so that it can be tested byte for byte): a row is the index's stored bf16 row divided by s = 2^j, j the smallest integer
with max|x| <= 448 * 2^j (j within -126 .. 127; s = 1 for a row of zeros), rounded to e4m3 (e4m3fn, round to nearest even).  Nothing
saturates, and data that e4m3 holds exactly -- integers of magnitude <= 15, for one -- is stored and scored exactly.  Queries are
quantised the same way.  Stage 1's bias is the index's for "dot" and "cosine"; for "l2" it is -|x_hat|^2 of the dequantised row (summed
in float64, stored as f32), so that its score is the negated squared distance between the dequantised operands.

There is no CPU fallback for search().  The same storage inside inverted lists -- the rows of the probed lists only, the same second
stage -- is coati_amd.ivf8.Ivf8Index, which uses this module's quantiser and rescore_candidates.  Storage below fp8 is
coati_amd.fp4_index.Fp4Index (e2m1 nibbles with one scale byte per block of 32, the same second stage) and coati_amd.pq.PQIndex (product
quantisation, one byte per 8 dimensions), which also has add() after build.  Out of scope here: add() after build (rebuild instead),
radius search, clustering or property heads over fp8 rows, fp6, bf16 rows kept in host memory, R > 128.  The reference has no counterpart."""
import torch

from . import _lib
from .ops import ptr, stream
from .search import _check_metric
from .two_stage import R_MAX, FlatTwoStage, rescore_candidates  # noqa: F401  (stage 2 and its limit are importable from here)

E4M3_MAX = 448.0


def scale_exponents(amax):
    """int32 [n]: per largest magnitude amax [n] f32 the smallest j with amax <= 448 * 2^j, within -126 .. 127; 0 where amax == 0.
    Integer arithmetic on frexp's parts: amax = m * 2^e with 0.5 <= m < 1 is <= 0.875 * 2^(j + 9) iff j >= e - 9 (m <= 0.875) or e - 8."""
    mant, exp = torch.frexp(amax.to(torch.float32))
    j = torch.where(mant <= 0.875, exp - 9, exp - 8).clamp(-126, 127)
    return torch.where(amax == 0, torch.zeros_like(j), j).to(torch.int32)


def quantise_rows(x16):
    """(bytes [n, E] uint8, scale [n] f32) of bf16 rows [n, E]: the storage rule above in plain torch, on the tensor's device --
    what coati_quant_rows_fp8 computes, bit for bit."""
    x = x16.to(torch.float32)
    j = scale_exponents(x.abs().amax(dim=1)) if x.shape[1] else torch.zeros(x.shape[0], dtype=torch.int32, device=x.device)
    scale = ((j + 127) << 23).to(torch.int32).view(torch.float32)               # 2^j, from its bits
    return (x / scale[:, None]).to(torch.float8_e4m3fn).view(torch.uint8), scale


def dequantise(bytes8, scale):
    """f32 [n, E]: the values the bytes and scales stand for (exact: an e4m3 value times a power of two)"""
    return bytes8.view(torch.float8_e4m3fn).to(torch.float32) * scale[:, None]


def stage1_bias(metric, vec8, scale, bias16):
    """stage 1's bias of rows with bytes vec8, scales `scale` and the bf16 rows' bias bias16: the latter, for "l2" -|x_hat|^2 of the
    dequantised row (summed in float64, stored f32) where it is above -inf"""
    if metric != "l2":
        return bias16
    norm = -(dequantise(vec8, scale).double() ** 2).sum(dim=1).float()
    return torch.where(bias16 > float("-inf"), norm, bias16)


def quantise_device(x16):
    """quantise_rows by the kernel (coati_quant_rows_fp8); x16 bf16 [n, E] contiguous on a GPU"""
    n, E = x16.shape
    out = torch.empty(n, E, dtype=torch.uint8, device=x16.device)
    scale = torch.empty(n, dtype=torch.float32, device=x16.device)
    if n:
        with torch.cuda.device(x16.device):
            _lib.call("coati_quant_rows_fp8", ptr(x16), n, E, ptr(out), ptr(scale), stream())
    return out, scale


class Fp8Index(FlatTwoStage):
    """The rows of an EmbeddingIndex at the time of build() as e4m3 bytes and scales; len() and the rows returned are the source's.
    Attributes: dim, dim_padded, metric, device, keep_rows."""
    _slices_entry = "coati_search8_slices"
    _payload = {"vectors8": "_vec8", "scales": "_scale"}
    _quantise_rows = staticmethod(quantise_rows)

    def __init__(self, dim, dim_padded, metric, vectors8, scales, bias, rows16=None, bias16=None, device="cuda:0"):
        _check_metric(metric)
        self.dim, self.dim_padded, self.metric, self.device = int(dim), int(dim_padded), metric, torch.device(device)
        self._vec8 = vectors8.to(self.device).contiguous()
        self._scale = scales.to(self.device, torch.float32).contiguous()
        self._bias = bias.to(self.device, torch.float32).contiguous()
        self._n = int(self._vec8.shape[0])
        if self._vec8.dtype != torch.uint8 or self._vec8.shape != (self._n, self.dim_padded) or self._scale.shape != (self._n,) \
                or self._bias.shape != (self._n,):
            raise ValueError("Fp8Index: bytes, scales and bias do not match")
        self._adopt_rows(rows16, self._bias if bias16 is None else bias16)

    # ---- building ----------------------------------------------------------------------------------------------------------------
    @classmethod
    def build(cls, index, keep_rows=True):
        """index: an EmbeddingIndex.  A snapshot: rows added to the index later are not seen, rows removed from it later are still
        returned (remove() them here too).  keep_rows=True holds a VIEW of the index's bf16 rows for stage 2, no copy;
        keep_rows=False holds bytes, scales and bias only -- half the index's memory -- and search() is stage 1 alone."""
        x16, bias16 = index.vectors, index.bias.clone()
        if x16.device.type == "cuda":
            vec8, scale = quantise_device(x16)
        else:
            vec8, scale = quantise_rows(x16)
        bias = stage1_bias(index.metric, vec8, scale, bias16)
        return cls(index.dim, index.dim_padded, index.metric, vec8, scale, bias, x16 if keep_rows else None, bias16 if keep_rows else None,
                   index.device)

    @property
    def vectors8(self):
        """the stored e4m3 bytes [N, dim_padded] uint8 (a view)"""
        return self._vec8

    @property
    def scales(self):
        """the rows' f32 scales [N] (a view): powers of two"""
        return self._scale

    @property
    def bias(self):
        """stage 1's f32 bias [N] (a view): the index's, -|x_hat|^2 for l2, -inf once removed"""
        return self._bias

    def dequantised(self):
        """f32 [N, dim_padded]: the rows the bytes and scales stand for"""
        return dequantise(self._vec8, self._scale)

    # ---- searching (FlatTwoStage) ----------------------------------------------------------------------------------------------------
    def _default_slices(self, qc, kk):
        return _lib.lib().coati_search8_slices(self._n, qc, kk)

    def _stage1_queries(self, q16, rescore):
        q8, qscale = quantise_device(q16)
        return (q8, qscale), None if rescore else dequantise(q8, qscale)

    def _stage1_call(self, qs, bias1, lo, n, kk, alpha, S, part_score, part_row, scores, rows, s):
        _lib.call("coati_search8_topk", ptr(self._vec8), ptr(self._scale), self._n, self.dim_padded, ptr(bias1), ptr(qs[0][lo:lo + n]),
                  ptr(qs[1][lo:lo + n]), n, kk, alpha, S, ptr(part_score), ptr(part_row), ptr(scores), ptr(rows), s)

    def search(self, queries, k, oversample=4, rescore=None, slices=None, bias=None):
        """(scores [Q, k] f32, rows [Q, k] int64): EmbeddingIndex.search's contract -- the metric's score, descending, row ascending among
        equal scores, (-inf, -1) where fewer rows qualify.  Stage 1 keeps R = min(oversample * k, 128) candidates per query, stage 2
        returns the best k of them by their exact scores.  rescore: default keep_rows; False: stage 1's k best with stage 1's scores (of
        the dequantised operands); True without the bf16 rows raises.  slices: the library slices of stage 1's grid (default:
        coati_search8_slices); the result does not depend on it.  bias: f32 [N], added to every row's score in both stages, -inf
        excluding a row."""
        return self._search(queries, k, oversample, rescore, slices, bias)

