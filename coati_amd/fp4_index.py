"""Four-bit search over an embedding library: the rows as OCP e2m1 (fp4) nibbles with one E8M0 scale byte per 32 elements -- the OCP
Microscaling block format, a quarter of the bf16 rows' bytes plus one byte in 32 -- and a two-stage search on top of them
(include/coati_search4.h, csrc/search4.hip).

    fp4 = index.fp4()                                    # a snapshot of an EmbeddingIndex's rows; keep_rows=False: codes and scales only
    scores, rows = fp4.search(queries, k=10)             # EmbeddingIndex.search's contract

Stage 1 streams the fp4 rows against e4m3 queries on the matrix cores (coati_search4_topk: v_mfma_scale_f32_16x16x128_f8f6f4, which
applies the block scales itself) and keeps the R = min(oversample * k, 128) best per query; stage 2 is Fp8Index's
(fp8_index.rescore_candidates, unchanged): it scores those R rows again from the bf16 rows with the exact search's arithmetic and
returns the best k.  When every row of the exact top k is among the R candidates the result IS EmbeddingIndex.search's, bit for bit;
otherwise every returned score is still the exact score of its row.  Without the bf16 rows (keep_rows=False, or rescore=False) the
result is stage 1's: the metric's score of the DEQUANTISED operands.

Storage (fixed, so that it can be tested byte for byte): E = the index's dim_padded, E4 = 128 * ceil(E / 128) the stored width
(128 <= E4 <= 512), elements at and beyond E taken as zero.  Block b of a row covers elements 32 b .. 32 b + 31; its exponent j is the
smallest integer with max|x| <= 6 * 2^j, within -126 .. 126, 0 for a block of zeros; its scale byte is j + 127 (E8M0; 127 in pad
blocks, never 255).  An element is x * 2^-j (exact) rounded to the nearest of {0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the even code, the
sign kept (-0 stays -0); its nibble is sign << 3 | code; byte i of a row's codes holds element 2 i in its low nibble and element
2 i + 1 in its high one.  Nothing saturates, and integers from {0, +-1, +-2, +-3, +-4, +-6} times any per-block power of two are stored
and scored exactly.  Queries are quantised as Fp8Index quantises them (coati_quant_rows_fp8 on the bf16 query zero-padded to E4):
they live in registers, so four-bit queries would cost recall and save nothing.  Stage 1's bias is Fp8Index's rule: the index's for
"dot" and "cosine", -|x_hat|^2 of the dequantised row (summed in float64, stored as f32) for "l2", -inf once removed.

There is no CPU fallback for search().  Out of scope here: inverted lists of fp4 rows, fp6, four-bit queries, scales finer or
coarser than 32 elements, add() after build (rebuild instead), R > 128, E4 > 512, radius search, clustering or property heads over
fp4 rows, several GPUs, bf16 rows kept in host memory.  The reference has no counterpart."""
import torch

from . import _lib
from . import fp8_index as _F8
from .ops import ptr, stream
from .search import _check_metric
from .two_stage import FlatTwoStage

E4_MAX = 512
BLOCK = 32                       # elements per scale byte
E2M1_MAX = 6.0
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def stored_width(E):
    """E4 = 128 * ceil(E / 128): the width of a stored row in elements; E % 32 == 0, E4 <= 512"""
    E = int(E)
    if E < 32 or E % 32:
        raise ValueError(f"Fp4Index: width {E} is not a positive multiple of 32")
    E4 = (E + 127) // 128 * 128
    if E4 > E4_MAX:
        raise ValueError(f"Fp4Index: a {E}-wide row is stored {E4} wide, above {E4_MAX}")
    return E4


def block_exponents(amax):
    """int32, amax's shape: per largest magnitude amax (f32) the smallest j with amax <= 6 * 2^j, within -126 .. 126; 0 where
    amax == 0.  Integer arithmetic on frexp's parts: amax = m * 2^e with 0.5 <= m < 1 is <= 0.75 * 2^(j + 3) iff j >= e - 3
    (m <= 0.75) or e - 2."""
    mant, exp = torch.frexp(amax.to(torch.float32))
    j = torch.where(mant <= 0.75, exp - 3, exp - 2).clamp(-126, 126)
    return torch.where(amax == 0, torch.zeros_like(j), j).to(torch.int32)


def quantise_rows(x16):
    """(codes [n, E4 / 2] uint8, scales [n, E4 / 32] uint8) of bf16 rows [n, E]: the storage rule above in plain torch, on the
    tensor's device -- what coati_quant_rows_fp4 computes, byte for byte."""
    n, E = x16.shape
    E4 = stored_width(E)
    x = torch.nn.functional.pad(x16.to(torch.float32), (0, E4 - E)).reshape(n, E4 // BLOCK, BLOCK)
    j = block_exponents(x.abs().amax(dim=2))                                        # [n, E4 / 32]
    inv = ((127 - j) << 23).to(torch.int32).view(torch.float32)                   # 2^-j, from its bits
    y = x * inv[:, :, None]                                                         # exact
    a = y.abs()
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8) + (a >= 1.75).to(torch.uint8)
            + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8) + (a > 5.0).to(torch.uint8))           # ties to the even code
    nib = (code | (torch.signbit(y).to(torch.uint8) << 3)).reshape(n, E4 // 2, 2)
    return (nib[:, :, 0] | (nib[:, :, 1] << 4)).contiguous(), (j + 127).to(torch.uint8)


def dequantise(codes, scales):
    """f32 [n, E4]: the values the nibbles and scale bytes stand for (exact: an e2m1 value times a power of two)"""
    n = codes.shape[0]
    table = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32, device=codes.device)
    nib = torch.stack([codes & 15, codes >> 4], dim=2).reshape(n, -1).long()
    two_j = (scales.to(torch.int32) << 23).view(torch.float32)                      # 2^(byte - 127)
    return (table[nib].reshape(n, -1, BLOCK) * two_j[:, :, None]).reshape(n, -1)


def stage1_bias(metric, codes, scales, bias16):
    """stage 1's bias of rows with these codes and scales and the bf16 rows' bias bias16: the latter, for "l2" -|x_hat|^2 of the
    dequantised row (summed in float64, stored f32) where it is above -inf"""
    if metric != "l2":
        return bias16
    norm = -(dequantise(codes, scales).double() ** 2).sum(dim=1).float()
    return torch.where(bias16 > float("-inf"), norm, bias16)


def quantise_device(x16):
    """quantise_rows by the kernel (coati_quant_rows_fp4); x16 bf16 [n, E] contiguous on a GPU"""
    n, E = x16.shape
    E4 = stored_width(E)
    codes = torch.empty(n, E4 // 2, dtype=torch.uint8, device=x16.device)
    scales = torch.empty(n, E4 // BLOCK, dtype=torch.uint8, device=x16.device)
    if n:
        with torch.cuda.device(x16.device):
            _lib.call("coati_quant_rows_fp4", ptr(x16), n, E, ptr(codes), ptr(scales), stream())
    return codes, scales


class Fp4Index(FlatTwoStage):
    """The rows of an EmbeddingIndex at the time of build() as e2m1 nibbles and block scales; len() and the rows returned are the
    source's.  Attributes: dim, dim_padded, dim_stored (E4), metric, device, keep_rows."""
    _slices_entry = "coati_search4_slices"
    _payload = {"codes": "_codes", "scales": "_scales"}
    _quantise_rows = staticmethod(quantise_rows)

    def __init__(self, dim, dim_padded, metric, codes, scales, bias, rows16=None, bias16=None, device="cuda:0"):
        _check_metric(metric)
        self.dim, self.dim_padded, self.metric, self.device = int(dim), int(dim_padded), metric, torch.device(device)
        self.dim_stored = stored_width(self.dim_padded)
        self._codes = codes.to(self.device).contiguous()
        self._scales = scales.to(self.device).contiguous()
        self._bias = bias.to(self.device, torch.float32).contiguous()
        self._n = int(self._codes.shape[0])
        if self._codes.dtype != torch.uint8 or self._codes.shape != (self._n, self.dim_stored // 2) or self._scales.dtype != torch.uint8 \
                or self._scales.shape != (self._n, self.dim_stored // BLOCK) or self._bias.shape != (self._n,):
            raise ValueError("Fp4Index: codes, scales and bias do not match")
        self._adopt_rows(rows16, self._bias if bias16 is None else bias16)

    # ---- building ----------------------------------------------------------------------------------------------------------------
    @classmethod
    def build(cls, index, keep_rows=True):
        """index: an EmbeddingIndex.  A snapshot: rows added to the index later are not seen, rows removed from it later are still
        returned (remove() them here too).  keep_rows=True holds a VIEW of the index's bf16 rows for stage 2, no copy;
        keep_rows=False holds codes, scales and bias only -- 140 B a row at width 256 against the index's 520 -- and search() is
        stage 1 alone."""
        stored_width(index.dim_padded)
        x16, bias16 = index.vectors, index.bias.clone()
        if x16.device.type == "cuda":
            codes, scales = quantise_device(x16)
        else:
            codes, scales = quantise_rows(x16)
        bias = stage1_bias(index.metric, codes, scales, bias16)
        return cls(index.dim, index.dim_padded, index.metric, codes, scales, bias, x16 if keep_rows else None, bias16 if keep_rows else None,
                   index.device)

    @property
    def codes(self):
        """the stored nibbles [N, E4 / 2] uint8 (a view): element 2 i in byte i's low nibble"""
        return self._codes

    @property
    def scales(self):
        """the blocks' E8M0 scale bytes [N, E4 / 32] uint8 (a view)"""
        return self._scales

    @property
    def bias(self):
        """stage 1's f32 bias [N] (a view): the index's, -|x_hat|^2 for l2, -inf once removed"""
        return self._bias

    def dequantised(self):
        """f32 [N, E4]: the rows the codes and scales stand for"""
        return dequantise(self._codes, self._scales)

    def bytes_per_row(self):
        """what stage 1 holds per row: E4 / 2 code bytes, E4 / 32 scale bytes and the f32 bias"""
        return self.dim_stored // 2 + self.dim_stored // BLOCK + 4

    # ---- searching (FlatTwoStage) ----------------------------------------------------------------------------------------------------
    def _default_slices(self, qc, kk):
        return _lib.lib().coati_search4_slices(self._n, qc, kk)

    def _stage1_queries(self, q16, rescore):
        E4 = self.dim_stored
        q16w = q16 if E4 == self.dim_padded else torch.nn.functional.pad(q16, (0, E4 - self.dim_padded)).contiguous()
        q8, qscale = _F8.quantise_device(q16w)
        return (q8, qscale), None if rescore else _F8.dequantise(q8, qscale)

    def _stage1_call(self, qs, bias1, lo, n, kk, alpha, S, part_score, part_row, scores, rows, s):
        _lib.call("coati_search4_topk", ptr(self._codes), ptr(self._scales), self._n, self.dim_stored, ptr(bias1), ptr(qs[0][lo:lo + n]),
                  ptr(qs[1][lo:lo + n]), n, kk, alpha, S, ptr(part_score), ptr(part_row), ptr(scores), ptr(rows), s)

    def search(self, queries, k, oversample=8, rescore=None, slices=None, bias=None):
        """(scores [Q, k] f32, rows [Q, k] int64): EmbeddingIndex.search's contract -- the metric's score, descending, row ascending among
        equal scores, (-inf, -1) where fewer rows qualify.  Stage 1 keeps R = min(oversample * k, 128) candidates per query, stage 2
        returns the best k of them by their exact scores.  rescore: default keep_rows; False: stage 1's k best with stage 1's scores (of
        the dequantised operands); True without the bf16 rows raises.  slices: the library slices of stage 1's grid (default:
        coati_search4_slices); the result does not depend on it.  bias: f32 [N], added to every row's score in both stages, -inf
        excluding a row.  oversample=8 is twice Fp8Index's default: four-bit rows rank the exact top k deeper (DESIGN.md section 6,
        "Four-bit search")."""
        return self._search(queries, k, oversample, rescore, slices, bias)

