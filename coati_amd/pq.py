"""Product-quantised search over an embedding library: every row as one code byte per 8 dimensions, 16 times fewer bytes than the bf16
row, and a two-stage search on top of the codes (include/coati_pq.h, csrc/pq.hip).

    pq = index.pq()                                      # a snapshot of an EmbeddingIndex's rows; keep_rows=False: codes and bias only
    scores, rows = pq.search(queries, k=10)              # EmbeddingIndex.search's contract

    pq = PQIndex.fit(sample_vectors, 256, "cosine")      # an empty index with code books trained on a sample ...
    pq.add(chunk)                                        # ... for a library that never exists in bf16: encode and append

Stage 1 streams the code bytes with the code books in LDS (coati_pq_topk: the exact search's kernel with the operand read from the
code book) and keeps the R = min(oversample * k, coati_pq_k_max(E)) best per query; stage 2 (coati_search_rescore, unchanged) scores
those R rows again from the bf16 rows with the exact search's arithmetic and returns the best k.  When every row of the exact top k is
among the R candidates the result IS EmbeddingIndex.search's, bit for bit; otherwise every returned score is still the exact score of
its row.  Without the bf16 rows (keep_rows=False, an index filled by add(), or rescore=False) the result is stage 1's: the metric's score
of the query against the RECONSTRUCTED rows, with the bits coati_search_topk gives on them.

Storage (fixed, so that it can be tested byte for byte): M = dim_padded / 8 sub-spaces, code books [M, 256, 8] bf16, codes [N, M] uint8;
codes[n][m] names the entry with the smallest squared distance to dimensions 8 m .. 8 m + 7 of the stored bf16 row (encode_rows: f32,
every operation rounded on its own, ascending dimension order, the lowest index among equal distances).  Stage 1's bias is 0 for "dot"
and "cosine"; for "l2" it is -|x_hat|^2 of the reconstructed row (summed in float64, stored as f32), so that its score is the negated
squared distance to the reconstructed row; -inf once removed.

There is no CPU fallback for search().  Codes of the rows' residuals inside inverted lists (IVF-PQ) are coati_amd.ivfpq.IvfPqIndex, built
on encode_rows / encode_device, fit_codebooks and reconstruct below.  Out of scope: rotated PQ, sub-vectors other than 8
dimensions or code counts other than 256, dim_padded > 256, radius search, clustering or property heads over codes, several GPUs,
re-scoring from rows in host memory, add() on a snapshot that holds a view of another index's rows.  The reference has no counterpart."""
import torch

from . import _lib
from .ops import ptr, stream
from .search import MIN_CAPACITY, padded_dim, prepare_rows, _check_metric
from .two_stage import FlatTwoStage

SUB = 8                          # dimensions per sub-space
CODES = 256                      # entries per code book
DIM_MAX = 256                    # the code books of a wider row do not fit a CU's LDS
_BIAS_CHUNK = 1 << 18            # the rows reconstructed at a time for the l2 bias
_CHUNK_ELEMS = 1 << 24           # the [rows, M, 256] f32 distances of one chunk of encode_rows


def _check_codebooks(codebooks, E=None):
    if not isinstance(codebooks, torch.Tensor) or codebooks.dtype != torch.bfloat16 or codebooks.dim() != 3 \
            or tuple(codebooks.shape[1:]) != (CODES, SUB) or (E is not None and codebooks.shape[0] * SUB != E):
        want = "M" if E is None else E // SUB
        raise ValueError(f"pq: code books must be bf16 [{want}, {CODES}, {SUB}], got "
                         f"{getattr(codebooks, 'dtype', type(codebooks))} {tuple(getattr(codebooks, 'shape', ()))}")


def k_max(E):
    """coati_pq_k_max(E): the largest k of stage 1 at this stored width"""
    lib = _lib.lib()
    km = lib.coati_pq_k_max(int(E))
    if km < 1:
        raise ValueError(f"coati_pq_k_max({E}) = {km}: {lib.coati_last_error().decode('utf-8', 'replace')}")
    return km


def _distances(x, cb):
    """[n, M, 256] f32 of x [n, M, 8] f32 and cb [M, 256, 8] f32: d = ((p0 + p1) + p2) + ... + p7, p_j = t_j * t_j, t_j = x_j - c_j, every
    operation a torch operation of its own (rounded to f32, nothing fused)"""
    d = None
    for j in range(SUB):
        t = x[:, :, None, j] - cb[None, :, :, j]
        p = t * t
        d = p if d is None else d + p
    return d


def _nearest(x, cb):
    """int64 [n, M]: per row and sub-space the entry of smallest _distances, the lowest index among equal ones; in chunks of rows"""
    n, M = x.shape[0], x.shape[1]
    out = torch.empty(n, M, dtype=torch.int64, device=x.device)
    step = max(1, _CHUNK_ELEMS // (M * CODES))
    idx = torch.arange(CODES, device=x.device)
    for lo in range(0, n, step):
        d = _distances(x[lo:lo + step], cb)
        out[lo:lo + step] = torch.where(d == d.amin(dim=2, keepdim=True), idx, CODES).amin(dim=2)
    return out


def encode_rows(x16, codebooks):
    """codes [n, M] uint8 of bf16 rows [n, E] under code books [M, 256, 8] bf16: the storage rule in plain torch, on the rows' device --
    what coati_pq_encode computes, byte for byte"""
    _check_codebooks(codebooks, x16.shape[1])
    M = codebooks.shape[0]
    return _nearest(x16.to(torch.float32).reshape(-1, M, SUB), codebooks.to(x16.device, torch.float32)).to(torch.uint8)


def encode_device(x16, codebooks):
    """encode_rows by the kernel (coati_pq_encode); x16 bf16 [n, E] contiguous on a GPU, the code books on the same device"""
    _check_codebooks(codebooks, x16.shape[1])
    n, E = x16.shape
    out = torch.empty(n, E // SUB, dtype=torch.uint8, device=x16.device)
    if n:
        x16, codebooks = x16.contiguous(), codebooks.to(x16.device).contiguous()
        with torch.cuda.device(x16.device):
            _lib.call("coati_pq_encode", ptr(x16), n, E, ptr(codebooks), ptr(out), stream())
    return out


def reconstruct(codes, codebooks):
    """bf16 [n, E]: the rows the codes stand for, the concatenation of their entries"""
    _check_codebooks(codebooks, codes.shape[1] * SUB)
    M = codebooks.shape[0]
    cb = codebooks.to(codes.device)
    return cb[torch.arange(M, device=codes.device)[None, :], codes.to(torch.int64)].reshape(codes.shape[0], M * SUB)


def _draw(n, sample, gen):
    """int64 [min(n, sample)]: distinct rows of 0 .. n - 1 in a seeded random order.  Up to 64 * sample rows a permutation of them all
    (at most 32 MB on the host at the default sample); beyond that, distinct values among seeded draws, so that a library of 10^9 rows does
    not cost a permutation of 10^9 indices for the 65536 it keeps"""
    if n <= 64 * sample:
        return torch.randperm(n, generator=gen)[:sample]
    picked = torch.unique(torch.randint(0, n, (2 * sample,), generator=gen))
    while picked.numel() < sample:                                                     # (n > 64 * sample: a repeat among 2 * sample draws is rare)
        picked = torch.unique(torch.cat([picked, torch.randint(0, n, (sample,), generator=gen)]))
    return picked[torch.randperm(picked.numel(), generator=gen)[:sample]]


def fit_codebooks(x16, seed=0, iters=20, sample=65536):
    """bf16 [M, 256, 8]: Lloyd's k-means per sub-space of the bf16 rows x16 [n, E], in torch f32 on the rows' device, over at most `sample`
    rows drawn with a CPU generator from `seed`.  The centres start at 256 drawn rows (fewer rows: the remaining entries repeat entry 0
    and are never chosen, the lowest index winning); a round assigns by encode_rows' rule and an empty cluster keeps its centre.  The
    cluster sums are differences of a float64 running sum over the rows sorted by cluster -- no atomics -- so the same seed on the same
    device gives the same bytes."""
    n, E = x16.shape
    if E % SUB or n < 1:
        raise ValueError(f"fit_codebooks: rows must be [n >= 1, a multiple of {SUB}], got {tuple(x16.shape)}")
    M, dev = E // SUB, x16.device
    gen = torch.Generator().manual_seed(int(seed))
    x = x16[_draw(n, int(sample), gen).to(dev)].to(torch.float32).reshape(-1, M, SUB)          # [n', M, 8]; its first 256 rows start the centres
    n = x.shape[0]
    cb = x[:CODES].permute(1, 0, 2).contiguous()                                       # [<= 256, M, 8] -> [M, <= 256, 8]
    live = cb.shape[1]
    if live < CODES:
        cb = torch.cat([cb, cb[:, :1].expand(M, CODES - live, SUB)], dim=1)
    edges = torch.arange(CODES + 1, device=dev)[None, :].expand(M, CODES + 1).contiguous()
    for _ in range(int(iters)):
        assign = _nearest(x, cb).T.contiguous()                                        # [M, n]
        sa, order = torch.sort(assign, dim=1, stable=True)
        xs = x.permute(1, 0, 2).gather(1, order[:, :, None].expand(M, n, SUB)).to(torch.float64)
        run = torch.cat([torch.zeros(M, 1, SUB, dtype=torch.float64, device=dev), xs.cumsum(dim=1)], dim=1)      # [M, n + 1, 8]
        b = torch.searchsorted(sa, edges)                                              # [M, 257]: cluster c is sorted rows b[c] .. b[c + 1] - 1
        sums = run.gather(1, b[:, 1:, None].expand(M, CODES, SUB)) - run.gather(1, b[:, :-1, None].expand(M, CODES, SUB))
        counts = (b[:, 1:] - b[:, :-1])[:, :, None]
        cb = torch.where(counts > 0, (sums / counts.clamp_min(1)).to(torch.float32), cb)
    if live < CODES:
        cb[:, live:] = cb[:, :1]
    return cb.to(torch.bfloat16).contiguous()


def stage1_bias(metric, codes, codebooks, bias16):
    """stage 1's bias of rows with these codes and the bf16 rows' bias bias16 (0, or -inf once removed; its l2 term is not used): bias16
    itself, for "l2" -|x_hat|^2 of the reconstructed row (summed in float64, stored f32) where bias16 is above -inf"""
    if metric != "l2":
        return bias16
    out = torch.empty_like(bias16)
    for lo in range(0, codes.shape[0], _BIAS_CHUNK):                                   # (the float64 rows of one chunk: 512 MB at E = 256)
        norm = -(reconstruct(codes[lo:lo + _BIAS_CHUNK], codebooks).double() ** 2).sum(dim=1).float()
        out[lo:lo + _BIAS_CHUNK] = torch.where(bias16[lo:lo + _BIAS_CHUNK] > float("-inf"), norm, bias16[lo:lo + _BIAS_CHUNK])
    return out


class PQIndex(FlatTwoStage):
    """Rows as PQ codes under fixed code books.  Starts empty; add() encodes and appends.  Attributes: dim, dim_padded, metric, device,
    keep_rows (bf16 rows for stage 2 are held: only a snapshot made by build(..., keep_rows=True), or loaded from the file of one, has them)."""
    _slices_entry = "coati_pq_slices"
    _rows_hint = "a snapshot built with keep_rows=True"

    def __init__(self, dim, metric="cosine", codebooks=None, device="cuda:0"):
        _check_metric(metric)
        self.dim, self.dim_padded = int(dim), padded_dim(int(dim))
        if self.dim_padded > DIM_MAX:
            raise ValueError(f"PQIndex: dim={dim} is stored {self.dim_padded} wide, above {DIM_MAX}")
        _check_codebooks(codebooks, self.dim_padded)
        self.metric, self.device = metric, torch.device(device)
        self._cb = codebooks.to(self.device).contiguous()
        self._m = self.dim_padded // SUB
        self._n = 0
        self._codes = self._bias = None                # [capacity, M] uint8, [capacity] f32
        self._adopt_rows(None, None)                   # (a snapshot adopts a view of the source's bf16 rows, and its own copy of their bias)

    # ---- building ----------------------------------------------------------------------------------------------------------------
    @classmethod
    def fit(cls, sample_vectors, dim, metric="cosine", device="cuda:0", seed=0, iters=20, sample=65536):
        """an empty index whose code books are fit_codebooks of sample_vectors [n, dim] as the index stores rows (prepare_rows)"""
        _, x16, _ = prepare_rows(sample_vectors, metric, int(dim), torch.device(device))
        return cls(dim, metric, fit_codebooks(x16, seed=seed, iters=iters, sample=sample), device)

    @classmethod
    def build(cls, index, keep_rows=True, seed=0, iters=20, sample=65536, codebooks=None):
        """index: an EmbeddingIndex.  A snapshot of its rows as codes under code books fitted on them (or `codebooks`): rows added to the
        index later are not seen, rows removed from it later are still returned (remove() them here too).  keep_rows=True holds a VIEW of
        the index's bf16 rows for stage 2, no copy, and refuses add(); keep_rows=False holds codes and bias only and search() is stage 1
        alone."""
        x16, bias16 = index.vectors, index.bias.clone()
        if codebooks is None:
            if x16.shape[0] == 0:
                raise ValueError("PQIndex.build: no rows to fit code books on; pass codebooks=")
            codebooks = fit_codebooks(x16, seed=seed, iters=iters, sample=sample)
        pq = cls(index.dim, index.metric, codebooks, index.device)
        gone = bias16 == float("-inf")
        pq._append(x16, torch.where(gone, bias16, torch.zeros_like(bias16)))
        if keep_rows:
            pq._adopt_rows(x16, bias16)
        return pq

    def _reserve(self, n):
        cap = 0 if self._codes is None else self._codes.shape[0]
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

        self._codes = grown(self._codes, (new, self._m), torch.uint8)
        self._bias = grown(self._bias, (new,), torch.float32)

    def _append(self, x16, alive_bias):
        """encodes stored bf16 rows and appends them; alive_bias [n]: 0, or -inf for a row that is already removed"""
        n = x16.shape[0]
        if self._n + n >= 2 ** 31:
            raise ValueError("PQIndex: more than 2^31 - 1 rows")
        lo, hi = self._n, self._n + n
        if n:
            codes = encode_device(x16, self._cb) if self.device.type == "cuda" else encode_rows(x16, self._cb)
            self._reserve(hi)
            self._codes[lo:hi], self._bias[lo:hi] = codes, stage1_bias(self.metric, codes, self._cb, alive_bias)
        self._n = hi
        return range(lo, hi)

    def add(self, vectors):
        """appends the rows of vectors [n, dim] (any float dtype, any device) -- prepared as an EmbeddingIndex prepares them, encoded,
        never stored in bf16 -- and returns their row indices"""
        if self.keep_rows:
            raise RuntimeError("PQIndex.add: this index is a snapshot with bf16 rows kept for the second stage (a view of another index's "
                               "rows, or the rows it was saved with); "
                               "rows added here would have none.  Add to the source index and build again, or build with keep_rows=False")
        _, x16, _ = prepare_rows(vectors, self.metric, self.dim, self.device)
        return self._append(x16.contiguous(), torch.zeros(x16.shape[0], dtype=torch.float32, device=self.device))

    @property
    def codes(self):
        """the stored code bytes [N, dim_padded / 8] uint8 (a view)"""
        return torch.empty(0, self._m, dtype=torch.uint8, device=self.device) if self._codes is None else self._codes[:self._n]

    @property
    def codebooks(self):
        """the code books [dim_padded / 8, 256, 8] bf16"""
        return self._cb

    @property
    def bias(self):
        """stage 1's f32 bias [N] (a view): 0, -|x_hat|^2 for l2, -inf once removed"""
        return torch.empty(0, dtype=torch.float32, device=self.device) if self._bias is None else self._bias[:self._n]

    def dequantised(self):
        """bf16 [N, dim_padded]: the rows the codes stand for"""
        return reconstruct(self.codes, self._cb)

    def bytes_per_row(self):
        """what stage 1 holds per row: the code bytes and the f32 bias"""
        return self._m + 4

    # ---- searching (FlatTwoStage) ----------------------------------------------------------------------------------------------------
    def _default_slices(self, qc, kk):
        return _lib.lib().coati_pq_slices(self._n, self.dim_padded, qc, kk)

    def _stage1_queries(self, q16, rescore):
        return q16, q16

    def _stage1_call(self, q16, bias1, lo, n, kk, alpha, S, part_score, part_row, scores, rows, s):
        _lib.call("coati_pq_topk", ptr(self._codes), self._n, self.dim_padded, ptr(self._cb), ptr(bias1), ptr(q16[lo:lo + n]), n, kk, alpha, S,
                  ptr(part_score), ptr(part_row), ptr(scores), ptr(rows), s)

    def search(self, queries, k, oversample=4, rescore=None, slices=None, bias=None):
        """(scores [Q, k] f32, rows [Q, k] int64): EmbeddingIndex.search's contract -- the metric's score, descending, row ascending among
        equal scores, (-inf, -1) where fewer rows qualify.  Stage 1 keeps R = min(oversample * k, coati_pq_k_max(dim_padded)) candidates
        per query, stage 2 returns the best k of them by their exact scores.  rescore: default keep_rows; False: stage 1's k best with
        stage 1's scores (of the reconstructed rows); True without the bf16 rows raises.  slices: the library slices of stage 1's grid
        (default: coati_pq_slices); the result does not depend on it.  bias: f32 [N], added to every row's score in both stages, -inf
        excluding a row.  oversample=4 is Fp8Index's default, kept: see DESIGN.md section 6 for what was and was not measured."""
        return self._search(queries, k, oversample, rescore, slices, bias, k_max(self.dim_padded),
                            f", the limit of coati_pq_k_max({self.dim_padded})")

    # ---- persistence ---------------------------------------------------------------------------------------------------------------
    def save(self, path):
        """code books, codes and bias; with the bf16 rows kept, those and their bias too"""
        d = {"dim": self.dim, "metric": self.metric, "codebooks": self._cb.cpu(), "codes": self.codes.cpu(), "bias": self.bias.cpu()}
        if self.keep_rows:
            d.update(rows16=self._rows16.cpu(), bias16=self._bias16.cpu())
        torch.save(d, path)

    @classmethod
    def load(cls, path, device="cuda:0"):
        d = torch.load(path, map_location="cpu")
        pq = cls(d["dim"], d["metric"], d["codebooks"], device)
        n = d["codes"].shape[0]
        if tuple(d["codes"].shape) != (n, pq._m) or d["codes"].dtype != torch.uint8 or tuple(d["bias"].shape) != (n,):
            raise ValueError("PQIndex.load: codes and bias do not match the code books")
        pq._reserve(n)
        if n:
            pq._codes[:n], pq._bias[:n] = d["codes"].to(pq.device), d["bias"].to(pq.device, torch.float32)
        pq._n = n
        if "rows16" in d:
            pq._adopt_rows(d["rows16"].to(pq.device), d["bias16"])
        return pq
