"""What the two-stage indices share: a compressed first stage keeps R = min(oversample * k, the stage's largest k, 128) candidates per
query, the second stage (coati_search_rescore) scores those R rows again from kept bf16 rows with the exact search's arithmetic and
returns the best k.

    TwoStage       the kept rows (rows16, bias16), the policy (k, oversample, rescore) -> (k, R, rescore), the stages' tail
    FlatTwoStage   the search over all rows of Fp8Index, Fp4Index and PQIndex: a class says how it prepares the queries for stage 1
                   (_stage1_queries) and which C entry scores a chunk of them (_stage1_call)
    ListTwoStage   the search over probed lists of Ivf8Index and IvfPqIndex: _stage1_queries and the scan call (_scan)

The sliced top-k driver, its plan and the range check of remove() are coati_amd.search's (sliced_topk, plan_chunks, check_rows)."""
import torch

from . import _lib
from .ivf import ListIndex
from .ops import ptr, stream
from .search import K_MAX, MERGE_MAX, check_bias, check_rows, finish_scores, metric_alpha, plan_chunks, prepare_queries, sliced_topk

R_MAX = 128                      # the candidates of stage 2: one workgroup ranks them in LDS


def rescore_candidates(rows16, bias, q16, cand, k, alpha=1.0):
    """Stage 2 alone (coati_search_rescore): (scores [Q, k] f32, rows [Q, k] int64), the best k of every query's candidates cand [Q, R]
    int64 (R <= 128, distinct rows of rows16 [N, E] bf16, -1 = none) by alpha * dot(q16, row) + bias[row] with coati_search_topk's bits:
    score descending, row ascending, (-inf, -1) padding; a candidate whose bias is -inf is not a result."""
    k = int(k)
    if k < 1 or k > K_MAX:
        raise ValueError(f"rescore_candidates: k={k} outside 1 .. {K_MAX}")
    if cand.dim() != 2 or cand.dtype != torch.int64 or cand.shape[0] != q16.shape[0] or not 1 <= cand.shape[1] <= R_MAX:
        raise ValueError(f"rescore_candidates: cand must be int64 [{q16.shape[0]}, 1 .. {R_MAX}], got {cand.dtype} {tuple(cand.shape)}")
    if rows16.device.type != "cuda":
        raise RuntimeError("rescore_candidates: the rows are not on a GPU; there is no CPU fallback")
    Q, R = cand.shape
    scores = torch.full((Q, k), float("-inf"), dtype=torch.float32, device=rows16.device)
    rows = torch.full((Q, k), -1, dtype=torch.int64, device=rows16.device)
    if Q and rows16.shape[0]:
        cand, q16 = cand.contiguous(), q16.contiguous()
        with torch.cuda.device(rows16.device):
            _lib.call("coati_search_rescore", ptr(rows16), rows16.shape[0], rows16.shape[1], ptr(bias), ptr(q16), Q, ptr(cand), R, k,
                      float(alpha), ptr(scores), ptr(rows), stream())
    return scores, rows


class TwoStage:
    """Mixin of the five two-stage indices.  The class has dim_padded, metric, device, _n (original rows) and _bias (stage 1's)."""
    _rows_hint = "keep_rows=True"                  # how this class comes to hold bf16 rows, for the error of rescore=True without them

    def _adopt_rows(self, rows16, bias16):
        """keep_rows, _rows16, _bias16 from the bf16 rows [N, dim_padded] (None: stage 1 alone) and their bias [N], by original row"""
        name = type(self).__name__
        self.keep_rows = rows16 is not None
        self._rows16 = self._bias16 = None
        if not self.keep_rows:
            return
        if bias16 is None:
            raise ValueError(f"{name}: the bf16 rows need their bias")
        self._rows16 = rows16 if rows16.device == self.device else rows16.to(self.device)      # (a view of the source's rows stays one)
        self._bias16 = bias16.to(self.device, torch.float32).contiguous()
        if self._rows16.dtype != torch.bfloat16 or self._rows16.shape != (self._n, self.dim_padded) or self._bias16.shape != (self._n,) \
                or not self._rows16.is_contiguous():
            raise ValueError(f"{name}: the bf16 rows do not match the index")

    def _policy(self, k, oversample, rescore, k_max=K_MAX, limit=""):
        """(k, kk, rescore) of a search's arguments: kk entries per list in stage 1, R with the second stage and k without; k_max:
        stage 1's largest k, `limit` naming where it comes from"""
        name, k, oversample = type(self).__name__, int(k), int(oversample)
        if k < 1 or k > k_max:
            raise ValueError(f"{name}.search: k={k} outside 1 .. {k_max}{limit}")
        if oversample < 1:
            raise ValueError(f"{name}.search: oversample={oversample} < 1")
        rescore = self.keep_rows if rescore is None else bool(rescore)
        if rescore and not self.keep_rows:
            raise ValueError(f"{name}.search: rescore=True needs the bf16 rows ({self._rows_hint})")
        return k, min(oversample * k, k_max, R_MAX) if rescore else k, rescore

    def _extra_bias(self, bias):
        """a search's bias argument, checked, on the device (or None)"""
        check_bias(f"{type(self).__name__}.search", bias, self._n)
        return None if bias is None else bias.to(self.device)

    def _stage2(self, scores, rows, q16, q_stage1, k, rescore, extra, alpha):
        """the finished (scores [Q, k], rows [Q, k]) from stage 1's [Q, kk]: stage 1's own (the metric's score against q_stage1, the
        queries as stage 1 saw them), or the best k of the kk by their exact scores from the bf16 rows"""
        if not rescore:
            return finish_scores(scores, self.metric, q_stage1), rows
        bias2 = self._bias16 if extra is None else self._bias16 + extra
        scores, rows = rescore_candidates(self._rows16, bias2, q16, rows, k, alpha)
        return finish_scores(scores, self.metric, q16), rows

    def _mark_removed(self, rows, pos=None):
        """-inf in both biases: stage 1's at the rows' stored positions (default: the rows themselves), stage 2's at the rows"""
        self._bias[rows if pos is None else pos] = float("-inf")
        if self.keep_rows:
            self._bias16[rows] = float("-inf")


class FlatTwoStage(TwoStage):
    """Fp8Index, Fp4Index, PQIndex.  A class sets _slices_entry and defines
        _default_slices(qc, kk)         the entry's default S
        _stage1_queries(q16, rescore)   (what _stage1_call gets as qs, the queries finish_scores is to see without the second stage)
        _stage1_call(qs, bias1, lo, n, kk, alpha, S, part_score, part_row, scores, rows, stream)   the C entry on queries lo .. lo + n - 1
    and a search() that fixes its defaults and its docstring."""
    _scratch = None                  # the partial lists, kept between searches

    def __len__(self):
        return self._n

    def remove(self, rows):
        """the rows are never returned again; len() and the other rows' indices do not change"""
        rows = check_rows(f"{type(self).__name__}.remove", rows, self._n)
        if rows.numel():
            self._mark_removed(rows.to(self.device))

    def _plan(self, Q, kk, slices):
        """(queries per call, slices) of stage 1: plan_chunks with the entry's default"""
        return plan_chunks(self._slices_entry, self._default_slices, Q, kk, slices)

    def _search(self, queries, k, oversample, rescore, slices, bias, k_max=K_MAX, limit=""):
        name = type(self).__name__
        k, kk, rescore = self._policy(k, oversample, rescore, k_max, limit)
        if slices is not None and (int(slices) < 1 or int(slices) * kk > MERGE_MAX):
            raise ValueError(f"{name}.search: slices={slices} outside 1 .. {MERGE_MAX // kk} at {kk} candidates")
        extra = self._extra_bias(bias)
        _, q16 = prepare_queries(queries, self.metric, self.dim, self.device)
        Q, alpha = q16.shape[0], metric_alpha(self.metric)
        qs = None
        if Q and self._n and self.device.type == "cuda":                              # (else the driver pads, or raises)
            qs, q_stage1 = self._stage1_queries(q16, rescore)
            bias1 = (self.bias if extra is None else self.bias + extra).contiguous()

        def call(lo, n, S, part_score, part_row, scores, rows, s):
            self._stage1_call(qs, bias1, lo, n, kk, alpha, S, part_score, part_row, scores, rows, s)

        scores, rows = sliced_topk(self, f"{name}.search", Q, kk, slices, call)
        if qs is None:
            return scores[:, :k], rows[:, :k]
        return self._stage2(scores, rows, q16, q_stage1, k, rescore, extra, alpha)

    # ---- persistence of Fp8Index and Fp4Index: _payload = {file key: attribute} of the two stored tensors, in the constructor's order;
    # _quantise_rows makes the two from bf16 rows ------------------------------------------------------------------------------------
    def save(self, path):
        """With the bf16 rows kept they are what is saved (load() quantises them again: the same bytes), else the stored bytes and scales."""
        d = {"dim": self.dim, "dim_padded": self.dim_padded, "metric": self.metric, "bias": self._bias.cpu()}
        if self.keep_rows:
            d.update(rows16=self._rows16.cpu(), bias16=self._bias16.cpu())
        else:
            d.update({key: getattr(self, attr).cpu() for key, attr in self._payload.items()})
        torch.save(d, path)

    @classmethod
    def load(cls, path, device="cuda:0"):
        """the index save() wrote, on `device`"""
        d = torch.load(path, map_location="cpu")
        if "rows16" in d:
            return cls(d["dim"], d["dim_padded"], d["metric"], *cls._quantise_rows(d["rows16"]), d["bias"], d["rows16"].to(device), d["bias16"],
                       device)
        return cls(d["dim"], d["dim_padded"], d["metric"], *(d[key] for key in cls._payload), d["bias"], None, None, device)


class ListTwoStage(ListIndex, TwoStage):
    """Ivf8Index, IvfPqIndex.  A class defines
        _stage1_queries(q16, rescore)   as FlatTwoStage's
        _scan(qs, pos_bias, kk, alpha, blocks)   the scan callable ListIndex._scan_merge takes
    and a search() that fixes its defaults and its docstring."""

    def remove(self, rows):
        """the rows (original indices) are never returned again by either stage; len() and the other rows' indices do not change"""
        self._mark_removed(*self._positions(rows))

    def _search(self, queries, k, nprobe, oversample, rescore, probes, seg_rows, bias, return_probes, blocks, k_max=K_MAX, limit=""):
        k, kk, rescore = self._policy(k, oversample, rescore, k_max, limit)
        extra = self._extra_bias(bias)
        q16, table, nprobe, seg_rows, segs = self._search_args(queries, kk, nprobe, probes, seg_rows)
        Q, alpha = q16.shape[0], metric_alpha(self.metric)
        pos_bias = self._bias if extra is None else (self._bias + extra[self._ids.long()]).contiguous()
        qs = None
        if Q and self._m and self.device.type == "cuda":                              # (else _scan_merge pads, or raises)
            qs, q_stage1 = self._stage1_queries(q16, rescore)
        scores, rows = self._scan_merge(self._scan(qs, pos_bias, kk, alpha, blocks), Q, table, nprobe, kk, seg_rows, segs)
        if qs is None:
            scores, rows = scores[:, :k], rows[:, :k]
        else:
            scores, rows = self._stage2(scores, rows, q16, q_stage1, k, rescore, extra, alpha)
        return (scores, rows, table.long()) if return_probes else (scores, rows)
