"""Radius search over an IVFIndex (include/coati_ivf_radius.h, csrc/ivf_radius.hip): every row of a query's probed lists within a
threshold, in CSR form, and what is built on it -- counts, the near-duplicate self-join in list order and greedy deduplication.

    offsets, scores, rows = ivf.radius_search(queries, 0.9, nprobe=8)    # EmbeddingIndex.radius_search's contract over the probed lists
    counts = ivf.radius_count(queries, 0.9, nprobe=8)                    # int64 [Q], the count pass alone
    keep = ivf.dedup(0.999, nprobe=8)                                    # bool [len(ivf)]

Per chunk of queries (the count table of a chunk stays within SCRATCH_BYTES): the probe table inverted into (list, query) pairs
(ivf.invert_probes), a count pass into counts [P, segs], the counts gathered into probe order through pair_slot, a prefix sum, ONE
.item() for the total, an allocation, the offsets scattered back to pair order, and a fill pass that computes the scores again and
writes every pair's hits where the offsets say: a query's hits are contiguous, list by list in probe order, row ascending inside a list.
order="row" / "score" then cost one stable torch sort each.  A (query, row) score has the bits EmbeddingIndex.search returns for it, the
rows are original rows, and nothing depends on seg_rows or blocks.  With every non-empty list probed the result IS
EmbeddingIndex.radius_search's.  The IVFIndex methods are thin wrappers.  There is no CPU fallback.  The reference has no counterpart."""
import torch

from . import _lib
from .ivf import invert_probes
from .ops import ptr, stream
from .radius import MAX_RESULTS, greedy_leaders, row_bounds, sort_segments_by_score, thresholds
from .search import SCRATCH_BYTES, metric_alpha, prepare_queries

ORDERS = ("row", "score", "probe")


def _empty(device, Q):
    return (torch.zeros(Q + 1, dtype=torch.int64, device=device), torch.empty(0, dtype=torch.float32, device=device),
            torch.empty(0, dtype=torch.int64, device=device))


def _need_gpu(ivf, what):
    if ivf.device.type != "cuda":
        raise RuntimeError(f"{what}: the index is not on a GPU; there is no CPU fallback")


def _segments(offsets, T):
    """the segment of every entry of a CSR's T values"""
    return torch.repeat_interleave(torch.arange(offsets.numel() - 1, device=offsets.device), offsets[1:] - offsets[:-1], output_size=T)


def sort_segments_by_row(offsets, scores, rows):
    """every CSR segment by row ascending: ONE stable sort on the key (segment, row)"""
    T = rows.numel()
    if T == 0:
        return scores, rows
    order = ((_segments(offsets, T) << 32) | rows).sort(stable=True).indices
    return scores[order], rows[order]


def rows_from_positions(offsets, scores, rows, ids, n):
    """A CSR with one segment per stored position p (offsets [M + 1]) as a CSR with one segment per ORIGINAL row 0 .. n - 1 (offsets
    [n + 1]): position p's segment becomes row ids[p]'s, its entries in the order they have; a row without a position gets an empty
    segment.  Pure torch, any device."""
    ids = ids.long()
    M, T, dev = ids.numel(), scores.numel(), offsets.device
    lens = offsets[1:] - offsets[:-1]
    row_len = torch.zeros(n, dtype=torch.int64, device=dev)
    row_len[ids] = lens
    out = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    out[1:] = row_len.cumsum(0)
    pos = torch.repeat_interleave(torch.arange(M, device=dev), lens, output_size=T)
    dest = out[ids[pos]] + (torch.arange(T, device=dev) - offsets[pos])
    s, r = torch.empty_like(scores), torch.empty_like(rows)
    s[dest], r[dest] = scores, rows
    return out, s, r


def _scan(ivf, q16, thr, row_hi, table, seg_rows, blocks, max_results, what, fill):
    """The two passes over chunks of prepared queries q16 [Q, E] bf16 with thr [Q] f32, row_hi [Q] int32 or None and the probe table
    [Q, nprobe] on the device.  fill: (offsets int64 [Q + 1], scores f32 [T], rows int64 [T]) in probe order; else counts int64 [Q]."""
    Q, nprobe, dev = q16.shape[0], table.shape[1], ivf.device
    l2 = ivf.metric == "l2"
    sub = (q16.float() ** 2).sum(dim=1).contiguous() if l2 else None          # finish_scores' |q|^2, the same reduction
    segs = max(1, -(-ivf._max_rows // seg_rows))
    table32 = table.to(torch.int32).contiguous()
    qc = max(1, min(Q, SCRATCH_BYTES // (nprobe * segs * 4)))
    offsets, scores, rows, counted, base = [torch.zeros(1, dtype=torch.int64, device=dev)], [], [], [], 0
    with torch.cuda.device(dev):
        s = stream()
        for lo in range(0, Q, qc):
            n = min(qc, Q - lo)
            P = n * nprobe
            pair_q, pair_off, item_off, pair_slot = invert_probes(table32[lo:lo + n], ivf._sizes, seg_rows, ivf._tables)
            common = (ptr(ivf._vec), ptr(ivf._ids), ptr(ivf._bias), ptr(ivf._list_off), ivf._m, ivf.dim_padded, ivf.nlist, ptr(q16[lo:lo + n]), n,
                      ptr(pair_q), ptr(pair_off), ptr(item_off), P, metric_alpha(ivf.metric), ptr(sub[lo:lo + n] if l2 else None), int(l2),
                      ptr(thr[lo:lo + n]), ptr(row_hi[lo:lo + n] if row_hi is not None else None), seg_rows, segs)
            # row P of the two tables is where the probe table's -1 entries point: a count of 0 that no kernel touches
            counts = torch.zeros(P + 1, segs, dtype=torch.int32, device=dev)
            _lib.call("coati_ivf_radius_count", *common, ptr(counts), int(blocks), s)
            slot = pair_slot.reshape(-1).long()
            slot = torch.where(slot < 0, P, slot)
            by_probe = counts[slot]                                             # [n * nprobe, segs]: a query's entries are contiguous
            if not fill:
                counted.append(by_probe.view(n, nprobe * segs).sum(dim=1, dtype=torch.int64))
                continue
            incl = by_probe.view(-1).cumsum(0, dtype=torch.int64)
            total = int(incl[-1].item())                                        # the chunk's only synchronisation
            if base + total > max_results:
                more = " so far" if lo + n < Q else ""
                raise ValueError(f"{what}: {base + total} results{more} exceed max_results={max_results}")
            offsets.append(incl.view(n, nprobe * segs)[:, -1] + base)
            sc = torch.empty(total, dtype=torch.float32, device=dev)
            rw = torch.empty(total, dtype=torch.int64, device=dev)
            if total > 0:
                where = torch.zeros(P + 1, segs, dtype=torch.int64, device=dev)
                where[slot] = (incl - by_probe.view(-1)).view(n * nprobe, segs)
                _lib.call("coati_ivf_radius_fill", *common, ptr(counts), ptr(where), ptr(sc), ptr(rw), int(blocks), s)
            scores.append(sc)
            rows.append(rw)
            base += total
    if not fill:
        return torch.cat(counted)
    return torch.cat(offsets), torch.cat(scores), torch.cat(rows)


def _ordered(order, offsets, scores, rows):
    if order == "probe":
        return offsets, scores, rows
    scores, rows = sort_segments_by_row(offsets, scores, rows)
    if order == "score":
        scores, rows = sort_segments_by_score(offsets, scores, rows)
    return offsets, scores, rows


def _seg_rows(ivf, seg_rows, Q, nprobe, what):
    seg_rows = ivf.plan(max(Q, 1), nprobe, 1) if seg_rows is None else int(seg_rows)
    if seg_rows < 64 or seg_rows % 64:
        raise ValueError(f"{what}: seg_rows={seg_rows} is not a positive multiple of 64")
    return seg_rows


def _query_args(ivf, queries, threshold, nprobe, probes, row_below, what):
    """validated arguments -> (q16, thr, row_hi, the caller's table or None, nprobe)"""
    _, q16 = prepare_queries(queries, ivf.metric, ivf.dim, ivf.device)
    Q = q16.shape[0]
    thr = thresholds(threshold, Q, ivf.device, what)
    row_hi = row_bounds(row_below, Q, ivf.device, what)
    table, nprobe = ivf._given_probes(probes, nprobe, Q, what.split(".")[-1])
    return q16, thr, row_hi, table, nprobe


def radius_count(ivf, queries, threshold, nprobe=8, probes=None, row_below=None):
    what = "IVFIndex.radius_count"
    q16, thr, row_hi, table, nprobe = _query_args(ivf, queries, threshold, nprobe, probes, row_below, what)
    Q = q16.shape[0]
    if Q == 0 or ivf._m == 0:
        return torch.zeros(Q, dtype=torch.int64, device=ivf.device)
    _need_gpu(ivf, what)
    if table is None:
        table = ivf._probe16(q16, nprobe)
    return _scan(ivf, q16, thr, row_hi, table, _seg_rows(ivf, None, Q, nprobe, what), 0, None, what, False)


def radius_search(ivf, queries, threshold, nprobe=8, probes=None, order="row", row_below=None, seg_rows=None, max_results=MAX_RESULTS,
                  blocks=0, return_probes=False):
    what = "IVFIndex.radius_search"
    if order not in ORDERS:
        raise ValueError(f"{what}: order {order!r} is not one of {ORDERS}")
    if isinstance(max_results, bool) or not isinstance(max_results, int) or max_results < 0:
        raise ValueError(f"{what}: max_results={max_results!r} is not a non-negative int")
    if isinstance(blocks, bool) or not isinstance(blocks, int) or blocks < 0:
        raise ValueError(f"{what}: blocks={blocks!r} is not a non-negative int")
    q16, thr, row_hi, table, nprobe = _query_args(ivf, queries, threshold, nprobe, probes, row_below, what)
    Q = q16.shape[0]
    seg_rows = _seg_rows(ivf, seg_rows, Q, nprobe, what)
    if Q == 0 or ivf._m == 0:
        out = _empty(ivf.device, Q)
        if table is None:
            table = torch.full((Q, nprobe), -1, dtype=torch.int64, device=ivf.device)
    else:
        _need_gpu(ivf, what)
        if table is None:
            table = ivf._probe16(q16, nprobe)
        out = _ordered(order, *_scan(ivf, q16, thr, row_hi, table, seg_rows, blocks, max_results, what, True))
    return out + (table.long(),) if return_probes else out


def near_duplicates(ivf, threshold, nprobe=8, chunk=4096):
    what = "IVFIndex.near_duplicates"
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"{what}: chunk={chunk} < 1")
    nprobe = ivf._check_nprobe(nprobe)
    dev, n, m = ivf.device, len(ivf), ivf._m
    thr_all = thresholds(threshold, 1, dev, what)[0]
    if n == 0 or m == 0:
        return _empty(dev, n)
    _need_gpu(ivf, what)
    inf = torch.full((), float("inf"), dtype=torch.float32, device=dev)
    ends = ivf._list_off[1:].long()
    offsets, scores, rows, base = [torch.zeros(1, dtype=torch.int64, device=dev)], [], [], 0
    for lo in range(0, m, chunk):
        hi = min(m, lo + chunk)
        q16 = ivf._vec[lo:hi]                                                   # the stored bits themselves, not re-prepared
        thr = torch.where(ivf._bias[lo:hi] > float("-inf"), thr_all, inf).contiguous()
        # a position's own list is always probed: where the coarse step did not name it, it takes the last entry's place
        table = ivf._probe16(q16, nprobe)
        own = torch.bucketize(torch.arange(lo, hi, device=dev), ends, right=True)
        named = (table == own[:, None]).any(dim=1)
        table[:, -1] = torch.where(named, table[:, -1], own)
        seg_rows = _seg_rows(ivf, None, hi - lo, nprobe, what)
        o, s, r = _ordered("row", *_scan(ivf, q16, thr, ivf._ids[lo:hi], table, seg_rows, 0, MAX_RESULTS, what, True))
        offsets.append(o[1:] + base)
        scores.append(s)
        rows.append(r)
        base += s.numel()
    return rows_from_positions(torch.cat(offsets), torch.cat(scores), torch.cat(rows), ivf._ids, n)


def dedup(ivf, threshold, nprobe=8):
    offsets, _, rows = near_duplicates(ivf, threshold, nprobe)
    live = torch.zeros(len(ivf), dtype=torch.bool, device=ivf.device)
    live[ivf._ids.long()] = ivf._bias > float("-inf")
    return greedy_leaders(offsets, rows, live).to(ivf.device)
