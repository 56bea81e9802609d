"""A pure-torch restatement of the radius search over inverted lists of include/coati_ivf_radius.h, in float64, for the tests:
radius_util.csr_of applied to the score matrix of the STORED operands (the rows in list order, their ids and bias, the bf16-rounded
queries), every (query, row) whose list the query does not probe masked to -inf, the columns put back in ORIGINAL row order.  And the
position -> row permutation of a CSR, restated with plain loops."""
import torch

from tests import radius_util, search_util

NEG_INF = float("-inf")


def list_of_positions(list_off):
    """[M] int64: the list of every stored position"""
    list_off = torch.as_tensor(list_off).long().cpu()
    return torch.bucketize(torch.arange(int(list_off[-1])), list_off[1:], right=True)


def masked_scores(lib16, ids, bias, list_off, q16, probes, n, alpha=1.0, l2=False):
    """[Q, n] float64 over ORIGINAL rows: the metric's score where the row is stored in a list the query probes, else -inf.  lib16
    [M, E] in list order, ids [M], bias [M] or None, list_off [L + 1], q16 [Q, E], probes [Q, w] (list, or -1)."""
    lib16, q16 = lib16.cpu(), q16.cpu()
    ids, list_off, probes = torch.as_tensor(ids).long().cpu(), torch.as_tensor(list_off).long().cpu(), torch.as_tensor(probes).long().cpu()
    L, Q = list_off.shape[0] - 1, q16.shape[0]
    s = search_util.score_matrix(lib16, None if bias is None else bias.cpu(), q16, alpha)               # [Q, M]
    if l2:
        s = (s - (q16.to(torch.float64) ** 2).sum(dim=1, keepdim=True)).clamp_max(0.0)
    probed = torch.zeros(Q, L + 1, dtype=torch.bool)
    probed.scatter_(1, torch.where(probes < 0, torch.full_like(probes, L), probes), True)
    s = torch.where(probed[:, :L][:, list_of_positions(list_off)], s, torch.full_like(s, NEG_INF))
    out = torch.full((Q, n), NEG_INF, dtype=torch.float64)
    out[:, ids] = s
    return out


def csr(lib16, ids, bias, list_off, q16, probes, n, thr, row_below=None, alpha=1.0, l2=False):
    """(offsets [Q + 1], scores float64 [T], rows int64 [T]), row ascending: the oracle of order="row" """
    s = masked_scores(lib16, ids, bias, list_off, q16, probes, n, alpha, l2)
    thr = torch.as_tensor(thr).cpu()
    return radius_util.csr_of(s, thr, None if row_below is None else torch.as_tensor(row_below).cpu())


def in_probe_order(offsets, scores, rows, probes, ids, list_off, n):
    """a row-ascending CSR with every segment put list by list in the query's probe order, row ascending inside a list"""
    ids, probes = torch.as_tensor(ids).long().cpu(), torch.as_tensor(probes).long().cpu()
    list_of_row = torch.full((n,), -1, dtype=torch.int64)
    list_of_row[ids] = list_of_positions(list_off)
    list_of_row = list_of_row.tolist()
    s_out, r_out = [], []
    for i, (a, b) in enumerate(zip(offsets[:-1].tolist(), offsets[1:].tolist())):
        rank = {int(l): j for j, l in enumerate(probes[i].tolist()) if l >= 0}
        key = torch.tensor([rank[list_of_row[r]] for r in rows[a:b].tolist()], dtype=torch.int64)
        order = torch.sort(key, stable=True).indices                                                   # the segment arrives row-ascending
        s_out.append(scores[a:b][order])
        r_out.append(rows[a:b][order])
    return (torch.cat(s_out), torch.cat(r_out)) if s_out else (scores, rows)


def rows_from_positions(offsets, scores, rows, ids, n):
    """a CSR with one segment per stored position as one with a segment per original row 0 .. n - 1: position p's entries, in their
    order, become row ids[p]'s; rows without a position are empty"""
    offsets, scores, rows, ids = [int(v) for v in offsets], list(scores), list(rows), [int(v) for v in ids]
    where = {r: p for p, r in enumerate(ids)}
    out, s_out, r_out = [0], [], []
    for row in range(n):
        if row in where:
            p = where[row]
            s_out += scores[offsets[p]:offsets[p + 1]]
            r_out += rows[offsets[p]:offsets[p + 1]]
        out.append(len(s_out))
    return out, s_out, r_out
