"""A pure-torch restatement of the IVF search of include/coati_ivf.h, in float64, for the tests, on the conventions of
tests/search_util.py: scores from the STORED bf16 rows and the bf16-rounded queries, per query the exact top k over the union of its
probed lists, score descending, ORIGINAL row ascending among equal scores, rows whose score is -inf never returned, padding (-inf, -1)."""
import torch

from tests import search_util
from tests.search_util import recall  # noqa: F401  (the tests reach it through this module)

NEG_INF = float("-inf")


def inverted(assign, nlist=None):
    """(ids int64 [M], list_off int64 [L + 1]) of an assignment [N] (-1 = left out): the rows sorted by (list, row) -- a stable sort -- and
    the lists' boundaries"""
    assign = torch.as_tensor(assign).long().cpu()
    L = int(assign.max()) + 1 if nlist is None else int(nlist)
    rows = torch.nonzero(assign >= 0).reshape(-1)
    ids = rows[torch.sort(assign[rows], stable=True).indices]
    sizes = torch.bincount(assign[rows], minlength=L)
    return ids, torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)])


def scan(lib16, ids, bias, list_off, q16, probes, k, alpha=1.0):
    """(scores [Q, k] float64, rows [Q, k] int64): lib16 [M, E] the stored rows in list order, ids [M] their original rows, bias [M] or
    None, list_off [L + 1], q16 [Q, E], probes [Q, n] (list, or -1).  A position outside the query's probed lists scores -inf; the
    columns are then put in ORIGINAL row order, so that search_util.topk's stable sort breaks ties by original row."""
    lib16, q16 = lib16.cpu(), q16.cpu()
    ids, list_off, probes = torch.as_tensor(ids).long().cpu(), torch.as_tensor(list_off).long().cpu(), torch.as_tensor(probes).long().cpu()
    M, L = lib16.shape[0], list_off.shape[0] - 1
    s = search_util.score_matrix(lib16, None if bias is None else bias.cpu(), q16, alpha)               # [Q, M]
    list_of = torch.bucketize(torch.arange(M), list_off[1:], right=True)                                # the list of every position
    probed = torch.zeros(q16.shape[0], L + 1, dtype=torch.bool)
    probed.scatter_(1, torch.where(probes < 0, torch.full_like(probes, L), probes), True)
    s = torch.where(probed[:, :L][:, list_of], s, torch.full_like(s, NEG_INF))
    order = torch.argsort(ids, stable=True)                                                             # positions in original-row order
    val, idx = search_util.topk(s[:, order], k)
    return val, torch.where(idx >= 0, ids[order][idx.clamp_min(0)], idx)
