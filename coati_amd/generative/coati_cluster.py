"""Diverse picks from an embedding library: the best rows under any score are near-duplicates of each other, so a batch is picked as one
best row per cluster of a k-means over the candidates (coati_amd.cluster, EmbeddingIndex.kmeans).  The reference has no counterpart."""
from typing import Optional, Tuple

import torch

from ..cluster import Clustering
from ..search import EmbeddingIndex


def _live(index, rows):
    live = index.bias > float("-inf")
    return live if rows is None else live[rows]


def diverse_subset(index: EmbeddingIndex, n: int, rows=None, scores: Optional[torch.Tensor] = None, iters: int = 20,
                   seed: int = 0) -> Tuple[torch.Tensor, Clustering]:
    """(picks [<= n] int64, clustering): the live rows (or the subset `rows`) clustered into n -- fewer when fewer rows are left -- and one
    row per non-empty cluster, in cluster order: the member with the largest scores[i] (scores aligned with the rows clustered: [N], or
    [len(rows)]; the lowest row among equal scores), or without scores the member nearest its centre."""
    n = int(n)
    if n < 1:
        raise ValueError(f"diverse_subset: n={n} < 1")
    if rows is not None:
        rows = torch.as_tensor(rows, dtype=torch.int64).reshape(-1).to(index.device)
    left = int(_live(index, rows).sum())
    if left == 0:
        raise ValueError("diverse_subset: no live row to pick from")
    clustering = index.kmeans(min(n, left), iters=iters, seed=seed, rows=rows)
    picks = clustering.representatives(scores)
    return picks[picks >= 0], clustering


def diverse_screen(index: EmbeddingIndex, head, n: int, pool: Optional[int] = None, output: int = 0, largest: bool = True,
                   acquisition: Optional[str] = None, beta: float = 1.0, best: Optional[float] = None, iters: int = 20,
                   seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, Clustering]:
    """(scores [<= n] f32, rows [<= n] int64, clustering): EmbeddingIndex.screen's ranking (head, output, largest, acquisition, beta, best
    mean what they mean there; the scores are the head's own values or the acquisition's), made diverse: the `pool` best live rows (torch.topk;
    default 20 n, any size) are clustered into n and every cluster gives its best-ranked row.  Score descending -- ascending for
    largest=False -- and row ascending among equal scores.  clustering.rows is the pool."""
    n, output = int(n), int(output)
    if n < 1:
        raise ValueError(f"diverse_screen: n={n} < 1")
    pool = 20 * n if pool is None else int(pool)
    if pool < n:
        raise ValueError(f"diverse_screen: pool={pool} < n={n}")
    if output < 0 or output >= head.num_outputs:
        raise ValueError(f"diverse_screen: output={output} outside 0 .. {head.num_outputs - 1}")
    if acquisition not in (None, "mean"):
        from ..models.regression.gp_head import ACQUISITIONS, acquisition_values
        if acquisition not in ACQUISITIONS:
            raise ValueError(f"diverse_screen: acquisition={acquisition!r} is not one of {ACQUISITIONS}")
        if acquisition == "ei" and best is None:
            raise ValueError("diverse_screen: acquisition='ei' needs best=, the value to improve on")
        mean, std = index.property_uncertainty(head)
        values = acquisition_values(mean[:, output], std[:, output], acquisition, beta, best).to(torch.float32).contiguous()
    else:
        values = index.property_scores(head)[:, output].contiguous()
    key = torch.where(_live(index, None), values if largest else -values, torch.full_like(values, float("-inf")))
    top = torch.topk(key, min(pool, len(index)))
    cand = top.indices[top.values > float("-inf")]
    picks, clustering = diverse_subset(index, n, rows=cand, scores=key[cand], iters=iters, seed=seed)
    picks = picks.sort().values
    picks = picks[key[picks].sort(descending=True, stable=True).indices]
    return values[picks], picks, clustering
