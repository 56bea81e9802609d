"""Embedding maps: exact t-SNE of a library of embeddings in two dimensions (include/coati_tsne.h, csrc/tsne.hip).

    result = index.tsne(perplexity=30.0)             # an EmbeddingIndex (coati_amd.search), "cosine" or "l2"
    result.y                                          # [len(index), 2] f32 by row, NaN for removed rows
    result.kl, result.kl_trace                        # the last KL(P | Q), and [(iteration, KL)] every kl_every iterations

The reference draws its pictures with sklearn.manifold.TSNE(n_components=2, learning_rate=100, init="random") (coati/generative/
embed_altair.py).  This is the same exact method -- sklearn's gradient and its gains / momentum descent, with no Barnes-Hut tree and no
interpolation grid -- with P held on a kNN graph: knn_graph() asks the index for every row's neighbours, coati_tsne_affinities turns their
distances into conditional probabilities of the given perplexity, joint() symmetrises them in torch, and an iteration is
coati_tsne_repulsion (all pairs, O(N^2)), a float64 torch sum for Z that stays on the device, and coati_tsne_step (attraction over the CSR
rows, gradient and update in one launch).  No kernel uses an atomic and none depends on its launch geometry, and the start is drawn on the
CPU, so a seed gives the same map bit for bit on every run.  What sklearn's loop has and this one does not: its early stop on
n_iter_without_progress / min_grad_norm (every run takes `iters` iterations).  There is no CPU fallback: off a GPU these raise
RuntimeError, like EmbeddingIndex.search."""
from collections import namedtuple

import torch

from . import _lib
from .ops import ptr, stream

K_MAX = 127                      # neighbours per row: the search returns at most 128, one of them the row itself
AFFINITY_K_MAX = 128             # coati_tsne_affinities: two entries per lane
TSNE_METRICS = ("cosine", "l2")
PART_BYTES_MAX = 256 << 20       # the repulsion's workspace is offered up to this size (N <= ~150 k); past it the tiles fill the device anyway

TSNEResult = namedtuple("TSNEResult", "y kl kl_trace")


def _need_gpu(t, what):
    if t.device.type != "cuda":
        raise RuntimeError(f"{what}: the operands are not on a GPU; there is no CPU fallback")


def chunk_points():
    """J of coati_tsne_repulsion: the points of one chunk of its sums"""
    return int(_lib.lib().coati_tsne_chunk())


def knn_graph(index, k, chunk=4096):
    """(rows int64 [n], nbr int32 [n, k], d2 f32 [n, k]) over the n live rows of an EmbeddingIndex: every live row's k nearest other live
    rows, nearest first, as POSITIONS in `rows`, and the squared distances to them -- "cosine": max(0, 2 - 2 s), the squared chord of unit
    rows; "l2": max(0, -s); "dot" has no distance and raises ValueError.  The stored bf16 rows are the queries, `chunk` at a time, for
    k + 1 neighbours; the row itself is dropped from its list, or the last entry when it is not among them (more than k duplicates).
    Fewer than k other live rows: the tail is (-1, 0).  1 <= k <= 127."""
    from .search import finish_scores
    if index.metric not in TSNE_METRICS:
        raise ValueError(f"knn_graph: metric {index.metric!r} is not one of {TSNE_METRICS} (a dot product is no distance)")
    k, chunk = int(k), int(chunk)
    if not 1 <= k <= K_MAX:
        raise ValueError(f"knn_graph: k={k} outside 1 .. {K_MAX}")
    if chunk < 1:
        raise ValueError(f"knn_graph: chunk={chunk} < 1")
    if index.device.type != "cuda":
        raise RuntimeError("knn_graph: the index is not on a GPU; there is no CPU fallback")
    dev = index.device
    rows = torch.nonzero(index.bias > float("-inf")).reshape(-1)
    n = rows.shape[0]
    nbr = torch.full((n, k), -1, dtype=torch.int32, device=dev)
    d2 = torch.zeros(n, k, dtype=torch.float32, device=dev)
    if n == 0:
        return rows, nbr, d2
    position = torch.full((len(index),), -1, dtype=torch.int64, device=dev)
    position[rows] = torch.arange(n, device=dev)
    for lo in range(0, n, chunk):
        own = rows[lo:lo + chunk]
        q16 = index.vectors[own].contiguous()
        scores, found = index._topk(q16, k + 1, None, index._bias)
        scores = finish_scores(scores, index.metric, q16)
        is_self = found == own[:, None]
        is_self[:, k] |= ~is_self.any(dim=1)                      # not among them: the last one goes
        keep = ~is_self
        found, scores = found[keep].reshape(-1, k), scores[keep].reshape(-1, k)
        there = found >= 0
        nbr[lo:lo + chunk] = torch.where(there, position[found.clamp_min(0)], found).to(torch.int32)
        dist = (2.0 - 2.0 * scores) if index.metric == "cosine" else -scores
        d2[lo:lo + chunk] = torch.where(there, dist.clamp_min(0.0), torch.zeros_like(dist))
    return rows, nbr, d2


def affinities(d2, nbr, perplexity, steps=100, return_beta=False):
    """p f32 [n, k]: coati_tsne_affinities on d2 f32 [n, k], nbr int32 [n, k] (-1 = no neighbour, p = 0): per row the conditional
    probabilities whose entropy is log(perplexity), by `steps` bisection steps on beta with no early exit.  return_beta: (p, beta [n])."""
    if d2.dtype != torch.float32 or nbr.dtype != torch.int32 or d2.dim() != 2 or d2.shape != nbr.shape or d2.device != nbr.device:
        raise ValueError("affinities: d2 must be f32 [n, k] and nbr int32 [n, k] on one device")
    n, k = d2.shape
    if not 1 <= k <= AFFINITY_K_MAX:
        raise ValueError(f"affinities: k={k} outside 1 .. {AFFINITY_K_MAX}")
    if not float(perplexity) > 0.0:
        raise ValueError(f"affinities: perplexity={perplexity} is not positive")
    _need_gpu(d2, "affinities")
    d2, nbr = d2.contiguous(), nbr.contiguous()
    p = torch.empty_like(d2)
    beta = torch.empty(n, dtype=torch.float32, device=d2.device)
    if n:
        with torch.cuda.device(d2.device):
            _lib.call("coati_tsne_affinities", ptr(d2), ptr(nbr), n, k, float(perplexity), int(steps), ptr(p), ptr(beta), stream())
    return (p, beta) if return_beta else p


def joint(nbr, p):
    """(offsets int64 [n + 1], cols int32 [nnz], vals f32 [nnz]): the CSR of the symmetric joint P = (P_cond + P_cond^T) / (2 n) of the
    conditional p [n, k] over the graph nbr [n, k] (-1: no entry); the columns of a row ascend.  Plain torch, on the operands' device."""
    n, k = nbr.shape
    dev = nbr.device
    there = nbr >= 0
    r = torch.arange(n, device=dev)[:, None].expand(n, k)[there]
    c = nbr[there].long()
    v = p[there].to(torch.float32)
    # the COO entries and their transpose, sorted by (row, col); equal keys are merged
    key = torch.cat([r * n + c, c * n + r])
    order = torch.sort(key, stable=True).indices
    key, v = key[order], torch.cat([v, v])[order]
    ukey, inverse = torch.unique_consecutive(key, return_inverse=True)
    # a key has at most two terms -- p[i, j] and p[j, i]: a kNN row lists a neighbour once -- and a + b = b + a, so the merged sum has the
    # same bits in whatever order index_add_ (atomics on a GPU) meets them
    vals = torch.zeros(ukey.shape[0], dtype=torch.float32, device=dev).index_add_(0, inverse, v) / float(2 * max(n, 1))
    counts = torch.bincount(ukey // max(n, 1), minlength=n)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), counts.cumsum(0)])
    return offsets, (ukey % max(n, 1)).to(torch.int32), vals


def part_for(n, device):
    """the workspace coati_tsne_repulsion may split its chunks with: f32 [coati_tsne_part_floats(n)], or None past PART_BYTES_MAX"""
    need = int(_lib.lib().coati_tsne_part_floats(int(n)))
    if need < 0:
        raise RuntimeError(f"coati_tsne_part_floats({n}): {_lib.lib().coati_last_error().decode('utf-8', 'replace')}")
    return torch.empty(need, dtype=torch.float32, device=device) if 4 * need <= PART_BYTES_MAX else None


def repulsion(y, part=None, blocks=0, out=None):
    """(rep f32 [n, 2], z f32 [n]) of coati_tsne_repulsion on y f32 [n, 2]: over all j != i, rep_i = sum q^2 (y_i - y_j), z_i = sum q, q =
    1 / (1 + |y_i - y_j|^2).  part: None or part_for(n); blocks: the workgroups (0 = default).  Neither changes a bit of the result."""
    if y.dtype != torch.float32 or y.dim() != 2 or y.shape[1] != 2 or not y.is_contiguous():
        raise ValueError("repulsion: y must be contiguous f32 [n, 2]")
    _need_gpu(y, "repulsion")
    n = y.shape[0]
    rep, z = out if out is not None else (torch.empty_like(y), torch.empty(n, dtype=torch.float32, device=y.device))
    if n:
        with torch.cuda.device(y.device):
            _lib.call("coati_tsne_repulsion", ptr(y), n, ptr(rep), ptr(z), ptr(part), 0 if part is None else part.numel(), int(blocks), stream())
    return rep, z


def step(y, rep, zsum, offsets, cols, vals, update, gains, y_out, exaggeration=1.0, momentum=0.8, lr=200.0, min_gain=0.01, kl_rows=None,
         att=None):
    """coati_tsne_step: one iteration's attraction over the CSR joint P, gradient and update.  update and gains [n, 2] are changed in
    place, y_out [n, 2] (not y) receives the new points; kl_rows [n] and att [n, 2], when given, the rows' KL terms and attraction sums."""
    n = y.shape[0]
    for name, t, shape, dtype in (("y", y, (n, 2), torch.float32), ("rep", rep, (n, 2), torch.float32), ("zsum", zsum, None, torch.float32),
                                  ("offsets", offsets, (n + 1,), torch.int64), ("cols", cols, None, torch.int32), ("vals", vals, None, torch.float32),
                                  ("update", update, (n, 2), torch.float32), ("gains", gains, (n, 2), torch.float32),
                                  ("y_out", y_out, (n, 2), torch.float32), ("kl_rows", kl_rows, (n,), torch.float32), ("att", att, (n, 2), torch.float32)):
        if t is None and name in ("kl_rows", "att"):
            continue
        if t.dtype != dtype or (shape is not None and tuple(t.shape) != shape) or not t.is_contiguous() or t.device != y.device:
            raise ValueError(f"step: {name} must be contiguous {dtype} {shape if shape is not None else ''} on y's device")
    if zsum.numel() != 1 or cols.shape != vals.shape:
        raise ValueError("step: zsum must hold one value, cols and vals as many as each other")
    if y_out.data_ptr() == y.data_ptr():
        raise ValueError("step: y_out is y (other rows read y: use two buffers in turn)")
    _need_gpu(y, "step")
    if n:
        with torch.cuda.device(y.device):
            _lib.call("coati_tsne_step", ptr(y), ptr(rep), ptr(zsum), ptr(offsets), ptr(cols), ptr(vals), n, float(exaggeration), float(momentum),
                      float(lr), float(min_gain), ptr(update), ptr(gains), ptr(y_out), ptr(kl_rows), ptr(att), stream())
    return y_out


def initial_points(n, init="random", seed=0):
    """the start of a map, f32 [n, 2] on the CPU: "random" = 1e-4 randn from a CPU generator seeded with `seed` (sklearn's scale; the same
    on any device), or a given [n, 2] tensor"""
    if isinstance(init, str):
        if init != "random":
            raise ValueError(f"layout: init={init!r} is neither 'random' nor a tensor")
        return 1e-4 * torch.randn(n, 2, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32)
    y = torch.as_tensor(init).detach().to(device="cpu", dtype=torch.float32)
    if tuple(y.shape) != (n, 2):
        raise ValueError(f"layout: init must be [{n}, 2], got {tuple(y.shape)}")
    return y.clone()


def layout(offsets, cols, vals, n, iters=1000, exaggeration=12.0, exaggeration_iters=250, lr="auto", momentum=(0.5, 0.8), min_gain=0.01,
           init="random", seed=0, kl_every=50, blocks=0):
    """TSNEResult(y f32 [n, 2], kl, kl_trace) of `iters` iterations of sklearn's descent on the CSR joint P (joint()): the first
    exaggeration_iters with P times `exaggeration` and momentum[0], the rest with P as it is and momentum[1].  lr: a number, or "auto" =
    max(n / exaggeration / 4, 50) as sklearn.  An iteration is the repulsion, Z = z.sum(float64) on the device (no host sync), and the
    step; the KL (of P un-exaggerated) is computed and read back after every kl_every-th iteration and the last one -- it belongs to the
    points that iteration started from.  blocks: the repulsion's workgroups; no bit of the result depends on it."""
    n, iters, kl_every = int(n), int(iters), int(kl_every)
    if iters < 0 or kl_every < 1:
        raise ValueError(f"layout: iters={iters} < 0 or kl_every={kl_every} < 1")
    if offsets.shape[0] != n + 1:
        raise ValueError(f"layout: offsets must be [{n + 1}]")
    _need_gpu(offsets, "layout")
    dev = offsets.device
    rate = max(n / float(exaggeration) / 4.0, 50.0) if isinstance(lr, str) else float(lr)
    if isinstance(lr, str) and lr != "auto":
        raise ValueError(f"layout: lr={lr!r} is neither 'auto' nor a number")
    y = initial_points(n, init, seed).to(dev).contiguous()
    other = torch.empty_like(y)
    update, gains = torch.zeros_like(y), torch.ones_like(y)
    rep, z = torch.empty_like(y), torch.empty(n, dtype=torch.float32, device=dev)
    kl_rows = torch.empty(n, dtype=torch.float32, device=dev)
    part = part_for(n, dev) if n else None
    trace = []
    for it in range(1, iters + 1):
        early = it <= int(exaggeration_iters)
        with_kl = it % kl_every == 0 or it == iters
        repulsion(y, part, blocks, out=(rep, z))
        zsum = z.sum(dtype=torch.float64).float().reshape(1)
        step(y, rep, zsum, offsets, cols, vals, update, gains, other, exaggeration=float(exaggeration) if early else 1.0,
             momentum=float(momentum[0] if early else momentum[1]), lr=rate, min_gain=float(min_gain), kl_rows=kl_rows if with_kl else None)
        if with_kl:
            trace.append((it, float(kl_rows.sum(dtype=torch.float64) + zsum.double().log()[0])))
        y, other = other, y
    return TSNEResult(y, trace[-1][1] if trace else float("nan"), trace)


def tsne_index(index, perplexity=30.0, iters=1000, seed=0, k=None, steps=100, **layout_args):
    """EmbeddingIndex.tsne: the map of the live rows, scattered to [len(index), 2] (NaN for removed rows)"""
    live = int((index.bias > float("-inf")).sum()) if len(index) else 0
    if live < 2:
        raise ValueError(f"tsne: {live} live rows; a map needs two")
    if k is None:
        k = min(live - 1, int(3 * float(perplexity)), K_MAX)
    rows, nbr, d2 = knn_graph(index, max(int(k), 1))
    p = affinities(d2, nbr, perplexity, steps)
    offsets, cols, vals = joint(nbr, p)
    res = layout(offsets, cols, vals, rows.shape[0], iters=iters, seed=seed, **layout_args)
    y = torch.full((len(index), 2), float("nan"), dtype=torch.float32, device=index.device)
    y[rows] = res.y
    return TSNEResult(y, res.kl, res.kl_trace)
