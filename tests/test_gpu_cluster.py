"""Library clustering on the GPU (include/coati_cluster.h, coati_amd/cluster.py, EmbeddingIndex.assign / kmeans,
coati_amd/generative/coati_cluster.py) against the float64 restatement of tests/cluster_util.py.  Integer data is exact in bf16 and in f32 in
any summation order, so those cases must EQUAL the restatement element for element, ties included; real-valued data is held to the f32
accumulation bound DESIGN.md section 6 uses for the search."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import cluster_util as C  # noqa: E402
from tests.gpu_util import log  # noqa: E402

DEV = "cuda:0"
NEG_INF = float("-inf")


def _dev(t):
    return None if t is None else t.to(DEV)


def _assign(x16, row_bias, c16, cbias, blocks=0):
    from coati_amd import cluster
    a, b = cluster.assign_call(_dev(x16), _dev(row_bias), _dev(c16), _dev(cbias), blocks)
    assert a.dtype == torch.int32 and b.dtype == torch.float32 and a.shape == b.shape == (x16.shape[0],)
    return a.cpu(), b.cpu()


def _exact(x16, row_bias, c16, cbias, label, blocks=0):
    """assign and best == the restatement, element for element; returns them"""
    a, b = _assign(x16, row_bias, c16, cbias, blocks)
    wa, wb = C.assign(x16, row_bias, c16, cbias)
    bad_a, bad_b = int((a != wa).sum()), int((b.double() != wb).sum())
    log(f"cluster assign {label}: {bad_a} centres and {bad_b} scores of {a.numel()} differ from the restatement")
    assert bad_a == 0 and bad_b == 0, label
    return a, b


# ---- 1. exact cases -------------------------------------------------------------------------------------------------------------------
# N in {1, 15, 16, 17, 63, 64, 65, 255, 257, 1000, 70001}, K in {1, 15, 16, 17, 64, 65, 257, 1000, 4096}, E in {32, 96, 256, 512}: each edge
# once, not the product
EXACT = [(1, 1, 32), (15, 15, 96), (16, 16, 256), (17, 17, 512), (63, 64, 32), (64, 65, 96), (65, 257, 256), (255, 1000, 512), (257, 4096, 32),
         (1000, 4096, 512), (1000, 17, 96), (70001, 1, 256), (70001, 64, 512), (70001, 257, 32), (70001, 16, 96)]


@pytest.mark.parametrize("N,K,E", EXACT)
def test_integer_data_equals_the_restatement(N, K, E):
    gen = torch.Generator().manual_seed(N + 3 * K + E)
    x16, c16 = C.ints((N, E), 1000 + N + E).to(torch.bfloat16), C.ints((K, E), 7 * K + E).to(torch.bfloat16)
    cbias = 0.5 * torch.randint(-6, 7, (K,), generator=gen).float()                      # half-integers: ties are frequent
    row_bias = torch.where(torch.rand(N, generator=gen) < 0.2, torch.full((N,), NEG_INF), torch.randn(N, generator=gen))
    label = f"N={N} K={K} E={E}"
    a0, _ = _exact(x16, None, c16, None, label + " plain")
    assert int(a0.min()) >= 0 and int(a0.max()) < K
    a, b = _exact(x16, row_bias, c16, cbias, label + " cbias, excluded rows")
    out = row_bias == NEG_INF
    assert bool((a[out] == -1).all() and (b[out] == NEG_INF).all() and (a[~out] >= 0).all())
    for blocks in (1, 3):                                                                 # the result does not depend on the grid
        a2, b2 = _assign(x16, row_bias, c16, cbias, blocks)
        assert torch.equal(a2, a) and torch.equal(b2, b), (label, blocks)


# ---- 2. the pad cannot win ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 17])
@pytest.mark.parametrize("E", [32, 256, 512])
def test_padded_centres_never_win(K, E):
    """every score negative: a zero (or any finite) score in a column >= K of the padded centre tile would beat them all"""
    x16 = -C.ints((300, E), 5, 1, 4).to(torch.bfloat16)
    c16 = C.ints((K, E), 6, 1, 4).to(torch.bfloat16)
    a, b = _exact(x16, None, c16, None, f"negative scores K={K} E={E}")
    assert int(a.min()) >= 0 and int(a.max()) <= K - 1 and float(b.max()) < 0
    x16 = C.ints((300, E), 7).to(torch.bfloat16)
    cbias = torch.full((K,), -100.0) - 4.0 * E
    a, b = _exact(x16, None, C.ints((K, E), 8).to(torch.bfloat16), cbias, f"cbias below every dot K={K} E={E}")
    assert int(a.min()) >= 0 and int(a.max()) <= K - 1 and float(b.max()) < 0


# ---- 3. tie order -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 34, 100, 1000])
def test_equal_centres_go_to_the_lowest_index(K):
    x16 = C.ints((777, 96), 11).to(torch.bfloat16)
    same = C.ints((1, 96), 12).to(torch.bfloat16).expand(K, 96).contiguous()
    a, _ = _exact(x16, None, same, None, f"identical centres K={K}")
    assert bool((a == 0).all())
    pairs = C.ints((K // 2, 96), 13).to(torch.bfloat16).repeat_interleave(2, dim=0).contiguous()
    a, _ = _exact(x16, None, pairs, None, f"centres equal in pairs K={K}")
    assert bool((a % 2 == 0).all())


# ---- 4. real data -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,E,metric", [(257, 256, "cosine"), (257, 256, "l2"), (64, 512, "cosine"), (1000, 32, "l2")])
def test_real_data_within_the_accumulation_bound(K, E, metric):
    """b = E 2^-23 |x| max|c| per row.  The centre chosen scores within 2 b of the best one, best is within b of that centre's float64
    score, and at least 99 % of the rows have the restatement's argmax (the restatement's own share of rows whose two best scores are
    closer than 2 b is logged: under 0.6 % on this data)."""
    from coati_amd import cluster
    N = 20000
    torch.manual_seed(0)
    x, c = torch.randn(N, E), torch.randn(K, E)
    if metric == "cosine":
        x = x / x.norm(dim=1, keepdim=True)
    x16 = x.to(torch.bfloat16)
    row_bias = -(x16.double() ** 2).sum(dim=1).float() if metric == "l2" else torch.zeros(N)
    _, c16, cbias = cluster.prepare_centres(c.to(DEV), metric, E)                      # the centres as the device prepared them
    c16, cbias = c16.cpu(), None if cbias is None else cbias.cpu()
    assert (cbias is None) == (metric == "cosine") and float((c16.double() - C.prepare_centres(c, metric)[1].double()).abs().max()) < 0.05
    a, best = _assign(x16, row_bias, c16, cbias)
    s = C.scores(x16, c16, cbias)
    want, top = C.argmax_low(s)
    b = E * 2.0 ** -23 * x16.double().norm(dim=1) * float(c16.double().norm(dim=1).max())
    assert int(a.min()) >= 0 and int(a.max()) < K
    got = s.gather(1, a.long()[:, None])[:, 0]
    top2 = s.topk(2, dim=1).values
    tight = int((top2[:, 0] - top2[:, 1] < 2 * b).sum())
    share = float((a.long() == want).float().mean())
    worst_gap, worst_best = float(((top - got) / b).max()), float(((best.double() - got).abs() / b).max())
    log(f"cluster assign real K={K} E={E} {metric}: {100 * share:.3f} % of {N} rows at the restatement's argmax; {tight} rows with a top-two "
        f"gap under 2 b; worst (max - chosen) / b = {worst_gap:.3g}, worst |best - s| / b = {worst_best:.3g}")
    assert bool((got >= top - 2 * b).all())
    assert bool(((best.double() - got).abs() <= b).all())
    assert share >= 0.99
    # the functional core on top: the same centres, the metric's score
    a2, score = cluster.assign_rows(x16.to(DEV), row_bias.to(DEV), c.to(DEV), metric)
    assert torch.equal(a2.cpu(), a)
    want_score = best if metric == "cosine" else (2.0 * best + row_bias).clamp_max(0.0)
    assert torch.equal(score.cpu(), want_score)
    if metric == "l2":
        d2 = ((x16.double() - c16.double()[a.long()]) ** 2).sum(dim=1)
        assert float((score.cpu().double() + d2).abs().max()) <= 4 * float(b.max()) + 1e-5 * float(d2.max())


# ---- 5. sums, exact -----------------------------------------------------------------------------------------------------------------------
def _sums(x16, assign, k, blocks=0):
    from coati_amd import cluster
    ch = cluster.chunk_rows()
    order, sizes = cluster.sorted_order(assign.to(DEV), k)
    offsets, item_off = cluster.item_table(sizes, ch)
    M = int(sizes.sum())
    return cluster.sums_call(x16.to(DEV), order[:M].to(torch.int32), offsets, item_off, blocks=blocks), sizes.cpu()


def _engineered(kind):
    """(assign int32 [N] in a random row order, k)"""
    from coati_amd import cluster
    ch = cluster.chunk_rows()
    if kind == "chunk edges":
        sizes = [0, 1, ch - 1, ch, ch + 1, 2 * ch + 1, 0, 3]
        labels = torch.cat([torch.full((n,), i) for i, n in enumerate(sizes)] + [torch.full((38,), -1)])     # and 38 excluded rows
    else:                                                                                                  # one cluster holds all but K - 1 rows
        k = 16
        labels = torch.cat([torch.zeros(70001 - (k - 1), dtype=torch.int64), torch.arange(1, k)])
        sizes = [70001 - (k - 1)] + [1] * (k - 1)
    perm = torch.randperm(labels.shape[0], generator=torch.Generator().manual_seed(len(sizes)))
    return labels[perm].to(torch.int32), len(sizes), sizes


@pytest.mark.parametrize("E", [32, 256, 512])
@pytest.mark.parametrize("kind", ["chunk edges", "skew"])
def test_sums_of_integer_rows_are_exact(kind, E):
    assign, k, sizes = _engineered(kind)
    x16 = C.ints((assign.shape[0], E), 21 + E).to(torch.bfloat16)
    want = C.sums(x16, assign, k)
    assert float(want.abs().max()) < 2 ** 24
    got, got_sizes = _sums(x16, assign, k)
    assert got.shape == (k, E) and got.dtype == torch.float32 and got_sizes.tolist() == sizes
    bad = int((got.cpu().double() != want).sum())
    log(f"cluster sums {kind} E={E}: {bad} of {want.numel()} elements differ from float64")
    assert bad == 0
    assert bool((got.cpu()[torch.tensor(sizes) == 0] == 0).all())
    for blocks in (1, 7):
        assert torch.equal(_sums(x16, assign, k, blocks)[0], got), (kind, E, blocks)


# ---- 6. sums, real data -------------------------------------------------------------------------------------------------------------------
def test_sums_of_real_rows_are_bounded_and_reproducible():
    """every element within n_k 2^-24 sum |x| of float64 (n_k - 1 f32 additions, each rounding a partial sum that is at most sum |x|);
    bitwise equal between calls, grids and streams"""
    N, K, E = 20000, 37, 256
    gen = torch.Generator().manual_seed(4)
    x16 = torch.randn(N, E, generator=gen).to(torch.bfloat16)
    assign = (torch.randint(0, K, (N,), generator=gen) ** 2 // K).to(torch.int32)          # uneven sizes
    assign[torch.rand(N, generator=gen) < 0.05] = -1
    want = C.sums(x16, assign, K)
    keep = assign >= 0
    mass = torch.zeros(K, E, dtype=torch.float64).index_add_(0, assign[keep].long(), x16.double().abs()[keep])
    got, sizes = _sums(x16, assign, K)
    bound = sizes.double()[:, None] * 2.0 ** -24 * mass
    err = (got.cpu().double() - want).abs()
    log(f"cluster sums real: worst error / bound = {float((err / bound.clamp_min(1e-300)).max()):.3g}, sizes {int(sizes.min())} .. {int(sizes.max())}")
    assert bool((err <= bound).all())
    assert torch.equal(_sums(x16, assign, K)[0], got)
    assert torch.equal(_sums(x16, assign, K, blocks=5)[0], got)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        junk = torch.randn(512, 512, device=DEV) @ torch.randn(512, 512, device=DEV)       # unrelated work first
        again, _ = _sums(x16, assign, K)
    side.synchronize()
    assert torch.equal(again, got) and bool(torch.isfinite(junk).all())


# ---- 7. the loop --------------------------------------------------------------------------------------------------------------------------
def _blobs(metric, N=5000, k=7, dim=24):
    """lattice centres 8 apart with integer offsets in -1 .. 1 (on the unit sphere once the cosine index has normalised them), and initial
    centres half way out on every blob's axis: the assignment is unambiguous in every round"""
    gen = torch.Generator().manual_seed(9)
    label = torch.randint(0, k, (N,), generator=gen)
    x = 8.0 * torch.eye(dim)[label] + torch.randint(-1, 2, (N, dim), generator=gen).float()
    init = 4.0 * torch.eye(dim)[:k] + 0.25
    return x, label, init


def _index(x, metric):
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(x.shape[1], metric=metric, device=DEV)
    index.add(x)
    return index


def _same_run(cl, want, n):
    assert cl.assign.dtype == torch.int32 and cl.assign.shape == (n,) and cl.sizes.dtype == torch.int64
    assert torch.equal(cl.assign.cpu(), want["assign"]) and torch.equal(cl.sizes.cpu(), want["sizes"])
    assert cl.iterations == want["iterations"] and cl.converged == want["converged"]
    dim = cl.centres.shape[1]
    err = float((cl.centres.cpu().double() - want["centres"][:, :dim].double()).abs().max()) / float(want["centres"].abs().max())
    assert cl.centres.dtype == torch.float32 and err <= 1e-6, err
    assert len(cl.inertia) == cl.iterations + 1 and all(v >= 0 for v in cl.inertia)
    return err


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_kmeans_is_the_restatements_run(metric):
    x, label, init = _blobs(metric)
    index = _index(x, metric)
    x16, bias = index.vectors.cpu(), index.bias.cpu()
    pad = torch.nn.functional.pad(init, (0, index.dim_padded - index.dim))
    cl = index.kmeans(7, init=init)
    want = C.kmeans(x16, bias, metric, pad)
    err = _same_run(cl, want, 5000)
    log(f"cluster kmeans {metric}: {cl.iterations} updates, converged {cl.converged}, centres within {err:.2e}, inertia {cl.inertia}")
    assert cl.converged is True and cl.iterations >= 1 and cl.centres.shape == (7, 24) and cl.rows is None
    assert torch.equal(cl.assign.cpu().long(), label) and cl.inertia[-1] <= cl.inertia[0]
    assert torch.equal(index.assign(cl.centres)[0], cl.assign)
    # a cap on the updates: the rows are assigned to the last centres, and nothing claims convergence
    capped = index.kmeans(7, iters=0, init=init)
    _same_run(capped, C.kmeans(x16, bias, metric, pad, iters=0), 5000)
    assert capped.iterations == 0 and capped.converged is False
    # removed rows are -1 and counted nowhere
    gone = torch.arange(0, 5000, 7)
    index.remove(gone)
    cl2 = index.kmeans(7, init=init)
    _same_run(cl2, C.kmeans(x16, index.bias.cpu(), metric, pad), 5000)
    assert bool((cl2.assign[gone.to(DEV)] == -1).all()) and int(cl2.sizes.sum()) == 5000 - gone.numel()
    assert int((cl2.assign >= 0).sum()) == 5000 - gone.numel() and bool((cl2.score[gone.to(DEV)] == NEG_INF).all())
    # rows=: the subset only, answered in library rows
    subset = torch.arange(1, 5000, 3)
    cl3 = index.kmeans(7, init=init, rows=subset)
    _same_run(cl3, C.kmeans(x16[subset], index.bias.cpu()[subset], metric, pad), subset.numel())
    assert torch.equal(cl3.rows.cpu(), subset)
    members = cl3.members(2).cpu()
    assert torch.equal(members, subset[cl3.assign.cpu() == 2]) and bool((label[members] == 2).all())


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_kmeans_from_a_seed_is_reproducible(metric):
    """seeded rows as gp_head._kmeans draws them (a CPU randperm over the live rows); the same seed twice: bitwise equal"""
    torch.manual_seed(1)
    x = torch.randn(6000, 40)
    index = _index(x, metric)
    index.remove(torch.arange(0, 6000, 11))
    live = torch.nonzero(index.bias.cpu() > NEG_INF).reshape(-1)
    pick = live[torch.randperm(live.numel(), generator=torch.Generator().manual_seed(5))[:19]]
    start = index.kmeans(19, iters=0, seed=5)
    drawn = index.vectors.cpu()[pick].float()[:, :40]
    if metric == "cosine":                                                            # centres are prepared as queries are: normalised again
        assert float((start.centres.cpu() - drawn / drawn.norm(dim=1, keepdim=True)).abs().max()) <= 1e-6
    else:
        assert torch.equal(start.centres.cpu(), drawn)
    one, two, other = index.kmeans(19, iters=6, seed=5), index.kmeans(19, iters=6, seed=5), index.kmeans(19, iters=6, seed=6)
    assert torch.equal(one.assign, two.assign) and torch.equal(one.centres, two.centres) and torch.equal(one.score, two.score)
    assert one.inertia == two.inertia and one.iterations == two.iterations and torch.equal(one.sizes, two.sizes)
    assert not torch.equal(one.assign, other.assign)
    assert one.inertia[-1] < one.inertia[0] and int(one.sizes.sum()) == live.numel()
    with pytest.raises(ValueError, match="centres from"):
        index.kmeans(4096, rows=torch.arange(1, 100))


# ---- 8. picks -----------------------------------------------------------------------------------------------------------------------------
def test_representatives_are_each_clusters_best_member():
    torch.manual_seed(2)
    index = _index(torch.randn(4000, 64), "cosine")
    index.remove(torch.arange(5, 4000, 50))
    cl = index.kmeans(23, iters=5, seed=1)
    scores = torch.randint(0, 6, (4000,), generator=torch.Generator().manual_seed(3)).float()      # few values: ties in every cluster
    reps = cl.representatives(scores.to(DEV))
    assert reps.dtype == torch.int64 and torch.equal(reps.cpu(), C.representatives(cl.assign, scores, 23))
    assert torch.equal(cl.representatives().cpu(), C.representatives(cl.assign, cl.score, 23))
    from coati_amd.generative import diverse_subset
    rows, cl2 = diverse_subset(index, 23, scores=scores.to(DEV), iters=5, seed=1)
    assert torch.equal(cl2.assign, cl.assign) and torch.equal(rows, reps[reps >= 0])


def _check_diverse(index, key, values, out, n, pool):
    scores, rows, cl = out
    scores, rows = scores.cpu(), rows.cpu()
    assert rows.dtype == torch.int64 and scores.dtype == torch.float32 and rows.shape == scores.shape == (n,)
    assert len(set(rows.tolist())) == n
    want_pool = torch.topk(key, pool).indices
    assert set(rows.tolist()) <= set(want_pool.tolist()) and set(cl.rows.cpu().tolist()) == set(want_pool.tolist())
    where = {int(r): i for i, r in enumerate(cl.rows.cpu().tolist())}
    clusters = [int(cl.assign[where[int(r)]]) for r in rows]
    assert sorted(clusters) == list(range(n))                                         # one per cluster
    for r, c in zip(rows.tolist(), clusters):
        members = cl.members(c).cpu()
        assert r in members.tolist() and float(key[r]) == float(key[members].max())    # the best-scored of its cluster
    assert torch.equal(scores, values[rows]) and bool((key[rows][:-1] >= key[rows][1:]).all())


def test_diverse_screen_with_a_property_head():
    from coati_amd.generative import diverse_screen
    from coati_amd.models.regression import PropertyHead
    torch.manual_seed(4)
    index = _index(torch.randn(3000, 64), "l2")
    index.remove(torch.arange(0, 3000, 40))
    head = PropertyHead(64, features=64, depth=1, num_outputs=1).to(DEV)
    values = index.property_scores(head)[:, 0].cpu()
    live = index.bias.cpu() > NEG_INF
    for largest in (True, False):
        key = torch.where(live, values if largest else -values, torch.full_like(values, NEG_INF))
        out = diverse_screen(index, head, 8, pool=200, largest=largest, iters=10, seed=2)
        _check_diverse(index, key, values, out, 8, 200)
    scores, rows, cl = diverse_screen(index, head, 8)                                  # the default pool: 20 n
    assert cl.rows.numel() == 160 and rows.numel() == 8


def test_diverse_screen_with_a_gp_head_and_ucb():
    from coati_amd.generative import diverse_screen
    from coati_amd.models.regression import acquisition_values
    from tests import gp_util as G
    index = _index(G.unit_rows(3000, 64, torch.Generator().manual_seed(6)).float(), "l2")      # unit rows: where random_gp's kernel varies
    gp, _ = G.random_gp(64, 64, 1, 1, 33, seed=8, n=200)
    gp = gp.to(DEV)
    mean, std = index.property_uncertainty(gp)
    values = acquisition_values(mean[:, 0], std[:, 0], "ucb", 2.0).float().cpu()
    assert values.unique().numel() > 2900                                               # (a ranking, not a plateau)
    out = diverse_screen(index, gp, 8, pool=200, acquisition="ucb", beta=2.0, iters=10, seed=2)
    _check_diverse(index, values, values, out, 8, 200)
