"""Embedding maps on the GPU (include/coati_tsne.h, coati_amd/tsne.py) against the float64 restatement of tests/tsne_util.py: the three
kernels one by one at the smallest shapes that can go wrong, the kNN graph against cdist + topk, and one map of 512 rows end to end.

Bounds.  U = 2^-24 is one f32 rounding.  A sum of m terms added one after the other is off by at most (m - 1) U sum|term|; the terms
themselves carry a few roundings each (at most ~10 in the repulsion: two subtractions, two fma for 1 + |d|^2, v_rcp_f32 at 1 ulp = 2 U,
squared, one more fma), which the "+ 16" covers.  So every accumulated quantity is held to (longest chain + 16) U sum|term|, the terms
taken from float64 -- the form DESIGN.md section 6 uses for the search.  Where the only honest bound is a measured one (the bisection's
beta at f32 resolution; two trajectories that diverge), the figure measured on an MI355X is in the test's docstring and the bound is the
stated multiple of it."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import tsne_util as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = R.U


def _tsne():
    from coati_amd import tsne
    return tsne


# ---- 1. affinities ----------------------------------------------------------------------------------------------------------------------
# measured on an MI355X over the six shapes below: max |p - p64| = AFF_P_MEASURED, max |perplexity attained - perplexity| / perplexity
# = AFF_PERP_MEASURED (f32 expf and the f32 resolution of beta are the only sources); the bounds are 4 x these
AFF_P_MEASURED = 1.44e-7
AFF_PERP_MEASURED = 7.7e-7


def _affinity_rows(N, k, perplexity, seed):
    """kNN-like rows (ascending d2), and among the first ones: equal distances, leading zeros, a -1 tail shorter than the perplexity, a
    row of -1 only, a spread of 10^6.  attainable: the rows whose perplexity can be met (more distinct valid entries than it)"""
    g = torch.Generator().manual_seed(seed)
    d2 = (torch.rand(N, k, generator=g) * 2.0 + 0.01).cumsum(dim=1) * torch.rand(N, 1, generator=g).mul(3).exp()
    nbr = torch.randint(0, max(N, 2), (N, k), generator=g, dtype=torch.int32)
    attainable = torch.full((N,), k > perplexity * 1.5, dtype=torch.bool)
    if N >= 6:
        d2[0] = 3.0
        d2[1, :min(3, k)] = 0.0
        short = max(1, min(k - 1, int(perplexity) - 1))
        nbr[2, short:] = -1
        nbr[3] = -1
        d2[4] = torch.logspace(0, 6, k)
        attainable[:4] = False
        if k >= 8:                             # holes anywhere, not only a tail.  (Not at k = 5, perplexity 2: exactly `perplexity` valid entries
            nbr[5, ::2] = -1                   # put the root at beta = 0 where H'(beta) = 0 -- a double root, found to sqrt(rounding) in any
            attainable[5] = k // 2 > perplexity * 1.5      # precision: one ulp of logf moved p by 5.6e-5 there, measured)
    return d2.contiguous(), nbr.contiguous(), attainable


@pytest.mark.parametrize("N,k,perplexity", [(1, 3, 2.0), (63, 5, 2.0), (64, 64, 30.0), (65, 90, 30.0), (257, 127, 42.0), (1000, 128, 30.0)])
def test_affinities(N, k, perplexity):
    T = _tsne()
    d2, nbr, attainable = _affinity_rows(N, k, perplexity, 7 * N + k)
    p, beta = T.affinities(d2.to(DEV), nbr.to(DEV), perplexity, return_beta=True)
    p, beta = p.cpu(), beta.cpu()
    p64, beta64, _ = R.affinities(d2, nbr, perplexity)
    assert torch.isfinite(p).all() and torch.isfinite(beta).all()
    assert torch.equal(p[nbr < 0], torch.zeros(int((nbr < 0).sum())))          # padded entries exactly 0
    some = (nbr >= 0).any(dim=1)
    sums = p.double().sum(dim=1)
    assert float((sums[some] - 1).abs().max()) <= (k + 8) * U
    assert torch.equal(sums[~some], torch.zeros(int((~some).sum()), dtype=torch.float64)) and torch.equal(beta[~some], torch.zeros(int((~some).sum())))
    err = float((p.double() - p64).abs().max())
    H = -(torch.where(p > 0, p.double() * p.double().clamp_min(1e-300).log(), torch.zeros_like(p64))).sum(dim=1)
    perp_err = float(((H.exp() - perplexity).abs() / perplexity)[attainable].max()) if bool(attainable.any()) else 0.0
    print(f"affinities N={N} k={k} perplexity={perplexity}: max |p - p64| {err:.3e}, perplexity attained off by {perp_err:.3e} (relative)")
    assert err <= 4 * AFF_P_MEASURED
    assert perp_err <= 4 * AFF_PERP_MEASURED
    if N >= 6:
        assert float((p[0] - 1.0 / k).abs().max()) <= 2 * U                   # equal distances: the uniform row


# ---- 2. repulsion -----------------------------------------------------------------------------------------------------------------------
def _points(N, scale, seed):
    g = torch.Generator().manual_seed(seed)
    y = (scale * torch.randn(N, 2, generator=g)).float()
    if N > 1:
        y[1] = y[0]                            # coincident points: q = 1, no force
    if N > 4:
        y[N // 2] = y[0]
        y[N - 1] = y[N - 2]
    return y.contiguous()


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 257, "J-1", "J", "J+1", "2J+17"])
def test_repulsion(N):
    T = _tsne()
    J = T.chunk_points()
    N = {"J-1": J - 1, "J": J, "J+1": J + 1, "2J+17": 2 * J + 17}.get(N, N)
    bound = (J + math.ceil(N / J) + 16) * U
    for scale in (1e-4, 1.0, 50.0):
        y = _points(N, scale, N + int(scale))
        rep64, z64, rep_abs, _ = R.repulsion(y)
        yd = y.to(DEV)
        rep, z = T.repulsion(yd)
        assert torch.isfinite(rep).all() and torch.isfinite(z).all()
        assert bool(((rep.cpu().double() - rep64).abs() <= bound * rep_abs).all()), (N, scale)
        assert bool(((z.cpu().double() - z64).abs() <= bound * z64).all()), (N, scale)
        part = T.part_for(N, DEV)
        assert part is not None
        for blocks in (0, 1, 3):
            for ws in (None, part):
                rep2, z2 = T.repulsion(yd, part=ws, blocks=blocks)
                assert torch.equal(rep2, rep) and torch.equal(z2, z), (N, scale, blocks, ws is not None)
    if N == 1:
        assert float(z[0]) == 0.0 and torch.equal(rep, torch.zeros_like(rep))


# ---- 3. step ----------------------------------------------------------------------------------------------------------------------------
def _step_case(N, seed):
    """a CSR with rows of every length -- row 3 empty, row 0 a hub of 3000 entries (N > 1) -- and a state that takes both gain branches,
    the min_gain floor and g = 0 (the empty row, with no repulsion either)"""
    g = torch.Generator().manual_seed(seed)
    counts = torch.randint(0, 200, (N,), generator=g)
    if N > 1:
        counts[0] = 3000
    if N > 3:
        counts[3] = 0
    if N == 1:
        counts[0] = 0
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
    nnz = int(offsets[-1])
    rows = R.csr_rows(offsets)
    cols = torch.randint(0, N, (nnz,), generator=g)
    cols = cols[torch.sort(rows * N + cols, stable=True).indices].to(torch.int32)       # ascending within a row (a hub repeats columns)
    vals = (torch.rand(nnz, generator=g) * 1e-3 + 1e-7).float()
    if nnz:
        vals[::17] = 0.0                                                              # an entry without mass: no KL term
    y = (3.0 * torch.randn(N, 2, generator=g)).float()
    rep = (0.5 * torch.randn(N, 2, generator=g)).float()
    update = torch.randn(N, 2, generator=g).float()
    update[::5] = 0.0
    gains = (torch.rand(N, 2, generator=g) * 2 + 0.05).float()
    gains[1::4] = 0.011                                                               # 0.8 x 0.011 < min_gain: the floor
    if N > 3:
        rep[3] = 0.0
    if N == 1:
        rep[0] = 0.0
    Z = float(N * 3.7) if N > 1 else 0.0
    return y, rep, Z, offsets, cols, vals, update, gains


@pytest.mark.parametrize("exaggeration", [12.0, 1.0])
@pytest.mark.parametrize("N", [1, 65, 1000])
def test_step(N, exaggeration):
    T = _tsne()
    y, rep, Z, offsets, cols, vals, update, gains = _step_case(N, 11 * N)
    momentum, lr, min_gain = 0.8, 37.5, 0.01
    want = R.step(y, rep, Z, offsets, cols, vals, update, gains, exaggeration, momentum, lr, min_gain)

    def run():
        d = [t.to(DEV) for t in (y, rep, torch.tensor([Z], dtype=torch.float32), offsets, cols, vals, update.clone(), gains.clone())]
        y_out, kl_rows, att = torch.empty(N, 2, device=DEV), torch.empty(N, device=DEV), torch.empty(N, 2, device=DEV)
        T.step(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], y_out, exaggeration=exaggeration, momentum=momentum, lr=lr, min_gain=min_gain,
               kl_rows=kl_rows, att=att)
        return [t.cpu() for t in (att, y_out, d[6], d[7], kl_rows)]

    att, y_out, new_update, new_gains, kl_rows = run()
    for a, b in zip(run(), (att, y_out, new_update, new_gains, kl_rows)):
        assert torch.equal(a, b)                                                      # two calls: identical bits
    # a lane adds ceil(len / 64) entries in turn, six butterfly levels follow; + 16 for the roundings inside a term
    chain = ((offsets[1:] - offsets[:-1] + 63) // 64 + 6 + 16).double() * U
    att_err = chain[:, None] * want["att_abs"]
    assert bool(((att.double() - want["att"]).abs() <= att_err).all())
    assert bool(((kl_rows.double() - want["kl_rows"]).abs() <= chain * want["kl_abs"]).all())
    repz = (rep.double() / Z).abs() if Z > 0 else torch.zeros(N, 2, dtype=torch.float64)
    g_err = 4 * (exaggeration * att_err + 3 * U * repz) + 4 * U * (4 * (exaggeration * want["att"].abs() + repz))
    robust = want["g"].abs() >= 2 * g_err                      # the gain's branch hangs on the sign of update g: compare where it is decided
    robust |= update == 0                                       # (update g = 0 is not < 0 whatever g)
    assert float(robust.double().mean()) >= 0.99
    assert bool(((new_gains.double() - want["gains"]).abs() <= 2 * U * want["gains"])[robust].all())
    upd_err = lr * want["gains"] * g_err + 6 * U * ((momentum * update.double()).abs() + (lr * want["gains"] * want["g"]).abs())
    assert bool(((new_update.double() - want["update"]).abs() <= upd_err)[robust].all())
    y_err = upd_err + 2 * U * (y.double().abs() + want["update"].abs())
    assert bool(((y_out.double() - want["y_out"]).abs() <= y_err)[robust].all())
    # the cases the state was built for are there
    inc = (update.double() * want["g"] < 0)
    floor = want["gains"] == min_gain
    if N > 1:
        assert bool(inc.any()) and bool((~inc).any()) and bool(floor.any())
    empty = 3 if N > 3 else (0 if N == 1 else None)
    if empty is not None:
        assert torch.equal(att[empty], torch.zeros(2)) and float(kl_rows[empty]) == 0.0 and bool((want["g"][empty] == 0).all())
        assert torch.equal(new_update[empty], (momentum * update[empty]).float() - 0.0)
    with pytest.raises(ValueError, match="y_out is y"):
        yd = y.to(DEV)
        T.step(yd, yd, torch.zeros(1, device=DEV), offsets.to(DEV), cols.to(DEV), vals.to(DEV), yd.clone(), yd.clone(), yd)


# ---- 4. the kNN graph -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_knn_graph(metric):
    """integer rows (exact in bf16), 1000 x 64, 50 of them removed.  l2: every score is exact, so the neighbours, their order (ties by row)
    and d2 must equal float64 cdist + a stable sort.  cosine: the stored rows are bf16 roundings of unit rows and their dot products are
    accumulated in f32 -- at most (E + 2) roundings of a sum of |products| <= 1, twice in 2 - 2 s: 2 (E + 2) 2^-24 < 1e-5 -- so the
    neighbour in every slot must be as near, within that, as float64 says the slot's neighbour is."""
    from coati_amd.search import EmbeddingIndex
    N, E, k = 1000, 64, 20
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (N, E), generator=g).float()
    index = EmbeddingIndex(E, metric=metric, device=DEV)
    index.add(x)
    removed = torch.randperm(N, generator=g)[:50]
    index.remove(removed)
    rows, nbr, d2 = index.knn_graph(k, chunk=300)
    rows, nbr, d2 = rows.cpu(), nbr.cpu().long(), d2.cpu().double()
    live = torch.ones(N, dtype=torch.bool)
    live[removed] = False
    assert torch.equal(rows, torch.nonzero(live).reshape(-1)) and nbr.shape == d2.shape == (950, k)
    assert int(nbr.min()) >= 0 and int(nbr.max()) < 950                         # positions in rows: no removed row can appear
    assert bool((nbr != torch.arange(950)[:, None]).all())                      # never the row itself
    assert bool((nbr.sort(dim=1).values.diff(dim=1) > 0).all())                 # nobody twice
    stored = index.vectors.cpu().double()[rows]
    if metric == "l2":
        full = (stored ** 2).sum(1)[:, None] + (stored ** 2).sum(1)[None, :] - 2 * stored @ stored.T      # exact in float64 on integers
    else:
        full = (2 - 2 * stored @ stored.T).clamp_min(0)
    full.fill_diagonal_(math.inf)
    order = torch.sort(full, dim=1, stable=True)
    if metric == "l2":
        assert torch.equal(nbr, order.indices[:, :k]) and torch.equal(d2, order.values[:, :k])
    else:
        tol = 1e-5
        assert float((d2 - order.values[:, :k]).abs().max()) <= tol
        assert float((full.gather(1, nbr) - order.values[:, :k]).abs().max()) <= tol
    with pytest.raises(ValueError, match="dot"):
        EmbeddingIndex(E, metric="dot", device=DEV).knn_graph(3)


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------------
# measured on an MI355X: (b) the map after 3 iterations against the restatement's from the same start and CSR, max |y - y64| / max |y64|
# = E2E_STEP3_MEASURED; (e) |KL of the GPU map re-evaluated in float64 - the restatement's own final KL| = E2E_KL_GAP_MEASURED
E2E_STEP3_MEASURED = 1.05e-7
E2E_KL_GAP_MEASURED = 2.07e-4


@pytest.fixture(scope="module")
def clustered_map():
    from coati_amd.search import EmbeddingIndex
    T = _tsne()
    x, lab = R.clustered_rows(512, 64, 8, 0.5, seed=0)
    index = EmbeddingIndex(64, metric="cosine", device=DEV)
    index.add(x)
    result = index.tsne(perplexity=30, iters=500, seed=0)
    rows, nbr, d2 = index.knn_graph(90)
    offsets, cols, vals = T.joint(nbr, T.affinities(d2, nbr, 30.0))
    return dict(index=index, lab=lab, result=result, csr=(offsets, cols, vals), y0=T.initial_points(512, "random", 0))


def test_map_is_reproducible(clustered_map):
    """(a) the same call twice, and with another launch geometry: identical bits"""
    index, first = clustered_map["index"], clustered_map["result"]
    again = index.tsne(perplexity=30, iters=500, seed=0)
    other = index.tsne(perplexity=30, iters=500, seed=0, blocks=3)
    assert first.y.shape == (512, 2) and torch.isfinite(first.y).all()
    assert torch.equal(first.y, again.y) and torch.equal(first.y, other.y)
    assert first.kl == again.kl == other.kl and first.kl_trace == again.kl_trace
    assert not torch.equal(first.y, index.tsne(perplexity=30, iters=500, seed=1).y)


def test_first_iterations_follow_the_restatement(clustered_map):
    """(b) three iterations from the same start and the same CSR: measured E2E_STEP3_MEASURED relative, the bound 4 x that"""
    T = _tsne()
    offsets, cols, vals = clustered_map["csr"]
    got = T.layout(offsets, cols, vals, 512, iters=3, seed=0).y.cpu().double()
    want, _ = R.layout(clustered_map["y0"], offsets.cpu(), cols.cpu(), vals.cpu(), 3)
    rel = float((got - want).abs().max() / want.abs().max())
    print(f"3 iterations: max |y - y64| / max |y64| = {rel:.3e}")
    assert rel <= 4 * E2E_STEP3_MEASURED


def test_map_separates_the_clusters(clustered_map):
    """(c) the KL falls after the exaggeration ends, (d) the 10 nearest map neighbours share the label in >= 0.99 of the cases (sklearn's
    exact TSNE and the float64 restatement both reach 1.00 on this data), (e) the map's KL, re-evaluated in float64, against the float64
    restatement's own final KL from the same start: measured gap E2E_KL_GAP_MEASURED (the f32 and f64 trajectories diverge; equality is
    not expected), the margin 3 x that"""
    result, lab = clustered_map["result"], clustered_map["lab"]
    offsets, cols, vals = (t.cpu() for t in clustered_map["csr"])
    trace = dict(result.kl_trace)
    assert result.kl_trace[-1][0] == 500 and result.kl == result.kl_trace[-1][1] and sorted(trace) == list(range(50, 501, 50))
    assert trace[500] < trace[250]
    purity = R.neighbour_purity(result.y.cpu(), lab, 10)
    y64, _ = R.layout(clustered_map["y0"], offsets, cols, vals, 500)
    kl_gpu, kl_ref = R.kl_csr(result.y.cpu(), offsets, cols, vals), R.kl_csr(y64, offsets, cols, vals)
    print(f"512 rows, 8 clusters: purity@10 {purity:.4f} (restatement {R.neighbour_purity(y64, lab, 10):.4f}), KL of the GPU map in float64 "
          f"{kl_gpu:.5f}, of the restatement's {kl_ref:.5f}, gap {abs(kl_gpu - kl_ref):.3e}; the GPU's own last KL {result.kl:.5f}")
    assert purity >= 0.99
    assert abs(kl_gpu - kl_ref) <= 3 * E2E_KL_GAP_MEASURED


def test_tsne_of_an_index_with_removed_rows():
    from coati_amd.search import EmbeddingIndex
    x, _ = R.clustered_rows(200, 32, 4, 0.5, seed=2)
    index = EmbeddingIndex(32, metric="l2", device=DEV)
    index.add(x)
    index.remove([0, 17, 199])
    res = index.tsne(perplexity=10.0, iters=20, kl_every=7)
    gone = torch.zeros(200, dtype=torch.bool)
    gone[[0, 17, 199]] = True
    assert res.y.shape == (200, 2) and torch.isnan(res.y[gone]).all() and torch.isfinite(res.y[~gone]).all()
    assert [it for it, _ in res.kl_trace] == [7, 14, 20] and all(math.isfinite(v) for _, v in res.kl_trace)


def test_embed_xy():
    from coati_amd.generative import embed_xy
    x, _ = R.clustered_rows(96, 32, 4, 0.5, seed=1)
    xy = embed_xy(x, iters=60, perplexity=10.0, device=DEV)
    assert xy.shape == (96, 2) and xy.dtype == torch.float32 and torch.isfinite(xy).all()
    records = [{"smiles": f"m{i}", "emb": x[i].numpy()} for i in range(96)]
    again = embed_xy(records, iters=60, perplexity=10.0, device=DEV)
    assert torch.equal(again, xy)                                   # the reference's call is the default: lr = 100, init = "random", seed 0
    assert all(isinstance(r["X"], float) and isinstance(r["Y"], float) for r in records)
    assert [r["X"] for r in records] == xy[:, 0].tolist() and [r["Y"] for r in records] == xy[:, 1].tolist()
