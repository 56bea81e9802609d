"""Radius search on the GPU (include/coati_radius.h, coati_amd/radius.py, the EmbeddingIndex methods, coati_amd/generative/coati_search.py)
against the float64 restatement of tests/radius_util.py.  Integer data is exact in bf16 and in f32 in any summation order, so those cases
must EQUAL the oracle element for element: offsets, rows and score bits.  Real-valued data is pinned to the exact search's own bits, and
held to test_gpu_search.py's f32-accumulation bound against float64 with thresholds placed where no row is undecided."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import radius_util as R  # noqa: E402
from tests import search_util  # noqa: E402
from tests.gpu_util import log  # noqa: E402
from tests.search_util import canon as _canon, ints as _ints, strings as _strings  # noqa: E402

DEV = "cuda:0"
INF = float("inf")
SMALL = dict(n_layer_e3gnn=2, n_layer_xformer=2, n_hidden_xformer=64, n_hidden_e3nn=64, n_embd_common=64, n_head=4, n_seq=24, n_tok=48)


def _index(vectors, metric="dot", **kw):
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(vectors.shape[1], metric=metric, device=DEV, **kw)
    assert index.add(vectors) == range(0, vectors.shape[0])
    return index


def _same(got, want, label):
    """a radius result == the oracle's, element for element (score bits: the oracle's float64 values are f32 values here)"""
    (o, s, r), (wo, ws, wr) = got, want
    assert o.dtype == torch.int64 and s.dtype == torch.float32 and r.dtype == torch.int64, label
    assert o.shape == wo.shape and torch.equal(o, wo), (label, o.tolist()[:8], wo.tolist()[:8])
    assert s.shape == r.shape == wr.shape, label
    bad_r, bad_s = int((r != wr).sum()), int((s.double() != ws).sum())
    log(f"radius {label}: {r.numel()} hits, {bad_r} rows and {bad_s} scores differ from the oracle")
    assert bad_r == 0 and bad_s == 0, label


def _exact(index, q, thr, label, row_below=None, **kw):
    """radius_search == oracle, and radius_count == the offsets' differences; returns the result"""
    got = index.radius_search(q, thr, row_below=row_below, **kw)
    wo, ws, wr, _ = R.index_radius(index, q, thr, row_below)
    _same(got, (wo, ws, wr), label)
    counts = index.radius_count(q, thr, row_below=row_below)
    assert counts.dtype == torch.int64 and torch.equal(counts, got[0][1:] - got[0][:-1]), label
    return got


def _mixed_thresholds(full):
    """per query, in turn: the oracle's best score (ties at the threshold are kept by >=), its rank-37 score, below its minimum (every
    row), above its maximum (no row)"""
    Q, N = full.shape
    ranked = full.sort(dim=1, descending=True).values
    kinds = torch.arange(Q, device=full.device) % 4
    choice = torch.stack([ranked[:, 0], ranked[:, min(37, N - 1)], ranked[:, -1] - 1.0, ranked[:, 0] + 1.0], dim=1)
    return choice.gather(1, kinds[:, None])[:, 0]


# ---- 1. shapes ----------------------------------------------------------------------------------------------------------------------
# N in {1, 15, 16, 17, 63, 64, 65, 1000, 70001}, Q in {1, 15, 16, 17, 64, 65, 130}, E in {32, 96, 256, 512}
SHAPES = [(1, 1, 32), (1, 17, 256), (15, 15, 96), (16, 16, 256), (17, 17, 512), (63, 64, 32), (64, 65, 96), (65, 130, 256), (1000, 17, 512),
          (1000, 130, 256), (1000, 64, 96), (70001, 16, 256), (70001, 65, 512), (70001, 1, 96), (70001, 130, 32)]


@pytest.mark.parametrize("metric", ["dot", "l2"])
@pytest.mark.parametrize("N,Q,E", SHAPES)
def test_integer_data_equals_the_oracle(N, Q, E, metric):
    index = _index(_ints((N, E), 1000 + N + E), metric=metric)
    q = _ints((Q, E), 7 * Q + E)
    thr = _mixed_thresholds(search_util.index_scores(index, q))
    o, s, r = _exact(index, q, thr, f"{metric} N={N} Q={Q} E={E}")
    counts = (o[1:] - o[:-1]).tolist()
    assert all(c >= 1 for c in counts[0::4]) and all(c == N for c in counts[2::4]) and all(c == 0 for c in counts[3::4])
    if metric == "l2":
        # the rows search() returns too carry search()'s bits
        k = min(128, N)
        ss, sr = index.search(q, k)
        dense = torch.full((Q, N), float("nan"), device=DEV)
        dense[torch.repeat_interleave(torch.arange(Q, device=DEV), o[1:] - o[:-1]), r] = s
        mine = dense.gather(1, sr.clamp_min(0))
        both = (sr >= 0) & ~mine.isnan()
        assert bool(both.any()) and torch.equal(mine[both], ss[both])


# ---- 2. adversarial layouts ------------------------------------------------------------------------------------------------------------
def _layout(kind, N=5000):
    """three queries q = (64, 1, 0, ...) and rows (a, b, 0, ...): score = 64 a + b, exact; (library, threshold, the rows that hit)"""
    n = torch.arange(N)
    x = torch.zeros(N, 32)
    if kind == "constant":                   # every row hits: every bit of every mask is set
        x[:, 0] = 1
        return x, 64.0, n
    if kind == "blocks":                     # blocks of 100 alternating
        x[:, 1] = (n // 100) % 2
        return x, 1.0, n[(n // 100) % 2 == 1]
    if kind == "first":
        x[0, 0] = 1
        return x, 64.0, n[:1]
    if kind == "last":                       # in the ragged last slab: 5000 = 78 * 64 + 8
        x[N - 1, 0] = 1
        return x, 64.0, n[N - 1:]
    assert kind == "last_slice"              # 7 slices of 768 rows: the last one begins at row 4608
    x[4608:, 0] = 1
    return x, 64.0, n[4608:]


@pytest.mark.parametrize("kind", ["constant", "blocks", "first", "last", "last_slice"])
def test_adversarial_layouts(kind):
    x, thr, hits = _layout(kind)
    N, Q = x.shape[0], 3
    index = _index(x)
    q = torch.zeros(Q, 32)
    q[:, 0], q[:, 1] = 64, 1
    for slices in (1, 7, None):
        o, s, r = _exact(index, q, thr, f"{kind} slices={slices}", slices=slices)
        assert o.tolist() == [i * hits.numel() for i in range(Q + 1)]
        assert torch.equal(r.cpu(), hits.repeat(Q))
    if kind == "constant":
        assert o.tolist() == [i * N for i in range(Q + 1)]


# ---- 3. geometry -------------------------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_the_slices():
    from coati_amd import _lib
    N, Q, E = 70001, 17, 96
    index, q = _index(_ints((N, E), 3)), _ints((Q, E), 4)
    full = search_util.index_scores(index, q)
    thr = _mixed_thresholds(full)
    want = R.csr_of(full, thr)
    default = _lib.lib().coati_radius_slices(N, Q)
    assert default == 512
    for slices in (1, 2, 7, None, default, 4000):                 # 4000 slices of 64 rows: the last 2906 lie past the library's end
        got = index.radius_search(q, thr, slices=slices)
        _same(got, want, f"slices={slices}")
        again = index.radius_search(q, thr, slices=slices)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), slices
    assert torch.equal(index.radius_count(q, thr), want[0][1:] - want[0][:-1])
    by_score = index.radius_search(q, thr, order="score")
    ws, wr = R.by_score(*want)
    assert torch.equal(by_score[0], want[0]) and torch.equal(by_score[2], wr) and torch.equal(by_score[1].double(), ws)


# ---- 4. thresholds, removal and row bounds --------------------------------------------------------------------------------------------------
def test_infinite_thresholds_and_removal():
    N, Q, E = 1000, 21, 64
    index, q = _index(_ints((N, E), 5)), _ints((Q, E), 6)
    o, s, r = _exact(index, q, -INF, "thr=-inf")
    assert o.tolist() == [i * N for i in range(Q + 1)]
    gone = torch.tensor([0, 1, 63, 64, 500, 999])
    index.remove(gone)
    o, s, r = _exact(index, q, -INF, "thr=-inf, 6 rows removed")
    assert o.tolist() == [i * (N - 6) for i in range(Q + 1)] and not set(gone.tolist()) & set(r.tolist())
    o, s, r = _exact(index, q, INF, "thr=+inf")
    assert o.tolist() == [0] * (Q + 1) and s.numel() == r.numel() == 0
    thr = torch.tensor([-INF, INF, 0.0] * 7)
    o, s, r = _exact(index, q, thr, "thr mixed")
    assert all(c == N - 6 for c in (o[1:] - o[:-1]).tolist()[0::3]) and all(c == 0 for c in (o[1:] - o[:-1]).tolist()[1::3])
    best = _exact(index, q, 3.0, "before removing the hits")
    index.remove(best[2][best[0][0]:best[0][1]])                   # query 0's hits
    after = _exact(index, q, 3.0, "after removing query 0's hits")
    assert int(best[0][1]) > 0 and int(after[0][1]) == 0


@pytest.mark.parametrize("metric", ["dot", "l2"])
def test_row_bounds_and_the_triangle_exit(metric):
    """tile 0 (queries 0 .. 63): bounds of at most 65, next to tile 1 (64 .. 127) whose largest is N, and tile 2 (128, 129) with none above 0"""
    N, Q, E = 1000, 130, 64
    index, q = _index(_ints((N, E), 8), metric=metric), _ints((Q, E), 9)
    below = torch.tensor([[0, 1, 64, 65][i % 4] for i in range(64)] + [[0, 1, 64, 65, N][i % 5] for i in range(64)] + [0, 0])
    full = search_util.index_scores(index, q)
    for thr, name in ((-INF, "-inf"), (_mixed_thresholds(full), "mixed")):
        for slices in (None, 1, 7):
            o, s, r = _exact(index, q, thr, f"{metric} row_below thr={name} slices={slices}", row_below=below, slices=slices)
            if name == "-inf":
                assert (o[1:] - o[:-1]).tolist() == below.tolist()
    index.remove([0, 64])
    _exact(index, q, -INF, f"{metric} row_below with rows removed", row_below=below)


# ---- 5, 6. real-valued data ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gaussian():
    N, Q, E = 70001, 65, 256
    g = torch.Generator().manual_seed(23)
    index = _index(torch.randn(N, E, generator=g), metric="cosine")
    return index, torch.randn(Q, E, generator=g)


def test_agrees_with_the_exact_search_bit_for_bit(gaussian):
    """pins "the bits of the exact kernel" against search(), which this change does not touch"""
    index, q = gaussian
    s, r = index.search(q, 128)
    thr = s[:, 39].clone()
    prefix = s >= thr[:, None]
    assert bool((prefix.sum(dim=1) < 128).all() and (prefix.sum(dim=1) >= 40).all())       # on the search output alone: nothing is cut at 128
    o, vs, vr = index.radius_search(q, thr, order="score")
    assert torch.equal(o[1:] - o[:-1], prefix.sum(dim=1))
    assert torch.equal(vr, r[prefix]) and torch.equal(vs, s[prefix])                       # row-major: query by query, rank by rank
    assert torch.equal(index.radius_count(q, thr), prefix.sum(dim=1))


def test_gaussian_data_against_float64(gaussian):
    """test_gpu_search.py's bound: u = 2^-23, the f32 sum of E exact bf16 products differs from the exact one by at most
    b = alpha E u |q| |x| in any order.  The threshold of a query sits in the middle of the widest gap between consecutive oracle scores
    among ranks 20 .. 60; that gap exceeds 2 b (asserted on the oracle alone), so no row is undecided."""
    from coati_amd import search as S
    index, q = gaussian
    E = index.dim_padded
    full = search_util.index_scores(index, q)
    _, q16 = S.prepare_queries(q, index.metric, index.dim, DEV)
    b = S.metric_alpha(index.metric) * E * 2.0 ** -23 * q16.double().norm(dim=1, keepdim=True) * index.vectors.double().norm(dim=1)[None, :]
    top = full.topk(61, dim=1).values
    gaps = top[:, 20:60] - top[:, 21:61]
    j = gaps.argmax(dim=1, keepdim=True)
    thr = ((top.gather(1, 20 + j) + top.gather(1, 21 + j)) / 2)[:, 0]
    widest = gaps.gather(1, j)[:, 0]
    log(f"radius gaussian: widest gaps between {float(widest.min()):.3e} and {float(widest.max()):.3e}, bound b up to {float(b.max()):.3e}")
    assert bool((widest > 2 * b.max(dim=1).values).all())         # each side of the threshold is wider than b
    wo, ws, wr = R.csr_of(full, thr)
    o, s, r = index.radius_search(q, thr)
    assert torch.equal(o, wo) and torch.equal(r, wr)
    qi = torch.repeat_interleave(torch.arange(q.shape[0], device=DEV), o[1:] - o[:-1])
    err = (s.double() - ws).abs()
    log(f"radius gaussian: {r.numel()} hits, largest score error {float(err.max()):.3e}")
    assert bool((err <= b[qi, r]).all())


# ---- 7. max_results ----------------------------------------------------------------------------------------------------------------------------
def test_max_results_is_checked_before_anything_is_allocated():
    x, thr, _ = _layout("constant")
    index = _index(x)
    q = torch.zeros(3, 32)
    q[:, 0] = 64
    with pytest.raises(ValueError, match="15000"):
        index.radius_search(q, thr, max_results=14999)
    assert index.radius_search(q, thr, max_results=15000)[2].numel() == 15000


# ---- 8. dedup -----------------------------------------------------------------------------------------------------------------------------------
def _library_with_copies(E=64, signs=False):
    """200 integer base rows (entries in -4 .. 4; signs: in {-1, 1}), exact copies of 80 of them and copies scaled by 2 of 80 (40 have
    both), shuffled with a fixed seed: (rows, origin of each)"""
    base = 2 * _ints((200, E), 51, 0, 1) - 1 if signs else _ints((200, E), 51)
    assert bool((base.abs().sum(dim=1) > 0).all())
    x = torch.cat([base, base[:80], 2 * base[40:120]])
    origin = torch.cat([torch.arange(200), torch.arange(80), torch.arange(40, 120)])
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(52))
    return x[perm], origin[perm]


def _first_occurrences(origin):
    seen, first = set(), []
    for o in origin.tolist():
        first.append(o not in seen)
        seen.add(o)
    return first


def test_dedup_keeps_the_first_occurrences():
    """under cosine a copy scaled by 2 normalises to the same stored bits (x / |x| = 2 x / |2 x| exactly), so a copy scores |x16|^2.  The
    base rows are 64 entries of +-1: |x| = 8, the stored +-1/8 are exact and |x16|^2 = 1 exactly -- bf16-rounded unit rows in general
    have |x16|^2 within 2^-8 of 1, on either side of 0.999.  Distinct rows score a multiple of 1/64 far below; every score is exact, so
    the self-join must equal the oracle bit for bit."""
    x, origin = _library_with_copies(signs=True)
    index = _index(x, metric="cosine")
    N = x.shape[0]
    first = _first_occurrences(origin)
    full = R.self_scores(index)
    same = origin[:, None] == origin[None, :]
    assert bool((full[same.to(DEV)] == 1.0).all() and (full[~same.to(DEV)] <= 0.75).all())
    want = R.index_near_duplicates(index, 0.999)
    for chunk in (4096, 128, 100):
        _same(index.near_duplicates(0.999, chunk=chunk), want, f"near_duplicates cosine chunk={chunk}")
    keep = index.dedup(0.999)
    assert keep.dtype == torch.bool and keep.shape == (N,) and keep.tolist() == first
    assert keep.tolist() == R.greedy(want[0], want[2], [True] * N)


def test_near_duplicates_l2_exact_and_removed_rows():
    """integer rows under l2: distinct rows are at squared distance >= 1, so a threshold of -0.5 finds the exact copies only, and every score
    is exact: the self-join must equal the oracle bit for bit, sub = |x|^2 included"""
    x, origin = _library_with_copies()
    index = _index(x, metric="l2")
    index.remove([3, 77, 78])
    for thr in (-0.5, -40.0):
        want = R.index_near_duplicates(index, thr)
        for chunk in (4096, 64):
            _same(index.near_duplicates(thr, chunk=chunk), want, f"near_duplicates l2 thr={thr} chunk={chunk}")
    keep = index.dedup(-0.5)
    want = R.index_near_duplicates(index, -0.5)
    live = (index.bias > -INF).tolist()
    assert keep.tolist() == R.greedy(want[0], want[2], live) and not any(keep[i] for i in (3, 77, 78))


def test_drop_near_duplicates_then_search_never_returns_a_dropped_row():
    from coati.generative import drop_near_duplicates
    x, origin = _library_with_copies(signs=True)
    index = _index(x, metric="cosine")
    kept = [f"s{i}" for i in range(len(index))]
    stay = drop_near_duplicates(index, kept, 0.999)
    first = _first_occurrences(origin)
    assert stay == [i for i, f in enumerate(first) if f] and len(index) == x.shape[0]
    s, r = index.search(x, 10)
    assert bool((r >= 0).all()) and set(r.flatten().tolist()) <= set(stay)
    first_of = {origin[j].item(): j for j in stay}
    assert r[:, 0].tolist() == [first_of[o] for o in origin.tolist()]                      # every row finds its group's first
    with pytest.raises(ValueError):
        drop_near_duplicates(index, kept[:-1], 0.999)


def test_smiles_within_end_to_end(golden_dir):
    from coati.generative import build_index, smiles_within
    from coati_amd.generative import coati_density
    from coati_amd.models.encoding.clip_e2e import e3gnn_smiles_clip_e2e
    from coati_amd.models.encoding.tokenizers import TrieTokenizer
    g = np.load(os.path.join(golden_dir, "generative_golden.npz"))
    voc = json.load(open(os.path.join(golden_dir, "tokenizer.json")))
    tk = TrieTokenizer(n_seq=int(g["n_seq"]), smiles_tokens=voc["smiles"], special_tokens=voc["special"])
    with contextlib.redirect_stdout(io.StringIO()):
        model = e3gnn_smiles_clip_e2e(**SMALL, device=torch.device(DEV))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "small_model_after3.npz")).items()}, strict=False)
    strings = _strings([t for t in voc["smiles"] if t.isascii() and "X" not in t], 40, 5)
    with contextlib.redirect_stdout(io.StringIO()):
        index, kept = build_index(strings, model, tk, batch_size=16, canon_smiles=_canon)
        emb = coati_density._batch_embeds(kept, model, tk, _canon)
    assert kept == strings
    for thr in (0.9, -1.5):
        with contextlib.redirect_stdout(io.StringIO()):
            within = smiles_within(kept + ["CXC"], index, kept, model, tk, threshold=thr, canon_smiles=_canon)
        counts = index.radius_count(emb, thr).tolist()
        assert len(within) == len(kept) + 1 and within[-1] == []
        for sm, hits, c in zip(kept, within, counts):
            assert len(hits) == c >= 1 and hits[0][0] == sm, (sm, hits[:3], c)
            assert [v for _, v in hits] == sorted((v for _, v in hits), reverse=True)
    assert all(len(hits) == 40 for hits in within[:-1])             # a cosine is never below -1.5
