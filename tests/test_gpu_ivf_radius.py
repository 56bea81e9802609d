"""Radius search over inverted lists on the GPU (include/coati_ivf_radius.h, coati_amd/ivf_radius.py, the IVFIndex methods,
coati_amd/generative/coati_search.py) against the float64 restatement of tests/ivf_radius_util.py and against the exact radius search
(EmbeddingIndex.radius_search / near_duplicates / dedup).  Integer data is exact in bf16 and in f32 in any summation order, so those
cases must EQUAL the oracle element for element: offsets, rows and score bits.  Real-valued data is pinned to the exact kernel's bits.

The lists are test_gpu_ivf.py's, given by hand: N = 3000 rows in L = 7 lists -- list 0 empty, list 1 one row, list 2 15 rows, list 3 150
rows (three segments at seg_rows = 64), list 4 203 rows (not a multiple of 16), lists 5 and 6 1200 and 1431 rows (23 segments) --
interleaved over the library, so that position order is not row order."""
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
from tests import ivf_radius_util as IR  # noqa: E402
from tests import radius_util as R  # noqa: E402
from tests.gpu_util import log  # noqa: E402
from tests.search_util import canon as _canon, ints as _ints, strings as _strings  # noqa: E402

DEV = "cuda:0"
INF = float("inf")
N, L = 3000, 7
SIZES = [0, 1, 15, 150, 203, 1200, 1431]
ONE_SEGMENT = 1472                                   # the longest list in one segment: the next multiple of 64
SMALL = dict(n_layer_e3gnn=2, n_layer_xformer=2, n_hidden_xformer=64, n_hidden_e3nn=64, n_embd_common=64, n_head=4, n_seq=24, n_tok=48)


def _hand_assign(seed=0):
    a = torch.cat([torch.full((n,), l, dtype=torch.int32) for l, n in enumerate(SIZES)])
    return a[torch.randperm(N, generator=torch.Generator().manual_seed(seed))]


_BUILT = {}


def _hand_index(dim, metric="l2", gaussian=False):
    """(EmbeddingIndex, IVFIndex) over N rows of width dim with the lists given by hand; built once per (dim, metric, kind).  Integer data
    under "cosine": the l2 index's integer rows stored as they are with a bias of 0 (EmbeddingIndex would normalise them), for the
    alpha = 1 form of the score on exact data; there is no EmbeddingIndex of it."""
    key = (dim, metric, gaussian)
    if key not in _BUILT:
        from coati_amd.search import EmbeddingIndex
        from coati_amd.ivf import IVFIndex
        if metric == "cosine" and not gaussian:
            _, l2 = _hand_index(dim)
            _BUILT[key] = (None, IVFIndex(dim, l2.dim_padded, "cosine", N, l2.centres, l2.vectors, l2.ids, torch.zeros_like(l2.bias), l2.sizes, DEV))
            return _BUILT[key]
        g = torch.Generator().manual_seed(100 + dim)
        x = torch.randn(N, dim, generator=g) if gaussian else _ints((N, dim), 100 + dim)
        index = EmbeddingIndex(dim, metric=metric, device=DEV)
        index.add(x)
        ivf = IVFIndex.build(index, L, centres=torch.randn(L, dim, generator=g), assign=_hand_assign())
        assert ivf.sizes.tolist() == SIZES and len(ivf) == N and ivf.nlist == L
        _BUILT[key] = (index, ivf)
    return _BUILT[key]


def _queries(Q, dim, seed, metric):
    """integer queries; under "cosine" 16 entries of +-1 per query: the norm is 4 and the prepared query +-0.25, exact in bf16"""
    if metric == "l2":
        return _ints((Q, dim), seed)
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros(Q, dim)
    for i in range(Q):
        q[i, torch.randperm(dim, generator=g)[:16]] = (2 * torch.randint(0, 2, (16,), generator=g) - 1).float()
    return q


def _tables(Q, seed):
    """probe tables [Q, n] for n in 1, 3, L: every row a seeded choice of distinct lists (the empty list among them), some entries -1,
    the last query probing nothing when Q > 1"""
    g = torch.Generator().manual_seed(seed)
    perm = torch.stack([torch.randperm(L, generator=g) for _ in range(Q)])
    out = []
    for n in (1, 3, L):
        t = perm[:, :n].clone()
        if n > 1:
            t[torch.rand(Q, n, generator=g) < 0.2] = -1
            if Q > 1:
                t[-1] = -1
        out.append(t)
    return out


def _oracle(ivf, q, probes, thr, row_below=None):
    """ivf_radius_util.csr on the stored operands: (offsets, scores float64, rows), row ascending, and the masked score matrix"""
    from coati_amd import search as S
    _, q16 = S.prepare_queries(q, ivf.metric, ivf.dim, DEV)
    args = (ivf.vectors, ivf.ids, ivf.bias, ivf.list_offsets, q16, probes, N)
    kw = dict(alpha=S.metric_alpha(ivf.metric), l2=ivf.metric == "l2")
    return IR.csr(*args, thr, row_below, **kw) + (IR.masked_scores(*args, **kw),)


def _mixed_thresholds(s):
    """per query, in turn: -inf (every live probed row: all 64 rows of an iteration hit), +inf (no row), the 30th best of the query's
    probed scores (0 where it probes fewer rows): some hits, ties at the threshold kept by >="""
    Q = s.shape[0]
    ranked = s.sort(dim=1, descending=True).values
    mid = torch.where(ranked[:, 29] > -INF, ranked[:, 29], torch.zeros(Q, dtype=s.dtype))
    kinds = torch.arange(Q) % 3
    return torch.where(kinds == 0, torch.full_like(mid, -INF), torch.where(kinds == 1, torch.full_like(mid, INF), mid)).float()


def _same(got, want, label):
    (o, s, r), (wo, ws, wr) = got, want
    assert o.dtype == torch.int64 and s.dtype == torch.float32 and r.dtype == torch.int64, label
    assert o.shape == wo.shape and torch.equal(o.cpu(), wo), (label, o.tolist()[:8], wo.tolist()[:8])
    assert s.shape == r.shape == wr.shape, label
    bad_r, bad_s = int((r.cpu() != wr).sum()), int((s.double().cpu() != ws).sum())
    log(f"ivf radius {label}: {r.numel()} hits, {bad_r} rows and {bad_s} scores differ from the oracle")
    assert bad_r == 0 and bad_s == 0, label


def _same_bits(got, want, label):
    for a, b, name in zip(got, want, ("offsets", "scores", "rows")):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (label, name)


# ---- 1. integer data against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("dim,Q", [(32, 1), (32, 40), (90, 17), (256, 40), (512, 17)])
def test_integer_data_equals_the_oracle(dim, Q, metric):
    _, ivf = _hand_index(dim, metric)
    q = _queries(Q, dim, 7 * Q + dim, metric)
    for t in _tables(Q, Q + dim):
        full = _oracle(ivf, q, t, -INF)[3]
        thr = _mixed_thresholds(full)
        wo, ws, wr, _ = _oracle(ivf, q, t, thr)
        counts = (wo[1:] - wo[:-1]).tolist()
        probed = [sum(SIZES[l] for l in row if l >= 0) for row in t.tolist()]
        assert counts[0::3] == probed[0::3] and not any(counts[1::3])                        # -inf: every probed row; +inf: none
        by = {"row": (ws, wr), "score": R.by_score(wo, ws, wr), "probe": IR.in_probe_order(wo, ws, wr, t, ivf.ids, ivf.list_offsets, N)}
        if t.shape[1] == L and Q > 1:
            assert not torch.equal(by["probe"][1], wr) and not torch.equal(by["score"][1], wr)
        for seg_rows in (64, ONE_SEGMENT):
            for blocks in (1, 0):
                for order in ("row", "score", "probe"):
                    got = ivf.radius_search(q, thr, probes=t, order=order, seg_rows=seg_rows, blocks=blocks)
                    _same(got, (wo,) + by[order], f"{metric} dim={dim} Q={Q} nprobe={t.shape[1]} seg_rows={seg_rows} blocks={blocks} {order}")
        c = ivf.radius_count(q, thr, probes=t)
        assert c.dtype == torch.int64 and c.tolist() == counts
        assert counts[-1] == 0 or Q == 1 or t.shape[1] == 1                                  # a query that probes nothing


# ---- 2. row bounds -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_row_bounds_and_the_segment_exit(metric):
    """bounds of 0, 1500 and N in turn; then 1500 for every query -- at seg_rows = 64 the later segments of the long lists begin above
    every bound of their group and are skipped whole -- and 0 for every query, where every item is"""
    _, ivf = _hand_index(96, metric)
    Q = 40
    q = _queries(Q, 96, 11, metric)
    full_table = torch.arange(L).repeat(Q, 1)
    for t in (full_table, _tables(Q, 12)[1]):
        for below in (torch.tensor([[0, 1500, N][i % 3] for i in range(Q)]), torch.full((Q,), 1500), torch.zeros(Q, dtype=torch.int64)):
            for thr, name in ((-INF, "-inf"), (_mixed_thresholds(_oracle(ivf, q, t, -INF)[3]), "mixed")):
                want = _oracle(ivf, q, t, thr, below)[:3]
                assert bool((want[2] < below[torch.repeat_interleave(torch.arange(Q), want[0][1:] - want[0][:-1])]).all())
                for seg_rows in (64, ONE_SEGMENT, None):
                    got = ivf.radius_search(q, thr, probes=t, row_below=below, seg_rows=seg_rows)
                    _same(got, want, f"{metric} row_below={below.tolist()[:3]} thr={name} nprobe={t.shape[1]} seg_rows={seg_rows}")
                assert ivf.radius_count(q, thr, probes=t, row_below=below).tolist() == (want[0][1:] - want[0][:-1]).tolist()
    # the long lists hold rows below 1500 in their first segments only: ids ascend inside a list
    assert int(ivf.list_rows(6)[64 * 12]) > 1500


# ---- 3. removed rows and infinite thresholds -----------------------------------------------------------------------------------------------------
def test_removed_rows_and_infinite_thresholds():
    from coati_amd.ivf import IVFIndex
    index, _ = _hand_index(96)
    ivf = IVFIndex.build(index, L, centres=torch.randn(L, 96, generator=torch.Generator().manual_seed(1)), assign=_hand_assign())
    Q = 17
    q = _ints((Q, 96), 21)
    t = torch.arange(L).repeat(Q, 1)
    o, s, r = ivf.radius_search(q, -INF, probes=t)
    assert o.tolist() == [i * N for i in range(Q + 1)] and torch.equal(r.cpu(), torch.arange(N).repeat(Q))
    gone = torch.cat([ivf.list_rows(1), ivf.list_rows(3)[:2], ivf.list_rows(6)[63:66], ivf.list_rows(6)[-1:]]).cpu()
    ivf.remove(gone)
    assert len(ivf) == N
    for thr, name in ((-INF, "-inf"), (_mixed_thresholds(_oracle(ivf, q, t, -INF)[3]), "mixed")):
        want = _oracle(ivf, q, t, thr)[:3]
        for order in ("row", "probe"):
            got = ivf.radius_search(q, thr, probes=t, order=order, seg_rows=64)
            assert not set(gone.tolist()) & set(got[2].tolist())
            if order == "row":
                _same(got, want, f"7 rows removed thr={name}")
        assert torch.equal(ivf.radius_count(q, thr, probes=t), got[0][1:] - got[0][:-1])
    o, s, r = ivf.radius_search(q, -INF, probes=t)
    assert o.tolist() == [i * (N - 7) for i in range(Q + 1)]
    o, s, r = ivf.radius_search(q, INF, probes=t)
    assert o.tolist() == [0] * (Q + 1) and s.numel() == r.numel() == 0
    assert ivf.radius_count(q, INF, probes=t).tolist() == [0] * Q


# ---- 4, 5. real-valued data against the exact radius search ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [256, 512])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_all_lists_equal_the_exact_radius_search_bitwise(metric, dim):
    """every live row is in one probed list and a row's MFMA sequence is the same in both kernels: offsets, rows and score BITS equal"""
    index, ivf = _hand_index(dim, metric, True)
    q = torch.randn(40, dim, generator=torch.Generator().manual_seed(5 + dim))
    thr = index.search(q, 40)[0][:, 39].clone()
    for order in ("row", "score"):
        want = index.radius_search(q, thr, order=order)
        assert bool((want[0][1:] - want[0][:-1] >= 40).all())
        got = ivf.radius_search(q, thr, nprobe=L, order=order)
        _same_bits(got, want, f"all lists {metric} dim={dim} {order}")
    assert torch.equal(ivf.radius_count(q, thr, nprobe=L), index.radius_count(q, thr))


@pytest.mark.parametrize("dim", [256, 512])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_coarse_probes_equal_the_exact_search_filtered_to_the_probed_lists(metric, dim):
    index, ivf = _hand_index(dim, metric, True)
    Q = 17
    q = torch.randn(Q, dim, generator=torch.Generator().manual_seed(9 + dim))
    thr = index.search(q, 128)[0][:, 127].clone()
    o, s, r, probes = ivf.radius_search(q, thr, nprobe=3, return_probes=True)
    assert torch.equal(probes, ivf.probe(q, 3)) and bool((probes >= 0).all())
    wo, ws, wr = index.radius_search(q, thr)
    qi = torch.repeat_interleave(torch.arange(Q, device=DEV), wo[1:] - wo[:-1])
    inside = (_hand_assign().to(DEV)[wr].long()[:, None] == probes[qi]).any(dim=1)
    fo = torch.zeros(Q + 1, dtype=torch.int64, device=DEV)
    fo[1:] = torch.bincount(qi[inside], minlength=Q).cumsum(0)
    log(f"ivf radius {metric} dim={dim} nprobe=3: {int(inside.sum())} of the exact search's {wr.numel()} hits are in probed lists")
    assert 0 < int(inside.sum()) < wr.numel()
    _same_bits((o, s, r), (fo, ws[inside], wr[inside]), f"nprobe=3 {metric} dim={dim}")


# ---- 6, 7. chunks of queries, max_results -------------------------------------------------------------------------------------------------------
def test_query_chunks_give_the_same_result(monkeypatch):
    """the count table of a call stays within a scratch budget: with the budget cut to 7 queries' worth, 40 queries go in six chunks"""
    from coati_amd import ivf_radius as mod
    _, ivf = _hand_index(96)
    Q = 40
    q = _ints((Q, 96), 78)
    t = _tables(Q, 79)[1]
    thr = _mixed_thresholds(_oracle(ivf, q, t, -INF)[3])
    below = torch.tensor([[N, 1500][i % 2] for i in range(Q)])
    whole = {order: ivf.radius_search(q, thr, probes=t, order=order, row_below=below, seg_rows=128) for order in ("row", "score", "probe")}
    _same(whole["row"], _oracle(ivf, q, t, thr, below)[:3], "one chunk")
    counts = ivf.radius_count(q, thr, probes=t, row_below=below)
    segs = -(-max(SIZES) // 128)
    monkeypatch.setattr(mod, "SCRATCH_BYTES", 7 * 3 * segs * 4)
    for order in whole:
        _same_bits(ivf.radius_search(q, thr, probes=t, order=order, row_below=below, seg_rows=128), whole[order], f"six chunks {order}")
    monkeypatch.setattr(mod, "SCRATCH_BYTES", 7 * 3 * -(-max(SIZES) // ivf.plan(Q, 3, 1)) * 4)
    assert torch.equal(ivf.radius_count(q, thr, probes=t, row_below=below), counts)
    with pytest.raises(ValueError, match="results so far exceed max_results=10"):
        ivf.radius_search(q, -INF, probes=t, seg_rows=128, max_results=10)


def test_max_results_is_checked_before_the_result_is_allocated():
    _, ivf = _hand_index(32)
    q = _ints((3, 32), 5)
    t = torch.arange(L).repeat(3, 1)
    with pytest.raises(ValueError, match="9000 results exceed max_results=8999"):
        ivf.radius_search(q, -INF, probes=t, max_results=8999)
    assert ivf.radius_search(q, -INF, probes=t, max_results=9000)[2].numel() == 9000


# ---- 8. the self-join ------------------------------------------------------------------------------------------------------------------------------
def _library_with_copies(E=64, signs=False):
    """1200 integer base rows (entries in -4 .. 4; signs: in {-1, 1}), exact copies of 480 of them and copies scaled by 2 of 480 (240
    have both), shuffled with a fixed seed: (2160 rows, origin of each)"""
    base = 2 * _ints((1200, E), 51, 0, 1) - 1 if signs else _ints((1200, E), 51)
    assert bool((base.abs().sum(dim=1) > 0).all())
    x = torch.cat([base, base[:480], 2 * base[240:720]])
    origin = torch.cat([torch.arange(1200), torch.arange(480), torch.arange(240, 720)])
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(52))
    return x[perm], origin[perm]


def _first_occurrences(keys):
    seen, first = set(), []
    for o in keys:
        first.append(o not in seen)
        seen.add(o)
    return first


def _pairs(csr, n):
    """the CSR's (row, neighbour) pairs as sorted int64 keys, and its scores in that order (the CSR is row-major, rows ascending)"""
    o, s, r = csr
    keys = torch.repeat_interleave(torch.arange(n, device=o.device), o[1:] - o[:-1]) * n + r
    assert bool((keys[1:] > keys[:-1]).all())
    return keys, s


def _copies(metric):
    """(metric, EmbeddingIndex, its ivf(8), the first occurrences, the thresholds: one only exact copies reach, one that many pairs reach).
    Cosine on rows of +-1: stored +-1/8, a copy (scaled or not) scores exactly 1 and every score is a multiple of 1/64; l2 on integers: a
    copy is at distance 0, every score an integer.  All of it exact, in any summation order."""
    from coati_amd.search import EmbeddingIndex
    x, origin = _library_with_copies(signs=metric == "cosine")
    index = EmbeddingIndex(64, metric=metric, device=DEV)
    index.add(x)
    ivf = index.ivf(8, iters=5, seed=1)
    assert len(ivf) == x.shape[0] == 2160 and int(ivf.sizes.sum()) == 2160
    keys = origin.tolist() if metric == "cosine" else [tuple(v) for v in x.tolist()]
    return metric, index, ivf, _first_occurrences(keys), ((0.999, 0.25) if metric == "cosine" else (-0.5, -600.0))


@pytest.fixture(scope="module", params=["cosine", "l2"])
def copies(request):
    """shared by the tests that leave it as it is"""
    return _copies(request.param)


def test_self_join_against_the_exact_one(copies):
    metric, index, ivf, first, (tight, wide) = copies
    n = len(index)
    sizes = {}
    for thr in (tight, wide):
        exact = index.near_duplicates(thr)
        _same_bits(ivf.near_duplicates(thr, nprobe=8), exact, f"self-join {metric} thr={thr} nprobe=8")
        _same_bits(ivf.near_duplicates(thr, nprobe=8, chunk=500), exact, f"self-join {metric} thr={thr} nprobe=8 chunk=500")
        ekeys, escores = _pairs(exact, n)
        seen = []
        for nprobe in (1, 2, 4, 8):
            keys, scores = _pairs(ivf.near_duplicates(thr, nprobe=nprobe), n)
            at = torch.searchsorted(ekeys, keys).clamp_max(max(ekeys.numel() - 1, 0))
            assert torch.equal(ekeys[at], keys) and torch.equal(escores[at], scores), (thr, nprobe)      # a subset, the same score bits
            seen.append(keys.numel())
        assert seen == sorted(seen) and seen[-1] == ekeys.numel()
        sizes[thr] = seen
        log(f"ivf self-join {metric} thr={thr}: pairs found at nprobe 1, 2, 4, 8 = {seen} of {ekeys.numel()}")
    # bit-identical rows are stored in one list, and a row's own list is always probed: nprobe = 1 finds every such pair
    assert sizes[tight][0] == sizes[tight][-1] > 0 and sizes[wide][0] < sizes[wide][-1]


def test_dedup_against_the_exact_one(copies):
    metric, index, ivf, first, (tight, wide) = copies
    for thr in (tight, wide):
        keep = ivf.dedup(thr, nprobe=8)
        assert keep.dtype == torch.bool and keep.shape == (len(index),) and torch.equal(keep, index.dedup(thr))
    keep = ivf.dedup(tight, nprobe=1)
    assert keep.tolist() == first and torch.equal(keep, index.dedup(tight))
    # at nprobe = 1 and the wide threshold: every dropped row is within the threshold of a kept one
    keep = ivf.dedup(wide, nprobe=1).cpu()
    o, _, r = (v.cpu() for v in index.near_duplicates(wide))
    o2, _, r2 = (v.cpu() for v in ivf.near_duplicates(wide, nprobe=1))
    for i in (~keep).nonzero().reshape(-1).tolist():
        assert bool(keep[r2[o2[i]:o2[i + 1]]].any()) and bool(keep[r[o[i]:o[i + 1]]].any()), i


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_self_join_after_remove(metric):
    """removed rows are neither queries nor hits (an index of its own: the rows are removed from both)"""
    metric, index, ivf, first, (tight, wide) = _copies(metric)
    before = ivf.near_duplicates(wide, nprobe=2)
    gone = torch.cat([before[2][:5].cpu(), torch.tensor([0, 7, 2159])]).unique().to(DEV)
    index.remove(gone)
    ivf.remove(gone)
    for nprobe in (2, 8):
        o, s, r = ivf.near_duplicates(wide, nprobe=nprobe)
        assert not set(gone.tolist()) & set(r.tolist()) and (o[gone + 1] - o[gone]).tolist() == [0] * gone.numel()
    _same_bits((o, s, r), index.near_duplicates(wide), f"self-join {metric} after remove")
    keep = ivf.dedup(wide, nprobe=8)
    assert torch.equal(keep, index.dedup(wide)) and not bool(keep[gone].any())


# ---- 9. streams -------------------------------------------------------------------------------------------------------------------------------------
def test_a_side_stream_gives_the_same_result():
    _, ivf = _hand_index(90)
    q = _ints((19, 90), 31)
    want = ivf.radius_search(q, -1000.0, nprobe=3, order="score")
    counts = ivf.radius_count(q, -1000.0, nprobe=3)
    assert int(want[0][-1]) > 0
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ivf.radius_search(q.to(DEV), -1000.0, nprobe=3, order="score")
        got_counts = ivf.radius_count(q.to(DEV), -1000.0, nprobe=3)
    side.synchronize()
    _same_bits(got, want, "side stream")
    assert torch.equal(got_counts, counts)
    one = ivf.radius_search(q[0], -1000.0, nprobe=3, order="score")                       # one vector is one query
    assert one[0].tolist() == want[0][:2].tolist() and torch.equal(one[2], want[2][:int(want[0][1])])


# ---- 10. the strings layer ----------------------------------------------------------------------------------------------------------------------------
def test_smiles_within_through_an_ivf_index(golden_dir):
    from coati.generative import build_index, smiles_within
    from coati_amd.ivf import IVFIndex
    from coati_amd.models.encoding.clip_e2e import e3gnn_smiles_clip_e2e
    from coati_amd.models.encoding.tokenizers import TrieTokenizer
    gold = np.load(os.path.join(golden_dir, "generative_golden.npz"))
    voc = json.load(open(os.path.join(golden_dir, "tokenizer.json")))
    tk = TrieTokenizer(n_seq=int(gold["n_seq"]), smiles_tokens=voc["smiles"], special_tokens=voc["special"])
    with contextlib.redirect_stdout(io.StringIO()):
        model = e3gnn_smiles_clip_e2e(**SMALL, device=torch.device(DEV))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "small_model_after3.npz")).items()}, strict=False)
    strings = _strings([t for t in voc["smiles"] if t.isascii() and "X" not in t], 40, 5)
    with contextlib.redirect_stdout(io.StringIO()):
        ivf, kept = build_index(strings, model, tk, batch_size=16, canon_smiles=_canon, nlist=4)
        exact, kept2 = build_index(strings, model, tk, batch_size=16, canon_smiles=_canon)
    assert isinstance(ivf, IVFIndex) and kept == kept2 == strings and ivf.nlist == 4
    for thr in (0.9, -1.5):
        with contextlib.redirect_stdout(io.StringIO()):
            near = smiles_within(kept + ["CXC"], ivf, kept, model, tk, threshold=thr, canon_smiles=_canon)
            want = smiles_within(kept + ["CXC"], exact, kept, model, tk, threshold=thr, canon_smiles=_canon)
        assert near == want and near[-1] == [] and all(hits and hits[0][0] == s for s, hits in zip(kept, near))   # the default nprobe covers the four lists
    assert all(len(hits) == 40 for hits in near[:-1])


def test_drop_near_duplicates_through_an_ivf_index_then_search_never_returns_a_dropped_row():
    from coati.generative import drop_near_duplicates
    from coati_amd.ivf import IVFIndex
    x, origin = _library_with_copies(signs=True)
    _, index, ivf, first, _ = _copies("cosine")
    kept =[f"s{i}" for i in range(len(index))]
    stay = drop_near_duplicates(index, kept, 0.999, ivf=ivf, nprobe=1)
    assert stay == [i for i, f in enumerate(first) if f] and len(index) == len(ivf) == x.shape[0]
    assert int((index.bias == -INF).sum()) == int((ivf.bias == -INF).sum()) == x.shape[0] - len(stay)
    for r in (index.search(x, 10)[1], ivf.search(x, 10, nprobe=2)[1]):
        assert bool((r[:, 0] >= 0).all()) and set(r[r >= 0].tolist()) <= set(stay)
    first_of = {origin[j].item(): j for j in stay}
    assert index.search(x, 1)[1][:, 0].tolist() == [first_of[o] for o in origin.tolist()]  # every row finds its group's first
    short = IVFIndex(64, 64, "cosine", 5, torch.zeros(1, 64), ivf.vectors[:5], torch.arange(5), ivf.bias[:5], torch.tensor([5]), DEV)
    with pytest.raises(ValueError, match="ivf of 5 rows"):
        drop_near_duplicates(index, kept, 0.999, ivf=short)
