"""IVF search over fp8 lists on the GPU (include/coati_ivf8.h, coati_amd/ivf8.py).  Integers of magnitude <= 15 are e4m3 values, so on
such data stage 1 must EQUAL the bf16 IVF search and the float64 oracle of tests/ivf_util.py element for element, ties and padding
included; on real-valued data stage 1 is held to the f32 accumulation bound against tests/ivf8_util.scan8, and the two stages to
IVFIndex.search bit for bit.

The hand-made lists: 12 lists of 0, 1, 15, 16, 17, 63, 64, 65, 129, 200, 0 and 449 rows (every remainder of the 16-row slab and the
64-row iteration, a 449-row list whose last segment has one row), two rows in no list, interleaved over the library so that position
order is not row order."""
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
from tests import ivf8_util as U8, ivf_util, search8_util as U, search_util  # noqa: E402
from tests.gpu_util import log  # noqa: E402
from tests.search_util import canon as _canon, ints as _ints, strings as _strings  # noqa: E402

DEV = "cuda:0"
NEG_INF = float("-inf")
SIZES = [0, 1, 15, 16, 17, 63, 64, 65, 129, 200, 0, 449]
L, LEFT_OUT = len(SIZES), 2
N = sum(SIZES) + LEFT_OUT
# how many queries name each list (clipped to Q): 0, 1, 16, 17 and 33 -- none, one pair, a full pair group, one more, two groups and one
NAMED = {0: 16, 1: 1, 2: 33, 3: 17, 4: 16, 5: 0, 6: 17, 7: 1, 8: 16, 9: 17, 10: 1, 11: 33}
SEG_ROWS = (64, 128, 192, 256, 448, None)                # a segment of the 449-row list runs 1, 2, 3, 4 and 7 iterations
SMALL = dict(n_layer_e3gnn=2, n_layer_xformer=2, n_hidden_xformer=64, n_hidden_e3nn=64, n_embd_common=64, n_head=4, n_seq=24, n_tok=48)


def _hand_assign(seed=0):
    a = torch.cat([torch.full((n,), l, dtype=torch.int32) for l, n in enumerate(SIZES)] + [torch.full((LEFT_OUT,), -1, dtype=torch.int32)])
    return a[torch.randperm(N, generator=torch.Generator().manual_seed(seed))]


def _index(x, metric="l2"):
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(x.shape[1], metric=metric, device=DEV)
    index.add(x)
    return index


_BUILT = {}


def _hand(dim):
    """(EmbeddingIndex, IVFIndex, Ivf8Index, assign) over N integer rows of width dim ("l2") with the lists given by hand; built once"""
    if dim not in _BUILT:
        from coati_amd.ivf import IVFIndex
        from coati_amd.ivf8 import Ivf8Index
        index = _index(_ints((N, dim), 300 + dim, -15, 15))
        centres = torch.randn(L, dim, generator=torch.Generator().manual_seed(dim))
        assign = _hand_assign()
        ivf = IVFIndex.build(index, L, centres=centres, assign=assign)
        ivf8 = Ivf8Index.build(index, L, centres=centres, assign=assign)
        assert ivf8.sizes.tolist() == SIZES and len(ivf8) == N and ivf8.nlist == L and ivf8.keep_rows
        _BUILT[dim] = (index, ivf, ivf8, assign)
    return _BUILT[dim]


def _named_table(Q):
    """[Q, n] int64: list l is named by min(NAMED[l], Q) queries -- queries shift_l, shift_l + 1, ... (mod Q) -- every query's lists in a
    seeded order, -1 behind them"""
    g = torch.Generator().manual_seed(Q)
    per_query = [[] for _ in range(Q)]
    for l, count in NAMED.items():
        for j in range(min(count, Q)):
            per_query[(3 * l + j) % Q].append(l)
    n = max(1, max(len(p) for p in per_query))
    t = torch.full((Q, n), -1, dtype=torch.int64)
    for i, lists in enumerate(per_query):
        lists = [lists[int(j)] for j in torch.randperm(len(lists), generator=g)]
        t[i, :len(lists)] = torch.tensor(lists, dtype=torch.int64)
    return t


def _oracle16(ivf, q, probes, k, bias=None):
    """ivf_util.scan on the bf16 IVF's stored operands, then the metric's finish in float64"""
    from coati_amd import search as S
    _, q16 = S.prepare_queries(q, ivf.metric, ivf.dim, DEV)
    b = ivf.bias if bias is None else ivf.bias + bias.to(DEV)[ivf.ids.long()]
    s, r = ivf_util.scan(ivf.vectors, ivf.ids, b, ivf.list_offsets, q16, probes, k, S.metric_alpha(ivf.metric))
    if ivf.metric == "l2":
        s = (s - (q16.double().cpu() ** 2).sum(dim=1, keepdim=True)).clamp_max(0.0)
    return s, r


def _equals(got, want, label):
    (s, r), (ws, wr) = got, want
    assert s.dtype == torch.float32 and r.dtype == torch.int64 and s.shape == r.shape == wr.shape, label
    bad_r, bad_s = int((r.cpu() != wr.cpu()).sum()), int((s.double().cpu() != ws.double().cpu()).sum())
    log(f"ivf8 {label}: {bad_r} rows and {bad_s} scores of {r.numel()} differ from the oracle")
    assert bad_r == 0 and bad_s == 0, label


# ---- 1. hand-made lists -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,Q,k", [(32, 1, 1), (96, 40, 10), (256, 40, 128), (512, 17, 10), (512, 1, 128)])
def test_hand_made_lists_equal_the_oracle_and_the_bf16_ivf(E, Q, k):
    index, ivf, ivf8, assign = _hand(E)
    assert ivf8.vectors8.shape == (N - LEFT_OUT, E) and torch.equal(ivf8.ids, ivf.ids) and torch.equal(ivf8.list_offsets, ivf.list_offsets)
    assert not torch.equal(ivf8.ids.long().cpu(), torch.arange(N - LEFT_OUT))            # position order is not row order
    assert torch.equal(ivf8.dequantised(), ivf.vectors.float())                          # e4m3 holds every row exactly
    left_out = set(torch.nonzero(assign < 0).reshape(-1).tolist())
    q = _ints((Q, E), 7 * Q + k + E, -15, 15)
    table = _named_table(Q)
    counts = torch.bincount(table[table >= 0], minlength=L).tolist()
    assert counts == [min(NAMED[l], Q) for l in range(L)]
    if Q == 40:
        assert sorted(set(counts)) == [0, 1, 16, 17, 33]
    ws, wr = _oracle16(ivf, q, table, k)
    s16, r16 = ivf.search(q, k, probes=table)
    _equals((s16, r16), (ws, wr), f"bf16 ivf E={E} Q={Q} k={k}")
    probed_rows = sum(SIZES[l] for l in set(table[0].tolist()) if l >= 0)
    for seg_rows in SEG_ROWS:
        s, r = ivf8.search(q, k, probes=table, seg_rows=seg_rows, rescore=False)
        _equals((s, r), (ws, wr), f"hand-made lists E={E} Q={Q} k={k} seg_rows={seg_rows}")
        assert torch.equal(s.view(torch.int32), s16.view(torch.int32)) and torch.equal(r, r16), seg_rows      # the bf16 IVF's bits
        assert not left_out & set(r.flatten().tolist())
        if k > probed_rows:                                                              # k above the probed rows: the tail is padding
            assert bool((r[0, probed_rows:] == -1).all() and (s[0, probed_rows:] == NEG_INF).all() and (r[0, :probed_rows] >= 0).all())
    # two short lists only (1 + 15 rows): with k above the probed rows the tail is padding
    few = torch.full((Q, 3), -1, dtype=torch.int64)
    few[:, 0], few[:, 2] = 2, 1
    s, r = ivf8.search(q, k, probes=few, rescore=False)
    _equals((s, r), _oracle16(ivf, q, few, k), f"hand-made lists E={E} Q={Q} k={k} two short lists")
    if k > 16:
        assert bool((r[:, 16:] == -1).all() and (s[:, 16:] == NEG_INF).all() and (r[:, :16] >= 0).all())


# ---- 2. mixed scales -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,k,E", [(33, 64, 256), (17, 128, 96)])
def test_mixed_scales_equal_the_exact_oracle(Q, k, E):
    """magnitudes up to 15 use all of e4m3's significand; every third row is small and every seventh times 0.125, so the rows' scales
    differ inside every slab; every list probed: the result is index.search's oracle"""
    n, nlist = 3000, 16
    x = _ints((n, E), 50 + n, -15, 15)
    x[::3] = _ints((x[::3].shape[0], E), 51 + n, -3, 3)
    x[1::7] *= 0.125
    q = _ints((Q, E), 52 + Q, -15, 15)
    q[::2] = _ints((q[::2].shape[0], E), 53, -2, 2)
    index = _index(x)
    assign = torch.randint(0, nlist, (n,), generator=torch.Generator().manual_seed(E), dtype=torch.int32)
    from coati_amd.ivf8 import Ivf8Index
    ivf8 = Ivf8Index.build(index, nlist, centres=torch.randn(nlist, E, generator=torch.Generator().manual_seed(1)), assign=assign, keep_rows=False)
    assert int(ivf8.scales.unique().numel()) >= 3 and not ivf8.keep_rows
    ws, wr, _ = search_util.index_search(index, q, k)
    every = torch.arange(nlist).repeat(Q, 1)
    _equals(ivf8.search(q, k, probes=every), (ws, wr), f"mixed scales Q={Q} k={k} E={E}")


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["constant", "blocks"])
@pytest.mark.parametrize("k", [7, 128])
def test_ties_across_lists(kind, k):
    """4096 rows dealt round-robin into 7 lists, every list probed: equal scores sit in different lists and different segments, and the
    order must still be original row ascending"""
    from coati_amd.ivf8 import Ivf8Index
    x, q = U.hex_library(kind)
    index = _index(x, "l2")
    assign = (torch.arange(4096) % 7).to(torch.int32)
    ivf8 = Ivf8Index.build(index, 7, centres=torch.randn(7, 32, generator=torch.Generator().manual_seed(2)), assign=assign)
    ws, wr, _ = search_util.index_search(index, q, k)
    every = torch.arange(7)[None, :]
    for seg_rows in (64, None):
        s, r = ivf8.search(q, k, probes=every, rescore=False, seg_rows=seg_rows)
        if kind == "constant":
            assert r[0].tolist() == list(range(k)), seg_rows
        else:
            assert r[0].tolist() == [i for i in range(4096) if (i // 100) % 2][:k], seg_rows
        _equals((s, r), (ws, wr), f"ties {kind} k={k} seg_rows={seg_rows}")


# ---- 4. geometry -----------------------------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_the_geometry():
    """blocks, seg_rows, what the scratch held before and the run: identical bits, in both stages"""
    index, ivf, ivf8, _ = _hand(96)
    Q, k = 40, 10
    q = _ints((Q, 96), 77, -15, 15)
    table = _named_table(Q)
    for rescore in (False, True):
        first = None
        for blocks in (0, 1, 3, 2048):
            for seg_rows in (64, 320, None):
                for _ in range(2):
                    if ivf8._scratch is not None:                                        # NaN bits where the last search left its lists
                        ivf8._scratch[0].fill_(float("nan"))
                        ivf8._scratch[1].fill_(-1)
                    s, r = ivf8.search(q, k, probes=table, seg_rows=seg_rows, blocks=blocks, rescore=rescore)
                    first = (s, r) if first is None else first
                    assert torch.equal(s.view(torch.int32), first[0].view(torch.int32)) and torch.equal(r, first[1]), (rescore, blocks, seg_rows)
        ws, wr = _oracle16(ivf, q, table, k)
        _equals(first, (ws, wr), f"geometry rescore={rescore}")


def test_query_chunks_give_the_same_result(monkeypatch):
    """the partial lists of a call stay within a scratch budget: with the budget cut to 7 queries' worth, 40 queries go in six calls"""
    from coati_amd import ivf as ivf_mod
    index, ivf, ivf8, _ = _hand(96)
    Q, k = 40, 10
    q = _ints((Q, 96), 78, -15, 15)
    for rescore, kk in ((False, k), (True, 4 * k)):
        s, r, probes = ivf8.search(q, k, nprobe=3, seg_rows=128, rescore=rescore, return_probes=True)
        assert torch.equal(probes, ivf.search(q, k, nprobe=3, return_probes=True)[2])    # the coarse step is the bf16 IVF's
        ws, wr = _oracle16(ivf, q, probes, k)
        _equals((s, r), (ws, wr), f"chunks rescore={rescore}")
        segs = -(-max(SIZES) // 128)
        monkeypatch.setattr(ivf_mod, "SCRATCH_BYTES", 7 * 3 * segs * kk * 8)
        ivf8._scratch = None
        s2, r2 = ivf8.search(q, k, nprobe=3, seg_rows=128, rescore=rescore)
        assert ivf8._scratch[0].numel() == 7 * 3 * segs * kk
        assert torch.equal(s2, s) and torch.equal(r2, r)
        monkeypatch.undo()


# ---- 5. real-valued data, stage 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [256, 512])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_gaussian_data_within_the_accumulation_bound(metric, E):
    """The oracle is scan8: the float64 score of the DEQUANTISED operands over the probed lists.  A product of two e4m3 values is exact
    in f32 and so is the power-of-two factor, so the error is the accumulation's alone (tests/test_gpu_search8.py, section 6): with
    u = 2^-23 the f32 sum of E exact products differs from the exact one by at most b = alpha E u |q_hat| |x_hat| in any order.
    Largest error observed on the MI355X: see DESIGN.md section 6, "Quantised approximate search"."""
    from coati_amd import search as S
    from coati_amd.ivf8 import Ivf8Index
    n, Q, k = 20000, 33, 10
    g = torch.Generator().manual_seed(11 + E)
    x = torch.randn(n, E, generator=g)
    index = _index(x, metric)
    q = torch.randn(Q, E, generator=g)
    ivf8 = Ivf8Index.build(index, 64, centres=x[:64], keep_rows=False)
    s, r, probes = ivf8.search(q, k, nprobe=8, return_probes=True)
    s, r = s.cpu(), r.cpu()
    ws, wr, full = U8.scan8(ivf8, q, probes, k + 1)                                       # full [Q, M] by position, -inf outside the probed lists
    q_hat = U8.dequantised_queries(ivf8, q)
    b = S.metric_alpha(metric) * E * 2.0 ** -23 * q_hat.double().norm(dim=1, keepdim=True) * ivf8.dequantised().cpu().double().norm(dim=1)[None, :]
    assert bool((r >= 0).all())
    pos = ivf8._inverse.cpu()[r]                                                          # the returned rows' positions
    assert bool((pos >= 0).all())
    of_returned, b_returned = full.gather(1, pos), b.gather(1, pos)
    assert bool((of_returned > NEG_INF).all())                                            # every returned row is in a probed list
    err = (s.double() - of_returned).abs()
    log(f"ivf8 gaussian {metric} E={E}: largest stage-1 score error {float(err.max()):.3e}, bound b between {float(b.min()):.3e} and "
        f"{float(b.max()):.3e}; {int((r != wr[:, :k]).sum())} of {r.numel()} rows differ from the oracle's order")
    assert bool((err <= b_returned).all())                                                # every score within b of the oracle's for that row
    assert bool((of_returned >= ws[:, k - 1:k] - 2 * b_returned).all())                   # every returned row belongs (to 2 b)
    clear = full > ws[:, k:k + 1] + 2 * b                                                 # probed rows that beat the (k + 1)-th by more than 2 b ...
    returned = torch.zeros_like(clear)
    returned.scatter_(1, pos, True)
    assert bool((returned | ~clear).all())                                                # ... are all returned
    assert bool((s[:, 1:] <= s[:, :-1]).all())


# ---- 6. two stages equal the bf16 IVF -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [256, 512])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
@pytest.mark.parametrize("data", ["gaussian", "clustered"])
def test_two_stages_equal_the_bf16_ivf(data, metric, E):
    """R = 8 * 10 = 80 candidates.  Asserted first, from the float64 emulation of stage 1 restricted to each query's probed rows: every
    row of IVFIndex.search's top 10 has stage-1 rank below R / 2 = 40, so f32 rounding in stage 1 cannot push one out of the 80 (on a
    CPU, with nearest-centre lists computed in float64, the largest rank over the eight cells was 21).  Then the two-stage result must
    be the bf16 IVF's, rows and score BITS; with every list probed, the exact search's."""
    from coati_amd.ivf import IVFIndex
    from coati_amd.ivf8 import Ivf8Index
    n, Q, k, over = 20000, 33, 10, 8
    if data == "gaussian":
        g = torch.Generator().manual_seed(23 + E)
        x, q = torch.randn(n, E, generator=g), torch.randn(Q, E, generator=g)
    else:
        draw = U.clustered(n, E, 29 + E)
        x, q = draw(n), draw(Q)
    index = _index(x, metric)
    ivf = IVFIndex.build(index, 64, centres=x[:64])
    ivf8 = Ivf8Index.from_ivf(ivf, index)
    assert ivf8.keep_rows and ivf8._rows16.data_ptr() == index.vectors.data_ptr()
    ws, wr, probes = ivf.search(q, k, nprobe=8, return_probes=True)
    assert bool((wr >= 0).all())
    _, _, full = U8.scan8(ivf8, q, probes, k)                                             # [Q, M] by position, -inf outside the probed lists
    pos = ivf8._inverse.cpu()[wr.cpu()]                                                   # [Q, k]: the positions of the bf16 IVF's top k
    mine = full.gather(1, pos)
    ids = ivf8.ids.long().cpu()
    above = (full[:, None, :] > mine[:, :, None]).sum(dim=2)
    ties_before = ((full[:, None, :] == mine[:, :, None]) & (ids[None, None, :] < wr.cpu()[:, :, None])).sum(dim=2)
    rank = above + ties_before
    log(f"ivf8 two stages {data} {metric} E={E}: the bf16 IVF's top {k} have emulated stage-1 ranks up to {int(rank.max())} (R = {over * k})")
    assert bool((mine > NEG_INF).all()) and int(rank.max()) < over * k // 2
    s, r, probes8 = ivf8.search(q, k, nprobe=8, oversample=over, return_probes=True)
    assert torch.equal(probes8, probes)
    assert torch.equal(r, wr) and torch.equal(s.view(torch.int32), ws.view(torch.int32))
    es, er = index.search(q, k)
    s, r = ivf8.search(q, k, nprobe=64, oversample=over)
    assert torch.equal(r, er) and torch.equal(s.view(torch.int32), es.view(torch.int32))


# ---- 7. bias and removal -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescore", [False, True])
def test_bias_and_removal(rescore):
    """every list probed, so the oracle is the exact search's; the integer rows are e4m3 values and the integer extra bias is added
    exactly, in stage 1 by position and in stage 2 by original row"""
    from coati_amd.ivf8 import Ivf8Index
    n, Q, k, E, nlist = 900, 17, 7, 64, 5
    x, q = _ints((n, E), 5, -15, 15), _ints((Q, E), 6, -15, 15)
    index = _index(x)
    assign = torch.randint(0, nlist, (n,), generator=torch.Generator().manual_seed(9), dtype=torch.int32)
    ivf8 = Ivf8Index.build(index, nlist, centres=torch.randn(nlist, E, generator=torch.Generator().manual_seed(3)), assign=assign)
    every = torch.arange(nlist).repeat(Q, 1)

    def search(**kw):
        return ivf8.search(q, k, probes=every, rescore=rescore, **kw)

    def oracle():
        return search_util.index_search(index, q, k)[:2]

    s0, r0 = search()
    _equals((s0, r0), oracle(), f"all lists rescore={rescore}")
    # bias= is added in both stages
    extra = _ints((n,), 8, -30, 30).to(DEV)
    extra[int(r0[1, 0])] = NEG_INF                             # ... and -inf excludes a row
    index.bias.add_(extra)
    sb, rb = search(bias=extra)
    _equals((sb, rb), oracle(), f"bias= rescore={rescore}")
    assert int(r0[1, 0]) not in rb.flatten().tolist()
    index.bias.copy_(ivf8._bias16)
    # removing the best rows of query 0 through the fp8 IVF brings the next ones up
    ivf8.remove(r0[0, :3])
    index.remove(r0[0, :3])
    assert len(ivf8) == n
    s1, r1 = search()
    _equals((s1, r1), oracle(), f"3 rows removed rescore={rescore}")
    assert not set(r0[0, :3].tolist()) & set(r1.flatten().tolist())
    assert r1[0, :k - 3].tolist() == r0[0, 3:].tolist()
    # all but k - 3 rows removed: three pads
    keep = r1[0, :k - 3].tolist()
    gone = [i for i in range(n) if i not in keep]
    ivf8.remove(gone)
    index.remove(gone)
    s3, r3 = search()
    _equals((s3, r3), oracle(), f"k - 3 rows left rescore={rescore}")
    assert bool((r3[:, k - 3:] == -1).all() and (s3[:, k - 3:] == NEG_INF).all() and (r3[:, :k - 3] >= 0).all())
    assert r3[0, :k - 3].tolist() == keep


# ---- 8. build -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_build_makes_the_bf16_ivf_lists(metric, tmp_path):
    from coati_amd import fp8_index as F
    from coati_amd.ivf import IVFIndex
    from coati_amd.ivf8 import Ivf8Index
    g = torch.Generator().manual_seed(31)
    x = torch.randn(5000, 96, generator=g) + 3 * torch.randn(32, 96, generator=g)[torch.randint(0, 32, (5000,), generator=g)]
    index = _index(x, metric)
    index.remove([5, 77])
    ivf8, ivf = index.ivf(32, fp8=True), index.ivf(32)
    assert isinstance(ivf8, Ivf8Index) and isinstance(ivf, IVFIndex) and ivf8.keep_rows
    assert torch.equal(ivf8.ids, ivf.ids) and torch.equal(ivf8.sizes, ivf.sizes) and torch.equal(ivf8.centres, ivf.centres)
    assert int(ivf8.sizes.sum()) == 4998
    b, s = F.quantise_rows(ivf.vectors)
    assert torch.equal(ivf8.vectors8, b) and torch.equal(ivf8.scales, s)                  # byte for byte
    if metric == "l2":
        assert torch.equal(ivf8.bias, -(F.dequantise(b, s).double() ** 2).sum(dim=1).float())
    else:
        assert torch.equal(ivf8.bias, ivf.bias)
    assert ivf8._rows16.data_ptr() == index.vectors.data_ptr()
    again = ivf.fp8(index)
    assert torch.equal(again.vectors8, b) and torch.equal(again.bias, ivf8.bias) and again._rows16.data_ptr() == index.vectors.data_ptr()
    q = x[:19] + 0.1 * torch.randn(19, 96, generator=g)
    for keep_rows in (True, False):
        src = ivf8 if keep_rows else index.ivf(32, fp8=True, keep_rows=False)
        assert src.keep_rows == keep_rows
        path = str(tmp_path / f"ivf8_{keep_rows}.pt")
        src.save(path)
        back = Ivf8Index.load(path, device=DEV)
        assert back.keep_rows == keep_rows and torch.equal(back.vectors8, src.vectors8) and torch.equal(back.scales, src.scales)
        s0, r0 = src.search(q, 10, nprobe=4)
        s1, r1 = back.search(q, 10, nprobe=4)
        assert torch.equal(s0.view(torch.int32), s1.view(torch.int32)) and torch.equal(r0, r1) and bool((r0 >= 0).all())
    # the rows kept: the result is the bf16 IVF's wherever its rows are among the candidates -- here recall is just logged
    _, want = ivf.search(q, 10, nprobe=4)
    log(f"ivf8 build {metric}: recall@10 of the two stages against the bf16 IVF {ivf_util.recall(ivf8.search(q, 10, nprobe=4)[1], want):.3f}")


# ---- 9. from strings ----------------------------------------------------------------------------------------------------------------------
def test_from_strings(golden_dir):
    from coati.generative import build_index, nearest_smiles
    from coati_amd.ivf8 import Ivf8Index
    from coati_amd.models.encoding.clip_e2e import e3gnn_smiles_clip_e2e
    from coati_amd.models.encoding.tokenizers import TrieTokenizer
    g = np.load(os.path.join(golden_dir, "generative_golden.npz"))
    voc = json.load(open(os.path.join(golden_dir, "tokenizer.json")))
    tk = TrieTokenizer(n_seq=int(g["n_seq"]), smiles_tokens=voc["smiles"], special_tokens=voc["special"])
    with contextlib.redirect_stdout(io.StringIO()):
        model = e3gnn_smiles_clip_e2e(**SMALL, device=torch.device(DEV))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "small_model_after3.npz")).items()}, strict=False)
    strings = _strings([t for t in voc["smiles"] if t.isascii() and "X" not in t], 40, 5)
    given = strings[:10] + ["CXC", None, "C~C"] + strings[10:]
    with contextlib.redirect_stdout(io.StringIO()):
        index, kept = build_index(given, model, tk, batch_size=16, canon_smiles=_canon, nlist=4, list_dtype="fp8")
        near = nearest_smiles(kept + ["CXC"], index, kept, model, tk, k=3, canon_smiles=_canon)      # the default nprobe covers the four lists
    assert isinstance(index, Ivf8Index) and index.keep_rows and kept == strings and len(index) == 40 and index.nlist == 4
    assert near[-1] == [] and len(near) == len(kept) + 1
    for s, hits in zip(kept, near):
        assert len(hits) == 3 and hits[0][0] == s, (s, hits)                   # every query string finds itself first
        assert [v for _, v in hits] == sorted((v for _, v in hits), reverse=True)
        assert abs(hits[0][1] - 1.0) <= 1e-2                                   # the exact score of the bf16 rows
