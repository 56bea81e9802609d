"""IVF approximate search on the GPU (include/coati_ivf.h, coati_amd/ivf.py) against the float64 restatement of tests/ivf_util.py and
against the exact kernel (EmbeddingIndex.search).  Integer data in -4 .. 4 is exact in bf16 and in f32 in any summation order (an "l2"
index adds the integers -|x|^2 and -|q|^2), so those cases must EQUAL the oracle element for element, ties and padding included.

The lists are given by hand (centres= with assign=): N = 3000 rows in L = 7 lists -- list 0 empty, list 1 one row, list 2 15 rows, list
3 150 rows (three segments at seg_rows = 64), list 4 203 rows (not a multiple of 16), lists 5 and 6 1200 and 1431 rows -- interleaved over
the library, so that position order is not row order."""
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
from tests import ivf_util, search_util  # noqa: E402
from tests.gpu_util import log  # noqa: E402
from tests.search_util import canon as _canon, ints as _ints, strings as _strings  # noqa: E402

DEV = "cuda:0"
NEG_INF = float("-inf")
N, L = 3000, 7
SIZES = [0, 1, 15, 150, 203, 1200, 1431]
ONE_SEGMENT = 1472                                   # the longest list in one segment: the next multiple of 64
SMALL = dict(n_layer_e3gnn=2, n_layer_xformer=2, n_hidden_xformer=64, n_hidden_e3nn=64, n_embd_common=64, n_head=4, n_seq=24, n_tok=48)


def _hand_assign(seed=0):
    a = torch.cat([torch.full((n,), l, dtype=torch.int32) for l, n in enumerate(SIZES)])
    return a[torch.randperm(N, generator=torch.Generator().manual_seed(seed))]


_BUILT = {}


def _hand_index(dim, metric="l2", gaussian=False):
    """(EmbeddingIndex, IVFIndex) over N rows of width dim with the lists given by hand; built once per (dim, metric, kind)"""
    key = (dim, metric, gaussian)
    if key not in _BUILT:
        from coati_amd.search import EmbeddingIndex
        from coati_amd.ivf import IVFIndex
        g = torch.Generator().manual_seed(100 + dim)
        x = torch.randn(N, dim, generator=g) if gaussian else _ints((N, dim), 100 + dim)
        index = EmbeddingIndex(dim, metric=metric, device=DEV)
        index.add(x)
        centres = torch.randn(L, dim, generator=g)
        ivf = IVFIndex.build(index, L, centres=centres, assign=_hand_assign())
        assert ivf.sizes.tolist() == SIZES and len(ivf) == N and ivf.nlist == L
        _BUILT[key] = (index, ivf)
    return _BUILT[key]


def _oracle(ivf, q, probes, k, bias=None):
    """ivf_util.scan on the stored operands, then the metric's finish in float64"""
    from coati_amd import search as S
    _, q16 = S.prepare_queries(q, ivf.metric, ivf.dim, DEV)
    b = ivf.bias if bias is None else ivf.bias + bias.to(DEV)[ivf.ids.long()]
    s, r = ivf_util.scan(ivf.vectors, ivf.ids, b, ivf.list_offsets, q16, probes, k, S.metric_alpha(ivf.metric))
    if ivf.metric == "l2":
        s = (s - (q16.double().cpu() ** 2).sum(dim=1, keepdim=True)).clamp_max(0.0)
    return s, r


def _exact(ivf, q, probes, k, label, **kw):
    s, r = ivf.search(q, k, probes=probes, **kw)
    ws, wr = _oracle(ivf, q, probes, k, kw.get("bias"))
    assert s.dtype == torch.float32 and r.dtype == torch.int64 and s.shape == r.shape == (q.shape[0], k)
    bad_r, bad_s = int((r.cpu() != wr).sum()), int((s.double().cpu() != ws).sum())
    log(f"ivf {label}: {bad_r} rows and {bad_s} scores of {r.numel()} differ from the oracle")
    assert bad_r == 0 and bad_s == 0, label
    return s, r


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


# ---- 1. explicit probe tables against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,Q,k", [(32, 1, 1), (32, 40, 10), (90, 17, 10), (256, 40, 128), (256, 17, 1), (512, 40, 10), (512, 1, 128)])
def test_probe_tables_equal_the_oracle(dim, Q, k):
    index, ivf = _hand_index(dim)
    assert ivf.vectors.shape == (N, (dim + 31) // 32 * 32) and ivf.ids.dtype == torch.int32
    for l in range(L):
        rows = ivf.list_rows(l)
        assert rows.numel() == SIZES[l] and bool((rows[1:] > rows[:-1]).all())          # ascending inside every list
    assert not torch.equal(ivf.ids.long().cpu(), torch.arange(N))                        # position order is not row order
    q = _ints((Q, dim), 7 * Q + k + dim)
    for t in _tables(Q, Q + k):
        s, r = _exact(ivf, q, t, k, f"dim={dim} Q={Q} k={k} nprobe={t.shape[1]}")
        assert bool((r.cpu()[t.max(dim=1).values < 0] == -1).all())                           # nothing probed: padding only
    # ties between rows of different lists: with 9 values per entry equal scores abound at dim 32; the oracle breaks them by original row
    if dim == 32 and k > 1:
        full = torch.arange(L).repeat(Q, 1)
        s, r = _exact(ivf, q, full, k, f"dim={dim} Q={Q} k={k} all lists")
        tied = (s[:, 1:] == s[:, :-1]).cpu()
        lists = _hand_assign()[r.cpu()]
        assert bool((tied & (lists[:, 1:] != lists[:, :-1])).any())
    # k larger than the rows probed: the one-row list and the 15-row list
    few = torch.tensor([[1, -1, 2]]).repeat(Q, 1)
    s, r = _exact(ivf, q, few, max(k, 20), "padding")
    assert bool((r[:, 16:] == -1).all() and (s[:, 16:] == NEG_INF).all() and (r[:, :16] >= 0).all())


def test_work_item_table_of_the_hand_made_lists():
    """the shapes of the work-item table the cases above run on: 40 queries on every list are three groups of <= 16 pairs"""
    from coati_amd.ivf import invert_probes
    _, ivf = _hand_index(32)
    table = torch.arange(L, dtype=torch.int32, device=DEV).repeat(40, 1)
    _, pair_off, item_off, _ = invert_probes(table, ivf.sizes, 64)
    assert (pair_off[1:] - pair_off[:-1]).tolist() == [40] * L
    assert (item_off[1:] - item_off[:-1]).tolist() == [0, 3, 3, 9, 12, 57, 69]


# ---- 2. nprobe = L is the exact search -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,metric,gaussian", [(32, "l2", False), (256, "cosine", True), (256, "l2", True), (512, "cosine", True), (512, "l2", True)])
def test_all_lists_equal_the_exact_search_bitwise(dim, metric, gaussian):
    """every live row is in one probed list, and a row's MFMA sequence is the same in both kernels: rows equal, scores equal BITWISE"""
    index, ivf = _hand_index(dim, metric, gaussian)
    g = torch.Generator().manual_seed(5 + dim)
    q = torch.randn(40, dim, generator=g) if gaussian else _ints((40, dim), 5 + dim)
    for k in (1, 10, 128):
        s, r, probes = ivf.search(q, k, nprobe=L, return_probes=True)
        assert probes.shape == (40, L) and bool((probes[:, :L - 1] >= 0).all() and (probes[:, L - 1] == -1).all())   # the empty list is never probed
        ws, wr = index.search(q, k)
        diff = float((s - ws).abs().nan_to_num(0.0).max())
        log(f"ivf all lists dim={dim} {metric} k={k}: {int((r != wr).sum())} rows differ from the exact search, largest score difference {diff:.3e}")
        assert torch.equal(r, wr) and torch.equal(s, ws)


# ---- 3. launch geometry and scratch contents ---------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_segments_blocks_or_scratch():
    _, ivf = _hand_index(96)
    Q, k = 40, 10
    q = _ints((Q, 96), 77)
    full = torch.arange(L).repeat(Q, 1)
    ws, wr = _oracle(ivf, q, full, k)
    for seg_rows in (64, 128, ONE_SEGMENT, None):
        for blocks in (1, 3, 0):
            s, r = ivf.search(q, k, probes=full, seg_rows=seg_rows, blocks=blocks)
            assert torch.equal(r.cpu(), wr) and torch.equal(s.double().cpu(), ws), (seg_rows, blocks)
            # whatever the scratch held: +inf scores of a fixed row in every slot, the ones no work item writes included
            ivf._scratch[0].fill_(float("inf"))
            ivf._scratch[1].fill_(5)
            s2, r2 = ivf.search(q, k, probes=full, seg_rows=seg_rows, blocks=blocks)
            assert torch.equal(s2, s) and torch.equal(r2, r), (seg_rows, blocks)
    with pytest.raises(ValueError, match="seg_rows"):
        ivf.search(q, k, probes=full, seg_rows=96)
    with pytest.raises(ValueError, match="16384"):
        ivf.search(q, 128, probes=full, seg_rows=64)                                     # 7 lists x 23 segments x 128


def test_query_chunks_give_the_same_result(monkeypatch):
    """the partial lists of a call stay within a scratch budget: with the budget cut to 7 queries' worth, 40 queries go in six calls"""
    from coati_amd import ivf as ivf_mod
    _, ivf = _hand_index(96)
    Q, k = 40, 10
    q = _ints((Q, 96), 78)
    s, r, probes = ivf.search(q, k, nprobe=3, seg_rows=128, return_probes=True)
    ws, wr = _oracle(ivf, q, probes, k)
    assert torch.equal(r.cpu(), wr) and torch.equal(s.double().cpu(), ws)
    segs = -(-max(SIZES) // 128)
    monkeypatch.setattr(ivf_mod, "SCRATCH_BYTES", 7 * 3 * segs * k * 8)
    ivf._scratch = None
    s2, r2 = ivf.search(q, k, nprobe=3, seg_rows=128)
    assert ivf._scratch[0].numel() == 7 * 3 * segs * k
    assert torch.equal(s2, s) and torch.equal(r2, r)


# ---- 4. real-valued data -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [256, 512])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_gaussian_data_within_the_accumulation_bound(metric, dim):
    """test_gpu_search.py's bound: the f32 sum of E exact bf16 products differs from the exact one by at most alpha E 2^-23 |q| |x|.  And
    the result is the exact kernel's with the unprobed rows biased to -inf (per query: the bias is per row)."""
    from coati_amd import search as S
    index, ivf = _hand_index(dim, metric, True)
    Q, k = 6, 10
    q = torch.randn(Q, dim, generator=torch.Generator().manual_seed(9 + dim))
    s, r, probes = ivf.search(q, k, nprobe=3, return_probes=True)
    assert bool((r >= 0).all() and (probes >= 0).all())
    assert torch.equal(probes, ivf.probe(q, 3))
    full = search_util.index_scores(index, q)                                            # [Q, N] float64, the metric's
    _, q16 = S.prepare_queries(q, metric, dim, DEV)
    b = S.metric_alpha(metric) * dim * 2.0 ** -23 * q16.double().norm(dim=1, keepdim=True) * index.vectors.double().norm(dim=1)[None, :]
    err = (s.double() - full.gather(1, r)).abs()
    log(f"ivf gaussian {metric} dim={dim}: largest score error {float(err.max()):.3e}, bound between {float(b.min()):.3e} and {float(b.max()):.3e}")
    assert bool((err <= b.gather(1, r)).all())
    assign = _hand_assign().to(DEV)
    for i in range(Q):
        inside = (assign[:, None] == probes[i][None, :].to(torch.int32)).any(dim=1)
        assert bool(inside[r[i]].all())                                                  # every returned row is in a probed list
        mask = torch.where(inside, 0.0, NEG_INF).to(torch.float32)
        ws, wr = index.search(q[i], k, bias=mask)
        assert torch.equal(r[i:i + 1], wr) and torch.equal(s[i:i + 1], ws), i
    assert bool((s[:, 1:] <= s[:, :-1]).all())


# ---- 5. recall ------------------------------------------------------------------------------------------------------------------------
def test_recall_is_monotone_in_nprobe_and_complete_at_all_lists():
    """the probed sets are nested (the coarse ranking's prefixes) and Gaussian scores are distinct, so the exact top k found can only grow"""
    index, ivf = _hand_index(256, "cosine", True)
    q = torch.randn(17, 256, generator=torch.Generator().manual_seed(13))
    _, exact = index.search(q, 10)
    seen = []
    for nprobe in (1, 2, 4, L):
        _, r = ivf.search(q, 10, nprobe=nprobe)
        seen.append(ivf_util.recall(r, exact))
    log(f"ivf recall@10 at nprobe 1, 2, 4, {L} on hand-made lists: {seen}")
    assert seen == sorted(seen) and seen[-1] == 1.0


# ---- 6. the index's other methods -------------------------------------------------------------------------------------------------------
def test_remove_and_bias():
    from coati_amd.ivf import IVFIndex
    index, _ = _hand_index(96)
    ivf = IVFIndex.build(index, L, centres=torch.randn(L, 96, generator=torch.Generator().manual_seed(1)), assign=_hand_assign())
    Q, k = 17, 10
    q = _ints((Q, 96), 21)
    full = torch.arange(L).repeat(Q, 1)
    s0, r0 = _exact(ivf, q, full, k, "before remove")
    ivf.remove(r0[0, :3])
    assert len(ivf) == N
    s1, r1 = _exact(ivf, q, full, k, "3 rows removed")
    assert not set(r0[0, :3].tolist()) & set(r1.flatten().tolist())
    assert r1[0, :k - 3].tolist() == r0[0, 3:].tolist()
    # bias over ORIGINAL rows: integers are added exactly, -inf excludes
    bias = _ints((N,), 22, -50, 50).to(DEV)
    bias[r1[1, :2]] = NEG_INF
    s2, r2 = _exact(ivf, q, full, k, "bias", bias=bias)
    assert not set(r1[1, :2].tolist()) & set(r2.flatten().tolist()) and not torch.equal(r2, r1)
    with pytest.raises(ValueError, match="bias"):
        ivf.search(q, k, bias=bias[:10])
    with pytest.raises(IndexError):
        ivf.remove([N])
    # an index built from a source with removed rows leaves them out
    from coati_amd.search import EmbeddingIndex
    index2 = EmbeddingIndex(32, metric="l2", device=DEV)
    index2.add(_ints((N, 32), 24))
    gone = [0, 5, 2999]
    index2.remove(gone)
    ivf2 = IVFIndex.build(index2, L, centres=torch.randn(L, 32, generator=torch.Generator().manual_seed(2)), assign=_hand_assign())
    assert int(ivf2.sizes.sum()) == N - 3 and len(ivf2) == N
    _, r = ivf2.search(_ints((5, 32), 23), 128, nprobe=L)
    assert not set(gone) & set(r.flatten().tolist())
    ws, wr = index2.search(_ints((5, 32), 23), 128)
    assert torch.equal(r, wr)


def test_save_load_and_streams(tmp_path):
    from coati_amd.ivf import IVFIndex
    _, ivf = _hand_index(90)
    q = _ints((19, 90), 31)
    s, r = ivf.search(q, 7, nprobe=3)
    ivf.save(str(tmp_path / "ivf.pt"))
    again = IVFIndex.load(str(tmp_path / "ivf.pt"), device=DEV)
    assert len(again) == N and again.metric == "l2" and again.dim == 90 and again.dim_padded == 96
    for a, b in ((again.vectors, ivf.vectors), (again.ids, ivf.ids), (again.bias, ivf.bias), (again.sizes, ivf.sizes),
                 (again.centres, ivf.centres), (again.list_offsets, ivf.list_offsets)):
        assert torch.equal(a, b)
    s1, r1 = again.search(q, 7, nprobe=3)
    assert torch.equal(s1, s) and torch.equal(r1, r)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s2, r2 = ivf.search(q.to(DEV), 7, nprobe=3)
    side.synchronize()
    assert torch.equal(s2, s) and torch.equal(r2, r)
    s3, r3 = ivf.search(q[0], 7, nprobe=3)                                               # one vector is one query
    assert torch.equal(s3, s[:1]) and torch.equal(r3, r[:1])


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_build_is_reproducible_and_probes_the_nearest_lists(metric):
    from coati_amd.search import EmbeddingIndex
    g = torch.Generator().manual_seed(41)
    means = 4.0 * torch.randn(12, 64, generator=g)
    x = means[torch.randint(0, 12, (N,), generator=g)] + torch.randn(N, 64, generator=g)
    index = EmbeddingIndex(64, metric=metric, device=DEV)
    index.add(x)
    a, b = index.ivf(12, iters=5, seed=3), index.ivf(12, iters=5, seed=3)
    for u, v in ((a.vectors, b.vectors), (a.ids, b.ids), (a.bias, b.bias), (a.sizes, b.sizes), (a.centres, b.centres)):
        assert torch.equal(u, v)
    assert int(a.sizes.sum()) == N and torch.equal(a.ids.long().sort().values, torch.arange(N, device=DEV))
    # the lists are the clustering's: every row sits in the list of its nearest centre (cosine: assign() normalises the centres once
    # more, which may move a bit of them, so only l2 is held to it)
    assign, _ = index.assign(a.centres)
    if metric == "l2":
        ids, off = ivf_util.inverted(assign.cpu(), 12)
        assert torch.equal(ids, a.ids.long().cpu()) and torch.equal(off, a.list_offsets.long().cpu())
    # probe(q, 1) of a stored row's own vector is the nearest centre's list -- its own list, the assignment kernel's choice
    rows = torch.arange(0, N, 97)
    assert torch.equal(a.probe(x[rows], 1)[:, 0].cpu(), assign.cpu()[rows].long())
    q = x[:40] + 0.1 * torch.randn(40, 64, generator=g)
    _, exact = index.search(q, 10)
    seen = [ivf_util.recall(a.search(q, 10, nprobe=n)[1], exact) for n in (1, 2, 4, 12)]
    log(f"ivf {metric} k-means lists, mixture of 12 Gaussians: recall@10 at nprobe 1, 2, 4, 12 = {seen}")
    assert seen == sorted(seen) and seen[-1] == 1.0


def test_nearest_smiles_through_an_ivf_index(golden_dir):
    from coati.generative import build_index, nearest_smiles
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
        near = nearest_smiles(kept, ivf, kept, model, tk, k=3, canon_smiles=_canon)
        want = nearest_smiles(kept, exact, kept, model, tk, k=3, canon_smiles=_canon)
    assert isinstance(ivf, IVFIndex) and kept == kept2 == strings and len(ivf) == 40 and ivf.nlist == 4
    assert near == want                                                                  # the default nprobe covers the four lists
    for s, hits in zip(kept, near):
        assert len(hits) == 3 and hits[0][0] == s and abs(hits[0][1] - 1.0) <= 1e-2, (s, hits)
