"""IVF-PQ search on the GPU (include/coati_ivfpq.h, coati_amd/ivfpq.py).  coati_ivfpq_scan is held to coati_ivf_scan BIT FOR BIT on the
widened library [centre | entry] against [q | q] at width 2 E; on integer data stage 1 equals the float64 oracle of tests/ivfpq_util.py
element for element, ties and padding included; on a library composed as centre + entry the two stages equal IVFIndex.search bit for bit;
on real-valued data stage 1 is held to the f32 accumulation bound and every two-stage score to the exact kernel's bits.

The hand-made lists: 7 lists of 0, 1, 63, 64, 65, 200 and 30 rows (an empty list, one row, every remainder of the 64-row iteration, a
list of several segments), interleaved over the library so that position order is not row order."""
import contextlib
import io
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import ivf_util, ivfpq_util as U, pq_util, search_util  # noqa: E402
from tests.gpu_util import log  # noqa: E402
from tests.search_util import canon as _canon, ints as _ints, strings as _strings  # noqa: E402

DEV = "cuda:0"
NEG_INF = float("-inf")
SIZES = [0, 1, 63, 64, 65, 200, 30]
L, N = len(SIZES), sum(SIZES)
SMALL = dict(n_layer_e3gnn=2, n_layer_xformer=2, n_hidden_xformer=64, n_hidden_e3nn=64, n_embd_common=64, n_head=4, n_seq=24, n_tok=48)


def _hand_assign(seed=0, sizes=SIZES):
    a = torch.cat([torch.full((n,), l, dtype=torch.int32) for l, n in enumerate(sizes)])
    return a[torch.randperm(a.shape[0], generator=torch.Generator().manual_seed(seed))]


def _index(x, metric="l2"):
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(x.shape[1], metric=metric, device=DEV)
    index.add(x)
    return index


def _equals(got, want, label):
    (s, r), (ws, wr) = got, want
    assert s.dtype == torch.float32 and r.dtype == torch.int64 and s.shape == r.shape == wr.shape, label
    bad_r, bad_s = int((r.cpu() != wr.cpu()).sum()), int((s.double().cpu() != ws.double().cpu()).sum())
    log(f"ivfpq {label}: {bad_r} rows and {bad_s} scores of {r.numel()} differ from the oracle")
    assert bad_r == 0 and bad_s == 0, label


def _bits(a, b):
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


# ---- 1. the bits of coati_ivf_scan on the widened library ---------------------------------------------------------------------------------
def _table(Q, nprobe, seed):
    """[Q, nprobe] int64: per query distinct lists in a seeded order; below nprobe = L list 6 is named by nobody (a list with no pairs);
    one query's later entries are -1"""
    g = torch.Generator().manual_seed(seed)
    pool = L if nprobe == L else L - 1
    t = torch.stack([torch.randperm(pool, generator=g)[:nprobe] for _ in range(Q)])
    if nprobe > 1:
        t[Q // 2, nprobe // 2:] = -1
    return t


@pytest.mark.parametrize("E", [32, 96, 256])
def test_scan_has_the_bits_of_the_bf16_scan_on_the_widened_library(E):
    """random codes under Gaussian bf16 code books, Gaussian bf16 centres, Gaussian bias.  Both scans write into scratch pre-filled with
    the same pattern, so equal arrays mean: the same slots written, and the same bits in every written slot."""
    from coati_amd import _lib, ivfpq, pq
    from coati_amd.ivf import invert_probes
    from coati_amd.ops import ptr, stream
    g = torch.Generator().manual_seed(100 + E)
    cb = torch.randn(E // 8, 256, 8, generator=g).to(torch.bfloat16).to(DEV)
    c16 = torch.randn(L, E, generator=g).to(torch.bfloat16).to(DEV)
    codes = torch.randint(0, 256, (N, E // 8), generator=g, dtype=torch.uint8).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    ids, off = ivf_util.inverted(_hand_assign(), L)
    ids32, list_off, sizes = ids.to(DEV, torch.int32), off.to(DEV, torch.int32), (off[1:] - off[:-1]).to(DEV)
    lists = U.position_lists(off).to(DEV)
    wide = torch.cat([c16[lists], pq.reconstruct(codes, cb)], dim=1).contiguous()            # [N, 2 E]: the row the codes stand for, unsummed
    km = ivfpq.k_max(E)
    assert km == (64 if E == 256 else 128)
    geometry = list(itertools.product((1.0, 2.0), (64, 128), (1, 3, 0)))                     # alpha, seg_rows, blocks
    n = written = 0
    with torch.cuda.device(DEV):
        s = stream()
        for Q, nprobe, k in itertools.product((1, 16, 17, 33), (1, 3, L), (1, 10, km)):
            alpha, seg_rows, blocks = geometry[n % len(geometry)]
            n += 1
            q = torch.randn(Q, E, generator=g).to(torch.bfloat16).to(DEV)
            q2 = torch.cat([q, q], dim=1).contiguous()
            table = _table(Q, nprobe, n).to(DEV, torch.int32).contiguous()
            pair_q, pair_off, item_off, pair_slot = invert_probes(table, sizes, seg_rows)
            P, segs = Q * nprobe, -(-max(SIZES) // seg_rows)
            part = [(torch.full((P * segs * k,), float("nan"), device=DEV), torch.full((P * segs * k,), -7, dtype=torch.int32, device=DEV))
                    for _ in range(2)]
            _lib.call("coati_ivfpq_scan", ptr(codes), ptr(ids32), ptr(bias), ptr(list_off), N, E, L, ptr(c16), ptr(cb), ptr(q), Q, ptr(pair_q),
                      ptr(pair_off), ptr(item_off), P, k, alpha, seg_rows, segs, ptr(part[0][0]), ptr(part[0][1]), blocks, s)
            _lib.call("coati_ivf_scan", ptr(wide), ptr(ids32), ptr(bias), ptr(list_off), N, 2 * E, L, ptr(q2), Q, ptr(pair_q), ptr(pair_off),
                      ptr(item_off), P, k, alpha, seg_rows, segs, ptr(part[1][0]), ptr(part[1][1]), 0, s)
            label = (E, Q, nprobe, k, alpha, seg_rows, blocks)
            assert torch.equal(part[0][0].view(torch.int32), part[1][0].view(torch.int32)), label
            assert torch.equal(part[0][1], part[1][1]), label
            written += int((part[0][1] >= 0).sum())
            out = [(torch.empty(Q, k, device=DEV), torch.empty(Q, k, dtype=torch.int64, device=DEV)) for _ in range(2)]
            for (ps, pr), (os_, or_) in zip(part, out):
                _lib.call("coati_ivf_merge", ptr(ps), ptr(pr), ptr(table), ptr(pair_slot), P, ptr(list_off), L, Q, nprobe, k, seg_rows, segs,
                          ptr(os_), ptr(or_), s)
            assert _bits(out[0], out[1]), label
            if nprobe > 1:
                live = table[Q // 2, :nprobe // 2].long()
                assert int((out[0][1][Q // 2] >= 0).sum()) == min(k, int(sizes[live].sum())), label     # the -1 entries name no list
    assert written > 0
    log(f"ivfpq bits E={E}: {n} cases, {written} written rows equal coati_ivf_scan at width {2 * E}")


# ---- integer data: exact in any order -----------------------------------------------------------------------------------------------------
def _int_index(E, sizes, seed, distinct=None):
    """an IvfPqIndex ("l2", no bf16 rows) through the constructor: integer centres, entries and so x_hat of magnitude <= 30; distinct: the
    positions of the LAST list draw their code vectors from that many"""
    from coati_amd.ivfpq import IvfPqIndex
    g = torch.Generator().manual_seed(seed)
    n, nl = sum(sizes), len(sizes)
    cb = pq_util.int_codebooks(E // 8, seed)
    centres = _ints((nl, E), seed + 1, -15, 15)
    codes = torch.randint(0, 256, (n, E // 8), generator=g, dtype=torch.uint8)
    ids, off = ivf_util.inverted(_hand_assign(seed, sizes), nl)
    if distinct:
        lo = int(off[-2])
        codes[lo:] = codes[lo:lo + distinct][torch.randint(0, distinct, (n - lo,), generator=g)]
    lists = U.position_lists(off)
    entry = cb[torch.arange(E // 8)[None, :], codes.long()].reshape(n, E)
    bias = -((centres[lists].double() + entry.double()) ** 2).sum(dim=1).float()
    return IvfPqIndex(E, E, "l2", n, centres, codes, cb, ids, bias, off[1:] - off[:-1], device=DEV)


# ---- 2. dead rows, padding and ties -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 64])
def test_dead_rows_padding_and_ties(k):
    sizes = [50, 5, 300]
    ivfpq = _int_index(64, sizes, 21, distinct=7)
    q = _ints((17, 64), 22, -15, 15)
    dead = ivfpq.ids[0::3].long().cpu()                                                         # a third of the rows: every third position
    ivfpq.remove(dead)
    assert int((ivfpq.bias == NEG_INF).sum()) == dead.numel()
    every = torch.arange(3).repeat(17, 1)
    for seg_rows in (64, None):
        s, r = ivfpq.search(q, k, probes=every, seg_rows=seg_rows)
        ws, wr, _ = U.scan(ivfpq, q, every, k)
        _equals((s, r), (ws, wr), f"dead rows k={k} seg_rows={seg_rows}")
        assert not set(dead.tolist()) & set(r.flatten().tolist())
    # the 300 positions of list 2 hold 7 code vectors: equal scores, which come back in ascending original row
    only = torch.full((17, 2), -1, dtype=torch.int64)
    only[:, 1] = 2
    s, r = ivfpq.search(q, k, probes=only)
    _equals((s, r), U.scan(ivfpq, q, only, k)[:2], f"ties k={k}")
    assert int(s[0].unique().numel()) <= 7 < k
    same = s[:, 1:] == s[:, :-1]
    assert bool(same.any()) and bool((r[:, 1:] > r[:, :-1])[same].all())
    # list 1 has 5 rows, fewer alive: the tail is padding
    few = torch.full((17, 3), -1, dtype=torch.int64)
    few[:, 2] = 1
    alive = int((ivfpq.bias[50:55] > NEG_INF).sum())                                            # (positions 51 and 54 are dead)
    s, r = ivfpq.search(q, k, probes=few)
    _equals((s, r), U.scan(ivfpq, q, few, k)[:2], f"padding k={k}")
    assert 0 < alive < 5 and bool((r[:, alive:] == -1).all() and (s[:, alive:] == NEG_INF).all() and (r[:, :alive] >= 0).all())


# ---- 3. exact data against the float64 oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,Q,k", [(32, 1, 1), (64, 33, 10), (256, 17, 64)])
def test_integer_data_equal_the_float64_oracle(E, Q, k):
    """centres, entries and queries are integers of magnitude <= 15: every partial sum of the 2 E products is an integer below 2^24 and
    exact in any order, and so is the l2 bias; stage 1 alone must be the oracle's rows and scores"""
    ivfpq = _int_index(E, SIZES, 30 + E)
    assert not ivfpq.keep_rows and ivfpq.sizes.tolist() == SIZES
    q = _ints((Q, E), 31 + E, -15, 15)
    table = torch.stack([torch.randperm(L, generator=torch.Generator().manual_seed(i))[:3] for i in range(Q)])
    table[0, 2] = -1
    for seg_rows, blocks in ((64, 0), (128, 3), (None, 0)):
        got = ivfpq.search(q, k, probes=table, seg_rows=seg_rows, blocks=blocks)
        _equals(got, U.scan(ivfpq, q, table, k)[:2], f"integers E={E} Q={Q} k={k} seg_rows={seg_rows} blocks={blocks}")
    every = torch.arange(L).repeat(Q, 1)
    _equals(ivfpq.search(q, k, probes=every), U.scan(ivfpq, q, every, k)[:2], f"integers E={E} Q={Q} k={k} every list")


# ---- 4. a library the codes hold without loss ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [64, 256])
def test_lossless_library_equals_the_bf16_ivf(E):
    """rows composed as centre + entry of integers: the residual IS the entry, the codes name it, x_hat is the row, and stage 1's candidates
    are ranked by the exact score: two stages equal IVFIndex.search on the same lists bit for bit, the exact search with every list probed"""
    from coati_amd.ivf import IVFIndex
    from coati_amd.ivfpq import IvfPqIndex, k_max as ivfpq_k_max
    Q, k = 33, 10
    cb = pq_util.int_codebooks(E // 8, 40 + E)
    entries, codes = pq_util.composed_rows(cb, N, 41 + E)
    centres = _ints((L, E), 42 + E, -15, 15)
    assign = _hand_assign()
    x = entries + centres[assign.long()]
    q = _ints((Q, E), 43 + E, -15, 15)
    index = _index(x, "l2")
    ivf = IVFIndex.build(index, L, centres=centres, assign=assign)
    ivfpq = IvfPqIndex.build(index, L, centres=centres, assign=assign, codebooks=cb)
    assert ivfpq.keep_rows and ivfpq._rows16.data_ptr() == index.vectors.data_ptr() and torch.equal(ivfpq.ids, ivf.ids)
    assert torch.equal(ivfpq.codes.cpu(), codes[ivfpq.ids.long().cpu()])                      # the codes name the composing entries
    assert torch.equal(ivfpq.dequantised(), ivf.vectors.float()) and torch.equal(ivfpq.bias, ivf.bias)
    want = ivf.search(q, k, nprobe=3, return_probes=True)
    got = ivfpq.search(q, k, nprobe=3, return_probes=True)
    assert torch.equal(got[2], want[2]) and _bits(got, want)
    assert _bits(ivfpq.search(q, k, nprobe=3, rescore=False), want)                          # stage 1 alone has the exact bits too
    assert _bits(ivfpq.search(q, k, nprobe=L), index.search(q, k))
    _equals(ivfpq.search(q, k, nprobe=L), search_util.index_search(index, q, k)[:2], f"lossless l2 E={E}")
    # "cosine": the normalised rows and centres are no integers, so neither the residuals nor the scores are exact and the library is
    # not lossless; rows only, against the float64 oracle of the two stages (the bf16 IVF's rows are logged next to them)
    index = _index(x, "cosine")
    ivf = IVFIndex.build(index, L, centres=centres, assign=assign)
    ivfpq = ivf.pq(index, pq_iters=4)
    R = min(4 * k, ivfpq_k_max(E))
    _, r_pq, probes = ivfpq.search(q, k, nprobe=3, return_probes=True)
    r_ivf = ivf.search(q, k, probes=probes)[1]
    want = U.two_stage(ivfpq, index, q, probes, k, R)[1]
    log(f"ivfpq lossless library, cosine E={E}: {int((r_pq.cpu() != want).sum())} of {r_pq.numel()} rows differ from the two-stage oracle's, "
        f"{int((r_pq != r_ivf).sum())} from the bf16 IVF's")
    assert torch.equal(r_pq.cpu(), want)


# ---- 5. a lossy Gaussian library ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [64, 256])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_gaussian_library(metric, E):
    """Two stages: every returned score has the bits index.search gives that row (searched again with every other row masked out).
    Stage 1 against the float64 oracle on x_hat = centre + entry: a product of two bf16 values is exact in f32, so with u = 2^-24 the f32
    accumulation of the 2 E products differs from the exact sum by at most 2 E u sum_j |q_j| |x_hat_j| in any order (both halves of
    x_hat counted on their own), times alpha; the epilogue alpha * acc + bias rounds once more, u |score|; for l2 the finish subtracts
    |q|^2 summed in f32 (E u |q|^2) and rounds once (u |score|).  A row may stand in another's place only where the oracle's scores are
    within the two rows' bounds of each other."""
    from coati_amd import search as S
    from coati_amd.ivfpq import IvfPqIndex
    n, Q, k, nlist = 5000, 33, 10, 32
    g = torch.Generator().manual_seed(50 + E)
    x, q = torch.randn(n, E, generator=g), torch.randn(Q, E, generator=g)
    index = _index(x, metric)
    ivfpq = IvfPqIndex.build(index, nlist, centres=x[:nlist], pq_iters=4, sample=4096)
    assert ivfpq.keep_rows
    # two stages
    s2, r2 = ivfpq.search(q, k, nprobe=8)
    assert bool((r2 >= 0).all()) and bool((s2[:, 1:] <= s2[:, :-1]).all())
    for i in range(Q):
        mask = torch.full((n,), NEG_INF, device=DEV)
        mask[r2[i]] = 0.0
        es, er = index.search(q[i:i + 1], k, bias=mask)
        assert torch.equal(er[0], r2[i]) and torch.equal(es[0].view(torch.int32), s2[i].view(torch.int32)), i
    # stage 1
    s, r, probes = ivfpq.search(q, k, nprobe=8, rescore=False, return_probes=True)
    s, r = s.cpu(), r.cpu()
    ws, wr, full = U.scan(ivfpq, q, probes, k + 1)                                           # full [Q, M] by position, -inf outside the probed lists
    _, q16 = S.prepare_queries(q, metric, E, "cpu")
    alpha, u = S.metric_alpha(metric), 2.0 ** -24
    lists = U.position_lists(ivfpq.list_offsets)
    cb, codes = ivfpq.codebooks.cpu(), ivfpq.codes.cpu().long()
    entry = cb[torch.arange(E // 8)[None, :], codes].reshape(codes.shape[0], E)
    mag = q16.double().abs() @ (ivfpq.centres16.cpu()[lists].double().abs() + entry.double().abs()).T     # [Q, M]: sum_j |q_j| (|c_j| + |e_j|)
    qn = (q16.double() ** 2).sum(dim=1, keepdim=True)
    raw = full + qn if metric == "l2" else full                                             # (where the clamp at 0 did not act; else the bound is only larger)
    b = alpha * 2 * E * u * mag + u * raw.abs().clamp_max(1e30)
    if metric == "l2":
        b = b + E * u * qn + u * full.abs().clamp_max(1e30)
    b = 1.001 * b                                                                             # (the terms of second order in u)
    pos = ivfpq._inverse.cpu()[r]
    assert bool((r >= 0).all()) and bool((pos >= 0).all())
    of_returned, b_returned = full.gather(1, pos), b.gather(1, pos)
    assert bool((of_returned > NEG_INF).all())                                                # every returned row is in a probed list
    err = (s.double() - of_returned).abs()
    log(f"ivfpq gaussian {metric} E={E}: largest stage-1 score error {float(err.max()):.3e}, bound between {float(b_returned.min()):.3e} and "
        f"{float(b_returned.max()):.3e}; {int((r != wr[:, :k]).sum())} of {r.numel()} rows differ from the oracle's order; two-stage recall "
        f"against the exact search {ivf_util.recall(r2, index.search(q, k)[1]):.3f}")
    assert bool((err <= b_returned).all())
    bmax = b.where(full > NEG_INF, torch.zeros_like(b)).amax(dim=1, keepdim=True)
    assert bool((of_returned >= ws[:, k - 1:k] - b_returned - bmax).all())                    # every returned row belongs, to the bounds
    clear = full > ws[:, k:k + 1] + b + bmax                                                  # probed rows that clearly beat the (k + 1)-th ...
    returned = torch.zeros_like(clear)
    returned.scatter_(1, pos, True)
    assert bool((returned | ~clear).all())                                                    # ... are all returned
    assert bool((s[:, 1:] <= s[:, :-1]).all())


# ---- 6. index behaviour ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescore", [False, True])
def test_bias_removal_and_probes(rescore):
    """a lossless integer library, so that both stages have the exact search's oracle: bias= by original row in both stages, remove(),
    probes= and return_probes"""
    from coati_amd.ivfpq import IvfPqIndex
    E, Q, k = 64, 17, 7
    cb = pq_util.int_codebooks(E // 8, 60)
    entries, _ = pq_util.composed_rows(cb, N, 61)
    centres = _ints((L, E), 62, -15, 15)
    assign = _hand_assign(1)
    x, q = entries + centres[assign.long()], _ints((Q, E), 63, -15, 15)
    index = _index(x)
    ivfpq = IvfPqIndex.build(index, L, centres=centres, assign=assign, codebooks=cb)
    every = torch.arange(L).repeat(Q, 1)

    def search(**kw):
        return ivfpq.search(q, k, probes=every, rescore=rescore, **kw)

    def oracle():
        return search_util.index_search(index, q, k)[:2]

    s0, r0 = search()
    _equals((s0, r0), oracle(), f"all lists rescore={rescore}")
    s, r, t = search(return_probes=True)
    assert torch.equal(t.cpu(), every) and t.dtype == torch.int64 and _bits((s, r), (s0, r0))
    s, r, t = ivfpq.search(q, k, nprobe=2, rescore=rescore, return_probes=True)
    assert torch.equal(t, ivfpq.probe(q, 2)) and _bits(ivfpq.search(q, k, probes=t, rescore=rescore), (s, r))
    _equals((s, r), U.scan(ivfpq, q, t, k)[:2], f"nprobe=2 rescore={rescore}")               # (lossless: stage 1's oracle is the exact one)
    extra = _ints((N,), 64, -30, 30).to(DEV)
    extra[int(r0[1, 0])] = NEG_INF
    index.bias.add_(extra)
    _equals(search(bias=extra), oracle(), f"bias= rescore={rescore}")
    assert int(r0[1, 0]) not in search(bias=extra)[1].flatten().tolist()
    index.bias.copy_(ivfpq._bias16)
    ivfpq.remove(r0[0, :3])
    index.remove(r0[0, :3])
    s1, r1 = search()
    _equals((s1, r1), oracle(), f"3 rows removed rescore={rescore}")
    assert not set(r0[0, :3].tolist()) & set(r1.flatten().tolist()) and r1[0, :k - 3].tolist() == r0[0, 3:].tolist()


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_build_from_ivf_and_save_load(metric, tmp_path):
    from coati_amd import pq
    from coati_amd.ivf import IVFIndex
    from coati_amd.ivfpq import IvfPqIndex
    g = torch.Generator().manual_seed(71)
    x = torch.randn(5000, 96, generator=g) + 3 * torch.randn(32, 96, generator=g)[torch.randint(0, 32, (5000,), generator=g)]
    index = _index(x, metric)
    index.remove([5, 77])
    ivfpq, ivf = index.ivfpq(32, pq_iters=3, sample=2048), index.ivf(32)
    assert isinstance(ivfpq, IvfPqIndex) and isinstance(ivf, IVFIndex) and ivfpq.keep_rows and int(ivfpq.sizes.sum()) == 4998
    assert torch.equal(ivfpq.ids, ivf.ids) and torch.equal(ivfpq.sizes, ivf.sizes) and torch.equal(ivfpq.centres, ivf.centres)
    # the storage rule on the device: the kernel's codes are the plain-torch rule's on the float64 restatement of the residuals
    r16 = U.residuals(index.vectors, ivfpq.ids, ivfpq.list_offsets, ivfpq.centres16)
    assert torch.equal(ivfpq.codes.cpu(), pq.encode_rows(r16, ivfpq.codebooks.cpu()))
    want = U.x_hat(ivfpq)
    assert torch.equal(ivfpq.bias.cpu(), -(want ** 2).sum(dim=1).float() if metric == "l2" else torch.zeros(4998))
    again = ivf.pq(index, pq_iters=3, sample=2048)                                           # from_ivf equals build with the same arguments
    for name in ("codebooks", "codes", "bias", "ids", "sizes", "centres16"):
        assert torch.equal(getattr(again, name), getattr(ivfpq, name)), name
    assert again._rows16.data_ptr() == index.vectors.data_ptr() and not ivf.pq(codebooks=ivfpq.codebooks).keep_rows
    q = x[:19] + 0.1 * torch.randn(19, 96, generator=g)
    for keep_rows in (True, False):
        src = ivfpq if keep_rows else index.ivfpq(32, keep_rows=False, codebooks=ivfpq.codebooks)
        assert src.keep_rows == keep_rows and torch.equal(src.codes, ivfpq.codes)
        path = str(tmp_path / f"ivfpq_{keep_rows}.pt")
        src.save(path)
        back = IvfPqIndex.load(path, device=DEV)
        assert back.keep_rows == keep_rows and torch.equal(back.codes, src.codes) and torch.equal(back.codebooks, src.codebooks)
        assert _bits(src.search(q, 10, nprobe=4), back.search(q, 10, nprobe=4))
    _, want_rows = ivf.search(q, 10, nprobe=4)
    log(f"ivfpq build {metric}: recall@10 of the two stages against the bf16 IVF {ivf_util.recall(ivfpq.search(q, 10, nprobe=4)[1], want_rows):.3f}")


def test_from_strings(golden_dir):
    from coati.generative import build_index, nearest_smiles
    from coati_amd.ivfpq import IvfPqIndex
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
        index, kept = build_index(given, model, tk, batch_size=16, canon_smiles=_canon, nlist=4, list_dtype="pq")
        near = nearest_smiles(kept + ["CXC"], index, kept, model, tk, k=3, canon_smiles=_canon)      # the default nprobe covers the four lists
    assert isinstance(index, IvfPqIndex) and index.keep_rows and kept == strings and len(index) == 40 and index.nlist == 4
    assert near[-1] == [] and len(near) == len(kept) + 1
    for s, hits in zip(kept, near):
        assert len(hits) == 3 and hits[0][0] == s, (s, hits)                   # 40 rows, 256 entries: every row has its own, and finds itself first
        assert [v for _, v in hits] == sorted((v for _, v in hits), reverse=True)
        assert abs(hits[0][1] - 1.0) <= 1e-2                                   # the exact score of the bf16 rows


# ---- 7. recall ---------------------------------------------------------------------------------------------------------------------------------
def _every_list(search, Q, nlist, R):
    """stage 1's best R of ALL nlist = 256 lists, which is more than one search may probe (128): the two halves of the lists searched
    apart and their results merged by score -- the best R of a union are among the best R of its parts.  search(probes, R) -> (scores,
    rows) [Q, R]."""
    halves = [search(torch.arange(lo, lo + nlist // 2).repeat(Q, 1), R) for lo in (0, nlist // 2)]
    s, r = torch.cat([h[0] for h in halves], dim=1), torch.cat([h[1] for h in halves], dim=1)
    top = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :R]
    return s.gather(1, top), r.gather(1, top)


def test_recall_is_not_below_flat_pq():
    """the clustered library of the fp8 and PQ tests (200 true centres), 256 lists, nprobe = 256 (every list), code books of both indices from
    seed 0, 8 rounds, 4096 sampled rows: residual codes must not lose to the flat PQIndex's at stage 1 nor after re-scoring at oversample 2
    and 4.  One search probes at most 128 lists, so every list is probed as two halves whose stage-1 candidates are merged (_every_list)
    and re-scored by the same stage 2 (rescore_candidates).  The bf16 IVF over every list is the ceiling.  Measured on the MI355X:
    DESIGN.md section 6, "Quantised inverted lists"."""
    from coati_amd.fp8_index import rescore_candidates
    from coati_amd.search import prepare_queries
    n, E, Q, k, nlist = 20000, 64, 64, 10, 256
    draw = pq_util.clustered(n, E, 31)
    x, q = draw(n), draw(Q)
    index = _index(x, "cosine")
    _, exact = index.search(q, k)
    flat = index.pq(seed=0, iters=8, sample=4096)
    ivfpq = index.ivfpq(nlist, iters=10, seed=0, pq_seed=0, pq_iters=8, sample=4096)
    ivf = index.ivf(nlist, iters=10, seed=0)
    assert torch.equal(ivf.ids, ivfpq.ids) and int((ivfpq.sizes > 0).sum()) > 128
    _, q16 = prepare_queries(q, "cosine", E, DEV)
    ceiling = ivf_util.recall(_every_list(lambda probes, R: ivf.search(q, R, probes=probes), Q, nlist, k)[1], exact)
    got = {"flat": [flat.search(q, k, rescore=False)[1]] + [flat.search(q, k, oversample=o)[1] for o in (2, 4)], "ivfpq": []}
    for R in (k, 2 * k, 4 * k):                                                               # stage 1 alone, oversample 2 and 4
        _, cand = _every_list(lambda probes, R: ivfpq.search(q, R, probes=probes, rescore=False), Q, nlist, R)
        got["ivfpq"].append(cand if R == k else rescore_candidates(index.vectors, index.bias, q16, cand.contiguous(), k)[1])
    got = {name: [ivf_util.recall(rows, exact) for rows in lists] for name, lists in got.items()}
    nprobe = nlist
    log(f"ivfpq recall@10, {n} x {E} clustered, {nlist} lists, nprobe {nprobe}: stage 1 / oversample 2 / oversample 4 = "
        + " / ".join(f"{v:.3f}" for v in got["ivfpq"]) + "; flat PQ " + " / ".join(f"{v:.3f}" for v in got["flat"])
        + f"; the bf16 IVF {ceiling:.3f}")
    for mine, theirs, what in zip(got["ivfpq"], got["flat"], ("stage 1", "oversample 2", "oversample 4")):
        assert mine >= theirs, (what, mine, theirs)
