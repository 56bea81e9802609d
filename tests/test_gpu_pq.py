"""Product-quantised search on the GPU (include/coati_pq.h, coati_amd/pq.py): the encoder byte for byte against its plain-torch
restatement, the scan over the codes against coati_search_topk on the reconstructed bf16 library BIT FOR BIT, and PQIndex.search's two
stages against EmbeddingIndex.search."""
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
from tests import pq_util as U, search_util  # noqa: E402
from tests.gpu_util import log  # noqa: E402
from tests.search_util import canon as _canon, ints as _ints, strings as _strings  # noqa: E402

DEV = "cuda:0"
NEG_INF = float("-inf")
SMALL = dict(n_layer_e3gnn=2, n_layer_xformer=2, n_hidden_xformer=64, n_hidden_e3nn=64, n_embd_common=64, n_head=4, n_seq=24, n_tok=48)


def _index(vectors, metric="dot", **kw):
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(vectors.shape[1], metric=metric, device=DEV, **kw)
    assert index.add(vectors) == range(0, vectors.shape[0])
    return index


def _out(Q, k, S):
    return (torch.empty(Q * S * k, dtype=torch.float32, device=DEV), torch.empty(Q * S * k, dtype=torch.int32, device=DEV),
            torch.full((Q, k), 7.0, dtype=torch.float32, device=DEV), torch.full((Q, k), -7, dtype=torch.int64, device=DEV))


def _pq_topk(codes, cb, bias, q16, k, alpha, S):
    from coati_amd import _lib
    from coati_amd.ops import ptr, stream
    Q = q16.shape[0]
    ps, pr, s, r = _out(Q, k, S)
    _lib.call("coati_pq_topk", ptr(codes), codes.shape[0], codes.shape[1] * 8, ptr(cb), ptr(bias), ptr(q16), Q, k, float(alpha), S, ptr(ps), ptr(pr),
              ptr(s), ptr(r), stream())
    return s, r


def _search_topk(x16, bias, q16, k, alpha, S=1):
    from coati_amd import _lib
    from coati_amd.ops import ptr, stream
    Q = q16.shape[0]
    ps, pr, s, r = _out(Q, k, S)
    _lib.call("coati_search_topk", ptr(x16), x16.shape[0], x16.shape[1], ptr(bias), ptr(q16), Q, k, float(alpha), S, ptr(ps), ptr(pr), ptr(s), ptr(r),
              stream())
    return s, r


def _same_bits(got, want, label):
    (s, r), (ws, wr) = got, want
    bad_r, bad_s = int((r != wr).sum()), int((s.view(torch.int32) != ws.view(torch.int32)).sum())
    assert bad_r == 0 and bad_s == 0, f"{label}: {bad_r} rows and {bad_s} score bit patterns of {r.numel()} differ from coati_search_topk's"


def _library(N, E, seed, distinct=256):
    """random codes under Gaussian bf16 code books, the reconstructed bf16 rows, a Gaussian bias"""
    from coati_amd import pq as P
    g = torch.Generator().manual_seed(seed)
    cb = torch.randn(E // 8, 256, 8, generator=g).to(torch.bfloat16).to(DEV)
    codes = torch.randint(0, distinct, (N, E // 8), generator=g).to(torch.uint8).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    return cb, codes, P.reconstruct(codes, cb).contiguous(), bias


# ---- 1. the encoder, byte for byte ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [32, 96, 256])
@pytest.mark.parametrize("n", [1, 63, 1000])
def test_encoder_equals_the_torch_restatement(n, E):
    from coati_amd import pq as P
    # integers of magnitude <= 15: every operation of the rule is exact, ties (duplicate entries) included
    cb = U.int_codebooks(E // 8, E + n, duplicates=True)
    rows, codes = U.composed_rows(cb, n, 2 * E + n, 128)
    x = torch.cat([_ints((n, E), 3 * E + n, -15, 15), rows])[torch.randperm(2 * n, generator=torch.Generator().manual_seed(n))][:n].to(torch.bfloat16)
    want = P.encode_rows(x, cb)                                                    # on the CPU
    got = P.encode_device(x.to(DEV), cb.to(DEV))
    assert got.dtype == torch.uint8 and got.shape == (n, E // 8)
    bad = int((got.cpu() != want).sum())
    log(f"pq encoder integers n={n} E={E}: {bad} of {got.numel()} bytes differ")
    assert bad == 0 and int(want.max()) < 128
    # Gaussian data: the chosen entry's float64 distance is within (1 + 4e-6) of the smallest (nine f32 roundings of 2^-24 on each of
    # two distances, times four); the bytes are reported against the restatement's
    g = torch.Generator().manual_seed(5 * E + n)
    x = torch.randn(n, E, generator=g).to(torch.bfloat16)
    cb = torch.randn(E // 8, 256, 8, generator=g).to(torch.bfloat16)
    got = P.encode_device(x.to(DEV), cb.to(DEV)).cpu()
    d = U.distances64(x, cb)
    chosen = d.gather(2, got.to(torch.int64)[:, :, None])[:, :, 0]
    log(f"pq encoder gaussian n={n} E={E}: {int((got != P.encode_rows(x, cb)).sum())} of {got.numel()} bytes differ from encode_rows, "
        f"largest chosen / smallest distance - 1 = {float((chosen / d.amin(dim=2)).max()) - 1:.3e}")
    assert bool((chosen <= (1 + 4e-6) * d.amin(dim=2)).all())


# ---- 2. the scan equals coati_search_topk on the reconstructed rows, bit for bit --------------------------------------------------------------
@pytest.mark.parametrize("E", [32, 96, 256])
def test_scan_has_the_exact_search_bits_on_the_reconstructed_rows(E):
    from coati_amd import pq as P
    km = P.k_max(E)
    g = torch.Generator().manual_seed(E)
    q_all = torch.randn(33, E, generator=g).to(torch.bfloat16).to(DEV)
    cases = 0
    for N in (1, 63, 64, 65, 1000):
        cb, codes, x_hat, bias = _library(N, E, 10 * E + N)
        for Q in (1, 16, 17, 33):
            q16 = q_all[:Q].contiguous()
            for k in (1, 10, km):
                for alpha in (1.0, 2.0):
                    want = _search_topk(x_hat, bias, q16, k, alpha)
                    for S in (1, 2, 5, 40):                                        # (40 slices of 64 rows and more: most lie past the end)
                        _same_bits(_pq_topk(codes, cb, bias, q16, k, alpha, S), want, f"N={N} E={E} Q={Q} k={k} alpha={alpha} S={S}")
                        cases += 1
                    if k > N:
                        assert bool((want[1][:, N:] == -1).all() and (want[1][:, :N] >= 0).all())
    log(f"pq scan E={E}: {cases} cases equal coati_search_topk on the reconstructed rows bit for bit (k_max = {km})")


@pytest.mark.parametrize("E", [32, 96, 256])
def test_scan_with_dead_rows_padding_and_ties(E):
    from coati_amd import pq as P
    km = P.k_max(E)
    g = torch.Generator().manual_seed(100 + E)
    q16 = torch.randn(17, E, generator=g).to(torch.bfloat16).to(DEV)
    # a third of the rows have -inf bias
    cb, codes, x_hat, bias = _library(1000, E, 200 + E)
    bias[::3] = NEG_INF
    for k, S in ((10, 1), (km, 5)):
        s, r = _pq_topk(codes, cb, bias, q16, k, 1.0, S)
        _same_bits((s, r), _search_topk(x_hat, bias, q16, k, 1.0), f"a third dead E={E} k={k}")
        assert bool((r % 3 != 0).all())
    # fewer than k rows alive: the tail is padding
    bias[:] = NEG_INF
    bias[[5, 64, 65, 700, 999]] = torch.tensor([0.5, -1.0, 0.0, 2.0, 0.25], device=DEV)
    for S in (1, 2, 40):
        s, r = _pq_topk(codes, cb, bias, q16, 10, 2.0, S)
        _same_bits((s, r), _search_topk(x_hat, bias, q16, 10, 2.0), f"5 alive E={E} S={S}")
        assert bool((r[:, 5:] == -1).all() and (s[:, 5:] == NEG_INF).all() and (r[:, :5] >= 0).all())
    # 300 rows drawn from 7 distinct code vectors, no bias: ties by ascending row
    cb, codes7, _, _ = _library(7, E, 300 + E)
    pick = torch.randint(0, 7, (300,), generator=g).to(DEV)
    codes = codes7[pick].contiguous()
    x_hat = P.reconstruct(codes, cb).contiguous()
    zero = torch.zeros(300, device=DEV)
    for k, S in ((10, 1), (km, 2), (km, 5)):
        s, r = _pq_topk(codes, cb, zero, q16, k, 1.0, S)
        _same_bits((s, r), _search_topk(x_hat, zero, q16, k, 1.0), f"ties E={E} k={k} S={S}")
        same = s[:, 1:] == s[:, :-1]
        assert int(same.sum()) > 0 and bool((r[:, 1:] > r[:, :-1])[same].all())
    # and against the float64 oracle (the scores are not exact here; the rows of equal code vectors must come in ascending order)
    ws, wr = search_util.search(x_hat.cpu(), None, q16.cpu(), 5)
    s, r = _pq_topk(codes, cb, zero, q16, 5, 1.0, 1)
    assert bool((pick[r] == pick[wr.to(DEV)]).all())


# ---- 3. PQIndex.search ---------------------------------------------------------------------------------------------------------------------
def _lossless(metric, N, E, seed):
    cb = U.int_codebooks(E // 8, seed)
    rows, codes = U.composed_rows(cb, N, seed + 1)
    return _index(rows, metric=metric), cb, rows, codes


@pytest.mark.parametrize("metric", ["dot", "l2"])
@pytest.mark.parametrize("E", [64, 256])
def test_lossless_library_two_stages_equal_the_exact_search(metric, E):
    """rows composed from the code books' own entries: stage 1's scores are the exact ones, so the exact top k are its first k
    candidates by construction and the result must be EmbeddingIndex.search's, rows and score BITS"""
    N, Q, k = 3000, 33, 10
    index, cb, rows, codes = _lossless(metric, N, E, 400 + E)
    pq = index.pq(codebooks=cb.to(DEV))
    assert torch.equal(pq.codes.cpu(), codes) and torch.equal(pq.dequantised(), index.vectors) and pq.keep_rows
    q = _ints((Q, E), 9, -15, 15)
    ws, wr = index.search(q, k)
    for kw in (dict(), dict(oversample=2), dict(oversample=1), dict(slices=3), dict(rescore=False)):
        s, r = pq.search(q, k, **kw)
        assert s.dtype == torch.float32 and r.dtype == torch.int64
        assert torch.equal(r, wr) and torch.equal(s.view(torch.int32), ws.view(torch.int32)), kw
    os_, or_, _ = search_util.index_search(index, q, k)
    assert torch.equal(wr.cpu(), or_.cpu()) and torch.equal(ws.double().cpu(), os_.cpu())
    bare = index.pq(keep_rows=False, codebooks=cb.to(DEV))
    s, r = bare.search(q, k)
    assert torch.equal(r, wr) and torch.equal(s.view(torch.int32), ws.view(torch.int32))
    with pytest.raises(ValueError, match="1 .. "):
        pq.search(q, bare_k_max(E) + 1)


def bare_k_max(E):
    from coati_amd import pq as P
    return P.k_max(E)


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_lossy_library_returns_exact_scores_of_its_rows(metric):
    """code books trained on other Gaussian rows: stage 1 may miss some of the exact top k, but every returned score has index.search's bits
    for its row (N <= 128: index.search(q, N) lists every row's score), in search order"""
    from coati_amd import pq as P
    N, Q, k, E = 120, 17, 10, 96
    g = torch.Generator().manual_seed(50)
    index = _index(torch.randn(N, E, generator=g), metric=metric)
    q = torch.randn(Q, E, generator=g)
    books = P.fit_codebooks(torch.randn(2000, E, generator=g).to(torch.bfloat16).to(DEV), iters=3)       # not these rows: a lossy code
    pq = index.pq(codebooks=books)
    assert not torch.equal(pq.dequantised(), index.vectors)
    all_s, all_r = index.search(q, N)
    exact = torch.empty(Q, N, dtype=torch.float32, device=DEV).scatter_(1, all_r, all_s)
    s, r = pq.search(q, k, oversample=2)
    assert bool((r >= 0).all()) and torch.equal(s.view(torch.int32), exact.gather(1, r).view(torch.int32))
    assert bool(((s[:, 1:] < s[:, :-1]) | ((s[:, 1:] == s[:, :-1]) & (r[:, 1:] > r[:, :-1]))).all())
    log(f"pq lossy {metric}: {int((r == all_r[:, :k]).sum())} of {r.numel()} results are the exact search's at R = 20 of {N} rows")
    s, r = pq.search(q, k, oversample=12)                                          # R = 120 = every row: the exact search
    assert torch.equal(r, all_r[:, :k]) and torch.equal(s.view(torch.int32), all_s[:, :k].view(torch.int32))


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
@pytest.mark.parametrize("keep_rows", [False, True])
def test_stage_1_alone_against_the_float64_oracle(metric, keep_rows):
    """The oracle is the float64 score of the query against the RECONSTRUCTED rows.  The tolerance is the fp8 search's stage-1 one
    (tests/test_gpu_search8.py): a product of two bf16 values is exact in f32, so the error is the accumulation's alone,
    b = alpha E 2^-23 |q| |x_hat|; every score within b, every returned row within 2 b of belonging, every clear winner returned."""
    from coati_amd import search as S
    N, Q, k, E = 5000, 33, 10, 256
    g = torch.Generator().manual_seed(60)
    index = _index(torch.randn(N, E, generator=g), metric=metric)
    q = torch.randn(Q, E, generator=g)
    pq = index.pq(keep_rows=keep_rows, iters=2, sample=2048)
    s, r = pq.search(q, k, rescore=False)
    s, r = s.cpu(), r.cpu()
    full, q16 = U.stage1_scores(pq, q)
    ws, wr = search_util.topk(full, k + 1)
    b = S.metric_alpha(metric) * E * 2.0 ** -23 * q16.double().norm(dim=1, keepdim=True) * pq.dequantised().cpu().double().norm(dim=1)[None, :]
    assert bool((r >= 0).all())
    of_returned, b_returned = full.gather(1, r), b.gather(1, r)
    err = (s.double() - of_returned).abs()
    log(f"pq stage 1 {metric} keep_rows={keep_rows}: largest score error {float(err.max()):.3e}, bound b from {float(b.min()):.3e}; "
        f"{int((r != wr[:, :k]).sum())} of {r.numel()} rows differ from the oracle's order")
    assert bool((err <= b_returned).all())
    assert bool((of_returned >= ws[:, k - 1:k] - 2 * b_returned).all())
    clear = full > ws[:, k:k + 1] + 2 * b
    returned = torch.zeros_like(clear)
    returned.scatter_(1, r, True)
    assert bool((returned | ~clear).all())
    assert bool((s[:, 1:] <= s[:, :-1]).all())


def test_bias_remove_save_and_load_on_the_device(tmp_path):
    from coati_amd import pq as P
    N, Q, k, E = 900, 17, 7, 64
    index, cb, rows, _ = _lossless("dot", N, E, 70)
    q = _ints((Q, E), 6, -15, 15)
    pq = index.pq(codebooks=cb.to(DEV))
    for rescore in (False, True):
        extra = _ints((N,), 8, -30, 30).to(DEV)                                    # an integer bias is added exactly, in both stages
        index.bias.add_(extra)
        ws, wr, _ = search_util.index_search(index, q, k)
        s, r = pq.search(q, k, rescore=rescore, bias=extra)
        assert torch.equal(r.cpu(), wr.cpu()) and torch.equal(s.double().cpu(), ws.cpu()), rescore
        index.bias.sub_(extra)
    s0, r0 = pq.search(q, k)
    pq.remove(r0[0, :3])
    index.remove(r0[0, :3])
    ws, wr, _ = search_util.index_search(index, q, k)
    for rescore in (False, True):
        s1, r1 = pq.search(q, k, rescore=rescore)
        assert torch.equal(r1.cpu(), wr.cpu()) and torch.equal(s1.double().cpu(), ws.cpu()) and r1[0, :k - 3].tolist() == r0[0, 3:].tolist()
    path = str(tmp_path / "pq.pt")
    pq.save(path)
    again = P.PQIndex.load(path, device=DEV)
    assert again.keep_rows and torch.equal(again.codes, pq.codes) and torch.equal(again.bias, pq.bias)
    s2, r2 = again.search(q, k)
    assert torch.equal(r2, r1) and torch.equal(s2, s1)
    gone = [i for i in range(N) if i not in r1[0, :4].tolist()]
    again.remove(gone)
    s3, r3 = again.search(q, k)
    assert bool((r3[:, 4:] == -1).all() and (s3[:, 4:] == NEG_INF).all()) and r3[0, :4].tolist() == r1[0, :4].tolist()


def test_fit_and_chunked_add_equal_the_snapshot():
    from coati_amd import pq as P
    N, E, k = 3000, 96, 10
    g = torch.Generator().manual_seed(80)
    x, q = torch.randn(N, E, generator=g), torch.randn(20, E, generator=g)
    grown = P.PQIndex.fit(x[:1500], E, "cosine", device=DEV, seed=1, iters=3)
    again = P.PQIndex.fit(x[:1500], E, "cosine", device=DEV, seed=1, iters=3)
    assert torch.equal(grown.codebooks.view(torch.int16), again.codebooks.view(torch.int16))          # same seed, same device, same bytes
    assert grown.add(x[:1]) == range(0, 1) and grown.add(x[1:1100]) == range(1, 1100) and grown.add(x[1100:]) == range(1100, N)
    index = _index(x, metric="cosine")
    snap = index.pq(keep_rows=False, codebooks=grown.codebooks)
    assert torch.equal(grown.codes, snap.codes) and torch.equal(grown.bias, snap.bias)
    s, r = grown.search(q, k)
    ws, wr = snap.search(q, k)
    assert torch.equal(r, wr) and torch.equal(s, ws) and bool((r >= 0).all())
    with pytest.raises(RuntimeError, match="snapshot"):
        index.pq(codebooks=grown.codebooks).add(x[:2])


# ---- 4. from strings -------------------------------------------------------------------------------------------------------------------------
def test_from_strings(golden_dir):
    from coati.generative import build_index, build_pq_index, nearest_smiles
    from coati_amd.pq import PQIndex
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
        index, kept = build_pq_index(given, model, tk, batch_size=16, canon_smiles=_canon, iters=3)
        exact, _ = build_index(given, model, tk, batch_size=16, canon_smiles=_canon)
        near = nearest_smiles(kept + ["CXC"], index, kept, model, tk, k=3, canon_smiles=_canon)
        want = nearest_smiles(kept + ["CXC"], exact, kept, model, tk, k=3, canon_smiles=_canon)
    assert isinstance(index, PQIndex) and index.keep_rows and kept == strings and len(index) == 40
    assert near[-1] == [] and len(near) == len(kept) + 1
    # 40 rows, 40 code book entries that ARE the rows: the library is lossless and R = 12 holds the exact top 3
    assert torch.equal(index.dequantised(), index._rows16) and torch.equal(index._rows16, exact.vectors)
    assert near == want
    for s, hits in zip(kept, near):
        assert len(hits) == 3 and hits[0][0] == s, (s, hits)                   # every query string finds itself first
        assert [v for _, v in hits] == sorted((v for _, v in hits), reverse=True)
        assert abs(hits[0][1] - 1.0) <= 1e-2                                   # the exact score of the bf16 rows, as in test_gpu_search.py
