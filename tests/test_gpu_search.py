"""Embedding-library search on the GPU (include/coati_search.h, coati_amd/search.py, coati_amd/generative/coati_search.py) against the
float64 restatement of tests/search_util.py.  Integer data is exact in bf16 and in f32 in any summation order, so those cases must
EQUAL the oracle element for element, ties and padding included; real-valued data is held to a bound derived from f32 accumulation."""
import contextlib
import inspect
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import search_util  # noqa: E402
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


def _exact(index, q, k, label, **kw):
    """search == oracle, element for element; returns the result"""
    s, r = index.search(q, k, **kw)
    ws, wr, _ = search_util.index_search(index, q, k)
    assert s.dtype == torch.float32 and r.dtype == torch.int64 and s.shape == r.shape == (q.shape[0], k)
    bad_r, bad_s = int((r != wr).sum()), int((s.double() != ws).sum())
    log(f"search {label}: {bad_r} rows and {bad_s} scores of {r.numel()} differ from the oracle")
    assert bad_r == 0 and bad_s == 0, label
    return s, r


# ---- 1. exact cases ---------------------------------------------------------------------------------------------------
# N in {1, 15, 16, 17, 63, 64, 65, 1000, 70001}, Q in {1, 15, 16, 17, 64, 65, 130}, k in {1, 7, 64, 128}, E in {32, 96, 256, 512}; k > N
EXACT = [(1, 1, 1, 32), (1, 17, 7, 256), (15, 15, 7, 96), (16, 16, 64, 256), (17, 17, 7, 512), (63, 64, 64, 32), (64, 65, 128, 96),
         (65, 130, 1, 256), (1000, 17, 128, 512), (1000, 130, 64, 256), (1000, 64, 7, 96), (70001, 16, 7, 256), (70001, 65, 128, 512),
         (70001, 1, 64, 96), (70001, 130, 1, 32)]


@pytest.mark.parametrize("N,Q,k,E", EXACT)
def test_integer_data_equals_the_oracle(N, Q, k, E):
    index = _index(_ints((N, E), 1000 + N + E))
    assert len(index) == N and index.vectors.shape == (N, E) and index.vectors.dtype == torch.bfloat16
    s, r = _exact(index, _ints((Q, E), 7 * Q + k), k, f"N={N} Q={Q} k={k} E={E}")
    if k > N:
        assert bool((r[:, N:] == -1).all() and (s[:, N:] == NEG_INF).all() and (r[:, :N] >= 0).all())


# ---- 2. adversarial orders ----------------------------------------------------------------------------------------------
def _ordered_library(kind, N=5000):
    """one query q = (64, 1, 0, ...) and rows (a, b, 0, ...) with small integers a, b: score = 64 a + b, exact"""
    n = torch.arange(N)
    x = torch.zeros(N, 32)
    if kind == "ascending":
        x[:, 0], x[:, 1] = n // 64, n % 64
    elif kind == "descending":
        x[:, 0], x[:, 1] = -(n // 64), -(n % 64)
    elif kind == "constant":
        x[:, 0] = 1
    else:                    # two values in blocks of 100
        x[:, 1] = (n // 100) % 2
    q = torch.zeros(1, 32)
    q[0, 0], q[0, 1] = 64, 1
    return x, q


@pytest.mark.parametrize("kind", ["ascending", "descending", "constant", "blocks"])
@pytest.mark.parametrize("k", [7, 128])
def test_adversarial_row_orders(kind, k):
    x, q = _ordered_library(kind)
    index = _index(x)
    for slices in (1, None):
        _, r = _exact(index, q, k, f"{kind} k={k} slices={slices}", slices=slices)
        if kind == "ascending":
            assert r[0].tolist() == list(range(4999, 4999 - k, -1))
        if kind in ("descending", "constant"):
            assert r[0].tolist() == list(range(k))
        if kind == "blocks":
            assert r[0].tolist() == [i for i in range(5000) if (i // 100) % 2][:k]


# ---- 3. slices ---------------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_the_slices():
    from coati_amd import _lib
    N, Q, k, E = 70001, 17, 64, 96
    index, q = _index(_ints((N, E), 3)), _ints((Q, E), 4)
    ws, wr, _ = search_util.index_search(index, q, k)
    default = _lib.lib().coati_search_slices(N, Q, k)
    assert 1 <= default <= 30720 // k
    for slices in (1, 2, 7, None, default, 30720 // k):
        s, r = index.search(q, k, slices=slices)
        assert torch.equal(r, wr) and torch.equal(s.double(), ws), slices
        s2, r2 = index.search(q, k, slices=slices)
        assert torch.equal(s, s2) and torch.equal(r, r2), slices
    with pytest.raises(ValueError):
        index.search(q, k, slices=30720 // k + 1)


@pytest.mark.parametrize("kind,rescore", [("exact", None), ("fp8", True), ("fp8", False), ("fp4", True), ("fp4", False), ("pq", True),
                                          ("pq", False)])
def test_flat_query_chunks_give_the_same_result(monkeypatch, kind, rescore):
    """the partial lists of a call stay within a scratch budget (coati_amd.search.sliced_topk, the loop of EmbeddingIndex, Fp8Index,
    Fp4Index and PQIndex): with the budget cut to 7 queries' worth, 40 queries go in six calls and the result is the whole search's,
    bit for bit.  Integer rows: ties abound, so the tie rule is under test."""
    from coati_amd import search as search_mod
    N, dim, Q, k = 1000, 64, 40, 5
    index, q, kw, kk = _index(_ints((N, dim), 4100)), _ints((Q, dim), 4101), {}, k
    if kind != "exact":
        index, kw = getattr(index, kind)(), dict(rescore=rescore)
        kk = k * inspect.signature(index.search).parameters["oversample"].default if rescore else k
    s, r = index.search(q, k, **kw)
    S = index._plan(Q, kk, None)[1]                                                 # what the whole search used
    monkeypatch.setattr(search_mod, "SCRATCH_BYTES", 7 * S * kk * 8)
    index._scratch = None
    s2, r2 = index.search(q, k, slices=S, **kw)
    assert index._scratch[0].numel() == 7 * S * kk
    assert torch.equal(s2, s) and torch.equal(r2, r)


# ---- 4. bias, removal, growth ------------------------------------------------------------------------------------------------
def test_bias_removal_and_growth():
    from coati_amd.search import MIN_CAPACITY
    N, Q, k, E = 900, 17, 7, 64
    x, q = _ints((N, E), 5), _ints((Q, E), 6)
    index = _index(x)
    index.bias.copy_(_ints((N,), 7, -50, 50))                # the view writes through: an integer bias is added exactly
    assert bool((index.bias != 0).any())
    s0, r0 = _exact(index, q, k, "integer bias")
    # removing the best rows of query 0 brings the next ones up
    index.remove(r0[0, :3])
    assert len(index) == N
    s1, r1 = _exact(index, q, k, "3 rows removed")
    assert not set(r0[0, :3].tolist()) & set(r1.flatten().tolist())
    assert r1[0, :k - 3].tolist() == r0[0, 3:].tolist()
    # growth across a capacity doubling keeps the earlier rows' results: the new rows score below every old one
    assert N < MIN_CAPACITY < N + 300
    low = torch.zeros(300, E)
    assert index.add(low) == range(N, N + 300)
    index.bias[N:] = -100000.0
    s2, r2 = _exact(index, q, k, "after growth")
    assert torch.equal(s2, s1) and torch.equal(r2, r1)
    # all but k - 3 rows removed: three pads
    keep = r2[0, :k - 3].tolist()
    index.remove([i for i in range(len(index)) if i not in keep])
    s3, r3 = _exact(index, q, k, "k - 3 rows left")
    assert bool((r3[:, k - 3:] == -1).all() and (s3[:, k - 3:] == NEG_INF).all() and (r3[:, :k - 3] >= 0).all())
    assert r3[0, :k - 3].tolist() == keep


# ---- 5. real-valued data ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [256, 512])
@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
def test_gaussian_data_within_the_accumulation_bound(metric, E):
    """u = 2^-23 (one f32 ulp: rounding of every partial sum, and the matrix core's truncating alignment).  The f32 sum of E exact bf16
    products differs from the exact one by at most b = E u sum|q_i x_i| <= E u |q| |x| in any order; alpha scales it (l2: 2).
    Largest error observed on the MI355X: see DESIGN.md section 6, "Library search"."""
    from coati_amd import search as S
    N, Q, k = 20000, 33, 10
    g = torch.Generator().manual_seed(11 + E)
    index = _index(torch.randn(N, E, generator=g), metric=metric)
    q = torch.randn(Q, E, generator=g)
    s, r = index.search(q, k)
    ws, wr, full = search_util.index_search(index, q, k + 1)
    _, q16 = S.prepare_queries(q, metric, E, DEV)
    b = S.metric_alpha(metric) * E * 2.0 ** -23 * q16.double().norm(dim=1, keepdim=True) * index.vectors.double().norm(dim=1)[None, :]   # [Q, N]
    assert bool((r >= 0).all())
    of_returned, b_returned = full.gather(1, r), b.gather(1, r)
    err = (s.double() - of_returned).abs()
    log(f"search gaussian {metric} E={E}: largest score error {float(err.max()):.3e}, bound b between {float(b.min()):.3e} and {float(b.max()):.3e}; "
        f"{int((r != wr[:, :k]).sum())} of {r.numel()} rows differ from the oracle's order")
    assert bool((err <= b_returned).all())                                                  # every score within b of the oracle's for that row
    assert bool((of_returned >= ws[:, k - 1:k] - 2 * b_returned).all())                     # every returned row belongs (to 2 b)
    clear = full > ws[:, k:k + 1] + 2 * b                                                   # rows that beat the (k + 1)-th by more than 2 b ...
    returned = torch.zeros_like(clear)
    returned.scatter_(1, r, True)
    assert bool((returned | ~clear).all())                                                  # ... are all returned
    assert bool((s[:, 1:] <= s[:, :-1]).all())


# ---- 6. rescore ----------------------------------------------------------------------------------------------------------------
def test_rescore_from_the_f32_copies():
    """Values i / 512 with |i| <= 500 need 10 bits (bf16 keeps 8: the bf16 search ranks them approximately), their products are multiples
    of 2^-18 and a sum of 64 of them is below 2^6: exact in f32 in any order, so the bmm and the test's sum agree to the last bit."""
    N, Q, k, E = 3000, 9, 10, 64
    x, q = _ints((N, E), 21, -500, 500) / 512, _ints((Q, E), 22, -500, 500) / 512
    index = _index(x, keep_f32=True)
    s, r = index.search(q, k, rescore=4)
    _, r16 = index.search(q, 4 * k)
    assert s.shape == r.shape == (Q, k) and bool((r >= 0).all())
    want = (x.to(DEV)[r] * q.to(DEV)[:, None, :]).sum(dim=2)
    assert torch.allclose(s, want, rtol=1e-6, atol=0.0)
    assert all(set(r[i].tolist()) <= set(r16[i].tolist()) for i in range(Q))
    assert bool((s[:, 1:] <= s[:, :-1]).all())
    full = x.to(DEV).double() @ q.to(DEV).double().T                                        # the exact top k, for the record
    hit = sum(len(set(r[i].tolist()) & set(full[:, i].topk(k).indices.tolist())) for i in range(Q))
    log(f"search rescore: {hit} of {Q * k} exact-top-{k} rows found through the bf16 top {4 * k}")
    with pytest.raises(ValueError):
        _index(x).search(q, k, rescore=4)


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------
def _end_to_end(model, tk, tokens, points=None):
    from coati.generative import build_index, nearest_smiles
    strings = _strings(tokens, 40, 5)
    given = strings[:10] + ["CXC", None, "C~C"] + strings[10:]          # no canonical form, not a string, a piece the tokenizer lacks
    with contextlib.redirect_stdout(io.StringIO()):
        index, kept = build_index(given, model, tk, batch_size=16, canon_smiles=_canon)
        near = nearest_smiles(kept + ["CXC"], index, kept, model, tk, k=3, canon_smiles=_canon)
    assert kept == strings and len(index) == 40                         # the three unusable ones are skipped, row i is kept[i]
    assert near[-1] == [] and len(near) == len(kept) + 1
    # the stored row and the query are the same bf16 rounding x (1 + d), |d| <= 2^-8, of one unit vector: score = |x (1 + d)|^2 within
    # (1 +- 2^-8)^2 of 1, i.e. 2 * 2^-8 + 2^-16 < 1e-2 (the f32 accumulation's E * 2^-23 is far below it)
    worst = 0.0
    for s, hits in zip(kept, near):
        assert len(hits) == 3 and hits[0][0] == s, (s, hits)
        assert [v for _, v in hits] == sorted((v for _, v in hits), reverse=True)
        worst = max(worst, abs(hits[0][1] - 1.0))
    log(f"search end to end: {len(kept)} of {len(given)} strings kept, self score within {worst:.2e} of 1")
    assert worst <= 1e-2
    if points is not None:
        h = model.encode_points(*points)
        from_points = nearest_smiles(h, index, kept, model, tk, k=5)
        assert len(from_points) == h.shape[0] and all(len(hits) == 5 and all(s in kept for s, _ in hits) for hits in from_points)


def test_end_to_end_coati1(golden_dir):
    from coati_amd.models.encoding.clip_e2e import e3gnn_smiles_clip_e2e
    from coati_amd.models.encoding.tokenizers import TrieTokenizer
    g = np.load(os.path.join(golden_dir, "generative_golden.npz"))
    voc = json.load(open(os.path.join(golden_dir, "tokenizer.json")))
    tk = TrieTokenizer(n_seq=int(g["n_seq"]), smiles_tokens=voc["smiles"], special_tokens=voc["special"])
    with contextlib.redirect_stdout(io.StringIO()):
        model = e3gnn_smiles_clip_e2e(**SMALL, device=torch.device(DEV))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "small_model_after3.npz")).items()}, strict=False)
    pts = np.load(os.path.join(golden_dir, "generation_golden.npz"))
    points = (torch.from_numpy(pts["points.atoms"]).to(DEV), torch.from_numpy(pts["points.coords"]).to(DEV))
    _end_to_end(model, tk, [t for t in voc["smiles"] if t.isascii() and "X" not in t], points)


def test_end_to_end_coati2(golden_dir):
    from coati_amd.models.simple_coati2.transformer_only import COATI_Smiles_Inference
    from coati_amd.models.simple_coati2.trie_tokenizer import TrieTokenizer
    with open(os.path.join(golden_dir, "coati2_vocab.json")) as f:
        voc = json.load(f)
    tk = TrieTokenizer(n_seq=voc["n_seq"], special_tokens=voc["special_tokens"], smiles_tokens=voc["smiles_tokens"])
    with contextlib.redirect_stdout(io.StringIO()):
        model = COATI_Smiles_Inference(n_layer_xformer=2, n_hidden_xformer=64, embed_dim=64, n_head=4, n_seq=voc["n_seq"],
                                       enc_to_coati="swiglu_resnet", n_tok=voc["ids"]["n_token"], device=DEV)
    _end_to_end(model, tk, voc["smiles_tokens"])


# ---- 8. streams and inputs -----------------------------------------------------------------------------------------------------
def test_streams_and_query_layouts():
    N, Q, k, E = 3000, 19, 7, 40                             # dim 40 is stored as 64 columns
    x, q = _ints((N, E), 31), _ints((Q, E), 32)
    index = _index(x)
    assert index.vectors.shape == (N, 64) and bool((index.vectors[:, E:] == 0).all())
    s, r = _exact(index, q, k, "dim 40")
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s1, r1 = index.search(q.to(DEV), k)
    side.synchronize()
    assert torch.equal(s1, s) and torch.equal(r1, r)
    wide = torch.zeros(Q, 2 * E, dtype=torch.float64)
    wide[:, ::2] = q.double()
    for other in (wide[:, ::2], q.T.contiguous().T, q.to(DEV).to(torch.float16)):
        assert other.shape == (Q, E)
        s2, r2 = index.search(other, k)
        assert torch.equal(s2, s) and torch.equal(r2, r)
    s3, r3 = index.search(q[0], k)                           # one vector is one query
    assert torch.equal(s3, s[:1]) and torch.equal(r3, r[:1])


def test_save_and_load(tmp_path):
    x, q = _ints((500, 96), 41), _ints((5, 96), 42)
    index = _index(x, metric="l2", keep_f32=True)
    index.remove([3, 4])
    index.save(str(tmp_path / "index.pt"))
    from coati_amd.search import EmbeddingIndex
    again = EmbeddingIndex.load(str(tmp_path / "index.pt"), device=DEV)
    assert len(again) == 500 and again.metric == "l2" and again.keep_f32
    assert torch.equal(again.vectors, index.vectors) and torch.equal(again.bias, index.bias)
    a, b = index.search(q, 9), again.search(q, 9)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _exact(again, q, 9, "l2 after load")
