"""Quantised search on the GPU (include/coati_search8.h, coati_amd/fp8_index.py): the quantiser byte for byte against its plain-torch
restatement, stage 1 on data that e4m3 holds exactly against the bf16 oracle of tests/search_util.py (which is also the check of the fp8
MFMA's operand map: the data is asymmetric in rows and columns), stage 1 on real-valued data against the f32 accumulation bound, and
the two stages against EmbeddingIndex.search bit for bit."""
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
from tests import search8_util as U, search_util  # noqa: E402
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


def _equals(got, want, label):
    """(scores, rows) == the oracle's, element for element"""
    (s, r), (ws, wr) = got, want
    assert s.dtype == torch.float32 and r.dtype == torch.int64 and s.shape == r.shape == wr.shape
    bad_r, bad_s = int((r.cpu() != wr.cpu()).sum()), int((s.double().cpu() != ws.double().cpu()).sum())
    log(f"search8 {label}: {bad_r} rows and {bad_s} scores of {r.numel()} differ from the oracle")
    assert bad_r == 0 and bad_s == 0, label


# ---- 1. the quantiser, byte for byte ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [32, 96, 256, 512])
@pytest.mark.parametrize("N", [1, 17, 1000])
def test_quantiser_equals_the_torch_restatement(N, E):
    from coati_amd import fp8_index as F
    x = U.quantiser_rows(N, E, 100 * N + E)
    want_b, want_s = F.quantise_rows(x)                                           # on the CPU
    b, s = F.quantise_device(x.to(DEV))
    assert b.dtype == torch.uint8 and b.shape == (N, E) and s.dtype == torch.float32 and s.shape == (N,)
    bad_b, bad_s = int((b.cpu() != want_b).sum()), int((s.cpu() != want_s).sum())
    log(f"search8 quantiser N={N} E={E}: {bad_b} of {b.numel()} bytes and {bad_s} of {N} scales differ")
    assert bad_b == 0 and bad_s == 0


# ---- 2. integer data: stage 1 alone equals the bf16 oracle ------------------------------------------------------------------------------
EXACT = [(1, 1, 1, 32), (15, 15, 7, 96), (16, 16, 64, 256), (17, 17, 7, 512), (63, 64, 64, 32), (64, 65, 128, 96), (65, 130, 1, 256),
         (1000, 17, 128, 512), (1000, 130, 64, 256), (70001, 16, 7, 256), (70001, 65, 128, 512)]


@pytest.mark.parametrize("N,Q,k,E", EXACT)
def test_integer_data_equals_the_bf16_oracle(N, Q, k, E):
    index = _index(_ints((N, E), 1000 + N + E))
    fp8 = index.fp8()
    assert len(fp8) == N and fp8.vectors8.shape == (N, E) and fp8.vectors8.dtype == torch.uint8
    q = _ints((Q, E), 7 * Q + k)
    ws, wr, _ = search_util.index_search(index, q, k)
    s, r = fp8.search(q, k, rescore=False)
    _equals((s, r), (ws, wr), f"stage 1 N={N} Q={Q} k={k} E={E}")
    if k > N:
        assert bool((r[:, N:] == -1).all() and (s[:, N:] == NEG_INF).all() and (r[:, :N] >= 0).all())


@pytest.mark.parametrize("metric", ["dot", "l2"])
@pytest.mark.parametrize("N,Q,k,E", [(1000, 17, 128, 96), (70001, 65, 7, 512), (3000, 33, 64, 256)])
def test_four_bit_integers_and_mixed_scales_equal_the_bf16_oracle(N, Q, k, E, metric):
    """magnitudes up to 15 use all of e4m3's significand; every third row is scaled down so that the rows' scales differ"""
    x = _ints((N, E), 50 + N, -15, 15)
    x[::3] = _ints((x[::3].shape[0], E), 51 + N, -3, 3)
    x[1::7] *= 0.125
    q = _ints((Q, E), 52 + Q, -15, 15)
    q[::2] = _ints((q[::2].shape[0], E), 53, -2, 2)
    index = _index(x, metric=metric)
    fp8 = index.fp8(keep_rows=False)
    assert int(fp8.scales.unique().numel()) >= 3
    ws, wr, _ = search_util.index_search(index, q, k)
    _equals(fp8.search(q, k), (ws, wr), f"stage 1 four bits {metric} N={N} Q={Q} k={k} E={E}")


# ---- 3. adversarial orders ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ascending", "descending", "constant", "blocks"])
@pytest.mark.parametrize("k", [7, 128])
def test_adversarial_row_orders(kind, k):
    x, q = U.hex_library(kind)
    index = _index(x)
    fp8 = index.fp8()
    if kind in ("ascending", "descending"):                  # the rows' largest digits differ, and so do their scales
        assert sorted(set(fp8.scales.tolist())) == [2.0 ** -8, 2.0 ** -7, 2.0 ** -6, 2.0 ** -5, 2.0 ** -4, 1.0]
    for slices in (1, None):
        ws, wr, _ = search_util.index_search(index, q, k)
        s, r = fp8.search(q, k, rescore=False, slices=slices)
        _equals((s, r), (ws, wr), f"{kind} k={k} slices={slices}")
        if kind == "ascending":
            assert r[0].tolist() == list(range(4095, 4095 - k, -1)) and s[0].tolist() == [float(v) for v in range(4095, 4095 - k, -1)]
        if kind in ("descending", "constant"):
            assert r[0].tolist() == list(range(k))
        if kind == "blocks":
            assert r[0].tolist() == [i for i in range(4096) if (i // 100) % 2][:k]


# ---- 4. slices ---------------------------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_the_slices():
    from coati_amd import _lib
    N, Q, k, E = 70001, 17, 64, 96
    index, q = _index(_ints((N, E), 3)), _ints((Q, E), 4)
    fp8 = index.fp8()
    ws, wr, _ = search_util.index_search(index, q, k)
    default = _lib.lib().coati_search8_slices(N, Q, k)
    assert 1 <= default <= 30720 // k
    for slices in (1, 2, 7, None, default, 30720 // k):
        s, r = fp8.search(q, k, rescore=False, slices=slices)
        assert torch.equal(r.cpu(), wr.cpu()) and torch.equal(s.double().cpu(), ws.cpu()), slices
        s2, r2 = fp8.search(q, k, rescore=False, slices=slices)
        assert torch.equal(s, s2) and torch.equal(r, r2), slices
    with pytest.raises(ValueError):
        fp8.search(q, k, rescore=False, slices=30720 // k + 1)


# ---- 5. bias and removal -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescore", [False, True])
def test_bias_and_removal(rescore):
    N, Q, k, E = 900, 17, 7, 64
    x, q = _ints((N, E), 5), _ints((Q, E), 6)
    index = _index(x)
    index.bias.copy_(_ints((N,), 7, -50, 50))                # the snapshot takes the index's bias: an integer bias is added exactly
    fp8 = index.fp8()
    s0, r0 = fp8.search(q, k, rescore=rescore)
    ws, wr, _ = search_util.index_search(index, q, k)
    _equals((s0, r0), (ws, wr), f"integer bias rescore={rescore}")
    # bias= is added in both stages
    extra = _ints((N,), 8, -30, 30).to(DEV)
    index.bias.add_(extra)
    ws, wr, _ = search_util.index_search(index, q, k)
    _equals(fp8.search(q, k, rescore=rescore, bias=extra), (ws, wr), f"bias= rescore={rescore}")
    index.bias.sub_(extra)
    # removing the best rows of query 0 brings the next ones up
    fp8.remove(r0[0, :3])
    index.remove(r0[0, :3])
    assert len(fp8) == N
    s1, r1 = fp8.search(q, k, rescore=rescore)
    ws, wr, _ = search_util.index_search(index, q, k)
    _equals((s1, r1), (ws, wr), f"3 rows removed rescore={rescore}")
    assert not set(r0[0, :3].tolist()) & set(r1.flatten().tolist())
    assert r1[0, :k - 3].tolist() == r0[0, 3:].tolist()
    # all but k - 3 rows removed: three pads
    keep = r1[0, :k - 3].tolist()
    gone = [i for i in range(N) if i not in keep]
    fp8.remove(gone)
    index.remove(gone)
    s3, r3 = fp8.search(q, k, rescore=rescore)
    ws, wr, _ = search_util.index_search(index, q, k)
    _equals((s3, r3), (ws, wr), f"k - 3 rows left rescore={rescore}")
    assert bool((r3[:, k - 3:] == -1).all() and (s3[:, k - 3:] == NEG_INF).all() and (r3[:, :k - 3] >= 0).all())
    assert r3[0, :k - 3].tolist() == keep


# ---- 6. real-valued data, stage 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [256, 512])
@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
def test_gaussian_data_within_the_accumulation_bound(metric, E):
    """The oracle is the float64 score of the DEQUANTISED operands.  A product of two e4m3 values (4-bit significands) is exact in f32,
    and so is the power-of-two factor, so the error is the accumulation's alone: with u = 2^-23 the f32 sum of E exact products differs
    from the exact one by at most b = E u sum|q_i x_i| <= E u |q_hat| |x_hat| in any order; alpha scales it (l2: 2).
    Largest error observed on the MI355X: see DESIGN.md section 6, "Quantised search"."""
    from coati_amd import search as S
    N, Q, k = 20000, 33, 10
    g = torch.Generator().manual_seed(11 + E)
    index = _index(torch.randn(N, E, generator=g), metric=metric)
    q = torch.randn(Q, E, generator=g)
    fp8 = index.fp8(keep_rows=False)
    s, r = fp8.search(q, k)
    s, r = s.cpu(), r.cpu()
    full, q_hat = U.stage1_scores(fp8, q)
    ws, wr = search_util.topk(full, k + 1)
    b = S.metric_alpha(metric) * E * 2.0 ** -23 * q_hat.double().norm(dim=1, keepdim=True) * fp8.dequantised().cpu().double().norm(dim=1)[None, :]
    assert bool((r >= 0).all())
    of_returned, b_returned = full.gather(1, r), b.gather(1, r)
    err = (s.double() - of_returned).abs()
    log(f"search8 gaussian {metric} E={E}: largest stage-1 score error {float(err.max()):.3e}, bound b between {float(b.min()):.3e} and "
        f"{float(b.max()):.3e}; {int((r != wr[:, :k]).sum())} of {r.numel()} rows differ from the oracle's order")
    assert bool((err <= b_returned).all())                                                  # every score within b of the oracle's for that row
    assert bool((of_returned >= ws[:, k - 1:k] - 2 * b_returned).all())                     # every returned row belongs (to 2 b)
    clear = full > ws[:, k:k + 1] + 2 * b                                                   # rows that beat the (k + 1)-th by more than 2 b ...
    returned = torch.zeros_like(clear)
    returned.scatter_(1, r, True)
    assert bool((returned | ~clear).all())                                                  # ... are all returned
    assert bool((s[:, 1:] <= s[:, :-1]).all())


# ---- 7. two stages equal the exact search ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [256, 512])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
@pytest.mark.parametrize("data", ["gaussian", "clustered"])
def test_two_stages_equal_the_exact_search(data, metric, E):
    """R = 8 * 10 = 80 candidates.  Asserted first, from the float64 emulation of stage 1: every row of the exact top 10 has stage-1 rank
    below R / 2 = 40, so f32 rounding in stage 1 (errors of E * 2^-23 relative, against rank gaps of tens) cannot push one out of the
    80.  Then the two-stage result must be the exact search's, rows and score BITS."""
    N, Q, k, over = 20000, 33, 10, 8
    if data == "gaussian":
        g = torch.Generator().manual_seed(23 + E)
        x, q = torch.randn(N, E, generator=g), torch.randn(Q, E, generator=g)
    else:
        draw = U.clustered(N, E, 29 + E)
        x, q = draw(N), draw(Q)
    index = _index(x, metric=metric)
    fp8 = index.fp8()
    ws, wr = index.search(q, k)
    full, _ = U.stage1_scores(fp8, q)
    mine = full.gather(1, wr.cpu())                                                         # [Q, k]: stage 1's score of the exact top k
    above = (full[:, None, :] > mine[:, :, None]).sum(dim=2)
    ties_before = ((full[:, None, :] == mine[:, :, None]) & (torch.arange(N)[None, None, :] < wr.cpu()[:, :, None])).sum(dim=2)
    rank = above + ties_before
    log(f"search8 two stages {data} {metric} E={E}: the exact top {k} have emulated stage-1 ranks up to {int(rank.max())} (R = {over * k})")
    assert int(rank.max()) < over * k // 2
    s, r = fp8.search(q, k, oversample=over)
    assert torch.equal(r, wr) and torch.equal(s.view(torch.int32), ws.view(torch.int32))


# ---- 8. the rescoring kernel alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 16, 17, 128])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_rescore_kernel_alone(R, metric):
    """candidates = what index.search(q, 128) returned, the best R of them, shuffled per query, the two worst replaced by -1; three of
    query 0's best rows are removed afterwards.  The then-current exact top k lies within the first k + 3 of the old order, all of
    them still candidates: the kernel's result must be index.search's, bit for bit."""
    from coati_amd import fp8_index as F, search as S
    N, Q, E = 3000, 19, 96
    k = 1 if R == 1 else 7
    g = torch.Generator().manual_seed(40 + R)
    index = _index(torch.randn(N, E, generator=g), metric=metric)
    q = torch.randn(Q, E, generator=g)
    _, top = index.search(q, 128)
    cand = top[:, :R].clone()
    if R > 1:
        cand[:, R - 2:] = -1
        index.remove(top[0, :3])
        perm = torch.stack([torch.randperm(R, generator=g) for _ in range(Q)]).to(DEV)
        cand = cand.gather(1, perm)
    ws, wr = index.search(q, k)
    _, q16 = S.prepare_queries(q, metric, E, DEV)
    s, r = F.rescore_candidates(index.vectors, index.bias, q16, cand, k, S.metric_alpha(metric))
    s = S.finish_scores(s, metric, q16)
    assert torch.equal(r, wr) and torch.equal(s.view(torch.int32), ws.view(torch.int32))
    # no candidate at all: padding
    s, r = F.rescore_candidates(index.vectors, index.bias, q16, torch.full((Q, R), -1, dtype=torch.int64, device=DEV), k)
    assert bool((r == -1).all() and (s == NEG_INF).all())


@pytest.mark.parametrize("N,Q,k,E,R", [(15, 15, 7, 96, 15), (1000, 17, 128, 512, 128), (1000, 130, 64, 256, 100), (70001, 65, 16, 32, 17)])
def test_rescore_kernel_on_integer_data_equals_the_oracle(N, Q, k, E, R):
    """every row a candidate of every query where N allows, else the oracle's best R in reverse order: ties abound, and the order must be
    (score descending, row ascending) whatever the candidates' order"""
    from coati_amd import fp8_index as F, search as S
    index = _index(_ints((N, E), 60 + N))
    q = _ints((Q, E), 61 + Q)
    ws, wr, _ = search_util.index_search(index, q, k)
    _, wide, _ = search_util.index_search(index, q, R)
    cand = wide.flip(1).contiguous().to(DEV)
    _, q16 = S.prepare_queries(q, "dot", E, DEV)
    _equals(F.rescore_candidates(index.vectors, index.bias, q16, cand, k), (ws, wr), f"rescore integers N={N} Q={Q} k={k} E={E} R={R}")


# ---- 9. from strings ----------------------------------------------------------------------------------------------------------------------
def test_from_strings(golden_dir):
    from coati.generative import build_index, nearest_smiles
    from coati_amd.fp8_index import Fp8Index
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
        index, kept = build_index(given, model, tk, batch_size=16, canon_smiles=_canon, fp8=True)
        exact, _ = build_index(given, model, tk, batch_size=16, canon_smiles=_canon)
        near = nearest_smiles(kept + ["CXC"], index, kept, model, tk, k=3, canon_smiles=_canon)
        want = nearest_smiles(kept + ["CXC"], exact, kept, model, tk, k=3, canon_smiles=_canon)
    assert isinstance(index, Fp8Index) and index.keep_rows and kept == strings and len(index) == 40
    assert near[-1] == [] and len(near) == len(kept) + 1
    for s, hits in zip(kept, near):
        assert len(hits) == 3 and hits[0][0] == s, (s, hits)                   # every query string finds itself first
        assert [v for _, v in hits] == sorted((v for _, v in hits), reverse=True)
        assert abs(hits[0][1] - 1.0) <= 1e-2                                   # the exact score of the bf16 rows, as in test_gpu_search.py
    agree = sum(a == b for a, b in zip(near, want))
    log(f"search8 from strings: {agree} of {len(near)} answers are the exact index's")
