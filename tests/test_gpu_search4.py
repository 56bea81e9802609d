"""Four-bit search on the GPU (include/coati_search4.h, coati_amd/fp4_index.py): the quantiser byte for byte against its plain-torch
restatement, stage 1 on data that e2m1 with block scales holds exactly against the bf16 oracle of tests/search_util.py (which is also
the check of the scaled MFMA's operand and scale maps: the data is asymmetric in rows, columns and blocks), stage 1 on real-valued
data against the f32 accumulation bound, and the two stages against EmbeddingIndex.search bit for bit."""
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
from tests import search4_util as U, search8_util as U8, search_util  # noqa: E402
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
    log(f"search4 {label}: {bad_r} rows and {bad_s} scores of {r.numel()} differ from the oracle")
    assert bad_r == 0 and bad_s == 0, label


# ---- 1. the quantiser, byte for byte ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [32, 96, 128, 256, 480, 512])
@pytest.mark.parametrize("N", [1, 17, 1000])
def test_quantiser_equals_the_torch_restatement(N, E):
    from coati_amd import fp4_index as F
    x = U.quantiser_rows(N, E, 100 * N + E)
    E4 = 128 * ((E + 127) // 128)
    want_c, want_s = F.quantise_rows(x)                                           # on the CPU
    c, s = F.quantise_device(x.to(DEV))
    assert c.dtype == torch.uint8 and c.shape == (N, E4 // 2) and s.dtype == torch.uint8 and s.shape == (N, E4 // 32)
    bad_c, bad_s = int((c.cpu() != want_c).sum()), int((s.cpu() != want_s).sum())
    log(f"search4 quantiser N={N} E={E}: {bad_c} of {c.numel()} code bytes and {bad_s} of {s.numel()} scale bytes differ")
    assert bad_c == 0 and bad_s == 0
    assert bool((c[:, E // 2:] == 0).all()) and bool((s[:, E // 32:] == 127).all())                      # the pad


# ---- 2. integer data: stage 1 alone equals the bf16 oracle ------------------------------------------------------------------------------
EXACT = [(1, 1, 1, 32), (15, 15, 7, 96), (16, 16, 64, 128), (17, 17, 7, 512), (63, 64, 64, 32), (64, 65, 128, 96), (65, 130, 1, 256),
         (1000, 17, 128, 384), (1000, 130, 64, 256), (70001, 16, 7, 128), (70001, 65, 128, 512)]


@pytest.mark.parametrize("N,Q,k,E", EXACT)
def test_integer_data_equals_the_bf16_oracle(N, Q, k, E):
    index = _index(_ints((N, E), 1000 + N + E))
    fp4 = index.fp4()
    E4 = 128 * ((E + 127) // 128)
    assert len(fp4) == N and fp4.codes.shape == (N, E4 // 2) and fp4.scales.shape == (N, E4 // 32) and fp4.codes.dtype == torch.uint8
    q = _ints((Q, E), 7 * Q + k)
    ws, wr, _ = search_util.index_search(index, q, k)
    s, r = fp4.search(q, k, rescore=False)
    _equals((s, r), (ws, wr), f"stage 1 N={N} Q={Q} k={k} E={E}")
    if k > N:
        assert bool((r[:, N:] == -1).all() and (s[:, N:] == NEG_INF).all() and (r[:, :N] >= 0).all())


# ---- 3. block scales ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["dot", "l2"])
@pytest.mark.parametrize("N,Q,k,E", [(1000, 17, 128, 96), (3000, 33, 64, 256), (70001, 65, 7, 512)])
def test_block_scales_equal_the_bf16_oracle(N, Q, k, E, metric):
    """every (row, block) has its own power of two: a scale applied to the wrong block changes a score by a power of two"""
    x = U.scaled_ints((N, E), 50 + N)
    q = _ints((Q, E), 52 + Q, -15, 15)
    q[::2] = _ints((q[::2].shape[0], E), 53, -2, 2)
    index = _index(x, metric=metric)
    fp4 = index.fp4(keep_rows=False)
    live = fp4.scales[:, :E // 32]
    assert int(live.unique().numel()) >= 4 and bool((live.amax(dim=1) > live.amin(dim=1)).any())
    assert torch.equal(fp4.dequantised()[:, :E].cpu(), x)
    ws, wr, _ = search_util.index_search(index, q, k)
    _equals(fp4.search(q, k), (ws, wr), f"stage 1 block scales {metric} N={N} Q={Q} k={k} E={E}")


# ---- 4. adversarial orders ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ascending", "descending", "constant", "blocks"])
@pytest.mark.parametrize("k", [7, 128])
def test_adversarial_row_orders(kind, k):
    x, q = U.quat_library(kind)
    index = _index(x)
    fp4 = index.fp4()
    for slices in (1, None):
        ws, wr, _ = search_util.index_search(index, q, k)
        s, r = fp4.search(q, k, rescore=False, slices=slices)
        _equals((s, r), (ws, wr), f"{kind} k={k} slices={slices}")
        if kind == "ascending":
            assert r[0].tolist() == list(range(4095, 4095 - k, -1)) and s[0].tolist() == [float(v) for v in range(4095, 4095 - k, -1)]
        if kind in ("descending", "constant"):
            assert r[0].tolist() == list(range(k))
        if kind == "blocks":
            assert r[0].tolist() == [i for i in range(4096) if (i // 100) % 2][:k]


# ---- 5. slices ---------------------------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_the_slices():
    from coati_amd import _lib
    N, Q, k, E = 70001, 17, 64, 96
    index, q = _index(_ints((N, E), 3)), _ints((Q, E), 4)
    fp4 = index.fp4()
    ws, wr, _ = search_util.index_search(index, q, k)
    default = _lib.lib().coati_search4_slices(N, Q, k)
    assert 1 <= default <= 30720 // k
    for slices in (1, 2, 7, None, default, 30720 // k):
        s, r = fp4.search(q, k, rescore=False, slices=slices)
        assert torch.equal(r.cpu(), wr.cpu()) and torch.equal(s.double().cpu(), ws.cpu()), slices
        s2, r2 = fp4.search(q, k, rescore=False, slices=slices)
        assert torch.equal(s, s2) and torch.equal(r, r2), slices
    with pytest.raises(ValueError):
        fp4.search(q, k, rescore=False, slices=30720 // k + 1)


# ---- 6. bias and removal -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescore", [False, True])
def test_bias_and_removal(rescore):
    N, Q, k, E = 900, 17, 7, 64
    x, q = _ints((N, E), 5), _ints((Q, E), 6)
    index = _index(x)
    index.bias.copy_(_ints((N,), 7, -50, 50))                # the snapshot takes the index's bias: an integer bias is added exactly
    fp4 = index.fp4()
    s0, r0 = fp4.search(q, k, rescore=rescore)
    ws, wr, _ = search_util.index_search(index, q, k)
    _equals((s0, r0), (ws, wr), f"integer bias rescore={rescore}")
    # bias= is added in both stages
    extra = _ints((N,), 8, -30, 30).to(DEV)
    index.bias.add_(extra)
    ws, wr, _ = search_util.index_search(index, q, k)
    _equals(fp4.search(q, k, rescore=rescore, bias=extra), (ws, wr), f"bias= rescore={rescore}")
    index.bias.sub_(extra)
    # removing the best rows of query 0 brings the next ones up
    fp4.remove(r0[0, :3])
    index.remove(r0[0, :3])
    assert len(fp4) == N
    s1, r1 = fp4.search(q, k, rescore=rescore)
    ws, wr, _ = search_util.index_search(index, q, k)
    _equals((s1, r1), (ws, wr), f"3 rows removed rescore={rescore}")
    assert not set(r0[0, :3].tolist()) & set(r1.flatten().tolist())
    assert r1[0, :k - 3].tolist() == r0[0, 3:].tolist()
    # all but k - 3 rows removed: three pads
    keep = r1[0, :k - 3].tolist()
    gone = [i for i in range(N) if i not in keep]
    fp4.remove(gone)
    index.remove(gone)
    s3, r3 = fp4.search(q, k, rescore=rescore)
    ws, wr, _ = search_util.index_search(index, q, k)
    _equals((s3, r3), (ws, wr), f"k - 3 rows left rescore={rescore}")
    assert bool((r3[:, k - 3:] == -1).all() and (s3[:, k - 3:] == NEG_INF).all() and (r3[:, :k - 3] >= 0).all())
    assert r3[0, :k - 3].tolist() == keep


# ---- 7. real-valued data, stage 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [256, 512])
@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
def test_gaussian_data_within_the_accumulation_bound(metric, E):
    """The oracle is the float64 score of the DEQUANTISED operands.  An e4m3 value times an e2m1 value times a power of two is exact in
    f32, and so is the power-of-two factor, so the error is the accumulation's alone: with u = 2^-23 the f32 sum of E exact terms
    differs from the exact one by at most b = E u sum|q_i x_i| <= E u |q_hat| |x_hat| in any order, under round-to-nearest or
    truncation at f32 precision; alpha scales it (l2: 2).  Largest error observed on the MI355X: see DESIGN.md section 6, "Four-bit
    search"."""
    from coati_amd import search as S
    N, Q, k = 20000, 33, 10
    g = torch.Generator().manual_seed(11 + E)
    index = _index(torch.randn(N, E, generator=g), metric=metric)
    q = torch.randn(Q, E, generator=g)
    fp4 = index.fp4(keep_rows=False)
    s, r = fp4.search(q, k)
    s, r = s.cpu(), r.cpu()
    full, q_hat = U.stage1_scores(fp4, q)
    ws, wr = search_util.topk(full, k + 1)
    b = S.metric_alpha(metric) * E * 2.0 ** -23 * q_hat.double().norm(dim=1, keepdim=True) * fp4.dequantised().cpu().double().norm(dim=1)[None, :]
    assert bool((r >= 0).all())
    of_returned, b_returned = full.gather(1, r), b.gather(1, r)
    err = (s.double() - of_returned).abs()
    log(f"search4 gaussian {metric} E={E}: largest stage-1 score error {float(err.max()):.3e}, largest err / b {float((err / b_returned).max()):.4f}, "
        f"bound b between {float(b.min()):.3e} and {float(b.max()):.3e}; {int((r != wr[:, :k]).sum())} of {r.numel()} rows differ from the "
        f"oracle's order")
    assert bool((err <= b_returned).all())                                                  # every score within b of the oracle's for that row
    assert bool((of_returned >= ws[:, k - 1:k] - 2 * b_returned).all())                     # every returned row belongs (to 2 b)
    clear = full > ws[:, k:k + 1] + 2 * b                                                   # rows that beat the (k + 1)-th by more than 2 b ...
    returned = torch.zeros_like(clear)
    returned.scatter_(1, r, True)
    assert bool((returned | ~clear).all())                                                  # ... are all returned
    assert bool((s[:, 1:] <= s[:, :-1]).all())


# ---- 8. two stages equal the exact search ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [256, 512])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
@pytest.mark.parametrize("data", ["gaussian", "clustered"])
def test_two_stages_equal_the_exact_search(data, metric, E):
    """R = 12 * 10 = 120 candidates.  Asserted first, from the float64 emulation of stage 1: every row of the exact top 10 has stage-1
    rank below 88, which leaves 32 ranks of slack against f32 rounding in stage 1 (errors of E * 2^-23 relative, against rank gaps of
    tens).  With these seeds the largest emulated ranks are 40, 37, 59, 66 (gaussian: cosine 256 / 512, l2 256 / 512) and 72, 54, 54, 35
    (clustered).  Then the two-stage result must be the exact search's, rows and score BITS."""
    N, Q, k, over = 20000, 33, 10, 12
    if data == "gaussian":
        g = torch.Generator().manual_seed(23 + E)
        x, q = torch.randn(N, E, generator=g), torch.randn(Q, E, generator=g)
    else:
        draw = U8.clustered(N, E, 29 + E)
        x, q = draw(N), draw(Q)
    index = _index(x, metric=metric)
    fp4 = index.fp4()
    ws, wr = index.search(q, k)
    full, _ = U.stage1_scores(fp4, q)
    rank = U.stage1_ranks(full, wr.cpu())
    log(f"search4 two stages {data} {metric} E={E}: the exact top {k} have emulated stage-1 ranks up to {int(rank.max())} (R = {over * k})")
    assert int(rank.max()) < 88
    s, r = fp4.search(q, k, oversample=over)
    assert torch.equal(r, wr) and torch.equal(s.view(torch.int32), ws.view(torch.int32))


# ---- 9. flags and persistence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_rows", [True, False])
def test_flags_and_persistence(tmp_path, keep_rows):
    from coati_amd.fp4_index import Fp4Index
    N, Q, k, E = 3000, 19, 10, 96
    g = torch.Generator().manual_seed(77)
    index = _index(torch.randn(N, E, generator=g), metric="cosine")
    q = torch.randn(Q, E, generator=g)
    fp4 = index.fp4(keep_rows=keep_rows)
    assert fp4.keep_rows == keep_rows and fp4.bytes_per_row() == 128 // 2 + 128 // 32 + 4
    if not keep_rows:
        with pytest.raises(ValueError, match="keep_rows"):
            fp4.search(q, k, rescore=True)
    # rescore=False is stage 1's k best: the float64 oracle's rows wherever its scores are further apart than the f32 sums can err
    s1, r1 = fp4.search(q, k, rescore=False)
    full, q_hat = U.stage1_scores(fp4, q)
    ws, wr = search_util.topk(full, k + 1)
    b = 128 * 2.0 ** -23 * q_hat.double().norm(dim=1, keepdim=True) * fp4.dequantised().cpu().double().norm(dim=1)[None, :]   # test 7's bound at E4 = 128
    gap = float((ws[:, :-1] - ws[:, 1:]).min())
    err = (s1.double().cpu() - full.gather(1, r1.cpu())).abs()
    log(f"search4 flags keep_rows={keep_rows}: stage-1 score error {float(err.max()):.3e}, bound up to {float(b.max()):.3e}, smallest gap among "
        f"the oracle's first {k + 1} scores {gap:.3e}")
    assert bool((err <= b.gather(1, r1.cpu())).all()) and (gap <= 2 * float(b.max()) or torch.equal(r1.cpu(), wr[:, :k]))
    if not keep_rows:
        sd, rd = fp4.search(q, k)                                                  # the default is stage 1 alone without the rows
        assert torch.equal(sd, s1) and torch.equal(rd, r1)
    fp4.remove(r1[0, :2])
    path = str(tmp_path / "fp4.pt")
    fp4.save(path)
    again = Fp4Index.load(path, device=DEV)
    assert again.keep_rows == keep_rows and len(again) == N and again.metric == "cosine" and again.dim == E
    assert torch.equal(again.codes, fp4.codes) and torch.equal(again.scales, fp4.scales) and torch.equal(again.bias, fp4.bias)
    a, b = fp4.search(q, k), again.search(q, k)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not set(r1[0, :2].tolist()) & set(b[1].flatten().tolist())
    a, b = fp4.search(q, k, rescore=False), again.search(q, k, rescore=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 10. from strings ---------------------------------------------------------------------------------------------------------------------
def test_from_strings(golden_dir):
    from coati.generative import build_fp4_index, build_index, nearest_smiles
    from coati_amd.fp4_index import Fp4Index
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
        index, kept = build_fp4_index(given, model, tk, batch_size=16, canon_smiles=_canon)
        exact, _ = build_index(given, model, tk, batch_size=16, canon_smiles=_canon)
        # k = 5 at the default oversample of 8: R = 40 candidates, the whole library, so the answer must be the exact index's
        near = nearest_smiles(kept + ["CXC"], index, kept, model, tk, k=5, canon_smiles=_canon)
        want = nearest_smiles(kept + ["CXC"], exact, kept, model, tk, k=5, canon_smiles=_canon)
    assert isinstance(index, Fp4Index) and index.keep_rows and kept == strings and len(index) == 40 and index.dim_stored == 128
    assert near[-1] == [] and len(near) == len(kept) + 1
    for s, hits in zip(kept, near):
        assert len(hits) == 5 and hits[0][0] == s, (s, hits)                   # every query string finds itself first
        assert abs(hits[0][1] - 1.0) <= 1e-2                                   # the exact score of the bf16 rows, as in test_gpu_search.py
    assert near == want
