"""Product-quantised search, host side (no GPU): include/coati_pq.h parses against coati_hip.h to exactly its four entries and the
library exports them, the entries refuse bad arguments before any device call, the plain-torch encoder keeps the storage rule, the code
books are reproducible, a lossless library is searched exactly, PQIndex adds, removes, saves and loads on the CPU and does not search
there, and trained code books reach the recall written down here."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import pq_util as U, search_util  # noqa: E402
from tests.search_util import ints as _ints  # noqa: E402

NAMES = ["coati_pq_encode", "coati_pq_k_max", "coati_pq_slices", "coati_pq_topk"]
NEG_INF = float("-inf")


# ---- 1. the seventeenth header -------------------------------------------------------------------------------------------------------
def test_pq_header_parses_into_a_table_of_its_own():
    from coati_amd import _abi, _lib, build
    assert sorted(_lib.PQ_PROTOTYPES) == NAMES
    for other in (_lib.PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.SEARCH_PROTOTYPES, _lib.GRAMMAR_PROTOTYPES, _lib.SCREEN_PROTOTYPES,
                  _lib.GUIDE_PROTOTYPES, _lib.LN_XHAT_PROTOTYPES, _lib.GP_PROTOTYPES, _lib.ACQ_PROTOTYPES, _lib.CLUSTER_PROTOTYPES,
                  _lib.IVF_PROTOTYPES, _lib.RADIUS_PROTOTYPES, _lib.GNN_OPS_PROTOTYPES, _lib.SEARCH8_PROTOTYPES, _lib.IVF8_PROTOTYPES,
                  _lib.IVF_RADIUS_PROTOTYPES):
        assert not set(_lib.PQ_PROTOTYPES) & set(other)
    assert not set(NAMES) & set(_lib.exported_symbols())
    assert len(_lib.PROTOTYPES) == 121 and _lib.ABI_VERSION == 5                   # coati_hip.h is unchanged
    Ci, P, L, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert _lib.PQ_PROTOTYPES["coati_pq_encode"] == (Ci, [P, L, Ci, P, P, P])
    assert _lib.PQ_PROTOTYPES["coati_pq_topk"] == (Ci, [P, L, Ci, P, P, P, Ci, Ci, F, Ci, P, P, P, P, P])
    assert _lib.PQ_PROTOTYPES["coati_pq_k_max"] == (Ci, [Ci])
    assert _lib.PQ_PROTOTYPES["coati_pq_slices"] == (Ci, [L, Ci, Ci, Ci])
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.PQ_HEADER) as f:
        text = f.read()
    again = _abi.parse(text, guard="COATI_PQ_H", name="coati_pq.h", base=base)
    assert again.prototypes == _lib.PQ_PROTOTYPES and again.version == _lib.ABI_VERSION and not again.experimental
    assert "pq.hip" in build.HIP_UNITS and build.PQ_HEADER in build._sources()
    assert '#include "coati_hip.h"' in text


def test_library_exports_the_pq_entries():
    from coati_amd import _lib
    l = _lib.lib()
    for name, (restype, argtypes) in _lib.PQ_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_entries_refuse_bad_arguments_with_a_code():
    """decided on the host before any device call: the pointers are host buffers that a refusal never looks at"""
    from coati_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def enc(x=p, n=10, E=64, cb=p, codes=p):
        return l.coati_pq_encode(x, n, E, cb, codes, None), l.coati_last_error().decode()

    def topk(codes=p, N=1000, E=64, cb=p, q=p, Q=4, k=10, S=2, part=p, out=p):
        return l.coati_pq_topk(codes, N, E, cb, p, q, Q, k, 1.0, S, part, part, out, out, None), l.coati_last_error().decode()

    for kw in (dict(x=None), dict(cb=None), dict(codes=None), dict(n=0), dict(n=2 ** 31), dict(E=0), dict(E=48), dict(E=288)):
        rc, msg = enc(**kw)
        assert rc < 0 and "pq_encode" in msg, kw
    for kw in (dict(codes=None), dict(cb=None), dict(q=None), dict(part=None), dict(out=None), dict(N=0), dict(N=2 ** 31), dict(E=0), dict(E=48),
               dict(E=288), dict(Q=0), dict(k=0), dict(k=129), dict(E=256, k=65), dict(S=0), dict(S=3073), dict(k=128, S=241)):
        rc, msg = topk(**kw)
        assert rc < 0 and "pq_topk" in msg, kw
    for E in (0, 48, 288):
        assert l.coati_pq_k_max(E) < 0 and "pq_k_max" in l.coati_last_error().decode()
        assert l.coati_pq_slices(1000, E, 1, 1) < 0 and "pq_slices" in l.coati_last_error().decode()
    assert l.coati_pq_slices(0, 64, 1, 1) < 0 and l.coati_pq_slices(10, 64, 0, 1) < 0 and l.coati_pq_slices(10, 64, 1, 0) < 0
    assert l.coati_pq_slices(10, 256, 1, 65) < 0 and l.coati_pq_slices(10, 64, 1, 129) < 0


def test_k_max_and_default_slices_are_arithmetic():
    """The budget: a CU's 160 KiB of LDS hold the code book (512 E bytes), the lists of a workgroup's 16 NP queries (16 NP (k + 128) 8
    bytes; NP = 2 up to E = 128, else 1) and 16 NP * 8 + 8 bytes of words.  k_max is 128 where that fits, else 64:
    E = 32: 16 KiB + 64 KiB fit -> 128; E = 224: 112 KiB + 32 KiB fit -> 128; E = 256: 128 KiB + 32 KiB + 136 B do not, 128 KiB + 24 KiB do -> 64."""
    from coati_amd import _lib
    l = _lib.lib()

    def lds(E, k):
        NP = 2 if E <= 128 else 1
        return 512 * E + 16 * NP * (k + 128) * 8 + 16 * NP * 8 + 8

    assert l.coati_pq_k_max(256) == 64 and l.coati_pq_k_max(32) == 128
    for E in range(32, 257, 32):
        km = l.coati_pq_k_max(E)
        assert km == (128 if lds(E, 128) <= 160 * 1024 else 64) and lds(E, km) <= 160 * 1024, E
        for N in (1, 63, 64, 65, 16384, 16385, 70001, 4 * 2 ** 20, 2 ** 31 - 1):
            for Q in (1, 16, 64, 65, 1024, 100000):
                for k in (1, 10, 40, km):
                    S = l.coati_pq_slices(N, E, Q, k)
                    # a slice of a library that has more than one is at least 16384 rows: 4 times the code book's bytes in codes
                    assert 1 <= S and S * k <= 30720 and (S == 1 or (S - 1) * 16384 < N), (N, E, Q, k, S)


# ---- 2. the encoder's rule in plain torch and the code books -----------------------------------------------------------------------------
@pytest.mark.parametrize("duplicates", [False, True])
def test_encode_rows_on_integers_is_the_brute_force(duplicates):
    """integers of magnitude <= 15: differences <= 30, squares <= 900, sums <= 7200 -- every operation exact in f32, so the restatement
    equals the float64 brute force byte for byte, ties included (a code book with duplicate entries: the lowest index wins)"""
    from coati_amd import pq as P
    cb = U.int_codebooks(12, 3, duplicates)
    x = _ints((700, 96), 4, -15, 15).to(torch.bfloat16)
    rows, codes = U.composed_rows(cb, 300, 5, 128 if duplicates else 256)
    x = torch.cat([x, rows.to(torch.bfloat16)])
    got = P.encode_rows(x, cb)
    assert got.dtype == torch.uint8 and got.shape == (1000, 12) and torch.equal(got, U.encode64(x, cb))
    assert torch.equal(got[700:], codes)                                           # a composed row gets its own codes back
    if duplicates:
        assert int(got.max()) < 128
    assert torch.equal(P.reconstruct(got[700:], cb), x[700:]) and P.reconstruct(got, cb).dtype == torch.bfloat16


def test_encode_rows_on_gaussian_data_is_within_the_rounding_bound():
    """The chosen entry's float64 distance is at most (1 + 4e-6) times the smallest: an f32 distance carries nine roundings of 2^-24
    relative (difference, square, seven sums of non-negative terms), the two compared distances twice that, 18 * 2^-24 = 1.07e-6, times
    four for head room.  Derived, not measured."""
    from coati_amd import pq as P
    g = torch.Generator().manual_seed(6)
    x = torch.randn(3000, 64, generator=g).to(torch.bfloat16)
    cb = torch.randn(8, 256, 8, generator=g).to(torch.bfloat16)
    got = P.encode_rows(x, cb)
    d = U.distances64(x, cb)
    chosen = d.gather(2, got.to(torch.int64)[:, :, None])[:, :, 0]
    assert bool((chosen <= (1 + 4e-6) * d.amin(dim=2)).all())
    assert float((got != U.encode64(x, cb)).float().mean()) < 1e-3


def test_fit_codebooks_is_reproducible_and_fills_short_samples():
    from coati_amd import pq as P
    g = torch.Generator().manual_seed(7)
    x = torch.randn(3000, 32, generator=g).to(torch.bfloat16)
    a = P.fit_codebooks(x, seed=1, iters=4, sample=1024)
    b = P.fit_codebooks(x, seed=1, iters=4, sample=1024)
    c = P.fit_codebooks(x, seed=2, iters=4, sample=1024)
    assert a.dtype == torch.bfloat16 and a.shape == (4, 256, 8) and a.is_contiguous()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and not torch.equal(a.view(torch.int16), c.view(torch.int16))
    # training lowers the quantisation error of the rows it saw and of the rest
    err = lambda cb: float(U.distances64(x, cb).amin(dim=2).sum())  # noqa: E731
    assert err(a) < err(P.fit_codebooks(x, seed=1, iters=0, sample=1024))
    # fewer than 256 rows: the rows themselves, then entry 0 again, which is never chosen
    few = P.fit_codebooks(x[:100], seed=0, iters=3)
    assert few.shape == (4, 256, 8) and torch.equal(few[:, 100:], few[:, :1].expand(4, 156, 8))
    codes = P.encode_rows(x[:100], few)
    assert int(codes.max()) < 100 and torch.equal(P.reconstruct(codes, few), x[:100])
    with pytest.raises(ValueError):
        P.fit_codebooks(x[:0])


# ---- 3. a lossless library -----------------------------------------------------------------------------------------------------------------
def _lossless(metric, N=400, E=64, seed=11, device="cpu"):
    from coati_amd.search import EmbeddingIndex
    cb = U.int_codebooks(E // 8, seed)
    rows, codes = U.composed_rows(cb, N, seed + 1)
    index = EmbeddingIndex(E, metric=metric, device=device)
    index.add(rows)
    return index, cb, rows, codes


@pytest.mark.parametrize("metric", ["dot", "l2"])
def test_lossless_library_is_searched_exactly(metric):
    from coati_amd import pq as P
    index, cb, rows, codes = _lossless(metric)
    pq = index.pq(codebooks=cb)
    assert isinstance(pq, P.PQIndex) and len(pq) == 400 and pq.keep_rows and pq.metric == metric and pq.dim == pq.dim_padded == 64
    assert torch.equal(pq.codes, codes) and pq.codes.dtype == torch.uint8 and torch.equal(pq.codebooks, cb)
    assert torch.equal(pq.dequantised(), index.vectors) and torch.equal(pq.dequantised().float(), rows)
    assert torch.equal(pq.bias, index.bias)                                        # l2: -|x_hat|^2 = -|x|^2; dot: zeros
    q = _ints((7, 64), 13, -15, 15)
    ws, wr, _ = search_util.index_search(index, q, 9)
    s, r, _ = U.stage1_search(pq, q, 9)
    assert torch.equal(s, ws) and torch.equal(r, wr)
    s2, r2 = U.two_stage_search(pq, index, q, 9, 36)
    assert torch.equal(s2, ws) and torch.equal(r2, wr)


# ---- 4. the index on the CPU -----------------------------------------------------------------------------------------------------------------
def _cpu_index(N=300, E=40, metric="l2", seed=1):
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(E, metric=metric, device="cpu")
    index.add(torch.randn(N, E, generator=torch.Generator().manual_seed(seed)))
    return index


def test_add_in_chunks_equals_add_at_once_and_the_snapshot():
    from coati_amd import pq as P
    x = torch.randn(2500, 40, generator=torch.Generator().manual_seed(2))
    once = P.PQIndex.fit(x, 40, "l2", device="cpu", seed=3, iters=3, sample=512)
    assert len(once) == 0 and once.codes.shape == (0, 8) and once.bias.shape == (0,) and not once.keep_rows and once.dim_padded == 64
    assert once.add(x) == range(0, 2500)
    chunks = P.PQIndex(40, "l2", once.codebooks, device="cpu")
    assert chunks.add(x[:1]) == range(0, 1) and chunks.add(x[1:1100]) == range(1, 1100) and chunks.add(x[1100:]) == range(1100, 2500)
    assert chunks.add(x[:0]) == range(2500, 2500) and len(chunks) == 2500
    assert torch.equal(chunks.codes, once.codes) and torch.equal(chunks.bias, once.bias)
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(40, metric="l2", device="cpu")
    index.add(x)
    snap = index.pq(keep_rows=False, codebooks=once.codebooks)
    assert torch.equal(snap.codes, once.codes) and torch.equal(snap.bias, once.bias) and not snap.keep_rows
    assert torch.equal(once.codes, P.encode_rows(index.vectors, once.codebooks))
    assert snap.add(x[:5]) == range(2500, 2505)                                    # nothing but codes: it may grow
    assert once.bytes_per_row() == 8 + 4


def test_bias_for_the_three_metrics_and_remove():
    from coati_amd import pq as P
    for metric in ("dot", "cosine", "l2"):
        index = _cpu_index(metric=metric)
        index.remove([5])
        pq = index.pq(iters=2, sample=256)
        want = -(pq.dequantised().double() ** 2).sum(dim=1).float() if metric == "l2" else torch.zeros(300)
        want[5] = NEG_INF
        assert torch.equal(pq.bias, want) and pq.bias.dtype == torch.float32, metric
        assert pq._rows16.data_ptr() == index.vectors.data_ptr()                   # a view, not a copy
        index.add(torch.randn(10, 40))
        index.remove([7])
        assert len(pq) == 300 and float(pq.bias[7]) > NEG_INF                      # neither is seen
        pq.remove([7, 8])
        assert float(pq.bias[8]) == NEG_INF and float(pq._bias16[8]) == NEG_INF and float(index.bias[8]) > NEG_INF
        with pytest.raises(IndexError):
            pq.remove([300])
        with pytest.raises(RuntimeError, match="snapshot"):
            pq.add(torch.randn(2, 40))
    bare = P.PQIndex.build(_cpu_index(metric="cosine"), keep_rows=False, iters=1, sample=256)
    assert not bare.keep_rows and bare._rows16 is None and bool((bare.bias == 0).all())


def test_search_refuses_bad_arguments_and_the_cpu():
    from coati_amd import pq as P
    index = _cpu_index()
    pq, bare = index.pq(iters=1, sample=256), index.pq(keep_rows=False, iters=1, sample=256)
    q = torch.randn(3, 40)
    for kw in (dict(k=0), dict(k=129), dict(k=10, oversample=0), dict(k=10, bias=torch.zeros(299)), dict(k=10, bias=torch.zeros(300, dtype=torch.float64)),
               dict(k=10, bias=[0.0] * 300), dict(k=10, slices=0), dict(k=10, slices=30720 // 40 + 1), dict(k=10, rescore=False, slices=3073)):
        with pytest.raises(ValueError):
            pq.search(q, **kw)
    wide = P.PQIndex(256, "dot", U.int_codebooks(32, 1), device="cpu")
    with pytest.raises(ValueError, match="1 .. 64"):
        wide.search(torch.randn(2, 256), 65)
    with pytest.raises(ValueError, match="keep_rows"):
        bare.search(q, 10, rescore=True)
    with pytest.raises(ValueError):
        pq.search(torch.randn(3, 41), 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pq.search(q, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bare.search(q, 10)
    s, r = pq.search(torch.zeros(0, 40), 10)
    assert s.shape == r.shape == (0, 10)
    with pytest.raises(ValueError):
        P.PQIndex(257, "dot", U.int_codebooks(36, 1), device="cpu")
    with pytest.raises(ValueError):
        P.PQIndex(64, "dot", U.int_codebooks(4, 1), device="cpu")
    with pytest.raises(ValueError):
        P.PQIndex(64, "dot", U.int_codebooks(8, 1).float(), device="cpu")


@pytest.mark.parametrize("keep_rows", [True, False])
def test_save_and_load_on_the_cpu(tmp_path, keep_rows):
    from coati_amd import pq as P
    pq = _cpu_index().pq(keep_rows=keep_rows, iters=1, sample=256)
    pq.remove([3])
    path = str(tmp_path / "pq.pt")
    pq.save(path)
    again = P.PQIndex.load(path, device="cpu")
    assert len(again) == 300 and again.keep_rows == keep_rows and again.metric == "l2" and again.dim == 40 and again.dim_padded == 64
    assert torch.equal(again.codes, pq.codes) and torch.equal(again.bias, pq.bias)
    assert torch.equal(again.codebooks.view(torch.int16), pq.codebooks.view(torch.int16))
    if keep_rows:
        assert torch.equal(again._rows16, pq._rows16) and torch.equal(again._bias16, pq._bias16) and float(again._bias16[3]) == NEG_INF
    else:
        assert again.add(torch.randn(4, 40)) == range(300, 304)


def test_build_index_keeps_its_signature_and_build_pq_index_its_own():
    import inspect
    from coati_amd.generative import build_index, build_pq_index
    assert list(inspect.signature(build_index).parameters)[-1] == "list_dtype"
    sig = inspect.signature(build_pq_index)
    assert list(sig.parameters) == ["smiles", "encoder", "tokenizer", "batch_size", "metric", "canon_smiles", "keep_rows", "seed", "iters"]
    assert [sig.parameters[n].default for n in ("batch_size", "metric", "canon_smiles", "keep_rows", "seed", "iters")] == [1024, "cosine", None, True, 0, 20]


# ---- 5. what trained code books recall -------------------------------------------------------------------------------------------------------
FLOOR_1, FLOOR_2, FLOOR_4 = 0.2066, 0.3722, 0.6019


def test_recall_of_trained_code_books():
    """A clustered 20 000 x 64 cosine library (200 centres, noise 0.5: search8_util.clustered, seed 31), 64 queries of the same law, code
    books fitted with seed 0, 8 rounds, 4096 sampled rows; k = 10; everything from the float64 oracles on the CPU.
    Measured recall@10 against the exact oracle: stage 1 alone 0.2266, two stages at oversample 2 0.3922, at oversample 4 0.6219
    (the rows of a centre differ by isotropic noise in all 64 dimensions, which 8 bytes a row resolve poorly: the candidates are of the
    right centre, their order within it is mostly the second stage's work).
    The floors are those values minus 2 points for seed-to-seed spread."""
    from coati_amd.search import EmbeddingIndex
    draw = U.clustered(20000, 64, 31)
    x, q = draw(20000), draw(64)
    index = EmbeddingIndex(64, metric="cosine", device="cpu")
    index.add(x)
    pq = index.pq(seed=0, iters=8, sample=4096)
    _, want, _ = search_util.index_search(index, q, 10)
    _, r1, _ = U.stage1_search(pq, q, 10)
    _, r2 = U.two_stage_search(pq, index, q, 10, 20)
    _, r4 = U.two_stage_search(pq, index, q, 10, 40)
    got = (U.recall(r1, want), U.recall(r2, want), U.recall(r4, want))
    print(f"pq recall@10 on 20000 x 64 clustered: stage 1 {got[0]:.4f}, oversample 2 {got[1]:.4f}, oversample 4 {got[2]:.4f}")
    assert got[0] >= FLOOR_1 and got[1] >= FLOOR_2 and got[2] >= FLOOR_4
