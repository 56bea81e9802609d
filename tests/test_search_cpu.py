"""Embedding-library search, host side (no GPU): include/coati_search.h parses against coati_hip.h and the library exports what it
declares, the entries refuse bad arguments with a code before any device call, coati_search_slices stays within its bounds, the float64
restatement the GPU tests compare against (tests/search_util.py) is right on hand-written cases, and EmbeddingIndex's host logic."""
import ctypes
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import search_util  # noqa: E402

ENTRIES = ("coati_search_topk", "coati_search_slices")
INF = float("inf")


# ---- the third header -----------------------------------------------------------------------------------------------------
def test_search_header_parses_into_a_table_of_its_own():
    from coati_amd import _abi, _lib, build
    assert sorted(_lib.SEARCH_PROTOTYPES) == sorted(ENTRIES)
    assert not set(_lib.SEARCH_PROTOTYPES) & set(_lib.PROTOTYPES) and not set(_lib.SEARCH_PROTOTYPES) & set(_lib.BEAM_PROTOTYPES)
    assert len(_lib.PROTOTYPES) == 121 and _lib.ABI_VERSION == 5 and len(_lib.BEAM_PROTOTYPES) == 4
    I, P, L, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert _lib.SEARCH_PROTOTYPES["coati_search_topk"] == (I, [P, L, I, P, P, I, I, F, I, P, P, P, P, P])
    assert _lib.SEARCH_PROTOTYPES["coati_search_slices"] == (I, [L, I, I])
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.SEARCH_HEADER) as f:
        text = f.read()
    again = _abi.parse(text, guard="COATI_SEARCH_H", name="coati_search.h", base=base)
    assert again.prototypes == _lib.SEARCH_PROTOTYPES and again.version == 5 and not again.experimental
    marker = "#endif /* COATI_SEARCH_H */"
    with pytest.raises(ValueError, match=r"coati_search\.h: coati_gemm_nt is already declared in coati_hip\.h"):
        _abi.parse(text.replace(marker, "int coati_gemm_nt(int a);\n" + marker), guard="COATI_SEARCH_H", name="coati_search.h", base=base)


def test_library_exports_the_search_entries():
    from coati_amd import _lib
    l = _lib.lib()
    assert l.coati_abi_version() == 5
    for name, (restype, argtypes) in _lib.SEARCH_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert not set(ENTRIES) & set(_lib.exported_symbols())


def test_missing_search_header_is_a_runtime_error_naming_the_path(monkeypatch, tmp_path):
    from coati_amd import _lib, build
    gone = str(tmp_path / "include" / "coati_search.h")
    monkeypatch.setattr(build, "SEARCH_HEADER", gone)
    try:
        with pytest.raises(RuntimeError, match="coati_search.h"):
            importlib.reload(_lib)
    finally:
        monkeypatch.undo()
        importlib.reload(_lib)
    assert sorted(_lib.SEARCH_PROTOTYPES) == sorted(ENTRIES)


# ---- bad arguments ----------------------------------------------------------------------------------------------------------
def test_search_topk_refuses_bad_arguments_with_a_code():
    """decided on the host before any device call: the pointers are host buffers that a refusal never looks at"""
    from coati_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def topk(lib=p, N=100, E=64, q=p, Q=3, k=5, S=2, ps=p, pr=p, os_=p, or_=p):
        rc = l.coati_search_topk(lib, N, E, None, q, Q, k, 1.0, S, ps, pr, os_, or_, None)
        return rc, l.coati_last_error().decode()

    for kw in (dict(lib=None), dict(q=None), dict(ps=None), dict(pr=None), dict(os_=None), dict(or_=None)):
        rc, msg = topk(**kw)
        assert rc < 0 and "null" in msg, (kw, rc, msg)
    for kw, word in ((dict(k=0), "k=0"), (dict(k=129), "k=129"), (dict(E=48), "E=48"), (dict(E=544), "E=544"), (dict(E=0), "E=0"),
                     (dict(N=0), "N=0"), (dict(N=2 ** 31), "N=2147483648"), (dict(Q=0), "Q=0"), (dict(S=0), "S=0"),
                     (dict(k=128, S=241), "S=241"), (dict(k=1, S=30721), "S=30721")):
        rc, msg = topk(**kw)
        assert rc < 0 and word in msg, (kw, rc, msg)


def test_search_slices_bounds_and_monotony():
    from coati_amd import _lib
    l = _lib.lib()
    for N in (1, 63, 64, 65, 1000, 70001, 4_000_000, 2 ** 31 - 1):
        for k in (1, 7, 10, 100, 128):
            last = None
            for Q in (1, 2, 16, 17, 64, 65, 130, 1024, 100000):
                S = l.coati_search_slices(N, Q, k)
                assert S >= 1 and S * k <= 30720 and (S - 1) * 64 < N, (N, Q, k, S)      # no slice shorter than one 64-row iteration
                assert last is None or S <= last, (N, Q, k, S, last)
                last = S
    assert l.coati_search_slices(4_000_000, 1, 10) > 1
    for bad in ((0, 1, 1), (2 ** 31, 1, 1), (100, 0, 1), (100, 1, 0), (100, 1, 129), (-5, 1, 1)):
        assert l.coati_search_slices(*bad) < 0 and "search_slices" in l.coati_last_error().decode(), bad


# ---- the oracle on hand-written cases ---------------------------------------------------------------------------------------
def test_oracle_ties_padding_and_removed_rows():
    rows = torch.tensor([[1., 0.], [2., 0.], [1., 0.], [0., 0.], [2., 0.], [-0., 0.]])
    q = torch.tensor([[1., 0.], [-1., 0.]])
    s, r = search_util.search(rows, None, q, 4)
    assert r.tolist() == [[1, 4, 0, 2], [3, 5, 0, 2]] and s.tolist() == [[2., 2., 1., 1.], [0., 0., -1., -1.]]
    assert str(float(s[1, 0])) == str(float(s[1, 1])) == "0.0"                                   # -0 has become +0 and ties with it, row ascending
    s, r = search_util.search(rows, None, q, 8)                          # k > N
    assert r[0].tolist() == [1, 4, 0, 2, 3, 5, -1, -1] and s[0, 6:].tolist() == [-INF, -INF]
    bias = torch.tensor([0., -INF, 0.5, 0., -INF, 0.])                   # rows 1 and 4 removed, row 2 lifted
    s, r = search_util.search(rows, bias, q, 5)
    assert r.tolist() == [[2, 0, 3, 5, -1], [3, 5, 2, 0, -1]] and s[0].tolist() == [1.5, 1., 0., 0., -INF]
    s, r = search_util.search(rows, None, q[:1], 3, alpha=2.0)
    assert s.tolist() == [[4., 4., 2.]] and r.tolist() == [[1, 4, 0]]


@pytest.mark.parametrize("metric", ["dot", "cosine", "l2"])
def test_oracle_metrics_against_torch(metric):
    from coati_amd.search import EmbeddingIndex
    g = torch.Generator().manual_seed(3)
    x, q = torch.randn(50, 40, generator=g), torch.randn(6, 40, generator=g)
    index = EmbeddingIndex(40, metric=metric, device="cpu")
    index.add(x)
    x16 = index.vectors.double()[:, :40]                                   # what is stored, and the queries as they are searched
    q16 = (torch.nn.functional.normalize(q, dim=1) if metric == "cosine" else q).to(torch.bfloat16).double()
    if metric == "dot":
        want = q16 @ x16.T
    elif metric == "cosine":                                               # of vectors that are unit up to bf16 rounding: cos * |q16| |x16|
        want = torch.nn.functional.cosine_similarity(q16[:, None, :], x16[None, :, :], dim=2) * q16.norm(dim=1)[:, None] * x16.norm(dim=1)[None, :]
        assert float((x16.norm(dim=1) - 1).abs().max()) < 2.0 ** -8
    else:
        want = -torch.cdist(q16, x16) ** 2
    got = search_util.index_scores(index, q)
    # the oracle adds the bias AS STORED, -|x|^2 rounded once to f32 (half an ulp: 2^-24 relative); everything else is float64
    tol = 1e-12 * float(want.abs().max()) + (2.0 ** -24 * float((x16 ** 2).sum(1).max()) if metric == "l2" else 0.0)
    assert got.shape == (6, 50) and float((got - want).abs().max()) <= tol
    s, r, _ = search_util.index_search(index, q, 5)
    assert torch.equal(r, want.topk(5, dim=1).indices) and bool((s[:, 1:] <= s[:, :-1]).all())
    if metric == "l2":
        assert bool((got <= 0).all())


# ---- EmbeddingIndex, host logic ------------------------------------------------------------------------------------------------
def test_metric_preparation():
    from coati_amd import search as S
    x = torch.tensor([[3., 4., 0.], [0.1, 0.2, 0.3]])
    f, x16, bias = S.prepare_rows(x, "dot", 3)
    assert f.shape == x16.shape == (2, 32) and x16.dtype == torch.bfloat16 and bool((f[:, 3:] == 0).all()) and bias.tolist() == [0., 0.]
    assert torch.equal(f[:, :3], x) and torch.equal(x16, f.to(torch.bfloat16)) and S.metric_alpha("dot") == 1.0
    f, x16, bias = S.prepare_rows(x, "cosine", 3)
    assert torch.allclose(f[0, :3], torch.tensor([0.6, 0.8, 0.])) and torch.allclose(f.norm(dim=1), torch.ones(2)) and bias.tolist() == [0., 0.]
    f, x16, bias = S.prepare_rows(x, "l2", 3)
    assert torch.equal(f[:, :3], x) and torch.equal(bias, -(x16.double() ** 2).sum(1).float()) and bias[0].item() == -25.0 and S.metric_alpha("l2") == 2.0
    assert bias[1].item() != -(x[1] ** 2).sum().item()                     # of the STORED values
    q32, q16 = S.prepare_queries(x.double(), "cosine", 3)
    assert q32.dtype == torch.float32 and q16.dtype == torch.bfloat16 and q16.is_contiguous() and torch.equal(q16, q32.to(torch.bfloat16))
    assert S.prepare_queries(x[0], "dot", 3)[1].shape == (1, 32)           # one vector is one query
    kernel = torch.tensor([[-20., -INF]])                                  # l2: 2 q.x - |x|^2, then - |q|^2, at most 0; padding stays
    assert S.finish_scores(kernel, "l2", x16[:1]).tolist() == [[-45., -INF]]
    assert S.finish_scores(torch.tensor([[30.]]), "l2", x16[:1]).tolist() == [[0.]]
    assert S.finish_scores(kernel, "dot", x16[:1]) is kernel
    for fn in (lambda: S.prepare_rows(x, "manhattan", 3), lambda: S.metric_alpha("x"), lambda: S.prepare_rows(x, "dot", 4)):
        with pytest.raises(ValueError):
            fn()


def test_index_padding_growth_removal_and_errors(tmp_path):
    from coati_amd.search import MIN_CAPACITY, EmbeddingIndex, padded_dim
    assert [padded_dim(d) for d in (1, 32, 33, 256, 500, 512)] == [32, 32, 64, 256, 512, 512]
    for bad in (0, 513, 1024):
        with pytest.raises(ValueError):
            EmbeddingIndex(bad)
    with pytest.raises(ValueError):
        EmbeddingIndex(64, metric="hamming")
    index = EmbeddingIndex(40, metric="l2", device="cpu", keep_f32=True)
    assert len(index) == 0 and index.vectors.shape == (0, 64) and index.bias.shape == (0,)
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(MIN_CAPACITY - 10, 40, generator=g), torch.randn(30, 40, generator=g).double()
    assert index.add(a) == range(0, MIN_CAPACITY - 10)
    first = index.vectors.clone()
    assert index.add(b) == range(MIN_CAPACITY - 10, MIN_CAPACITY + 20)      # crosses a doubling
    assert len(index) == MIN_CAPACITY + 20 and index._vec.shape[0] == 2 * MIN_CAPACITY
    assert torch.equal(index.vectors[:MIN_CAPACITY - 10], first) and bool((index.vectors[:, 40:] == 0).all())
    assert torch.equal(index.vectors[MIN_CAPACITY - 10:, :40], b.float().to(torch.bfloat16))
    assert torch.equal(index.bias, -(index.vectors.double() ** 2).sum(1).float()) and torch.equal(index._f32[:len(index), :40], torch.cat([a, b.float()]))
    index.remove([3, 5])
    index.remove(torch.tensor([7]))
    assert len(index) == MIN_CAPACITY + 20 and index.bias[[3, 5, 7]].tolist() == [-INF] * 3 and torch.isfinite(index.bias).sum() == len(index) - 3
    with pytest.raises(IndexError):
        index.remove([len(index)])
    with pytest.raises(ValueError):
        index.add(torch.randn(3, 41))
    q = torch.randn(2, 40)
    for k in (0, 129, -1):
        with pytest.raises(ValueError):
            index.search(q, k)
    with pytest.raises(ValueError):
        index.search(torch.randn(2, 39), 3)
    with pytest.raises(ValueError, match="keep_f32"):
        EmbeddingIndex(40, device="cpu").search(q, 3, rescore=2)
    with pytest.raises(ValueError):
        index.search(q, 128, slices=241)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.search(q, 3)                                                    # a missing device is an error, not a torch fallback
    s, r = EmbeddingIndex(40, device="cpu").search(q, 3)                      # an empty index: padding only
    assert s.tolist() == [[-INF] * 3] * 2 and r.tolist() == [[-1] * 3] * 2
    index.save(str(tmp_path / "i.pt"))
    again = EmbeddingIndex.load(str(tmp_path / "i.pt"), device="cpu")
    assert len(again) == len(index) and again.metric == "l2" and again.dim == 40 and again.keep_f32
    assert torch.equal(again.vectors, index.vectors) and torch.equal(again.bias, index.bias) and torch.equal(again._f32[:len(again)], index._f32[:len(index)])


def test_generative_exports():
    import coati.generative as G
    from coati_amd.generative import coati_search
    assert G.build_index is coati_search.build_index and G.nearest_smiles is coati_search.nearest_smiles
