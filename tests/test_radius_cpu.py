"""Radius search, host side (no GPU): include/coati_radius.h parses against coati_hip.h to exactly its three entries and the library
exports them, the entries refuse bad arguments with a code before any device call, coati_radius_slices keeps its bounds, the Python layer
refuses what it must, and the float64 restatement of tests/radius_util.py and the greedy leader rule are checked on hand-made CSR."""
import ctypes
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import radius_util as R  # noqa: E402

NAMES = ["coati_radius_count", "coati_radius_fill", "coati_radius_slices"]
INF = float("inf")


# ---- 1. the twelfth header -----------------------------------------------------------------------------------------------------------
def test_radius_header_parses_into_a_table_of_its_own():
    from coati_amd import _abi, _lib, build
    assert sorted(_lib.RADIUS_PROTOTYPES) == NAMES
    for other in (_lib.PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.SEARCH_PROTOTYPES, _lib.GRAMMAR_PROTOTYPES, _lib.SCREEN_PROTOTYPES,
                  _lib.GUIDE_PROTOTYPES, _lib.LN_XHAT_PROTOTYPES, _lib.GP_PROTOTYPES, _lib.ACQ_PROTOTYPES, _lib.CLUSTER_PROTOTYPES,
                  _lib.IVF_PROTOTYPES):
        assert not set(_lib.RADIUS_PROTOTYPES) & set(other)
    assert not set(NAMES) & set(_lib.exported_symbols())
    assert _lib.ABI_VERSION == 5
    Ci, P, L, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    operands = [P, L, Ci, P, P, Ci, F, P, Ci, P, P, Ci]        # lib, N, E, bias, q, Q, alpha, sub, clamp0, thr, row_hi, S
    assert _lib.RADIUS_PROTOTYPES["coati_radius_count"] == (Ci, operands + [P, P])
    assert _lib.RADIUS_PROTOTYPES["coati_radius_fill"] == (Ci, operands + [P, P, P, P, P])
    assert _lib.RADIUS_PROTOTYPES["coati_radius_slices"] == (Ci, [L, Ci])
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.RADIUS_HEADER) as f:
        text = f.read()
    again = _abi.parse(text, guard="COATI_RADIUS_H", name="coati_radius.h", base=base)
    assert again.prototypes == _lib.RADIUS_PROTOTYPES and again.version == 5 and not again.experimental
    assert "radius.hip" in build.HIP_UNITS and build.RADIUS_HEADER in build._sources()
    assert '#include "coati_hip.h"' in text


def test_declaring_a_name_of_coati_hip_h_is_refused():
    from coati_amd import _abi, build
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.RADIUS_HEADER) as f:
        text = f.read()
    again = text.replace("int coati_radius_slices(int64_t N, int Q);", "int coati_radius_slices(int64_t N, int Q);\nint coati_abi_version(void);")
    assert again != text
    with pytest.raises(ValueError, match="coati_abi_version"):
        _abi.parse(again, guard="COATI_RADIUS_H", name="coati_radius.h", base=base)


def test_library_exports_the_radius_entries():
    from coati_amd import _lib
    l = _lib.lib()
    assert l.coati_abi_version() == 5
    for name, (restype, argtypes) in _lib.RADIUS_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments_with_a_code():
    """decided on the host before any device call: the pointers are host buffers that a refusal never looks at"""
    from coati_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def call(fill, lib=p, N=1000, E=64, bias=None, q=p, Q=4, alpha=1.0, sub=None, clamp0=0, thr=p, row_hi=None, S=2, counts=p, offsets=p,
             out_score=p, out_row=p):
        if fill:
            rc = l.coati_radius_fill(lib, N, E, bias, q, Q, alpha, sub, clamp0, thr, row_hi, S, counts, offsets, out_score, out_row, None)
        else:
            rc = l.coati_radius_count(lib, N, E, bias, q, Q, alpha, sub, clamp0, thr, row_hi, S, counts, None)
        return rc, l.coati_last_error().decode()

    common = [(dict(lib=None), "lib"), (dict(q=None), "q is null"), (dict(thr=None), "thr"), (dict(counts=None), "counts"),
              (dict(E=48), "E=48"), (dict(E=544), "E=544"), (dict(E=0), "E=0"), (dict(N=0), "N=0"), (dict(N=2 ** 31), f"N={2 ** 31}"),
              (dict(Q=0), "Q=0"), (dict(S=0), "S=0"), (dict(S=65536), "S=65536")]
    for fill, name, cases in ((False, "radius_count", common),
                              (True, "radius_fill", common + [(dict(offsets=None), "offsets"), (dict(out_score=None), "out_score"),
                                                              (dict(out_row=None), "out_row")])):
        for kw, word in cases:
            rc, msg = call(fill, **kw)
            assert rc < 0 and name in msg and word in msg, (name, kw, rc, msg)


def test_radius_slices_bounds():
    """enough slices to bring ceil(Q / 64) query tiles to the 512 workgroups that fill the device, no slice below 64 rows, at most 65535;
    no merge bound"""
    from coati_amd import _lib
    l = _lib.lib()
    for N in (1, 63, 64, 65, 1000, 70001, 4 * 2 ** 20, 2 ** 31 - 1):
        for Q in (1, 16, 64, 65, 1024, 100000):
            S = l.coati_radius_slices(N, Q)
            assert S == max(1, min(-(-512 // -(-Q // 64)), -(-N // 64), 65535)), (N, Q, S)
    assert l.coati_radius_slices(4 * 2 ** 20, 1) == 512 and l.coati_radius_slices(4 * 2 ** 20, 1024) == 32
    for bad in ((0, 1), (2 ** 31, 1), (100, 0)):
        assert l.coati_radius_slices(*bad) < 0 and "radius_slices" in l.coati_last_error().decode(), bad


# ---- 3. the Python layer ---------------------------------------------------------------------------------------------------------------
def _cpu_index(metric="cosine", n=50):
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(40, metric=metric, device="cpu")
    if n:
        index.add(torch.randn(n, 40, generator=torch.Generator().manual_seed(0)))
    return index


def test_a_cpu_index_raises_no_cpu_fallback():
    q = torch.randn(3, 40, generator=torch.Generator().manual_seed(1))
    for metric in ("dot", "cosine", "l2"):
        index = _cpu_index(metric)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            index.radius_search(q, 0.5)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            index.radius_count(q, 0.5)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            index.near_duplicates(0.5)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            index.dedup(0.5)


def test_nothing_to_search_gives_empty_results():
    q = torch.randn(3, 40, generator=torch.Generator().manual_seed(1))
    for index, queries, Q in ((_cpu_index(n=0), q, 3), (_cpu_index(), q[:0], 0)):
        offsets, scores, rows = index.radius_search(queries, 0.5)
        assert offsets.tolist() == [0] * (Q + 1) and offsets.dtype == torch.int64
        assert scores.shape == rows.shape == (0,) and scores.dtype == torch.float32 and rows.dtype == torch.int64
        counts = index.radius_count(queries, 0.5)
        assert counts.tolist() == [0] * Q and counts.dtype == torch.int64
    offsets, scores, rows = _cpu_index(n=0).near_duplicates(0.5)
    assert offsets.tolist() == [0] and scores.numel() == rows.numel() == 0
    assert _cpu_index(n=0).dedup(0.5).tolist() == []


def test_argument_validation():
    index = _cpu_index()
    q = torch.randn(3, 40, generator=torch.Generator().manual_seed(1))
    for bad in (torch.zeros(2), torch.zeros(3, 1), torch.zeros(4), "0.5", None):
        with pytest.raises(ValueError, match="threshold"):
            index.radius_search(q, bad)
        with pytest.raises(ValueError, match="threshold"):
            index.radius_count(q, bad)
    with pytest.raises(ValueError, match="order"):
        index.radius_search(q, 0.5, order="rank")
    for bad in (-1, 1.5, None):
        with pytest.raises(ValueError, match="max_results"):
            index.radius_search(q, 0.5, max_results=bad)
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(3), [1, 2]):
        with pytest.raises(ValueError, match="row_below"):
            index.radius_search(q, 0.5, row_below=bad)
    for bad in (0, 65536):
        with pytest.raises(ValueError, match="slices"):
            index.radius_search(q, 0.5, slices=bad)
    with pytest.raises(ValueError, match="chunk"):
        index.near_duplicates(0.5, chunk=0)
    with pytest.raises(ValueError):
        index.radius_search(torch.zeros(3, 41), 0.5)


def test_exports():
    import coati.generative as G
    import coati_amd.generative as AG
    from coati_amd.generative import coati_search
    from coati_amd.search import EmbeddingIndex
    assert G.smiles_within is AG.smiles_within is coati_search.smiles_within
    assert G.drop_near_duplicates is AG.drop_near_duplicates is coati_search.drop_near_duplicates
    assert list(inspect.signature(EmbeddingIndex.radius_search).parameters) == ["self", "queries", "threshold", "order", "row_below", "slices",
                                                                                 "max_results"]
    assert inspect.signature(EmbeddingIndex.radius_search).parameters["max_results"].default == 1 << 28
    assert list(inspect.signature(EmbeddingIndex.radius_count).parameters) == ["self", "queries", "threshold", "row_below"]
    assert list(inspect.signature(EmbeddingIndex.near_duplicates).parameters) == ["self", "threshold", "chunk"]
    assert list(inspect.signature(AG.smiles_within).parameters) == ["queries", "index", "kept", "encoder", "tokenizer", "threshold", "canon_smiles"]


def test_sort_segments_by_score_is_one_stable_sort():
    from coati_amd.radius import sort_segments_by_score
    offsets = torch.tensor([0, 4, 4, 9])
    scores = torch.tensor([1.0, 3.0, 1.0, -2.0, 0.0, -0.0, 5.0, -INF, 5.0])
    rows = torch.tensor([2, 5, 7, 9, 0, 1, 3, 4, 8])
    s, r = sort_segments_by_score(offsets, scores, rows)
    assert r.tolist() == [5, 2, 7, 9, 3, 8, 0, 1, 4] and s.tolist() == [3.0, 1.0, 1.0, -2.0, 5.0, 5.0, 0.0, 0.0, -INF]
    ws, wr = R.by_score(offsets, scores, rows)
    assert torch.equal(wr, r) and torch.equal(ws, s)


# ---- 4. the oracle and the greedy rule ------------------------------------------------------------------------------------------------
def test_oracle_on_a_hand_made_score_matrix():
    s = torch.tensor([[1.0, 3.0, -INF, 3.0, 0.0], [2.0, 2.0, 2.0, -INF, 2.0], [0.0, 0.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    offsets, scores, rows = R.csr_of(s, 3.0)                                  # ties at the threshold are kept by >=
    assert offsets.tolist() == [0, 2, 2, 2] and rows.tolist() == [1, 3] and scores.tolist() == [3.0, 3.0]
    offsets, scores, rows = R.csr_of(s, torch.tensor([-INF, 2.0, INF]))       # -inf: every live row, never a removed one; +inf: nothing
    assert offsets.tolist() == [0, 4, 8, 8] and rows.tolist() == [0, 1, 3, 4, 0, 1, 2, 4]
    offsets, scores, rows = R.csr_of(s, -INF, torch.tensor([0, 3, 5]))
    assert offsets.tolist() == [0, 0, 3, 8] and rows.tolist() == [0, 1, 2, 0, 1, 2, 3, 4]
    ss, rr = R.by_score(*R.csr_of(s, -INF))
    assert rr.tolist() == [1, 3, 0, 4, 0, 1, 2, 4, 0, 1, 2, 3, 4]


def test_greedy_leader_rule_on_hand_made_csr():
    """a chain a ~ b ~ c with a not~ c: a is kept, b is dropped, c is kept (its only earlier neighbour was dropped)"""
    from coati_amd.radius import greedy_leaders
    cases = [
        # rows 0 = a, 1 = b, 2 = c
        ([0, 0, 1, 2], [0, 1], [True, True, True], [True, False, True]),
        # a triangle: only the first stays
        ([0, 0, 1, 3], [0, 0, 1], [True, True, True], [True, False, False]),
        # a removed row is False and, being nobody's neighbour, protects nobody: row 2 ~ row 0 only
        ([0, 0, 0, 1, 1], [0], [True, False, True, True], [True, False, False, True]),
        # row 3's neighbours 1 (dropped) and 2 (kept)
        ([0, 0, 1, 1, 3, 4], [0, 1, 2, 3], [True] * 5, [True, False, True, False, True]),
        ([0], [], [], []),
    ]
    for offsets, rows, live, want in cases:
        assert R.greedy(offsets, rows, live) == want
        got = greedy_leaders(torch.tensor(offsets), torch.tensor(rows, dtype=torch.int64), torch.tensor(live, dtype=torch.bool))
        assert got.dtype == torch.bool and got.tolist() == want
