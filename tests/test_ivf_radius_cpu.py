"""Radius search over inverted lists, host side (no GPU): include/coati_ivf_radius.h parses against coati_hip.h to exactly its two entries
and the library exports them, the entries refuse bad arguments with a code before any device call, the Python layer refuses what it
must, and the float64 restatement of tests/ivf_radius_util.py and the position -> row permutation are checked on hand-made data."""
import ctypes
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import ivf_radius_util as IR, ivf_util as I  # noqa: E402

NAMES = ["coati_ivf_radius_count", "coati_ivf_radius_fill"]
INF = float("inf")


# ---- 1. the sixteenth header ---------------------------------------------------------------------------------------------------------
def test_ivf_radius_header_parses_into_a_table_of_its_own():
    from coati_amd import _abi, _lib, build
    assert sorted(_lib.IVF_RADIUS_PROTOTYPES) == NAMES
    for other in (_lib.PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.SEARCH_PROTOTYPES, _lib.GRAMMAR_PROTOTYPES, _lib.SCREEN_PROTOTYPES,
                  _lib.GUIDE_PROTOTYPES, _lib.LN_XHAT_PROTOTYPES, _lib.GP_PROTOTYPES, _lib.ACQ_PROTOTYPES, _lib.CLUSTER_PROTOTYPES,
                  _lib.IVF_PROTOTYPES, _lib.RADIUS_PROTOTYPES, _lib.GNN_OPS_PROTOTYPES, _lib.SEARCH8_PROTOTYPES, _lib.IVF8_PROTOTYPES):
        assert not set(_lib.IVF_RADIUS_PROTOTYPES) & set(other)
    assert not set(NAMES) & set(_lib.exported_symbols())
    assert _lib.ABI_VERSION == 5
    Ci, P, L, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    # lib, ids, bias, list_off, M, E, L, q, Q, pair_q, pair_off, item_off, P, alpha, sub, clamp0, thr, row_hi, seg_rows, segs
    operands = [P, P, P, P, L, Ci, Ci, P, Ci, P, P, P, L, F, P, Ci, P, P, Ci, Ci]
    assert _lib.IVF_RADIUS_PROTOTYPES["coati_ivf_radius_count"] == (Ci, operands + [P, Ci, P])
    assert _lib.IVF_RADIUS_PROTOTYPES["coati_ivf_radius_fill"] == (Ci, operands + [P, P, P, P, Ci, P])
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.IVF_RADIUS_HEADER) as f:
        text = f.read()
    again = _abi.parse(text, guard="COATI_IVF_RADIUS_H", name="coati_ivf_radius.h", base=base)
    assert again.prototypes == _lib.IVF_RADIUS_PROTOTYPES and again.version == 5 and not again.experimental
    assert "ivf_radius.hip" in build.HIP_UNITS and build.IVF_RADIUS_HEADER in build._sources()
    assert '#include "coati_hip.h"' in text


def test_library_exports_the_ivf_radius_entries():
    from coati_amd import _lib
    l = _lib.lib()
    assert l.coati_abi_version() == 5
    for name, (restype, argtypes) in _lib.IVF_RADIUS_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments_with_a_code():
    """decided on the host before any device call: the pointers are host buffers that a refusal never looks at"""
    from coati_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def call(fill, lib=p, ids=p, bias=None, list_off=p, M=1000, E=64, L=8, q=p, Q=4, pair_q=p, pair_off=p, item_off=p, P=16, alpha=1.0,
             sub=None, clamp0=0, thr=p, row_hi=None, seg_rows=128, segs=2, counts=p, offsets=p, out_score=p, out_row=p, blocks=0):
        head = (lib, ids, bias, list_off, M, E, L, q, Q, pair_q, pair_off, item_off, P, alpha, sub, clamp0, thr, row_hi, seg_rows, segs)
        if fill:
            rc = l.coati_ivf_radius_fill(*head, counts, offsets, out_score, out_row, blocks, None)
        else:
            rc = l.coati_ivf_radius_count(*head, counts, blocks, None)
        return rc, l.coati_last_error().decode()

    common = [(dict(lib=None), "lib is null"), (dict(ids=None), "ids"), (dict(list_off=None), "list_off"), (dict(q=None), "q is null"),
              (dict(pair_q=None), "pair_q"), (dict(pair_off=None), "pair_off"), (dict(item_off=None), "item_off"), (dict(thr=None), "thr"),
              (dict(counts=None), "counts"),
              (dict(E=48), "E=48"), (dict(E=544), "E=544"), (dict(E=0), "E=0"), (dict(M=0), "M=0"), (dict(M=2 ** 31), f"M={2 ** 31}"),
              (dict(L=0), "L=0"), (dict(L=4097), "L=4097"), (dict(Q=0), "Q=0"), (dict(P=0), "P=0"), (dict(P=2 ** 31), f"P={2 ** 31}"),
              (dict(seg_rows=0), "seg_rows=0"), (dict(seg_rows=96), "seg_rows=96"), (dict(seg_rows=-64), "seg_rows=-64"),
              (dict(segs=0), "segs=0"), (dict(blocks=-1), "blocks=-1")]
    for fill, name, cases in ((False, "ivf_radius_count", common),
                              (True, "ivf_radius_fill", common + [(dict(offsets=None), "offsets"), (dict(out_score=None), "out_score"),
                                                                  (dict(out_row=None), "out_row")])):
        for kw, word in cases:
            rc, msg = call(fill, **kw)
            assert rc < 0 and name in msg and word in msg, (name, kw, rc, msg)


# ---- 3. the Python layer ---------------------------------------------------------------------------------------------------------------
def _cpu_ivf(metric="l2", n=50, nlist=4, stored=True):
    """an IVFIndex put together by hand on the CPU: row i in list i % nlist (stored=False: every row left out)"""
    from coati_amd.ivf import IVFIndex
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(40, metric=metric, device="cpu")
    index.add(torch.randn(n, 40, generator=torch.Generator().manual_seed(0)))
    assign = torch.arange(n) % nlist if stored else torch.full((n,), -1)
    ids, off = I.inverted(assign, nlist)
    return IVFIndex(40, 64, metric, n, torch.zeros(nlist, 40), index.vectors[ids], ids, index.bias[ids], off[1:] - off[:-1], "cpu")


def test_a_cpu_index_raises_no_cpu_fallback():
    q = torch.randn(3, 40, generator=torch.Generator().manual_seed(1))
    table = torch.tensor([[0, 1], [2, -1], [3, 0]])
    for metric in ("cosine", "l2"):
        ivf = _cpu_ivf(metric)
        for kw in (dict(probes=table), dict(nprobe=2), {}):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                ivf.radius_search(q, 0.5, **kw)
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                ivf.radius_count(q, 0.5, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ivf.near_duplicates(0.5)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ivf.dedup(0.5)


def test_nothing_to_search_gives_empty_results():
    q = torch.randn(3, 40, generator=torch.Generator().manual_seed(1))
    for ivf, queries, Q in ((_cpu_ivf(stored=False), q, 3), (_cpu_ivf(), q[:0], 0)):
        for order in ("row", "score", "probe"):
            offsets, scores, rows = ivf.radius_search(queries, 0.5, order=order)
            assert offsets.tolist() == [0] * (Q + 1) and offsets.dtype == torch.int64
            assert scores.shape == rows.shape == (0,) and scores.dtype == torch.float32 and rows.dtype == torch.int64
        out = ivf.radius_search(queries, 0.5, nprobe=3, return_probes=True)
        assert len(out) == 4 and out[3].shape == (Q, 3) and out[3].dtype == torch.int64
        counts = ivf.radius_count(queries, 0.5)
        assert counts.tolist() == [0] * Q and counts.dtype == torch.int64
    offsets, scores, rows = _cpu_ivf(stored=False).near_duplicates(0.5)
    assert offsets.tolist() == [0] * 51 and scores.numel() == rows.numel() == 0
    assert _cpu_ivf(stored=False).dedup(0.5).tolist() == [False] * 50


def test_argument_validation():
    ivf = _cpu_ivf()
    q = torch.randn(3, 40, generator=torch.Generator().manual_seed(1))
    for bad in (torch.zeros(2), torch.zeros(3, 1), torch.zeros(4), "0.5", None):
        with pytest.raises(ValueError, match="threshold"):
            ivf.radius_search(q, bad)
        with pytest.raises(ValueError, match="threshold"):
            ivf.radius_count(q, bad)
    with pytest.raises(ValueError, match="threshold"):
        ivf.near_duplicates(torch.zeros(2))
    for bad in ("rank", "list", None):
        with pytest.raises(ValueError, match="order"):
            ivf.radius_search(q, 0.5, order=bad)
    for bad in (-1, 1.5, None):
        with pytest.raises(ValueError, match="max_results"):
            ivf.radius_search(q, 0.5, max_results=bad)
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(3), [1, 2]):
        with pytest.raises(ValueError, match="row_below"):
            ivf.radius_search(q, 0.5, row_below=bad)
        with pytest.raises(ValueError, match="row_below"):
            ivf.radius_count(q, 0.5, row_below=bad)
    table = torch.tensor([[0, 1, -1], [2, -1, -1], [3, 0, 1]])
    for bad in (table[:2], table.float(), table.reshape(-1), torch.zeros(3, 129, dtype=torch.int64), torch.zeros(3, 0, dtype=torch.int64)):
        with pytest.raises(ValueError, match="probes"):
            ivf.radius_search(q, 0.5, probes=bad)
        with pytest.raises(ValueError, match="probes"):
            ivf.radius_count(q, 0.5, probes=bad)
    for bad in (0, 129):
        with pytest.raises(ValueError, match="nprobe"):
            ivf.radius_search(q, 0.5, nprobe=bad)
        with pytest.raises(ValueError, match="nprobe"):
            ivf.radius_count(q, 0.5, nprobe=bad)
        with pytest.raises(ValueError, match="nprobe"):
            ivf.near_duplicates(0.5, nprobe=bad)
    for bad in (0, 32, 96, -64):
        with pytest.raises(ValueError, match="seg_rows"):
            ivf.radius_search(q, 0.5, probes=table, seg_rows=bad)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="blocks"):
            ivf.radius_search(q, 0.5, probes=table, blocks=bad)
    with pytest.raises(ValueError, match="chunk"):
        ivf.near_duplicates(0.5, chunk=0)
    with pytest.raises(ValueError):
        ivf.radius_search(torch.zeros(3, 41), 0.5)


def test_exports_and_defaults():
    import coati.generative as G
    import coati_amd.generative as AG
    from coati_amd.ivf import IVFIndex
    from coati_amd.ivf8 import Ivf8Index
    assert G.drop_near_duplicates is AG.drop_near_duplicates
    assert list(inspect.signature(IVFIndex.radius_search).parameters) == ["self", "queries", "threshold", "nprobe", "probes", "order", "row_below",
                                                                         "seg_rows", "max_results", "blocks", "return_probes"]
    sig = inspect.signature(IVFIndex.radius_search).parameters
    assert sig["nprobe"].default == 8 and sig["order"].default == "row" and sig["max_results"].default == 1 << 28 and sig["blocks"].default == 0
    assert list(inspect.signature(IVFIndex.radius_count).parameters) == ["self", "queries", "threshold", "nprobe", "probes", "row_below"]
    assert list(inspect.signature(IVFIndex.near_duplicates).parameters) == ["self", "threshold", "nprobe", "chunk"]
    assert inspect.signature(IVFIndex.near_duplicates).parameters["chunk"].default == 4096
    assert list(inspect.signature(IVFIndex.dedup).parameters) == ["self", "threshold", "nprobe"]
    sig = inspect.signature(AG.drop_near_duplicates).parameters
    assert list(sig) == ["index", "kept", "threshold", "ivf", "nprobe"] and sig["ivf"].default is None and sig["nprobe"].default == 8
    for name in ("radius_search", "radius_count", "near_duplicates", "dedup"):
        assert not hasattr(Ivf8Index, name), name


def test_drop_near_duplicates_refuses_an_ivf_of_another_length():
    from coati_amd.generative import drop_near_duplicates
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(40, metric="l2", device="cpu")
    index.add(torch.randn(49, 40, generator=torch.Generator().manual_seed(0)))
    with pytest.raises(ValueError, match="ivf of 50 rows"):
        drop_near_duplicates(index, ["s"] * 49, -0.5, ivf=_cpu_ivf())


# ---- 4. the oracle and the permutation -------------------------------------------------------------------------------------------------
def _hand_made():
    """six rows of width 2 in three lists: list 0 = rows (1, 4), list 1 = none, list 2 = rows (0, 2, 5); row 3 is left out.  Two queries
    e0, e1: query 0 scores a row's first entry, query 1 its second"""
    x = torch.tensor([[1.0, 0.0], [2.0, 5.0], [3.0, 1.0], [9.0, 9.0], [2.0, -1.0], [-1.0, 2.0]])
    assign = torch.tensor([2, 0, 2, -1, 0, 2])
    ids, off = I.inverted(assign, 3)
    assert ids.tolist() == [1, 4, 0, 2, 5] and off.tolist() == [0, 2, 2, 5]
    bias = torch.zeros(5)
    bias[3] = -INF                                                            # position 3 = row 2 is removed
    return x[ids], ids, bias, off, torch.eye(2)


def test_oracle_on_hand_made_lists():
    lib, ids, bias, off, q = _hand_made()
    probes = torch.tensor([[2, 0], [0, -1]])
    s = IR.masked_scores(lib, ids, bias, off, q, probes, 6)
    assert s[0].tolist() == [1.0, 2.0, -INF, -INF, 2.0, -1.0]                 # the removed and the left-out row are -inf
    assert s[1].tolist() == [-INF, 5.0, -INF, -INF, -1.0, -INF]               # query 1 probes list 0 alone
    offsets, scores, rows = IR.csr(lib, ids, bias, off, q, probes, 6, torch.tensor([1.0, -INF]))
    assert offsets.tolist() == [0, 3, 5] and rows.tolist() == [0, 1, 4, 1, 4] and scores.tolist() == [1.0, 2.0, 2.0, 5.0, -1.0]
    ps, pr = IR.in_probe_order(offsets, scores, rows, probes, ids, off, 6)
    assert pr.tolist() == [0, 1, 4, 1, 4] and ps.tolist() == [1.0, 2.0, 2.0, 5.0, -1.0]     # list 2 (row 0) before list 0 (rows 1, 4)
    ps, pr = IR.in_probe_order(offsets, scores, rows, torch.tensor([[0, 2], [-1, 0]]), ids, off, 6)
    assert pr.tolist() == [1, 4, 0, 1, 4]
    offsets, scores, rows = IR.csr(lib, ids, bias, off, q, probes, 6, -INF, torch.tensor([4, 2]))
    assert offsets.tolist() == [0, 2, 3] and rows.tolist() == [0, 1, 1]
    # l2: min(2 q.x - |x|^2 - |q|^2, 0) with the bias carrying -|x|^2
    l2 = IR.masked_scores(lib, ids, -(lib ** 2).sum(dim=1), off, q, torch.tensor([[0], [2]]), 6, 2.0, True)
    assert l2[0].tolist() == [-INF, -26.0, -INF, -INF, -2.0, -INF] and l2[1].tolist() == [-2.0, -INF, -9.0, -INF, -INF, -2.0]
    assert IR.csr(lib, ids, bias, off, q, torch.tensor([[-1], [1]]), 6, -INF)[0].tolist() == [0, 0, 0]   # nothing probed, an empty list


def test_rows_from_positions_on_hand_made_csr():
    from coati_amd.ivf_radius import rows_from_positions, sort_segments_by_row
    ids = torch.tensor([1, 4, 0, 2, 5], dtype=torch.int32)
    offsets = torch.tensor([0, 2, 2, 3, 3, 6])                                # positions 0 .. 4 hold 2, 0, 1, 0, 3 entries
    scores = torch.tensor([0.5, 1.5, 2.5, 3.5, 4.5, 5.5])
    rows = torch.tensor([0, 0, 7, 1, 2, 4])
    o, s, r = rows_from_positions(offsets, scores, rows, ids, 7)
    assert o.dtype == torch.int64 and o.tolist() == [0, 1, 3, 3, 3, 3, 6, 6]  # row 0 <- position 2, row 1 <- 0, row 5 <- 4; 3 and 6 have none
    assert r.tolist() == [7, 0, 0, 1, 2, 4] and s.tolist() == [2.5, 0.5, 1.5, 3.5, 4.5, 5.5]
    wo, ws, wr = IR.rows_from_positions(offsets, scores.tolist(), rows.tolist(), ids, 7)
    assert wo == o.tolist() and ws == s.tolist() and wr == r.tolist()
    o, s, r = rows_from_positions(torch.zeros(6, dtype=torch.int64), scores[:0], rows[:0], ids, 7)
    assert o.tolist() == [0] * 8 and s.numel() == r.numel() == 0
    s, r = sort_segments_by_row(torch.tensor([0, 3, 3, 6]), scores, torch.tensor([5, 1, 3, 2, 0, 1]))
    assert r.tolist() == [1, 3, 5, 0, 1, 2] and s.tolist() == [1.5, 2.5, 0.5, 4.5, 5.5, 3.5]
