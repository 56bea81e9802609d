"""IVF approximate search, host side (no GPU): include/coati_ivf.h parses against coati_hip.h and the library exports what it declares,
every entry refuses bad arguments with a code before any device call, coati_ivf_plan keeps its bounds, the Python layer refuses what it
must, and the float64 restatement of tests/ivf_util.py is checked on hand-made ties, padding and removed rows."""
import ctypes
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import ivf_util as I  # noqa: E402

NAMES = ["coati_ivf_merge", "coati_ivf_plan", "coati_ivf_scan"]
NEG_INF = float("-inf")


# ---- 1. the eleventh header ---------------------------------------------------------------------------------------------------------
def test_ivf_header_parses_into_a_table_of_its_own():
    from coati_amd import _abi, _lib, build
    assert sorted(_lib.IVF_PROTOTYPES) == NAMES
    for other in (_lib.PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.SEARCH_PROTOTYPES, _lib.GRAMMAR_PROTOTYPES, _lib.SCREEN_PROTOTYPES,
                  _lib.GUIDE_PROTOTYPES, _lib.LN_XHAT_PROTOTYPES, _lib.GP_PROTOTYPES, _lib.ACQ_PROTOTYPES, _lib.CLUSTER_PROTOTYPES):
        assert not set(_lib.IVF_PROTOTYPES) & set(other)
    assert not set(NAMES) & set(_lib.exported_symbols())
    assert _lib.ABI_VERSION == 5
    Ci, P, L, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert _lib.IVF_PROTOTYPES["coati_ivf_scan"] == (Ci, [P, P, P, P, L, Ci, Ci, P, Ci, P, P, P, L, Ci, F, Ci, Ci, P, P, Ci, P])
    assert _lib.IVF_PROTOTYPES["coati_ivf_merge"] == (Ci, [P, P, P, P, L, P, Ci, Ci, Ci, Ci, Ci, Ci, P, P, P])
    assert _lib.IVF_PROTOTYPES["coati_ivf_plan"] == (L, [L, Ci, Ci, Ci])
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.IVF_HEADER) as f:
        again = _abi.parse(f.read(), guard="COATI_IVF_H", name="coati_ivf.h", base=base)
    assert again.prototypes == _lib.IVF_PROTOTYPES and again.version == 5 and not again.experimental
    assert "ivf.hip" in build.HIP_UNITS and build.IVF_HEADER in build._sources()


def test_library_exports_the_ivf_entries():
    from coati_amd import _lib
    l = _lib.lib()
    assert l.coati_abi_version() == 5
    for name, (restype, argtypes) in _lib.IVF_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


# ---- 2. refusals --------------------------------------------------------------------------------------------------------------------
def _host_pointer():
    buf = (ctypes.c_char * 4096)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_ivf_scan_refuses_bad_arguments_with_a_code():
    """decided on the host before any device call: the pointers are host buffers that a refusal never looks at"""
    from coati_amd import _lib
    l = _lib.lib()
    buf, p = _host_pointer()

    def call(lib=p, ids=p, bias=None, list_off=p, M=1000, E=64, L=8, q=p, Q=4, pair_q=p, pair_off=p, item_off=p, P=16, k=10, alpha=1.0,
             seg_rows=128, segs=2, part_score=p, part_row=p, blocks=0):
        rc = l.coati_ivf_scan(lib, ids, bias, list_off, M, E, L, q, Q, pair_q, pair_off, item_off, P, k, alpha, seg_rows, segs, part_score,
                              part_row, blocks, None)
        return rc, l.coati_last_error().decode()

    cases = [(dict(lib=None), "lib"), (dict(ids=None), "ids"), (dict(list_off=None), "list_off"), (dict(q=None), "q is null"),
             (dict(pair_q=None), "pair_q"), (dict(pair_off=None), "pair_off"), (dict(item_off=None), "item_off"),
             (dict(part_score=None), "part_score"), (dict(part_row=None), "part_row"),
             (dict(E=48), "E=48"), (dict(E=544), "E=544"), (dict(E=0), "E=0"), (dict(M=0), "M=0"), (dict(M=2 ** 31), f"M={2 ** 31}"),
             (dict(L=0), "L=0"), (dict(L=4097), "L=4097"), (dict(Q=0), "Q=0"), (dict(P=0), "P=0"), (dict(P=2 ** 31), f"P={2 ** 31}"),
             (dict(k=0), "k=0"), (dict(k=129), "k=129"), (dict(seg_rows=0), "seg_rows=0"), (dict(seg_rows=96), "seg_rows=96"),
             (dict(segs=0), "segs=0"), (dict(blocks=-1), "blocks=-1")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc < 0 and "ivf_scan" in msg and word in msg, (kw, rc, msg)


def test_ivf_merge_refuses_bad_arguments_with_a_code():
    from coati_amd import _lib
    l = _lib.lib()
    buf, p = _host_pointer()

    def call(part_score=p, part_row=p, probes=p, pair_slot=p, P=16, list_off=p, L=8, Q=4, nprobe=4, k=10, seg_rows=128, segs=2,
             out_score=p, out_row=p):
        rc = l.coati_ivf_merge(part_score, part_row, probes, pair_slot, P, list_off, L, Q, nprobe, k, seg_rows, segs, out_score, out_row, None)
        return rc, l.coati_last_error().decode()

    cases = [(dict(part_score=None), "part_score"), (dict(part_row=None), "part_row"), (dict(probes=None), "probes"),
             (dict(pair_slot=None), "pair_slot"), (dict(list_off=None), "list_off"), (dict(out_score=None), "out_score"),
             (dict(out_row=None), "out_row"), (dict(P=0), "P=0"), (dict(L=0), "L=0"), (dict(L=4097), "L=4097"), (dict(Q=0), "Q=0"),
             (dict(nprobe=0), "nprobe=0"), (dict(nprobe=129), "nprobe=129"), (dict(k=0), "k=0"), (dict(k=129), "k=129"),
             (dict(seg_rows=32), "seg_rows=32"), (dict(seg_rows=200), "seg_rows=200"), (dict(segs=0), "segs=0"),
             (dict(nprobe=128, k=128, segs=2), "16384"), (dict(nprobe=8, k=10, segs=205), "16384")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc < 0 and "ivf_merge" in msg and word in msg, (kw, rc, msg)


def test_ivf_plan_bounds():
    """a multiple of 64 of at least 128 rows with nprobe * ceil(max / seg_rows) * k within the merge's row; the value is the header's rule:
    as many segments as bring Q * nprobe pairs to the 512 work items that fill the device, as far as the merge allows"""
    from coati_amd import _lib
    l = _lib.lib()
    for rows in (1, 63, 64, 65, 1000, 4096, 70001, 2 ** 31 - 1):
        for Q in (1, 16, 64, 1024):
            for nprobe in (1, 8, 32, 128):
                for k in (1, 10, 100, 128):
                    seg = l.coati_ivf_plan(rows, Q, nprobe, k)
                    segs = min(-(-512 // (Q * nprobe)), 16384 // (nprobe * k))
                    want = max(128, (-(-rows // segs) + 63) // 64 * 64)
                    if want >= 2 ** 31:                    # one segment of more than 2^31 - 64 rows: no int holds its length
                        assert seg < 0 and "ivf_plan" in l.coati_last_error().decode(), (rows, Q, nprobe, k, seg)
                        continue
                    assert seg == want and seg % 64 == 0 and 128 <= seg < 2 ** 31, (rows, Q, nprobe, k, seg)
                    assert nprobe * -(-rows // seg) * k <= 16384, (rows, Q, nprobe, k, seg)
    assert l.coati_ivf_plan(4096, 1, 8, 10) == 128 and l.coati_ivf_plan(4096, 1024, 32, 100) == 4096
    assert l.coati_ivf_plan(2 ** 20, 1, 1, 10) == 2 ** 20 // 512
    for kw in ((0, 1, 1, 1), (2 ** 31, 1, 1, 1), (100, 0, 1, 1), (100, 1, 0, 1), (100, 1, 129, 1), (100, 1, 1, 0), (100, 1, 1, 129),
               (100, 1, 128, 129)):
        assert l.coati_ivf_plan(*kw) < 0 and "ivf_plan" in l.coati_last_error().decode(), kw


# ---- 3. the Python layer --------------------------------------------------------------------------------------------------------------
def test_python_layer_refuses():
    from coati_amd.ivf import IVFIndex
    from coati_amd.search import EmbeddingIndex
    x = torch.randn(50, 40, generator=torch.Generator().manual_seed(0))
    dot = EmbeddingIndex(40, metric="dot", device="cpu")
    dot.add(x)
    with pytest.raises(ValueError, match="dot"):
        IVFIndex.build(dot, 4)
    with pytest.raises(ValueError, match="dot"):
        dot.ivf(4)
    for metric in ("cosine", "l2"):
        index = EmbeddingIndex(40, metric=metric, device="cpu")
        index.add(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            index.ivf(4)
        with pytest.raises(ValueError, match="nlist"):
            index.ivf(0)
        with pytest.raises(ValueError, match="nlist"):
            index.ivf(4097)


def test_invert_probes_is_the_header_table():
    """the pairs sorted by (list, query), -1 entries behind them; item_off = cumsum(ceil(pairs / 16) * ceil(rows / seg_rows))"""
    from coati_amd.ivf import invert_probes
    probes = torch.tensor([[2, 0, -1], [0, 2, 3], [-1, -1, -1], [3, 0, 2]], dtype=torch.int32)
    sizes = torch.tensor([100, 5, 0, 129])
    pair_q, pair_off, item_off, pair_slot = invert_probes(probes, sizes, 64)
    assert pair_q.dtype == pair_off.dtype == item_off.dtype == pair_slot.dtype == torch.int32
    assert pair_off.tolist() == [0, 3, 3, 6, 8] and pair_q[:8].tolist() == [0, 1, 3, 0, 1, 3, 1, 3]
    assert item_off.tolist() == [0, 2, 2, 2, 5]            # list 1 has no pairs, list 2 no rows
    assert pair_slot.tolist() == [[3, 0, -1], [1, 4, 6], [-1, -1, -1], [7, 2, 5]]
    many = torch.zeros(40, 1, dtype=torch.int32)           # 40 pairs on one list: three groups of <= 16
    assert invert_probes(many, torch.tensor([130]), 64)[2].tolist() == [0, 9]


def test_exports():
    import coati.generative as G
    import coati_amd.generative as AG
    from coati_amd.generative import coati_search
    from coati_amd.ivf import IVFIndex
    from coati_amd.search import EmbeddingIndex
    assert G.build_index is AG.build_index is coati_search.build_index
    assert G.nearest_smiles is AG.nearest_smiles is coati_search.nearest_smiles
    assert inspect.signature(AG.build_index).parameters["nlist"].default is None
    assert list(inspect.signature(IVFIndex.search).parameters)[:3] == ["self", "queries", "k"]
    assert list(inspect.signature(EmbeddingIndex.search).parameters)[:3] == ["self", "queries", "k"]
    assert inspect.signature(IVFIndex.search).parameters["nprobe"].default == 8
    assert callable(EmbeddingIndex.ivf) and callable(IVFIndex.build)


# ---- 4. the oracle ------------------------------------------------------------------------------------------------------------------
def test_inverted_and_recall():
    ids, off = I.inverted(torch.tensor([2, 0, 0, -1, 2, 4, 0]), 5)
    assert ids.tolist() == [1, 2, 6, 0, 4, 5] and off.tolist() == [0, 3, 3, 5, 5, 6]
    exact = torch.tensor([[3, 5, 7], [1, 2, -1]])
    assert I.recall(exact, exact) == 1.0
    assert I.recall(torch.tensor([[7, 9, 3], [2, -1, -1]]), exact) == 3 / 5
    assert I.recall(torch.tensor([[-1, -1, -1], [-1, -1, -1]]), exact) == 0.0


def test_oracle_on_hand_made_ties_padding_and_removed_rows():
    """three lists over original rows 0 .. 7; one query (1, 0): the score is the row's first entry (+ bias).
    list 0 = rows {1, 4, 6}, list 1 = rows {0, 5}, list 2 = rows {2, 3, 7}; positions are in list order"""
    assign = torch.tensor([1, 0, 2, 2, 0, 1, 0, 2])
    ids, off = I.inverted(assign, 3)
    assert ids.tolist() == [1, 4, 6, 0, 5, 2, 3, 7]
    first = torch.tensor([5.0, 3.0, 5.0, 1.0, 5.0, 2.0, 3.0, 0.0])          # by ORIGINAL row: rows 0, 2, 4 tie at 5; rows 1, 6 at 3
    x = torch.zeros(8, 32)
    x[:, 0] = first
    lib16 = x[ids].to(torch.bfloat16)
    q16 = torch.zeros(1, 32, dtype=torch.bfloat16)
    q16[0, 0] = 1
    # all lists: the ties between rows of different lists resolve by original row, not by position (row 4 sits before row 0)
    s, r = I.scan(lib16, ids, None, off, q16, torch.tensor([[2, 0, 1]]), 5)
    assert r.tolist() == [[0, 2, 4, 1, 6]] and s.tolist() == [[5.0, 5.0, 5.0, 3.0, 3.0]]
    # lists 0 and 2 only; a -1 entry is no list
    s, r = I.scan(lib16, ids, None, off, q16, torch.tensor([[0, -1, 2]]), 4)
    assert r.tolist() == [[2, 4, 1, 6]]
    # k larger than the rows probed: padding
    s, r = I.scan(lib16, ids, None, off, q16, torch.tensor([[1, -1, -1]]), 4)
    assert r.tolist() == [[0, 5, -1, -1]] and s.tolist() == [[5.0, 2.0, NEG_INF, NEG_INF]]
    # nothing probed
    s, r = I.scan(lib16, ids, None, off, q16, torch.tensor([[-1, -1, -1]]), 2)
    assert r.tolist() == [[-1, -1]] and s.tolist() == [[NEG_INF, NEG_INF]]
    # a removed row (bias -inf at its POSITION) is never returned; alpha scales the dot, the bias is added after
    bias = torch.zeros(8)
    bias[ids.tolist().index(2)] = NEG_INF
    bias[ids.tolist().index(7)] = 11.0
    s, r = I.scan(lib16, ids, bias, off, q16, torch.tensor([[0, 1, 2]]), 4, alpha=2.0)
    assert r.tolist() == [[7, 0, 4, 1]] and s.tolist() == [[11.0, 10.0, 10.0, 6.0]]
    # -0 and +0 tie: row 7 (score +0) against a row scoring -0
    x2 = x.clone()
    x2[3, 0] = -0.0
    s, r = I.scan(x2[ids].to(torch.bfloat16), ids, None, off, q16, torch.tensor([[2, -1, -1]]), 3)
    assert r.tolist() == [[2, 3, 7]]
