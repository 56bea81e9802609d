"""IVF search over fp8 lists, host side (no GPU): include/coati_ivf8.h parses against coati_hip.h and the library exports what it
declares, coati_ivf8_scan refuses bad arguments with a code before any device call, an Ivf8Index put together by hand keeps the layout
rules, the Python layer refuses what it must, and the float64 restatement of tests/ivf8_util.py equals tests/ivf_util.py's on data that
e4m3 holds exactly."""
import ctypes
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import ivf8_util as I8, ivf_util as I, search_util as SU  # noqa: E402

NEG_INF = float("-inf")
SIZES = [5, 0, 70, 1, 130]


def _assign(sizes=SIZES, left_out=2, seed=3):
    """a shuffled assignment with the given list sizes and `left_out` rows in no list"""
    a = torch.cat([torch.full((n,), l) for l, n in enumerate(sizes)] + [torch.full((left_out,), -1)])
    return a[torch.randperm(a.shape[0], generator=torch.Generator().manual_seed(seed))]


# ---- 1. the fifteenth header ----------------------------------------------------------------------------------------------------------
def test_ivf8_header_parses_into_a_table_of_its_own():
    from coati_amd import _abi, _lib, build
    assert sorted(_lib.IVF8_PROTOTYPES) == ["coati_ivf8_scan"]
    for other in (_lib.PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.SEARCH_PROTOTYPES, _lib.GRAMMAR_PROTOTYPES, _lib.SCREEN_PROTOTYPES,
                  _lib.GUIDE_PROTOTYPES, _lib.LN_XHAT_PROTOTYPES, _lib.GP_PROTOTYPES, _lib.ACQ_PROTOTYPES, _lib.CLUSTER_PROTOTYPES,
                  _lib.IVF_PROTOTYPES, _lib.RADIUS_PROTOTYPES, _lib.GNN_OPS_PROTOTYPES, _lib.SEARCH8_PROTOTYPES):
        assert not set(_lib.IVF8_PROTOTYPES) & set(other)
    assert "coati_ivf8_scan" not in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 5
    Ci, P, L, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    restype, argtypes = _lib.IVF8_PROTOTYPES["coati_ivf8_scan"]
    assert len(argtypes) == 23
    assert (restype, argtypes) == (Ci, [P, P, P, P, P, L, Ci, Ci, P, P, Ci, P, P, P, L, Ci, F, Ci, Ci, P, P, Ci, P])
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.IVF8_HEADER) as f:
        again = _abi.parse(f.read(), guard="COATI_IVF8_H", name="coati_ivf8.h", base=base)
    assert again.prototypes == _lib.IVF8_PROTOTYPES and again.version == 5 and not again.experimental
    assert "ivf8.hip" in build.HIP_UNITS and build.IVF8_HEADER in build._sources()


def test_library_exports_the_ivf8_entry():
    from coati_amd import _lib
    l = _lib.lib()
    assert l.coati_abi_version() == 5
    for name, (restype, argtypes) in _lib.IVF8_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


# ---- 2. refusals --------------------------------------------------------------------------------------------------------------------
def test_ivf8_scan_refuses_bad_arguments_with_a_code():
    """decided on the host before any device call: the pointers are host buffers that a refusal never looks at"""
    from coati_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def call(lib8=p, scale=p, ids=p, bias=p, list_off=p, M=1000, E=64, L=8, q8=p, qscale=p, Q=4, pair_q=p, pair_off=p, item_off=p, P=16, k=10,
             alpha=1.0, seg_rows=128, segs=2, part_score=p, part_row=p, blocks=0):
        rc = l.coati_ivf8_scan(lib8, scale, ids, bias, list_off, M, E, L, q8, qscale, Q, pair_q, pair_off, item_off, P, k, alpha, seg_rows, segs,
                               part_score, part_row, blocks, None)
        return rc, l.coati_last_error().decode()

    cases = [(dict(lib8=None), "lib8"), (dict(scale=None), "scale is null"), (dict(ids=None), "ids"), (dict(bias=None), "bias"),
             (dict(list_off=None), "list_off"), (dict(q8=None), "q8"), (dict(qscale=None), "qscale"), (dict(pair_q=None), "pair_q"),
             (dict(pair_off=None), "pair_off"), (dict(item_off=None), "item_off"), (dict(part_score=None), "part_score"),
             (dict(part_row=None), "part_row"),
             (dict(E=48), "E=48"), (dict(E=544), "E=544"), (dict(E=0), "E=0"), (dict(M=0), "M=0"), (dict(M=2 ** 31), f"M={2 ** 31}"),
             (dict(L=0), "L=0"), (dict(L=4097), "L=4097"), (dict(Q=0), "Q=0"), (dict(P=0), "P=0"), (dict(P=2 ** 31), f"P={2 ** 31}"),
             (dict(k=0), "k=0"), (dict(k=129), "k=129"), (dict(seg_rows=0), "seg_rows=0"), (dict(seg_rows=96), "seg_rows=96"),
             (dict(segs=0), "segs=0"), (dict(blocks=-1), "blocks=-1")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc < 0 and "ivf8_scan" in msg and word in msg, (kw, rc, msg)


# ---- 3. the index put together by hand ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_layout_rules(metric):
    from coati_amd import fp8_index as F
    x = torch.randn(208, 40, generator=torch.Generator().manual_seed(1)) * 3
    assign = _assign()
    ivf8, index = I8.by_hand(x, assign, metric)
    assert len(ivf8) == 208 and ivf8.nlist == 5 and ivf8.keep_rows and ivf8.dim == 40 and ivf8.dim_padded == 64 and ivf8.metric == metric
    assert ivf8.sizes.tolist() == SIZES and ivf8.list_offsets.tolist() == [0, 5, 5, 75, 76, 206] and ivf8.list_offsets.dtype == torch.int32
    ids = ivf8.ids.long()
    assert ivf8.ids.dtype == torch.int32 and sorted(ids.tolist()) == torch.nonzero(assign >= 0).reshape(-1).tolist()
    for l in range(5):                                                       # ids ascend inside every list, and the list is the assignment's
        rows = ivf8.list_rows(l)
        assert torch.equal(rows, torch.nonzero(assign == l).reshape(-1)) and bool((rows[1:] > rows[:-1]).all())
    with pytest.raises(IndexError):
        ivf8.list_rows(5)
    # the bytes are quantise_rows of the rows in list order
    b, s = F.quantise_rows(index.vectors[ids])
    assert ivf8.vectors8.dtype == torch.uint8 and torch.equal(ivf8.vectors8, b) and torch.equal(ivf8.scales, s)
    assert torch.equal(ivf8.dequantised(), F.dequantise(b, s))
    # stage 1's bias: the index's, for l2 -|x_hat|^2 of the dequantised row
    if metric == "l2":
        assert torch.equal(ivf8.bias, -(F.dequantise(b, s).double() ** 2).sum(dim=1).float())
        assert not torch.equal(ivf8.bias, index.bias[ids])
    else:
        assert torch.equal(ivf8.bias, index.bias[ids])
    # stage 2 reads the index's rows in place
    assert ivf8._rows16.data_ptr() == index.vectors.data_ptr() and ivf8._bias16.data_ptr() != index.bias.data_ptr()
    assert torch.equal(ivf8._bias16, index.bias)
    bare, _ = I8.by_hand(x, assign, metric, keep_rows=False)
    assert not bare.keep_rows and bare._rows16 is None and bare._bias16 is None


def test_l2_bias_stays_minus_infinity_where_the_index_removed_a_row():
    from coati_amd.ivf8 import stage1_bias
    from coati_amd import fp8_index as F
    x16 = torch.randn(6, 32, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    b, s = F.quantise_rows(x16)
    bias16 = -(x16.double() ** 2).sum(dim=1).float()
    bias16[4] = NEG_INF
    out = stage1_bias("l2", b, s, bias16)
    assert out[4] == NEG_INF and torch.equal(out[:4], -(F.dequantise(b, s).double() ** 2).sum(dim=1).float()[:4])
    assert torch.equal(stage1_bias("cosine", b, s, bias16), bias16)


def test_remove_hits_both_biases():
    x = torch.randn(208, 40, generator=torch.Generator().manual_seed(1))
    assign = _assign()
    ivf8, index = I8.by_hand(x, assign, "l2")
    left_out = torch.nonzero(assign < 0).reshape(-1)
    gone = [int(ivf8.ids[0]), int(ivf8.ids[100]), int(left_out[0])]
    ivf8.remove(gone)
    removed = torch.nonzero(ivf8.bias == NEG_INF).reshape(-1)
    assert sorted(ivf8.ids[removed].tolist()) == sorted(gone[:2])           # by position in stage 1 (a left-out row has none) ...
    assert sorted(torch.nonzero(ivf8._bias16 == NEG_INF).reshape(-1).tolist()) == sorted(gone)   # ... by original row in stage 2
    assert bool((index.bias > NEG_INF).all()) and len(ivf8) == 208          # the source index is not touched
    ivf8.remove([])
    for bad in ([-1], [208], [0, 300]):
        with pytest.raises(IndexError, match="0 .. 207"):
            ivf8.remove(bad)
    bare, _ = I8.by_hand(x, assign, "l2", keep_rows=False)
    bare.remove(gone)
    assert int((bare.bias == NEG_INF).sum()) == 2


@pytest.mark.parametrize("keep_rows", [True, False])
def test_save_load_round_trip(tmp_path, keep_rows):
    from coati_amd.ivf8 import Ivf8Index
    x = torch.randn(208, 40, generator=torch.Generator().manual_seed(4)) * 2
    ivf8, index = I8.by_hand(x, _assign(), "l2", keep_rows=keep_rows)
    ivf8.remove([int(ivf8.ids[7])])
    path = str(tmp_path / "ivf8.pt")
    ivf8.save(path)
    saved = torch.load(path, map_location="cpu")
    assert ("rows16" in saved) == keep_rows and ("vectors8" in saved) != keep_rows      # the bf16 rows or the bytes, never both
    back = Ivf8Index.load(path, device="cpu")
    assert back.keep_rows == keep_rows and len(back) == 208 and back.metric == "l2" and back.dim == 40 and back.nlist == 5
    for name in ("vectors8", "scales", "bias", "ids", "sizes", "list_offsets", "centres"):
        assert torch.equal(getattr(back, name), getattr(ivf8, name)), name               # re-quantised on load: the same bytes
    if keep_rows:
        assert torch.equal(back._rows16, ivf8._rows16) and torch.equal(back._bias16, ivf8._bias16)


# ---- 4. the Python layer ----------------------------------------------------------------------------------------------------------------
def test_search_refuses():
    x = torch.randn(208, 40, generator=torch.Generator().manual_seed(5))
    ivf8, _ = I8.by_hand(x, _assign(), "cosine")
    bare, _ = I8.by_hand(x, _assign(), "cosine", keep_rows=False)
    q = x[:3]
    table = torch.tensor([[0, 2, -1], [4, -1, -1], [3, 4, 0]])
    for k in (0, 129):
        with pytest.raises(ValueError, match=f"k={k}"):
            ivf8.search(q, k, probes=table)
    with pytest.raises(ValueError, match="oversample=0"):
        ivf8.search(q, 5, oversample=0, probes=table)
    with pytest.raises(ValueError, match="keep_rows"):
        bare.search(q, 5, rescore=True, probes=table)
    for bias in (torch.zeros(207), torch.zeros(208, dtype=torch.float64), [0.0] * 208):
        with pytest.raises(ValueError, match="bias"):
            ivf8.search(q, 5, probes=table, bias=bias)
    for seg_rows in (0, 32, 96, -64):
        with pytest.raises(ValueError, match="seg_rows"):
            ivf8.search(q, 5, probes=table, seg_rows=seg_rows)
    for probes in (table[:2], table.float(), table.reshape(-1), torch.zeros(3, 129, dtype=torch.int64), torch.zeros(3, 0, dtype=torch.int64)):
        with pytest.raises(ValueError, match="probes"):
            ivf8.search(q, 5, probes=probes)
    for nprobe in (0, 129):
        with pytest.raises(ValueError, match="nprobe"):
            ivf8.search(q, 5, nprobe=nprobe)
    # nprobe * segs * kk: 128 lists x 3 segments of 64 rows (the longest list has 130) x 128 candidates
    wide = torch.full((3, 128), -1, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"nprobe \* segs \* k <= 16384"):
        ivf8.search(q, 32, oversample=4, probes=wide, seg_rows=64)
    with pytest.raises(ValueError, match=r"nprobe \* segs \* k <= 16384"):
        bare.search(q, 128, probes=wide, seg_rows=64)


def test_no_cpu_fallback_and_empty_queries():
    x = torch.randn(208, 40, generator=torch.Generator().manual_seed(6))
    ivf8, _ = I8.by_hand(x, _assign(), "l2")
    table = torch.tensor([[0, 2], [4, -1]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ivf8.search(x[:2], 5, probes=table)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ivf8.search(x[:2], 5, probes=table, rescore=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ivf8.search(x[:2], 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ivf8.probe(x[:2], 2)
    for rescore in (None, False):
        s, r = ivf8.search(x[:0], 7, rescore=rescore)
        assert s.shape == (0, 7) and r.shape == (0, 7) and s.dtype == torch.float32 and r.dtype == torch.int64
    s, r, t = ivf8.search(x[:0], 7, nprobe=3, return_probes=True)
    assert s.shape == (0, 7) and t.shape == (0, 3) and t.dtype == torch.int64


def test_building_refuses():
    from coati_amd.ivf import IVFIndex
    from coati_amd.ivf8 import Ivf8Index
    from coati_amd.search import EmbeddingIndex
    x = torch.randn(50, 40, generator=torch.Generator().manual_seed(0))
    dot = EmbeddingIndex(40, metric="dot", device="cpu")
    dot.add(x)
    with pytest.raises(ValueError, match="dot"):
        Ivf8Index.build(dot, 4)
    with pytest.raises(ValueError, match="dot"):
        dot.ivf(4, fp8=True)
    index = EmbeddingIndex(40, metric="l2", device="cpu")
    index.add(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.ivf(4, fp8=True)
    for nlist in (0, 4097):
        with pytest.raises(ValueError, match="nlist"):
            index.ivf(nlist, fp8=True, keep_rows=False)
    # from_ivf: the source index must be the IVFIndex's
    assign = torch.arange(50) % 4
    ids, off = I.inverted(assign, 4)
    ivf = IVFIndex(40, 64, "l2", 50, torch.zeros(4, 40), index.vectors[ids], ids, index.bias[ids], off[1:] - off[:-1], "cpu")
    ivf8 = ivf.fp8(index)
    assert isinstance(ivf8, Ivf8Index) and ivf8.keep_rows and ivf8._rows16.data_ptr() == index.vectors.data_ptr()
    assert torch.equal(ivf8.ids, ivf.ids) and torch.equal(ivf8.sizes, ivf.sizes) and not Ivf8Index.from_ivf(ivf).keep_rows
    other = EmbeddingIndex(40, metric="cosine", device="cpu")
    other.add(x)
    short = EmbeddingIndex(40, metric="l2", device="cpu")
    short.add(x[:49])
    for wrong in (other, short):
        with pytest.raises(ValueError, match="source"):
            Ivf8Index.from_ivf(ivf, wrong)


def test_build_index_keywords():
    from coati_amd.generative import build_index
    with pytest.raises(ValueError, match="fp8"):
        build_index([], None, None, nlist=4, fp8=True)
    with pytest.raises(ValueError, match='list_dtype="fp8"'):
        build_index([], None, None, nlist=4, fp8=True)                        # ... and points at the keyword that does it
    with pytest.raises(ValueError, match="nlist"):
        build_index([], None, None, list_dtype="fp8")
    with pytest.raises(ValueError, match="fp4"):
        build_index([], None, None, nlist=4, list_dtype="fp4")
    with pytest.raises(ValueError, match="fp4"):
        build_index([], None, None, list_dtype="fp4")


def test_exports_and_defaults():
    import coati.generative as G
    import coati_amd.generative as AG
    from coati_amd.ivf import IVFIndex, ListIndex, make_lists
    from coati_amd.ivf8 import Ivf8Index
    from coati_amd.search import EmbeddingIndex
    assert G.build_index is AG.build_index
    assert inspect.signature(AG.build_index).parameters["list_dtype"].default == "bf16"
    assert list(inspect.signature(AG.build_index).parameters)[-1] == "list_dtype"
    sig = inspect.signature(Ivf8Index.search).parameters
    assert list(sig) == ["self", "queries", "k", "nprobe", "oversample", "rescore", "probes", "seg_rows", "bias", "return_probes", "blocks"]
    assert sig["nprobe"].default == 8 and sig["oversample"].default == 4 and sig["rescore"].default is None and sig["blocks"].default == 0
    assert list(inspect.signature(EmbeddingIndex.ivf).parameters) == ["self", "nlist", "iters", "seed", "centres", "fp8", "keep_rows"]
    assert inspect.signature(EmbeddingIndex.ivf).parameters["fp8"].default is False
    assert inspect.signature(EmbeddingIndex.ivf).parameters["keep_rows"].default is True
    assert list(inspect.signature(Ivf8Index.build).parameters) == ["index", "nlist", "iters", "seed", "centres", "assign", "keep_rows"]
    assert list(inspect.signature(IVFIndex.build).parameters) == ["index", "nlist", "iters", "seed", "centres", "assign"]
    assert list(inspect.signature(IVFIndex.fp8).parameters) == ["self", "index"]
    assert issubclass(Ivf8Index, ListIndex) and issubclass(IVFIndex, ListIndex) and callable(make_lists)
    for name in ("probe", "plan", "remove", "sizes", "ids", "bias", "list_offsets", "list_rows", "vectors8", "scales", "dequantised", "save",
                 "load", "from_ivf", "__len__"):
        assert hasattr(Ivf8Index, name), name


# ---- 5. the oracle ------------------------------------------------------------------------------------------------------------------
def test_oracle_equals_the_bf16_oracle_on_integers():
    """integers of magnitude <= 15 are e4m3 values: the dequantised operands ARE the bf16 ones, so scan8 is ivf_util.scan under the
    metric -- scores, rows, ties by original row, padding, a removed row and an extra bias included"""
    from coati_amd.search import metric_alpha, prepare_queries
    x = SU.ints((208, 40), 7, -15, 15)
    q = SU.ints((6, 40), 8, -15, 15)
    x[50:60] = x[10]                                                         # ties across lists
    assign = _assign()
    probes = torch.tensor([[0, 2, 4], [4, -1, -1], [1, -1, -1], [3, 0, -1], [-1, -1, -1], [2, 4, 3]])
    extra = SU.ints((208,), 9, -3, 3)
    extra[11] = NEG_INF
    for metric in ("l2", "cosine"):
        ivf8, index = I8.by_hand(x, assign, metric)
        ivf8.remove([int(ivf8.ids[80])])
        ids = ivf8.ids.long()
        _, q16 = prepare_queries(q, metric, 40, "cpu")
        if metric == "l2":
            assert torch.equal(ivf8.dequantised(), index.vectors[ids].float()) and torch.equal(I8.dequantised_queries(ivf8, q), q16.float())
        for k, ex in ((5, None), (100, None), (7, extra)):
            got_s, got_r, _ = I8.scan8(ivf8, q, probes, k, ex)
            if metric == "cosine":                                           # (normalised rows are no e4m3 values: only the form is checked)
                assert got_s.shape == (6, k) and bool((got_s[:, 1:] <= got_s[:, :-1]).all()) and bool((got_r[4] == -1).all())
                continue
            bias = ivf8.bias if ex is None else ivf8.bias + ex[ids]
            want_s, want_r = I.scan(index.vectors[ids], ids, bias, ivf8.list_offsets, q16, probes, k, metric_alpha(metric))
            want_s = (want_s - (q16.double() ** 2).sum(dim=1, keepdim=True)).clamp_max(0.0)
            assert torch.equal(got_r, want_r) and torch.equal(got_s, want_s), (metric, k)
            assert int(ivf8.ids[80]) not in got_r.tolist()[0] and 11 not in (got_r.tolist()[0] if ex is not None else [])
