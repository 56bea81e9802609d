"""IVF-PQ search, host side (no GPU): include/coati_ivfpq.h parses against coati_hip.h and the library exports what it declares,
coati_ivfpq_scan refuses bad arguments with a code before any device call, coati_ivfpq_k_max is the restated LDS arithmetic, an
IvfPqIndex put together through the constructor keeps the storage rule byte for byte, the Python layer refuses what it must, and the
signatures of the new and of the pinned entry points are what the issue names."""
import ctypes
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import ivfpq_util as U, pq_util, search_util as SU  # noqa: E402

NEG_INF = float("-inf")
SIZES = [5, 0, 70, 1, 130]
N, DIM = sum(SIZES) + 2, 40


def _assign(sizes=SIZES, left_out=2, seed=3):
    a = torch.cat([torch.full((n,), l) for l, n in enumerate(sizes)] + [torch.full((left_out,), -1)])
    return a[torch.randperm(a.shape[0], generator=torch.Generator().manual_seed(seed))]


def _by_hand(metric="l2", keep_rows=True, seed=1):
    """integer rows and centres of magnitude <= 15 (the residuals up to 30: bf16 values), integer code books"""
    x = SU.ints((N, DIM), seed, -15, 15)
    centres = SU.ints((len(SIZES), DIM), seed + 1, -15, 15)
    cb = pq_util.int_codebooks(64 // 8, seed + 2)
    return U.by_hand(x, _assign(), centres, metric, keep_rows=keep_rows, codebooks=cb) + (cb,)


# ---- 1. the eighteenth header ---------------------------------------------------------------------------------------------------------
def test_ivfpq_header_parses_into_a_table_of_its_own():
    from coati_amd import _abi, _lib, build
    assert sorted(_lib.IVFPQ_PROTOTYPES) == ["coati_ivfpq_k_max", "coati_ivfpq_scan"]
    for other in (_lib.PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.SEARCH_PROTOTYPES, _lib.GRAMMAR_PROTOTYPES, _lib.SCREEN_PROTOTYPES,
                  _lib.GUIDE_PROTOTYPES, _lib.LN_XHAT_PROTOTYPES, _lib.GP_PROTOTYPES, _lib.ACQ_PROTOTYPES, _lib.CLUSTER_PROTOTYPES,
                  _lib.IVF_PROTOTYPES, _lib.RADIUS_PROTOTYPES, _lib.GNN_OPS_PROTOTYPES, _lib.SEARCH8_PROTOTYPES, _lib.IVF8_PROTOTYPES,
                  _lib.IVF_RADIUS_PROTOTYPES, _lib.PQ_PROTOTYPES):
        assert not set(_lib.IVFPQ_PROTOTYPES) & set(other)
    assert "coati_ivfpq_scan" not in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 5
    Ci, P, L, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert _lib.IVFPQ_PROTOTYPES["coati_ivfpq_scan"] == (Ci, [P, P, P, P, L, Ci, Ci, P, P, P, Ci, P, P, P, L, Ci, F, Ci, Ci, P, P, Ci, P])
    assert _lib.IVFPQ_PROTOTYPES["coati_ivfpq_k_max"] == (Ci, [Ci])
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.IVFPQ_HEADER) as f:
        again = _abi.parse(f.read(), guard="COATI_IVFPQ_H", name="coati_ivfpq.h", base=base)
    assert again.prototypes == _lib.IVFPQ_PROTOTYPES and again.version == 5 and not again.experimental
    assert "ivfpq.hip" in build.HIP_UNITS and build.IVFPQ_HEADER in build._sources()


def test_library_exports_the_ivfpq_entries():
    from coati_amd import _lib
    l = _lib.lib()
    assert l.coati_abi_version() == 5
    for name, (restype, argtypes) in _lib.IVFPQ_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


# ---- 2. refusals ------------------------------------------------------------------------------------------------------------------------
def test_ivfpq_scan_refuses_bad_arguments_with_a_code():
    """decided on the host before any device call: the pointers are host buffers that a refusal never looks at"""
    from coati_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def call(codes=p, ids=p, bias=p, list_off=p, M=1000, E=64, L=8, centres=p, codebook=p, q=p, Q=4, pair_q=p, pair_off=p, item_off=p, P=16,
             k=10, alpha=1.0, seg_rows=128, segs=2, part_score=p, part_row=p, blocks=0):
        rc = l.coati_ivfpq_scan(codes, ids, bias, list_off, M, E, L, centres, codebook, q, Q, pair_q, pair_off, item_off, P, k, alpha, seg_rows,
                                segs, part_score, part_row, blocks, None)
        return rc, l.coati_last_error().decode()

    cases = [(dict(codes=None), "codes"), (dict(ids=None), "ids"), (dict(bias=None), "bias"), (dict(list_off=None), "list_off"),
             (dict(centres=None), "centres"), (dict(codebook=None), "codebook"), (dict(q=None), "q is null"), (dict(pair_q=None), "pair_q"),
             (dict(pair_off=None), "pair_off"), (dict(item_off=None), "item_off"), (dict(part_score=None), "part_score"),
             (dict(part_row=None), "part_row"),
             (dict(E=48), "E=48"), (dict(E=288), "E=288"), (dict(E=512), "E=512"), (dict(E=0), "E=0"), (dict(M=0), "M=0"),
             (dict(M=2 ** 31), f"M={2 ** 31}"), (dict(L=0), "L=0"), (dict(L=4097), "L=4097"), (dict(Q=0), "Q=0"), (dict(P=0), "P=0"),
             (dict(P=2 ** 31), f"P={2 ** 31}"), (dict(k=0), "k=0"), (dict(k=129), "k=129"), (dict(E=256, k=65), "k=65"),
             (dict(seg_rows=0), "seg_rows=0"), (dict(seg_rows=96), "seg_rows=96"), (dict(segs=0), "segs=0"), (dict(blocks=-1), "blocks=-1")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc < 0 and "ivfpq_scan" in msg and word in msg, (kw, rc, msg)


def test_k_max_is_the_lds_arithmetic():
    """the code book (512 E bytes), 16 lists of cap = k + 128 keys of 8 bytes, 16 counts, 16 thresholds and 2 flags in 160 KiB: 128 where
    that fits, else 64"""
    from coati_amd import _lib, ivfpq
    l = _lib.lib()
    for E in range(32, 257, 32):
        want = next(k for k in (128, 64) if 512 * E + 16 * (k + 128) * 8 + 16 * 8 + 8 <= 160 * 1024)
        assert l.coati_ivfpq_k_max(E) == want == ivfpq.k_max(E), E
    assert l.coati_ivfpq_k_max(256) == 64 and l.coati_ivfpq_k_max(224) == 128
    for E in (0, 16, 48, 288, 512, -32):
        assert l.coati_ivfpq_k_max(E) < 0 and f"E={E}" in l.coati_last_error().decode(), E
        with pytest.raises(ValueError, match="coati_ivfpq_k_max"):
            ivfpq.k_max(E)


# ---- 3. the storage rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_storage_rule(metric):
    from coati_amd import pq
    ivfpq, index, cb = _by_hand(metric)
    assign = _assign()
    assert len(ivfpq) == N and ivfpq.nlist == 5 and ivfpq.keep_rows and ivfpq.dim == DIM and ivfpq.dim_padded == 64 and ivfpq.metric == metric
    assert ivfpq.sizes.tolist() == SIZES and ivfpq.list_offsets.tolist() == [0, 5, 5, 75, 76, 206]
    ids = ivfpq.ids.long()
    assert ivfpq.ids.dtype == torch.int32 and sorted(ids.tolist()) == torch.nonzero(assign >= 0).reshape(-1).tolist()
    for l in range(5):
        rows = ivfpq.list_rows(l)
        assert torch.equal(rows, torch.nonzero(assign == l).reshape(-1)) and bool((rows[1:] > rows[:-1]).all())
    # the codes are encode_rows of the residuals, byte for byte; the residuals are the float64 restatement's
    r16 = U.residuals(index.vectors, ids, ivfpq.list_offsets, ivfpq.centres16)
    assert ivfpq.codes.dtype == torch.uint8 and ivfpq.codes.shape == (206, 8)
    assert torch.equal(ivfpq.codes, pq.encode_rows(r16, cb)) and torch.equal(ivfpq.codes, pq_util.encode64(r16, cb))
    assert torch.equal(ivfpq.codebooks, cb) and ivfpq.centres16.dtype == torch.bfloat16 and ivfpq.centres16.shape == (5, 64)
    # dequantised() is the centre plus the entry
    lists = U.position_lists(ivfpq.list_offsets)
    want = ivfpq.centres16[lists].double() + pq.reconstruct(ivfpq.codes, cb).double()
    assert torch.equal(U.x_hat(ivfpq), want)
    deq = ivfpq.dequantised()
    assert deq.dtype == torch.float32 and deq.shape == (206, 64)
    if metric == "l2":                                                       # (integers: the f32 addition is exact)
        assert torch.equal(deq.double(), want)
        assert torch.equal(ivfpq.bias, -(want ** 2).sum(dim=1).float()) and not torch.equal(ivfpq.bias, index.bias[ids])
    else:
        assert float((deq.double() - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())
        assert torch.equal(ivfpq.bias, torch.zeros(206))
    assert ivfpq.bytes_per_row() == 64 // 8 + 8
    # stage 2 reads the index's rows in place
    assert ivfpq._rows16.data_ptr() == index.vectors.data_ptr() and ivfpq._bias16.data_ptr() != index.bias.data_ptr()
    assert torch.equal(ivfpq._bias16, index.bias)
    bare, _, _ = _by_hand(metric, keep_rows=False)
    assert not bare.keep_rows and bare._rows16 is None and bare._bias16 is None and torch.equal(bare.codes, ivfpq.codes)


def test_lossless_library_names_its_entries():
    """rows composed as centre + entry: the residual is the entry, exactly, and the codes name it"""
    cb = pq_util.int_codebooks(8, 5)
    entries, codes = pq_util.composed_rows(cb, N, 6)
    centres = SU.ints((5, 64), 7, -15, 15)
    assign = _assign()
    x = entries + centres[assign.clamp_min(0)]
    ivfpq, _ = U.by_hand(x, assign, centres, "l2", codebooks=cb)
    assert torch.equal(ivfpq.codes, codes[ivfpq.ids.long()]) and torch.equal(ivfpq.dequantised(), x[ivfpq.ids.long()])


def test_fitted_codebooks_are_reproducible_and_sampled():
    x = torch.randn(N, DIM, generator=torch.Generator().manual_seed(8))
    centres = torch.randn(5, DIM, generator=torch.Generator().manual_seed(9))
    a, _ = U.by_hand(x, _assign(), centres, "l2", seed=3, iters=2, sample=100)
    b, _ = U.by_hand(x, _assign(), centres, "l2", seed=3, iters=2, sample=100)
    c, _ = U.by_hand(x, _assign(), centres, "l2", seed=4, iters=2, sample=100)
    assert a.codebooks.shape == (8, 256, 8) and a.codebooks.dtype == torch.bfloat16
    assert torch.equal(a.codebooks, b.codebooks) and torch.equal(a.codes, b.codes) and not torch.equal(a.codebooks, c.codebooks)
    assert int(a.codebooks[0].float().unique(dim=0).shape[0]) <= 100          # 100 sampled rows: at most 100 distinct entries


def test_remove_hits_both_biases():
    ivfpq, index, _ = _by_hand("l2")
    left_out = torch.nonzero(_assign() < 0).reshape(-1)
    gone = [int(ivfpq.ids[0]), int(ivfpq.ids[100]), int(left_out[0])]
    ivfpq.remove(gone)
    removed = torch.nonzero(ivfpq.bias == NEG_INF).reshape(-1)
    assert sorted(ivfpq.ids[removed].tolist()) == sorted(gone[:2])
    assert sorted(torch.nonzero(ivfpq._bias16 == NEG_INF).reshape(-1).tolist()) == sorted(gone)
    assert bool((index.bias > NEG_INF).all()) and len(ivfpq) == N
    ivfpq.remove([])
    for bad in ([-1], [N], [0, 300]):
        with pytest.raises(IndexError, match=f"0 .. {N - 1}"):
            ivfpq.remove(bad)
    bare, _, _ = _by_hand("l2", keep_rows=False)
    bare.remove(gone)
    assert int((bare.bias == NEG_INF).sum()) == 2


@pytest.mark.parametrize("keep_rows", [True, False])
def test_save_load_round_trip(tmp_path, keep_rows):
    from coati_amd.ivfpq import IvfPqIndex
    ivfpq, _, _ = _by_hand("l2", keep_rows=keep_rows)
    ivfpq.remove([int(ivfpq.ids[7])])
    path = str(tmp_path / "ivfpq.pt")
    ivfpq.save(path)
    saved = torch.load(path, map_location="cpu")
    assert ("rows16" in saved) == keep_rows and "codes" in saved and "codebooks" in saved
    back = IvfPqIndex.load(path, device="cpu")
    assert back.keep_rows == keep_rows and len(back) == N and back.metric == "l2" and back.dim == DIM and back.nlist == 5
    for name in ("codes", "codebooks", "centres16", "bias", "ids", "sizes", "list_offsets", "centres"):
        assert torch.equal(getattr(back, name), getattr(ivfpq, name)), name
    if keep_rows:
        assert torch.equal(back._rows16, ivfpq._rows16) and torch.equal(back._bias16, ivfpq._bias16)


# ---- 4. the Python layer ----------------------------------------------------------------------------------------------------------------
def test_search_refuses():
    ivfpq, _, _ = _by_hand("cosine")
    bare, _, _ = _by_hand("cosine", keep_rows=False)
    q = SU.ints((3, DIM), 11, -15, 15)
    table = torch.tensor([[0, 2, -1], [4, -1, -1], [3, 4, 0]])
    for k in (0, 129):
        with pytest.raises(ValueError, match=f"k={k}"):
            ivfpq.search(q, k, probes=table)
    with pytest.raises(ValueError, match="oversample=0"):
        ivfpq.search(q, 5, oversample=0, probes=table)
    with pytest.raises(ValueError, match="keep_rows"):
        bare.search(q, 5, rescore=True, probes=table)
    for bias in (torch.zeros(N - 1), torch.zeros(N, dtype=torch.float64), [0.0] * N):
        with pytest.raises(ValueError, match="bias"):
            ivfpq.search(q, 5, probes=table, bias=bias)
    for seg_rows in (0, 32, 96, -64):
        with pytest.raises(ValueError, match="seg_rows"):
            ivfpq.search(q, 5, probes=table, seg_rows=seg_rows)
    for nprobe in (0, 129):
        with pytest.raises(ValueError, match="nprobe"):
            ivfpq.search(q, 5, nprobe=nprobe)
    # no CPU fallback, in either stage and in the coarse step
    for kw in (dict(probes=table), dict(probes=table, rescore=False), dict()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ivfpq.search(q, 5, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ivfpq.probe(q, 2)
    for rescore in (None, False):
        s, r = ivfpq.search(q[:0], 7, rescore=rescore)
        assert s.shape == (0, 7) and r.shape == (0, 7) and s.dtype == torch.float32 and r.dtype == torch.int64


def test_k_above_the_limit_of_a_256_wide_index_raises():
    """dim_padded = 256: the code book leaves room for k <= 64"""
    x = SU.ints((20, 256), 12, -15, 15)
    ivfpq, _ = U.by_hand(x, torch.arange(20) % 2, SU.ints((2, 256), 13, -15, 15), "l2", codebooks=pq_util.int_codebooks(32, 14))
    with pytest.raises(ValueError, match="k=65 outside 1 .. 64"):
        ivfpq.search(x[:1], 65, probes=torch.tensor([[0, 1]]))


def test_building_refuses():
    from coati_amd.ivf import IVFIndex
    from coati_amd.ivfpq import IvfPqIndex
    from coati_amd.search import EmbeddingIndex
    x = torch.randn(50, 40, generator=torch.Generator().manual_seed(0))
    dot = EmbeddingIndex(40, metric="dot", device="cpu")
    dot.add(x)
    with pytest.raises(ValueError, match="dot"):
        IvfPqIndex.build(dot, 4)
    with pytest.raises(ValueError, match="dot"):
        dot.ivfpq(4)
    wide = EmbeddingIndex(260, metric="l2", device="cpu")
    wide.add(torch.randn(5, 260, generator=torch.Generator().manual_seed(1)))
    with pytest.raises(ValueError, match="288 wide, above 256"):
        wide.ivfpq(2)
    with pytest.raises(ValueError, match="above 256"):
        IvfPqIndex(260, 288, "l2", 5, torch.zeros(1, 260), torch.zeros(5, 36, dtype=torch.uint8), pq_util.int_codebooks(36, 0),
                   torch.arange(5), torch.zeros(5), torch.tensor([5]), device="cpu")
    index = EmbeddingIndex(40, metric="l2", device="cpu")
    index.add(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.ivfpq(4)
    for nlist in (0, 4097):
        with pytest.raises(ValueError, match="nlist"):
            index.ivfpq(nlist, keep_rows=False)
    with pytest.raises(ValueError, match="code books"):
        IvfPqIndex(40, 64, "l2", 50, torch.zeros(1, 40), torch.zeros(50, 8, dtype=torch.uint8), torch.zeros(8, 256, 8), torch.arange(50),
                   torch.zeros(50), torch.tensor([50]), device="cpu")
    # from_ivf: the source index must be the IVFIndex's; the result is the constructor's for the same lists
    from tests import ivf_util as I
    assign = torch.arange(50) % 4
    ids, off = I.inverted(assign, 4)
    centres = torch.randn(4, 40, generator=torch.Generator().manual_seed(2))
    ivf = IVFIndex(40, 64, "l2", 50, centres, index.vectors[ids], ids, index.bias[ids], off[1:] - off[:-1], "cpu")
    a = ivf.pq(index, pq_iters=2)
    b, _ = U.by_hand(x, assign, centres, "l2", iters=2)
    assert isinstance(a, IvfPqIndex) and a.keep_rows and a._rows16.data_ptr() == index.vectors.data_ptr()
    assert torch.equal(a.ids, ivf.ids) and torch.equal(a.sizes, ivf.sizes) and not IvfPqIndex.from_ivf(ivf, pq_iters=1).keep_rows
    assert torch.equal(a.codebooks, b.codebooks) and torch.equal(a.codes, b.codes) and torch.equal(a.bias, b.bias)
    other = EmbeddingIndex(40, metric="cosine", device="cpu")
    other.add(x)
    short = EmbeddingIndex(40, metric="l2", device="cpu")
    short.add(x[:49])
    for wrong in (other, short):
        with pytest.raises(ValueError, match="source"):
            IvfPqIndex.from_ivf(ivf, wrong)


def test_build_index_keywords():
    from coati_amd.generative import build_index
    with pytest.raises(ValueError, match="nlist"):
        build_index([], None, None, list_dtype="pq")
    with pytest.raises(ValueError, match='"pq"'):
        build_index([], None, None, nlist=4, list_dtype="fp4")


# ---- 5. signatures ----------------------------------------------------------------------------------------------------------------------
def test_signatures():
    import coati.generative as G
    import coati_amd.generative as AG
    from coati_amd.ivf import IVFIndex, ListIndex
    from coati_amd.ivf8 import Ivf8Index
    from coati_amd.ivfpq import IvfPqIndex
    from coati_amd.search import EmbeddingIndex

    def names(f):
        return list(inspect.signature(f).parameters)

    def defaults(f):
        return {n: p.default for n, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}

    assert names(IvfPqIndex.build) == ["index", "nlist", "iters", "seed", "centres", "assign", "keep_rows", "pq_seed", "pq_iters", "sample", "codebooks"]
    assert defaults(IvfPqIndex.build) == dict(iters=20, seed=0, centres=None, assign=None, keep_rows=True, pq_seed=0, pq_iters=20, sample=65536,
                                              codebooks=None)
    assert names(IvfPqIndex.from_ivf)[:2] == ["ivf", "index"] and defaults(IvfPqIndex.from_ivf)["index"] is None
    assert names(IvfPqIndex.search) == names(Ivf8Index.search) == ["self", "queries", "k", "nprobe", "oversample", "rescore", "probes", "seg_rows",
                                                                   "bias", "return_probes", "blocks"]
    assert defaults(IvfPqIndex.search) == defaults(Ivf8Index.search)
    assert names(EmbeddingIndex.ivfpq) == ["self", "nlist", "iters", "seed", "centres", "keep_rows", "pq_seed", "pq_iters", "sample", "codebooks"]
    assert defaults(EmbeddingIndex.ivfpq) == dict(iters=20, seed=0, centres=None, keep_rows=True, pq_seed=0, pq_iters=20, sample=65536, codebooks=None)
    assert names(IVFIndex.pq)[:2] == ["self", "index"] and defaults(IVFIndex.pq)["index"] is None
    assert issubclass(IvfPqIndex, ListIndex)
    for name in ("probe", "plan", "remove", "sizes", "ids", "list_rows", "codes", "codebooks", "centres16", "bias", "dequantised", "bytes_per_row",
                 "save", "load", "from_ivf", "build", "__len__"):
        assert hasattr(IvfPqIndex, name), name
    # the pinned ones stay as they were
    assert names(EmbeddingIndex.ivf) == ["self", "nlist", "iters", "seed", "centres", "fp8", "keep_rows"]
    assert names(IVFIndex.build) == ["index", "nlist", "iters", "seed", "centres", "assign"]
    assert names(Ivf8Index.build) == ["index", "nlist", "iters", "seed", "centres", "assign", "keep_rows"]
    assert names(IVFIndex.fp8) == ["self", "index"]
    assert G.build_index is AG.build_index and names(AG.build_index)[-1] == "list_dtype" and defaults(AG.build_index)["list_dtype"] == "bf16"
    assert names(AG.build_pq_index) == ["smiles", "encoder", "tokenizer", "batch_size", "metric", "canon_smiles", "keep_rows", "seed", "iters"]
