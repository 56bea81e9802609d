"""Four-bit search, host side (no GPU): include/coati_search4.h parses against coati_hip.h to exactly its three entries and the
library exports them, the entries refuse bad arguments before any device call, the plain-torch quantiser keeps the storage rule byte
for byte on hand-made rows, Fp4Index refuses what it must, saves and loads on the CPU and does not search there, and the float64
oracle of stage 1 keeps its recall on a clustered library."""
import ctypes
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import search4_util as U, search8_util as U8, search_util  # noqa: E402
from tests.search_util import ints as _ints  # noqa: E402

NAMES = ["coati_quant_rows_fp4", "coati_search4_slices", "coati_search4_topk"]


# ---- 1. the nineteenth header ----------------------------------------------------------------------------------------------------------
def test_search4_header_parses_into_a_table_of_its_own():
    from coati_amd import _abi, _lib, build
    assert sorted(_lib.SEARCH4_PROTOTYPES) == NAMES
    for other in (_lib.PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.SEARCH_PROTOTYPES, _lib.GRAMMAR_PROTOTYPES, _lib.SCREEN_PROTOTYPES,
                  _lib.GUIDE_PROTOTYPES, _lib.LN_XHAT_PROTOTYPES, _lib.GP_PROTOTYPES, _lib.ACQ_PROTOTYPES, _lib.CLUSTER_PROTOTYPES,
                  _lib.IVF_PROTOTYPES, _lib.RADIUS_PROTOTYPES, _lib.GNN_OPS_PROTOTYPES, _lib.SEARCH8_PROTOTYPES, _lib.IVF8_PROTOTYPES,
                  _lib.IVF_RADIUS_PROTOTYPES, _lib.PQ_PROTOTYPES, _lib.IVFPQ_PROTOTYPES):
        assert not set(_lib.SEARCH4_PROTOTYPES) & set(other)
    assert not set(NAMES) & set(_lib.exported_symbols())
    Ci, P, L, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert _lib.SEARCH4_PROTOTYPES["coati_quant_rows_fp4"] == (Ci, [P, L, Ci, P, P, P])
    assert _lib.SEARCH4_PROTOTYPES["coati_search4_topk"] == (Ci, [P, P, L, Ci, P, P, P, Ci, Ci, F, Ci, P, P, P, P, P])
    assert _lib.SEARCH4_PROTOTYPES["coati_search4_slices"] == (Ci, [L, Ci, Ci])
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.SEARCH4_HEADER) as f:
        text = f.read()
    again = _abi.parse(text, guard="COATI_SEARCH4_H", name="coati_search4.h", base=base)
    assert again.prototypes == _lib.SEARCH4_PROTOTYPES and again.version == _lib.ABI_VERSION and not again.experimental
    assert "search4.hip" in build.HIP_UNITS and build.SEARCH4_HEADER in build._sources()
    assert '#include "coati_hip.h"' in text


def test_library_exports_the_search4_entries():
    from coati_amd import _lib
    l = _lib.lib()
    for name, (restype, argtypes) in _lib.SEARCH4_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_entries_refuse_bad_arguments_with_a_code():
    """decided on the host before any device call: the pointers are host buffers that a refusal never looks at"""
    from coati_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def quant(x=p, n=10, E=64, codes=p, scales=p):
        return l.coati_quant_rows_fp4(x, n, E, codes, scales, None), l.coati_last_error().decode()

    def topk(codes=p, scales=p, N=1000, E4=128, bias=p, q=p, qscale=p, Q=4, k=10, S=2, part=p, out=p):
        return l.coati_search4_topk(codes, scales, N, E4, bias, q, qscale, Q, k, 1.0, S, part, part, out, out, None), l.coati_last_error().decode()

    for kw in (dict(x=None), dict(codes=None), dict(scales=None), dict(n=0), dict(n=2 ** 31), dict(E=48), dict(E=0), dict(E=544)):
        rc, msg = quant(**kw)
        assert rc < 0 and "quant_rows_fp4" in msg, kw
    for kw in (dict(codes=None), dict(scales=None), dict(bias=None), dict(q=None), dict(qscale=None), dict(part=None), dict(out=None),
               dict(N=0), dict(N=2 ** 31), dict(E4=0), dict(E4=32), dict(E4=64), dict(E4=96), dict(E4=160), dict(E4=320), dict(E4=640),
               dict(Q=0), dict(k=0), dict(k=129), dict(S=0), dict(S=3073), dict(k=128, S=241)):
        rc, msg = topk(**kw)
        assert rc < 0 and "search4_topk" in msg, kw
    assert l.coati_search4_slices(0, 1, 1) < 0 and l.coati_search4_slices(2 ** 31, 1, 1) < 0 and l.coati_search4_slices(10, 1, 129) < 0
    assert l.coati_search4_slices(10, 1, 0) < 0 and l.coati_search4_slices(10, 0, 1) < 0 and "search4_slices" in l.coati_last_error().decode()


def test_default_slices_equal_their_restated_arithmetic():
    from coati_amd import _lib
    l = _lib.lib()
    for N in (1, 63, 64, 65, 70001, 4 * 2 ** 20, 2 ** 31 - 1):
        for Q in (1, 16, 64, 65, 1024, 100000):
            for k in (1, 10, 40, 128):
                tiles = (Q + 63) // 64
                want = max(1, min((512 + tiles - 1) // tiles, (N + 63) // 64, 30720 // k))
                S = l.coati_search4_slices(N, Q, k)
                assert S == want and 1 <= S and S * k <= 30720 and (S == 1 or (S - 1) * 64 < N), (N, Q, k, S)
                assert S == l.coati_search8_slices(N, Q, k)


# ---- 2. the storage rule in plain torch ---------------------------------------------------------------------------------------------------
def test_block_exponents_step_where_the_rule_says():
    from coati_amd import fp4_index as F
    am = torch.tensor([0.0, 6.0, 6.03125, 5.96875, 3.0, 3.015625, 6 * 2.0 ** -9, 6.03125 * 2.0 ** 5, 2.0 ** -133, 3.3895e38, 1.0, 0.75, 0.7539])
    assert F.block_exponents(am).tolist() == [0, 0, 1, 0, -1, 0, -9, 6, -126, 126, -2, -3, -2]
    assert F.block_exponents(am).dtype == torch.int32


@pytest.mark.parametrize("E", [32, 96, 128, 480, 512])
def test_quantise_rows_keeps_the_storage_rule(E):
    from coati_amd import fp4_index as F
    n = 600
    x = U.quantiser_rows(n, E, 3 + E)
    E4 = 128 * ((E + 127) // 128)
    codes, scales = F.quantise_rows(x)
    assert codes.dtype == torch.uint8 and codes.shape == (n, E4 // 2) and scales.dtype == torch.uint8 and scales.shape == (n, E4 // 32)
    assert bool((scales >= 1).all() and (scales <= 253).all())
    assert bool((codes[:, E // 2:] == 0).all()) and bool((scales[:, E // 32:] == 127).all())              # the pad: nibbles 0, scale 127
    xf = torch.nn.functional.pad(x.float(), (0, E4 - E))
    amax = xf.reshape(n, -1, 32).abs().amax(dim=2).double()
    two_j = 2.0 ** (scales.double() - 127)
    nz = amax > 0
    assert bool((amax[nz] <= 6 * two_j[nz]).all() and (amax[nz] > 3 * two_j[nz]).all())                   # the SMALLEST such j
    assert bool((scales[~nz] == 127).all())
    x_hat = F.dequantise(codes, scales)
    assert x_hat.dtype == torch.float32 and x_hat.shape == (n, E4)
    # the error is at most half the local step times the block scale: steps 0.5 below 2, 1 from 2 to 4, 2 from 4 to 6
    y = (xf.reshape(n, -1, 32).double() / two_j[:, :, None]).abs()
    half = torch.where(y <= 2, 0.25, torch.where(y <= 4, 0.5, 1.0)) * two_j[:, :, None]
    assert bool(((x_hat.reshape(n, -1, 32).double() - xf.reshape(n, -1, 32).double()).abs() <= half).all())
    # zeros keep their sign
    nib = torch.stack([codes & 15, codes >> 4], dim=2).reshape(n, E4)[:, :E]
    zero, negz = x.float() == 0, torch.signbit(x.float())
    assert bool((nib[zero & ~negz] == 0).all()) and bool((nib[zero & negz] == 8).all()) and int((zero & negz).sum()) > E
    # the hand-made rows, literally (special i is row n - 1 - i)
    two = E >= 64
    assert nib[n - 1, :32].tolist() == [0] * 32 and int(scales[n - 1, 0]) == 127
    if two:
        assert nib[n - 1, 32:64].tolist() == [7] * 32 and int(scales[n - 1, 1]) == 136 and codes[n - 1, 16:32].tolist() == [0x77] * 16
    for i, j in enumerate((-9, 0, 5)):
        at, above = n - 2 - 2 * i, n - 3 - 2 * i
        assert float(x[at, 16]) == -6.0 * 2.0 ** j and float(x[above, 16]) == 6.03125 * 2.0 ** j
        assert int(scales[at, 0]) == 127 + j and nib[at, :32].tolist() == [1] * 16 + [15] + [1] * 15
        assert int(scales[above, 0]) == 128 + j and nib[above, :32].tolist() == [0] * 16 + [5] + [0] * 15     # 0.25 ties to 0, 3.0156 -> 3
        assert codes[at, 7:10].tolist() == [0x11, 0x1F, 0x11]                        # element 16 is byte 8's LOW nibble
    mid = n - 8
    assert x[mid, :16].float().tolist() == U.MIDPOINTS and int(scales[mid, 0]) == 127
    assert nib[mid, :16].tolist() == U.MIDPOINT_NIBBLES == [7, 0, 2, 2, 4, 4, 6, 6, 8, 10, 10, 12, 12, 14, 14, 8]
    assert codes[mid, :8].tolist() == [0x07, 0x22, 0x44, 0x66, 0xA8, 0xCA, 0xEC, 0x8E]          # low nibble first
    steps = n - 9
    assert nib[steps, :16].tolist() == U.STEP_NIBBLES == [2, 4, 5, 6, 7, 10, 12, 13, 14, 15, 1, 3, 9, 11, 0, 8] and int(scales[steps, 0]) == 127
    if two:
        assert nib[steps, 32:48].tolist() == U.STEP_NIBBLES and int(scales[steps, 1]) == 107                 # 2^-20 below its neighbour
        assert torch.equal(x_hat[steps, :64], x[steps, :64].float())
    assert nib[n - 11].tolist() == [8] * E and scales[n - 11].tolist() == [127] * (E4 // 32)


def test_scaled_integers_are_stored_exactly():
    from coati_amd import fp4_index as F
    x = U.scaled_ints((500, 96), 5)
    codes, scales = F.quantise_rows(x.to(torch.bfloat16))
    assert torch.equal(F.dequantise(codes, scales)[:, :96], x) and bool((F.dequantise(codes, scales)[:, 96:] == 0).all())
    assert int(scales[:, :3].unique().numel()) >= 4 and bool((scales[:, :3].amax(dim=1) > scales[:, :3].amin(dim=1)).any())
    x = _ints((500, 256), 6)
    codes, scales = F.quantise_rows(x.to(torch.bfloat16))
    assert torch.equal(F.dequantise(codes, scales), x)
    for kind in ("ascending", "descending", "constant", "blocks"):
        x, q = U.quat_library(kind)
        codes, scales = F.quantise_rows(x.to(torch.bfloat16))
        assert torch.equal(F.dequantise(codes, scales)[:, :32], x)
        if kind == "ascending":
            assert torch.equal((x.double() @ q.double().T)[:, 0], torch.arange(4096).double())


# ---- 3. the index on the CPU -------------------------------------------------------------------------------------------------------------
def _cpu_index(N=300, E=40, metric="l2", seed=1):
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(E, metric=metric, device="cpu")
    index.add(torch.randn(N, E, generator=torch.Generator().manual_seed(seed)))
    return index


def test_build_is_a_snapshot_with_the_stage_1_bias():
    from coati_amd import fp4_index as F
    index = _cpu_index()
    index.remove([5])
    fp4 = index.fp4()
    assert isinstance(fp4, F.Fp4Index) and len(fp4) == 300 and fp4.keep_rows and fp4.metric == "l2" and fp4.dim == 40
    assert fp4.dim_padded == 64 and fp4.dim_stored == 128 and fp4.bytes_per_row() == 128 // 2 + 128 // 32 + 4 == 72
    codes, scales = F.quantise_rows(index.vectors)
    assert torch.equal(fp4.codes, codes) and torch.equal(fp4.scales, scales) and fp4.codes.dtype == fp4.scales.dtype == torch.uint8
    assert fp4.codes.shape == (300, 64) and fp4.scales.shape == (300, 4)
    want = -(fp4.dequantised().double() ** 2).sum(dim=1).float()
    want[5] = float("-inf")
    assert torch.equal(fp4.bias, want) and fp4.dequantised().dtype == torch.float32 and fp4.dequantised().shape == (300, 128)
    assert fp4._rows16.data_ptr() == index.vectors.data_ptr()                    # a view, not a copy
    index.add(torch.randn(10, 40))
    index.remove([7])
    assert len(fp4) == 300 and float(fp4.bias[7]) > float("-inf")                 # neither is seen
    fp4.remove([7, 8])
    assert float(fp4.bias[8]) == float("-inf") and float(fp4._bias16[8]) == float("-inf") and float(index.bias[8]) > float("-inf")
    with pytest.raises(IndexError):
        fp4.remove([300])
    bare = F.Fp4Index.build(_cpu_index(metric="cosine"), keep_rows=False)
    assert not bare.keep_rows and bare._rows16 is None and bool((bare.bias == 0).all())
    wide = _cpu_index(N=20, E=256, metric="dot")
    assert wide.fp4().bytes_per_row() == 140 and _cpu_index(N=20, E=500).fp4().bytes_per_row() == 276
    with pytest.raises(ValueError, match="512"):
        _cpu_index(N=20, E=544).fp4()


def test_search_refuses_bad_arguments_and_the_cpu():
    index = _cpu_index()
    fp4, bare = index.fp4(), index.fp4(keep_rows=False)
    q = torch.randn(3, 40)
    for kw in (dict(k=0), dict(k=129), dict(k=10, oversample=0), dict(k=10, bias=torch.zeros(299)), dict(k=10, bias=torch.zeros(300, dtype=torch.float64)),
               dict(k=10, bias=[0.0] * 300), dict(k=10, slices=0), dict(k=10, slices=30720 // 80 + 1), dict(k=10, rescore=False, slices=3073)):
        with pytest.raises(ValueError):
            fp4.search(q, **kw)
    with pytest.raises(ValueError, match="keep_rows"):
        bare.search(q, 10, rescore=True)
    with pytest.raises(ValueError):
        fp4.search(torch.randn(3, 41), 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fp4.search(q, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bare.search(q, 10)
    s, r = fp4.search(torch.zeros(0, 40), 10)
    assert s.shape == r.shape == (0, 10)


@pytest.mark.parametrize("keep_rows", [True, False])
def test_save_and_load_on_the_cpu(tmp_path, keep_rows):
    from coati_amd import fp4_index as F
    fp4 = _cpu_index().fp4(keep_rows=keep_rows)
    fp4.remove([3])
    path = str(tmp_path / "fp4.pt")
    fp4.save(path)
    assert set(torch.load(path)) == {"dim", "dim_padded", "metric", "bias"} | ({"rows16", "bias16"} if keep_rows else {"codes", "scales"})
    again = F.Fp4Index.load(path, device="cpu")
    assert len(again) == 300 and again.keep_rows == keep_rows and again.metric == "l2" and again.dim == 40 and again.dim_padded == 64
    assert torch.equal(again.codes, fp4.codes) and torch.equal(again.scales, fp4.scales) and torch.equal(again.bias, fp4.bias)
    assert float(again.bias[3]) == float("-inf")
    if keep_rows:
        assert torch.equal(again._rows16, fp4._rows16) and torch.equal(again._bias16, fp4._bias16)
        assert float(again._bias16[3]) == float("-inf")


# ---- 4. signatures -----------------------------------------------------------------------------------------------------------------------
def test_signatures():
    from coati.generative import build_fp4_index as aliased
    from coati_amd.fp4_index import Fp4Index
    from coati_amd.generative import build_fp4_index, build_index
    from coati_amd.search import EmbeddingIndex
    assert aliased is build_fp4_index

    def spec(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert spec(Fp4Index.search) == [("self", E), ("queries", E), ("k", E), ("oversample", 8), ("rescore", None), ("slices", None), ("bias", None)]
    assert spec(Fp4Index.build) == [("index", E), ("keep_rows", True)]
    assert spec(EmbeddingIndex.fp4) == [("self", E), ("keep_rows", True)]
    assert spec(build_fp4_index) == [("smiles", E), ("encoder", E), ("tokenizer", E), ("batch_size", 1024), ("metric", "cosine"),
                                     ("canon_smiles", None), ("keep_rows", True)]
    for name in ("codes", "scales", "bias"):
        assert isinstance(getattr(Fp4Index, name), property)
    for name in ("remove", "dequantised", "bytes_per_row", "save", "load", "__len__"):
        assert callable(getattr(Fp4Index, name))
    assert spec(build_index)[-1] == ("list_dtype", "bf16")
    with pytest.raises(ValueError, match="fp4") as e:
        build_index([], None, None, nlist=4, list_dtype="fp4")
    assert '"pq"' in str(e.value)


def test_stage_1_oracle_on_exact_data_is_the_bf16_oracle():
    """the float64 restatement used on the GPU side, checked where it must agree with tests/search_util.py: data that e2m1 with block
    scales holds exactly against queries that e4m3 holds exactly"""
    from coati_amd.search import EmbeddingIndex
    for metric in ("dot", "l2"):
        index = EmbeddingIndex(96, metric=metric, device="cpu")
        index.add(U.scaled_ints((200, 96), 2))
        q = _ints((5, 96), 3, -15, 15)
        ws, wr, _ = search_util.index_search(index, q, 9)
        s, r, _ = U.stage1_search(index.fp4(), q, 9)
        assert torch.equal(s, ws) and torch.equal(r, wr)


# ---- 5. recall of the storage rule, from the float64 oracles -------------------------------------------------------------------------------
def recall_figures(N=20000, E=256, seed=285, Q=64, k=10):
    """(recall@k of stage 1 alone, {oversample: recall@k of two stages}) of the float64 oracles on the clustered library"""
    from coati_amd.search import EmbeddingIndex
    draw = U8.clustered(N, E, seed)
    index = EmbeddingIndex(E, metric="cosine", device="cpu")
    index.add(draw(N))
    q = draw(Q)
    _, exact, _ = search_util.index_search(index, q, k)
    full, _ = U.stage1_scores(index.fp4(keep_rows=False), q)
    rank = U.stage1_ranks(full, exact)                       # two stages return an exact-top-k row iff stage 1 ranks it below R
    return float((rank < k).float().mean()), {over: float((rank < min(over * k, 128)).float().mean()) for over in (2, 4, 8)}


def test_recall_floors_of_the_float64_oracle():
    """Measured with this seed (clustered(20000, 256, 285), cosine, 64 queries of the same law, k = 10): recall@10 of stage 1 alone
    0.5500, of two stages at oversample 2 / 4 / 8 0.7859 / 0.9578 / 1.0000.  The floors are those values minus 2 points for
    seed-to-seed spread, as test_recall_of_trained_code_books takes them."""
    stage1, two = recall_figures()
    print(f"search4 recall@10, float64 oracle: stage 1 alone {stage1:.4f}, two stages at oversample 2 / 4 / 8: "
          f"{two[2]:.4f} / {two[4]:.4f} / {two[8]:.4f}")
    assert stage1 >= 0.5500 - 0.02 and two[2] >= 0.7859 - 0.02 and two[4] >= 0.9578 - 0.02 and two[8] >= 1.0 - 0.02
    assert stage1 <= two[2] <= two[4] <= two[8] <= 1.0
