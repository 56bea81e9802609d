"""Quantised search, host side (no GPU): include/coati_search8.h parses against coati_hip.h to exactly its four entries and the
library exports them, the entries refuse bad arguments before any device call, the plain-torch quantiser keeps the storage rule's
properties, Fp8Index refuses what it must, saves and loads on the CPU, and does not search there."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import search8_util as U  # noqa: E402
from tests.search_util import ints as _ints  # noqa: E402

NAMES = ["coati_quant_rows_fp8", "coati_search8_slices", "coati_search8_topk", "coati_search_rescore"]


# ---- 1. the fourteenth header --------------------------------------------------------------------------------------------------------
def test_search8_header_parses_into_a_table_of_its_own():
    from coati_amd import _abi, _lib, build
    assert sorted(_lib.SEARCH8_PROTOTYPES) == NAMES
    for other in (_lib.PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.SEARCH_PROTOTYPES, _lib.GRAMMAR_PROTOTYPES, _lib.SCREEN_PROTOTYPES,
                  _lib.GUIDE_PROTOTYPES, _lib.LN_XHAT_PROTOTYPES, _lib.GP_PROTOTYPES, _lib.ACQ_PROTOTYPES, _lib.CLUSTER_PROTOTYPES,
                  _lib.IVF_PROTOTYPES, _lib.RADIUS_PROTOTYPES, _lib.GNN_OPS_PROTOTYPES):
        assert not set(_lib.SEARCH8_PROTOTYPES) & set(other)
    assert not set(NAMES) & set(_lib.exported_symbols())
    Ci, P, L, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert _lib.SEARCH8_PROTOTYPES["coati_quant_rows_fp8"] == (Ci, [P, L, Ci, P, P, P])
    assert _lib.SEARCH8_PROTOTYPES["coati_search8_topk"] == (Ci, [P, P, L, Ci, P, P, P, Ci, Ci, F, Ci, P, P, P, P, P])
    assert _lib.SEARCH8_PROTOTYPES["coati_search_rescore"] == (Ci, [P, L, Ci, P, P, Ci, P, Ci, Ci, F, P, P, P])
    assert _lib.SEARCH8_PROTOTYPES["coati_search8_slices"] == (Ci, [L, Ci, Ci])
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.SEARCH8_HEADER) as f:
        text = f.read()
    again = _abi.parse(text, guard="COATI_SEARCH8_H", name="coati_search8.h", base=base)
    assert again.prototypes == _lib.SEARCH8_PROTOTYPES and again.version == _lib.ABI_VERSION and not again.experimental
    assert "search8.hip" in build.HIP_UNITS and build.SEARCH8_HEADER in build._sources()
    assert '#include "coati_hip.h"' in text


def test_library_exports_the_search8_entries():
    from coati_amd import _lib
    l = _lib.lib()
    for name, (restype, argtypes) in _lib.SEARCH8_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_entries_refuse_bad_arguments_with_a_code():
    """decided on the host before any device call: the pointers are host buffers that a refusal never looks at"""
    from coati_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def quant(x=p, n=10, E=64, out=p, scale=p):
        return l.coati_quant_rows_fp8(x, n, E, out, scale, None), l.coati_last_error().decode()

    def topk(lib=p, scale=p, N=1000, E=64, bias=p, q=p, qscale=p, Q=4, k=10, S=2, part=p, out=p):
        return l.coati_search8_topk(lib, scale, N, E, bias, q, qscale, Q, k, 1.0, S, part, part, out, out, None), l.coati_last_error().decode()

    def resc(lib=p, N=1000, E=64, q=p, Q=4, cand=p, R=40, k=10, out=p):
        return l.coati_search_rescore(lib, N, E, None, q, Q, cand, R, k, 1.0, out, out, None), l.coati_last_error().decode()

    for kw in (dict(x=None), dict(out=None), dict(scale=None), dict(n=0), dict(n=2 ** 31), dict(E=48), dict(E=0), dict(E=544)):
        rc, msg = quant(**kw)
        assert rc < 0 and "quant_rows_fp8" in msg, kw
    for kw in (dict(lib=None), dict(scale=None), dict(bias=None), dict(q=None), dict(qscale=None), dict(part=None), dict(out=None), dict(N=0),
               dict(N=2 ** 31), dict(E=16), dict(E=544), dict(E=100), dict(Q=0), dict(k=0), dict(k=129), dict(S=0), dict(S=3073)):
        rc, msg = topk(**kw)
        assert rc < 0 and "search8_topk" in msg, kw
    for kw in (dict(lib=None), dict(q=None), dict(cand=None), dict(out=None), dict(N=0), dict(E=16), dict(E=544), dict(Q=0), dict(R=0),
               dict(R=129), dict(k=0), dict(k=129)):
        rc, msg = resc(**kw)
        assert rc < 0 and "search_rescore" in msg, kw
    assert l.coati_search8_slices(0, 1, 1) < 0 and l.coati_search8_slices(10, 1, 129) < 0 and l.coati_search8_slices(10, 0, 1) < 0


def test_default_slices_keep_their_bounds():
    from coati_amd import _lib
    l = _lib.lib()
    for N in (1, 63, 64, 65, 70001, 4 * 2 ** 20, 2 ** 31 - 1):
        for Q in (1, 16, 64, 65, 1024, 100000):
            for k in (1, 10, 40, 128):
                S = l.coati_search8_slices(N, Q, k)
                assert 1 <= S and S * k <= 30720 and (S == 1 or (S - 1) * 64 < N), (N, Q, k, S)
                assert S == l.coati_search_slices(N, Q, k)


# ---- 2. the storage rule in plain torch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [32, 96, 512])
def test_quantise_rows_keeps_the_storage_rule(E):
    from coati_amd import fp8_index as F
    x = U.quantiser_rows(1000, E, 3 + E)
    b, s = F.quantise_rows(x)
    assert b.dtype == torch.uint8 and b.shape == x.shape and s.dtype == torch.float32 and s.shape == (1000,)
    mant, _ = torch.frexp(s)
    assert bool((mant == 0.5).all())                                              # a power of two
    amax = x.float().abs().amax(dim=1)
    ratio = amax.double() / s.double()
    nz = amax > 0
    assert int(nz.sum()) >= 990 and bool((ratio[nz] > 224).all() and (ratio[nz] <= 448).all())
    assert bool((s[~nz] == 1).all()) and int((~nz).sum()) >= 2
    x_hat = F.dequantise(b, s)
    assert bool(torch.isfinite(x_hat).all())                                      # nothing saturated into e4m3fn's NaN
    assert bool(((x_hat - x.float()).abs() <= 16 * s[:, None]).all())             # half an ulp of e4m3's top binade (256 .. 448: 32) at most
    # zeros keep their sign: a row of +0, a row of -0, and -0 among other values
    zero, negz = x.float() == 0, torch.signbit(x.float())
    assert bool((b[zero & ~negz] == 0x00).all()) and bool((b[zero & negz] == 0x80).all()) and int((zero & negz).sum()) > E
    # the edges: 448 * 2^j takes scale 2^j and the byte of 448, the next bf16 value the next scale
    # (quantiser_rows puts its hand-made rows last: zeros, then the pairs, then the small entries)
    for i, j in enumerate((-9, 0, 5)):
        at, above = 1000 - 2 - 2 * i, 1000 - 3 - 2 * i
        assert float(x[at, E // 2]) == -448.0 * 2.0 ** j and float(x[above, E // 2]) == 450.0 * 2.0 ** j
        assert float(s[at]) == 2.0 ** j and int(b[at, E // 2]) == 0xFE and float(s[above]) == 2.0 ** (j + 1)
    # the row 300, 2^-7, 3 * 2^-9, -2^-9, 2^-10, -2^-11, 5 * 2^-9, 2^-6, -7 * 2^-9: subnormals in steps of 2^-9, ties to even, signed zeros
    small = 1000 - 8
    assert float(x[small, 0]) == 300.0 and float(s[small]) == 1.0
    assert b[small, 1:9].tolist() == [0x04, 0x03, 0x81, 0x00, 0x80, 0x05, 0x08, 0x87]


def test_small_integers_are_stored_exactly():
    from coati_amd import fp8_index as F
    for lo, hi in ((-4, 4), (-15, 15)):
        x = _ints((500, 96), 5, lo, hi)
        b, s = F.quantise_rows(x.to(torch.bfloat16))
        assert torch.equal(F.dequantise(b, s), x)
    x, _ = U.hex_library("ascending")
    b, s = F.quantise_rows(x.to(torch.bfloat16))
    assert torch.equal(F.dequantise(b, s), x) and sorted(set(s.tolist())) == [2.0 ** -8, 2.0 ** -7, 2.0 ** -6, 2.0 ** -5, 2.0 ** -4, 1.0]


# ---- 3. the index on the CPU -------------------------------------------------------------------------------------------------------------
def _cpu_index(N=300, E=40, metric="l2", seed=1):
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(E, metric=metric, device="cpu")
    index.add(torch.randn(N, E, generator=torch.Generator().manual_seed(seed)))
    return index


def test_build_is_a_snapshot_with_the_stage_1_bias():
    from coati_amd import fp8_index as F
    index = _cpu_index()
    index.remove([5])
    fp8 = index.fp8()
    assert isinstance(fp8, F.Fp8Index) and len(fp8) == 300 and fp8.keep_rows and fp8.metric == "l2" and fp8.dim == 40 and fp8.dim_padded == 64
    b, s = F.quantise_rows(index.vectors)
    assert torch.equal(fp8.vectors8, b) and torch.equal(fp8.scales, s) and fp8.vectors8.dtype == torch.uint8
    want = -(fp8.dequantised().double() ** 2).sum(dim=1).float()
    want[5] = float("-inf")
    assert torch.equal(fp8.bias, want) and fp8.dequantised().dtype == torch.float32
    assert fp8._rows16.data_ptr() == index.vectors.data_ptr()                    # a view, not a copy
    index.add(torch.randn(10, 40))
    index.remove([7])
    assert len(fp8) == 300 and float(fp8.bias[7]) > float("-inf")                 # neither is seen
    fp8.remove([7, 8])
    assert float(fp8.bias[8]) == float("-inf") and float(fp8._bias16[8]) == float("-inf") and float(index.bias[8]) > float("-inf")
    with pytest.raises(IndexError):
        fp8.remove([300])
    bare = F.Fp8Index.build(_cpu_index(metric="cosine"), keep_rows=False)
    assert not bare.keep_rows and bare._rows16 is None and bool((bare.bias == 0).all())


def test_search_refuses_bad_arguments_and_the_cpu():
    index = _cpu_index()
    fp8, bare = index.fp8(), index.fp8(keep_rows=False)
    q = torch.randn(3, 40)
    for kw in (dict(k=0), dict(k=129), dict(k=10, oversample=0), dict(k=10, bias=torch.zeros(299)), dict(k=10, bias=torch.zeros(300, dtype=torch.float64)),
               dict(k=10, bias=[0.0] * 300), dict(k=10, slices=0), dict(k=10, slices=30720 // 40 + 1), dict(k=10, rescore=False, slices=3073)):
        with pytest.raises(ValueError):
            fp8.search(q, **kw)
    with pytest.raises(ValueError, match="keep_rows"):
        bare.search(q, 10, rescore=True)
    with pytest.raises(ValueError):
        fp8.search(torch.randn(3, 41), 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fp8.search(q, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bare.search(q, 10)
    s, r = fp8.search(torch.zeros(0, 40), 10)
    assert s.shape == r.shape == (0, 10)


@pytest.mark.parametrize("keep_rows", [True, False])
def test_save_and_load_on_the_cpu(tmp_path, keep_rows):
    from coati_amd import fp8_index as F
    fp8 = _cpu_index().fp8(keep_rows=keep_rows)
    fp8.remove([3])
    path = str(tmp_path / "fp8.pt")
    fp8.save(path)
    assert set(torch.load(path)) == {"dim", "dim_padded", "metric", "bias"} | ({"rows16", "bias16"} if keep_rows else {"vectors8", "scales"})
    again = F.Fp8Index.load(path, device="cpu")
    assert len(again) == 300 and again.keep_rows == keep_rows and again.metric == "l2" and again.dim == 40 and again.dim_padded == 64
    assert torch.equal(again.vectors8, fp8.vectors8) and torch.equal(again.scales, fp8.scales) and torch.equal(again.bias, fp8.bias)
    if keep_rows:
        assert torch.equal(again._rows16, fp8._rows16) and torch.equal(again._bias16, fp8._bias16)
        assert float(again._bias16[3]) == float("-inf")


def test_build_index_takes_one_kind_of_index():
    from coati_amd.generative import build_index
    with pytest.raises(ValueError, match="fp8"):
        build_index([], None, None, nlist=4, fp8=True)


def test_stage_1_oracle_on_exact_data_is_the_bf16_oracle():
    """the float64 restatement used on the GPU side, checked where it must agree with tests/search_util.py: integers of magnitude <= 15"""
    from tests import search_util
    from coati_amd.search import EmbeddingIndex
    for metric in ("dot", "l2"):
        index = EmbeddingIndex(64, metric=metric, device="cpu")
        index.add(_ints((200, 64), 2, -15, 15))
        q = _ints((5, 64), 3, -15, 15)
        ws, wr, _ = search_util.index_search(index, q, 9)
        s, r, _ = U.stage1_search(index.fp8(), q, 9)
        assert torch.equal(s, ws) and torch.equal(r, wr)
