"""Library clustering, host side (no GPU): include/coati_cluster.h parses against coati_hip.h and the library exports what it declares,
both entries refuse bad arguments with a code before any device call, the Python layer refuses what it must, and
Clustering.representatives against the restatement of tests/cluster_util.py."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import cluster_util as C  # noqa: E402

NAMES = ["coati_cluster_assign", "coati_cluster_chunk", "coati_cluster_items_max", "coati_cluster_sums"]


# ---- 1. the tenth header ------------------------------------------------------------------------------------------------------------
def test_cluster_header_parses_into_a_table_of_its_own():
    from coati_amd import _abi, _lib, build
    assert sorted(_lib.CLUSTER_PROTOTYPES) == NAMES
    for other in (_lib.PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.SEARCH_PROTOTYPES, _lib.GRAMMAR_PROTOTYPES, _lib.SCREEN_PROTOTYPES,
                  _lib.GUIDE_PROTOTYPES, _lib.LN_XHAT_PROTOTYPES, _lib.GP_PROTOTYPES, _lib.ACQ_PROTOTYPES):
        assert not set(_lib.CLUSTER_PROTOTYPES) & set(other)
    assert not set(NAMES) & set(_lib.exported_symbols())
    assert _lib.ABI_VERSION == 5
    I, P, L = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert _lib.CLUSTER_PROTOTYPES["coati_cluster_assign"] == (I, [P, L, I, P, P, I, P, P, P, I, P])
    assert _lib.CLUSTER_PROTOTYPES["coati_cluster_sums"] == (I, [P, L, I, P, L, P, P, I, P, L, P, I, P])
    assert _lib.CLUSTER_PROTOTYPES["coati_cluster_chunk"] == (I, [])
    assert _lib.CLUSTER_PROTOTYPES["coati_cluster_items_max"] == (L, [L, I])
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.CLUSTER_HEADER) as f:
        again = _abi.parse(f.read(), guard="COATI_CLUSTER_H", name="coati_cluster.h", base=base)
    assert again.prototypes == _lib.CLUSTER_PROTOTYPES and again.version == 5 and not again.experimental
    assert "cluster.hip" in build.HIP_UNITS and build.CLUSTER_HEADER in build._sources()


def test_library_exports_the_cluster_entries():
    from coati_amd import _lib
    l = _lib.lib()
    assert l.coati_abi_version() == 5
    for name, (restype, argtypes) in _lib.CLUSTER_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_host_helpers():
    from coati_amd import _lib, cluster
    l = _lib.lib()
    ch = l.coati_cluster_chunk()
    assert ch == cluster.chunk_rows() == 512
    assert l.coati_cluster_items_max(0, 1) == 1 and l.coati_cluster_items_max(ch, 7) == 8 and l.coati_cluster_items_max(70001, 4096) == 136 + 4096
    for M, K in ((-1, 4), (2 ** 31, 4), (10, 0), (10, 4097)):
        assert l.coati_cluster_items_max(M, K) < 0 and "cluster_items_max" in l.coati_last_error().decode()
    # the item table of the header, and the bound the helper promises, on sizes around the chunk length
    sizes = torch.tensor([0, 1, ch - 1, ch, ch + 1, 2 * ch + 1, 0, 70001])
    offsets, item_off = cluster.item_table(sizes, ch)
    assert offsets.dtype == item_off.dtype == torch.int32
    assert offsets.tolist() == [0] + sizes.cumsum(0).tolist()
    assert (item_off[1:] - item_off[:-1]).tolist() == [0, 1, 1, 1, 2, 3, 0, 137]
    assert int(item_off[-1]) <= l.coati_cluster_items_max(int(sizes.sum()), len(sizes))


# ---- 2. refusals --------------------------------------------------------------------------------------------------------------------
def _host_pointer():
    buf = (ctypes.c_char * 4096)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_cluster_assign_refuses_bad_arguments_with_a_code():
    """decided on the host before any device call: the pointers are host buffers that a refusal never looks at"""
    from coati_amd import _lib
    l = _lib.lib()
    buf, p = _host_pointer()

    def call(lib=p, N=100, E=64, row_bias=None, c=p, K=8, cbias=None, assign=p, best=p, blocks=0):
        rc = l.coati_cluster_assign(lib, N, E, row_bias, c, K, cbias, assign, best, blocks, None)
        return rc, l.coati_last_error().decode()

    cases = [(dict(lib=None), "lib"), (dict(c=None), "c is null"), (dict(assign=None), "assign"), (dict(best=None), "best"),
             (dict(E=48), "E=48"), (dict(E=544), "E=544"), (dict(E=0), "E=0"), (dict(K=0), "K=0"), (dict(K=4097), "K=4097"),
             (dict(N=0), "N=0"), (dict(N=2 ** 31), f"N={2 ** 31}"), (dict(blocks=-1), "blocks=-1")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc < 0 and "cluster_assign" in msg and word in msg, (kw, rc, msg)


def test_cluster_sums_refuses_bad_arguments_with_a_code():
    from coati_amd import _lib
    l = _lib.lib()
    buf, p = _host_pointer()

    def call(lib=p, N=1000, E=64, order=p, M=1000, offsets=p, item_off=p, K=8, part=p, items_max=9, sums=p, blocks=0):
        rc = l.coati_cluster_sums(lib, N, E, order, M, offsets, item_off, K, part, items_max, sums, blocks, None)
        return rc, l.coati_last_error().decode()

    cases = [(dict(lib=None), "lib"), (dict(order=None), "order"), (dict(offsets=None), "offsets"), (dict(item_off=None), "item_off"),
             (dict(part=None), "part"), (dict(sums=None), "sums is null"), (dict(E=48), "E=48"), (dict(E=544), "E=544"), (dict(K=0), "K=0"),
             (dict(K=4097), "K=4097"), (dict(N=0), "N=0"), (dict(M=0), "M=0"), (dict(M=1001), "M=1001"), (dict(items_max=8), "items_max=8"),
             (dict(blocks=-1), "blocks=-1")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc < 0 and "cluster_sums" in msg and word in msg, (kw, rc, msg)


def test_python_layer_refuses():
    from coati_amd import cluster
    from coati_amd.search import EmbeddingIndex
    x = torch.randn(50, 40, generator=torch.Generator().manual_seed(0))
    dot = EmbeddingIndex(40, metric="dot", device="cpu")
    dot.add(x)
    with pytest.raises(ValueError, match="dot"):
        dot.kmeans(4)
    with pytest.raises(ValueError, match="dot"):
        dot.assign(x[:4])
    x16 = torch.zeros(8, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="dot"):
        cluster.assign_rows(x16, None, torch.zeros(2, 64), "dot")
    with pytest.raises(ValueError, match="dot"):
        cluster.kmeans_rows(x16, None, "dot", 2)
    for metric in ("cosine", "l2"):
        index = EmbeddingIndex(40, metric=metric, device="cpu")
        index.add(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            index.kmeans(4)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            index.assign(x[:4])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cluster.assign_rows(x16, None, torch.zeros(2, 64), metric)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cluster.kmeans_rows(x16, None, metric, 2)
    with pytest.raises(ValueError, match="bf16"):
        cluster.assign_rows(x16.float(), None, torch.zeros(2, 64), "l2")
    with pytest.raises(ValueError, match="centres"):
        cluster.prepare_centres(torch.zeros(4097, 64), "l2", 64)


def test_prepare_centres_is_the_restatement():
    from coati_amd import cluster
    c = torch.randn(17, 40, generator=torch.Generator().manual_seed(1))
    for metric in ("cosine", "l2"):
        c32, c16, cbias = cluster.prepare_centres(c, metric, 64)
        w32, w16, wbias = C.prepare_centres(torch.nn.functional.pad(c, (0, 24)), metric)
        assert c32.shape == (17, 64) and torch.equal(c32, w32) and torch.equal(c16, w16)
        assert (cbias is None and wbias is None) if metric == "cosine" else torch.equal(cbias, wbias)


def test_exports():
    import coati.generative as G
    import coati_amd.generative as AG
    from coati_amd.generative import coati_cluster
    assert G.diverse_screen is AG.diverse_screen is coati_cluster.diverse_screen
    assert G.diverse_subset is AG.diverse_subset is coati_cluster.diverse_subset


# ---- 3. representatives -------------------------------------------------------------------------------------------------------------
def test_representatives_on_a_hand_made_assignment():
    """five clusters: ties inside a cluster (the lowest row wins), an empty cluster (-1), a removed row (-1 in assign: nobody's), one member"""
    from coati_amd.cluster import Clustering
    assign = torch.tensor([2, 0, 0, -1, 2, 4, 0, 2, 4, 0, 2, 1], dtype=torch.int32)
    scores = torch.tensor([5.0, 1.0, 3.0, 99.0, 5.0, -2.0, 3.0, 4.0, -2.0, 3.0, 5.0, float("-inf")])
    cl = Clustering(torch.zeros(5, 8), assign, score=-scores)
    assert cl.sizes.tolist() == [4, 1, 4, 0, 2] and cl.sizes.dtype == torch.int64
    assert cl.members(0).tolist() == [1, 2, 6, 9] and cl.members(3).tolist() == [] and cl.members(4).tolist() == [5, 8]
    reps = cl.representatives(scores)
    assert reps.dtype == torch.int64 and reps.tolist() == [2, 11, 0, -1, 5]
    assert torch.equal(reps, C.representatives(assign, scores, 5))
    # no scores: the member nearest its centre (here score = -scores)
    assert torch.equal(cl.representatives(), C.representatives(assign, -scores, 5)) and cl.representatives().tolist() == [1, 11, 7, -1, 5]
    # a clustered subset answers in library rows
    sub = Clustering(torch.zeros(5, 8), assign, score=-scores, rows=100 + 2 * torch.arange(12))
    assert sub.representatives(scores).tolist() == [104, 122, 100, -1, 110] and sub.members(4).tolist() == [110, 116]
    with pytest.raises(ValueError, match="scores"):
        cl.representatives(scores[:5])
    with pytest.raises(IndexError):
        cl.members(5)
    gen = torch.Generator().manual_seed(3)
    for _ in range(5):
        a = torch.randint(-1, 9, (300,), generator=gen).to(torch.int32)
        v = torch.randint(0, 4, (300,), generator=gen).float()
        assert torch.equal(Clustering(torch.zeros(9, 8), a).representatives(v), C.representatives(a, v, 9))
