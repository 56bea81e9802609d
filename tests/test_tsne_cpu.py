"""Embedding maps, host side (no GPU): the float64 restatement of tests/tsne_util.py against sklearn's exact t-SNE objective,
coati_amd.tsne.joint against the dense definition, the refusals of knn_graph, and include/coati_tsne.h: it parses against coati_hip.h
and the library exports what it declares and refuses bad arguments with a code before any device call."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import tsne_util as U  # noqa: E402

NAMES = ["coati_tsne_affinities", "coati_tsne_chunk", "coati_tsne_part_floats", "coati_tsne_repulsion", "coati_tsne_step"]


# ---- 1. the restatement is sklearn's objective ----------------------------------------------------------------------------------------
def test_restatement_is_sklearns_kl_divergence():
    """two float64 evaluations of one formula on a dense P at n = 40: 1e-10 relative, for the KL and for every gradient entry (relative to
    the largest one)"""
    pytest.importorskip("sklearn")
    import numpy as np
    from scipy.spatial.distance import squareform
    from sklearn.manifold._t_sne import _kl_divergence
    n = 40
    g = torch.Generator().manual_seed(3)
    A = torch.rand(n, n, generator=g, dtype=torch.float64) + 0.05
    P = A + A.T
    P.fill_diagonal_(0.0)
    P = P / P.sum()
    for scale in (1e-4, 1.0, 10.0):
        y = scale * torch.randn(n, 2, generator=g, dtype=torch.float64)
        kl, grad = U.kl_and_grad(y, P)
        want_kl, want_grad = _kl_divergence(y.numpy().ravel().copy(), squareform(P.numpy(), checks=False), 1.0, n, 2)
        want_grad = torch.from_numpy(np.asarray(want_grad)).reshape(n, 2)
        assert abs(float(kl) - want_kl) <= 1e-10 * abs(want_kl), (scale, float(kl), want_kl)
        assert float((grad - want_grad).abs().max()) <= 1e-10 * float(want_grad.abs().max()), scale


def test_restated_affinities_reach_the_perplexity_and_survive_the_hard_rows():
    d2 = torch.tensor([[0.5, 1.0, 2.0, 4.0, 8.0, 9.0], [3.0] * 6, [0.0, 0.0, 0.0, 1.0, 2.0, 3.0], [1.0, 2.0, 0.0, 0.0, 0.0, 0.0],
                       [0.0] * 6, [1.0, 1e6, 2e6, 3e6, 4e6, 5e6]])
    nbr = torch.tensor([[1, 2, 3, 4, 5, 0]] * 6, dtype=torch.int32)
    nbr[3, 2:] = -1
    nbr[4, :] = -1
    p, beta, H = U.affinities(d2, nbr, 3.0)
    assert torch.isfinite(p).all() and torch.isfinite(beta).all()
    assert abs(float(H[0].exp()) - 3.0) < 1e-9 and abs(float(H[5].exp()) - 3.0) < 1e-6
    assert torch.allclose(p[1], torch.full((6,), 1 / 6, dtype=torch.float64))        # equal distances: uniform
    assert torch.equal(p[3, 2:], torch.zeros(4, dtype=torch.float64)) and abs(float(p[3].sum()) - 1) < 1e-12   # 2 entries < perplexity 3
    assert torch.equal(p[4], torch.zeros(6, dtype=torch.float64)) and float(beta[4]) == 0.0
    assert torch.allclose(p.sum(dim=1)[[0, 1, 2, 3, 5]], torch.ones(5, dtype=torch.float64))


# ---- 2. joint --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(2, 1), (7, 3), (300, 17)])
def test_joint_is_the_dense_symmetrised_p(n, k):
    from coati_amd import tsne
    g = torch.Generator().manual_seed(n)
    nbr = torch.stack([torch.tensor([j for j in torch.randperm(n, generator=g).tolist() if j != i][:k]) for i in range(n)]).to(torch.int32)
    p = torch.rand(n, k, generator=g)
    if n > 2:
        nbr[1, k - 1] = -1          # a padded entry, and a row without any
        nbr[2, :] = -1
    p = torch.where(nbr >= 0, p, torch.zeros_like(p))
    p = p / p.sum(dim=1, keepdim=True).clamp_min(1e-30)
    offsets, cols, vals = tsne.joint(nbr, p)
    assert offsets.dtype == torch.int64 and cols.dtype == torch.int32 and vals.dtype == torch.float32
    assert offsets.shape == (n + 1,) and int(offsets[0]) == 0 and int(offsets[-1]) == cols.shape[0] == vals.shape[0]
    rows = U.csr_rows(offsets)
    dense = torch.zeros(n, n, dtype=torch.float32)
    dense[rows, cols.long()] = vals
    # element for element: the f32 sum of at most two f32 terms, then one division
    P32 = torch.zeros(n, n, dtype=torch.float32)
    there = nbr >= 0
    P32[torch.arange(n)[:, None].expand(n, k)[there], nbr[there].long()] = p[there]
    assert torch.equal(dense, (P32 + P32.T) / float(2 * n))
    assert torch.equal(dense, dense.T)
    key = rows * n + cols.long()
    assert bool((key[1:] > key[:-1]).all())                       # rows in order, columns ascending, no key twice
    assert float((dense.double() - U.joint_dense(nbr, p)).abs().max()) <= 2.0 ** -24 * float(dense.max()) * 2
    live = int((p.sum(dim=1) > 0).sum())
    assert abs(float(vals.double().sum()) - live / n) <= n * k * 2.0 ** -24


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------------
def test_knn_graph_refuses_dot_and_k_out_of_range():
    from coati_amd import tsne
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(32, metric="dot", device="cpu")
    with pytest.raises(ValueError, match="dot"):
        tsne.knn_graph(index, 5)
    with pytest.raises(ValueError, match="dot"):
        index.knn_graph(5)
    for metric in ("cosine", "l2"):
        index = EmbeddingIndex(32, metric=metric, device="cpu")
        index.add(torch.randn(10, 32))
        for k in (0, -1, 128, 1000):
            with pytest.raises(ValueError, match="k="):
                index.knn_graph(k)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            index.knn_graph(3)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            index.tsne(perplexity=2.0, iters=1)


def test_python_layer_refuses_what_it_must():
    from coati_amd import tsne
    d2, nbr = torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(ValueError):
        tsne.affinities(d2.double(), nbr, 2.0)
    with pytest.raises(ValueError):
        tsne.affinities(torch.zeros(4, 129), torch.zeros(4, 129, dtype=torch.int32), 2.0)
    with pytest.raises(ValueError, match="perplexity"):
        tsne.affinities(d2, nbr, 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsne.affinities(d2, nbr, 2.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsne.repulsion(torch.zeros(4, 2))
    with pytest.raises(ValueError):
        tsne.repulsion(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="init"):
        tsne.initial_points(4, "pca")
    a, b = tsne.initial_points(100, "random", 5), tsne.initial_points(100, "random", 5)
    assert torch.equal(a, b) and a.dtype == torch.float32 and 0 < float(a.abs().max()) < 1e-3
    import coati.generative as G
    import coati_amd.generative as AG
    assert G.embed_xy is AG.embed_xy
    with pytest.raises(ValueError, match="embed_xy"):
        AG.embed_xy(torch.zeros(1, 8))


# ---- 4. the twentieth header -------------------------------------------------------------------------------------------------------------
def test_tsne_header_parses_into_a_table_of_its_own():
    from coati_amd import _abi, _lib, build
    assert sorted(_lib.TSNE_PROTOTYPES) == NAMES
    for other in (_lib.PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.SEARCH_PROTOTYPES, _lib.CLUSTER_PROTOTYPES, _lib.RADIUS_PROTOTYPES,
                  _lib.SEARCH4_PROTOTYPES):
        assert not set(_lib.TSNE_PROTOTYPES) & set(other)
    assert _lib.ABI_VERSION == 5
    I, P, L, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert _lib.TSNE_PROTOTYPES["coati_tsne_affinities"] == (I, [P, P, L, I, F, I, P, P, P])
    assert _lib.TSNE_PROTOTYPES["coati_tsne_repulsion"] == (I, [P, L, P, P, P, L, I, P])
    assert _lib.TSNE_PROTOTYPES["coati_tsne_step"] == (I, [P, P, P, P, P, P, L, F, F, F, F, P, P, P, P, P, P])
    assert _lib.TSNE_PROTOTYPES["coati_tsne_chunk"] == (I, [])
    assert _lib.TSNE_PROTOTYPES["coati_tsne_part_floats"] == (L, [L])
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.TSNE_HEADER) as f:
        again = _abi.parse(f.read(), guard="COATI_TSNE_H", name="coati_tsne.h", base=base)
    assert again.prototypes == _lib.TSNE_PROTOTYPES and again.version == 5 and not again.experimental
    assert "tsne.hip" in build.HIP_UNITS and build.TSNE_HEADER in build._sources()


def test_library_exports_the_tsne_entries():
    """(_lib.exported_symbols() is coati_hip.h's table alone -- tests/test_host_cpu.py holds it to that; a further header's names are
    checked where lib() checks them: every one is a bound symbol of the loaded library)"""
    from coati_amd import _lib
    l = _lib.lib()
    assert l.coati_abi_version() == 5
    for name, (restype, argtypes) in _lib.TSNE_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_host_helpers():
    from coati_amd import _lib, tsne
    l = _lib.lib()
    J = l.coati_tsne_chunk()
    assert J == tsne.chunk_points() == 1024
    assert l.coati_tsne_part_floats(1) == 3 and l.coati_tsne_part_floats(J) == 3 * J and l.coati_tsne_part_floats(J + 1) == 6 * (J + 1)
    assert l.coati_tsne_part_floats(2 ** 31 - 1) == 3 * (2 ** 31 - 1) * 2 ** 21
    for N in (0, -1, 2 ** 31):
        assert l.coati_tsne_part_floats(N) < 0 and "tsne_part_floats" in l.coati_last_error().decode()


def _host_pointer():
    buf = (ctypes.c_char * 4096)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_entries_refuse_bad_arguments_with_a_code():
    """every refusal comes before any HIP call: the pointers here are host memory"""
    from coati_amd import _lib
    l = _lib.lib()
    keep, a = _host_pointer()
    keep2, b = _host_pointer()

    def affinities(d2=a, nbr=a, N=4, k=3, perplexity=2.0, steps=10, p=a, beta=a):
        return l.coati_tsne_affinities(d2, nbr, N, k, perplexity, steps, p, beta, None)

    def repulsion(y=a, N=4, rep=a, z=a, part=None, part_floats=0, blocks=0):
        return l.coati_tsne_repulsion(y, N, rep, z, part, part_floats, blocks, None)

    def step(y=a, rep=a, zsum=a, offsets=a, cols=a, vals=a, N=4, update=a, gains=a, y_out=b):
        return l.coati_tsne_step(y, rep, zsum, offsets, cols, vals, N, 1.0, 0.5, 100.0, 0.01, update, gains, y_out, None, None, None)

    for fn, what, cases in ((affinities, "tsne_affinities", (dict(d2=None), dict(nbr=None), dict(p=None), dict(N=0), dict(N=2 ** 31), dict(k=0),
                                                            dict(k=129), dict(perplexity=0.0), dict(perplexity=float("inf")),
                                                            dict(perplexity=float("nan")), dict(steps=-1), dict(steps=10001))),
                            (repulsion, "tsne_repulsion", (dict(y=None), dict(rep=None), dict(z=None), dict(N=0), dict(N=2 ** 31), dict(blocks=-1),
                                                          dict(part_floats=-1))),
                            (step, "tsne_step", (dict(y=None), dict(rep=None), dict(zsum=None), dict(offsets=None), dict(update=None),
                                                 dict(gains=None), dict(y_out=None), dict(y_out=a), dict(N=0), dict(N=2 ** 31)))):
        for kw in cases:
            rc = fn(**kw)
            msg = l.coati_last_error().decode()
            assert rc < 0 and what in msg, (what, kw, rc, msg)
