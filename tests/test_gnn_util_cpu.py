"""tests/gnn_util.py proves itself before the GPU tests lean on it: the edge list equals a brute-force enumeration of the dense grid (what
launch_gnn_compact's four kernels do), e_rev is an involution that swaps receiver and sender, graph G1 holds every chunk-edge degree, and
every reference backward equals float64 autograd of its reference forward.  No GPU."""
import math

import pytest
import torch

from tests import gnn_util as U

GRAPHS = {"g1": U.graph_g1, "g2": U.graph_g2, "g3": U.graph_g3, "pair": U.graph_pair, "empty": U.graph_empty}


@pytest.fixture(scope="module", params=sorted(GRAPHS))
def graph(request):
    return GRAPHS[request.param]()


def test_list_equals_the_dense_enumeration():
    """gnn_compact_count / scan / fill / rev, restated as loops over the dense [B, A, A] grid (G1: every degree; the pair; the empty list)"""
    for make in (U.graph_g1, U.graph_pair, U.graph_empty):
        g = make()
        adj_w = torch.zeros(g.B, g.A, g.A)
        adj_w.view(-1)[(g.e_bj.long() * g.A + g.e_bk.long() % g.A)] = g.e_w        # the dense weights the list stands for
        d2 = torch.zeros(g.B, g.A, g.A)
        d2.view(-1)[(g.e_bj.long() * g.A + g.e_bk.long() % g.A)] = g.e_d2
        wl, dl = adj_w.reshape(-1, g.A).tolist(), d2.reshape(-1, g.A).tolist()
        seg, ebj, ebk, ed2, ew, pos = [0], [], [], [], [], {}
        for bj in range(g.BA):
            b = bj // g.A
            for k in range(g.A):
                if wl[bj][k] > 0:
                    pos[(bj, k)] = len(ebj)
                    ebj.append(bj); ebk.append(b * g.A + k); ed2.append(dl[bj][k]); ew.append(wl[bj][k])
            seg.append(len(ebj))
        rev = [pos[(bk, bj % g.A)] for bj, bk in zip(ebj, ebk)]
        assert g.E == len(ebj) == int(g.n_edges[0]) == int(g.seg[-1])
        assert g.seg.tolist() == seg and g.e_bj.tolist() == ebj and g.e_bk.tolist() == ebk and g.e_rev.tolist() == rev
        assert g.e_d2.tolist() == ed2 and g.e_w.tolist() == ew
        assert all(t.dtype == torch.int32 for t in (g.seg, g.e_bj, g.e_bk, g.e_rev, g.n_edges))


def test_order_reverse_and_symmetry(graph):
    g = graph
    assert g.seg.numel() == g.BA + 1 and int(g.seg[0]) == 0 and int(g.seg[-1]) == g.E and g.cap == g.BA * g.A
    key = g.e_bj.long() * g.cap + g.e_bk.long()
    assert bool((key[1:] > key[:-1]).all())                                      # receiver-major, senders ascending, no duplicate
    assert torch.equal(torch.bincount(g.e_bj.long(), minlength=g.BA).cumsum(0), g.seg[1:].long())
    assert bool((g.e_bj // g.A == g.e_bk // g.A).all()) and bool((g.e_bj != g.e_bk).all())
    r = g.e_rev.long()
    assert torch.equal(r[r], torch.arange(g.E)) and torch.equal(g.e_bj[r], g.e_bk) and torch.equal(g.e_bk[r], g.e_bj)
    assert torch.equal(g.e_d2[r], g.e_d2) and torch.equal(g.e_w[r], g.e_w)
    if g.E:
        assert float(g.e_w.min()) > 0 and float(g.e_w.max()) <= 1 and float(g.e_d2.min()) > 0


def test_degree_sets_and_sizes():
    g1, g2, g3 = U.graph_g1(), U.graph_g2(), U.graph_g3()
    assert set(U.G1_DEGREES) <= set(g1.degrees) and g1.A == 130 and 129 in g1.degrees
    assert g1.E < 65536 <= g1.cap and 1500 <= g1.BA <= 2500
    assert g2.BA > 4096 and g2.BA % 16 != 0 and g2.BA % 256 != 0 and g2.BA % math.ceil(g2.BA / 256) != 0
    assert math.ceil(g2.BA / 256) > 16                                                   # the fused forward's waves take a second receiver
    assert 65536 < g3.E and g3.E % 16 != 0 and math.ceil(math.ceil(g3.E / 16) / 256) > 16     # the resident kernel's waves take a second slab
    assert U.graph_pair().E == 2 and U.graph_empty().E == 0
    ge = U.graph_g1(exact=True)
    assert torch.equal(ge.e_d2 * 4, (ge.e_d2 * 4).round()) and torch.equal(ge.e_w * 4, (ge.e_w * 4).round())
    assert torch.equal(ge.e_bk, g1.e_bk) and torch.equal(ge.seg, g1.seg)


def _close(a, b):
    torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12 * float(b.abs().max()))


@pytest.fixture(scope="module")
def small():
    """a graph small enough for autograd with every kind of segment: G1's degrees up to 17 and the pair"""
    A = 24
    g = U.build(U.molecules(A, [(U._atoms_for(A, d), d) for d in (0, 1, 3, 4, 5, 15, 16, 17)]), seed=9)
    gen = torch.Generator().manual_seed(11)
    H = 12
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    return g, H, r


def test_edge_backwards_equal_autograd(small):
    g, H, r = small
    P, w1c, b1, W3, b3 = (r(g.BA, 2 * H).requires_grad_(), r(H).requires_grad_(), r(H).requires_grad_(), r(H, H), r(H))
    pre = U.edge_pre_act(P, g.e_bj, g.e_bk, g.e_d2, w1c, b1)
    dpre = r(g.E, H)
    gP, gw, gb = torch.autograd.grad(pre, (P, w1c, b1), dpre)
    dP, dw1c, db1 = U.edge_pre_bwd(dpre, g.e_bj, g.e_rev, g.e_d2, g.BA)
    _close(dP, gP); _close(dw1c, gw); _close(db1, gb)
    # the second Linear's input gradient through SiLU: EPI_EDGE_DPRE with B = W3^T
    pre = pre.detach().requires_grad_()
    ds2 = r(g.E, H)
    (gpre,) = torch.autograd.grad(U.edge_linear(U.silu(pre), W3, b3), pre, ds2)
    _close(U.edge_dpre(ds2, W3.t().contiguous(), P.detach(), g.e_bj, g.e_bk, g.e_d2, w1c.detach(), b1.detach()), gpre)
    s2 = r(g.E, H).requires_grad_()
    dmi = r(g.BA, H)
    (gs2,) = torch.autograd.grad(U.edge_reduce(s2, g.e_bj, g.e_w, g.BA), s2, dmi)
    _close(U.edge_reduce_bwd(dmi, s2.detach(), g.e_bj, g.e_w), gs2)


ATOMS = [0, 1, 6, 8, 35, 92, 125, 1, 1, 6, 89, 103, 104, 57, 71, 2, 118, 119, -3]


def test_node_backwards_equal_autograd(small):
    _, H, r = small
    lx, ly = U.luts()
    atoms = torch.tensor(ATOMS)
    ix, iy = U.hot_indices(atoms, lx, ly)
    assert int(iy[5]) == -1 and int(ix[5]) >= 0 and int(iy[2]) >= 0 and torch.equal(ix[6], ix[-2]) and int(iy[10]) == -1   # 92, 89: actinides
    oh = U.onehot(atoms, lx, ly)
    assert oh.sum(1).tolist()[:6] == [2, 2, 2, 2, 2, 1] and float(oh.sum(1).min()) >= 1
    W, b, de = r(H, 28).requires_grad_(), r(H).requires_grad_(), r(len(ATOMS), H)
    gW, gb = torch.autograd.grad(U.embed_pre(atoms, lx, ly, W, b), (W, b), de)
    dW, db = U.embed_bwd(atoms, lx, ly, de)
    _close(dW, gW); _close(db, gb)
    # an actinide contributes to db and to its ix column only
    one = torch.zeros(len(ATOMS), H, dtype=torch.float64); one[5] = 1
    dW1, db1 = U.embed_bwd(atoms, lx, ly, one)
    assert torch.equal(db1, torch.ones(H, dtype=torch.float64)) and dW1.sum(0).nonzero().flatten().tolist() == [int(ix[5])]
    T = r(84, H).requires_grad_()
    (gT,) = torch.autograd.grad(T[atoms.clamp(0, 83)], T, de)
    _close(U.embed_table_bwd(atoms, de), gT)
    W3c, u = r(H, 28).requires_grad_(), r(len(ATOMS), H)
    (gW3,) = torch.autograd.grad(U.node_res_pre(u, atoms, lx, ly, W3c), W3c, de)
    _close(U.onehot_wgrad(atoms, lx, ly, de), gW3)
    o = r(3, 5, H).requires_grad_()
    mask = torch.tensor([[1, 1, 0, 1, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]], dtype=torch.float64)
    dhp = r(3, H)
    (go,) = torch.autograd.grad(U.readout(o, mask), o, dhp)
    _close(U.readout_bwd(dhp, mask), go)
    Wl, x, dy = r(7, H).requires_grad_(), r(20, H), r(20, 7)
    bl = r(7).requires_grad_()
    gWl, gbl = torch.autograd.grad(x @ Wl.t() + bl, (Wl, bl), dy)
    dWl, dbl = U.wgrad(dy, x)
    _close(dWl, gWl); _close(dbl, gbl)


def test_header_is_bound_and_refuses_bad_arguments_on_the_host():
    """include/coati_gnn_ops.h is read into a table of its own, the library exports its entries, and the wrappers' argument checks answer
    with codes before any HIP call"""
    import ctypes
    from coati_amd import _lib, build
    assert build.GNN_OPS_HEADER in build._sources() and len(_lib.GNN_OPS_PROTOTYPES) == 12
    assert not set(_lib.GNN_OPS_PROTOTYPES) & set(_lib.PROTOTYPES)
    l = _lib.lib()
    for name in _lib.GNN_OPS_PROTOTYPES:
        assert hasattr(l, name), name
    fake, res = 4096, ctypes.c_int32(-1)      # never dereferenced
    assert l.coati_gemm_rows_dev(None, fake, 256, fake, 256, 64, 256, 256, fake, 256, None, 0, None, 0, None, None, 0, None, 0, 0, None, None,
                                 ctypes.byref(res), None) < 0 and b"null argument" in l.coati_last_error()
    assert l.coati_gemm_rows_dev(fake, fake, 256, fake, 256, 64, 256, 256, fake, 256, None, 5, None, 0, None, None, 0, None, 0, 0, None, None,
                                 ctypes.byref(res), None) < 0 and b"EPI_BF16 and EPI_EDGE_DPRE only" in l.coati_last_error()
    assert l.coati_gnn_edge_fwd_fused(*([fake, 256] + [fake] * 5 + [1, fake, fake, 128, fake, fake, fake, fake, 128, 10, 128, None])) < 0
    assert b"H = 256 only" in l.coati_last_error()
    assert l.coati_wgrad_rows_dev(None, fake, 256, fake, 256, 64, 256, 256, fake, 256, None, None) < 0
    assert l.coati_wgrad_split_workspace_bytes(0, None, None, 4) == 0
