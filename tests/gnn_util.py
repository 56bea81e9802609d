"""Edge lists for the point encoder's operator tests, built on the CPU from a boolean adjacency so that the TEST chooses the segment
lengths, and float64 references of every kernel of csrc/gnn.hip / the edge path of csrc/gemm_rb16.hip, written as gathers and
index_add_ (they restate the formulas of csrc/kernels.h and csrc/gnn.hip).  Plain torch, any device, no library call."""
import math
from types import SimpleNamespace

import torch

# the degrees graph G1 must hold: 0 / 1 / 3 / 4 / 5 the 4-edge unroll and its tail, 15 / 16 / 17 and 31 / 32 / 33 the fused launch's 16-edge
# slabs, 63 / 64 / 65 the list kernels' 64-edge chunks, 71 a ragged second chunk, 128 / 129 a full second and a third chunk
G1_DEGREES = (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 71, 128, 129)


def circulant(n, deg):
    """bool [n, n]: atom j joined to j +- 1 .. +- deg // 2 (mod n), plus the perfect matching j <-> j + n / 2 for an odd degree"""
    r = deg // 2
    assert 0 <= deg < n and 2 * r < n and (deg % 2 == 0 or (n % 2 == 0 and r < n // 2)), (n, deg)
    j = torch.arange(n)
    adj = torch.zeros(n, n, dtype=torch.bool)
    for s in range(1, r + 1):
        adj[j, (j + s) % n] = True
        adj[j, (j - s) % n] = True
    if deg % 2:
        adj[j, (j + n // 2) % n] = True
    return adj


def molecules(A, specs):
    """bool [B, A, A]: molecule b is circulant(n, deg) of specs[b] on its first n slots, the other slots are isolated atoms"""
    adj = torch.zeros(len(specs), A, A, dtype=torch.bool)
    for b, (n, deg) in enumerate(specs):
        adj[b, :n, :n] = circulant(n, deg)
    return adj


def _atoms_for(A, deg):
    n = min(A, deg + 5)
    return n + 1 if (deg % 2 and n % 2) else n


def edge_list(adj, d2, w):
    """What launch_gnn_compact emits for the dense weights `w * adj`: receiver-major, senders ascending.  adj [B, A, A] bool, symmetric,
    zero diagonal; d2 / w [B, A, A] symmetric.  Index tensors are int32, as on the device."""
    B, A, _ = adj.shape
    assert adj.dtype == torch.bool and torch.equal(adj, adj.transpose(1, 2)) and not bool(adj.diagonal(dim1=1, dim2=2).any())
    assert torch.equal(d2, d2.transpose(1, 2)) and torch.equal(w, w.transpose(1, 2))
    b, j, k = adj.nonzero(as_tuple=True)          # row-major: (b, j) ascending, then k ascending
    E = b.numel()
    pos = torch.full((B, A, A), -1, dtype=torch.long)
    pos[b, j, k] = torch.arange(E)
    seg = torch.zeros(B * A + 1, dtype=torch.long)
    seg[1:] = adj.reshape(B * A, A).sum(1).cumsum(0)
    g = SimpleNamespace(B=B, A=A, BA=B * A, E=E, cap=B * A * A)
    g.seg, g.e_bj, g.e_bk, g.e_rev = seg.int(), (b * A + j).int(), (b * A + k).int(), pos[b, k, j].int()
    g.e_d2, g.e_w = d2[b, j, k].float().contiguous(), w[b, j, k].float().contiguous()
    g.n_edges = torch.tensor([E], dtype=torch.int32)
    g.degrees = sorted(set(adj.reshape(B * A, A).sum(1).tolist()))
    assert E == 0 or (float(g.e_w.min()) > 0 and float(g.e_w.max()) <= 1)
    return g


def _geometry(B, A, seed, exact):
    """symmetric [B, A, A] d2 and w; exact: quarter-integers (d2 in 1/4 .. 4, w in 1/4 .. 1), else d2 in (0, 25) and w in (0, 1]"""
    gen = torch.Generator().manual_seed(seed)
    if exact:
        d2 = torch.randint(1, 17, (B, A, A), generator=gen).float() / 4
        w = torch.randint(1, 5, (B, A, A), generator=gen).float() / 4
    else:
        d2 = torch.rand(B, A, A, generator=gen) * 24.9 + 0.05
        w = 1.0 - torch.rand(B, A, A, generator=gen) * 0.98
    up = torch.ones(A, A).triu().bool()
    return torch.where(up, d2, d2.transpose(1, 2)), torch.where(up, w, w.transpose(1, 2))


def build(adj, seed=0, exact=False):
    d2, w = _geometry(adj.shape[0], adj.shape[1], seed, exact)
    return edge_list(adj, d2, w)


def graph_g1(exact=False):
    """chunk edges: A = 130, one molecule per target degree; capacity B A A >= 65 536 > E"""
    A = 130
    g = build(molecules(A, [(_atoms_for(A, d), d) for d in G1_DEGREES]), seed=1, exact=exact)
    assert set(G1_DEGREES) <= set(g.degrees), g.degrees
    assert 1500 <= g.BA <= 2500 and 10000 < g.E < 65536 <= g.cap
    return g


def graph_g2(exact=False):
    """second passes: degrees 2 .. 5 on more than 4096 node rows; the row count is no multiple of 16, 256 or ceil(BA / 256)"""
    B, A = 71, 59
    g = build(molecules(A, [(40 + 2 * (b % 10), 2 + b % 4) for b in range(B)]), seed=2, exact=exact)
    assert g.BA > 4096 and g.BA % 16 and g.BA % 256 and g.BA % math.ceil(g.BA / 256) and g.degrees == [0, 2, 3, 4, 5]
    assert int(g.seg[-1]) > int(g.seg[4096 + 16])   # rows of the second pass have edges
    return g


def graph_g3(exact=False):
    """long list: E just above 65 536 and no multiple of 16"""
    B, A = 197, 22
    g = build(molecules(A, [(21, 16)] * (B - 1) + [(8, 3)]), seed=3, exact=exact)
    assert 65536 < g.E < 65536 + 512 and g.E % 16 and g.BA > 4096
    return g


def graph_pair(exact=False):
    return build(molecules(2, [(2, 1)]), seed=4, exact=exact)       # E = 2


def graph_empty(exact=False):
    return build(torch.zeros(2, 5, 5, dtype=torch.bool), seed=5, exact=exact)   # E = 0: every atom isolated


# ---- float64 references -------------------------------------------------------------------------------------------------------------
def silu(x):
    return x * torch.sigmoid(x)


def dsilu(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def _l(i):
    return i.long()


def edge_pre_act(P, e_bj, e_bk, e_d2, w1c, b1):
    """pre[e] = Pa[bj] + Pb[bk] + d2[e] w1c + b1 with P = [Pa | Pb] per node"""
    H = P.shape[1] // 2
    return P[_l(e_bj), :H] + P[_l(e_bk), H:] + e_d2.to(P.dtype).unsqueeze(1) * w1c + b1


def edge_pre(P, e_bj, e_bk, e_d2, w1c, b1):
    return silu(edge_pre_act(P, e_bj, e_bk, e_d2, w1c, b1))


def edge_linear(e1, W3, b3):
    return e1 @ W3.t() + b3


def edge_reduce(s2, e_bj, e_w, BA):
    return torch.zeros(BA, s2.shape[1], dtype=s2.dtype, device=s2.device).index_add_(0, _l(e_bj), silu(s2) * e_w.to(s2.dtype).unsqueeze(1))


def edge_reduce_bwd(dmi, s2, e_bj, e_w):
    return dmi[_l(e_bj)] * e_w.to(s2.dtype).unsqueeze(1) * dsilu(s2)


def edge_dpre(ds2, Bw, P, e_bj, e_bk, e_d2, w1c, b1):
    """EPI_EDGE_DPRE: (ds2 Bw^T) * SiLU'(pre); Bw [N, K] is the GEMM's B operand (the transposed second edge Linear)"""
    return (ds2 @ Bw.t()) * dsilu(edge_pre_act(P, e_bj, e_bk, e_d2, w1c, b1))


def edge_pre_bwd(dpre, e_bj, e_rev, e_d2, BA):
    """-> dP [BA, 2H] (receiver sums | sender sums through the reverse edges), dw1c [H], db1 [H]"""
    z = torch.zeros(BA, dpre.shape[1], dtype=dpre.dtype, device=dpre.device)
    dPa = z.clone().index_add_(0, _l(e_bj), dpre)
    dPb = z.clone().index_add_(0, _l(e_bj), dpre[_l(e_rev)])
    return torch.cat([dPa, dPb], 1), (dpre * e_d2.to(dpre.dtype).unsqueeze(1)).sum(0), dpre.sum(0)


def luts(device="cpu"):
    from coati_amd import periodic
    ix, iy = periodic.onehot_lut()
    return torch.tensor(ix, dtype=torch.int32, device=device), torch.tensor(iy, dtype=torch.int32, device=device)


def hot_indices(atoms, lut_ix, lut_iy):
    """per atom the two hot one-hot columns as the kernels read them: Z clamped to 0 .. 119, -1 = no column, iy dropped where it repeats ix"""
    z = atoms.clamp(0, 119)
    ix, iy = _l(lut_ix)[z], _l(lut_iy)[z]
    return ix, torch.where(iy == ix, torch.full_like(iy, -1), iy)


def onehot(atoms, lut_ix, lut_iy, dtype=torch.float64):
    """[BA, 28] multi-hot rows"""
    ix, iy = hot_indices(atoms, lut_ix, lut_iy)
    oh = torch.zeros(atoms.numel(), 28, dtype=dtype, device=atoms.device)
    for i in (ix, iy):
        oh[torch.arange(atoms.numel(), device=atoms.device)[i >= 0], i[i >= 0]] = 1
    return oh


def embed_pre(atoms, lut_ix, lut_iy, W, b):
    """e = W[:, ix] + W[:, iy] + b (before the instance norm); W [H, 28]"""
    return onehot(atoms, lut_ix, lut_iy, W.dtype) @ W.t() + b


def embed_bwd(atoms, lut_ix, lut_iy, de):
    """-> dW [H, 28], db [H]"""
    return de.t() @ onehot(atoms, lut_ix, lut_iy, de.dtype), de.sum(0)


def embed_table_bwd(atoms, de):
    return torch.zeros(84, de.shape[1], dtype=de.dtype, device=de.device).index_add_(0, atoms.clamp(0, 83), de)


def node_res_pre(u, atoms, lut_ix, lut_iy, W3c):
    """u + the hot columns of W3c [H, 28]"""
    return u + onehot(atoms, lut_ix, lut_iy, u.dtype) @ W3c.t()


def onehot_wgrad(atoms, lut_ix, lut_iy, du):
    return du.t() @ onehot(atoms, lut_ix, lut_iy, du.dtype)


def readout(o, mask):
    """o [B, A, H], mask [B, A] -> [B, H]"""
    n = mask.sum(1).clamp(min=1)
    return (o * mask.unsqueeze(2)).sum(1) / n.unsqueeze(1)


def readout_bwd(dhp, mask):
    n = mask.sum(1).clamp(min=1)
    return (dhp / n.unsqueeze(1)).unsqueeze(1) * mask.unsqueeze(2)


def wgrad(A, Bm):
    """-> dW [N, K] = A^T B, dbias [N] = colsum(A)"""
    return A.t() @ Bm, A.sum(0)
