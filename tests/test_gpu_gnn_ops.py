"""The point encoder's edge, backward and device-side-row-count kernels one by one, through the C ABI of include/coati_gnn_ops.h, against
the float64 references of tests/gnn_util.py on edge lists whose segment lengths the test chooses (tests/test_gnn_util_cpu.py proves the
helper).  Two kinds of input:

  * exact: small integers (quarter-integers for e_d2 / e_w), every product and every fp32 sum exact in any order (the totals are asserted to
    stay below 2^24), outputs compared with torch.equal -- a dropped, duplicated or misplaced edge or row changes an integer;
  * real-valued, for what holds SiLU / SiLU': per element |got - ref| <= 2^-8 |ref| + TAU * max|ref| (one bf16 rounding with room for a
    flipped tie, plus the fp32 evaluation), and the project's check(..., TB).  A stage that consumes a bf16 tensor an earlier stage of the
    same launch wrote is compared with the reference evaluated on the DEVICE's bits of that tensor.

Outputs of a launch with a device-side row count are allocated at capacity and filled with a sentinel; the rows past the count must keep it."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gnn_util as U  # noqa: E402
from tests.gpu_util import check, log  # noqa: E402

DEV = "cuda:0"
TB = 6e-3       # tests/test_gpu_ops.py's bf16-output tolerance
# the fp32 evaluation's share of the bound (fast exponential, summation order), relative to max|ref|.  Measured on the MI355X: the worst
# residual beyond 2^-8 |ref| over every real-valued comparison of this file is MEASURED_RESIDUAL = 3.387e-8 (s2 of the fused forward on G3; the
# products' write-outs reach 1.7e-8 .. 3.0e-8, e1 / mi / ds2 / the node kernels stay below 2e-9: most elements sit inside one bf16 rounding)
# and TAU = 6.774e-8 is twice that; bound() logs every comparison's figure through log().  None of this runs atomics or depends on a launch's
# timing, so the figures repeat from run to run.  A kernel that needs more than 1e-4 is a finding to explain, not a constant to raise.
MEASURED_RESIDUAL = 3.387e-8
TAU = 2 * MEASURED_RESIDUAL
assert TAU <= 1e-4
SENT16 = 0x5A5B     # bf16 bit pattern of untouched rows
EPI_BF16, EPI_EDGE_DPRE = 0, 10
ATOMS = [0, 1, 6, 8, 35, 92, 125]     # padding, H, C, O, Br, an actinide (no period bit), one above 119 (clamped)


def _call(name, *args):
    from coati_amd import _lib
    _lib.call(name, *args)


def _ptr(t, offset=0):
    if t is None:
        return None
    # (an empty view reports a null data_ptr(): take the address it has inside its buffer)
    base = t.data_ptr() if t.numel() else t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()
    return ctypes.c_void_p(base + offset * t.element_size())


def _stream():
    from coati_amd.ops import stream
    return stream()


def _to_dev(g):
    """device copies; every array is a view of a buffer with 8 zero elements behind it, so the empty list's arrays are not null pointers"""
    for k in ("seg", "e_bj", "e_bk", "e_rev", "e_d2", "e_w", "n_edges"):
        t = getattr(g, k)
        buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=DEV)
        buf[:t.numel()] = t.to(DEV)
        setattr(g, k, buf[:t.numel()])
    return g


@pytest.fixture(scope="module")
def graphs():
    make = {"g1": U.graph_g1, "g2": U.graph_g2, "g3": U.graph_g3, "pair": U.graph_pair, "empty": U.graph_empty}
    return {(n, ex): _to_dev(f(exact=ex)) for n, f in make.items() for ex in (False, True)}


def sent16(rows, cols):
    return torch.full((max(rows, 1), cols), SENT16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def kept16(t):
    return bool((t.view(torch.int16) == SENT16).all())


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def ints(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen, device=DEV).float()


def randn(gen, *shape):
    return torch.randn(*shape, generator=gen, device=DEV)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def bound(name, got, ref):
    """one bf16 rounding of the float64 reference plus TAU of its scale, element by element; then the project's check"""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if ref.numel() == 0:
        return
    ref = ref.double()
    scale = max(float(ref.abs().max()), 1e-30)
    resid = float(((got.double() - ref).abs() - 2.0 ** -8 * ref.abs()).clamp(min=0).max()) / scale
    log(f"{name:60s} residual beyond 2^-8|ref| {resid:.3e} of scale  TAU {TAU:.1e}  {'OK' if resid <= TAU else 'FAIL'}")
    assert bool(torch.isfinite(got.float()).all()), name
    assert resid <= TAU, f"{name}: {resid:.3e} of scale beyond one bf16 rounding > TAU {TAU:.1e}"
    check(name, got.float(), ref.float(), TB)


def edge_params(gen, BA, H):
    """P [BA, 2H] bf16, the first edge Linear [H, 2H + 1] f32 whose last column is w1c (the engine's stride), b1"""
    P = randn(gen, BA, 2 * H).bfloat16()
    W1 = (randn(gen, H, 2 * H + 1) * 0.05)
    b1 = (randn(gen, H) * 0.1)
    return P, W1, b1


# ---- forward edge path ---------------------------------------------------------------------------------------------------------------
def _fwd_refs(g, P, W1, b1, W3, b3, e1, s2, mi, H, name):
    """stage by stage: e1 from the inputs, s2 from the device's e1 bits, mi from the device's s2 bits"""
    E = g.E
    bound(f"{name} e1", e1[:E], U.edge_pre(P.double(), g.e_bj, g.e_bk, g.e_d2, W1[:, 2 * H].double(), b1.double()))
    bound(f"{name} s2", s2[:E], U.edge_linear(e1[:E].double(), W3.double(), b3.double()))
    bound(f"{name} mi", mi, U.edge_reduce(s2[:E].double(), g.e_bj, g.e_w, g.BA))
    deg = g.seg[1:] - g.seg[:-1]
    assert bool((mi[deg == 0].contiguous().view(torch.int16) == 0).all()), f"{name}: a receiver without edges has a non-zero mi row"
    assert kept16(e1[E:]) and kept16(s2[E:]), f"{name}: a row past the {E} edges was written"


def _fwd_operands(g, H, seed):
    gen = _gen(seed)
    P, W1, b1 = edge_params(gen, g.BA, H)
    W3 = (randn(gen, H, H) / 16).bfloat16()
    b3 = (randn(gen, H) * 0.1)
    return P, W1, b1, W3, b3


@pytest.mark.parametrize("gname", ["g1", "g2", "g3", "empty", "pair"])
def test_edge_fwd_fused(graphs, gname):
    """gnn_edge_fwd_fused_kernel (H = 256, always this kernel): G1 every slab count from 1 to 9 with every tail, G2 / G3 a second receiver per
    wave (more than 4096 node rows), the empty list and the single pair"""
    g, H = graphs[(gname, False)], 256
    P, W1, b1, W3, b3 = _fwd_operands(g, H, 17)
    e1, s2, hcat = sent16(g.cap, H), sent16(g.cap, H), sent16(g.BA, 2 * H)      # mi is the right half of [h | mi], as in the engine
    _call("coati_gnn_edge_fwd_fused", _ptr(P), 2 * H, _ptr(g.seg), _ptr(g.e_bk), _ptr(g.e_d2), _ptr(g.e_w), _ptr(W1, 2 * H), 2 * H + 1, _ptr(b1),
          _ptr(W3), H, _ptr(b3), _ptr(e1), _ptr(s2), _ptr(hcat, H), 2 * H, g.BA, H, _stream())
    torch.cuda.synchronize()
    assert kept16(hcat[:, :H].contiguous()), "the h half of [h | mi] was written"
    _fwd_refs(g, P, W1, b1, W3, b3, e1, s2, hcat[:, H:], H, f"edge_fwd_fused {gname}")


def test_edge_fwd_fused_refuses_other_widths(graphs):
    g, H = graphs[("pair", False)], 128
    P, W1, b1, W3, b3 = _fwd_operands(g, H, 18)
    e1, s2, mi = sent16(g.cap, H), sent16(g.cap, H), sent16(g.BA, H)
    with pytest.raises(RuntimeError, match="H = 256 only"):
        _call("coati_gnn_edge_fwd_fused", _ptr(P), 2 * H, _ptr(g.seg), _ptr(g.e_bk), _ptr(g.e_d2), _ptr(g.e_w), _ptr(W1, 2 * H), 2 * H + 1, _ptr(b1),
              _ptr(W3), H, _ptr(b3), _ptr(e1), _ptr(s2), _ptr(mi), H, g.BA, H, _stream())
    torch.cuda.synchronize()
    assert kept16(e1) and kept16(s2) and kept16(mi)


def _gemm_rows_dev(g, A, Bw, C, bias, epi, N, K, expect_resident, edge=None):
    res = ctypes.c_int32(-1)
    P, ldp, d2, w1c, stride, b1, H = edge if edge is not None else (None, 0, None, None, 0, None, 0)
    _call("coati_gemm_rows_dev", _ptr(g.n_edges), _ptr(A), K, _ptr(Bw), K, g.cap, N, K, _ptr(C), N, _ptr(bias), epi, _ptr(P), ldp, _ptr(d2),
          w1c, stride, _ptr(b1), g.A, H, _ptr(g.e_bj) if edge is not None else None, _ptr(g.e_bk) if edge is not None else None,
          ctypes.byref(res), _stream())
    torch.cuda.synchronize()
    assert res.value == int(expect_resident), f"gemm_rb16_resident_supported = {res.value}, the test expected {int(expect_resident)}"


def test_edge_fwd_three_launches(graphs):
    """the H != 256 route at H = 256 for comparison: gnn_edge_pre_c, the device-row-count product (the resident kernel: K = 256, capacity
    >= 4096), gnn_edge_reduce_c -- each against the reference, not against the fused launch (their accumulation orders differ)"""
    g, H = graphs[("g1", False)], 256
    P, W1, b1, W3, b3 = _fwd_operands(g, H, 17)
    e1, s2, mi = sent16(g.cap, H), sent16(g.cap, H), sent16(g.BA, H)
    _call("coati_gnn_edge_pre", _ptr(P), 2 * H, _ptr(g.seg), _ptr(g.e_bk), _ptr(g.e_d2), _ptr(W1, 2 * H), 2 * H + 1, _ptr(b1), _ptr(e1), g.BA, H, _stream())
    _gemm_rows_dev(g, e1, W3, s2, b3, EPI_BF16, H, H, True)
    _call("coati_gnn_edge_reduce", _ptr(s2), _ptr(g.seg), _ptr(g.e_w), _ptr(mi), H, g.BA, H, _stream())
    torch.cuda.synchronize()
    _fwd_refs(g, P, W1, b1, W3, b3, e1, s2, mi, H, "edge forward, three launches g1")


# ---- backward edge path --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", ["g1", "g2", "empty", "pair"])
@pytest.mark.parametrize("H", [64, 128, 256, 320])
def test_edge_reduce_bwd(graphs, gname, H):
    """gnn_edge_reduce_bwd_c_kernel: H = 64 leaves lanes without channels, 320 takes a second, partly active 256-channel turn"""
    g = graphs[(gname, False)]
    gen = _gen(H)
    dmi = randn(gen, g.BA, H).bfloat16()
    s2 = (randn(gen, max(g.E, 1), H) * 2).bfloat16()
    ds2 = sent16(g.E + 64, H)
    _call("coati_gnn_edge_reduce_bwd", _ptr(dmi), H, _ptr(s2), _ptr(g.seg), _ptr(g.e_w), _ptr(ds2), g.BA, H, _stream())
    torch.cuda.synchronize()
    bound(f"edge_reduce_bwd {gname} H={H}", ds2[:g.E], U.edge_reduce_bwd(dmi.double(), s2[:g.E].double(), g.e_bj, g.e_w))
    assert kept16(ds2[g.E:])


@pytest.mark.parametrize("gname", ["g1", "g2", "empty", "pair"])
@pytest.mark.parametrize("H", [64, 128, 256, 320])
def test_edge_pre_bwd_exact(graphs, gname, H):
    """gnn_edge_pre_bwd_c_kernel on integers: both halves of dP, dw1c (the engine's stride 2H + 1) and db1 bit for bit.  G2 has more than
    4096 node rows: the 256 workgroups of 16 waves go over the receivers a second time."""
    g = graphs[(gname, True)]
    gen = _gen(100 + H)
    dpre = ints(gen, -3, 3, max(g.E, 1), H).bfloat16()
    dP = sent16(g.BA, 2 * H)
    W1_0, db1_0 = ints(gen, -9, 9, H, 2 * H + 1), ints(gen, -9, 9, H + 8)
    W1, db1 = W1_0.clone(), db1_0.clone()
    _call("coati_gnn_edge_pre_bwd", _ptr(dpre), _ptr(g.seg), _ptr(g.e_rev), _ptr(g.e_d2), _ptr(dP), 2 * H, _ptr(W1, 2 * H), 2 * H + 1, _ptr(db1),
          g.BA, H, _stream())
    torch.cuda.synchronize()
    x = dpre[:g.E].double()
    assert float((x.abs() * g.e_d2.double().unsqueeze(1)).sum(0).max()) * 4 + 9 * 4 < 2 ** 24     # quarter-integers: exact in fp32
    rP, rw, rb = U.edge_pre_bwd(x, g.e_bj, g.e_rev, g.e_d2, g.BA)
    assert same(dP, rP.bfloat16()), "dP (receiver sums | reverse-edge sums)"
    want = W1_0.clone()
    want[:, 2 * H] += rw.float()
    assert same(W1, want), "dw1c, or a neighbouring column of the first edge Linear's gradient"
    want = db1_0.clone()
    want[:H] += rb.float()
    assert same(db1, want), "db1"
    if g.E == 0:
        assert bool((dP.view(torch.int16) == 0).all())


# ---- the products whose row count is read on the device ---------------------------------------------------------------------------------
# (graph, N, K, resident): gemm_rb16_resident_supported takes K = 256, N % 16 == 0, N <= 256 at a capacity of >= 4096 rows; every other shape
# runs on the tiled kernel (K = 256 below 4096 rows is too small for the row-block kernels)
GEMM_CASES = [("g1", 256, 256, True), ("g3", 256, 256, True), ("g1", 80, 256, True), ("g1", 128, 128, False), ("g1", 64, 64, False),
              ("pair", 256, 256, False), ("empty", 256, 256, False), ("empty", 128, 128, False)]


@pytest.mark.parametrize("gname,N,K,resident", GEMM_CASES)
def test_gemm_rows_dev_bf16_exact(graphs, gname, N, K, resident):
    """EPI_BF16 on integers: G3 (66 000-odd rows, no multiple of 16) gives a wave of the resident kernel a second slab and a ragged last
    one; N = 80 a partial last 64-column tile"""
    g = graphs[(gname, True)]
    gen = _gen(N + K)
    A, Bw, bias = ints(gen, -2, 2, g.cap, K).bfloat16(), ints(gen, -2, 2, N, K).bfloat16(), ints(gen, -8, 8, N)
    C = sent16(g.cap, N)
    _gemm_rows_dev(g, A, Bw, C, bias, EPI_BF16, N, K, resident)
    assert 4 * K + 8 < 2 ** 24
    ref = (A[:g.E].double() @ Bw.double().t() + bias.double()).bfloat16()
    assert same(C[:g.E], ref[:g.E]) if g.E else True
    assert kept16(C[g.E:]), f"a row past the {g.E} that exist was written"


@pytest.mark.parametrize("gname,N,K,resident", [c for c in GEMM_CASES if c[1] == c[2]])
def test_gemm_rows_dev_edge_dpre(graphs, gname, N, K, resident):
    """EPI_EDGE_DPRE on the resident kernel (H = 256) and on the tiled one (H = 128, 64)"""
    g, H = graphs[(gname, False)], N
    gen = _gen(N)
    P, W1, b1 = edge_params(gen, g.BA, H)
    ds2 = randn(gen, g.cap, H).bfloat16()
    Bw = (randn(gen, H, H) / 16).bfloat16()
    C = sent16(g.cap, H)
    _gemm_rows_dev(g, ds2, Bw, C, None, EPI_EDGE_DPRE, H, H, resident, edge=(P, 2 * H, g.e_d2, _ptr(W1, 2 * H), 2 * H + 1, b1, H))
    bound(f"gemm_rows_dev EDGE_DPRE {gname} H={H} resident={resident}", C[:g.E],
          U.edge_dpre(ds2[:g.E].double(), Bw.double(), P.double(), g.e_bj, g.e_bk, g.e_d2, W1[:, 2 * H].double(), b1.double()))
    assert kept16(C[g.E:])


# launch_wgrad, bf16 A, N = K = 256 (4 tiles of 128 x 128): the LDS-DMA kernel (wgrad_dma_kernel) from a capacity of 16 * 64 * 64 = 65 536 rows
# on, the register-staged kernel (wgrad_kernel) below; both read WgradArgs::m_dev.  g1: the DMA kernel with a count below 65 536; g3: the DMA
# kernel with 66 000-odd rows; small (capacity 20 000, 12 345 rows) and empty (capacity 50, no row): the register-staged kernel
@pytest.mark.parametrize("which,dma", [("g1", True), ("g3", True), ("small", False), ("empty", False)])
def test_wgrad_rows_dev_exact(graphs, which, dma):
    cap, rows = {"g1": (graphs[("g1", True)].cap, graphs[("g1", True)].E), "g3": (graphs[("g3", True)].cap, graphs[("g3", True)].E),
                 "small": (20000, 12345), "empty": (50, 0)}[which]
    assert (cap >= 65536) == dma
    N = K = 256
    gen = _gen(cap)
    A, Bm = ints(gen, -2, 2, cap, N).bfloat16(), ints(gen, -2, 2, cap, K).bfloat16()      # the rows past the count are NOT zero
    dW0, db0 = ints(gen, -9, 9, N, K + 1), ints(gen, -9, 9, N + 8)
    dW, db = dW0.clone(), db0.clone()
    m_dev = torch.tensor([rows], dtype=torch.int32, device=DEV)
    _call("coati_wgrad_rows_dev", _ptr(m_dev), _ptr(A), N, _ptr(Bm), K, cap, N, K, _ptr(dW), K + 1, _ptr(db), _stream())
    torch.cuda.synchronize()
    assert 4 * rows + 9 < 2 ** 24
    rW, rb = U.wgrad(A[:rows].double(), Bm[:rows].double())
    want = dW0.clone()
    want[:, :K] += rW.float()
    assert same(dW, want), "dW, or the untouched column of its odd leading dimension"
    want = db0.clone()
    want[:N] += rb.float()
    assert same(db, want), "dbias"


@pytest.mark.parametrize("BA", [37, 1000, 4480])
@pytest.mark.parametrize("H", [128, 256])
def test_wgrad_split_exact(H, BA):
    """wgrad_table_append_split + launch_wgrad_split_table (wgrad_dma_split_table_kernel, that launch's only kernel) on the engine's node-level problems (gnn_wgrad_group): the two decoder Linears,
    node_mlp.2, node_mlp.0 ([H, 2H] out of a [H, 2H + 28] matrix) and the two dP halves into the first edge Linear's [H, 2H + 1] gradient"""
    gen = _gen(H + BA)
    op = lambda cols: ints(gen, -2, 2, BA, cols).bfloat16()
    do2, td, dtd, hfin, DO16, t, du, hcat, dP = op(H), op(H), op(H), op(H), op(H), op(H), op(H), op(2 * H), op(2 * H)
    g0 = lambda *s: ints(gen, -9, 9, *s)
    Wd3, bd3, Wd0, bd0, Wn3, bn3, Wn0, bn0, We0 = g0(H, H), g0(H), g0(H, H), g0(H), g0(H, H), g0(H), g0(H, 2 * H + 28), g0(H), g0(H, 2 * H + 1)
    outs = [Wd3, bd3, Wd0, bd0, Wn3, bn3, Wn0, bn0, We0]
    before = [o.clone() for o in outs]
    # (A, column offset, lda, B, ldb, N, K, dW, column offset, ldw, dbias)
    probs = [(do2, 0, H, td, H, H, H, Wd3, 0, H, bd3), (dtd, 0, H, hfin, H, H, H, Wd0, 0, H, bd0), (DO16, 0, H, t, H, H, H, Wn3, 0, H, bn3),
             (du, 0, H, hcat, 2 * H, H, 2 * H, Wn0, 0, 2 * H + 28, bn0), (dP, 0, 2 * H, hcat, 2 * H, H, H, We0, 0, 2 * H + 1, None),
             (dP, H, 2 * H, hcat, 2 * H, H, H, We0, H, 2 * H + 1, None)]
    n = len(probs)
    PV, LV, IV = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    Ns, Ks = IV(*[p[5] for p in probs]), IV(*[p[6] for p in probs])
    from coati_amd import _lib
    nbytes = _lib.lib().coati_wgrad_split_workspace_bytes(n, Ns, Ks, 4)
    assert nbytes > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    _call("coati_wgrad_split", n, PV(*[_ptr(p[0], p[1]).value for p in probs]), LV(*[p[2] for p in probs]), PV(*[_ptr(p[3]).value for p in probs]),
          LV(*[p[4] for p in probs]), BA, Ns, Ks, PV(*[_ptr(p[7], p[8]).value for p in probs]), LV(*[p[9] for p in probs]),
          PV(*[(_ptr(p[10]).value if p[10] is not None else None) for p in probs]), 4, _ptr(ws), nbytes, _stream())
    torch.cuda.synchronize()
    assert 4 * BA + 9 < 2 ** 24
    want = [o.clone() for o in before]
    for (A, ao, lda, Bm, ldb, N, K, dW, wo, ldw, db) in probs:
        rW, rb = U.wgrad(A[:, ao:ao + N].double(), Bm[:, :K].double())
        want[[id(o) for o in outs].index(id(dW))][:, wo:wo + K] += rW.float()
        if db is not None:
            want[[id(o) for o in outs].index(id(db))] += rb.float()
    for i, (o, w) in enumerate(zip(outs, want)):
        assert same(o, w), f"output {i} of (Wd3, bd3, Wd0, bd0, Wn3, bn3, Wn0 [H, 2H + 28], bn0, We0 [H, 2H + 1])"


# ---- node level ------------------------------------------------------------------------------------------------------------------------
def _atoms(BA):
    return torch.tensor(ATOMS).repeat(BA // len(ATOMS) + 1)[:BA].to(DEV)


@pytest.mark.parametrize("H", [64, 256])
def test_node_res_silu(H):
    BA = 101
    gen = _gen(H)
    lx, ly = U.luts(DEV)
    atoms = _atoms(BA)
    u = randn(gen, BA, H)
    W3 = randn(gen, H, 2 * H + 28)
    upre, t16 = sent16(BA, H), sent16(BA, H)
    _call("coati_gnn_node_res_silu", _ptr(u), _ptr(atoms), _ptr(lx), _ptr(ly), _ptr(W3, 2 * H), 2 * H + 28, _ptr(upre), _ptr(t16), BA, H, _stream())
    torch.cuda.synchronize()
    v = U.node_res_pre(u.double(), atoms, lx, ly, W3[:, 2 * H:].double())
    bound(f"node_res_silu upre H={H}", upre, v)
    bound(f"node_res_silu t H={H}", t16, U.silu(v))


@pytest.mark.parametrize("BA", [37, 300, 4480])      # one, eight and 128 chunks of atoms
@pytest.mark.parametrize("H", [64, 256])
def test_onehot_wgrad_exact(H, BA):
    gen = _gen(H + BA)
    lx, ly = U.luts(DEV)
    atoms = _atoms(BA)
    du = ints(gen, -3, 3, BA, H).bfloat16()
    W0 = ints(gen, -9, 9, H, 2 * H + 28)
    W = W0.clone()
    _call("coati_gnn_onehot_wgrad", _ptr(atoms), _ptr(lx), _ptr(ly), _ptr(du), _ptr(W, 2 * H), 2 * H + 28, BA, H, _stream())
    torch.cuda.synchronize()
    assert 3 * BA + 9 < 2 ** 24
    want = W0.clone()
    want[:, 2 * H:] += U.onehot_wgrad(atoms, lx, ly, du.double()).float()
    assert same(W, want)


@pytest.mark.parametrize("BA", [37, 300, 4480])      # one, eight and 128 chunks of atoms
@pytest.mark.parametrize("H", [64, 256])
def test_embed_bwd_exact(H, BA):
    """both forms.  One-hot: Z = 92 has no period bit (lut_iy = -1) -- it adds to db and to its group column only, as the forward does.
    Table: Z up to 83 in runs of 20 equal atoms, which cross the 32-row chunks."""
    gen = _gen(H + BA)
    lx, ly = U.luts(DEV)
    atoms = _atoms(BA)
    assert int(ly[92]) == -1 and int(lx[92]) >= 0
    de = ints(gen, -3, 3, BA, H)
    dW0, db0 = ints(gen, -9, 9, H, 28), ints(gen, -9, 9, H)
    dW, db = dW0.clone(), db0.clone()
    _call("coati_gnn_embed_bwd", _ptr(atoms), _ptr(lx), _ptr(ly), _ptr(de), _ptr(dW), _ptr(db), BA, H, _stream())
    torch.cuda.synchronize()
    assert 3 * BA + 9 < 2 ** 24
    rW, rb = U.embed_bwd(atoms, lx, ly, de.double())
    assert same(dW, dW0 + rW.float()) and same(db, db0 + rb.float())
    z = ((torch.arange(BA) // 20 * 7) % 84).to(DEV)
    z[-1] = 83
    assert int(z.max()) == 83 and int(z[31]) == int(z[32])
    T0 = ints(gen, -9, 9, 84, H)
    T = T0.clone()
    _call("coati_gnn_embed_bwd", _ptr(z), None, None, _ptr(de), _ptr(T), None, BA, H, _stream())
    torch.cuda.synchronize()
    assert same(T, T0 + U.embed_table_bwd(z, de.double()).float())


@pytest.mark.parametrize("A", [1, 16, 130])
@pytest.mark.parametrize("H", [64, 320])
def test_readout_and_bwd_exact(H, A):
    """molecules with 0, 1, every power of two up to A, and A real atoms.  Sums of integers are exact; the one division is IEEE fp32 on both
    sides (exact itself for the power-of-two counts)"""
    counts = sorted({0, 1, A} | {2 ** i for i in range(8) if 2 ** i <= A})
    B = len(counts)
    gen = _gen(H + A)
    mask = torch.zeros(B, A, device=DEV)
    for b, c in enumerate(counts):
        mask[b, torch.randperm(A, generator=gen, device=DEV)[:c]] = 1
    o = ints(gen, -4, 4, B, A, H)
    hp = torch.full((B, H), float("nan"), device=DEV)
    _call("coati_gnn_readout", _ptr(o), _ptr(mask), _ptr(hp), B, A, H, _stream())
    torch.cuda.synchronize()
    assert 4 * A < 2 ** 24
    n = mask.sum(1).clamp(min=1).cpu()
    sums = (o * mask.unsqueeze(2)).sum(1).cpu()
    assert same(hp.cpu(), sums / n.unsqueeze(1))                 # (the quotient on the host: IEEE fp32 division)
    p2 = torch.tensor([c & (c - 1) == 0 for c in counts], device=DEV)
    assert same(hp[p2].double(), U.readout(o.double(), mask.double())[p2])
    dhp = ints(gen, -64, 64, B, H)
    dout = sent16(B * A, H)
    _call("coati_gnn_readout_bwd", _ptr(dhp), _ptr(mask), _ptr(dout), B, A, H, _stream())
    torch.cuda.synchronize()
    want = ((dhp.cpu() / n.unsqueeze(1)).unsqueeze(1) * mask.cpu().unsqueeze(2)).bfloat16()
    assert same(dout.view(B, A, H).cpu(), want)
    assert same(dout.view(B, A, H)[p2], U.readout_bwd(dhp.double(), mask.double()).bfloat16()[p2])
