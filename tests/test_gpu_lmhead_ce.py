"""lm_head cross-entropy with the row statistics kept in registers (gemm_rb16.hip EPI_CE_LSE + ce_lse_finish, ops.ce_lse_fwd) against a
float64 logsumexp of the upcast bf16 operands' product, and against the per-tile path (ops.ce_fwd) on the same inputs.

Inputs: K = 256, bf16 operands from a seeded generator, W ~ 0.5 N(0, 1) so that the logits have sigma = 8 and reach about +-30 (the
running sum is rescaled many times per row).  Column 0 of W is a ramp -1 .. 1 over the vocabulary; row 1 of a is 30 e_0 (logits ascend
with the column: the maximum moves in every tile) and row 2 is -30 e_0 (the maximum sits in tile 0, column 0)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import check, log  # noqa: E402

DEV = "cuda:0"
K = 256
# (M, V): 3 slabs with a partial last one, 2 full tiles + a straddling tile of 18 columns | one slab, one tile | 4 workgroups of 8 waves
# (the starting tile rotates with the workgroup) at the real vocabulary width
SHAPES = [(37, 146), (16, 64), (389, 10322)]
SPLIT_M, SPLIT_V = 82000, 146      # above 65 536 rows: two launches of 41 008 and 40 992 rows (engine.cpp row_split_plan)
_cache = {}


@pytest.fixture(scope="module")
def ops():
    from coati_amd import ops as o
    return o


def case(M, V):
    """inputs (device, bf16), targets and the float64 reference of one shape: made once, shared, never modified"""
    if (M, V) in _cache:
        return _cache[(M, V)]
    g = torch.Generator().manual_seed(1000 * V + M)
    a = torch.randn(M, K, generator=g)
    W = torch.randn(V, K, generator=g) * 0.5
    W[:, 0] = torch.linspace(-1.0, 1.0, V)
    if M > 2:
        a[1].zero_(); a[1, 0] = 30.0
        a[2].zero_(); a[2, 0] = -30.0
    a, W = a.bfloat16(), W.bfloat16()
    tgt = torch.randint(0, V, (M,), generator=g)
    tgt[::5] = -1
    if V % 64:
        straddle0 = V // 64 * 64
        tgt[3], tgt[4], tgt[6] = straddle0, V - 1, 0      # first and last valid column of the straddling tile, column 0
        tgt[M - 1] = V - 1                                # (a row of the partial last slab)
    logits = a.double() @ W.double().t()
    lse = torch.logsumexp(logits, -1)
    valid = tgt >= 0
    idx = torch.arange(M)
    loss_sum = float((lse[valid] - logits[idx[valid], tgt[valid]]).sum())
    c = dict(a=a.to(DEV), W=W.to(DEV), tgt=tgt.to(DEV), tgt_cpu=tgt, logits=logits, lse=lse, loss_sum=loss_sum, count=int(valid.sum()))
    _cache[(M, V)] = c
    return c


def lse_errors(ops, c, name, pick=True):
    new, scal = ops.ce_lse_fwd(c["a"], c["W"], c["tgt"], pick=pick)
    old, _ = ops.ce_fwd(c["a"], c["W"], c["tgt"])
    e_new = float((new.double().cpu() - c["lse"]).abs().max())
    e_old = float((old.double().cpu() - c["lse"]).abs().max())
    msg = f"{name}: lse max abs error vs float64: registers {e_new:.3e}, per-tile {e_old:.3e}, |lse| max {float(c['lse'].abs().max()):.2f}"
    print(msg)
    log(msg)
    return new, scal, e_new, e_old


@pytest.mark.parametrize("pick", [True, False])      # the target logit picked inside the product / recomputed by the finish
@pytest.mark.parametrize("M,V", SHAPES)
def test_ce_lse_vs_float64(ops, M, V, pick):
    c = case(M, V)
    assert float(c["logits"].abs().max()) > 25.0      # the logits do reach the range where the rescale matters
    new, scal, e_new, e_old = lse_errors(ops, c, f"ce_lse M{M} V{V} pick={pick}", pick)
    assert torch.isfinite(new).all()
    # the same terms summed in another order (per-lane chains over all tiles instead of per-tile groups): at most twice the per-tile path's error
    assert e_new <= 2.0 * e_old, (e_new, e_old)
    s = scal.cpu()
    assert int(s[1]) == c["count"]
    check(f"ce_lse loss M{M} V{V} pick={pick}", (s[0].double() / c["count"]).reshape(1), torch.tensor([c["loss_sum"] / c["count"]], dtype=torch.float64), 6e-7)


def test_ce_lse_late_and_early_maxima(ops):
    """row 1: the logits ascend with the column (every tile moves the maximum, the last valid column of the straddling tile holds it); row 2:
    they descend (the maximum is column 0 of tile 0, every later tile only adds small terms)"""
    for M, V in SHAPES[::2]:
        c = case(M, V)
        lg = c["logits"]
        ntiles = (V + 63) // 64
        tile_max = torch.stack([lg[1:3, 64 * j:min(64 * j + 64, V)].max(-1).values for j in range(ntiles)], -1)
        if V == 146:
            assert bool((tile_max[0, 1:] > tile_max[0, :-1]).all())
        assert int(lg[1].argmax()) >= 64 * (ntiles - 1) and int(tile_max[0].argmax()) == ntiles - 1      # (the bf16 ramp has ties at its ends)
        assert int(lg[2].argmax()) < 64 and int(tile_max[1].argmax()) == 0
        new, _ = ops.ce_lse_fwd(c["a"], c["W"], c["tgt"])
        old, _ = ops.ce_fwd(c["a"], c["W"], c["tgt"])
        e_new = (new.double().cpu() - c["lse"]).abs()[1:3]
        e_old = float((old.double().cpu() - c["lse"]).abs().max())
        msg = f"ce_lse M{M} V{V} ascending / descending rows: abs error {float(e_new[0]):.3e} / {float(e_new[1]):.3e} (per-tile path, all rows: {e_old:.3e})"
        print(msg)
        log(msg)
        assert float(e_new.max()) <= 2.0 * e_old, (e_new, e_old)


@pytest.mark.parametrize("M,V", SHAPES)
def test_ce_bwd_from_register_lse(ops, M, V):
    c = case(M, V)
    lse, scal = ops.ce_lse_fwd(c["a"], c["W"], c["tgt"])
    d = ops.ce_bwd(c["a"], c["W"], c["tgt"], lse, scal)
    tgt = c["tgt_cpu"]
    ref = torch.softmax(c["logits"], -1)
    valid = tgt >= 0
    ref[torch.arange(M)[valid], tgt[valid]] -= 1.0
    ref[~valid] = 0.0
    ref /= c["count"]
    check(f"ce_lse dlogits M{M} V{V}", d[:, :V].float().cpu(), ref.float(), 5e-3)
    if d.shape[1] > V:
        assert float(d[:, V:].float().abs().max()) == 0.0


@pytest.mark.parametrize("M", [37, 389])
def test_lmhead_wgrad_split256(ops, M):
    """dW[V, 256] += dlogits[M, Vpad]^T a[M, 256] on 256 x 256 tiles with M split over the workgroups of a tile (gemm.hip
    wgrad256_split_kernel: V = 10 322 gives 41 tiles, the last one half outside Vpad = 10 368).  The padded columns V .. Vpad of dlogits
    hold a sentinel: they must reach neither the gradient nor the memory behind its V rows.  Tolerance: the existing wgrad tests' bound for
    fp32 accumulation over M rows."""
    V = 10322
    c = case(389, V)
    a, tgt = c["a"][:M], c["tgt"][:M]
    lse, scal = ops.ce_lse_fwd(a, c["W"], tgt)
    d = ops.ce_bwd(a, c["W"], tgt, lse, scal).clone()
    Vpad = d.shape[1]
    assert Vpad > V
    d[:, V:] = 1000.0
    g = torch.Generator().manual_seed(M)
    buf = torch.randn(V + 64, K, generator=g).to(DEV)      # dW = its first V rows; the 64 rows behind them must stay as they are
    buf0 = buf.clone()
    ops.wgrad(d, a, buf[:V], n_out=V)
    ref = buf0[:V].double() + d[:, :V].double().t() @ a.double()
    check(f"lmhead wgrad split256 M{M}", buf[:V], ref.float(), 8.5e-6)
    assert torch.equal(buf[V:], buf0[V:])


def test_ce_lse_row_split(ops):
    """82 000 rows through the operator: gemm_rows runs the product as two launches on the row ranges [0, 41 008) and [41 008, 82 000) --
    the same launches as the two halves alone, so lse agrees bit for bit, and the sums add up."""
    c = case(SPLIT_M, SPLIT_V)
    rows = ((SPLIT_M + 1) // 2 + 15) // 16 * 16
    whole, scal, e_new, e_old = lse_errors(ops, c, f"ce_lse row split M{SPLIT_M} V{SPLIT_V}")
    assert e_new <= 2.0 * e_old, (e_new, e_old)
    parts = [ops.ce_lse_fwd(c["a"][r0:r1], c["W"], c["tgt"][r0:r1]) for r0, r1 in ((0, rows), (rows, SPLIT_M))]
    assert torch.equal(whole[:rows], parts[0][0]) and torch.equal(whole[rows:], parts[1][0])
    s = scal.cpu()
    assert int(s[1]) == c["count"] == int(parts[0][1][1]) + int(parts[1][1][1])
    check("ce_lse row split loss vs halves", s[0].reshape(1), (parts[0][1][0] + parts[1][1][0]).cpu().reshape(1), 1.7e-6)
    check("ce_lse row split loss", (s[0].double() / c["count"]).reshape(1), torch.tensor([c["loss_sum"] / c["count"]], dtype=torch.float64), 1.7e-6)
