"""A LayerNorm fused into a Linear's operand load saves xhat = (x - mean) * rstd in bf16 instead of its output (include/coati_ln_xhat.h): the
LayerNorm backward in the ring GEMM's write-out reads it in place of f32 x, the grouped weight gradient applies gamma / beta to its finished
tiles.  Operator by operator against fp32 torch, then the engine's step with the save form on against the step with it off."""
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import check, log, rbf  # noqa: E402

DEV = "cuda:0"
TB = 6e-3    # bf16-output tolerance relative to the tensor scale (tests/test_gpu_ops.py)


@pytest.fixture(scope="module")
def ops():
    from coati_amd import ops as o
    return o


# the ends of the one-round ring kernel's row range and a ragged span; the chained product once
@pytest.mark.parametrize("M,K,chain", [(40961, 1024, True), (57344, 256, False), (45000, 768, False)])
def test_gemm_lnbwd_reads_saved_xhat(ops, M, K, chain):
    """coati_gemm_lnbwd_xhat against (a) the fp32 LayerNorm-backward formula evaluated on the SAME bf16-rounded xhat, at the tolerances the
    f32-x form is held to (tests/test_gpu_ops.py: 2e-6 dx, 3e-6 dgamma / dbeta, TB for the bf16 outputs), and (b) exact autograd through
    F.layer_norm at TB: an xhat is off by at most 2^-9 relative and enters dx only through xhat * c2, c2 a mean over the 256 columns."""
    g = torch.Generator().manual_seed(M + K)
    dY = rbf(torch.randn(M, K, generator=g) * 0.5).to(DEV)
    WT = rbf(torch.randn(256, K, generator=g) / math.sqrt(K)).to(DEV)
    x = (torch.randn(M, 256, generator=g) * 1.7 + 0.2).to(DEV)
    gamma = (1 + 0.2 * torch.randn(256, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(256, generator=g)).to(DEV)
    dres = torch.randn(M, 256, generator=g).to(DEV)
    _, _, mean, rstd = ops.layernorm_fwd(x, gamma, beta, want16=True, want32=False)
    xhat16 = ((x - mean[:, None]) * rstd[:, None]).bfloat16()
    xh = xhat16.float()
    dy = dY @ WT.t()                                  # fp32 product of the bf16-valued operands
    gg = dy * gamma
    c1, c2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    ref_dx = rstd[:, None] * (gg - c1 - xh * c2) + dres
    ref_dg, ref_db = (dy * xh).sum(0), dy.sum(0)
    dY16, WT16 = dY.bfloat16(), WT.bfloat16()
    dx, dx16, dg, db = ops.gemm_lnbwd_xhat(dY16, WT16, xhat16, rstd, gamma, dres)
    check(f"gemm+ln bwd (xhat) dx {M}x{K}", dx, ref_dx, 2e-6)
    check(f"gemm+ln bwd (xhat) dx16 {M}x{K}", dx16.float(), ref_dx, TB)
    check(f"gemm+ln bwd (xhat) dgamma {M}x{K}", dg, ref_dg, 3e-6)
    check(f"gemm+ln bwd (xhat) dbeta {M}x{K}", db, ref_db, 3e-6)
    # exact autograd (fp32 xhat)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (256,), gr, br, 1e-5).backward(dy)
    check(f"gemm+ln bwd (xhat) dx vs autograd {M}x{K}", dx, xr.grad + dres, TB)
    check(f"gemm+ln bwd (xhat) dgamma vs autograd {M}x{K}", dg, gr.grad, TB)
    check(f"gemm+ln bwd (xhat) dbeta vs autograd {M}x{K}", db, br.grad, TB)
    # in place (dx = dres, as the engine runs it on the residual-stream gradient) and without the bf16 copy: bit for bit
    dres2 = dres.clone()
    ops.gemm_lnbwd_xhat(dY16, WT16, xhat16, rstd, gamma, dres2, want16=False, out=dres2)
    assert torch.equal(dres2, dx)
    if chain:
        Wc = rbf(torch.randn(256, 256, generator=g) / 16.0).to(DEV)
        dx_c, dx16_c, _, _, ch = ops.gemm_lnbwd_xhat(dY16, WT16, xhat16, rstd, gamma, dres, chain_W=Wc.bfloat16())
        assert torch.equal(dx_c, dx) and torch.equal(dx16_c, dx16)
        check(f"gemm+ln bwd (xhat) chained product {M}x{K}", ch.float(), dx16.float() @ Wc.t(), TB)


@pytest.mark.parametrize("M", [37, 4099])
def test_wgrad_grouped_applies_gamma_and_beta(ops, M):
    """coati_wgrad_grouped_affine on 256-wide tiles: the two LayerNorm-fed Linears of a layer (c_attn [768, 256], c_fc [1024, 256]) with
    gamma / beta, in one table with the two that have none (c_proj, the MLP's c_proj): dW0 + A^T (Xhat gamma + beta) in fp32 at the bound
    of test_wgrad_grouped, pre-filled outputs with an odd leading dimension, db as there."""
    g = torch.Generator().manual_seed(M + 256)
    shapes = [(768, 256, True), (256, 256, False), (1024, 256, True), (256, 1024, False)]
    probs, refs = [], []
    for N, K, aff in shapes:
        A = rbf(torch.randn(M, N, generator=g)).to(DEV)
        X = rbf(torch.randn(M, K, generator=g)).to(DEV)
        ga = (1 + 0.3 * torch.randn(K, generator=g)).to(DEV) if aff else None
        be = (0.3 * torch.randn(K, generator=g)).to(DEV) if aff else None
        dW0 = torch.randn(N, K + 1, generator=g).to(DEV)
        db0 = torch.randn(N, generator=g).to(DEV)
        dW, db = dW0.clone(), db0.clone()
        probs.append((A.bfloat16(), X.bfloat16(), dW[:, :K], db, ga, be))
        refs.append((dW, dW0, db, db0, A, X, ga, be))
    ops.wgrad_grouped_affine(probs, tile_size=256)
    for (N, K, aff), (dW, dW0, db, db0, A, X, ga, be) in zip(shapes, refs):
        inp = X * ga + be if aff else X
        check(f"wgrad_grouped affine={aff} dW {M}x{N}x{K}", dW[:, :K], dW0[:, :K] + A.t() @ inp, 8.5e-6)
        check(f"wgrad_grouped affine={aff} untouched col {M}x{N}x{K}", dW[:, K], dW0[:, K], 0.0)
        check(f"wgrad_grouped affine={aff} db {M}x{N}", db, db0 + A.sum(0), 8.5e-6)


def test_wgrad_grouped_refuses_gamma_beta_where_a_tile_lacks_the_column_sum(ops):
    """gamma / beta on the finished tile need the workgroup that owns it to hold the whole column sum: 256-wide tiles, K = 256.  Anything
    else is an argument error, and nothing is written."""
    M = 37
    def prob(N, K):
        z = lambda *s: torch.zeros(*s, device=DEV)
        return (z(M, N).bfloat16(), z(M, K).bfloat16(), z(N, K), z(N), torch.ones(K, device=DEV), z(K))
    for (N, K), tile in (((768, 256), 128), ((256, 512), 256)):
        p = prob(N, K)
        with pytest.raises(RuntimeError, match="b_gamma"):
            ops.wgrad_grouped_affine([p], tile_size=tile)
        torch.cuda.synchronize()
        assert float(p[2].abs().max()) == 0.0 and float(p[3].abs().max()) == 0.0


@pytest.mark.parametrize("M", [36877, 50003])
def test_fused_forward_saves_either_form_and_computes_the_same(ops, M):
    """coati_gemm_ln_gelu_grad (gemm_rb16.hip, LayerNorm in the slab load, EPI_GELU_GRAD): g, the NewGELU' codes, mean and rstd are the same
    bits whichever copy is saved; the copy is bf16(xhat) or bf16(xhat gamma + beta), each within one bf16 ulp of its fp32 value."""
    N = 1024
    g = torch.Generator().manual_seed(M)
    x = (torch.randn(M, 256, generator=g) * 1.7 + 0.2).to(DEV)
    gamma = (1 + 0.3 * torch.randn(256, generator=g)).to(DEV)
    beta = (0.3 * torch.randn(256, generator=g)).to(DEV)
    W = rbf(torch.randn(N, 256, generator=g) / 16.0).to(DEV).bfloat16()
    bias = (0.1 * torch.randn(N, generator=g)).to(DEV)
    ga, ca, sa, ma, ra = ops.gemm_ln_gelu_grad(x, gamma, beta, W, bias, save_xhat=False)
    gx, cx, sx, mx, rx = ops.gemm_ln_gelu_grad(x, gamma, beta, W, bias, save_xhat=True)
    assert torch.equal(ga, gx) and torch.equal(ca, cx) and torch.equal(ma, mx) and torch.equal(ra, rx)
    xhat = (x - ma[:, None]) * ra[:, None]

    # "the fp32 value" is itself only defined up to the fp32 rounding of the terms it is a difference of (x - mean; xhat gamma + beta with
    # opposite signs: the kernel's fma and torch's multiply-then-add differ by up to 2^-24 of the TERMS, which near a zero of the result
    # is many ulps of the result): that much, 2^-23 of the terms' magnitude, is allowed on top of the one bf16 ulp
    def within_one_ulp(name, saved, ref, terms):
        _, e = torch.frexp(ref.abs().clamp_min(1e-30))            # |ref| = m 2^e, m in [0.5, 1): one bf16 ulp = 2^(e - 8)
        ulp = torch.ldexp(torch.ones_like(ref), e - 8)
        err = (saved.float() - ref).abs()
        rel = (err - terms * 2.0 ** -23).clamp_min(0) / ulp
        worst, at = float(rel.max()), int(rel.argmax())
        log(f"{name} M = {M}: worst |saved - fp32| = {worst:.3f} bf16 ulp (without the fp32 allowance {float((err / ulp).max()):.3f}); "
            f"at element {at}: saved {float(saved.flatten()[at]):.9g} fp32 {float(ref.flatten()[at]):.9g}")
        assert worst <= 1.0, (name, worst)

    t_xhat = (x.abs() + ma[:, None].abs()) * ra[:, None]
    within_one_ulp("fused LN forward, saved xhat", sx, xhat, t_xhat)
    within_one_ulp("fused LN forward, saved LayerNorm output", sa, xhat * gamma + beta, t_xhat * gamma.abs() + (xhat * gamma).abs() + beta.abs())
    # and the product itself against fp32 torch on the bf16 operand
    ref = sa.float() @ W.float().t() + bias
    gelu = 0.5 * ref * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (ref + 0.044715 * ref ** 3)))
    check(f"fused LN forward g {M}", gx.float(), gelu, TB)


_STEP_SCRIPT = """
import sys, torch
sys.path.insert(0, {root!r})
from coati_amd.engine import Engine, ModelConfig
from coati_amd.synthetic import make_batch
kw = dict(n_layer_e3gnn=1, n_layer_xformer=2, n_hidden_xformer=256, n_hidden_e3nn=64, n_embd_common=256, n_head=16, n_seq=100, n_tok=600)
eng = Engine(ModelConfig(**kw), "cuda:0")
g = torch.Generator().manual_seed(11)
with torch.no_grad():
    for name, (off, shape) in eng.layout.items():
        v = eng.view(name)
        if len(shape) == 2:
            v.copy_((torch.randn(shape, generator=g) * (0.05 if "tok_emb" not in name else 1.0)).to("cuda:0"))
        elif ".ln_" in name and name.endswith("weight"):
            v.copy_((1.0 + 0.3 * torch.randn(shape, generator=g)).to("cuda:0"))
        elif ".ln_" in name and name.endswith("bias"):
            v.copy_((0.3 * torch.randn(shape, generator=g)).to("cuda:0"))
        elif name.endswith("clip.0.weight"):
            v.copy_((1.0 + 0.1 * torch.randn(shape, generator=g)).to("cuda:0"))
        else:
            v.copy_((0.02 * torch.randn(shape, generator=g)).to("cuda:0"))
eng.refresh_shadows()
b, up = make_batch(1000, 82, 6, 600, seed=3, n_special=12, min_len=12, with_rows=True)     # ~ 47 000 / 49 000 packed rows
db = {{k: (v.to("cuda:0") if k != "rows" else v) for k, v in b.items()}}
out = {{"rows": b["rows"]}}
for tag, batch in (("packed", db), ("padded", {{k: v for k, v in db.items() if k != "rows"}})):    # padded: 80 000 / 82 000 rows
    eng.train_step(batch, up.to("cuda:0"), lr=1e-3, optimizer=False)
    torch.cuda.synchronize()
    out[tag] = {{"losses": eng.losses(), "xhat": (eng.ln_saves_xhat(0), eng.ln_saves_xhat(1)),
                "grads": {{k: v.cpu().clone() for k, v in eng.named_views("grads").items()}}}}
torch.save(out, {out!r})
"""


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    """the same step (d = 256, two layers, LayerNorm weights 1 + 0.3 randn, biases 0.3 randn) on the packed and on the padded layout, in two
    fresh processes: as the engine runs it, and under COATI_NO_LNBWD_FUSE=1, which keeps the LayerNorm backward out of the GEMM and with it the
    LayerNorm's output in the saved rows"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tmp_path_factory.mktemp("ln_xhat")
    res = {}
    for tag, env in (("xhat", {}), ("a", {"COATI_NO_LNBWD_FUSE": "1"})):
        out = str(d / f"{tag}.pt")
        e = dict(os.environ, **env)
        if tag == "xhat":
            e.pop("COATI_NO_LNBWD_FUSE", None)
        r = subprocess.run([sys.executable, "-c", _STEP_SCRIPT.format(root=root, out=out)], env=e, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = torch.load(out)
    return res


@pytest.mark.parametrize("layout", ["packed", "padded"])
def test_step_with_saved_xhat_equals_step_with_saved_layernorm_output(steps, layout):
    """End to end: every reader of the saved rows -- the LayerNorm backward in the ring GEMM, the grouped weight gradient -- takes them as what
    the forward recorded.  With these LayerNorm weights a reader that took xhat for the LayerNorm's output would be off by tens of percent.
    Bounds of test_layernorm_backward_in_the_gemm_write_out_equals_the_two_kernels: losses 5e-6 relative, gradients 1e-2 of their maximum.
    packed: ~ 47 000 / 49 000 rows, both passes save xhat.  padded: the decoder pass (82 000 rows) runs as two row ranges of the packed-size
    kernels and saves xhat; the encoder pass (80 000 rows: halves of 40 000, below those kernels' range) keeps the 32-row slabs and the
    LayerNorm's output -- the two forms side by side in one step."""
    a, b = steps["xhat"], steps["a"]
    r1, r2 = (int(x) for x in a["rows"])
    assert 40960 < r1 <= 57344 and 40960 < r2 <= 57344, (r1, r2)
    assert b[layout]["xhat"] == (False, False), b[layout]["xhat"]
    assert a[layout]["xhat"] == ((True, True) if layout == "packed" else (False, True)), a[layout]["xhat"]
    la, lb, ga, gb = a[layout]["losses"], b[layout]["losses"], a[layout]["grads"], b[layout]["grads"]
    for k in ("ar_loss", "clip_loss"):
        assert abs(la[k] - lb[k]) <= 5e-6 * abs(lb[k]), (k, la, lb)
    worst = sorted(((float((ga[k] - gb[k]).abs().max()) / max(float(gb[k].abs().max()), 1e-30), k)
                    for k in gb if float(gb[k].abs().max()) > 0), reverse=True)
    log(f"step with saved xhat vs saved LayerNorm output, {layout} ({r1} / {r2} packed rows): worst gradient deviations {worst[:3]}")
    assert worst[0][0] <= 1e-2, worst[:5]
