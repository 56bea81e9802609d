"""The head's input gradient on the GPU: coati_head_grad (csrc/guide.hip) against PropertyHead.reference_grad -- bit for bit on heads whose
sums are exact, its `out` bit for bit coati_head_eval's, within the f32 restatements' own error where only the forward is exact, by the
share of rows within 1e-5 on dense random heads --, its strides and canaries, value_and_grad, fused, and guided_ascent on the kernel.

The launcher has two tiles for F = 64 and F = 128 (one panel per wave while 128-row workgroups are at most one round of the device -- up
to 32 768 rows at F = 128 and 65 536 at F = 64 on 256 CUs --, two from there on) and one for F = 256; N_WIDE rows are past the switch on a
device of up to 273 CUs, every other size here is below it.

Measured on an MI355X (errors per row, max |g - reference_grad64| / max |reference_grad64|):
  exact forward, inexact backward -- rows within 1e-5: 99.60 % (256, 256, 4, 1), 99.50 % (256, 128, 4, 2), 98.90 % (512, 256, 8, 3), 100 % (32, 64, 1, 1),
    98.90 % (64, 128, 16, 8), where the two CPU f32 restatements give 99.60 / 99.60, 99.50 / 99.40, 98.90 / 98.65, 100 / 100 and 98.90 / 99.05 %;
    largest error 2.71e-3 at (512, 256, 8, 3), the restatements' own worst, against the bound 4 x 2.71e-3;
  dense random heads -- rows within 1e-5: 99.05 % (256, 256, 4, 1), 99.35 % (256, 128, 4, 2), 97.10 % (512, 256, 8, 3), 100 % (32, 64, 1, 1), where the CPU
    restatements give 99.10 / 99.30, 99.35 / 99.35, 97.60 / 97.40 and 100 / 100 %; largest errors (flipped masks) 1.5e-2, 8.5e-3, 2.1e-2, 8.4e-8;
  guided_ascent, 512 starts, 20 steps: 100 % of the trajectories climbed, mean gain 0.04576 (float64 autograd run: 0.04562);
  speed (tools/guide_bench.py, E = F = 256, D = 4, P = 1): 0.098 / 0.238 / 3.80 ms at 4096 / 65 536 / 1 M rows, 0.24 / 0.53 / 0.56 of the torch
    bf16 chain with autograd and 1.23 / 1.36 / 1.31 of two coati_head_eval calls."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import guide_util as G  # noqa: E402
from tests import screen_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

EXACT_N = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)
N_WIDE = 70001                      # 547 workgroups of the narrow tile, more than two per CU: the wide tile runs


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ids(s):
    return "x".join(map(str, s))


# ---- 1. exact heads, bit-equal ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.EXACT_SHAPES, ids=_ids)
def test_exact_heads_are_bit_equal(shape):
    E, F, D, P = shape
    head = U.exact_head(E, F, D, P, seed=100 + G.EXACT_SHAPES.index(shape))
    sizes = EXACT_N + (N_WIDE,)
    rows, cot = U.exact_rows(max(sizes), E, seed=7), G.exact_cot(max(sizes), P, seed=8)
    want_out, want_g = head.reference_grad(rows, cot)
    o32, g32 = head.reference_grad(rows[:1000], cot[:1000], torch.float32)                     # exact in any arithmetic
    assert torch.equal(o32.double(), want_out[:1000]) and torch.equal(g32.double(), want_g[:1000])
    want_out, want_g = want_out.float(), want_g.float()
    head = head.to(DEV)
    rows_d, cot_d = rows.to(DEV), cot.to(DEV)
    for n in sizes:
        out, g = head.grad_rows(rows_d[:n], cot_d[:n])
        assert out.shape == (n, P) and g.shape == (n, E) and out.dtype == g.dtype == torch.float32
        bad = (_bits(out.cpu()) != _bits(want_out[:n])).any(dim=1).nonzero().flatten()
        assert bad.numel() == 0, ("out", shape, n, bad[:8].tolist())
        bad = (_bits(g.cpu()) != _bits(want_g[:n])).any(dim=1).nonzero().flatten()
        assert bad.numel() == 0, ("g", shape, n, bad[:8].tolist(), g.cpu()[bad[:2], :8].tolist(), want_g[bad[:2], :8].tolist())


# ---- 2. out is coati_head_eval's out ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_cases():
    """per shape: the head, 2000 unit rows, cotangents, reference_grad64, and of the two CPU f32 restatements (one-piece and 8-chunk K
    sums) the share of rows within 1e-5 of scale and the largest error"""
    from coati_amd.models.regression import PropertyHead
    cases = {}
    for i, (E, F, D, P) in enumerate(G.RANDOM_SHAPES):
        torch.manual_seed(20 + i)
        head = PropertyHead(E, features=F, depth=D, num_outputs=P)
        x = torch.randn(2000, E)
        x16 = (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)
        cot = torch.randn(2000, P)
        _, ref = head.reference_grad(x16, cot)
        cpu = []
        for g32 in (head.reference_grad(x16, cot, torch.float32)[1], G.restate(head, x16, cot, torch.float32, chunks=8)[1]):
            err = G.row_error(g32, ref)
            cpu.append((float((err <= 1e-5).float().mean()), float(err.max())))
        cases[(E, F, D, P)] = (head, x16, cot, ref, cpu)
    return cases


@pytest.mark.parametrize("shape", G.RANDOM_SHAPES, ids=_ids)
def test_out_is_head_evals_out(shape, random_cases):
    """at 2000 rows (the narrow tile where there are two) and at 70001 rows (the wide one), which also shows that a row's results do not
    depend on the tile: the 70001 rows are the 2000 repeated"""
    head, x16, cot, _, _ = random_cases[shape]
    head.to(DEV)
    try:
        x_d, c_d = x16.to(DEV), cot.to(DEV)
        out, g = head.grad_rows(x_d, c_d)
        assert torch.equal(_bits(out), _bits(head.predict_rows(x_d)))
        reps = N_WIDE // 2000 + 1
        xw, cw = x_d.repeat(reps, 1)[:N_WIDE].contiguous(), c_d.repeat(reps, 1)[:N_WIDE].contiguous()
        outw, gw = head.grad_rows(xw, cw)
        assert torch.equal(_bits(outw), _bits(head.predict_rows(xw)))
        assert torch.equal(_bits(outw), _bits(out.repeat(reps, 1)[:N_WIDE])) and torch.equal(_bits(gw), _bits(g.repeat(reps, 1)[:N_WIDE]))
    finally:
        head.cpu()


# ---- 3. exact forward, inexact backward -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ternary_cases():
    cases, worst = {}, 0.0
    for i, (E, F, D, P) in enumerate(G.TERNARY_SHAPES):
        head = G.ternary_head(E, F, D, P, seed=40 + i)
        rows = U.exact_rows(2000, E, seed=50 + i)
        cot = torch.randn(2000, P, generator=torch.Generator().manual_seed(60 + i))
        _, ref, m64 = G.restate(head, rows, cot)
        assert torch.equal(ref, head.reference_grad(rows, cot)[1])
        _, g1, m1 = G.restate(head, rows, cot, torch.float32)
        _, g8, m8 = G.restate(head, rows, cot, torch.float32, chunks=8)
        assert torch.equal(m64, m1) and torch.equal(m64, m8), (E, F, D, P)                     # the masks are the same in any arithmetic
        assert D == 0 or 0.2 < float(m64.float().mean()) < 0.8
        cpu = []
        for g32 in (g1, g8):
            err = G.row_error(g32, ref)
            cpu.append((float((err <= 1e-5).float().mean()), float(err.max())))
            worst = max(worst, float(err.max()))
        cases[(E, F, D, P)] = (head, rows, cot, ref, cpu)
    return cases, worst


@pytest.mark.parametrize("shape", G.TERNARY_SHAPES, ids=_ids)
def test_exact_forward_inexact_backward(shape, ternary_cases):
    """the masks are those of the restatements, so every difference is rounding of d: per row max |g - ref64| / max |ref64| stays within
    4 x the worst error of the two CPU f32 restatements over the five shapes, and the share of rows within 1e-5 within 3 points of theirs"""
    cases, worst = ternary_cases
    head, rows, cot, ref, cpu = cases[shape]
    _, g = head.to(DEV).grad_rows(rows.to(DEV), cot.to(DEV))
    head.cpu()
    err = G.row_error(g.cpu(), ref)
    within, largest = float((err <= 1e-5).float().mean()), float(err.max())
    print(f"head_grad ternary {shape}: rows within 1e-5 of scale {100 * within:.2f} % (CPU f32: {100 * cpu[0][0]:.2f} / {100 * cpu[1][0]:.2f} %), "
          f"largest error {largest:.3g} (CPU f32: {cpu[0][1]:.3g} / {cpu[1][1]:.3g}; bound 4 x {worst:.3g})")
    assert largest <= 4 * worst
    assert within >= min(cpu[0][0], cpu[1][0]) - 0.03


# ---- 4. dense random heads ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.RANDOM_SHAPES, ids=_ids)
def test_random_heads_by_the_share_of_close_rows(shape, random_cases):
    """a rounding of h that falls the other way can flip a mask, a legitimate discrete change of the gradient: the share of rows within
    1e-5 of scale is bounded (the smaller CPU f32 share - 0.03), the largest error is printed"""
    head, x16, cot, ref, cpu = random_cases[shape]
    _, g = head.to(DEV).grad_rows(x16.to(DEV), cot.to(DEV))
    head.cpu()
    err = G.row_error(g.cpu(), ref)
    within, largest = float((err <= 1e-5).float().mean()), float(err.max())
    print(f"head_grad random {shape}: rows within 1e-5 of scale {100 * within:.2f} % (CPU f32: {100 * cpu[0][0]:.2f} / {100 * cpu[1][0]:.2f} %), "
          f"largest error {largest:.3g} (CPU f32: {cpu[0][1]:.3g} / {cpu[1][1]:.3g})")
    assert within >= min(cpu[0][0], cpu[1][0]) - 0.03


# ---- 5. strides and canaries ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 128, 3, 8), (256, 256, 4, 1)], ids=_ids)
def test_strides_and_canaries(shape):
    E, F, D, P = shape
    n, extra, PAT = 300, 5, 0x7FC12345
    torch.manual_seed(4)
    from coati_amd.models.regression import PropertyHead
    head = PropertyHead(E, features=F, depth=D, num_outputs=P).to(DEV)
    x16 = torch.randn(n, E).to(torch.bfloat16).to(DEV)
    cot = torch.randn(n, P).to(DEV)
    out0, g0 = head.grad_rows(x16, cot)
    wide = torch.full((n, E + 8), 7.0, dtype=torch.bfloat16, device=DEV)
    wide[:, :E] = x16
    view = wide[:, :E]
    assert view.stride(0) == E + 8
    o1, g1 = head.grad_rows(view, cot)                                                        # the strided rows are read in place
    assert torch.equal(_bits(o1), _bits(out0)) and torch.equal(_bits(g1), _bits(g0))

    def canary(rows, cols):
        return torch.full((rows, cols), PAT, dtype=torch.int32, device=DEV)

    cot_c, out_c, g_c = canary(n + extra, P + 2), canary(n + extra, P + 3), canary(n + extra, E + 4)
    cot_c.view(torch.float32)[:n, :P] = cot
    U_out, U_g = out_c.view(torch.float32), g_c.view(torch.float32)
    G.head_grad_raw(head, view, cot_c.view(torch.float32), U_out, U_g, n)
    torch.cuda.synchronize()
    assert g_c.stride(0) == E + 4
    assert torch.equal(_bits(U_out[:n, :P]), _bits(out0)) and torch.equal(_bits(U_g[:n, :E]), _bits(g0))
    assert bool((out_c[:n, P:] == PAT).all()) and bool((out_c[n:] == PAT).all())
    assert bool((g_c[:n, E:] == PAT).all()) and bool((g_c[n:] == PAT).all())
    assert bool((cot_c[:n, P:] == PAT).all()) and bool((cot_c[n:] == PAT).all()) and torch.equal(cot_c.view(torch.float32)[:n, :P], cot)


# ---- 6. value_and_grad ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit_input", [False, True])
def test_value_and_grad(unit_input):
    from coati_amd.models.regression import PropertyHead
    from coati_amd.models.regression.property_head import unit_input_chain
    torch.manual_seed(5)
    head = PropertyHead(100, features=128, depth=2, num_outputs=2, unit_input=unit_input).to(DEV)
    x = torch.randn(333, 100)
    cot = torch.randn(333, 2)
    values, grad = head.value_and_grad(x, cot)                                                # f32 vectors on the CPU
    assert values.device.type == "cuda" and values.shape == (333, 2) and grad.shape == (333, 100) and grad.dtype == torch.float32
    assert torch.equal(_bits(values), _bits(head.predict(x)))
    g_rows = head.grad_rows(head.prepare(x), cot.to(DEV))[1][:, :100]
    want = unit_input_chain(g_rows, x.to(DEV)) if unit_input else g_rows
    assert torch.equal(_bits(grad), _bits(want))
    if unit_input:                                                                            # the gradient of a function of x / |x| is orthogonal to x
        assert float((grad.cpu() * x).sum(dim=1).abs().max()) <= 1e-4 * float(grad.abs().max()) * float(x.norm(dim=1).max())
    w = torch.tensor([1.0, -0.5])
    v1, g1 = head.value_and_grad(x, w)
    v2, g2 = head.value_and_grad(x, w[None].expand(333, 2))
    assert torch.equal(_bits(g1), _bits(g2)) and torch.equal(_bits(v1), _bits(values))
    v3, g3 = head.value_and_grad(x)
    v4, g4 = head.value_and_grad(x, torch.ones(333, 2))
    assert torch.equal(_bits(g3), _bits(g4)) and not torch.equal(g3, g1)
    with torch.no_grad():
        head.residuals[0].weight.mul_(0.5)
    v5, g5 = head.value_and_grad(x, cot)                                                      # the operand cache follows _version
    assert not torch.equal(g5, grad) and not torch.equal(v5, values)
    ref_out, ref_g = head.reference_grad(head.prepare(x), cot.to(DEV))
    want5 = ref_g[:, :100].float()
    want5 = unit_input_chain(want5, x.to(DEV)) if unit_input else want5
    assert float((g5 - want5).abs().max()) <= 2e-2 * float(want5.abs().max())                 # (loose: the tight checks are tests 1 to 4)


# ---- 7. fused ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit_input", [False, True])
def test_fused_is_predict_with_a_gradient_for_x_only(unit_input):
    from coati_amd.models.regression import PropertyHead
    torch.manual_seed(6)
    head = PropertyHead(100, features=128, depth=2, num_outputs=2, unit_input=unit_input).to(DEV)
    x = torch.randn(77, 100, device=DEV, requires_grad=True)
    c = torch.tensor([1.0, -0.5], device=DEV)
    y = head.fused(x)
    assert y.requires_grad and torch.equal(_bits(y.detach()), _bits(head.predict(x)))
    (y * c).sum().backward()
    assert torch.equal(_bits(x.grad), _bits(head.value_and_grad(x, c)[1]))
    assert all(p.grad is None for p in head.parameters())


# ---- 8. guided_ascent on the kernel ---------------------------------------------------------------------------------------------
def test_guided_ascent_on_the_kernel():
    """20 steps of lr = 0.01 from 512 starts: every trajectory of the float64 autograd run climbs; of the kernel-driven run at least 99 %"""
    from coati_amd.generative import guided_ascent
    from coati_amd.models.regression import PropertyHead
    torch.manual_seed(12)
    head = PropertyHead(256, features=256, depth=4, num_outputs=2)
    start = torch.randn(512, 256)
    w = [1.0, -0.5]
    head.double()
    cpu = guided_ascent(start.double(), head, weights=w, steps=20, lr=0.01, value_and_grad=G.autograd_value_and_grad(head))
    head.float()
    assert bool((cpu.history[-1] > cpu.history[0]).all())
    head.to(DEV)
    start_d = start.to(DEV)
    one = guided_ascent(start_d, head, weights=w, steps=1, lr=0.01)
    assert one.vectors.device.type == "cuda" and one.vectors.dtype == torch.float32
    want = start_d + 0.01 * head.value_and_grad(start_d, torch.tensor(w))[1]
    assert torch.equal(_bits(one.vectors), _bits(want))
    run = guided_ascent(start_d, head, weights=w, steps=20, lr=0.01)
    again = guided_ascent(start_d, head, weights=w, steps=20, lr=0.01)
    assert torch.equal(_bits(run.vectors), _bits(again.vectors)) and torch.equal(_bits(run.history), _bits(again.history))
    climbed = float((run.history[-1] > run.history[0]).float().mean())
    print(f"guided_ascent: {100 * climbed:.2f} % of 512 trajectories climbed; mean gain {float((run.history[-1] - run.history[0]).mean()):.4g} "
          f"(float64 autograd run: {float((cpu.history[-1] - cpu.history[0]).mean()):.4g})")
    assert climbed >= 0.99
    assert run.history.shape == (21, 512) and torch.equal(_bits(run.values), _bits(head.predict(run.vectors)))
    hills = guided_ascent(start_d, head, weights=w, steps=11, lr=0.01, bump_every=5, bump_height=0.5, bump_width=0.3)
    assert hills.n_centres == 2
    five = guided_ascent(start_d, head, weights=w, steps=5, lr=0.01, bump_every=5, bump_height=0.5, bump_width=0.3)
    assert torch.equal(_bits(hills.centres[:, 0]), _bits(five.vectors))                       # the centres are the visited vectors
    ten = guided_ascent(start_d, head, weights=w, steps=10, lr=0.01, bump_every=5, bump_height=0.5, bump_width=0.3)
    assert torch.equal(_bits(hills.centres[:, 1]), _bits(ten.vectors))
    assert not torch.equal(ten.vectors, guided_ascent(start_d, head, weights=w, steps=10, lr=0.01).vectors)       # and the hills push
