"""The acquisition gradient on the GPU: coati_head_gp_grad (csrc/gp_grad.hip) against GPHead.reference_acq_grad -- its forward bit for bit
coati_head_gp's, its gradient by the share of rows within 1e-5 of scale on dense random heads and within the f32 restatements' own error
where the forward is exact --, ragged sizes and the two tiles, strides and canaries, padded inducing points, AcquisitionObjective,
fused, guided_ascent and guided_generation on the kernel.

The launcher has launch_head_grad's two tiles for F = 64 and F = 128 (one panel per wave while 128-row workgroups are at most one round of
the device, two from there on) and one for F = 256; N_WIDE rows are past the switch on a device of up to 273 CUs.

The threshold of "close" rows is test_gpu_guide.py's 1e-5 of scale wherever both CPU f32 restatements alone keep at least 0.9 of their rows
within it: the smallest share is 0.9435 at (256, 256, 4, 1, 60), ei.  At (512, 256, 16, 3, 64) they do not: 17 masked bf16 operands of 256
values per row leave them 0.22 .. 0.60 of their rows within 1e-5, 0.28 .. 0.53 within 1e-4 and 0.78 .. 0.86 within 1e-3; the first decade at
which both reach 0.9 is 1e-2 (0.9955 .. 0.9965), so that shape is judged at 1e-2 (acq_util.THRESHOLDS) and its largest errors by test 3.

Measured on an MI355X (errors per row, max |g - reference64| / max |reference64|; the four cases are ucb, lcb+noise+rs, ei, ei+noise+rs):
  acq against acquisition_values in f32: at most 4.77e-7, (96, 128, 2, 2, 32) lcb+noise+rs, against 4 ulp of scale = 2.23e-6;
  dense random heads -- rows within 1e-5: 100 / 99.90 / 99.95 / 99.90 % (32, 64, 1, 1, 8), 99.35 / 99.40 / 99.35 / 99.30 % (96, 128, 2, 2, 32),
    99.00 / 99.15 / 99.00 / 99.20 % (64, 128, 3, 8, 33), 95.00 / 95.45 / 94.45 / 94.60 % (256, 256, 4, 1, 60), where the two CPU restatements give
    99.95 .. 100, 99.00 .. 99.60, 98.70 .. 99.40 and 96.40 .. 97.10 %; within 1e-2: 99.15 / 99.65 / 99.50 / 99.50 % (512, 256, 16, 3, 64), the
    restatements 99.25 .. 99.70 %; largest errors 1.5e-3, 4.5e-3, 2.2e-3, 7.8e-3, 2.1e-2 (the restatements': 1.5e-3, 1.4e-3, 1.8e-3, 7.8e-3, 2.2e-2);
  ternary extractors -- largest error 3.1e-5, 6.2e-4, 8.0e-4, 2.1e-3, 4.3e-3 per shape, the restatements' worst 4.46e-3, against the bound 4 x that;
  guided_ascent on ucb, 512 starts, 20 steps: 100 % of the trajectories climbed, mean gain 3.875 (float64 run on the reference: 100 %, 3.875);
  speed (tools/acq_bench.py, E = F = 256, D = 4, P = 1, M = 60): 0.101 / 0.229 / 3.60 ms at 4096 / 65 536 / 1 M rows, 0.69 / 0.68 / 0.68 of
    coati_head_gp + coati_head_grad back to back and 0.10 / 0.22 / 0.29 of a torch bf16 chain with autograd."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import acq_util as A  # noqa: E402
from tests import gp_util as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_WIDE = 70001                      # 547 workgroups of the narrow tile, more than two per CU: the wide tile runs
RAGGED_N = (1, 31, 32, 33, 127, 128, 129, 257, 1000)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def random_cases():
    return {shape: A.random_case(shape, i) for i, shape in enumerate(A.SHAPES)}


@pytest.fixture(scope="module")
def ternary_cases():
    cases = {shape: A.ternary_case(shape, i) for i, shape in enumerate(A.SHAPES)}
    worst = max(e for _, _, per in cases.values() for _, _, cpu in per for _, e in cpu)
    return cases, worst


# ---- 1. the forward is undisturbed --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", A.SHAPES, ids=A.ids)
def test_forward_is_head_gps_forward(shape, random_cases):
    """mean is coati_head_gp's on any head, bit for bit; var too on the head whose q is symmetric; acq is acquisition_values in f32 on
    the kernel's own mean and var, within 4 ulp of max(|mean|, |kappa| sqrt(s2))"""
    from coati_amd.models.regression import GPHead, acquisition_values
    gp, x16, per = random_cases[shape]
    sym = GPHead(gp.extractor, gp.z, gp.alpha, (0.5 * (gp.q + gp.q.T)).float().double(), gp.const, gp.lengthscale, gp.signal_var,
                 gp.noise_var).to(DEV)
    gp.to(DEV)
    try:
        x_d = x16.to(DEV)
        mean0, _ = gp.gp_rows(x_d)
        means, vars_ = sym.gp_rows(x_d)
        assert torch.equal(_bits(means), _bits(mean0))
        for case, ref, _ in per:
            name, wm, kappa, var_add, mode, best, rs = case
            mean, var, acq, g = A.run_case(gp, x_d, case)
            assert mean.shape == (2000, shape[3]) and var.shape == acq.shape == (2000,) and g.shape == (2000, shape[0])
            assert torch.equal(_bits(mean), _bits(mean0)), (shape, name)
            ms, vs, as_, gs = A.run_case(sym, x_d, case)
            assert torch.equal(_bits(ms), _bits(means)) and torch.equal(_bits(vs), _bits(vars_)), (shape, name)
            assert _same((ms, vs, as_, gs), (mean, var, acq, g))                                  # qs of q is qs of its symmetric part
            m = mean[:, shape[3] - 1]
            std = (var + A.f32_scalar(var_add)).sqrt()
            if mode == 0:
                want = acquisition_values(m, std, "ucb", kappa)
            else:
                want = acquisition_values(m, A.f32_scalar(kappa) * std, "ei", best=A.f32_scalar(best))
            scale = max(float(m.abs().max()), abs(kappa) * gp.signal_var ** 0.5)
            err = float((acq - want).abs().max())
            print(f"acq {shape} {name}: largest |acq - acquisition_values| {err:.3g}, 4 ulp of scale {4 * scale * 2 ** -23:.3g}")
            assert err <= 4 * scale * 2.0 ** -23, (shape, name)
    finally:
        gp.cpu()


# ---- 2. the gradient against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", A.SHAPES, ids=A.ids)
def test_gradient_by_the_share_of_close_rows(shape, random_cases):
    """dense random heads: a rounding of h that falls the other way can flip a mask, a legitimate discrete change of the gradient, so the
    share of rows within 1e-5 of scale is bounded (the smaller CPU f32 share - 0.03) and the largest error printed.  var spans
    (0.05 s2, s2) by construction: no clamp decision can flip.  Both modes, var_add = 0 and noise_var, with and without rs."""
    gp, x16, per = random_cases[shape]
    gp.to(DEV)
    try:
        x_d = x16.to(DEV)
        for case, ref, cpu in per:
            assert min(cpu[0][0], cpu[1][0]) >= 0.9, (shape, case[0], cpu)                         # the threshold is meaningful on the CPU
            assert float(ref[1].min()) > 0.02 * gp.signal_var
            _, _, _, g = A.run_case(gp, x_d, case)
            err = A.row_error(g.cpu(), ref[3])
            within, largest = float((err <= A.threshold(shape)).float().mean()), float(err.max())
            print(f"head_gp_grad random {shape} {case[0]}: rows within {A.threshold(shape):g} of scale {100 * within:.2f} % (CPU f32: {100 * cpu[0][0]:.2f} / "
                  f"{100 * cpu[1][0]:.2f} %), largest error {largest:.3g} (CPU f32: {cpu[0][1]:.3g} / {cpu[1][1]:.3g})")
            assert within >= min(cpu[0][0], cpu[1][0]) - 0.03, (shape, case[0])
    finally:
        gp.cpu()


# ---- 3. exact-forward heads -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", A.SHAPES, ids=A.ids)
def test_exact_forward_heads(shape, ternary_cases):
    """ternary extractors under a GP: the masks are those of the restatements (asserted where the cases are built), so every difference is
    rounding: the largest row error stays within 4 x the worst of the two CPU f32 restatements over the shapes, the factor
    test_gpu_guide.py's test_exact_forward_inexact_backward uses"""
    cases, worst = ternary_cases
    gp, x16, per = cases[shape]
    gp.to(DEV)
    try:
        x_d = x16.to(DEV)
        for case, ref, cpu in per:
            _, _, _, g = A.run_case(gp, x_d, case)
            err = A.row_error(g.cpu(), ref[3])
            within, largest = float((err <= A.threshold(shape)).float().mean()), float(err.max())
            print(f"head_gp_grad ternary {shape} {case[0]}: rows within {A.threshold(shape):g} of scale {100 * within:.2f} % (CPU f32: {100 * cpu[0][0]:.2f} / "
                  f"{100 * cpu[1][0]:.2f} %), largest error {largest:.3g} (CPU f32: {cpu[0][1]:.3g} / {cpu[1][1]:.3g}; bound 4 x {worst:.3g})")
            assert largest <= 4 * worst, (shape, case[0])
    finally:
        gp.cpu()


# ---- 4. ragged sizes and tiles --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", A.SHAPES, ids=A.ids)
def test_ragged_sizes_and_tiles(shape, random_cases):
    """the first n rows give the 2000-row run's bits at every n, and 70001 rows (the 2000 repeated; the wide tile where there are two) the
    repeats' bits: a row's results depend neither on the rows around it nor on the tile"""
    gp, x16, per = random_cases[shape]
    gp.to(DEV)
    try:
        x_d = x16.to(DEV)
        case = per[3][0]                                                                        # ei, noise, rs: every operand in play
        full = A.run_case(gp, x_d, case)
        for n in RAGGED_N:
            part = A.run_case(gp, x_d[:n], case)
            assert part[3].shape == (n, shape[0]) and _same(part, [t[:n] for t in full]), (shape, n)
        reps = N_WIDE // 2000 + 1
        xw = x_d.repeat(reps, 1)[:N_WIDE].contiguous()
        _, wm, kappa, var_add, mode, best, rs = case
        wide = gp.acq_rows(xw, wm, kappa, var_add, mode, best, rs.to(DEV).repeat(reps)[:N_WIDE].contiguous())
        torch.cuda.synchronize()
        assert _same(wide, [t.repeat(reps, *([1] * (t.dim() - 1)))[:N_WIDE] for t in full]), shape
    finally:
        gp.cpu()


# ---- 5. strides, canaries, padded inducing points ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 128, 3, 8, 33), (256, 256, 4, 1, 60)], ids=A.ids)
def test_strides_and_canaries(shape, random_cases):
    E, F, D, P, M = shape
    gp, x16, per = random_cases[shape]
    n, extra, PAT = 300, 5, 0x7FC12345
    gp.to(DEV)
    try:
        case = per[1][0]                                                                        # lcb, noise, rs
        x_d = x16[:n].to(DEV)
        rs = case[6][:n].to(DEV)
        want = A.run_case(gp, x_d, case)
        wide = torch.full((n, E + 8), 7.0, dtype=torch.bfloat16, device=DEV)
        wide[:, :E] = x_d
        view = wide[:, :E]
        assert view.stride(0) == E + 8
        assert _same(A.run_case(gp, view, case), want)                                          # the strided rows are read in place

        def canary(*shape_):
            return torch.full(shape_, PAT, dtype=torch.int32, device=DEV)

        mean_c, var_c, acq_c, g_c, rs_c = canary(n + extra, P + 3), canary(n + extra), canary(n + extra), canary(n + extra, E + 4), canary(n + extra)
        rs_c.view(torch.float32)[:n] = rs
        f = [t.view(torch.float32) for t in (mean_c, var_c, acq_c, g_c)]
        A.head_gp_grad_raw(gp, view, case, f[0], f[1], f[2], f[3], n, rs=rs_c.view(torch.float32))
        assert g_c.stride(0) == E + 4 and mean_c.stride(0) == P + 3
        assert _same((f[0][:n, :P], f[1][:n], f[2][:n], f[3][:n, :E]), want)
        assert bool((mean_c[:n, P:] == PAT).all()) and bool((mean_c[n:] == PAT).all())
        assert bool((g_c[:n, E:] == PAT).all()) and bool((g_c[n:] == PAT).all())
        assert bool((var_c[n:] == PAT).all()) and bool((acq_c[n:] == PAT).all())
        assert bool((rs_c[n:] == PAT).all()) and torch.equal(rs_c.view(torch.float32)[:n], rs)
    finally:
        gp.cpu()


@pytest.mark.parametrize("M", [31, 33, 60])
def test_padded_inducing_rows_do_not_matter(M):
    """the rows of z (and columns of zt) past M random against zero: the same bits.  31 is the last M before the Mp switch."""
    gp, x16 = G.random_gp(64, 128, 2, 2, M, seed=700 + M, n=500)
    cases = A.acq_cases(gp, x16, seed=M)
    gp.to(DEV)
    x_d = x16.to(DEV)
    Mp = 32 if M <= 32 else 64
    for case in cases:
        want = A.run_case(gp, x_d, case)
        z = gp._gp_operands()[0].clone()
        assert z.shape == (Mp, 128) and bool((z[M:] == 0).all())
        z[M:] = torch.randn(Mp - M, 128, generator=torch.Generator().manual_seed(M)).to(torch.bfloat16).to(DEV)
        out = [torch.empty_like(t) for t in want]
        A.head_gp_grad_raw(gp, x_d, case, out[0], out[1], out[2], out[3], 500, z=z)
        assert _same(out, want), (M, case[0])


# ---- 6. the objective on the kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit_input", [False, True])
def test_objective_on_the_kernel(unit_input):
    from coati_amd.models.regression import GPHead, acquisition_values
    from coati_amd.models.regression.property_head import unit_input_chain
    gp, x16 = G.random_gp(100, 128, 2, 2, 40, seed=800, n=333, unit_input=unit_input)
    gp = GPHead(gp.extractor, gp.z, gp.alpha, gp.q, gp.const, gp.lengthscale, gp.signal_var, gp.noise_var, [0.3, -0.2], [1.5, 2.5]).to(DEV)
    x = x16.float() * (0.5 + torch.rand(333, 1, generator=torch.Generator().manual_seed(1)))     # f32 vectors on the CPU
    mean, std = gp.predict_with_std(x, include_noise=True)
    best = float(mean[:, 1].median())
    for kind in ("mean", "ucb", "lcb", "ei"):
        obj = gp.acquisition(kind, beta=1.3, best=best if kind == "ei" else None, output=1, include_noise=True)
        values, grad = obj.value_and_grad(x)
        assert values.device.type == "cuda" and values.shape == (333, 1) and grad.shape == (333, 100) and grad.dtype == torch.float32
        assert torch.equal(_bits(values), _bits(obj.predict(x)))
        want = acquisition_values(mean[:, 1], std[:, 1], kind, 1.3, best)
        assert float((values[:, 0] - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max())), kind
        g_rows = obj.acq_rows(obj.prepare(x))[3][:, :100]
        want_g = unit_input_chain(g_rows, x.to(DEV)) if unit_input else g_rows
        assert torch.equal(_bits(grad), _bits(want_g))
        if unit_input:                                                                          # orthogonal to x
            assert float((grad.cpu() * x).sum(dim=1).abs().max()) <= 1e-4 * float(grad.abs().max()) * float(x.norm(dim=1).max())
        v1, g1 = obj.value_and_grad(x, torch.tensor([-0.5]))
        v2, g2 = obj.value_and_grad(x, torch.full((333, 1), -0.5))
        assert torch.equal(_bits(g1), _bits(g2)) and torch.equal(_bits(v1), _bits(values)) and not torch.equal(g1, grad)
        assert torch.equal(_bits(obj.value_and_grad(x, torch.ones(1))[1]), _bits(grad))
        xg = x.to(DEV).requires_grad_(True)
        y = obj.fused(xg)
        assert y.requires_grad and torch.equal(_bits(y.detach()), _bits(values))
        y.sum().backward()
        assert torch.equal(_bits(xg.grad), _bits(grad))
        assert all(p.grad is None for p in gp.parameters()) and all(b.grad is None for b in gp.buffers())
    obj = gp.acquisition("ucb", beta=1.3, output=1)
    before = obj.value_and_grad(x)
    gp.alpha.mul_(0.5)                                                                            # the operand cache follows _version
    after = obj.value_and_grad(x)
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1])
    gp.q.mul_(0.5)
    assert not torch.equal(obj.value_and_grad(x)[1], after[1])
    with pytest.raises(NotImplementedError, match="extractor"):
        gp.value_and_grad(x)


# ---- 7. guided_ascent and guided_generation on the kernel ---------------------------------------------------------------------------------
def test_guided_ascent_on_the_kernel():
    """512 starts, 20 steps of lr = 0.01 on ucb with beta = 1: the share of trajectories whose acquisition rose is at least that of the
    float64 run on the reference (the straight-through model's gradient, test_acq_cpu.py) minus 0.01"""
    from coati_amd.generative import guided_ascent
    gp, x16 = G.random_gp(256, 256, 4, 1, 60, seed=900, n=512)
    obj = gp.acquisition("ucb", beta=1.0)
    start = x16.float()
    cpu = guided_ascent(start.double(), obj, steps=20, lr=0.01, value_and_grad=A.reference_value_and_grad(obj))
    want = float((cpu.history[-1] > cpu.history[0]).float().mean())
    gp.to(DEV)
    start_d = start.to(DEV)
    with pytest.raises(TypeError, match="extractor"):
        guided_ascent(start_d, gp, steps=1)
    one = guided_ascent(start_d, obj, steps=1, lr=0.01)
    assert one.vectors.device.type == "cuda" and one.vectors.dtype == torch.float32
    assert torch.equal(_bits(one.vectors), _bits(start_d + 0.01 * obj.value_and_grad(start_d, torch.ones(1))[1]))
    run = guided_ascent(start_d, obj, steps=20, lr=0.01)
    again = guided_ascent(start_d, obj, steps=20, lr=0.01)
    assert torch.equal(_bits(run.vectors), _bits(again.vectors)) and torch.equal(_bits(run.history), _bits(again.history))
    climbed = float((run.history[-1] > run.history[0]).float().mean())
    print(f"guided_ascent on ucb: {100 * climbed:.2f} % of 512 trajectories climbed (float64 reference run: {100 * want:.2f} %); mean gain "
          f"{float((run.history[-1] - run.history[0]).mean()):.4g} (float64 reference run: {float((cpu.history[-1] - cpu.history[0]).mean()):.4g})")
    assert climbed >= want - 0.01
    assert run.history.shape == (21, 512) and run.values.shape == (512, 1) and torch.equal(_bits(run.values), _bits(obj.predict(run.vectors)))
    hills = guided_ascent(start_d, obj, steps=11, lr=0.01, anchor=0.2, bump_every=5, bump_height=0.5, bump_width=0.3)
    assert hills.n_centres == 2
    five = guided_ascent(start_d, obj, steps=5, lr=0.01, anchor=0.2, bump_every=5, bump_height=0.5, bump_width=0.3)
    assert torch.equal(_bits(hills.centres[:, 0]), _bits(five.vectors))                         # the centres are the visited vectors
    ten = guided_ascent(start_d, obj, steps=10, lr=0.01, anchor=0.2, bump_every=5, bump_height=0.5, bump_width=0.3)
    assert torch.equal(_bits(hills.centres[:, 1]), _bits(ten.vectors))
    assert not torch.equal(ten.vectors, guided_ascent(start_d, obj, steps=10, lr=0.01, anchor=0.2).vectors)       # the hills push
    assert not torch.equal(guided_ascent(start_d, obj, steps=10, lr=0.01, anchor=0.2).vectors,
                           guided_ascent(start_d, obj, steps=10, lr=0.01).vectors)               # and the anchor holds


def test_guided_generation_orders_by_the_objective():
    from coati_amd.generative import guided_generation
    gp, x16 = G.random_gp(64, 128, 2, 2, 20, seed=901, n=40)
    gp.to(DEV)
    obj = gp.acquisition("lcb", beta=2.0, output=1)
    start = x16.float()

    def decode(V):                                               # every fifth end point does not decode; the name is the row number
        decode.kept = V.detach().clone()
        return [None if i % 5 == 4 else f"m{i}" for i in range(V.shape[0])]

    def embed(strings):                                          # a decoded molecule is (here) another library row, not the vector it came from
        return torch.stack([start[(7 * int(s[1:]) + 3) % 40] for s in strings])

    recs = guided_generation(start, obj, None, None, steps=5, lr=0.01, anchor=0.1, decode=decode, embed=embed)
    assert len(recs) == 32 and all(isinstance(r["start"], int) and r["start"] % 5 != 4 for r in recs)
    values = [r["decoded_value"] for r in recs]
    assert values == sorted(values, reverse=True)
    again = obj.predict(embed([r["smiles"] for r in recs]))[:, 0].cpu().tolist()
    assert values == again
    first = obj.predict(start)[:, 0].cpu().tolist()
    last = obj.predict(decode.kept)[:, 0].cpu().tolist()
    for r in recs:
        assert r["start_value"] == first[r["start"]] and r["vector_value"] == last[r["start"]]
