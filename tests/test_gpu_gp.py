"""The GP head on the GPU: coati_head_gp (csrc/gp.hip) against GPHead.reference within the summation-order error of f32, ragged tiles,
strides and canaries, the shared forward bit for bit against coati_head_eval, padding, and the consumers: EmbeddingIndex's
property_uncertainty / screen(acquisition=), sampled_virtual_screen(beta=) and fit_gp_head end to end.

Measured on an MI355X (mean error of max |mean| / var error of s2; bound 4 x 4.73e-4 / 4 x 9.08e-4 from the CPU f32 restatements):
(32, 64, 0, 1, 1) 1.1e-5 / 1.2e-6, (32, 64, 1, 1, 32) 4.1e-7 / 2.8e-7, (64, 128, 3, 8, 33) 5.9e-4 / 1.1e-3, (256, 256, 4, 1, 60)
3.8e-4 / 8.4e-4, (512, 256, 2, 3, 64) 5.4e-4 / 9.1e-4; the fit on the device: mean 5.9e-6 (bound 4 x 5.7e-6), std 1.7e-4 (bound 4.3e-4)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import gp_util as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")

SHAPES = [(32, 64, 0, 1, 1), (32, 64, 1, 1, 32), (64, 128, 3, 8, 33), (256, 256, 4, 1, 60), (512, 256, 2, 3, 64)]   # (E, F, D, P, M)
RAGGED_SHAPES = [(64, 128, 3, 8, 33), (256, 256, 4, 1, 60)]
RAGGED_N = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1000)
IDS = lambda s: "x".join(map(str, s))  # noqa: E731


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. against float64 ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    """per shape: the GP head, its 2000 unit rows, reference64; and the worst error of two CPU f32 restatements over all shapes"""
    out, worst_mean, worst_var = {}, 0.0, 0.0
    for i, shape in enumerate(SHAPES):
        gp, x16 = G.random_gp(*shape, seed=200 + i)
        ref_mean, ref_var = gp.reference(x16)
        em, ev, pairs = G.restatement_errors(gp, x16, ref_mean, ref_var)
        print(f"head_gp {shape}: CPU f32 restatements: mean {pairs[0][0]:.3g} / {pairs[1][0]:.3g} of max |mean|, var {pairs[0][1]:.3g} / "
              f"{pairs[1][1]:.3g} of s2; var in {float(ref_var.min()) / gp.signal_var:.3g} .. {float(ref_var.max()) / gp.signal_var:.3g} of s2")
        worst_mean, worst_var = max(worst_mean, em), max(worst_var, ev)
        out[shape] = (gp, x16, ref_mean, ref_var)
    return out, worst_mean, worst_var


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_against_float64(shape, cases):
    table, worst_mean, worst_var = cases
    gp, x16, ref_mean, ref_var = table[shape]
    gp.to(DEV)
    mean, var = gp.gp_rows(x16.to(DEV))
    mean, var = mean.cpu(), var.cpu()
    gp.cpu()
    assert mean.shape == ref_mean.shape and var.shape == ref_var.shape and mean.dtype == var.dtype == torch.float32
    em, ev = G.errors(gp, mean, var, ref_mean, ref_var)
    print(f"head_gp {shape}: mean error {em:.3g} of max |mean| (bound 4 x {worst_mean:.3g}), var error {ev:.3g} of s2 (bound 4 x {worst_var:.3g})")
    assert float(ref_var.min()) < 0.5 * gp.signal_var and float(ref_var.max()) > 0.5 * gp.signal_var     # var spans its range
    assert em <= 4 * worst_mean
    assert ev <= 4 * worst_var


# ---- 2. ragged tiles ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RAGGED_SHAPES, ids=IDS)
def test_ragged_tiles_are_bit_equal(shape, cases):
    gp, x16, _, _ = cases[0][shape]
    gp.to(DEV)
    rows = x16[:1000].to(DEV)
    mean_all, var_all = gp.gp_rows(rows)
    for n in RAGGED_N:
        mean, var = gp.gp_rows(rows[:n])
        assert mean.shape == (n, shape[3]) and var.shape == (n,)
        assert torch.equal(_bits(mean), _bits(mean_all[:n])) and torch.equal(_bits(var), _bits(var_all[:n])), (shape, n)
    gp.cpu()


# ---- 3. strides and canaries ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RAGGED_SHAPES, ids=IDS)
def test_strides_and_canaries(shape, cases):
    E, F, D, P, M = shape
    gp, x16, _, _ = cases[0][shape]
    gp.to(DEV)
    n, extra = 300, 5
    rows = x16[:n].to(DEV)
    plain_mean, plain_var = gp.gp_rows(rows)
    wide = torch.full((n, E + 8), 7.0, dtype=torch.bfloat16, device=DEV)
    wide[:, :E] = rows
    view = wide[:, :E]
    assert view.stride(0) == E + 8
    m2, v2 = gp.gp_rows(view)                                                                  # the strided rows are read in place
    assert torch.equal(_bits(m2), _bits(plain_mean)) and torch.equal(_bits(v2), _bits(plain_var))
    cm = torch.empty(n + extra, P + 3, dtype=torch.int32, device=DEV).fill_(0x7FC12345)         # a NaN pattern
    cv = torch.empty(n + extra, dtype=torch.int32, device=DEV).fill_(0x7FC12345)
    co = torch.empty(n + extra, gp.extractor.num_outputs + 2, dtype=torch.int32, device=DEV).fill_(0x7FC12345)
    G.head_gp_raw(gp, view, cm.view(torch.float32), cv.view(torch.float32), n, out=co.view(torch.float32))
    torch.cuda.synchronize()
    assert torch.equal(cm[:n, :P], _bits(plain_mean)) and torch.equal(cv[:n], _bits(plain_var))
    assert bool((cm[:n, P:] == 0x7FC12345).all()) and bool((cm[n:] == 0x7FC12345).all()) and bool((cv[n:] == 0x7FC12345).all())
    PL = gp.extractor.num_outputs
    assert torch.equal(co[:n, :PL], _bits(gp.extractor.predict_rows(rows)))
    assert bool((co[:n, PL:] == 0x7FC12345).all()) and bool((co[n:] == 0x7FC12345).all())
    gp.cpu()


# ---- 4. the shared forward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_linear_output_is_head_evals_bit_for_bit(shape, cases):
    gp, x16, _, _ = cases[0][shape]
    gp.to(DEV)
    rows = x16.to(DEV)
    mean, var, out = gp.gp_rows(rows, linear=True)
    want = gp.extractor.predict_rows(rows)                                                     # coati_head_eval
    assert out.shape == want.shape and torch.equal(_bits(out), _bits(want))
    m2, v2 = gp.gp_rows(rows)                                                                  # and the GP's numbers do not depend on it
    assert torch.equal(_bits(mean), _bits(m2)) and torch.equal(_bits(var), _bits(v2))
    gp.cpu()


# ---- 5. padding -----------------------------------------------------------------------------------------------------------------
def test_padding_rows_of_z_do_not_matter(cases):
    gp, x16, _, _ = cases[0][(64, 128, 3, 8, 33)]
    gp.to(DEV)
    rows = x16.to(DEV)
    z = gp._gp_operands()[0]
    assert z.shape == (64, 128) and bool((z[33:] == 0).all())
    mean0, var0 = gp.gp_rows(rows)
    zr = z.clone()
    zr[33:] = (3.0 * torch.randn(31, 128, generator=torch.Generator().manual_seed(3))).to(torch.bfloat16).to(DEV)
    mean1, var1 = torch.empty_like(mean0), torch.empty_like(var0)
    G.head_gp_raw(gp, rows, mean1, var1, rows.shape[0], z=zr)
    assert torch.equal(_bits(mean0), _bits(mean1)) and torch.equal(_bits(var0), _bits(var1))
    gp.cpu()


# ---- 6. consumers ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def screened():
    from coati_amd.search import EmbeddingIndex
    g = torch.Generator().manual_seed(6)
    x = torch.randn(5000, 256, generator=g)
    index = EmbeddingIndex(256, metric="cosine", device=DEV)
    index.add(x)
    removed = torch.randperm(5000, generator=g)[:200]
    index.remove(removed)
    gp, _ = G.random_gp(256, 256, 4, 2, 60, seed=77, n=500, unit_input=True)
    return index, gp.to(DEV), removed


def test_property_uncertainty_is_the_kernel_on_the_stored_rows(screened):
    index, gp, _ = screened
    mean, std = index.property_uncertainty(gp)
    want_mean, want_std = gp.predict_rows_with_std(index.vectors)
    assert mean.shape == std.shape == (5000, 2) and std.dtype == torch.float32
    assert torch.equal(_bits(mean), _bits(want_mean)) and torch.equal(_bits(std), _bits(want_std))
    assert torch.equal(_bits(index.property_scores(gp)), _bits(mean))
    _, var = gp.gp_rows(index.vectors)
    assert torch.equal(std, gp.y_scale.float()[None, :] * var.sqrt()[:, None]) and bool((std >= 0).all())
    noisy = gp.predict_rows_with_std(index.vectors, include_noise=True)[1]
    assert bool((noisy > std).all())


@pytest.mark.parametrize("k", [1, 10, 128])
def test_ucb_screen_is_the_stable_sort_of_the_live_rows(screened, k):
    index, gp, removed = screened
    mean, std = index.property_uncertainty(gp)
    values = (mean[:, 1] + 2.0 * std[:, 1]).cpu()
    live = torch.ones(5000, dtype=torch.bool)
    live[removed] = False
    rows_live = live.nonzero().flatten()
    order = values[rows_live].sort(descending=True, stable=True).indices[:k]
    s, r = index.screen(gp, k, output=1, acquisition="ucb", beta=2)
    assert s.shape == (k,) and r.dtype == torch.int64
    assert torch.equal(r.cpu(), rows_live[order])
    assert torch.equal(_bits(s.cpu()), _bits(values[rows_live[order]]))                        # the acquisition's own values
    assert not bool(torch.isin(r.cpu(), removed).any())
    s0, r0 = index.screen(gp, k, output=1)                                                     # mean: property_scores' order
    want0 = mean[:, 1].cpu()[rows_live].sort(descending=True, stable=True).indices[:k]
    assert torch.equal(r0.cpu(), rows_live[want0])
    s1, r1 = index.screen(gp, k, output=1, acquisition="mean")
    assert torch.equal(r0, r1) and torch.equal(_bits(s0), _bits(s1))


def test_screen_pads_with_an_acquisition(screened):
    from coati_amd.search import EmbeddingIndex
    _, gp, _ = screened
    small = EmbeddingIndex(256, metric="cosine", device=DEV)
    small.add(torch.randn(9, 256, generator=torch.Generator().manual_seed(8)))
    small.remove([0, 2, 4, 6])
    s, r = small.screen(gp, 10, acquisition="lcb", beta=1.0)
    assert sorted(r[:5].tolist()) == [1, 3, 5, 7, 8] and r[5:].tolist() == [-1] * 5 and s[5:].tolist() == [-INF] * 5
    assert bool((s[:4] >= s[1:5]).all())
    mean, std = small.property_uncertainty(gp)
    se, re_ = small.screen(gp, 5, acquisition="ei", best=float(mean[:, 0].median()))
    assert sorted(re_.tolist()) == [1, 3, 5, 7, 8] and bool((se >= 0).all())


def test_virtual_screen_with_beta_on_the_device(screened):
    from coati_amd.generative import sampled_virtual_screen
    index, gp, _ = screened
    vectors = index.vectors.float().cpu()
    mean, std = gp.predict_with_std(vectors)
    lower = (mean[:, 0] - std[:, 0]).cpu()
    thresh = float(lower.sort().values[-40])                                                   # 39 rows lie above it

    class Maker:
        def __init__(self):
            self.at = 0

        def rsample(self, shape):
            v = vectors[self.at:self.at + shape[0]]
            self.at += shape[0]
            return v

    names = {}

    def decode(V):
        out = []
        for v in V:
            names[f"C{len(names)}"] = v.clone()
            out.append(f"C{len(names) - 1}")
        return out

    def embed(strings):
        return torch.stack([names[s] for s in strings])

    hits = sampled_virtual_screen(Maker(), gp, None, None, hit_thresh=thresh, n_to_draw=100, batch_size=1000, max_batches=5, decode=decode,
                                  embed=embed, beta=1.0)
    assert len(hits) == 39 and all(set(h) == {"smiles", "score", "std"} for h in hits)
    assert all(h["score"] - h["std"] > thresh for h in hits)
    kept = sorted(float(h["score"] - h["std"]) for h in hits)
    assert np.allclose(kept, sorted(lower[lower > thresh].tolist()), rtol=0, atol=1e-6)


# ---- 7. the fit, end to end -----------------------------------------------------------------------------------------------------
def test_fit_end_to_end_on_the_device():
    """fit_gp_head on the GPU returns the kernel's numbers: they must equal reference() on the test rows within test 1's bound, 4 x the
    worst error of the two CPU f32 restatements, taken on these rows"""
    from coati_amd.models.regression import fit_gp_head
    records, x, y = G.synthetic_records(1500, 3, seed=9)
    gp, (ys, pred, std) = fit_gp_head(records, x_field="emb", y_field="prop", n_inducing=60, gp_steps=40, steps=50, depth=0, features=64,
                                      test_frac=0.2, device=DEV)
    np.random.seed(510)
    test_idx = np.random.permutation(1500)[:300]
    assert gp.device.type == "cuda" and np.array_equal(ys, y[test_idx]) and pred.shape == std.shape == (300,)
    assert gp.fit_info["bound"] >= gp.fit_info["initial_bound"] and bool((std > 0).all())
    cpu = gp.cpu()
    x16 = cpu.prepare(torch.tensor(x[test_idx]))
    ref_mean, ref_var = cpu.reference(x16)
    wm, wv, _ = G.restatement_errors(cpu, x16, ref_mean, ref_var)
    ref_std = cpu.std_from_var(ref_var)
    em = float((torch.tensor(pred).double()[:, None] - ref_mean).abs().max()) / float(ref_mean.abs().max())
    # std = y_scale sqrt(var): an error dv of var is an error y_scale dv / (2 sqrt(var)) of std
    bound_std = float(cpu.y_scale[0]) * 4 * wv * cpu.signal_var / (2.0 * float(ref_var.min().sqrt()))
    es = float((torch.tensor(std).double()[:, None] - ref_std).abs().max())
    print(f"fit on the device: mean error {em:.3g} of max |mean| (bound 4 x {wm:.3g}), std error {es:.3g} (bound {bound_std:.3g}); "
          f"l {cpu.lengthscale:.4g}, s2 {cpu.signal_var:.4g}, noise {cpu.noise_var:.4g}")
    assert em <= 4 * wm
    assert es <= bound_std + 2.0 ** -23 * float(ref_std.max())             # (+ one f32 rounding: the root and the scale are f32 torch)
