"""Library density without a GPU (include/coati_gmm.h, coati_amd/gmm.py): the header and its host arithmetic, the parameter rows, the float64
EM against scikit-learn from the common start of tests/gmm_util.py, the mixture object and its use as a virtual screen's sample maker."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import gmm_util as U  # noqa: E402


def test_header_names_and_prototypes():
    import ctypes as C
    from coati_amd import _lib
    P = _lib.GMM_PROTOTYPES
    assert sorted(P) == ["coati_gmm_chunk", "coati_gmm_estep", "coati_gmm_mstep", "coati_gmm_part_floats", "coati_gmm_ranges"]
    restype, args = P["coati_gmm_estep"]
    assert restype is C.c_int and len(args) == 11 and args[1] is C.c_int64 and args[2] is C.c_int and args[5] is C.c_int
    restype, args = P["coati_gmm_mstep"]
    assert restype is C.c_int and len(args) == 15 and args[9] is C.c_int64
    assert P["coati_gmm_chunk"] == (C.c_int, []) or (P["coati_gmm_chunk"][0] is C.c_int and not list(P["coati_gmm_chunk"][1]))
    assert P["coati_gmm_ranges"][0] is C.c_int64 and list(P["coati_gmm_ranges"][1]) == [C.c_int64]
    assert P["coati_gmm_part_floats"][0] is C.c_int64 and list(P["coati_gmm_part_floats"][1]) == [C.c_int64, C.c_int, C.c_int]


def test_host_arithmetic():
    from coati_amd import _lib
    l = _lib.lib()
    ch = l.coati_gmm_chunk()
    assert ch >= 16 and ch % 16 == 0
    for N in (1, ch - 1, ch, ch + 1, 1000, 512 * ch, 512 * ch + 1, 2 ** 31 - 1):
        chunks = (N + ch - 1) // ch
        R = l.coati_gmm_ranges(N)
        assert R == min(chunks, 512) and 1 <= R <= chunks
        for E, K in ((32, 1), (256, 17), (512, 256)):
            assert l.coati_gmm_part_floats(N, E, K) == R * K * (2 * E + 1)
    for N in (0, -1, 2 ** 31):
        assert l.coati_gmm_ranges(N) < 0 and l.coati_gmm_part_floats(N, 32, 1) < 0
    for E, K in ((0, 1), (33, 1), (544, 1), (32, 0), (32, 257)):
        assert l.coati_gmm_part_floats(100, E, K) < 0
    assert b"gmm_part_floats" in l.coati_last_error()


def test_null_and_range_arguments_are_refused_before_any_device_call():
    from coati_amd import _lib
    l = _lib.lib()
    one = 4096                                                                # any non-null address: refused before it is looked at
    assert l.coati_gmm_estep(None, 1, 32, None, one, 1, one, one, None, 0, None) == -1 and b"lib is null" in l.coati_last_error()
    assert l.coati_gmm_estep(one, 1, 32, None, None, 1, one, one, None, 0, None) == -1
    assert l.coati_gmm_estep(one, 1, 32, None, one, 1, one, None, None, 0, None) == -1
    for N, E, K, blocks in ((0, 32, 1, 0), (2 ** 31, 32, 1, 0), (1, 48, 1, 0), (1, 544, 1, 0), (1, 32, 0, 0), (1, 32, 257, 0), (1, 32, 1, -1)):
        assert l.coati_gmm_estep(one, N, E, None, one, K, one, one, None, blocks, None) == -2, (N, E, K, blocks)
        assert l.coati_gmm_mstep(one, N, E, None, one, K, one, one, one, 2 ** 40, one, one, one, blocks, None) == -2, (N, E, K, blocks)
    assert l.coati_gmm_mstep(one, 100, 32, None, one, 3, one, one, None, 2 ** 40, one, one, one, 0, None) == -1
    assert l.coati_gmm_mstep(one, 100, 32, None, one, 3, one, one, one, 2 * 3 * 65 - 1, one, one, one, 0, None) == -2
    assert b"part_floats" in l.coati_last_error()


def test_prepare_params_is_the_log_density_and_ignores_the_padding():
    from coati_amd import gmm
    g = torch.Generator().manual_seed(3)
    K, dim, width = 5, 24, 32
    w = torch.rand(K, generator=g, dtype=torch.float64) + 0.1
    w = w / w.sum()
    mu = torch.randn(K, dim, generator=g, dtype=torch.float64)
    var = torch.rand(K, dim, generator=g, dtype=torch.float64) + 0.05
    par, cst = gmm.prepare_params(w, mu, var, width)
    assert par.dtype == cst.dtype == torch.float32 and par.shape == (K, 2 * width) and cst.shape == (K,)
    assert not par[:, dim:width].any() and not par[:, width + dim:].any()
    par64, cst64 = gmm.prepare_params_f64(w, mu, var, width)
    assert torch.equal(par, par64.float()) and torch.equal(cst, cst64.float())
    x = torch.randn(40, dim, generator=g).to(torch.bfloat16)
    want = torch.distributions.Independent(torch.distributions.Normal(mu, var.sqrt()), 1).log_prob(x.double()[:, None, :]) + w.log()
    got = gmm.reference_logits(U.padded(x, width), par64, cst64)
    assert (got - want).abs().max() < 1e-10
    narrow, cn = gmm.prepare_params_f64(w, mu, var, dim)
    assert torch.equal(gmm.reference_logits(x, narrow, cn), got)               # the dim-24 density, bit for bit: the padding adds zeros
    with pytest.raises(ValueError):
        gmm.prepare_params(w, mu, var, 16)


@pytest.mark.parametrize("name", ["a", "c"])
def test_reference_fit_is_sklearn_and_its_trace_never_falls(name):
    """float64 against float64 from the same start: 1e-9 on means and weights, 1e-9 relative on variances (measured: 3e-13 or less; the
    margin covers the BLAS order); each step of the trace loses no more than 1e-9"""
    mixture = pytest.importorskip("sklearn.mixture")
    from coati_amd import gmm
    N, dim, C, K, noise = U.LIBRARIES[name]
    x16 = U.library(N, dim, C, noise)
    w0, m0, v0 = U.common_start(N, dim, C, noise, K)
    w, m, v, trace = gmm.reference_fit(x16, None, w0, m0, v0, 30)
    assert all(b - a >= -1e-9 for a, b in zip(trace, trace[1:])), trace
    assert float(v.min()) >= 1.6e-4 and float(w.min()) >= 0.025              # no component collapses
    sk = mixture.GaussianMixture(K, covariance_type="diag", tol=0, max_iter=30, reg_covar=1e-6, weights_init=w0.numpy(), means_init=m0.numpy(),
                                 precisions_init=(1.0 / v0).numpy())
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk.fit(x16.double().numpy())
    dm, dw = (m - torch.from_numpy(sk.means_)).abs().max(), (w - torch.from_numpy(sk.weights_)).abs().max()
    dv = ((v - torch.from_numpy(sk.covariances_)) / v).abs().max()
    print(f"gmm reference_fit vs sklearn on {name}: means {float(dm):.2e}, weights {float(dw):.2e}, variances (relative) {float(dv):.2e}")
    assert dm <= 1e-9 and dw <= 1e-9 and dv <= 1e-9
    par, cst = gmm.prepare_params_f64(w, m, v, dim)
    lse, _ = gmm.reference_estep(x16, None, par, cst)
    assert (lse - torch.from_numpy(sk.score_samples(x16.double().numpy()))).abs().max() <= 1e-9


def _mixture(seed=5, K=6, dim=24):
    from coati_amd.gmm import GaussianMixture
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(K, generator=g) + 0.1
    return GaussianMixture(w / w.sum(), torch.randn(K, dim, generator=g) * 0.2, torch.rand(K, dim, generator=g) * 0.01 + 0.001)


def test_rsample_shapes_seed_and_component_frequencies():
    gm = _mixture()
    s = gm.rsample([7])
    assert s.shape == (7, 24) and s.dtype == torch.float32 and gm.sample((2, 3)).shape == (2, 3, 24)
    a = gm.rsample([100], generator=torch.Generator().manual_seed(9))
    assert torch.equal(a, gm.rsample([100], generator=torch.Generator().manual_seed(9)))
    n = 200000
    gm.metric = "dot"                                                         # the draws as they are: no normalisation before predict
    comp = gm.predict(gm.rsample([n], generator=torch.Generator().manual_seed(1)))
    # the components are 0.2 apart with sigma <= 0.105 in 24 dimensions: the most responsible component IS the one drawn
    freq = torch.bincount(comp.long(), minlength=gm.k).double() / n
    p = gm.weights.double()
    se = (p * (1 - p) / n).sqrt()
    assert ((freq - p).abs() <= 4 * se).all(), (freq, p)


def test_to_torch_log_prob_is_log_prob():
    gm = _mixture()
    gm.metric = "dot"
    x = (torch.randn(50, 24, generator=torch.Generator().manual_seed(2)) * 0.2).to(torch.bfloat16)
    from coati_amd import gmm
    w = gm.weights.double() / gm.weights.double().sum()                      # (a Categorical normalises its probs: f32 weights sum to 1 +- 1e-7)
    par, cst = gmm.prepare_params_f64(w, gm.means, gm.variances, 32)
    lse, assign = gmm.reference_estep(U.padded(x, 32), None, par, cst)
    assert (gm.to_torch().log_prob(x.double()) - lse).abs().max() <= 1e-10
    assert gm.log_prob(x.float()).dtype == torch.float32 and (gm.log_prob(x.float()).double() - lse).abs().max() <= 1e-4 * lse.abs().max()
    assert torch.equal(gm.predict(x.float()).long(), assign)
    r = gm.responsibilities(x.float())
    assert r.shape == (50, gm.k) and (r.sum(dim=1) - 1).abs().max() < 1e-5 and torch.equal(r.argmax(dim=1), assign)


def test_save_load_round_trip_and_bic(tmp_path):
    from coati_amd.gmm import GaussianMixture
    gm = _mixture()
    gm.log_likelihood, gm.trace, gm.iterations, gm.converged = 12.5, [11.0, 12.5], 2, True
    gm.save(str(tmp_path / "g.pt"))
    back = GaussianMixture.load(str(tmp_path / "g.pt"))
    assert all(torch.equal(a, b) for a, b in ((gm.weights, back.weights), (gm.means, back.means), (gm.variances, back.variances)))
    assert (back.log_likelihood, back.trace, back.iterations, back.converged, back.metric) == (12.5, [11.0, 12.5], 2, True, "cosine")
    assert back.bic(1000) == pytest.approx(-2 * 12.5 * 1000 + (6 * 49 - 1) * math.log(1000))


def test_a_mixture_is_a_virtual_screen_s_sample_maker():
    from coati_amd.generative import fit_library_density, sampled_virtual_screen
    import coati.generative as G
    assert G.fit_library_density is fit_library_density
    gm = _mixture(dim=4)

    class Head:
        def predict(self, v):
            return v[:, :1].clone()

    seen = []

    def decode(V):
        seen.append(V.shape)
        return [f"C{i}" for i in range(V.shape[0])]

    hits = sampled_virtual_screen(gm, Head(), None, None, hit_thresh=-10.0, n_to_draw=5, batch_size=16, max_batches=2, decode=decode,
                                  embed=lambda strings: torch.ones(len(strings), 4))
    assert seen == [(16, 4)] and [h["smiles"] for h in hits] == [f"C{i}" for i in range(5)]


def test_off_a_gpu_the_index_raises_and_dot_is_refused():
    from coati_amd.search import EmbeddingIndex
    index = EmbeddingIndex(24, metric="cosine", device="cpu")
    index.add(torch.randn(10, 24))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.gmm(2)
    with pytest.raises(ValueError, match="dot"):
        EmbeddingIndex(24, metric="dot", device="cpu").gmm(2)
