"""The acquisition gradient, host side (no GPU): include/coati_acq.h parses against coati_hip.h and the library exports what it declares,
the entry refuses bad arguments with a code before any device call, GPHead.reference_acq_grad against torch.autograd (unrounded and with
straight-through roundings), padding, exact zeros, the guard on the variance term, AcquisitionObjective's contract and guided_ascent on a
reference-backed callable."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import acq_util as A  # noqa: E402
from tests import gp_util as G  # noqa: E402


def _cast(t):
    return t.detach().to(torch.float64)


# ---- 1. the ninth header ------------------------------------------------------------------------------------------------------------
def test_acq_header_parses_into_a_table_of_its_own():
    from coati_amd import _abi, _lib, build
    assert sorted(_lib.ACQ_PROTOTYPES) == ["coati_head_gp_grad"]
    for other in (_lib.PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.SEARCH_PROTOTYPES, _lib.GRAMMAR_PROTOTYPES, _lib.SCREEN_PROTOTYPES,
                  _lib.GUIDE_PROTOTYPES, _lib.LN_XHAT_PROTOTYPES, _lib.GP_PROTOTYPES):
        assert not set(_lib.ACQ_PROTOTYPES) & set(other)
    assert "coati_head_gp_grad" not in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 5 and sorted(_lib.GP_PROTOTYPES) == ["coati_head_gp"]
    I, P, L, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert _lib.ACQ_PROTOTYPES["coati_head_gp_grad"] == (I, [P, L, L, I, P, P, P, P, I, I, P, P, P, P, P, P, P, P, F, F, I, I, P, F, F, I, F, P,
                                                             P, L, P, P, P, L, P])
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.ACQ_HEADER) as f:
        again = _abi.parse(f.read(), guard="COATI_ACQ_H", name="coati_acq.h", base=base)
    assert again.prototypes == _lib.ACQ_PROTOTYPES and again.version == 5 and not again.experimental
    assert "gp_grad.hip" in build.HIP_UNITS and build.ACQ_HEADER in build._sources()


def test_library_exports_the_acquisition_entry():
    from coati_amd import _lib
    l = _lib.lib()
    assert l.coati_abi_version() == 5
    for name, (restype, argtypes) in _lib.ACQ_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


# ---- 2. refusals --------------------------------------------------------------------------------------------------------------------
def test_head_gp_grad_refuses_bad_arguments_with_a_code():
    """decided on the host before any device call: the pointers are host buffers that a refusal never looks at"""
    from coati_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def call(x=p, ldx=64, N=100, E=64, w0=p, b0=p, wr=p, br=p, D=2, F=64, w0t=p, wrt=p, z=p, zt=p, zn=p, alpha=p, qs=p, c=p, inv2l2=0.5, s2=1.0,
             P=1, Mp=64, wm=p, kappa=1.0, var_add=0.0, mode=0, best=0.0, rs=None, mean=p, ldm=1, var=p, acq=p, g=p, ldg=64):
        rc = l.coati_head_gp_grad(x, ldx, N, E, w0, b0, wr, br, D, F, w0t, wrt, z, zt, zn, alpha, qs, c, inv2l2, s2, P, Mp, wm, kappa, var_add,
                                  mode, best, rs, mean, ldm, var, acq, g, ldg, None)
        return rc, l.coati_last_error().decode()

    cases = [(dict(g=None), "g"), (dict(Mp=48), "Mp=48"), (dict(F=100), "F=100"), (dict(ldg=66), "ldg=66"), (dict(mode=2), "mode=2"),
             (dict(mode=1, kappa=0.0), "kappa"), (dict(mode=1, kappa=-1.0), "kappa"),
             (dict(x=None), "x"), (dict(w0t=None), "w0t"), (dict(zt=None), "zt"), (dict(qs=None), "qs"), (dict(wm=None), "wm"),
             (dict(acq=None), "acq"), (dict(mean=None), "mean"), (dict(var=None), "var"), (dict(wrt=None), "D=2"), (dict(D=17), "D=17"),
             (dict(E=48, ldx=48, ldg=48), "E=48"), (dict(P=0), "P=0"), (dict(P=9, ldm=9), "P=9"), (dict(P=3, ldm=2), "ldm=2"),
             (dict(ldx=68), "ldx=68"), (dict(ldg=32), "ldg=32"), (dict(N=0), "N=0"), (dict(zt=ctypes.c_void_p(p.value + 2)), "16-byte"),
             (dict(g=ctypes.c_void_p(p.value + 4)), "16-byte")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc < 0 and "head_gp_grad" in msg and word in msg, (kw, rc, msg)


# ---- 3. the reference against autograd ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_cases():
    """per (shape, unit_input): a gp_util.random_gp head (non-symmetric q) with 300 of its rows as float64 vectors -- scaled per row where
    unit_input, so that the normalisation has something to do -- and the acquisition cases"""
    out = {}
    for i, (E, F, D, P, M) in enumerate(A.SHAPES[:4]):
        for unit_input in (False, True):
            gp, x16 = G.random_gp(E, F, D, P, M, seed=300 + i, n=300, unit_input=unit_input)
            assert not torch.equal(gp.q, gp.q.T)
            v = x16.double()
            if unit_input:
                v = v * (0.5 + 2.0 * torch.rand(300, 1, generator=torch.Generator().manual_seed(i), dtype=torch.float64))
            out[(E, F, D, P, M), unit_input] = (gp, v, A.acq_cases(gp, gp.prepare(v), seed=i))
    return out


@pytest.mark.parametrize("unit_input", [False, True])
@pytest.mark.parametrize("rounded", [False, True], ids=["unrounded", "straight-through"])
@pytest.mark.parametrize("shape", A.SHAPES[:4], ids=A.ids)
def test_reference_acq_grad_is_autograd(shape, rounded, unit_input, small_cases):
    """float64, the stored operands (f32_operands=False), q non-symmetric in the autograd model and symmetrised in the reference: with a
    plain cast for round_fn the reference is the exact gradient of the unrounded model, with the roundings on that of the model whose
    forward roundings are straight-through and whose three backward roundings act on the gradient where it passes.  Bound: 1e-9 of the
    largest gradient entry, seven orders above float64 round-off."""
    from coati_amd.models.regression.property_head import unit_input_chain
    gp, v, cases = small_cases[shape, unit_input]
    x16 = gp.prepare(v)
    for case in cases:
        name, wm, kappa, var_add, mode, best, rs = case
        acq, grad = A.autograd_acq(gp, v, wm, kappa, var_add, mode, best, rs, rounded)
        mean, var, a, g = gp.reference_acq_grad(x16, wm, kappa, var_add, mode, best, rs, torch.float64, None if rounded else _cast,
                                                f32_operands=False)
        assert mean.shape == (300, shape[3]) and var.shape == a.shape == (300,) and g.shape == (300, gp.input_dim_padded)
        assert float(var.min()) > 0.02 * gp.signal_var                                            # no clamp, no guard in play
        g_rows, g = g, g[:, :gp.input_dim]
        if unit_input:
            g = unit_input_chain(g, v)
        scale = float(grad.abs().max())
        assert scale > 0 and float((a - acq).abs().max()) <= 1e-12 * max(1.0, float(acq.abs().max()))
        err = float((g - grad).abs().max()) / scale
        assert err <= 1e-9, (shape, name, rounded, unit_input, err)
        if rs is not None:                                                                      # the scale multiplies the gradient, not acq
            _, _, a1, g1 = gp.reference_acq_grad(x16, wm, kappa, var_add, mode, best, None, torch.float64, None if rounded else _cast,
                                                 f32_operands=False)
            assert torch.equal(a1, a) and not torch.equal(g1, g_rows)


def test_reference_forward_is_reference_with_the_symmetric_part():
    """mean is reference()'s; var is reference()'s of the head whose q is the symmetric part"""
    from coati_amd.models.regression import GPHead
    gp, x16 = G.random_gp(64, 128, 3, 8, 33, seed=5, n=200)
    wm = torch.zeros(8)
    wm[2] = 1.0
    mean, var, acq, _ = gp.reference_acq_grad(x16, wm, 2.0, 0.0, 0, 0.0)
    m0, v0 = gp.reference(x16)
    assert torch.equal(mean, m0) and float((var - v0).abs().max()) <= 1e-6 * gp.signal_var
    sym = GPHead(gp.extractor, gp.z, gp.alpha, 0.5 * (gp.q + gp.q.T), gp.const, gp.lengthscale, gp.signal_var, gp.noise_var)
    assert float((var - sym.reference(x16)[1]).abs().max()) <= 1e-12 * gp.signal_var
    assert float((acq - (mean[:, 2] + 2.0 * var.sqrt())).abs().max()) <= 1e-12
    with pytest.raises(ValueError, match="mode"):
        gp.reference_acq_grad(x16, wm, 0.0, 0.0, 1, 0.0)
    with pytest.raises(ValueError, match="wm"):
        gp.reference_acq_grad(x16, torch.ones(3), 1.0)
    with pytest.raises(ValueError, match="bf16"):
        gp.reference_acq_grad(x16.float(), wm, 1.0)


@pytest.mark.parametrize("M", [8, 31, 33, 60])
def test_padded_inducing_points_change_nothing(M):
    """a head of Mp points whose last Mp - M carry zero alpha and zero rows and columns of q -- and ANY z -- gives the bits of the head of M"""
    from coati_amd.models.regression import GPHead
    gp, x16 = G.random_gp(64, 128, 2, 2, M, seed=40 + M, n=150)
    Mp = 32 if M <= 32 else 64
    gen = torch.Generator().manual_seed(M)
    z = torch.cat([gp.z.float(), torch.randn(Mp - M, 128, generator=gen)])
    alpha = torch.nn.functional.pad(gp.alpha, (0, Mp - M))
    q = torch.nn.functional.pad(gp.q, (0, Mp - M, 0, Mp - M))
    padded = GPHead(gp.extractor, z, alpha, q, gp.const, gp.lengthscale, gp.signal_var, gp.noise_var)
    for case in A.acq_cases(gp, x16):
        _, wm, kappa, var_add, mode, best, rs = case
        for dtype in (torch.float64, torch.float32):
            a = gp.reference_acq_grad(x16, wm, kappa, var_add, mode, best, rs, dtype)
            b = padded.reference_acq_grad(x16, wm, kappa, var_add, mode, best, rs, dtype)
            for ta, tb in zip(a, b):
                assert torch.equal(ta, tb), (M, case[0], dtype)
    zt, qs = padded._gp_grad_operands()
    assert zt.shape == (128, Mp) and qs.shape == (Mp, Mp) and bool((qs[M:] == 0).all()) and bool((qs[:, M:] == 0).all())
    assert torch.equal(qs, qs.T) and torch.equal(zt, padded._gp_operands()[0].T)


def test_zero_alpha_and_zero_kappa_give_a_zero_gradient():
    from coati_amd.models.regression import GPHead
    gp, x16 = G.random_gp(96, 128, 2, 2, 32, seed=9, n=100)
    flat = GPHead(gp.extractor, gp.z, torch.zeros_like(gp.alpha), gp.q, gp.const, gp.lengthscale, gp.signal_var, gp.noise_var)
    for dtype in (torch.float64, torch.float32):
        mean, var, acq, g = flat.reference_acq_grad(x16, torch.tensor([0.0, 1.0]), 0.0, 0.0, 0, 0.0, dtype=dtype)
        assert bool((g == 0).all()) and torch.equal(acq, mean[:, 1])
    assert bool((A.restate_acq_f32(flat, x16, torch.tensor([0.0, 1.0]), 0.0, 0.0, 0, 0.0)[3] == 0).all())
    _, _, _, g = gp.reference_acq_grad(x16, torch.tensor([0.0, 1.0]), 0.0, 0.0, 0, 0.0)            # (and the mean term alone is not zero)
    assert float(g.abs().max()) > 0


def test_rows_with_a_clamped_variance_get_the_mean_term_only():
    """q scaled up until k q k passes s2 on some rows: there v = 0, B = 0 and the gradient is that of kappa = 0; elsewhere it is not.
    With var_add the acquisition still carries kappa sqrt(var_add) on such a row, the gradient still has no variance term."""
    from coati_amd.models.regression import GPHead
    gp, x16 = G.random_gp(64, 128, 3, 8, 33, seed=12, n=400)
    big = GPHead(gp.extractor, gp.z, gp.alpha, 1.6 * gp.q, gp.const, gp.lengthscale, gp.signal_var, gp.noise_var)
    wm = torch.zeros(8)
    wm[0] = 1.0
    for var_add in (0.0, 0.01):
        mean, var, acq, g = big.reference_acq_grad(x16, wm, 1.5, var_add, 0, 0.0)
        _, _, _, g0 = big.reference_acq_grad(x16, wm, 0.0, var_add, 0, 0.0)
        clamped = var == 0
        assert 10 <= int(clamped.sum()) <= 390
        assert torch.equal(g[clamped], g0[clamped]) and bool((g[~clamped] != g0[~clamped]).any(dim=1).all())
        assert float((acq[clamped] - (mean[clamped, 0] + 1.5 * var_add ** 0.5)).abs().max()) <= 1e-6
        best = float(mean[:, 0].median())
        _, _, ei, ge = big.reference_acq_grad(x16, wm, 1.0, var_add, 1, best)
        mu = mean[:, 0] - G_f32(best)
        if var_add == 0.0:                                                                    # s == 0: a = max(mu, 0), A = [mu > 0]
            assert torch.equal(ei[clamped], mu[clamped].clamp_min(0.0))
            up = clamped & (mu > 0)
            assert int(up.sum()) > 0 and torch.equal(ge[up], g0[up]) and bool((ge[clamped & (mu <= 0)] == 0).all())


def G_f32(v):
    return A.f32_scalar(v)


# ---- 4. the objective ---------------------------------------------------------------------------------------------------------------
class _ReferenceGP:
    """a GPHead whose acq_rows is reference_acq_grad in float32: what a CPU test can hand to AcquisitionObjective"""

    @staticmethod
    def of(gp):
        from coati_amd.models.regression import GPHead

        class Stub(GPHead):
            def acq_rows(self, x16, wm, kappa, var_add=0.0, mode=0, best=0.0, row_scale=None):
                return tuple(t.float() for t in self.reference_acq_grad(x16, wm, kappa, var_add, mode, best, row_scale))

        return Stub(gp.extractor, gp.z, gp.alpha, gp.q, gp.const, gp.lengthscale, gp.signal_var, gp.noise_var,
                    torch.arange(gp.num_outputs).double() * 0.3, 1.0 + torch.arange(gp.num_outputs).double())


@pytest.mark.parametrize("unit_input", [False, True])
def test_objective_predict_is_acquisition_values(unit_input):
    from coati_amd.models.regression import ACQUISITIONS, AcquisitionObjective, acquisition_values
    gp, x16 = G.random_gp(96, 128, 2, 2, 32, seed=21, n=120, unit_input=unit_input)
    stub = _ReferenceGP.of(gp)
    v = x16.float()
    mean, var = stub.reference(stub.prepare(v))
    best = float(mean[:, 1].median())
    for kind in ACQUISITIONS:
        for include_noise in (False, True):
            obj = stub.acquisition(kind, beta=1.7, best=best if kind == "ei" else None, output=1, include_noise=include_noise)
            assert isinstance(obj, AcquisitionObjective)
            std = stub.std_from_var(var, include_noise)
            want = acquisition_values(mean[:, 1], std[:, 1], kind, 1.7, best)
            got = obj.predict(v)
            assert got.shape == (120, 1) and got.dtype == torch.float32
            assert float((got[:, 0].double() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max())), (kind, include_noise)
            values, grad = obj.value_and_grad(v)
            assert torch.equal(values, got) and grad.shape == (120, 96)
            _, g1 = obj.value_and_grad(v, torch.tensor([-2.0]))
            _, gn = obj.value_and_grad(v, torch.full((120, 1), -2.0))
            assert torch.equal(g1, gn) and float((g1 + 2.0 * grad).abs().max()) <= 2e-2 * float(grad.abs().max()) + 1e-30
    wm, kappa, var_add, mode, b = stub.acquisition("lcb", beta=2.0, output=1, include_noise=True).operands()
    assert wm.tolist() == [0.0, 1.0] and kappa == -2.0 * float(stub.y_scale[1]) and var_add == stub.noise_var and (mode, b) == (0, 0.0)
    assert stub.acquisition("ei", best=0.25, output=0).operands()[1:] == (float(stub.y_scale[0]), 0.0, 1, 0.25)
    assert stub.acquisition("mean").operands()[1] == 0.0


def test_objective_has_the_contract_of_a_head():
    from coati_amd.models.regression import ACQUISITIONS, AcquisitionObjective
    gp, x16 = G.random_gp(40, 64, 1, 3, 8, seed=22, n=10)
    obj = gp.acquisition("ucb", beta=0.5, output=2)
    assert ACQUISITIONS == ("mean", "ucb", "lcb", "ei")
    assert obj.has_input_gradient is True and obj.num_outputs == 1 and obj.input_dim == 40 and obj.input_dim_padded == 64
    assert obj.device == gp.device and obj.kind == "ucb" and obj.output == 2 and obj.unit_input is False
    assert torch.equal(obj.prepare(x16.float()), gp.prepare(x16.float()))
    assert gp.has_input_gradient is False                                                      # the bare head keeps refusing
    with pytest.raises(NotImplementedError):
        gp.value_and_grad(x16.float())
    with pytest.raises(ValueError, match="best"):
        gp.acquisition("ei")
    with pytest.raises(ValueError, match="kind"):
        gp.acquisition("pi")
    with pytest.raises(ValueError, match="output"):
        gp.acquisition("ucb", output=3)
    with pytest.raises(ValueError, match="beta"):
        gp.acquisition("lcb", beta=-1.0)
    with pytest.raises(TypeError, match="GPHead"):
        AcquisitionObjective(gp.extractor)
    with pytest.raises(ValueError, match="cotangent"):
        obj._row_scale(torch.ones(2), 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        obj.predict(x16.float())
    assert [t.shape for t in gp.acq_rows(torch.zeros(0, 64, dtype=torch.bfloat16), torch.ones(3), 1.0)] == [(0, 3), (0,), (0,), (0, 64)]


def test_regression_exports():
    import coati.models.regression as R
    import coati_amd.models.regression as AR
    from coati_amd.models.autograd_funs import property as prop
    from coati_amd.models.regression import acquisition
    assert AR.AcquisitionObjective is acquisition.AcquisitionObjective and R.AcquisitionObjective is acquisition.AcquisitionObjective
    assert R.ACQUISITIONS == AR.ACQUISITIONS and callable(prop.acquisition_fused) and callable(prop.head_fused)


# ---- 5. guided_ascent on a reference-backed callable ----------------------------------------------------------------------------------
def test_guided_ascent_climbs_an_acquisition_on_the_cpu():
    """64 starts, 10 steps on the reference (roundings on, float64) against the same loop on autograd of the unrounded float64 model: the
    share of trajectories whose acquisition rose is at least the latter's minus 0.01"""
    from coati_amd.generative import guided_ascent
    gp, x16 = G.random_gp(64, 128, 3, 8, 33, seed=31, n=64)
    obj = gp.acquisition("ucb", beta=1.0, output=4)
    start = x16.double()
    with pytest.raises(TypeError, match="extractor"):
        guided_ascent(start, gp, steps=1)                                                       # the bare head: still refused
    run = guided_ascent(start, obj, steps=10, lr=0.01, value_and_grad=A.reference_value_and_grad(obj))
    exact = guided_ascent(start, obj, steps=10, lr=0.01, value_and_grad=A.autograd_value_and_grad(obj))
    assert run.history.shape == (11, 64) and run.values.shape == (64, 1) and run.vectors.dtype == torch.float64
    climbed, want = float((run.history[-1] > run.history[0]).float().mean()), float((exact.history[-1] > exact.history[0]).float().mean())
    print(f"guided_ascent on the reference: {100 * climbed:.2f} % of 64 trajectories climbed (unrounded float64 autograd: {100 * want:.2f} %); "
          f"mean gain {float((run.history[-1] - run.history[0]).mean()):.4g} against {float((exact.history[-1] - exact.history[0]).mean()):.4g}")
    assert climbed >= want - 0.01
    one = guided_ascent(start, obj, steps=1, lr=0.01, anchor=0.5, value_and_grad=A.reference_value_and_grad(obj))
    assert torch.equal(one.vectors, start + 0.01 * A.reference_value_and_grad(obj)(start, torch.ones(1))[1])
