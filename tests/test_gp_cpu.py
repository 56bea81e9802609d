"""The GP head, host side (no GPU): include/coati_gp.h parses against coati_hip.h and the library exports what it declares, the entry refuses
bad arguments with a code before any device call, GPHead.reference against the exact GP posterior, from_variational, padding, the fit,
the acquisitions, files and the refusals of what is not implemented."""
import ctypes
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import gp_util as G  # noqa: E402


# ---- 1. the eighth header -----------------------------------------------------------------------------------------------------
def test_gp_header_parses_into_a_table_of_its_own():
    from coati_amd import _abi, _lib, build
    assert sorted(_lib.GP_PROTOTYPES) == ["coati_head_gp"]
    for other in (_lib.PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.SEARCH_PROTOTYPES, _lib.GRAMMAR_PROTOTYPES, _lib.SCREEN_PROTOTYPES,
                  _lib.GUIDE_PROTOTYPES, _lib.LN_XHAT_PROTOTYPES):
        assert not set(_lib.GP_PROTOTYPES) & set(other)
    assert "coati_head_gp" not in _lib.exported_symbols()
    assert len(_lib.PROTOTYPES) == 121 and _lib.ABI_VERSION == 5
    I, P, L, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert _lib.GP_PROTOTYPES["coati_head_gp"] == (I, [P, L, L, I, P, P, P, P, I, I, P, P, I, P, L, P, P, P, P, P, F, F, I, I, P, L, P, P])
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.GP_HEADER) as f:
        text = f.read()
    again = _abi.parse(text, guard="COATI_GP_H", name="coati_gp.h", base=base)
    assert again.prototypes == _lib.GP_PROTOTYPES and again.version == 5 and not again.experimental
    assert "gp.hip" in build.HIP_UNITS and build.GP_HEADER in build._sources()


def test_library_exports_the_gp_entry():
    from coati_amd import _lib
    l = _lib.lib()
    assert l.coati_abi_version() == 5
    for name, (restype, argtypes) in _lib.GP_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_missing_gp_header_is_a_runtime_error_naming_the_path(monkeypatch, tmp_path):
    from coati_amd import _lib, build
    gone = str(tmp_path / "include" / "coati_gp.h")
    monkeypatch.setattr(build, "GP_HEADER", gone)
    try:
        with pytest.raises(RuntimeError, match="coati_gp.h"):
            importlib.reload(_lib)
    finally:
        monkeypatch.undo()
        importlib.reload(_lib)
    assert sorted(_lib.GP_PROTOTYPES) == ["coati_head_gp"]


# ---- 2. refusals ------------------------------------------------------------------------------------------------------------------
def test_head_gp_refuses_bad_arguments_with_a_code():
    """decided on the host before any device call: the pointers are host buffers that a refusal never looks at"""
    from coati_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def call(x=p, ldx=64, N=100, E=64, w0=p, b0=p, wr=p, br=p, D=2, F=64, wl=None, bl=None, P_lin=1, out=None, ldo=1, z=p, zn=p, alpha=p,
             q=p, c=p, inv2l2=0.5, s2=1.0, P=1, Mp=64, mean=p, ldm=1, var=p):
        rc = l.coati_head_gp(x, ldx, N, E, w0, b0, wr, br, D, F, wl, bl, P_lin, out, ldo, z, zn, alpha, q, c, inv2l2, s2, P, Mp, mean, ldm,
                             var, None)
        return rc, l.coati_last_error().decode()

    cases = [(dict(x=None), "x"), (dict(w0=None), "w0"), (dict(b0=None), "b0"), (dict(z=None), "z"), (dict(zn=None), "zn"),
             (dict(alpha=None), "alpha"), (dict(q=None), "q"), (dict(c=None), "c"), (dict(mean=None), "mean"), (dict(var=None), "var"),
             (dict(wr=None), "D=2"), (dict(br=None), "D=2"), (dict(Mp=0), "Mp=0"), (dict(Mp=16), "Mp=16"), (dict(Mp=96), "Mp=96"),
             (dict(P=0), "P=0"), (dict(P=9, ldm=9), "P=9"), (dict(F=96), "F=96"), (dict(P=3, ldm=2), "ldm=2"),
             (dict(z=ctypes.c_void_p(p.value + 2)), "16-byte"), (dict(wl=p, bl=p, out=None), "out"), (dict(wl=p, bl=None, out=p), "bl"),
             (dict(wl=p, bl=p, out=p, P_lin=9, ldo=9), "P_lin=9"), (dict(wl=p, bl=p, out=p, P_lin=3, ldo=2), "ldo=2"),
             (dict(N=0), "N=0"), (dict(E=48, ldx=48), "E=48"), (dict(D=17), "D=17"), (dict(ldx=68), "ldx=68")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc < 0 and "head_gp" in msg and word in msg, (kw, rc, msg)


# ---- 3. the exact-GP identity -----------------------------------------------------------------------------------------------------
def _identity_extractor(dim=64):
    from coati_amd.models.regression import PropertyHead
    ex = PropertyHead(dim, features=dim, depth=0, num_outputs=1)
    with torch.no_grad():
        ex.first.weight.copy_(torch.eye(dim))
        ex.first.bias.zero_()
    return ex


def test_reference_is_the_exact_gp_posterior_when_z_is_the_training_set():
    """Z = X, jitter = 0: the collapsed posterior IS the exact GP's, so reference() in float64 must give k (K + noise I)^-1 y and
    s2 - k (K + noise I)^-1 k^T.  cond(K) <= 1e4 keeps float64 round-off (1e-16 x cond) four orders of magnitude under the bound."""
    from coati_amd.models.regression import GPHead
    from coati_amd.models.regression.gp_head import collapsed_posterior, rbf_kernel
    gen = torch.Generator().manual_seed(11)
    ex = _identity_extractor(64)
    X16 = torch.randn(48, 64, generator=gen).to(torch.bfloat16)              # features = inputs, exact in bf16
    X = X16.double()
    l, s2, noise = 9.0, 1.3, 0.05
    pair = torch.cdist(X, X) + 1e9 * torch.eye(48, dtype=torch.float64)
    assert float(pair.min()) >= l / 2
    K = rbf_kernel(X, X, l, s2)
    assert float(torch.linalg.cond(K)) <= 1e4
    y = torch.randn(48, 2, generator=gen).double()
    alpha, q, _, _ = collapsed_posterior(X, y, X, l, s2, noise, jitter=0.0)
    gp = GPHead(ex, X16, alpha, q, None, l, s2, noise)
    T16 = (0.8 * torch.randn(200, 64, generator=gen)).to(torch.bfloat16)
    assert torch.equal(gp.features_reference(T16), T16.double())
    mean, var = gp.reference(T16, torch.float64, f32_operands=False)
    kt = rbf_kernel(T16.double(), X, l, s2)
    Ky = K + noise * torch.eye(48, dtype=torch.float64)
    want_mean = kt @ torch.linalg.solve(Ky, y)
    want_var = s2 - (kt * torch.linalg.solve(Ky, kt.T).T).sum(dim=1)
    em = float((mean - want_mean).abs().max()) / float(y.abs().max())
    ev = float((var - want_var).abs().max()) / s2
    print(f"exact GP: mean error {em:.3g} of max |y|, var error {ev:.3g} of s2, var in {float(want_var.min() / s2):.3g} .. "
          f"{float(want_var.max() / s2):.3g} of s2")
    assert mean.shape == (200, 2) and var.shape == (200,)
    assert em <= 1e-8 and ev <= 1e-8
    assert float(want_var.min()) < 0.9 * s2                                 # (the test points are not all at the prior)


# ---- 4. from_variational ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    from coati_amd.models.regression import fit_gp_head
    records, x, y = G.synthetic_records(2000, 3, seed=4)
    gp, triple = fit_gp_head(records, x_field="emb", y_field="prop", n_inducing=60, gp_steps=100, steps=50, depth=0, features=64,
                             device="cpu")
    return gp, triple, records, x, y


def test_from_variational_reproduces_the_closed_form():
    """The optimal q(u) = N(m, S) of the collapsed bound, m = Kzz Sigma Kzf y / noise and S = Kzz Sigma Kzz, packed by from_variational,
    must give back fit_gp_head's alpha and q.  Going through Kzz and Kzz^-1 costs about eps x cond(Kzz) in float64, so the case is one
    whose Kzz is well conditioned (few inducing points, a jitter of 1e-3: cond <= 1e4, asserted), which keeps that floor at 1e-12."""
    from coati_amd.models.regression import GPHead, fit_gp_head
    from coati_amd.models.regression.gp_head import rbf_kernel
    records, x, y = G.synthetic_records(600, 8, seed=6)
    gp, _ = fit_gp_head(records, x_field="emb", y_field="prop", n_inducing=10, gp_steps=10, jitter=1e-3, steps=50, depth=1, features=64,
                        device="cpu")
    np.random.seed(510)
    train_idx = np.random.permutation(600)[int(0.03 * 600):]
    phi = gp.features_reference(gp.prepare(torch.tensor(x[train_idx])))
    ys = (torch.tensor(y[train_idx], dtype=torch.float64)[:, None] - gp.y_mean) / gp.y_scale
    z = gp.z.double()
    l, s2, noise = gp.lengthscale, gp.signal_var, gp.noise_var
    jitter = gp.fit_info["jitter"]
    assert jitter == 1e-3
    Kzz = rbf_kernel(z, z, l, s2) + jitter * s2 * torch.eye(z.shape[0], dtype=torch.float64)
    cond = float(torch.linalg.cond(Kzz))
    assert cond <= 1e4
    Kzf = rbf_kernel(z, phi, l, s2)
    Sigma = torch.linalg.inv(Kzz + Kzf @ Kzf.T / noise)
    S = Kzz @ Sigma @ Kzz
    m = (Kzz @ Sigma @ Kzf @ ys / noise).T
    again = GPHead.from_variational(gp.extractor, gp.z, m, S, None, l, s2, noise, gp.y_mean, gp.y_scale, jitter=jitter)
    ea = float((again.alpha - gp.alpha).abs().max() / gp.alpha.abs().max())
    eq = float((again.q - gp.q).abs().max() / gp.q.abs().max())
    print(f"from_variational: cond(Kzz) {cond:.3g}; alpha {ea:.3g}, q {eq:.3g} (relative)")
    assert again.alpha.dtype == torch.float64 and ea <= 1e-10 and eq <= 1e-10
    for a, b in zip(again.reference(gp.prepare(torch.tensor(x[:50]))), gp.reference(gp.prepare(torch.tensor(x[:50])))):
        assert float((a - b).abs().max()) <= 1e-6


# ---- 5. padding -------------------------------------------------------------------------------------------------------------------
def test_padded_inducing_points_change_nothing_in_reference():
    from coati_amd.models.regression import GPHead
    gp, x16 = G.random_gp(64, 128, 3, 8, 33, seed=31, n=300)
    gen = torch.Generator().manual_seed(32)

    def padded(zpad):
        z = torch.cat([gp.z.float(), zpad])
        alpha = torch.nn.functional.pad(gp.alpha, (0, 31))
        q = torch.nn.functional.pad(gp.q, (0, 31, 0, 31))
        return GPHead(gp.extractor, z, alpha, q, gp.const, gp.lengthscale, gp.signal_var, gp.noise_var)

    zero, rand = padded(torch.zeros(31, 128)), padded(3.0 * torch.randn(31, 128, generator=gen))
    for dtype in (torch.float64, torch.float32):
        m0, v0 = zero.reference(x16, dtype)
        m1, v1 = rand.reference(x16, dtype)
        mb, vb = gp.reference(x16, dtype)
        assert torch.equal(m0, m1) and torch.equal(v0, v1)
        if dtype == torch.float64:
            assert float((m0 - mb).abs().max()) <= 1e-12 * float(mb.abs().max()) and float((v0 - vb).abs().max()) <= 1e-12
    z, zn, alpha, q, c, Mp = gp._gp_operands()                               # what the kernel gets: padded the same way
    assert Mp == 64 and z.shape == (64, 128) and bool((alpha[:, 33:] == 0).all()) and bool((q[33:] == 0).all()) and bool((q[:, 33:] == 0).all())
    assert zn.shape == (64,) and torch.equal(zn[:33], (gp.z.double() ** 2).sum(dim=1).float())
    small, _ = G.random_gp(32, 64, 1, 1, 32, seed=33, n=10)
    assert small._gp_operands()[5] == 32


# ---- 6. the fit -------------------------------------------------------------------------------------------------------------------
def test_fit_gives_uncertainty_that_grows_away_from_the_data(fitted):
    gp, (ys, pred, std), records, x, y = fitted
    np.random.seed(510)
    perm = np.random.permutation(2000)
    test_idx, train_idx = perm[:60], perm[60:]
    assert np.array_equal(ys, y[test_idx]) and pred.shape == std.shape == ys.shape == (60,)
    info = gp.fit_info
    print(f"fit: bound {info['bound']:.6g} from {info['initial_bound']:.6g}; l {gp.lengthscale:.4g}, s2 {gp.signal_var:.4g}, "
          f"noise {gp.noise_var:.4g}; test mse {float(((pred - ys) ** 2).mean()):.4g} of variance {float(ys.var()):.4g}")
    assert info["bound"] >= info["initial_bound"]
    assert bool((std > 0).all())
    assert 0.0 <= info["f32_var_error"] < 1e-4                               # handing the operands to the kernel in f32 costs nothing here
    assert gp.num_inducing == 60 and gp.z.dtype == torch.bfloat16 and gp.alpha.dtype == torch.float64
    _, var_train = gp.reference(gp.prepare(torch.tensor(x[train_idx])))
    std_train = float(gp.std_from_var(var_train).mean())
    prior = float(gp.y_scale[0]) * math.sqrt(gp.signal_var)
    # rows at 3 x the training set's scale, read both ways: the training rows times 3, and random directions at 3 x their rms norm
    u = torch.randn(1940, 3, generator=torch.Generator().manual_seed(1))
    rms = float(np.sqrt((x[train_idx] ** 2).sum(axis=1).mean()))
    for name, far in (("3 x the training rows", torch.tensor(3.0 * x[train_idx])), ("3 x their rms norm", 3.0 * rms * u / u.norm(dim=1, keepdim=True))):
        _, var_far = gp.reference(gp.prepare(far))
        std_far = float(gp.std_from_var(var_far).mean())
        print(f"fit: mean std on the training rows {std_train:.4g}, at {name} {std_far:.4g}, the prior's {prior:.4g}")
        assert std_far > std_train
        assert std_far > 0.9 * prior
    assert float(((pred - ys) ** 2).mean()) < 0.5 * float(ys.var())          # and the mean is a regressor


def test_fit_uses_a_given_head_frozen_and_leaves_fit_property_head_alone():
    from coati_amd.models.regression import fit_gp_head, fit_property_head
    records, x, y = G.synthetic_records(400, 8, seed=5)
    head, (ys, pred, none) = fit_property_head(records, x_field="emb", y_field="prop", steps=20, depth=1, features=64, device="cpu")
    assert none is None                                                      # the deterministic fit still has no third slot
    before = {k: v.clone() for k, v in head.state_dict().items()}
    gp, (ys2, pred2, std2) = fit_gp_head(records, x_field="emb", y_field=["prop", "prop"], head=head, n_inducing=16, gp_steps=5,
                                         device="cpu")
    for k, v in head.state_dict().items():
        assert torch.equal(v, before[k]) and torch.equal(gp.extractor.state_dict()[k], v), k
    assert gp.num_outputs == 2 and ys2.shape == pred2.shape == std2.shape == (12, 2)
    assert np.array_equal(std2[:, 0], std2[:, 1])                            # equal targets, equal scales: one variance per row
    assert all(not p.requires_grad for p in gp.parameters())
    with pytest.raises(ValueError, match="n_inducing"):
        fit_gp_head(records, x_field="emb", y_field="prop", head=head, n_inducing=65, device="cpu")


# ---- 7. acquisitions ----------------------------------------------------------------------------------------------------------------
def test_acquisitions_against_scalar_formulas():
    from coati_amd.models.regression import PropertyHead, acquisition_values
    from coati_amd.search import EmbeddingIndex
    mu = torch.tensor([0.0, 1.0, 2.5, -1.0, 0.7, 0.3])
    sd = torch.tensor([1.0, 0.5, 0.0, 2.0, 0.0, 1e-3])
    best = 0.5
    assert acquisition_values(mu, sd, None) is mu and acquisition_values(mu, sd, "mean") is mu
    assert torch.equal(acquisition_values(mu, sd, "ucb", beta=2.0), mu + 2.0 * sd)
    assert torch.equal(acquisition_values(mu, sd, "lcb", beta=0.5), mu - 0.5 * sd)
    ei = acquisition_values(mu.double(), sd.double(), "ei", best=best)
    for i in range(6):
        m, s = float(mu[i]), float(sd[i])
        if s == 0.0:
            want = max(m - best, 0.0)
        else:
            u = (m - best) / s
            want = (m - best) * 0.5 * (1.0 + math.erf(u / math.sqrt(2.0))) + s * math.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
        assert abs(float(ei[i]) - want) <= 1e-12, (i, float(ei[i]), want)
    assert bool((ei >= 0).all()) and float(ei[2]) == 2.0 and float(ei[4]) == pytest.approx(0.2)
    with pytest.raises(ValueError, match="best"):
        acquisition_values(mu, sd, "ei")
    with pytest.raises(ValueError, match="thompson"):
        acquisition_values(mu, sd, "thompson")
    index = EmbeddingIndex(40, metric="cosine", device="cpu")
    index.add(torch.randn(30, 40, generator=torch.Generator().manual_seed(2)))
    unit = PropertyHead(40, features=64, depth=1, unit_input=True)
    with pytest.raises(ValueError, match="ucb"):
        index.screen(unit, 3, acquisition="ucb")                            # a plain head has no standard deviation
    with pytest.raises(ValueError, match="GPHead"):
        index.property_uncertainty(unit)
    gp, _ = G.random_gp(40, 64, 1, 2, 20, seed=41, n=10, unit_input=True)
    with pytest.raises(ValueError, match="acquisition"):
        index.screen(gp, 3, acquisition="thompson")
    with pytest.raises(ValueError, match="best"):
        index.screen(gp, 3, acquisition="ei")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.screen(gp, 3, acquisition="ucb", beta=2.0)                    # a valid call gets as far as the device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.property_scores(gp)
    s, r = EmbeddingIndex(40, metric="cosine", device="cpu").screen(gp, 3, acquisition="lcb")   # an empty index: padding only
    assert s.tolist() == [float("-inf")] * 3 and r.tolist() == [-1] * 3


class _Maker:
    def rsample(self, shape):
        n = shape[0]
        v = torch.zeros(n, 4)
        v[:, 0] = torch.arange(n).float()
        v[:, 1] = 2.0
        v[:, 2] = (torch.arange(n) % 3).float()                              # the standard deviation: 0, 1, 2, 0, ...
        return v


class _StdHead:
    def predict(self, v):
        return v[:, 1:2].clone()

    def predict_with_std(self, v):
        return v[:, 1:2].clone(), v[:, 2:3].clone()


def test_virtual_screen_with_beta_filters_on_the_lower_bound():
    from coati_amd.generative import sampled_virtual_screen
    decode = lambda V: [f"C{int(v[0])}" for v in V]                          # noqa: E731

    def embed(strings):
        e = torch.zeros(len(strings), 4)
        for i, s in enumerate(strings):
            k = int(s[1:])
            e[i, 0], e[i, 1], e[i, 2] = k, 2.0, (0.0 if k % 2 == 0 else 1.5)  # re-embedding: odd names are unsure now
        return e

    hits = sampled_virtual_screen(_Maker(), _StdHead(), None, None, hit_thresh=0.9, n_to_draw=4, batch_size=12, max_batches=1,
                                  decode=decode, embed=embed, beta=1.0)
    # first filter: 2 - std > 0.9 keeps std in {0, 1}: names 0, 1, 3, 4, 6, 7, 9, 10; second: 2 - 1.5 falls, so even names only
    assert [h["smiles"] for h in hits] == ["C0", "C4", "C6", "C10"]
    assert all(h["score"] == 2.0 and h["std"] == 0.0 for h in hits)
    plain = sampled_virtual_screen(_Maker(), _StdHead(), None, None, hit_thresh=0.9, n_to_draw=3, batch_size=12, max_batches=1,
                                   decode=decode, embed=embed)
    assert [h["smiles"] for h in plain] == ["C0", "C1", "C2"] and "std" not in plain[0]        # beta = 0: today's path

    class _NoStd:
        def predict(self, v):
            return v[:, 1:2]

    with pytest.raises(TypeError, match="predict_with_std"):
        sampled_virtual_screen(_Maker(), _NoStd(), None, None, hit_thresh=0.9, decode=decode, embed=embed, beta=1.0)


# ---- 8. files and what is not there -------------------------------------------------------------------------------------------------
def test_save_load_round_trip(tmp_path):
    from coati_amd.models.regression import GPHead
    gp, x16 = G.random_gp(48, 128, 2, 3, 33, seed=51, n=40, unit_input=True)
    gp.fit_info = {"bound": 1.5}
    path = str(tmp_path / "gp.pt")
    gp.save(path)
    again = GPHead.load(path, "cpu")
    assert again.gp_hyper() == gp.gp_hyper() and again.extractor.hyper() == gp.extractor.hyper() and not again.training
    assert again.fit_info == {"bound": 1.5}
    for k, v in gp.state_dict().items():
        assert torch.equal(again.state_dict()[k], v) and again.state_dict()[k].dtype == v.dtype, k
    for a, b in zip(again.reference(x16), gp.reference(x16)):
        assert torch.equal(a, b)
    assert again.input_dim == 48 and again.input_dim_padded == 64 and again.unit_input and again.num_outputs == 3


def test_constructor_and_cpu_refusals():
    from coati_amd.models.regression import GPHead, PropertyHead
    ex = PropertyHead(32, features=64, depth=0)
    z, a, q = torch.zeros(4, 64), torch.zeros(1, 4), torch.zeros(4, 4)
    for args, word in (((torch.zeros(65, 64), torch.zeros(1, 65), torch.zeros(65, 65)), "64"), ((torch.zeros(4, 32), a, q), "z must"),
                       ((z, torch.zeros(1, 5), q), "alpha"), ((z, torch.zeros(9, 4), q), "alpha"), ((z, a, torch.zeros(4, 5)), "q must")):
        with pytest.raises(ValueError, match=word):
            GPHead(ex, *args, None, 1.0, 1.0, 0.1)
    with pytest.raises(ValueError, match="lengthscale"):
        GPHead(ex, z, a, q, None, 0.0, 1.0, 0.1)
    with pytest.raises(TypeError, match="PropertyHead"):
        GPHead(torch.nn.Linear(3, 3), z, a, q, None, 1.0, 1.0, 0.1)
    gp = GPHead(ex, z, a, q, None, 1.0, 1.0, 0.1)
    x = torch.randn(5, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gp.predict(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gp.predict_with_std(x)
    assert gp.predict_rows(torch.zeros(0, 32, dtype=torch.bfloat16)).shape == (0, 1)
    mean, var = gp.reference(gp.prepare(x))
    assert bool((mean == 0).all()) and bool((var == 1.0).all())              # alpha = 0, q = 0: the prior


def test_gradients_are_refused_by_name():
    from coati_amd.generative import guided_ascent, guided_generation
    gp, _ = G.random_gp(32, 64, 1, 1, 8, seed=61, n=10)
    x = torch.randn(3, 32)
    with pytest.raises(NotImplementedError, match="extractor"):
        gp.fused(x)
    with pytest.raises(NotImplementedError, match="extractor"):
        gp.value_and_grad(x)
    with pytest.raises(TypeError, match="extractor"):
        guided_ascent(x, gp, steps=2)
    with pytest.raises(TypeError, match="extractor"):
        guided_generation(x, gp, None, None, steps=2, decode=lambda V: ["C"] * len(V), embed=lambda s: torch.zeros(len(s), 32))


def test_alias_exports():
    import coati.models.regression as R
    from coati_amd.models.regression import GPHead, acquisition_values, fit_gp_head
    assert R.GPHead is GPHead and R.fit_gp_head is fit_gp_head and R.acquisition_values is acquisition_values
