"""Guided latent optimisation, host side (no GPU): include/coati_guide.h parses against coati_hip.h and the library exports what it
declares, the entry refuses bad arguments with a code before any device call, PropertyHead.reference_grad and unit_input_chain against
float64 autograd, guided_ascent against a from-scratch restatement of its objective, and guided_generation's control flow on stubs."""
import ctypes
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import guide_util as G  # noqa: E402
from tests import screen_util as U  # noqa: E402


# ---- the sixth header -----------------------------------------------------------------------------------------------------------
def test_guide_header_parses_into_a_table_of_its_own():
    from coati_amd import _abi, _lib, build
    assert sorted(_lib.GUIDE_PROTOTYPES) == ["coati_head_grad"]
    for other in (_lib.PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.SEARCH_PROTOTYPES, _lib.GRAMMAR_PROTOTYPES, _lib.SCREEN_PROTOTYPES):
        assert not set(_lib.GUIDE_PROTOTYPES) & set(other)
    assert "coati_head_grad" not in _lib.exported_symbols()
    assert len(_lib.PROTOTYPES) == 121 and _lib.ABI_VERSION == 5 and sorted(_lib.SCREEN_PROTOTYPES) == ["coati_head_eval"]
    I, P, L = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert _lib.GUIDE_PROTOTYPES["coati_head_grad"] == (I, [P, L, L, I, P, P, P, P, I, P, P, I, I, P, P, P, L, P, L, P, L, P])
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.GUIDE_HEADER) as f:
        text = f.read()
    again = _abi.parse(text, guard="COATI_GUIDE_H", name="coati_guide.h", base=base)
    assert again.prototypes == _lib.GUIDE_PROTOTYPES and again.version == 5 and not again.experimental
    assert "guide.hip" in build.HIP_UNITS and build.GUIDE_HEADER in build._sources()


def test_library_exports_the_gradient_entry():
    from coati_amd import _lib
    l = _lib.lib()
    assert l.coati_abi_version() == 5
    for name, (restype, argtypes) in _lib.GUIDE_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_missing_guide_header_is_a_runtime_error_naming_the_path(monkeypatch, tmp_path):
    from coati_amd import _lib, build
    gone = str(tmp_path / "include" / "coati_guide.h")
    monkeypatch.setattr(build, "GUIDE_HEADER", gone)
    try:
        with pytest.raises(RuntimeError, match="coati_guide.h"):
            importlib.reload(_lib)
    finally:
        monkeypatch.undo()
        importlib.reload(_lib)
    assert sorted(_lib.GUIDE_PROTOTYPES) == ["coati_head_grad"]


def test_head_grad_refuses_bad_arguments_with_a_code():
    """decided on the host before any device call: the pointers are host buffers that a refusal never looks at"""
    from coati_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    off = ctypes.c_void_p(p.value + 4)

    def call(x=p, ldx=64, N=100, E=64, w0=p, b0=p, wr=p, br=p, D=2, wl=p, bl=p, P=1, F=64, w0t=p, wrt=p, cot=p, ldc=1, out=p, ldo=1, g=p,
             ldg=64):
        rc = l.coati_head_grad(x, ldx, N, E, w0, b0, wr, br, D, wl, bl, P, F, w0t, wrt, cot, ldc, out, ldo, g, ldg, None)
        return rc, l.coati_last_error().decode()

    cases = [dict(x=None), dict(w0=None), dict(b0=None), dict(wr=None), dict(br=None), dict(wl=None), dict(bl=None), dict(w0t=None),
             dict(wrt=None), dict(cot=None), dict(out=None), dict(g=None), dict(wrt=None, D=1), dict(wr=None, D=1),
             dict(E=48, ldx=48, ldg=48), dict(E=544, ldx=544, ldg=544), dict(E=0), dict(F=96), dict(F=512), dict(D=-1), dict(D=17),
             dict(P=0), dict(P=9, ldo=9, ldc=9), dict(N=0), dict(N=2 ** 31), dict(ldx=32), dict(ldx=68), dict(P=3, ldo=2, ldc=3),
             dict(P=3, ldo=3, ldc=2), dict(ldg=32), dict(ldg=66), dict(g=off), dict(w0t=off), dict(wrt=off),
             dict(x=ctypes.c_void_p(p.value + 2))]
    for kw in cases:
        rc, msg = call(**kw)
        assert rc < 0 and "head_grad" in msg, (kw, rc, msg)
    assert not any(buf.raw)                                                                   # nothing was touched


# ---- reference_grad ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_grad_on_exact_heads_is_the_same_in_any_arithmetic(shape):
    E, F, D, P = shape
    head = U.exact_head(E, F, D, P, seed=100 + G.EXACT_SHAPES.index(shape))
    rows, cot = U.exact_rows(300, E, seed=7), G.exact_cot(300, P, seed=8)
    out64, g64 = head.reference_grad(rows, cot)
    assert out64.dtype == torch.float64 and g64.shape == (300, E) and torch.equal(out64, head.reference(rows))
    out32, g32 = head.reference_grad(rows, cot, torch.float32)
    assert out32.dtype == torch.float32 and torch.equal(out32.double(), out64) and torch.equal(g32.double(), g64)
    out8, g8, _ = G.restate(head, rows, cot, torch.float32, chunks=8)
    assert torch.equal(out8.double(), out64) and torch.equal(g8.double(), g64)
    o1, g1, _ = G.restate(head, rows, cot)                                                    # the test's restatement is reference_grad
    assert torch.equal(o1, out64) and torch.equal(g1, g64)
    assert bool((g64.abs().sum(dim=1) > 0).float().mean() > 0.5)                              # (and it is not a table of zeros)


@pytest.mark.parametrize("shape", G.EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_grad_without_rounding_is_autograd_through_forward(shape):
    E, F, D, P = shape
    torch.manual_seed(30 + G.EXACT_SHAPES.index(shape))
    from coati_amd.models.regression import PropertyHead
    head = PropertyHead(E, features=F, depth=D, num_outputs=P)
    x16 = torch.randn(64, E).to(torch.bfloat16)
    cot = torch.randn(64, P, dtype=torch.float64)
    out, g = head.reference_grad(x16, cot, round_fn=lambda t: t.detach().to(torch.float64))
    head.double()
    x = x16.double().requires_grad_(True)
    values = head(x)
    (want,) = torch.autograd.grad((values * cot).sum(), x)
    head.float()
    scale = float(want.abs().max())
    assert float((out - values.detach()).abs().max()) <= 1e-12 * max(1.0, float(values.abs().max()))
    assert float((g - want).abs().max()) <= 1e-12 * max(1.0, scale), float((g - want).abs().max())


def test_reference_grad_pads_and_checks_its_arguments():
    from coati_amd.models.regression import PropertyHead
    torch.manual_seed(2)
    head = PropertyHead(40, features=64, depth=2, num_outputs=3)
    x16, cot = torch.randn(20, 40).to(torch.bfloat16), torch.randn(20, 3)
    out, g = head.reference_grad(x16, cot)
    outp, gp = head.reference_grad(torch.nn.functional.pad(x16, (0, 24)), cot)
    assert gp.shape == (20, 64) and torch.equal(gp[:, :40], g) and bool((gp[:, 40:] == 0).all()) and torch.equal(outp, out)
    with pytest.raises(ValueError):
        head.reference_grad(x16.float(), cot)
    with pytest.raises(ValueError):
        head.reference_grad(x16, cot[:, :2])
    w0t, wrt = head._grad_operands()
    w0, _, wr, _, _, _ = head._operands()
    assert w0t.shape == (64, 64) and torch.equal(w0t, w0.T) and w0t.is_contiguous()
    assert wrt.shape == (2, 64, 64) and torch.equal(wrt, wr.transpose(1, 2)) and wrt.is_contiguous()
    with torch.no_grad():
        head.residuals[0].weight.mul_(2.0)
    assert torch.equal(head._grad_operands()[1][0], head.residuals[0].weight.detach().to(torch.bfloat16).T)      # one cache key
    assert PropertyHead(32, features=64, depth=0)._grad_operands()[1] is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head.value_and_grad(torch.randn(5, 40))
    with pytest.raises(ValueError, match="cotangent"):
        head.value_and_grad(torch.randn(5, 40), torch.ones(2))
    assert [t.shape for t in head.grad_rows(torch.zeros(0, 64, dtype=torch.bfloat16), torch.zeros(0, 3))] == [(0, 3), (0, 64)]


def test_unit_input_chain_is_the_gradient_through_the_normalisation():
    from coati_amd.models.regression.property_head import unit_input_chain
    torch.manual_seed(3)
    x = (torch.randn(50, 37, dtype=torch.float64) * 3.0).requires_grad_(True)
    a = torch.randn(50, 37, dtype=torch.float64)
    u = x / x.norm(dim=1, keepdim=True)
    f = (torch.sin(u) * a).sum()                                                              # any function of u
    (g_u,) = torch.autograd.grad(f, u, retain_graph=True)
    (want,) = torch.autograd.grad(f, x)
    got = unit_input_chain(g_u.detach(), x.detach())
    assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-15
    assert unit_input_chain(g_u.detach().float(), x.detach()).dtype == torch.float32


# ---- guided_ascent ------------------------------------------------------------------------------------------------------------------
def _objective_run(head, start, w, steps, lr, anchor, bump_every, height, width, max_step):
    """the loop written out from its objective: autograd of J_i, centres kept in a list"""
    v, centres, visited = start.clone(), [], []
    for t in range(steps):
        if bump_every and t > 0 and t % bump_every == 0:
            centres.append(v.clone())
        visited.append(v.clone())
        x = v.clone().requires_grad_(True)
        J = (head(x) * w).sum(dim=1) - anchor * ((x - start) ** 2).sum(dim=1)
        for c in centres:
            J = J - height * torch.exp(-((x - c) ** 2).sum(dim=1) / (2 * width ** 2))
        (grad,) = torch.autograd.grad(J.sum(), x)
        step = lr * grad
        if max_step is not None:
            length = step.norm(dim=1, keepdim=True)
            step = torch.where(length > max_step, step * (max_step / length), step)
        v = v + step
    return v, centres, visited


@pytest.mark.parametrize("anchor, bump_every, max_step", [(0.0, 0, None), (0.3, 0, None), (0.0, 3, None), (0.3, 3, 0.02), (0.0, 0, 0.01)])
def test_guided_ascent_follows_its_objective(anchor, bump_every, max_step):
    from coati_amd.generative import guided_ascent
    from coati_amd.models.regression import PropertyHead
    torch.manual_seed(11)
    head = PropertyHead(24, features=64, depth=2, num_outputs=2).double()
    start = torch.randn(9, 24, dtype=torch.float64)
    w = torch.tensor([1.0, -0.5], dtype=torch.float64)
    res = guided_ascent(start, head, weights=[1.0, -0.5], steps=12, lr=0.05, anchor=anchor, bump_every=bump_every, bump_height=0.7,
                        bump_width=0.4, max_step=max_step, value_and_grad=G.autograd_value_and_grad(head))
    want, centres, visited = _objective_run(head, start, w, 12, 0.05, anchor, bump_every, 0.7, 0.4, max_step)
    assert res.vectors.dtype == torch.float64 and float((res.vectors - want).abs().max()) <= 1e-10
    assert res.history.shape == (13, 9) and res.values.shape == (9, 2)
    assert float((res.values - head(want).detach()).abs().max()) <= 1e-9
    assert float((res.history[0] - (head(start).detach() * w).sum(dim=1)).abs().max()) <= 1e-12
    assert float((res.history[-1] - (res.values * w).sum(dim=1)).abs().max()) <= 1e-12
    assert res.n_centres == len(centres) == (3 if bump_every else 0)
    for m, c in enumerate(centres):                                                           # the hills stand on visited points
        assert float((res.centres[:, m] - c).abs().max()) <= 1e-10 and float((c - visited[bump_every * (m + 1)]).abs().max()) == 0.0
    assert bool((res.centres[:, res.n_centres:] == 0).all()) and res.centres.shape == (9, 64, 24)
    if max_step is not None:
        assert not torch.equal(want, _objective_run(head, start, w, 12, 0.05, anchor, bump_every, 0.7, 0.4, None)[0])     # it did clip
    again = guided_ascent(start, head, weights=[1.0, -0.5], steps=12, lr=0.05, anchor=anchor, bump_every=bump_every, bump_height=0.7,
                          bump_width=0.4, max_step=max_step, value_and_grad=G.autograd_value_and_grad(head))
    assert torch.equal(again.vectors, res.vectors) and torch.equal(again.history, res.history)


def test_guided_ascent_refuses_a_65th_centre_before_the_first_step():
    from coati_amd.generative import guided_ascent
    from coati_amd.models.regression import PropertyHead
    head = PropertyHead(8, features=64, depth=0)
    calls = []

    def never(v, cot):
        calls.append(1)
        raise AssertionError("a step was taken")

    with pytest.raises(ValueError, match="64"):
        guided_ascent(torch.zeros(2, 8), head, steps=66, bump_every=1, value_and_grad=never)
    assert not calls
    ok = guided_ascent(torch.zeros(2, 8), head, steps=65, bump_every=1, lr=0.0, value_and_grad=G.autograd_value_and_grad(head))
    assert ok.n_centres == 64
    with pytest.raises(ValueError, match="weights"):
        guided_ascent(torch.zeros(2, 8), head, weights=[1.0, 2.0], steps=1, value_and_grad=never)


# ---- guided_generation on stubs -----------------------------------------------------------------------------------------------------
class _Head:
    """value = the second channel; its gradient is constant"""
    num_outputs = 1
    device = torch.device("cpu")

    def predict(self, v):
        return torch.as_tensor(v)[:, 1:2].clone()

    def value_and_grad(self, v, cot=None):
        g = torch.zeros_like(v)
        g[:, 1] = 1.0 if cot is None else float(cot[0])
        return v[:, 1:2].clone(), g


def test_guided_generation_drops_sorts_and_passes_the_grammar():
    from coati_amd.generative import guided_generation
    seen = {}

    def decode(V):                                           # the name is channel 0; every third end point does not decode
        return [None if int(v[0]) % 3 == 2 else f"C{int(v[0])}" for v in V]

    def embed(strings):
        e = torch.zeros(len(strings), 4)
        for i, s in enumerate(strings):
            e[i, 0] = float(s[1:])
            e[i, 1] = -float(s[1:]) if s[1:] != "4" else 50.0                                # the decoded molecule scores on its own
        return e

    start = torch.zeros(6, 4)
    start[:, 0] = torch.arange(6).float()
    start[:, 1] = torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0, 5.0])
    recs = guided_generation(start, _Head(), None, None, steps=10, lr=0.1, decode=decode, embed=embed)
    assert [r["start"] for r in recs] == [4, 0, 1, 3] and [r["smiles"] for r in recs] == ["C4", "C0", "C1", "C3"]
    assert [r["decoded_value"] for r in recs] == [50.0, 0.0, -1.0, -3.0]
    assert recs[1]["start_value"] == 0.0 and abs(recs[1]["vector_value"] - 1.0) < 1e-6      # ten steps of 0.1 up the second channel
    assert set(recs[0]) == {"start", "smiles", "start_value", "vector_value", "decoded_value"}
    assert guided_generation(start[2:3], _Head(), None, None, steps=1, decode=decode, embed=embed) == []

    # strings in: embedded with the same callable, named by their string; the default decoder gets grammar=
    from coati_amd.generative import coati_guide
    def fake_decoder(V, encoder, tokenizer, canon_smiles=None, generator=None, grammar=None, **kw):
        seen["grammar"], seen["canon"] = grammar, canon_smiles
        return [f"C{int(v[0])}" for v in V]
    real = coati_guide._P.force_decode_valid_batches
    coati_guide._P.force_decode_valid_batches = fake_decoder
    try:
        recs = guided_generation(["C7", "C1"], _Head(), None, None, steps=2, lr=0.1, grammar="the grammar", canon_smiles="canon", embed=embed)
    finally:
        coati_guide._P.force_decode_valid_batches = real
    assert seen == {"grammar": "the grammar", "canon": "canon"}
    assert [r["start"] for r in recs] == ["C1", "C7"] and [r["decoded_value"] for r in recs] == [-1.0, -7.0]


def test_generative_exports():
    import coati.generative as CG
    import coati_amd.generative as AG
    from coati_amd.generative import coati_guide
    assert AG.guided_ascent is coati_guide.guided_ascent and AG.guided_generation is coati_guide.guided_generation
    assert CG.guided_ascent is coati_guide.guided_ascent
    from coati_amd.models.autograd_funs import property as prop
    assert callable(prop.head_fused)
