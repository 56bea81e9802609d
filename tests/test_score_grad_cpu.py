"""The likelihood's gradient w.r.t. the injected embedding, host side: the C ABI declares and exports coati_engine_score_grad and refuses
what it must before anything reaches a device; the fixture tests/golden/score_grad_golden.npz (gen_golden_score_grad.py, autograd through
the imported reference) is consistent with itself; HclipLikelihood wires Engine.score / Engine.score_grad into torch.autograd.  Needs no
GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "score_grad_golden.npz"))


def test_header_declares_and_library_exports_score_grad():
    from coati_amd import _lib
    assert "coati_engine_score_grad" in _lib.PROTOTYPES, "include/coati_hip.h does not declare coati_engine_score_grad"
    restype, argtypes = _lib.PROTOTYPES["coati_engine_score_grad"]
    assert restype is ctypes.c_int and len(argtypes) == 14
    assert "coati_engine_score_grad" in _lib.exported_symbols()
    l = _lib.lib()
    assert hasattr(l, "coati_engine_score_grad")
    assert l.coati_abi_version() == 5          # additive: the ABI version does not move


def _engine(l, fp8=0, coati2=None):
    from coati_amd import _lib
    cfg = _lib.CoatiConfig(2, 2, 128, 64, 128, 8, 24, 48, 5.0, 0, 1, 7, fp8, 1, 1, 0 if coati2 is not None else 1, 1)
    h = ctypes.c_void_p()
    if coati2 is None:
        assert l.coati_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, l.coati_last_error()
    else:
        assert l.coati_engine_create_coati2(ctypes.byref(cfg), coati2, ctypes.byref(h)) == 0, l.coati_last_error()
    return h


def test_score_grad_refuses_with_a_code_and_a_message():
    """COATI2 engines, fp8 engines and null arguments: an error code and coati_last_error, decided on the host before the workspace is
    carved or anything is enqueued (the pointers below are host buffers: a launch would fault, a refusal never looks at them)."""
    from coati_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(h, h_clip=p, dh=p, tokens=p, nll=p):
        return l.coati_engine_score_grad(h, p, 4096 * 4, 1, 8, h_clip, tokens, p, 0, None, nll, dh, p, None)

    for h, word in ((_engine(l, coati2=0), b"COATI2"), (_engine(l, fp8=1), b"fp8")):
        assert call(h) == -1 and word in l.coati_last_error(), l.coati_last_error()
        l.coati_engine_destroy(h)
    h = _engine(l)
    assert call(None) == -1 and b"null" in l.coati_last_error()
    assert call(h, h_clip=None) == -1 and b"null" in l.coati_last_error()
    assert call(h, dh=None) == -1 and b"null" in l.coati_last_error()
    assert call(h, tokens=None) == -1 and b"engine_score_grad" in l.coati_last_error()     # (an unbound engine: refused either way)
    l.coati_engine_destroy(h)


@pytest.mark.parametrize("part", ["small", "grande"])
def test_fixture_gradient_agrees_with_its_central_difference(golden, part):
    """|dh| from autograd against the stored directional central difference along dh (eps 1e-2, float64): 5e-3 relative on every row."""
    dh, cd = golden[part + ".dh"].astype(np.float64), golden[part + ".cd"].astype(np.float64)
    n = np.linalg.norm(dh, axis=1)
    assert dh.shape[0] == cd.shape[0] == golden[part + ".nll"].shape[0] and (n > 0).all()
    rel = np.abs(cd - n) / n
    print(f"{part}: |dh| {n.min():.3f} .. {n.max():.3f}, central difference vs |dh| worst rel {rel.max():.2e}")
    assert (rel <= 5e-3).all(), rel


def test_fixture_descent_trajectory_is_strictly_decreasing(golden):
    t = golden["small.traj"].astype(np.float64)
    assert t.shape == (6, 11) and np.array_equal(t[:, 0].astype(np.float32), golden["small.nll"])
    assert (np.diff(t, axis=1) < 0).all(), t
    assert ((t[:, 0] - t[:, -1]) > 0.4).all()      # the drops the descent test on the device halves: 0.46 .. 0.96


def test_fixture_grande_rows_are_masked_like_the_reference(golden):
    tok, y = golden["grande.tokens"], golden["grande.y_next"]
    assert tok.shape == y.shape == (16, 63) and (tok[:, :5] == np.array([8, 7, 2, 5, 6])).all()
    n = (tok != 0).sum(1)
    assert n.min() >= 14 and n.max() <= 63
    for b in range(16):
        assert tok[b, n[b] - 1] == 1 and (y[b, :4] == -1).all() and (y[b, 4:n[b] - 1] == tok[b, 5:n[b]]).all() and (y[b, n[b] - 1:] == -1).all()


class _FakeEngine:
    """records the calls; nll = sum h^2 per row, so that d nll / d h = 2 h"""

    def __init__(self):
        self.calls = []

    def score(self, tokens, y_next, h_clip=None, raw_tokens=None, rows=None):
        self.calls.append(("score", h_clip.requires_grad, rows))
        return (h_clip.detach() ** 2).sum(1)

    def score_grad(self, tokens, y_next, h_clip, weights=None, rows=None):
        self.calls.append(("score_grad", weights.clone(), rows))
        return (h_clip.detach() ** 2).sum(1), weights[:, None] * 2 * h_clip.detach()


def test_hclip_likelihood_autograd_wiring():
    from coati_amd.models.autograd_funs.likelihood import HclipLikelihood
    eng = _FakeEngine()
    h = torch.randn(3, 5, requires_grad=True)
    tok = torch.zeros(3, 4, dtype=torch.long)
    y = torch.zeros(3, 4, dtype=torch.long).requires_grad_(False)
    nll = HclipLikelihood.apply(h, eng, tok, y, (0, 9))
    assert nll.requires_grad and nll.grad_fn is not None and [c[0] for c in eng.calls] == ["score"]     # forward: the cheap path only
    w = torch.tensor([1.0, 0.0, -2.5])
    (nll * w).sum().backward()
    assert [c[0] for c in eng.calls] == ["score", "score_grad"]
    assert torch.equal(eng.calls[1][1], w) and eng.calls[1][2] == (0, 9)          # grad_output goes in as the weights, rows pass through
    assert h.grad.shape == (3, 5) and torch.allclose(h.grad, w[:, None] * 2 * h.detach())
    assert tok.grad is None and y.grad is None
    # no gradient wanted: nothing recorded
    eng2 = _FakeEngine()
    with torch.no_grad():
        out = HclipLikelihood.apply(h, eng2, tok, y, None)
    assert not out.requires_grad and [c[0] for c in eng2.calls] == ["score"]
