"""COATI2 likelihood scoring and its gradient w.r.t. the embedding, host side: the C ABI declares and exports coati_engine_score_coati2,
coati_engine_score_grad_coati2 and coati_swiglu_bwd and refuses what it must before anything reaches a device; the fixture
tests/golden/coati2_likelihood_golden.npz (gen_golden_coati2_likelihood.py, autograd through the imported reference's modules) is
consistent with itself; HcoatiLikelihood wires Engine.score_coati2 / Engine.score_grad_coati2 into torch.autograd; the token builders
give the fixture's rows.  Needs no GPU."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANTS = ("linear", "swiglu_mlp", "swiglu_resnet")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "coati2_likelihood_golden.npz"))


@pytest.fixture(scope="module")
def tokenizer(golden_dir):
    from coati_amd.models.simple_coati2.trie_tokenizer import TrieTokenizer
    v = json.load(open(os.path.join(golden_dir, "coati2_vocab.json")))
    return TrieTokenizer(n_seq=v["n_seq"], special_tokens=v["special_tokens"], smiles_tokens=v["smiles_tokens"])


# ---- 1. the C ABI ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_args", [("coati_engine_score_coati2", 15), ("coati_engine_score_grad_coati2", 14), ("coati_swiglu_bwd", 9)])
def test_header_declares_and_library_exports(name, n_args):
    from coati_amd import _lib
    assert name in _lib.PROTOTYPES, f"include/coati_hip.h does not declare {name}"
    restype, argtypes = _lib.PROTOTYPES[name]
    assert restype is ctypes.c_int and len(argtypes) == n_args
    assert name in _lib.exported_symbols()
    l = _lib.lib()
    assert hasattr(l, name)
    assert l.coati_abi_version() == 5          # additive: the ABI version does not move
    assert _lib.ABI_VERSION == 5               # (COATI_ABI_VERSION of the header)


def _engine(l, coati2=None):
    from coati_amd import _lib
    cfg = _lib.CoatiConfig(2, 2, 128, 64, 128, 8, 24, 48, 5.0, 0, 1, 7, 0, 1, 1, 0 if coati2 is not None else 1, 1)
    h = ctypes.c_void_p()
    if coati2 is None:
        assert l.coati_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, l.coati_last_error()
    else:
        assert l.coati_engine_create_coati2(ctypes.byref(cfg), coati2, ctypes.byref(h)) == 0, l.coati_last_error()
    return h


def test_new_entries_refuse_with_a_code_and_a_message():
    """COATI1 engines, null arguments and bad shapes: an error code and a coati_last_error that names the entry, decided on the host before
    the workspace is carved or anything is enqueued (the pointers below are host buffers: a launch would fault, a refusal never looks at
    them; the engines are not bound, so a call that got past every check would be refused as unbound, with another message)."""
    from coati_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nbytes = 4096 * 4

    def score(h, B=1, T1=1, T2=8, raw=None, hc=p, tokens=p, y=p, r1=0, r2=0, nll=p, scal=p, ws=p):
        return l.coati_engine_score_coati2(h, ws, nbytes, B, T1, T2, raw, hc, tokens, y, r1, r2, nll, scal, None)

    def grad(h, B=1, T2=8, hc=p, tokens=p, y=p, r2=0, nll=p, dh=p, scal=p, ws=p):
        return l.coati_engine_score_grad_coati2(h, ws, nbytes, B, T2, hc, tokens, y, r2, None, nll, dh, scal, None)

    def err():
        return l.coati_last_error()

    c1 = _engine(l)
    assert score(c1) == -1 and b"COATI2" in err() and b"engine_score_coati2" in err(), err()
    assert grad(c1) == -1 and b"COATI2" in err() and b"engine_score_grad_coati2" in err(), err()
    l.coati_engine_destroy(c1)
    for variant in (0, 1, 2):
        h = _engine(l, coati2=variant)
        # null arguments
        assert score(None) == -1 and b"null" in err() and b"engine_score_coati2" in err()
        for kw in (dict(tokens=None), dict(y=None), dict(nll=None), dict(scal=None), dict(ws=None)):
            assert score(h, **kw) == -1 and b"null" in err() and b"engine_score_coati2" in err(), (kw, err())
            assert grad(h, **kw) == -1 and b"null" in err() and b"engine_score_grad_coati2" in err(), (kw, err())
        assert grad(None) == -1 and b"null" in err() and b"engine_score_grad_coati2" in err()
        assert grad(h, hc=None) == -1 and b"null" in err() and b"engine_score_grad_coati2" in err()
        assert grad(h, dh=None) == -1 and b"null" in err() and b"engine_score_grad_coati2" in err()
        # exactly one of raw_tokens / h_coati
        assert score(h, hc=None) == -1 and b"exactly one" in err() and b"h_coati" in err()
        assert score(h, raw=p) == -1 and b"exactly one" in err() and b"engine_score_coati2" in err()
        # shapes: B, T2 beyond n_seq = 24, T1 beyond n_seq, packed row counts that do not fit
        for kw in (dict(B=0), dict(T2=0), dict(T2=25), dict(r2=9), dict(r2=-1)):
            assert score(h, **kw) == -2 and b"engine_score_coati2" in err(), (kw, err())
            assert grad(h, **kw) == -2 and b"engine_score_grad_coati2" in err(), (kw, err())
        assert score(h, raw=p, hc=None, T1=25) == -2 and b"engine_score_coati2" in err()
        assert score(h, raw=p, hc=None, T1=8, r1=0, r2=5) == -2 and b"packed" in err()     # packed rows for one pass only
        # everything in order but the engine has no buffers bound: refused as such, still on the host
        assert score(h) == -1 and b"not bound" in err() and b"engine_score_coati2" in err()
        assert grad(h) == -1 and b"not bound" in err() and b"engine_score_grad_coati2" in err()
        l.coati_engine_destroy(h)


# ---- 2. the fixture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", VARIANTS + ("full",))
def test_fixture_gradient_agrees_with_its_central_difference(golden, part):
    """|dh| from autograd against the stored directional central difference along dh (eps 1e-2, float64): 5e-3 relative on every row."""
    dh, cd = golden[part + ".dh"].astype(np.float64), golden[part + ".cd"].astype(np.float64)
    n = np.linalg.norm(dh, axis=1)
    assert dh.shape[0] == cd.shape[0] == golden[part + ".nll"].shape[0] == 16 and (n > 0).all()
    assert dh.shape == golden[part + ".h"].shape
    rel = np.abs(cd - n) / n
    print(f"{part}: |dh| {n.min():.3f} .. {n.max():.3f}, central difference vs |dh| worst rel {rel.max():.2e}")
    assert (rel <= 5e-3).all(), rel


@pytest.mark.parametrize("variant", VARIANTS)
def test_fixture_descent_trajectories_are_strictly_decreasing(golden, variant):
    t = golden[variant + ".traj"].astype(np.float64)
    assert t.shape == (16, 11) and np.array_equal(t[:, 0].astype(np.float32), golden[variant + ".nll"])
    assert float(golden[variant + ".step"]) in (20.0, 10.0, 5.0, 2.0, 1.0)
    assert (np.diff(t, axis=1) < 0).all(), t


@pytest.mark.parametrize("part", ["small", "full"])
def test_fixture_rows_are_masked_like_the_reference(golden, part):
    tok, y = golden[part + ".tokens"], golden[part + ".y_next"]
    masked, stop, pad = set(golden["masked_ids"].tolist()), int(golden["stop_token"]), int(golden["pad_token"])
    assert masked == {2, 31, 39, 44, 41, 21} and stop == 40 and pad == 31
    assert tok.shape == y.shape and tok.shape[0] == 16
    n = (tok != pad).sum(1)
    for b in range(16):
        sfx = bool(golden["small.do_suffix"][b]) if part == "small" else bool(b % 2)
        pre = [2, 44, 39] + ([41, 21] if sfx else [])
        P = len(pre)
        assert tok[b, :P].tolist() == pre and tok[b, n[b] - 1] == stop and (tok[b, n[b]:] == pad).all()
        assert not (set(y[b].tolist()) & masked)                                   # no target is a masked id
        assert (y[b, :P - 1] == -1).all() and (y[b, n[b] - 1:] == -1).all()        # nothing predicted inside the prompt or behind [STOP]
        assert (y[b, P - 1:n[b] - 1] == tok[b, P:n[b]]).all() and y[b, n[b] - 2] == stop   # every row's last target is [STOP]
    if part == "full":
        assert n.min() >= 3 + 8 + 1 and n.max() <= 5 + 57 + 1 and (tok[tok != pad] < 4266).all()
        body = [tok[b, (5 if b % 2 else 3):n[b] - 1] for b in range(16)]
        assert all((r >= 330).all() for r in body)


def test_fixture_full_weight_recipe_reproduces_its_checksums(golden):
    from tests.coati2_full_weights import SEED, checksums, full_param_shapes, full_weights
    names = [n for n, _ in full_param_shapes()]
    assert names == [str(n) for n in golden["full.names"]] and int(golden["full.seed"]) == SEED
    W = full_weights()
    assert all(tuple(W[n].shape) == s and W[n].dtype == torch.float32 for n, s in full_param_shapes())
    ws, wa = checksums(W, names)
    assert np.allclose(ws, golden["full.wsum"], rtol=0, atol=1e-6 * np.abs(golden["full.wabs"]).max())
    assert np.allclose(wa, golden["full.wabs"], rtol=1e-9)


def test_fixture_round_trip_rows(golden):
    """the round trip's embedding is the stored encode row, so its NLL is that of the plain row (the fixture's two routes agree)"""
    assert golden["s2s.mask"].tolist() == [True] * 8 + [False, False]
    for v in VARIANTS:
        assert golden[v + ".s2s.nll"].shape == (8,)
        assert np.allclose(golden[v + ".s2s.nll"], golden[v + ".nll"][:8], rtol=1e-5)


# ---- 3. autograd wiring -----------------------------------------------------------------------------------------------------------------
class _FakeEngine:
    """records the calls; nll = sum h^2 per row, so that d nll / d h = 2 h"""

    def __init__(self):
        self.calls = []

    def score_coati2(self, tokens, y_next, h_coati=None, raw_tokens=None, rows=None):
        self.calls.append(("score_coati2", h_coati.requires_grad, rows))
        return (h_coati.detach() ** 2).sum(1)

    def score_grad_coati2(self, tokens, y_next, h_coati, weights=None, rows=None):
        self.calls.append(("score_grad_coati2", weights.clone(), rows))
        return (h_coati.detach() ** 2).sum(1), weights[:, None] * 2 * h_coati.detach()


def test_hcoati_likelihood_autograd_wiring():
    from coati_amd.models.autograd_funs.likelihood import HcoatiLikelihood, hcoati_likelihood
    eng = _FakeEngine()
    h = torch.randn(3, 5, requires_grad=True)
    tok = torch.zeros(3, 4, dtype=torch.long)
    y = torch.zeros(3, 4, dtype=torch.long)
    nll = HcoatiLikelihood.apply(h, eng, tok, y, (0, 9))
    assert nll.requires_grad and nll.grad_fn is not None and [c[0] for c in eng.calls] == ["score_coati2"]     # forward: the cheap path only
    w = torch.tensor([1.0, 0.0, -2.5])
    (nll * w).sum().backward()
    assert [c[0] for c in eng.calls] == ["score_coati2", "score_grad_coati2"]
    assert torch.equal(eng.calls[1][1], w) and eng.calls[1][2] == (0, 9)          # grad_output goes in as the weights, rows pass through
    assert h.grad.shape == (3, 5) and torch.allclose(h.grad, w[:, None] * 2 * h.detach())
    assert tok.grad is None and y.grad is None
    eng2 = _FakeEngine()
    with torch.no_grad():
        out = hcoati_likelihood(h, eng2, tok, y)
    assert not out.requires_grad and [c[0] for c in eng2.calls] == ["score_coati2"]


# ---- 4. token builders ------------------------------------------------------------------------------------------------------------------
def test_token_builders_give_the_fixture_rows(golden, tokenizer, golden_dir):
    from coati_amd.models.encoding.clip_e2e import hcoati_likelihood_tokens, injection_prefix, s2s_hcoati_likelihood_tokens
    smiles = [str(s) for s in golden["smiles"]]
    pad = tokenizer.pad_token
    ref_tok, ref_y = torch.from_numpy(golden["small.tokens"]), torch.from_numpy(golden["small.y_next"])
    for sfx, sl in ((False, slice(0, 8)), (True, slice(8, 16))):
        tok, y = hcoati_likelihood_tokens(smiles, tokenizer, do_suffix=sfx)
        T = tok.shape[1]
        assert tok[0, :(5 if sfx else 3)].tolist() == injection_prefix(tokenizer, "[SMILES]", sfx)
        assert torch.equal(tok, ref_tok[sl, :T]) and torch.equal(y, ref_y[sl, :T])
        assert bool((ref_tok[sl, T:] == pad).all()) and bool((ref_y[sl, T:] == -1).all())
    # the round trip: the rows that fit, the mask, the encoder rows of coati2_golden.npz
    s2s = [str(s) for s in golden["s2s.smiles"]]
    raw, tok, y, mask = s2s_hcoati_likelihood_tokens(s2s, tokenizer)
    assert mask.tolist() == golden["s2s.mask"].tolist() and raw.shape[0] == tok.shape[0] == y.shape[0] == 8
    tok8, y8 = hcoati_likelihood_tokens(smiles, tokenizer)
    assert torch.equal(tok, tok8) and torch.equal(y, y8)
    enc = torch.from_numpy(np.load(os.path.join(golden_dir, "coati2_golden.npz"))["tokens"])
    assert torch.equal(raw, enc[:, :raw.shape[1]]) and bool((enc[:, raw.shape[1]:] == pad).all())
    # over-long SMILES ("CC" is one piece): 29 ids with [STOP] fit behind the 3 prompt ids of n_seq = 32, 30 do not -- although the
    # string alone would fit n_seq; behind the 5 ids of the suffix form 27 fit
    assert tokenizer.n_seq == 32
    _, _, _, m = s2s_hcoati_likelihood_tokens(["C" * 56, "C" * 57], tokenizer)
    assert m.tolist() == [True, False]
    _, _, _, m = s2s_hcoati_likelihood_tokens(["C" * 52, "C" * 53], tokenizer, do_suffix=True)
    assert m.tolist() == [True, False]
    raw, tok, y, m = s2s_hcoati_likelihood_tokens(["C" * 59], tokenizer)
    assert m.tolist() == [False] and raw.shape[0] == tok.shape[0] == y.shape[0] == 0
