"""The likelihood's gradient w.r.t. the injected embedding on the engine (coati_engine_score_grad: ce_seq_bwd_kernel, EPI_CE_BWD_ROW, the
inputs-only decoder backward, the token head's backward to dh): parity with autograd through the reference (tests/golden/
score_grad_golden.npz) at the small and the grande shape, the constructor flags against the oracle's autograd, the weights' semantics, the
row split above 65 536 rows, gradient descent, the absence of side effects, and the refusals."""
import contextlib
import io
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.gpu_util import log  # noqa: E402
from tests.test_gpu_engine import TOL_GRAD, TOL_GRAD_SIM  # noqa: E402

DEV = "cuda:0"
SMALL = dict(n_layer_e3gnn=2, n_layer_xformer=2, n_hidden_xformer=64, n_hidden_e3nn=64, n_embd_common=64, n_head=4,
             n_seq=24, n_tok=48)
GRANDE = dict(n_layer_e3gnn=5, n_layer_xformer=16, n_hidden_xformer=256, n_hidden_e3nn=256, n_embd_common=256, n_head=16,
              n_seq=250, n_tok=10322)
# Per-row error of dh: max|dh_b - ref_b| / max|ref_b|.  The bounds follow the rule at the top of test_gpu_engine.py -- at most 2x the
# worst value measured on the MI355X -- and never exceed TOL_GRAD, the project's bound for bf16-path gradients against the fp32 reference.
TOL_DH_SMALL = 1.7e-2     # measured 8.53e-3 (Engine.score_grad and the autograd route, batch form), 6.09e-3 (single form)
TOL_DH_GRANDE = 2.3e-2    # measured 1.17e-2 (padded and packed rows vs the reference), 1.10e-2 (a row of a 1024 x 82 call vs a 16-row call)
assert TOL_DH_SMALL <= TOL_GRAD and TOL_DH_GRANDE <= TOL_GRAD


def _quiet():
    return contextlib.redirect_stdout(io.StringIO())


def _row_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return (got - ref).abs().amax(1) / ref.abs().amax(1)


def _check_rows(name, got, ref, tol):
    assert bool(torch.isfinite(got).all()), name
    e = _row_err(got, ref)
    log(f"{name:60s} worst row err {float(e.max()):.3e}  tol {tol:.1e}  {'OK' if float(e.max()) <= tol else 'FAIL'}")
    print(f"{name}: worst row err {float(e.max()):.3e} (tol {tol:.1e})")
    assert float(e.max()) <= tol, (name, e)


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "score_grad_golden.npz"))


@pytest.fixture(scope="module")
def small(golden_dir, fixture):
    from coati_amd.models.encoding.clip_e2e import e3gnn_smiles_clip_e2e, hclip_likelihood_tokens
    from coati_amd.models.encoding.tokenizers import TrieTokenizer
    lk = np.load(os.path.join(golden_dir, "likelihood_golden.npz"))
    voc = json.load(open(os.path.join(golden_dir, "tokenizer.json")))
    tk = TrieTokenizer(n_seq=int(lk["n_seq"]), smiles_tokens=voc["smiles"], special_tokens=voc["special"])
    with _quiet():
        model = e3gnn_smiles_clip_e2e(**SMALL, device=torch.device(DEV))
    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "small_model_after3.npz")).items()}
    model.load_state_dict(sd, strict=False)
    smiles = [str(s) for s in fixture["small.smiles"]]
    tok, y = hclip_likelihood_tokens(smiles, tk)
    return model, tk, smiles, tok.to(DEV).contiguous(), y.to(DEV).contiguous(), sd


@pytest.fixture(scope="module")
def grande(fixture):
    from coati_amd.engine import Engine, ModelConfig
    from oracle import coati_oracle as O
    P = O.init_params(O.OracleConfig(**GRANDE), seed=int(fixture["grande.seed"]))
    names = [str(n) for n in fixture["grande.names"]]
    ws = np.array([float(P[n].double().sum()) for n in names])
    wa = np.array([float(P[n].double().abs().sum()) for n in names])
    assert np.allclose(ws, fixture["grande.wsum"], rtol=0, atol=1e-6 * np.abs(fixture["grande.wabs"]).max()) and \
        np.allclose(wa, fixture["grande.wabs"], rtol=1e-9), "init_params(seed) no longer reproduces the weights of score_grad_golden.npz"
    eng = Engine(ModelConfig(**GRANDE), DEV, train=False)
    eng.load_state_dict(P)
    return eng


# ---- 1. parity with the reference, small model ----------------------------------------------------------------------------------
def test_small_parity_direct_autograd_and_single_form(small, fixture):
    model, tk, smiles, tok, y, _ = small
    eng = model.engine
    h = torch.from_numpy(fixture["small.hclip"]).to(DEV)
    ref = torch.from_numpy(fixture["small.dh"])
    nll, dh = eng.score_grad(tok, y, h)
    nll, dh = nll.clone(), dh.clone()
    assert torch.equal(nll, eng.score(tok, y, h_clip=h))                       # the same bits as the scoring call
    assert float((nll.cpu() - torch.from_numpy(fixture["small.nll"])).abs().max()) <= 0.16
    _check_rows("small dh, Engine.score_grad vs reference autograd", dh, ref, TOL_DH_SMALL)
    # through the model's method and torch.autograd
    hg = h.clone().requires_grad_(True)
    out = model.hclip_and_tokens_to_likelihood(hg, smiles, tk)
    assert out.grad_fn is not None and out.shape == (len(smiles),)
    out.sum().backward()
    _check_rows("small dh, hclip_and_tokens_to_likelihood().sum().backward()", hg.grad, ref, TOL_DH_SMALL)
    # the reference's form: [E] + str -> [1]
    h3 = h[3].clone().requires_grad_(True)
    one = model.hclip_and_tokens_to_likelihood(h3, smiles[3], tk)
    assert one.shape == (1,)
    one.sum().backward()
    assert h3.grad.shape == h[3].shape
    _check_rows("small dh, single [E] + str form", h3.grad.unsqueeze(0), ref[3:4], TOL_DH_SMALL)
    # without a gradient request: the plain path, bit for bit, nothing recorded
    plain = model.hclip_and_tokens_to_likelihood(h, smiles, tk)
    with torch.no_grad():
        plain2 = model.hclip_and_tokens_to_likelihood(hg, smiles, tk)
    assert plain.grad_fn is None and plain2.grad_fn is None and torch.equal(plain, out.detach()) and torch.equal(plain2, plain)


# ---- 2. parity at the grande shape ---------------------------------------------------------------------------------------------------
def test_grande_parity_padded_and_packed(grande, fixture):
    eng = grande
    tok = torch.from_numpy(fixture["grande.tokens"]).to(DEV)
    y = torch.from_numpy(fixture["grande.y_next"]).to(DEV)
    h = torch.from_numpy(fixture["grande.hclip"]).to(DEV)
    ref = torch.from_numpy(fixture["grande.dh"])
    rows = (0, int((tok != 0).sum()))
    nll_p, dh_p = (t.clone() for t in eng.score_grad(tok, y, h))
    assert torch.equal(nll_p, eng.score(tok, y, h_clip=h))
    nll_k, dh_k = (t.clone() for t in eng.score_grad(tok, y, h, rows=rows))
    assert torch.equal(nll_k, eng.score(tok, y, h_clip=h, rows=rows))
    assert int(eng.scal[6:7].view(torch.int32).item()) == 0
    n_t = (y >= 0).sum(1).cpu().double()
    assert bool(((nll_p.cpu().double() - torch.from_numpy(fixture["grande.nll"]).double()).abs() <= 2e-2 * n_t).all())
    _check_rows("grande dh, padded rows vs reference autograd", dh_p, ref, TOL_DH_GRANDE)
    _check_rows("grande dh, packed rows vs reference autograd", dh_k, ref, TOL_DH_GRANDE)
    _check_rows("grande dh, packed vs padded", dh_k, dh_p, TOL_DH_GRANDE)


# ---- 3. constructor flags against the oracle's autograd --------------------------------------------------------------------------------
def _oracle_nll_grad(O, P, ocfg, tok, y, h):
    hg = h.clone().requires_grad_(True)
    with O.sim_bf16():
        inj = O.silu_linear(hg, P, token_mlp=ocfg.token_mlp)
        xf = O.xformer(tok, P, ocfg, injection=inj)
        logits = O.linear(O.rb(xf), P["xformer.lm_head.weight"])
        ce = torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), y.reshape(-1), ignore_index=-1, reduction="none")
        nll = ce.reshape(tok.shape).sum(1)
    nll.sum().backward()
    return nll.detach(), hg.grad


def _flag_rows(V, T=20, B=6, seed=5):
    """[CLIP][UNK][SMILES][SUFFIX][MIDDLE] body [STOP] rows; row 1 carries a second [UNK] inside its body, row 2 has no target at all"""
    g = torch.Generator().manual_seed(seed)
    tok = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        n = int(torch.randint(4, T - 6, (1,), generator=g))
        row = torch.cat([torch.tensor([8, 7, 2, 5, 6]), torch.randint(12, V, (n,), generator=g), torch.tensor([1])])
        tok[b, :len(row)] = row
    tok[1, 7] = 7
    y = torch.zeros_like(tok)
    y[:, :-1] = tok[:, 1:]
    for t in (8, 0, 2, 7, 5, 6):
        y[y == t] = -1
    y[2] = -1
    return tok, y


@pytest.mark.parametrize("flags", [dict(token_mlp=False), dict(norm_embed=True), dict(biases=False), dict()], ids=lambda f: "-".join(f) or "default")
def test_flags_vs_oracle_autograd(flags):
    from coati_amd.engine import Engine, ModelConfig
    from oracle import coati_oracle as O
    ocfg = O.OracleConfig(**SMALL, **flags)
    P = O.init_params(ocfg, seed=21)
    eng = Engine(ModelConfig(**SMALL, **flags), DEV, train=False)
    eng.load_state_dict(P)
    tok, y = _flag_rows(SMALL["n_tok"])
    assert int((tok[1] == 7).sum()) == 2 and int((y[2] >= 0).sum()) == 0
    h = torch.randn(tok.shape[0], SMALL["n_embd_common"], generator=torch.Generator().manual_seed(8))
    ref_nll, ref = _oracle_nll_grad(O, P, ocfg, tok, y, h)
    nll, dh = eng.score_grad(tok.to(DEV), y.to(DEV), h.to(DEV))
    tag = "-".join(flags) or "default"
    assert float((nll.cpu() - ref_nll).abs().max()) <= 2e-2 * int((y >= 0).sum(1).max())
    assert float(dh[2].abs().max()) == 0.0 and float(ref[2].abs().max()) == 0.0        # no target: exactly zero
    keep = [0, 1, 3, 4, 5]
    _check_rows(f"flags {tag}: dh vs oracle autograd (sim_bf16)", dh[keep], ref[keep], TOL_GRAD_SIM)
    # the row with two [UNK] positions: its gradient is the sum over both, i.e. it differs from what position 1 alone would give
    tok1 = tok.clone()
    tok1[1, 7] = 13
    _, dh1 = eng.score_grad(tok1.to(DEV), y.to(DEV), h.to(DEV))
    assert float((dh1[1] - dh[1]).abs().max()) > 1e-3 * float(dh[1].abs().max())


# ---- 4. semantics of the weights, row independence ---------------------------------------------------------------------------------------
def test_weights_scale_exactly_and_rows_are_independent(grande, fixture):
    eng = grande
    tok = torch.from_numpy(fixture["grande.tokens"]).to(DEV)
    y = torch.from_numpy(fixture["grande.y_next"]).to(DEV)
    h = torch.from_numpy(fixture["grande.hclip"]).to(DEV)
    B = tok.shape[0]
    nll1, dh1 = (t.clone() for t in eng.score_grad(tok, y, h))
    ones = torch.ones(B, device=DEV)
    nllw, dhw = (t.clone() for t in eng.score_grad(tok, y, h, weights=ones))
    assert torch.equal(dhw, dh1) and torch.equal(nllw, nll1)                     # None = ones
    nll4, dh4 = (t.clone() for t in eng.score_grad(tok, y, h, weights=4 * ones))
    assert torch.equal(nll4, nll1)                                               # the weights do not touch nll
    assert torch.equal(dh4, 4 * dh1)                                             # a power of two scales dlogits exactly, before rounding
    w = ones.clone()
    w[3], w[9], w[5] = 0.0, 0.5, -2.0
    _, dhz = eng.score_grad(tok, y, h, weights=w)
    assert float(dhz[3].abs().max()) == 0.0 and float(dhz[9].abs().max()) > 0
    assert torch.equal(dhz[9], 0.5 * dh1[9]) and torch.equal(dhz[5], -2.0 * dh1[5]) and torch.equal(dhz[0], dh1[0])
    # the same rows in another order, and one row alone
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(2)).to(DEV)
    _, dhp = eng.score_grad(tok[perm].contiguous(), y[perm].contiguous(), h[perm].contiguous())
    _check_rows("grande dh, rows in another batch order", dhp, dh1[perm], TOL_DH_GRANDE)
    for i in (4, 13):
        L = int((tok[i] != 0).sum())
        _, dha = eng.score_grad(tok[i:i + 1, :L].contiguous(), y[i:i + 1, :L].contiguous(), h[i:i + 1].contiguous())
        _check_rows(f"grande dh, row {i} alone vs in the batch", dha, dh1[i:i + 1], TOL_DH_GRANDE)


# ---- 5. more than 65 536 rows: the products run as two launches on equal row ranges -------------------------------------------------------
def _big_rows(B, T, V, seed):
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(8, T - 6 + 1, (B,), generator=g)
    body = torch.randint(1596, V, (B, T), generator=g)
    tok = torch.zeros(B, T, dtype=torch.long)
    tok[:, :5] = torch.tensor([8, 7, 2, 5, 6])
    ar = torch.arange(T).unsqueeze(0)
    inb = (ar >= 5) & (ar < 5 + n.unsqueeze(1))
    tok = torch.where(inb, body, tok)
    tok[torch.arange(B), 5 + n] = 1
    y = torch.zeros_like(tok)
    y[:, :-1] = tok[:, 1:]
    for t in (8, 0, 2, 7, 5, 6):
        y[y == t] = -1
    return tok, y


def test_row_split_advances_the_per_row_operands(grande):
    """B = 1024 x T2 = 82 padded rows = 83 968 > 65 536: lm_head partials, dlogits and the lm_head input gradient each run as two launches
    of 41 984 rows (sequences 0..511 | 512..1023).  Non-uniform weights: a launch that read the first half's per-row factors (or lse /
    targets) in the second half would give those rows another row's scale."""
    eng = grande
    B, T = 1024, 82
    tok, y = _big_rows(B, T, GRANDE["n_tok"], seed=77)
    assert B * T > 65536
    g = torch.Generator().manual_seed(78)
    h = torch.randn(B, GRANDE["n_embd_common"], generator=g)
    w = 0.25 + 2.0 * torch.rand(B, generator=g)
    tok, y, h, w = tok.to(DEV), y.to(DEV), h.to(DEV), w.to(DEV)
    nll, dh = (t.clone() for t in eng.score_grad(tok, y, h, weights=w))
    assert torch.equal(nll, eng.score(tok, y, h_clip=h))
    assert bool(torch.isfinite(dh).all())
    pick = torch.tensor([0, 1, 255, 509, 510, 511, 3, 77, 512, 513, 514, 700, 901, 1021, 1022, 1023], device=DEV)
    assert int((pick < 512).sum()) == 8
    nll16, dh16 = eng.score_grad(tok[pick].contiguous(), y[pick].contiguous(), h[pick].contiguous(), weights=w[pick].contiguous())
    n_t = (y[pick] >= 0).sum(1).double().cpu()
    assert bool(((nll16.cpu().double() - nll[pick].cpu().double()).abs() <= 2e-2 * n_t).all())
    _check_rows("grande dh, row split: first launch half vs 16-row call", dh[pick[:8]], dh16[:8], TOL_DH_GRANDE)
    _check_rows("grande dh, row split: second launch half vs 16-row call", dh[pick[8:]], dh16[8:], TOL_DH_GRANDE)
    # the same batch on packed rows (about 48 000 rows: one launch of the 16-row-slab kernels) against the padded, split run: every row
    rows = (0, int((tok != 0).sum()))
    nll_k, dh_k = eng.score_grad(tok, y, h, weights=w, rows=rows)
    assert int(eng.scal[6:7].view(torch.int32).item()) == 0 and rows[1] <= 65536
    _check_rows("grande dh, 1024 x 82: packed rows vs padded rows", dh_k, dh, TOL_DH_GRANDE)


# ---- 6. descent --------------------------------------------------------------------------------------------------------------------------
def test_gradient_descent_lowers_the_nll_like_the_reference(small, fixture):
    model, tk, smiles, tok, y, _ = small
    eng = model.engine
    traj = torch.from_numpy(fixture["small.traj"]).double()
    ref_drop = traj[:, 0] - traj[:, -1]
    step = float(fixture["step"])
    h = torch.from_numpy(fixture["small.hclip"]).to(DEV)
    n0 = eng.score(tok, y, h_clip=h).clone()
    for _ in range(traj.shape[1] - 1):
        _, dh = eng.score_grad(tok, y, h)
        h = h - step * dh
    n1 = eng.score(tok, y, h_clip=h).clone()
    drop = (n0 - n1).double().cpu()
    log(f"descent: engine drops {drop.tolist()} reference {ref_drop.tolist()}")
    print(f"descent: engine drops {drop.tolist()} reference {ref_drop.tolist()}")
    assert bool((drop >= 0.5 * ref_drop).all()), (drop, ref_drop)


# ---- 7. no side effects ------------------------------------------------------------------------------------------------------------------
def test_score_grad_has_no_side_effects_on_training(small):
    from coati_amd.engine import Engine, ModelConfig
    from coati_amd.synthetic import make_batch
    _, tk, smiles, tok, y, sd = small
    b, up = make_batch(16, 20, 6, 48, seed=3, n_special=12, min_len=4, with_rows=True)
    db = {k: (v if k == "rows" else v.to(DEV)) for k, v in b.items()}
    up = up.to(DEV)
    h = torch.randn(tok.shape[0], 64, generator=torch.Generator().manual_seed(4)).to(DEV)

    def engine(train=True):
        e = Engine(ModelConfig(**SMALL), DEV, train=train)
        e.load_state_dict(sd, strict=False)
        return e

    a, c = engine(), engine()
    a.train_step(db, up, lr=5e-4)
    a.train_step(db, up, lr=5e-4)
    La = a.losses()
    c.train_step(db, up, lr=5e-4)
    before = {k: getattr(c, k).clone() for k in ("params", "grads", "adam_m", "adam_v", "shadow")}
    nll, dh = (t.clone() for t in c.score_grad(tok, y, h))
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(c, k), v), k
    with pytest.raises(RuntimeError):
        c.backward()
    # no weight-gradient launch: the engine's site profiler counts none (and does count the dlogits product)
    for sites, want in (("xf_wgrad,lmhead_wgrad", 0), ("lmhead_dlogits", 1)):
        c.prof_select(sites)
        c.score_grad(tok, y, h)
        _, n, _ = c.prof_collect()
        assert n == want, (sites, n)
    c.prof_select(-1)
    for k, v in before.items():
        assert torch.equal(getattr(c, k), v), k
    c.train_step(db, up, lr=5e-4)
    Lc = c.losses()
    log(f"train/score_grad/train vs train/train: {Lc} vs {La}")
    for k in ("ar_loss", "clip_loss", "grad_norm"):
        assert math.isfinite(Lc[k]) and abs(Lc[k] - La[k]) <= 5e-6 * abs(La[k]), (k, Lc, La)
    # a forward-only engine (no gradient buffer bound) with c's weights at the time of the call: the same bits
    e = Engine(ModelConfig(**SMALL), DEV, train=False)
    assert e.grads is None
    e.params.copy_(before["params"])
    e.refresh_shadows()
    nll_e, dh_e = e.score_grad(tok, y, h)
    assert bool(torch.isfinite(nll_e).all()) and bool(torch.isfinite(dh_e).all()) and float(dh_e.abs().max()) > 0
    assert torch.equal(nll_e, nll) and torch.equal(dh_e, dh)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_coati2_and_fp8_engines_refuse():
    from coati_amd.engine import Engine, ModelConfig
    kw = dict(n_layer_xformer=2, n_hidden_xformer=128, n_hidden_e3nn=128, n_embd_common=128, n_head=8, n_seq=32, n_tok=80)
    tok, y = _flag_rows(80, T=16, B=3)
    tok, y = tok.to(DEV), y.to(DEV)
    h = torch.zeros(3, 128, device=DEV)
    c2 = Engine(ModelConfig(n_layer_e3gnn=0, use_point_encoder=False, enc_to_coati="linear", **kw), DEV, train=False)
    with pytest.raises(RuntimeError, match="COATI2"):
        c2.score_grad(tok, y, h)
    f8 = Engine(ModelConfig(n_layer_e3gnn=1, fp8=True, **kw), DEV, train=False)
    with pytest.raises(RuntimeError, match="fp8"):
        f8.score_grad(tok, y, h)
