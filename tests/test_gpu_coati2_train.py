"""The COATI2 training step on the engine (coati_engine_forward / _backward / _optimizer_step on a COATI2 engine bound with gradient and
Adam buffers) against the step built from the reference's modules under autograd (tests/golden/coati2_train_golden*.npz,
gen_golden_coati2_train.py): forward, AR loss, every parameter gradient with and without an external dh_coati, clip-norm, AdamW, a 20-step
curve, padded vs packed rows, the staged backward, the split forward, edge shapes, the full COATI2 shape, the absence of side effects of
score_grad_coati2, the refusals and finetune_coati2.

Tolerances are relative to tensor scale against the fp32 fixture; each constant is at most 2x the worst value measured on the MI355X (the
project's rule, tests/test_gpu_engine.py) and none exceeds COATI1's for the same-sized model (TOL_FWD 6.5e-3, TOL_GRAD 3.8e-2, TOL_LOSS 1e-3,
TOL_CURVE 2.5e-3).  measured -> bound:
    small model, three variants, one row alone and the failure-row batch, padded = packed rows
      h_coati 2.38e-3, logits 4.28e-3 (swiglu_mlp)                 -> TOL_FWD 6.5e-3 (COATI1's: 2x would be 8.6e-3)
      AR loss 1.47e-4 (failure-row batch; 5.8e-5 on the 16 rows)    -> TOL_LOSS 2.9e-4
      parameter gradients 9.44e-3 (h.0.ln_1.weight, swiglu_mlp)     -> TOL_GRAD 1.88e-2
      clip_grad_norm_ value 2.94e-4 (failure-row batch)             -> TOL_GRADNORM 5.8e-4
      per-parameter gradient norm 3.52e-3 (one row alone)           -> TOL_PARAM_NORM 7.0e-3
      20-step curve, per step 2.83e-4 (linear, step 15)             -> TOL_CURVE 5.6e-4
      displacement cosine after 1 / 3 steps 0.915 / 0.948           -> > 0.9 (tests/test_gpu_engine.py's bound; see the test)
    full shape (12 layers, d = 512), padded = packed rows
      h_coati 3.06e-3 -> TOL_FULL_FWD 6.1e-3; AR loss 3.0e-6 -> TOL_FULL_LOSS 6e-6; sampled gradient elements 1.43e-2 (h.11.attn.c_proj.weight)
      -> TOL_FULL_GRAD 2.85e-2; per-parameter norm 1.93e-3 -> TOL_FULL_PARAM_NORM 3.8e-3; clip_grad_norm_ value 9.81e-4 -> TOL_FULL_GRADNORM 1.96e-3
    two layouts / stagings of one step: gradients 3.6e-7, loss sums 3.0e-7 -> TOL_SAME 1e-5 (the bound of tests/test_gpu_engine.py where only the
    order of float atomics differs)
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.coati2_full_weights import FULL, checksums, full_weights  # noqa: E402
from tests.gpu_util import check, log, relerr  # noqa: E402

DEV = "cuda:0"
VARIANTS = ("linear", "swiglu_mlp", "swiglu_resnet")
PAD, STOP, UNK = 31, 40, 44
TOL_FWD = 6.5e-3
TOL_GRAD = 1.88e-2
TOL_LOSS = 2.9e-4
TOL_GRADNORM = 5.8e-4
TOL_PARAM_NORM = 7.0e-3
TOL_CURVE = 5.6e-4
TOL_FULL_FWD = 6.1e-3
TOL_FULL_LOSS = 6e-6
TOL_FULL_GRAD = 2.85e-2
TOL_FULL_PARAM_NORM = 3.8e-3
TOL_FULL_GRADNORM = 1.96e-3
TOL_SAME = 1e-5           # two layouts / stagings of the same step: only the order of the embedding table's atomics differs (tests/test_gpu_engine.py)
assert TOL_FWD <= 6.5e-3 and TOL_GRAD <= 3.8e-2 and TOL_LOSS <= 1e-3 and TOL_CURVE <= 2.5e-3   # COATI1's, same-sized model


def _quiet():
    return contextlib.redirect_stdout(io.StringIO())


def _report(msg):
    log(msg)
    print(msg)


@pytest.fixture(scope="module")
def golden(golden_dir):
    files = {"": "coati2_train_golden.npz", "steps": "coati2_train_golden_steps.npz"}
    files.update({v: f"coati2_train_golden_{v}.npz" for v in VARIANTS})
    return {k: np.load(os.path.join(golden_dir, f)) for k, f in files.items()}


@pytest.fixture(scope="module")
def tokenizer(golden_dir):
    from coati_amd.models.simple_coati2.trie_tokenizer import TrieTokenizer
    v = json.load(open(os.path.join(golden_dir, "coati2_vocab.json")))
    return TrieTokenizer(n_seq=v["n_seq"], special_tokens=v["special_tokens"], smiles_tokens=v["smiles_tokens"])


def _small_model(golden_dir, tokenizer, variant, trainable=True, **kw):
    from coati_amd.models.simple_coati2.transformer_only import COATI_Smiles_Inference
    g = np.load(os.path.join(golden_dir, "coati2_golden.npz"))
    with _quiet():
        m = COATI_Smiles_Inference(n_layer_xformer=2, n_hidden_xformer=64, embed_dim=64, n_head=4, n_seq=int(g["n_seq"]), enc_to_coati=variant,
                                   n_tok=tokenizer.n_token, device=DEV, trainable=trainable, **kw)
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}
    sd.update({k[len(variant) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(variant + ".w.")})
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(".attn.bias") for k in missing), (missing, unexpected)
    return m, {k: v for k, v in sd.items()}


@pytest.fixture(scope="module")
def small(golden_dir, tokenizer):
    """variant -> (trainable model of coati2_golden.npz, its initial state dict), built on first use"""
    made = {}

    def get(variant):
        if variant not in made:
            made[variant] = _small_model(golden_dir, tokenizer, variant)
        return made[variant]
    return get


def _reset(eng, P0):
    eng.load_state_dict(P0)
    eng.step_count = 0
    eng.adam_m.zero_(); eng.adam_v.zero_()


def _batch(g, tag, packed=False):
    b = {k: torch.from_numpy(g[f"{tag}.{k}"]).to(DEV).contiguous() for k in ("raw_tokens", "tokens", "y_next")}
    if packed:
        from coati_amd.synthetic import packed_rows
        b["rows"] = packed_rows(b["raw_tokens"].cpu(), b["tokens"].cpu(), b["y_next"].cpu(), pad=PAD)
    return b


def _grad_norm(eng):
    from coati_amd import _lib
    from coati_amd.ops import ptr, stream
    part = torch.zeros(1024, device=DEV); out = torch.zeros(2, device=DEV)
    _lib.call("coati_grad_sqnorm", ptr(eng.grads), eng.n_params, ptr(part), 1024, ptr(out[0:1]), 10.0, ptr(out[1:2]), stream())
    return out[0:1].cpu()


def _check_grads(name, eng, ref, prefix, tol):
    grads = eng.named_views("grads")
    worst = sorted(((relerr(grads[k], torch.from_numpy(ref[prefix + k])), k) for k in eng.layout), reverse=True)
    _report(f"{name}: worst parameter gradient {worst[0][0]:.3e} ({worst[0][1]}), tol {tol:.1e}")
    for e, k in worst:
        assert bool(torch.isfinite(grads[k]).all()), k
    assert worst[0][0] <= tol, worst[:6]
    return worst[0][0]


def _check_sampled(name, eng, g, tag, tol_grad, tol_norm):
    """per parameter: the gradient's 2-norm, and every ceil(numel / 1024)-th element of the flat gradient relative to the samples' scale"""
    grads = eng.named_views("grads")
    names = [str(n) for n in g[f"{tag}.names"]]
    assert set(names) == set(eng.layout)
    w_el, w_nm = (0.0, ""), (0.0, "")
    for n, ref_norm in zip(names, g[f"{tag}.gnorm"]):
        flat = grads[n].flatten()
        assert bool(torch.isfinite(flat).all()), n
        ref = torch.from_numpy(g[f"{tag}.gs.{n}"])
        got = flat[::-(-flat.numel() // 1024)].cpu()
        if float(ref.abs().max()) == 0.0:
            assert float(flat.abs().max()) == 0.0, n
            continue
        w_el = max(w_el, (relerr(got, ref), n))
        w_nm = max(w_nm, (abs(float(flat.double().norm()) - float(ref_norm)) / float(ref_norm), n))
    _report(f"{name}: worst sampled gradient elements {w_el[0]:.3e} ({w_el[1]}) tol {tol_grad:.1e}; worst per-parameter norm {w_nm[0]:.3e} ({w_nm[1]}) tol {tol_norm:.1e}")
    assert w_el[0] <= tol_grad and w_nm[0] <= tol_norm, (w_el, w_nm)


# ---- 1. parity with the reference step, small model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_small_step_matches_reference(variant, small, golden):
    m, P0 = small(variant)
    eng = m.engine
    g, gv = golden[""], golden[variant]
    b = _batch(g, "small")
    _reset(eng, P0)
    he, h, bad = eng.forward(b["raw_tokens"], b["tokens"], y_next=b["y_next"], train=True)
    logits = eng.logits()
    assert float(he.abs().max()) == 0.0
    check(f"coati2 train {variant} h_coati", h.cpu(), torch.from_numpy(g[f"{variant}.h"]), TOL_FWD)
    check(f"coati2 train {variant} logits", logits.cpu(), torch.from_numpy(g[f"{variant}.logits"]), TOL_FWD)
    eng.backward(None, None)
    L = eng.losses()
    check(f"coati2 train {variant} ar loss", torch.tensor([L["ar_loss"]]), torch.from_numpy(g[f"{variant}.ar"]).reshape(1).float(), TOL_LOSS)
    assert L["clip_loss"] == 0.0
    _check_grads(f"coati2 train {variant} gradients, dh_ext = 0", eng, gv, "g0.", TOL_GRAD)
    check(f"coati2 train {variant} gradient norm, dh_ext = 0", _grad_norm(eng), torch.from_numpy(g[f"{variant}.gradnorm0"]).reshape(1).float(), TOL_GRADNORM)
    # an external gradient w.r.t. h_coati, through train_step
    eng.train_step(b, None, lr=0.0, do_clip=False, optimizer=False, dh_coati=torch.from_numpy(g["small.dh_ext"]).to(DEV))
    _check_grads(f"coati2 train {variant} gradients, seeded dh_ext", eng, gv, "g1.", TOL_GRAD)
    check(f"coati2 train {variant} gradient norm, seeded dh_ext", _grad_norm(eng), torch.from_numpy(g[f"{variant}.gradnorm1"]).reshape(1).float(), TOL_GRADNORM)
    # eval_step: the same loss, nothing written
    before = eng.grads.clone()
    eng.eval_step(b, None, do_clip=False)
    assert abs(eng.losses()["ar_loss"] - L["ar_loss"]) <= TOL_LOSS * L["ar_loss"] and torch.equal(eng.grads, before)


@pytest.mark.parametrize("variant", VARIANTS)
def test_small_twenty_step_curve(variant, small, golden):
    m, P0 = small(variant)
    eng = m.engine
    g = golden[""]
    b = _batch(g, "small", packed=True)
    lr = float(g[f"{variant}.lr"])
    kw = dict(weight_decay=float(g["weight_decay"]), max_norm=float(g["max_norm"]), betas=tuple(float(x) for x in g["betas"]), eps=float(g["eps"]))
    _reset(eng, P0)
    ref, ref_gn = g[f"{variant}.curve"], g[f"{variant}.curve_gradnorm"]
    losses, norms, after = [], [], {}
    for step in range(len(ref)):
        eng.train_step(b, None, lr, do_clip=False, **kw)
        L = eng.losses()
        losses.append(L["ar_loss"]); norms.append(L["grad_norm"])
        if variant == "swiglu_resnet" and step + 1 in (1, 3):
            after[step + 1] = {k: v.cpu() for k, v in eng.state_dict().items()}
    losses = np.array(losses)
    dev = np.abs(losses - ref) / np.abs(ref)
    dgn = np.abs(np.array(norms) - ref_gn) / np.abs(ref_gn)
    _report(f"coati2 train {variant} 20-step curve, lr {lr}: {losses[0]:.4f} -> {losses[-1]:.4f} (reference {ref[0]:.4f} -> {ref[-1]:.4f}), worst relative "
            f"deviation {dev.max():.3e} (step {int(dev.argmax())}) tol {TOL_CURVE:.1e}; gradient norm {dgn.max():.3e} (median {np.median(dgn):.3e})")
    assert losses[-4:].mean() < 0.85 * losses[:4].mean()          # the engine's own curve descends
    assert dev.max() <= TOL_CURVE
    assert dgn[0] <= TOL_GRADNORM
    # parameters after 1 and 3 steps: Adam's first steps are sign-like (m / sqrt(v) ~ +-1), so an element whose gradient is near zero can
    # flip under bf16 noise: the DISPLACEMENT's direction per tensor, as tests/test_gpu_engine.py compares it (cosine > 0.9)
    for k_step, sd in after.items():
        worst = (2.0, "")
        for k in eng.layout:
            d_hip = (sd[k] - P0[k]).flatten().double()
            d_ref = (torch.from_numpy(golden["steps"][f"after{k_step}.{k}"]) - P0[k]).flatten().double()
            worst = min(worst, (float((d_hip @ d_ref) / (d_hip.norm() * d_ref.norm() + 1e-30)), k))
        _report(f"coati2 train swiglu_resnet parameters after {k_step} step(s): smallest displacement cosine {worst[0]:.4f} ({worst[1]})")
        assert worst[0] > 0.9, worst


def _worst_vs(eng, g_a, g_b):
    """worst per-parameter relative difference of two copies of the flat gradient buffer"""
    out = (0.0, "")
    for k, (off, shape) in eng.layout.items():
        n = int(np.prod(shape))
        out = max(out, (relerr(g_a[off:off + n], g_b[off:off + n]), k))
    return out


# ---- 2. padded layout vs packed rows ---------------------------------------------------------------------------------------------------------
def _step_grads(eng, b, stages=(0,), split=False, dh=None):
    he, h, bad = eng.forward(b["raw_tokens"], b["tokens"], y_next=b["y_next"], train=True, rows=b.get("rows"), stop_after_heads=split)
    if split:
        eng.forward_decoder()
    for st in stages:
        eng.backward(dh if st in (0, 1) else None, None, st)
    torch.cuda.synchronize()
    return h.clone(), eng.scal[:2].clone(), eng.grads.clone()


@pytest.mark.parametrize("variant", VARIANTS)
def test_padded_vs_packed_rows(variant, small, golden):
    m, P0 = small(variant)
    eng = m.engine
    _reset(eng, P0)
    g = golden[""]
    dh = torch.from_numpy(g["small.dh_ext"]).to(DEV)
    h_p, s_p, g_p = _step_grads(eng, _batch(g, "small"), dh=dh)
    h_k, s_k, g_k = _step_grads(eng, _batch(g, "small", packed=True), dh=dh)
    assert int(eng.scal[6:7].view(torch.int32).item()) == 0
    check(f"coati2 train {variant} packed vs padded h_coati", h_k, h_p, TOL_SAME)
    check(f"coati2 train {variant} packed vs padded loss sums", s_k, s_p, TOL_SAME)
    worst = _worst_vs(eng, g_k, g_p)
    _report(f"coati2 train {variant} packed vs padded rows: worst parameter gradient {worst[0]:.3e} ({worst[1]}), tol {TOL_SAME:.1e}")
    assert worst[0] <= TOL_SAME, worst


# ---- 3. staged backward, 4. split forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_staged_backward_and_split_forward(variant, small, golden):
    m, P0 = small(variant)
    eng = m.engine
    _reset(eng, P0)
    g = golden[""]
    b = _batch(g, "small", packed=True)
    dh = torch.from_numpy(g["small.dh_ext"]).to(DEV)
    h0, s0, g0 = _step_grads(eng, b, dh=dh)
    for stages in ((1, 2), (1, 4, 5, 3)):
        _, s1, g1 = _step_grads(eng, b, stages=stages, dh=dh)
        w = _worst_vs(eng, g1, g0)
        _report(f"coati2 train {variant} staged backward {stages} vs stage 0: worst parameter gradient {w[0]:.3e} ({w[1]}), tol {TOL_SAME:.1e}")
        assert relerr(s1, s0) <= TOL_SAME and w[0] <= TOL_SAME, w
    # train | 2 + forward_decoder: the same launches in the same order -- the same bits of what the forward computes without float
    # atomics: h_coati and, on padded rows, the logits.  The loss sum is added up with atomicAdd across workgroups (loss.hip) and the
    # token table's gradient is an atomic scatter: two identical calls differ there in the last bits, so they and the gradients get TOL_SAME
    for bb in (b, _batch(g, "small")):
        h1, s1, g1 = _step_grads(eng, bb, dh=dh)
        lg1 = eng.logits().clone() if "rows" not in bb else None
        h2, s2, g2 = _step_grads(eng, bb, split=True, dh=dh)
        assert torch.equal(h2, h1) and relerr(s2, s1) <= TOL_SAME
        assert lg1 is None or torch.equal(eng.logits(), lg1)
        w = _worst_vs(eng, g2, g1)
        _report(f"coati2 train {variant} train | 2 + forward_decoder vs one call ({'packed' if 'rows' in bb else 'padded'}): h_coati"
                f"{' and logits' if lg1 is not None else ''} bit-equal, worst parameter gradient {w[0]:.3e} ({w[1]}), tol {TOL_SAME:.1e}")
        assert w[0] <= TOL_SAME, w


# ---- 5. edge shapes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,packed", [("one", False), ("one", True), ("fail", False), ("fail", True)])
def test_one_row_and_failure_row(tag, packed, small, golden):
    """B = 1 with a 3-token body; a batch with an all-[PAD] decoder row whose encoder row is a lone [STOP]"""
    m, P0 = small("swiglu_resnet")
    eng = m.engine
    _reset(eng, P0)
    g = golden[""]
    b = _batch(g, tag, packed=packed)
    he, h, bad = eng.train_step(b, None, lr=0.0, do_clip=False, optimizer=False)
    L = eng.losses()
    name = f"coati2 train edge '{tag}' ({'packed' if packed else 'padded'})"
    check(f"{name} h_coati", h.cpu(), torch.from_numpy(g[f"{tag}.h"]), TOL_FWD)
    check(f"{name} ar loss", torch.tensor([L["ar_loss"]]), torch.from_numpy(g[f"{tag}.ar"]).reshape(1).float(), TOL_LOSS)
    _check_sampled(name, eng, g, tag, TOL_GRAD, TOL_PARAM_NORM)
    check(f"{name} gradient norm", _grad_norm(eng), torch.from_numpy(g[f"{tag}.gradnorm"]).reshape(1).float(), TOL_GRADNORM)


# ---- 6. the full COATI2 shape ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full(golden):
    from coati_amd.engine import Engine, ModelConfig
    g = golden[""]
    W = full_weights()
    names = [str(n) for n in g["full.names"]]
    ws, wa = checksums(W, names)
    assert np.allclose(ws, g["full.wsum"], rtol=0, atol=1e-6 * np.abs(g["full.wabs"]).max()) and np.allclose(wa, g["full.wabs"], rtol=1e-9), \
        "full_weights() no longer reproduces the weights of coati2_train_golden.npz"
    cfg = ModelConfig(n_layer_xformer=FULL["n_layer_xformer"], n_layer_e3gnn=0, n_hidden_xformer=FULL["n_hidden_xformer"],
                      n_hidden_e3nn=FULL["n_hidden_xformer"], n_embd_common=FULL["embed_dim"], n_head=FULL["n_head"], n_seq=FULL["n_seq"],
                      n_tok=FULL["n_tok"], pad_token=PAD, stop_token=STOP, unk_token=UNK, use_point_encoder=False, biases=True,
                      enc_to_coati="swiglu_resnet")
    eng = Engine(cfg, DEV, train=True)
    eng.load_state_dict(W)
    return eng


@pytest.mark.parametrize("packed", [False, True])
def test_full_shape_step(packed, full, golden):
    eng = full
    g = golden[""]
    b = _batch(g, "full", packed=packed)
    he, h, bad = eng.train_step(b, None, lr=0.0, do_clip=False, optimizer=False)
    L = eng.losses()
    name = f"coati2 train full shape ({'packed' if packed else 'padded'})"
    check(f"{name} h_coati", h.cpu(), torch.from_numpy(g["full.h"]), TOL_FULL_FWD)
    check(f"{name} ar loss", torch.tensor([L["ar_loss"]]), torch.from_numpy(g["full.ar"]).reshape(1).float(), TOL_FULL_LOSS)
    _check_sampled(name, eng, g, "full", TOL_FULL_GRAD, TOL_FULL_PARAM_NORM)
    check(f"{name} gradient norm", _grad_norm(eng), torch.from_numpy(g["full.gradnorm"]).reshape(1).float(), TOL_FULL_GRADNORM)


# ---- 7. score_grad_coati2 on an engine that trains: no side effects ------------------------------------------------------------------------------
def test_score_grad_leaves_the_training_state_alone(small, golden, golden_dir, tokenizer):
    m, P0 = small("swiglu_resnet")
    eng = m.engine
    _reset(eng, P0)
    g = golden[""]
    b = _batch(g, "small")
    eng.train_step(b, None, lr=float(g["swiglu_resnet.lr"]), do_clip=False)          # grads, Adam state and shadows all non-trivial
    torch.cuda.synchronize()
    before = {k: getattr(eng, k).clone() for k in ("params", "grads", "adam_m", "adam_v", "shadow")}
    h = torch.from_numpy(g["swiglu_resnet.h"]).to(DEV)
    nll, dh = (t.clone() for t in eng.score_grad_coati2(b["tokens"], b["y_next"], h))
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(eng, k), v), k
    assert bool(torch.isfinite(dh).all()) and torch.equal(nll, eng.score_coati2(b["tokens"], b["y_next"], h_coati=h))
    with pytest.raises(RuntimeError, match="no forward"):            # scoring keeps nothing for a backward
        eng.backward(None, None)
    # the forward-only model: the same scoring bits, no gradient buffer, the step refused before any other check
    m0, _ = _small_model(golden_dir, tokenizer, "swiglu_resnet", trainable=False)
    m0.load_state_dict(eng.state_dict(), strict=False)
    assert m0.engine.grads is None and m0.engine.adam_m is None and all(p.grad is None for p in m0.parameters())
    n0, d0 = m0.engine.score_grad_coati2(b["tokens"], b["y_next"], h)
    assert torch.equal(n0, nll) and torch.equal(d0, dh)
    for call in (lambda: m0.engine.forward(b["raw_tokens"], b["tokens"], y_next=b["y_next"], train=False),
                 lambda: m0.engine.backward(None, None), lambda: m0.engine.optimizer_step(1e-3), lambda: m0(b["raw_tokens"], b["tokens"], tokenizer)):
        with pytest.raises(RuntimeError, match="inference-only"):
            call()


# ---- 8. refusals on an engine that trains ---------------------------------------------------------------------------------------------------
def test_refusals_on_a_trainable_engine(small, golden, golden_dir, tokenizer):
    m, P0 = small("swiglu_mlp")
    eng = m.engine
    _reset(eng, P0)
    g = golden[""]
    b = _batch(g, "small")
    he, h, bad = eng.forward(b["raw_tokens"], b["tokens"], y_next=b["y_next"], train=True)
    with pytest.raises(RuntimeError, match="dh_e3gnn"):
        eng.backward(None, torch.zeros_like(h))
    with pytest.raises(RuntimeError, match="inference-only"):
        eng.infonce(h, h, h, h, torch.zeros(h.shape[0], dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="do_clip"):
        eng.train_step(b, None, lr=1e-3, do_clip=True)
    with pytest.raises(ValueError, match="do_clip"):
        eng.eval_step(b, None)
    with pytest.raises(NotImplementedError, match="dropout"):
        _small_model(golden_dir, tokenizer, "swiglu_mlp", trainable=True, mlp_dropout=0.1)
    # the model's forward: h_coati and logits of the evaluation forward; parameters carry their gradient slices
    hm, lg = m(b["raw_tokens"], b["tokens"], tokenizer)
    check("coati2 train swiglu_mlp model.forward h_coati", hm.cpu(), torch.from_numpy(g["swiglu_mlp.h"]), TOL_FWD)
    check("coati2 train swiglu_mlp model.forward logits", lg.cpu(), torch.from_numpy(g["swiglu_mlp.logits"]), TOL_FWD)
    eng.train_step(b, None, lr=0.0, do_clip=False, optimizer=False)
    for n, p in m.named_parameters():
        assert p.grad is not None and p.grad.data_ptr() == eng.view(n, "grads").data_ptr(), n
    assert all(float(p.grad.abs().max()) > 0 for n, p in m.named_parameters() if n.startswith(("coati_to_token.", "smiles_to_coati.")))


# ---- 9. finetune_coati2 -----------------------------------------------------------------------------------------------------------------------
def test_finetune_lowers_the_round_trip_nll(small, golden_dir, tokenizer):
    import random
    from coati_amd.training import finetune_coati2
    m, P0 = small("swiglu_resnet")
    _reset(m.engine, P0)
    smiles = [str(s) for s in np.load(os.path.join(golden_dir, "coati2_likelihood_golden.npz"))["smiles"]]
    with _quiet():
        nll0, mask = m.batch_smiles_to_s2s_likelihood(smiles, tokenizer)
        losses = finetune_coati2(m, tokenizer, smiles, n_steps=20, batch_size=8, lr=1e-3, rng=random.Random(3))
        nll1, _ = m.batch_smiles_to_s2s_likelihood(smiles, tokenizer)
    _report(f"coati2 finetune: 20 steps at lr 1e-3 on 8 SMILES: step loss {losses[0]:.4f} -> {losses[-1]:.4f}, mean round-trip NLL {float(nll0.mean()):.3f} -> {float(nll1.mean()):.3f}")
    assert bool(mask.all()) and len(losses) == 20 and all(np.isfinite(losses))
    assert float(nll1.mean()) < float(nll0.mean())
    _reset(m.engine, P0)
