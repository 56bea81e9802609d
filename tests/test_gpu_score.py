"""Likelihood scoring on the engine (coati_engine_score, ce_seq_kernel): e3gnn_smiles_clip_e2e.hclip_and_tokens_to_likelihood and
batch_smiles_to_s2s_likelihood against the reference (tests/golden/likelihood_golden.npz), the per-sequence sums against the
training forward's own cross-entropy, the grande shape (incl. the row-split lm_head), layouts, determinism and the absence of side
effects on training."""
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

DEV = "cuda:0"
SMALL = dict(n_layer_e3gnn=2, n_layer_xformer=2, n_hidden_xformer=64, n_hidden_e3nn=64, n_embd_common=64, n_head=4,
             n_seq=24, n_tok=48)
GRANDE = dict(n_layer_e3gnn=5, n_layer_xformer=16, n_hidden_xformer=256, n_hidden_e3nn=256, n_embd_common=256, n_head=16,
              n_seq=250, n_tok=10322)
# Per-token bound of the bf16 path against the fp32 reference: the forward logits are held to 7e-3 of the logit scale
# (test_gpu_decode.py, 3.5e-3 measured) and a token's cross-entropy is lse - logit[target], two such values; the small model's logits
# are O(1), so a token's NLL may move by ~1e-2.  A sequence's bound is this per-token figure times its number of targets.
TOKEN_TOL = 2e-2


def _quiet():
    return contextlib.redirect_stdout(io.StringIO())


@pytest.fixture(scope="module")
def small(golden_dir):
    from coati_amd.models.encoding.clip_e2e import e3gnn_smiles_clip_e2e
    from coati_amd.models.encoding.tokenizers import TrieTokenizer
    g = np.load(os.path.join(golden_dir, "likelihood_golden.npz"))
    voc = json.load(open(os.path.join(golden_dir, "tokenizer.json")))
    tk = TrieTokenizer(n_seq=int(g["n_seq"]), smiles_tokens=voc["smiles"], special_tokens=voc["special"])
    with _quiet():
        model = e3gnn_smiles_clip_e2e(**SMALL, device=torch.device(DEV))
    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "small_model_after3.npz")).items()}
    model.load_state_dict(sd, strict=False)
    return model, tk, g, sd


def _within_token_bound(name, got, ref, n_targets):
    err = (got.double().cpu() - ref.double()).abs()
    per_token = float((err / n_targets.double().clamp(min=1)).max())
    log(f"{name:60s} worst |dNLL| {float(err.max()):.3e}, per target {per_token:.3e}  tol/target {TOKEN_TOL:.0e}")
    assert bool(torch.isfinite(got).all())
    assert bool((err <= TOKEN_TOL * n_targets.double()).all()), (got, ref)


def test_s2s_likelihood_matches_reference(small):
    model, tk, g, _ = small
    with _quiet():
        nll, mask = model.batch_smiles_to_s2s_likelihood(g["smiles"].tolist(), tk)
    assert mask.device.type == "cuda" and mask.dtype == torch.bool
    assert mask.cpu().tolist() == g["s2s.mask"].tolist()
    ref = torch.from_numpy(g["s2s.nll"])
    assert nll.shape == ref.shape
    n_t = torch.from_numpy((g["s2s.targets"].reshape(ref.shape[0], -1) >= 0).sum(1))
    _within_token_bound("s2s likelihood vs reference", nll, ref, n_t)


def test_hclip_likelihood_matches_reference(small):
    model, tk, g, _ = small
    hclip = torch.from_numpy(g["hclip_in"]).to(DEV)
    smiles = g["hclip_smiles"].tolist()
    ref = torch.from_numpy(np.concatenate([g[f"hclip.{i}.nll"] for i in range(len(smiles))]))
    n_t = torch.tensor([int((g[f"hclip.{i}.targets"] >= 0).sum()) for i in range(len(smiles))])
    nll = model.hclip_and_tokens_to_likelihood(hclip, smiles, tk)            # [B, E] + list: one engine call
    assert nll.shape == (len(smiles),)
    _within_token_bound("hclip likelihood (batch form) vs reference", nll, ref, n_t)
    one = model.hclip_and_tokens_to_likelihood(hclip[3], smiles[3], tk)       # the reference's form: [E] + str -> [1]
    assert one.shape == (1,)
    _within_token_bound("hclip likelihood (single form) vs reference", one, ref[3:4], n_t[3:4])


def test_score_equals_the_forward_cross_entropy(small):
    """Arithmetic pin on the padded layout: score(raw_tokens) per row against torch's cross-entropy on Engine.logits() of the
    eval forward with use_point = 0 (the injection is then the SMILES embedding's special token), and the sum against the forward's
    own AR sum.  Same kernels up to the lm_head, whose partials and logits come from different GEMM epilogues (fp32 sums in another
    order): 1e-4 per row; the sums differ by summation order only: 1e-5."""
    from coati_amd.engine import SCAL_AR_SUM
    from coati_amd.models.encoding.clip_e2e import s2s_likelihood_tokens
    model, tk, g, _ = small
    eng = model.engine
    with _quiet():
        raw, tok, y, _ = s2s_likelihood_tokens(g["smiles"].tolist(), tk)
    raw, tok, y = raw.to(DEV), tok.to(DEV), y.to(DEV)
    nll = eng.score(tok, y, raw_tokens=raw).cpu().double()
    B = raw.shape[0]
    atoms = torch.full((B, 2), 6, dtype=torch.long, device=DEV)
    coords = torch.tensor([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0]], device=DEV).expand(B, 2, 3).contiguous()
    eng.forward(raw, tok, atoms, coords, torch.zeros(B, dtype=torch.uint8, device=DEV), y_next=y, train=False)
    ar_sum = float(eng.scal[SCAL_AR_SUM])
    lg = eng.logits().double()
    ce = torch.nn.functional.cross_entropy(lg.reshape(-1, lg.shape[-1]), y.reshape(-1), ignore_index=-1, reduction="none")
    ref = ce.reshape(B, -1).sum(1).cpu()
    rel = float(((nll - ref).abs() / ref.abs()).max())
    srel = abs(float(nll.sum()) - ar_sum) / abs(ar_sum)
    log(f"score vs forward logits + torch CE: worst row rel {rel:.3e}; sum vs forward AR sum rel {srel:.3e}")
    assert rel <= 1e-4 and srel <= 1e-5


@pytest.fixture(scope="module")
def grande():
    from coati_amd.engine import Engine, ModelConfig
    eng = Engine(ModelConfig(**GRANDE), DEV, train=False)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, (off, shape) in eng.layout.items():
            v = eng.view(name)
            if len(shape) == 2:
                v.copy_((torch.randn(shape, generator=g) * (0.02 if "tok_emb" not in name else 1.0)).to(DEV))
            elif name.endswith("weight"):
                v.fill_(1.0)
    eng.refresh_shadows()
    return eng


def _grande_batch(B, seed):
    from coati_amd.synthetic import make_batch
    b, up = make_batch(B, 82, 6, GRANDE["n_tok"], seed=seed, min_len=12, with_rows=True)
    return {k: (v if k == "rows" else v.to(DEV)) for k, v in b.items()}


@pytest.mark.parametrize("B", [1024, 2048])
def test_grande_packed_sum_equals_eval_forward(grande, B):
    """grande shape, synthetic rows of realistic lengths, packed: sum of the per-sequence NLLs == the eval forward's AR sum (use_point = 0,
    same rows; summation order only).  B = 2048 has more than 65 536 decoder rows: the lm_head runs as row-split launches."""
    from coati_amd.engine import SCAL_AR_SUM
    eng = grande
    b = _grande_batch(B, seed=B)
    assert b["rows"][1] > 65536 or B == 1024
    nll = eng.score(b["tokens"], b["y_next"], raw_tokens=b["raw_tokens"], rows=b["rows"])
    assert int(eng.scal[6:7].view(torch.int32).item()) == 0
    nll = nll.cpu().double()
    eng.forward(b["raw_tokens"], b["tokens"], b["atoms"], b["coords"], torch.zeros(B, dtype=torch.uint8, device=DEV), y_next=b["y_next"],
                train=False, rows=b["rows"])
    ar_sum = float(eng.scal[SCAL_AR_SUM])
    srel = abs(float(nll.sum()) - ar_sum) / abs(ar_sum)
    log(f"grande B={B} rows {b['rows'].tolist()}: sum nll {float(nll.sum()):.6e} vs forward AR sum {ar_sum:.6e}, rel {srel:.3e}")
    assert bool(torch.isfinite(nll).all()) and srel <= 1e-5


def test_grande_layouts_and_determinism(grande):
    """Packed == padded to bf16 rounding (the two layouts run different GEMM / attention kernels); the same call twice is bit-identical
    (one workgroup per sequence, fixed-order sums); a molecule scored alone agrees with the same molecule in the batch."""
    eng = grande
    B = 1024
    b = _grande_batch(B, seed=11)
    n_t = (b["y_next"] >= 0).sum(1).cpu()
    packed = eng.score(b["tokens"], b["y_next"], raw_tokens=b["raw_tokens"], rows=b["rows"]).clone()
    again = eng.score(b["tokens"], b["y_next"], raw_tokens=b["raw_tokens"], rows=b["rows"]).clone()
    padded = eng.score(b["tokens"], b["y_next"], raw_tokens=b["raw_tokens"]).clone()
    padded2 = eng.score(b["tokens"], b["y_next"], raw_tokens=b["raw_tokens"]).clone()
    assert torch.equal(packed, again) and torch.equal(padded, padded2)
    mean_rel = abs(float(packed.double().sum() - padded.double().sum())) / abs(float(padded.double().sum()))
    log(f"grande packed vs padded: mean rel {mean_rel:.3e}")
    _within_token_bound("grande packed vs padded (per sequence)", packed, padded.cpu(), n_t)
    assert mean_rel <= 5e-4
    for i in (1, 517):
        L = int((b["tokens"][i] != 0).sum()) + 1
        alone = eng.score(b["tokens"][i:i + 1, :L].contiguous(), b["y_next"][i:i + 1, :L].contiguous(),
                          raw_tokens=b["raw_tokens"][i:i + 1].contiguous())
        _within_token_bound(f"grande molecule {i} alone vs in the batch", alone, packed[i:i + 1].cpu(), n_t[i:i + 1])


def test_score_has_no_side_effects_on_training(small):
    """train_step, score, train_step == two train_steps (the step's own float atomics make two runs equal to rounding only: 5e-6, the
    bound of the other A/B step tests); score leaves every flat buffer bit-identical; backward() right after score is refused; an
    engine made with train=False gives the same scores bit for bit."""
    from coati_amd.engine import Engine, ModelConfig
    from coati_amd.synthetic import make_batch
    _, tk, g, sd = small
    b, up = make_batch(16, 20, 6, 48, seed=3, n_special=12, min_len=4, with_rows=True)
    db = {k: (v if k == "rows" else v.to(DEV)) for k, v in b.items()}
    up = up.to(DEV)

    def engine(train=True):
        e = Engine(ModelConfig(**SMALL), DEV, train=train)
        e.load_state_dict(sd, strict=False)
        return e

    def score(e):
        return e.score(db["tokens"], db["y_next"], raw_tokens=db["raw_tokens"], rows=db["rows"]).clone()

    a, c = engine(), engine()
    a.train_step(db, up, lr=5e-4)
    a.train_step(db, up, lr=5e-4)
    La = a.losses()
    c.train_step(db, up, lr=5e-4)
    before = {k: getattr(c, k).clone() for k in ("params", "grads", "adam_m", "adam_v", "shadow")}
    s1 = score(c)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(c, k), v), k
    with pytest.raises(RuntimeError):
        c.backward()
    c.train_step(db, up, lr=5e-4)
    Lc = c.losses()
    log(f"train/score/train vs train/train: {Lc} vs {La}")
    for k in ("ar_loss", "clip_loss", "grad_norm"):
        assert math.isfinite(Lc[k]) and abs(Lc[k] - La[k]) <= 5e-6 * abs(La[k]), (k, Lc, La)
    # train=False engine, same weights as c at the time of s1
    e = Engine(ModelConfig(**SMALL), DEV, train=False)
    e.params.copy_(before["params"])
    e.refresh_shadows()
    assert torch.equal(score(e), s1)
