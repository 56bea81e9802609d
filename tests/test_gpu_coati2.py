"""COATI2 inference (coati_amd.models.simple_coati2): the SwiGLU kernel against torch, the three smiles_to_coati variants and
coati_to_token against the reference's own outputs (tests/golden/coati2_golden.npz, gen_golden_coati2.py), generation, load_coati2,
the full COATI2 shape, the refusals of the training entries, and COATI1 left untouched."""
import json
import math
import os
import pickle
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.gpu_util import check, log, relerr  # noqa: E402

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VARIANTS = ("linear", "swiglu_mlp", "swiglu_resnet")
MARGIN = 2e-2   # near-tie rule: a step whose recorded top-2 margin (relative to the largest |logit|) is below this may flip on bf16 operands
FULL = dict(n_layer_xformer=12, n_hidden_xformer=512, embed_dim=512, n_head=16, n_seq=250, n_tok=4266)
PAD, STOP, UNK = 31, 40, 44


def _g():
    return np.load(os.path.join(GOLDEN, "coati2_golden.npz"))


def _vocab():
    with open(os.path.join(GOLDEN, "coati2_vocab.json")) as f:
        return json.load(f)


def _tokenizer(vocab=None):
    from coati_amd.models.simple_coati2.trie_tokenizer import TrieTokenizer
    v = vocab or _vocab()
    return TrieTokenizer(n_seq=_vocab()["n_seq"], special_tokens=v["special_tokens"], smiles_tokens=v["smiles_tokens"])


def _state(g, variant):
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}
    sd.update({k[len(variant) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(variant + ".w.")})
    return sd


def _small(variant, g=None):
    from coati_amd.models.simple_coati2.transformer_only import COATI_Smiles_Inference
    g = g if g is not None else _g()
    m = COATI_Smiles_Inference(n_layer_xformer=2, n_hidden_xformer=64, embed_dim=64, n_head=4, n_seq=int(g["n_seq"]), enc_to_coati=variant,
                               n_tok=_vocab()["ids"]["n_token"], device=DEV)
    missing, unexpected = m.load_state_dict(_state(g, variant), strict=False)
    assert not unexpected and all(k.endswith(".attn.bias") for k in missing), (missing, unexpected)
    return m


# ---- 1. the SwiGLU kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(1, 64), (7, 256), (1024, 512), (2048, 512)])
def test_swiglu_matches_torch(B, N):
    from coati_amd import _lib, ops
    gen = torch.Generator(device=DEV).manual_seed(B + N)
    for pad_u, pad_g in ((0, 0), (8, 4), (12, 3)):          # (12, 3): strides that are not multiples of 4 -> the scalar path
        u = torch.randn(B, 2 * N + pad_u, device=DEV, generator=gen) * 4
        ref = torch.nn.functional.silu(u[:, N:2 * N]) * u[:, :N]
        out = torch.full((B, N + pad_g), 7.0, device=DEV)
        _lib.call("coati_swiglu", ops.ptr(u), u.stride(0), ops.ptr(out), out.stride(0), B, N, ops.stream())
        e = relerr(out[:, :N], ref)
        log(f"swiglu B={B} N={N} ldu={u.stride(0)} ldg={out.stride(0)}: relerr {e:.2e}")
        assert e <= 1e-6, e
        assert bool((out[:, N:] == 7.0).all()), "wrote beyond N columns"
    assert torch.equal(ops.swiglu(u[:, :2 * N]), out[:, :N])


# ---- 2. heads and encode against the reference ------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_encode_and_token_head_match_reference(variant):
    g = _g()
    m = _small(variant, g)
    tok = _tokenizer()
    h = m.encode_tokens(torch.from_numpy(g["tokens"]), tok)
    check(f"coati2 {variant} encode_tokens", h, torch.from_numpy(g[f"{variant}.encode"]).to(DEV), 6.5e-3)
    t = m.engine.token_head(torch.from_numpy(g["token_head.in"]).to(DEV))
    check(f"coati2 {variant} coati_to_token", t, torch.from_numpy(g[f"{variant}.token_head"]).to(DEV), 1e-5)
    assert list(m.state_dict().keys()) == g[f"{variant}.keys"].tolist()


def _near_tie_compare(label, got, ref, margin, start):
    """tokens [start, len(ref)) of one row, up to the first step whose recorded margin is a near-tie; returns the count compared"""
    n = 0
    for t in range(start, len(ref)):
        if margin[t - start] < MARGIN:
            break
        assert got[t] == int(ref[t]), (label, t, got, ref.tolist())
        n += 1
    return n


# ---- 3. generation against the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_generation_matches_reference(variant):
    g = _g()
    m = _small(variant, g)
    tok = _tokenizer()
    ref = g[f"{variant}.batch.tokens"]
    h = torch.from_numpy(g[f"{variant}.encode"]).to(DEV)
    _, gen = m.hcoati_to_2d_batch(h, tok, k=2, inv_temp=1e4, return_tokens=True, generator=torch.Generator(device=DEV).manual_seed(0))
    p = 3
    compared = 0
    for b, row in enumerate(gen):
        assert row[:p] == [2, UNK, 39] and len(row) <= ref.shape[1], row
        padded = row + [PAD] * (ref.shape[1] - len(row))     # (every row of this call stopped earlier: what follows is [PAD])
        compared += _near_tie_compare(f"{variant} batch row {b}", padded, ref[b], g[f"{variant}.batch.margin"][b], p)
        assert row.count(STOP) == 1 and all(x == PAD for x in row[row.index(STOP) + 1:]), row
    for r in ref.tolist():      # the fixture's own rows: [PAD] behind a [STOP], or a forced [STOP] at the end
        gen_part = r[p:]
        assert gen_part.count(STOP) == 1 and (gen_part[-1] == STOP or all(x == PAD for x in gen_part[gen_part.index(STOP) + 1:]))
    log(f"coati2 {variant} hcoati_to_2d_batch: {compared} generated tokens compared before the rows' first near-tie")
    # hcoati_to_2d: one [1, E] row and one 1-D vector (payload = the scalar h_token[0])
    seen = []
    inner = m.xformer.generate_topk_with_inj
    object.__setattr__(m.xformer, "generate_topk_with_inj", lambda **kw: seen.append(inner(**kw)) or seen[-1])
    for name in ("row", "vec"):
        seen.clear()
        s = m.hcoati_to_2d(torch.from_numpy(g[f"{variant}.{name}.in"]).to(DEV), tok, k=1)
        got, want, n = seen[0], g[f"{variant}.{name}.tokens"], int(g[f"{variant}.{name}.len"])
        assert got[:p] == [2, UNK, 39] and len(got) <= n
        c = _near_tie_compare(f"{variant} {name}", got + [0] * (n - len(got)), want[:n], g[f"{variant}.{name}.margin"][p:], p)
        log(f"coati2 {variant} hcoati_to_2d {name}: {c} generated tokens compared, string {s!r}")
        assert s == tok.decode(got, special=False)


# ---- 4. load_coati2 -----------------------------------------------------------------------------------------------------
def test_load_coati2_reads_reference_document(tmp_path, monkeypatch):
    from coati_amd.models.simple_coati2.io import load_coati2
    g = _g()
    variant = "swiglu_resnet"
    v = _vocab()
    kwargs = dict(n_layer_xformer=2, n_hidden_xformer=64, embed_dim=64, n_head=4, n_seq=int(g["n_seq"]), mlp_dropout=0.1,
                  enc_to_coati=variant, n_direct_clr=16, n_tok=v["ids"]["n_token"], biases=True, device=torch.device("cpu"), dtype=torch.float)
    model = {"module." + k: t for k, t in _state(g, variant).items()}
    model["module.extra_head.weight"] = torch.zeros(3)
    doc = {"model_kwargs": kwargs, "model": model, "train_args": {"tokenizer_vocab": "coati2_fixture"}, "n_toks_processed": 0}
    path = tmp_path / "coati2.pkl"
    with open(path, "wb") as f:
        pickle.dump(doc, f)
    vdir = tmp_path / "vocabs"
    vdir.mkdir()
    with open(vdir / "coati2_fixture.json", "w") as f:
        json.dump({"special_tokens": v["special_tokens"], "smiles_tokens": v["smiles_tokens"]}, f)
    monkeypatch.setenv("COATI_VOCAB_PATH", str(vdir))
    m, tok = load_coati2(str(path), device=DEV)
    assert all(not p.requires_grad for p in m.parameters())
    for name, want in v["ids"].items():
        assert getattr(tok, name) == want, name
    direct = _small(variant, g)
    tokens = torch.from_numpy(g["tokens"])
    assert torch.equal(m.encode_tokens(tokens, tok), direct.encode_tokens(tokens, tok))


# ---- 5. the full COATI2 shape -----------------------------------------------------------------------------------------------
def _full_tokenizer():
    v = _vocab()
    special = v["special_tokens"] + [f"[X{i}]" for i in range(len(v["special_tokens"]), 330)]
    return _tokenizer({"special_tokens": special, "smiles_tokens": [f"<{i}>" for i in range(330, FULL["n_tok"])]})


def _rows(B, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(60, 100, (B,), generator=g)
    T = int(lens.max())
    t = torch.full((B, T), PAD, dtype=torch.long)
    for b, n in enumerate(lens.tolist()):
        t[b, 0] = 39
        t[b, 1:n - 1] = torch.randint(330, FULL["n_tok"], (n - 2,), generator=g)
        t[b, n - 1] = STOP
    return t


@pytest.mark.parametrize("variant", ["linear", "swiglu_resnet"])
def test_full_shape_deterministic_and_generation_rows(variant):
    from coati_amd.models.simple_coati2.transformer_only import COATI_Smiles_Inference
    torch.manual_seed(11)
    m = COATI_Smiles_Inference(**FULL, enc_to_coati=variant, device=DEV)
    tok = _full_tokenizer()
    for B in (1024, 100):    # B = 100: the sgemm grids have fewer than 128 tiles
        t = _rows(B, B)
        a = m.encode_tokens(t, tok).clone()
        b = m.encode_tokens(t, tok)
        assert a.shape == (B, 512) and bool(torch.isfinite(a).all()), variant
        assert torch.equal(a, b), (variant, B)
        ta, tb = m.engine.token_head(a).clone(), m.engine.token_head(a)
        assert torch.equal(ta, tb) and bool(torch.isfinite(ta).all())
    h = m.encode_tokens(_rows(1024, 5), tok)
    _, gen = m.hcoati_to_2d_batch(h, tok, k=100, return_tokens=True, generator=torch.Generator(device=DEV).manual_seed(2))
    assert len(gen) == 1024
    for row in gen:
        assert row[:3] == [2, UNK, 39] and row.count(STOP) == 1, row
        assert all(x == PAD for x in row[row.index(STOP) + 1:]), row
    log(f"coati2 full shape {variant}: encode deterministic at B = 1024 / 100; {sum(r[-1] == STOP for r in gen)}/1024 rows forced to [STOP]")


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_coati2_refuses_training_and_foreign_tokenizers():
    from coati_amd import _lib, ops
    from coati_amd.engine import Engine, ModelConfig
    from coati_amd.models.simple_coati2.transformer_only import COATI_Smiles_Inference
    m = _small("swiglu_mlp")
    eng = m.engine
    B, T = 2, 4
    tokens = torch.full((B, T), PAD, dtype=torch.long, device=DEV)
    tokens[:, 0], tokens[:, 1] = 39, STOP
    with pytest.raises(RuntimeError, match="inference-only"):
        eng.forward(tokens, tokens, torch.ones(B, 1, dtype=torch.long, device=DEV), torch.zeros(B, 1, 3, device=DEV),
                    torch.zeros(B, dtype=torch.uint8, device=DEV), train=False)
    with pytest.raises(RuntimeError, match="inference-only"):
        eng.backward(None, None)
    with pytest.raises(RuntimeError, match="inference-only"):
        eng.optimizer_step(1e-3)
    with pytest.raises(RuntimeError, match="inference-only"):
        eng.score(tokens, tokens.clone(), h_clip=torch.zeros(B, 64, device=DEV))
    with pytest.raises(RuntimeError, match="inference-only"):
        out = torch.empty(B * T, 80, device=DEV)
        _lib.check(eng.l.coati_engine_logits(eng.h, ops.ptr(out), 80, ops.stream()), "coati_engine_logits")
    with pytest.raises(RuntimeError, match="inference-only"):
        h = torch.zeros(B, 64, device=DEV)
        eng.infonce(h, h, h, h, torch.zeros(B, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="point encoder"):
        eng.encode(atoms=torch.ones(B, 1, dtype=torch.long, device=DEV), coords=torch.zeros(B, 1, 3, device=DEV))
    with pytest.raises(RuntimeError, match="fp8"):
        Engine(ModelConfig(n_layer_xformer=2, n_layer_e3gnn=0, n_hidden_xformer=128, n_hidden_e3nn=128, n_embd_common=128, n_head=8,
                           n_seq=32, n_tok=80, use_point_encoder=False, fp8=True, enc_to_coati="linear"), DEV, train=False)
    with pytest.raises(RuntimeError, match="embed_dim"):
        COATI_Smiles_Inference(n_layer_xformer=2, n_hidden_xformer=64, embed_dim=128, n_head=4, n_seq=32, n_tok=80, device=DEV)
    with pytest.raises(ValueError):
        COATI_Smiles_Inference(n_layer_xformer=2, n_hidden_xformer=64, embed_dim=64, n_head=4, n_seq=32, n_tok=80, enc_to_coati="mlp",
                               device=DEV)
    with pytest.raises(NotImplementedError):
        COATI_Smiles_Inference(n_layer_xformer=2, n_hidden_xformer=64, embed_dim=64, n_head=4, n_seq=32, n_tok=80, device="cpu")
    # tokenizers whose stop / unk / pad ids differ from the model's
    v = _vocab()
    sp = list(v["special_tokens"])
    for a, b in (("[STOP]", "[SET]"), ("[UNK]", "[VALID]" if "[VALID]" in sp else "[TRUE]"), ("[PAD]", "[PREFIX]")):
        s2 = list(sp)
        i, j = s2.index(a), s2.index(b)
        s2[i], s2[j] = s2[j], s2[i]
        other = _tokenizer({"special_tokens": s2, "smiles_tokens": v["smiles_tokens"]})
        with pytest.raises(NotImplementedError):
            m.encode_tokens(torch.from_numpy(_g()["tokens"]), other)
        with pytest.raises(NotImplementedError):
            m.hcoati_to_2d_batch(torch.zeros(2, 64, device=DEV), other, k=2)
    with pytest.raises(RuntimeError, match="not a COATI2 engine"):
        from coati_amd.models.encoding.clip_e2e import e3gnn_smiles_clip_e2e
        c1 = e3gnn_smiles_clip_e2e(n_layer_e3gnn=2, n_layer_xformer=2, n_hidden_xformer=64, n_hidden_e3nn=64, n_embd_common=64, n_head=4,
                                   n_seq=24, n_tok=48, device=torch.device(DEV))
        c1.engine.token_head(torch.zeros(2, 64, device=DEV))


# ---- 7. COATI1 untouched --------------------------------------------------------------------------------------------------------------
def test_coati1_untouched_by_coati2():
    """In one process: a COATI1 model's encode_tokens (bit for bit) and one training step (to the 5e-6 of the step's own float atomics,
    as in the other A/B step tests) are the same before and after a COATI2 model has been built and used."""
    from coati_amd.models.encoding.clip_e2e import e3gnn_smiles_clip_e2e
    from coati_amd.synthetic import make_batch
    small = dict(n_layer_e3gnn=2, n_layer_xformer=2, n_hidden_xformer=64, n_hidden_e3nn=64, n_embd_common=64, n_head=4, n_seq=24, n_tok=48)
    b, up = make_batch(16, 20, 6, 48, seed=3, n_special=12, min_len=4, with_rows=True)
    db = {k: (v if k == "rows" else v.to(DEV)) for k, v in b.items()}
    up = up.to(DEV)

    def run():
        m = e3gnn_smiles_clip_e2e(**small, device=torch.device(DEV))
        m.reset_parameters(seed=5)
        h = m.encode_tokens(db["raw_tokens"], None).clone()
        m.engine.train_step(db, up, lr=5e-4)
        return h, m.engine.losses(), m.engine.params.clone()

    h0, L0, p0 = run()
    c2 = _small("swiglu_resnet")
    g = _g()
    c2.encode_tokens(torch.from_numpy(g["tokens"]), _tokenizer())
    c2.hcoati_to_2d_batch(torch.from_numpy(g["swiglu_resnet.encode"]).to(DEV), _tokenizer(), k=2)
    h1, L1, p1 = run()
    assert torch.equal(h0, h1)
    for k in ("ar_loss", "clip_loss", "grad_norm"):
        assert math.isfinite(L1[k]) and abs(L1[k] - L0[k]) <= 5e-6 * abs(L0[k]), (k, L0, L1)
    log(f"coati1 before / after coati2: encode identical, step params max diff {float((p1 - p0).abs().max()):.2e}")
