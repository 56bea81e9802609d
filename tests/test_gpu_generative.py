"""coati.generative on the engine: the packed-row encode (coati_engine_encode_packed) against the padded one, the decoder logits
(coati_engine_decoder_logits) against the reference and against coati_engine_score, coati_group_mean_rows against float64, the batched
purification / forced decoding against their per-vector forms, the reference's outputs (tests/golden/generative_golden.npz), the
density fit, an unscripted grande run and the absence of side effects on training."""
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
EMBED_TOL = 6.5e-3      # encode_tokens against the reference (test_gpu_api.py)
LOGIT_TOL = 7e-3        # forward logits against the reference, of the logit scale (test_gpu_decode.py)


def _quiet():
    return contextlib.redirect_stdout(io.StringIO())


def _canon(s):
    if not s or "X" in s:
        return None
    return min(s, s[::-1])


@pytest.fixture(scope="module")
def small(golden_dir):
    from coati_amd.models.encoding.clip_e2e import e3gnn_smiles_clip_e2e
    from coati_amd.models.encoding.tokenizers import TrieTokenizer
    g = np.load(os.path.join(golden_dir, "generative_golden.npz"))
    voc = json.load(open(os.path.join(golden_dir, "tokenizer.json")))
    tk = TrieTokenizer(n_seq=int(g["n_seq"]), smiles_tokens=voc["smiles"], special_tokens=voc["special"])
    with _quiet():
        model = e3gnn_smiles_clip_e2e(**SMALL, device=torch.device(DEV))
    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "small_model_after3.npz")).items()}
    model.load_state_dict(sd, strict=False)
    return model, tk, g, sd


def _close(name, got, ref, tol, scale=None):
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    err = float((got - ref).abs().max())
    s = float(ref.abs().max()) if scale is None else scale
    log(f"{name:58s} max |d| {err:.3e}  scale {s:.3e}  tol {tol:.1e}")
    assert bool(torch.isfinite(got).all())
    assert err <= tol * max(s, 1.0), (name, err)


def _rand_rows(B, lo, hi, n_tok, stop, pad, first, avoid, seed):
    """[B, T] int64 rows: first, random ids of [12, n_tok) outside avoid, [STOP]; lengths lo..hi tokens (incl. first / [STOP])"""
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(lo, hi + 1, (B,), generator=g)
    T = int(n.max())
    ids = torch.randint(12, n_tok, (B, T), generator=g)
    for a in avoid:
        ids[ids == a] = 12
    ids[:, 0] = first
    cols = torch.arange(T).unsqueeze(0)
    ids[cols == (n - 1).unsqueeze(1)] = stop
    ids[cols >= n.unsqueeze(1)] = pad
    return ids, int(n.sum())


def _packed_vs_padded(label, eng, tok, rows1):
    t = tok.to(DEV)
    h_pad, _ = eng.encode(raw_tokens=t)
    h_pk, _ = eng.encode(t, rows=rows1)
    assert int(eng.scal[6:7].view(torch.int32).item()) == 0
    h_pk2, _ = eng.encode(t, rows=rows1)
    assert torch.equal(h_pk, h_pk2), "packed encode is not bit-identical on repeat"
    _close(f"{label}: packed vs padded encode", h_pk, h_pad, EMBED_TOL)
    eng.encode(t, rows=rows1 - 1)
    assert int(eng.scal[6:7].view(torch.int32).item()) & 2, "a wrong rows1 must set bit 1"
    return h_pk


def test_encode_packed_small_and_golden(small):
    from coati.generative import coati_purifications as P
    model, tk, g, _ = small
    rows = [tk.tokenize_text("[SMILES]" + s + "[STOP]", pad=True) for s in g["batch_in"].tolist()]
    tok = torch.tensor(rows, dtype=torch.long)
    n = int((tok != 0).sum())
    _packed_vs_padded("small", model.engine, tok, n)
    with _quiet():
        got = P.embed_smiles_batch(g["batch_in"].tolist(), model, tk)
        one = torch.stack([P.embed_smiles(s, model, tk, canon_smiles=_canon) for s in g["embed_smiles_in"].tolist()])
    _close("embed_smiles_batch vs reference", got, g["embed_smiles_batch"], EMBED_TOL)
    _close("embed_smiles vs reference", one, g["embed_smiles"], EMBED_TOL)
    # a row without [STOP] sets bit 0
    bad = tok.clone()
    bad[bad == tk.stop_token] = tk.vocab["C"]
    model.engine.encode(bad.to(DEV), rows=int((bad != 0).sum()))
    assert int(model.engine.scal[6:7].view(torch.int32).item()) & 1


@pytest.mark.parametrize("variant", [None, "linear", "swiglu_mlp", "swiglu_resnet"])
def test_encode_packed_grande(variant):
    """B = 1024 rows of 38-76 tokens in a 250-column layout: packed == padded to bf16 rounding, COATI1 and the three COATI2 heads"""
    if variant is None:
        from coati_amd.models.encoding.clip_e2e import e3gnn_smiles_clip_e2e
        with _quiet():
            model = e3gnn_smiles_clip_e2e(**GRANDE, device=torch.device(DEV))
        stop, pad, first, avoid = 1, 0, 2, ()
    else:
        from coati_amd.models.simple_coati2.transformer_only import COATI_Smiles_Inference
        with _quiet():
            model = COATI_Smiles_Inference(n_layer_xformer=16, n_hidden_xformer=256, embed_dim=256, n_head=16, n_seq=250, enc_to_coati=variant,
                                           n_tok=GRANDE["n_tok"], device=torch.device(DEV))
        stop, pad, first, avoid = 40, 31, 35, (31, 40, 44)
    tok, n = _rand_rows(1024, 38, 76, GRANDE["n_tok"], stop, pad, first, avoid, seed=5)
    full = torch.full((1024, 250), pad, dtype=torch.long)
    full[:, :tok.shape[1]] = tok
    _packed_vs_padded(f"grande {variant or 'coati1'}", model.engine, full, n)
    del model
    torch.cuda.empty_cache()


def test_decoder_logits_match_reference(small):
    model, tk, g, _ = small
    idx = torch.from_numpy(g["logits.tokens"]).to(DEV)
    V = torch.from_numpy(g["V"]).to(DEV)
    inj = model.point_clip_to_special_tokens(torch.cat([V, V[:1]]))
    _close("point_clip_to_special_tokens vs reference", inj, g["logits.injection"], 1e-5)
    f = model.xformer(idx)
    assert f.shape == (3, 24, 48) and f.dtype == torch.float32
    _close("xformer.forward vs reference", f, g["logits.forward"], LOGIT_TOL)
    r = model.xformer.forward_with_replacement(idx, inj, tk)
    _close("xformer.forward_with_replacement vs reference", r, g["logits.replacement"], LOGIT_TOL)
    # rows without [UNK] are forward's rows; the logits are the same on a repeat
    assert torch.equal(r[1], f[1])
    assert torch.equal(model.xformer.forward_with_replacement(idx, inj, tk), r)
    with pytest.raises(NotImplementedError):
        model.xformer.forward_with_replacement(idx, inj, tk, inject_token="[CLIP]")


def _ce_vs_score(label, model, B, T, seed, tok_bound):
    """sum over a row of cross_entropy(forward_with_replacement logits) == coati_engine_score's NLL for h on the same padded rows"""
    eng = model.engine
    c = eng.cfg
    g = torch.Generator().manual_seed(seed)
    tokens, _ = _rand_rows(B, 8, T - 3, c.n_tok, c.stop_token, c.pad_token, 2, (c.unk_token,), seed)
    tokens = torch.cat([torch.full((B, 2), 8, dtype=torch.long), tokens], 1)
    tokens[:, 1] = c.unk_token
    y = torch.full_like(tokens, -1)
    y[:, :-1] = tokens[:, 1:]
    y[y == c.pad_token] = -1
    y[:, :2] = -1
    tokens, y = tokens.to(DEV), y.to(DEV)
    h = torch.randn(B, c.n_embd_common, generator=g).to(DEV)

    class Tk:
        vocab = {"[UNK]": c.unk_token}

    logits = model.xformer.forward_with_replacement(tokens, model.point_clip_to_special_tokens(h), Tk())
    ce = torch.nn.functional.cross_entropy(logits.reshape(-1, c.n_tok), y.reshape(-1), ignore_index=-1, reduction="none").view(B, -1).sum(1)
    nll = eng.score(tokens, y, h_clip=h)
    n_t = (y >= 0).sum(1).double().cpu()
    err = (ce.double().cpu() - nll.double().cpu()).abs()
    log(f"{label:58s} worst |dNLL| {float(err.max()):.3e}, per target {float((err / n_t).max()):.3e}  tol/target {tok_bound:.0e}")
    assert bool(torch.isfinite(ce).all())
    assert bool((err <= tok_bound * n_t).all())


def test_replacement_ce_equals_score_grande():
    from coati_amd.models.encoding.clip_e2e import e3gnn_smiles_clip_e2e
    with _quiet():
        model = e3gnn_smiles_clip_e2e(**GRANDE, device=torch.device(DEV))
    # the same bf16 activations feed both; score merges per-tile (max, sum exp) partials of the same product
    _ce_vs_score("grande CE(forward_with_replacement) vs score", model, 256, 80, 3, 2e-3)
    del model
    torch.cuda.empty_cache()


def test_replacement_ce_equals_score_norm_embed():
    from coati_amd.models.encoding.clip_e2e import e3gnn_smiles_clip_e2e
    with _quiet():
        model = e3gnn_smiles_clip_e2e(**dict(SMALL, n_tok=300, n_seq=64), norm_embed=True, device=torch.device(DEV))
    _ce_vs_score("norm_embed CE(forward_with_replacement) vs score", model, 32, 40, 4, 2e-3)


def test_decoder_logits_coati2():
    from coati_amd.models.simple_coati2.transformer_only import COATI_Smiles_Inference
    with _quiet():
        model = COATI_Smiles_Inference(n_layer_xformer=2, n_hidden_xformer=64, embed_dim=64, n_head=4, n_seq=32, n_tok=64,
                                       enc_to_coati="swiglu_resnet", device=torch.device(DEV))
    idx, _ = _rand_rows(4, 6, 20, 64, 40, 31, 35, (31, 40, 44), seed=8)
    idx[:, 1] = 44
    idx = idx.to(DEV)

    class Tk:
        vocab = {"[UNK]": 44}

    h = model.coati_to_token(torch.randn(4, 64, device=DEV))
    f, r = model.xformer(idx), model.xformer.forward_with_replacement(idx, h, Tk())
    assert f.shape == r.shape == (4, idx.shape[1], 64)
    assert bool(torch.isfinite(f).all() and torch.isfinite(r).all())
    assert torch.equal(f[:, :1], r[:, :1]) and not torch.equal(f[:, 1:], r[:, 1:])   # causal: position 0 precedes the injection


def test_group_mean_rows():
    from coati_amd import ops
    g = torch.Generator().manual_seed(1)
    for E in (64, 256, 300, 512):
        sizes = [3, 0, 1, 7, 0, 128, 2]
        off = [0]
        for s in sizes:
            off.append(off[-1] + s)
        N = off[-1] + 5
        x = torch.randn(N, E, generator=g)
        w = torch.randint(1, 9, (N,), generator=g).float()
        fb = torch.randn(len(sizes), E, generator=g)
        out = ops.group_mean_rows(x.to(DEV), off, w=w.to(DEV), fallback=fb.to(DEV))
        ref = torch.stack([(x[a:b].double() * w[a:b, None].double()).sum(0) / w[a:b].double().sum() if b > a else fb[i].double()
                           for i, (a, b) in enumerate(zip(off[:-1], off[1:]))])
        _close(f"group_mean_rows E={E} vs float64", out, ref, 2e-6)
        for i, s in enumerate(sizes):
            if s == 0:
                assert torch.equal(out[i].cpu(), fb[i])
        assert torch.equal(ops.group_mean_rows(x.to(DEV), off, w=w.to(DEV), fallback=fb.to(DEV)), out)
        unw = ops.group_mean_rows(x.to(DEV), off, fallback=fb.to(DEV))
        assert torch.allclose(unw[0].cpu(), x[0:3].mean(0), atol=1e-6)


class _Scripted:
    """replaces the model's hclip_to_2d_batch by a script of per-call lists (the rows a call receives are checked)"""

    def __init__(self, model, script):
        self.model, self.script, self.calls = model, list(script), []

    def __enter__(self):
        def fn(h, tokenizer, **kw):
            self.calls.append(int(h.shape[0]))
            item = self.script.pop(0)
            assert len(item) == h.shape[0], (len(item), h.shape)
            return list(item)
        object.__setattr__(self.model, "hclip_to_2d_batch", fn)
        return self

    def __exit__(self, *a):
        del self.model.__dict__["hclip_to_2d_batch"]


def test_batched_forms_equal_per_vector_forms(small):
    from coati.generative import coati_purifications as P
    model, tk, g, _ = small
    rng = np.random.default_rng(3)
    pool = ["CCO", "OCC", "CCN", "NCC", "C=CC#N", "CX", "CxC", "", "NCCO", "OCCN", "FC(F)(F)S", "CC(=O)O", "X"]
    N, n_rep = 5, 16
    dec = [[pool[i] for i in rng.integers(0, len(pool), n_rep)] for _ in range(N)]
    dec[2] = ["CX"] * n_rep                                   # nothing survives: V[2] comes back
    V = torch.randn(N, SMALL["n_embd_common"], generator=torch.Generator().manual_seed(2)).to(DEV)
    with _quiet():
        with _Scripted(model, [sum(dec, [])]) as s:
            batched = P.purify_vectors(V, model, tk, n_rep=n_rep, canon_smiles=_canon)
        assert s.calls == [N * n_rep]
        with _Scripted(model, dec):
            single = [P.purify_vector(V[i], model, tk, n_rep=n_rep, canon_smiles=_canon) for i in range(N)]
    assert single[2] is V[2] or torch.equal(single[2], V[2])
    _close("purify_vectors vs stacked purify_vector", batched, torch.stack([t.cpu() for t in single]), 1e-5)
    assert torch.equal(batched[2], V[2])
    # force_decode_valid_batches == per-vector force_decode_valid_batch, attempt by attempt
    att = [[[pool[i] for i in rng.integers(0, len(pool), 6)] for _ in range(N)] for _ in range(3)]
    att[0][1] = ["X"] * 6
    att[1][1] = ["CX"] * 6
    want = []
    for v in range(N):
        script = [att[a][v] for a in range(3)]
        with _Scripted(model, script):
            want.append(P.force_decode_valid_batch(V[v], model, tk, batch_size=6, max_attempts=3, canon_smiles=_canon))
    script, todo = [], list(range(N))
    for a in range(3):
        script.append(sum((att[a][v] for v in todo), []))
        todo = [v for v in todo if P.most_frequent_valid(att[a][v], _canon) is None]
    with _Scripted(model, script):
        got = P.force_decode_valid_batches(V, model, tk, batch_size=6, max_attempts=3, canon_smiles=_canon)
    log(f"force_decode_valid_batches {got}")
    assert got == want


def test_purify_and_force_match_golden(small):
    from coati.generative import coati_purifications as P
    model, tk, g, _ = small
    V = torch.from_numpy(g["V"]).to(DEV)
    with _quiet():
        with _Scripted(model, [g["purify.0.in"].tolist()]):
            p0 = P.purify_vector(V[0], model, tk, n_rep=8, canon_smiles=_canon)
        _close("purify_vector vs reference", p0, g["purify.0.out"], EMBED_TOL)
        for i in range(2):
            attempts = [g[f"force_batch.{i}.in.{j}"].tolist() for j in range(2)]
            with _Scripted(model, attempts):
                assert P.force_decode_valid_batch(V[0], model, tk, batch_size=6, max_attempts=2, canon_smiles=_canon) == str(g[f"force_batch.{i}.out"])


def test_density_matches_golden(small, monkeypatch):
    from coati.generative import coati_density as D
    model, tk, g, _ = small
    trils, real = [], D.MultivariateNormal

    def mvn(loc, scale_tril=None, **k):
        trils.append(scale_tril.detach().double().cpu())
        return real(loc, scale_tril=scale_tril, **k)

    monkeypatch.setattr(D, "MultivariateNormal", mvn)
    # the golden's own embeddings: the fit itself is held tightly
    emb = torch.from_numpy(g["density.embeds"]).to(DEV)
    parts = list(torch.split(emb, g["density.batch_rows"].tolist()))
    real_embeds = D._batch_embeds
    monkeypatch.setattr(D, "_batch_embeds", lambda *a, **k: parts.pop(0))
    with _quiet():
        assert D.estimate_density_batchwise(g["density.in"].tolist(), model, tk, batch_size=4, epochs=2, canon_smiles=_canon) is None
    _close("density fit on the reference's embeddings (scale_tril)", torch.stack(trils), g["density.scale_tril"], 2e-5)
    # end to end: the engine's embeddings
    trils.clear()
    monkeypatch.setattr(D, "_batch_embeds", real_embeds)
    with _quiet():
        assert D.estimate_density_batchwise(g["density.in"].tolist(), model, tk, batch_size=4, epochs=2, canon_smiles=_canon) is None
    _close("density fit end to end (scale_tril)", torch.stack(trils), g["density.scale_tril"], 2e-3)
    # an early return below entropy_limit hands back the distribution
    with _quiet():
        d = D.estimate_density_batchwise(g["density.in"].tolist(), model, tk, batch_size=4, epochs=1, entropy_limit=1e9, canon_smiles=_canon)
    assert d is not None and d.loc.shape == (SMALL["n_embd_common"],)


def test_unscripted_grande():
    """random grande weights, N = 8 vectors x 128 copies: finite output of the right shapes (decodes run to full length)"""
    from coati.generative import coati_purifications as P
    from coati_amd.models.encoding.clip_e2e import e3gnn_smiles_clip_e2e
    from coati_amd.models.encoding.tokenizers import TrieTokenizer
    voc = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tokenizer.json")))
    tk = TrieTokenizer(n_seq=250, special_tokens=voc["special"], smiles_tokens=[f"Z{i}Z" for i in range(GRANDE["n_tok"] - len(voc["special"]))])
    with _quiet():
        model = e3gnn_smiles_clip_e2e(**GRANDE, device=torch.device(DEV))
    V = torch.randn(8, GRANDE["n_embd_common"], generator=torch.Generator().manual_seed(9)).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(1)
    with _quiet():
        out = P.purify_vectors(V, model, tk, n_rep=128, generator=gen)
        strs = P.force_decode_valid_batches(V, model, tk, batch_size=128, max_attempts=1, generator=gen)
    assert out.shape == V.shape and bool(torch.isfinite(out).all())
    assert len(strs) == 8 and all(isinstance(s, str) for s in strs)
    log(f"unscripted grande: purified rows changed {int((out != V).any(1).sum())}/8, strings of length {[len(s) for s in strs]}")


def test_training_untouched(small):
    """train_step, every new call, train_step == two train_steps; the flat buffers do not move under the new calls"""
    from coati_amd import ops
    from coati_amd.engine import Engine, ModelConfig
    from coati_amd.synthetic import make_batch
    _, tk, g, sd = small
    b, up = make_batch(16, 20, 6, 48, seed=3, n_special=12, min_len=4, with_rows=True)
    db = {k: (v if k == "rows" else v.to(DEV)) for k, v in b.items()}
    up = up.to(DEV)

    def engine():
        e = Engine(ModelConfig(**SMALL), DEV, train=True)
        e.load_state_dict(sd, strict=False)
        return e

    a, c = engine(), engine()
    a.train_step(db, up, lr=5e-4)
    a.train_step(db, up, lr=5e-4)
    La = a.losses()
    c.train_step(db, up, lr=5e-4)
    before = {k: getattr(c, k).clone() for k in ("params", "grads", "adam_m", "adam_v", "shadow")}
    raw = db["raw_tokens"]
    c.encode(raw, rows=int(b["rows"][0]))
    c.decoder_logits(db["tokens"], torch.randn(16, SMALL["n_hidden_xformer"], device=DEV))
    ops.group_mean_rows(torch.randn(8, 64, device=DEV), [0, 3, 8], fallback=torch.zeros(2, 64, device=DEV))
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(c, k), v), k
    with pytest.raises(RuntimeError):
        c.backward()
    c.train_step(db, up, lr=5e-4)
    Lc = c.losses()
    log(f"train/new calls/train vs train/train: {Lc} vs {La}")
    for k in ("ar_loss", "clip_loss", "grad_norm"):
        assert math.isfinite(Lc[k]) and abs(Lc[k] - La[k]) <= 5e-6 * abs(La[k]), (k, Lc, La)
