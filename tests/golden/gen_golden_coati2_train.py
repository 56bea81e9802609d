"""
Golden vectors for the COATI2 training step, produced by IMPORTING THE REFERENCE in the build container (stubs of gen_golden.py).  The
reference has no COATI2 training code: the step is defined from its own modules under autograd, fp32 on the CPU, dropout 0,

    h      = model.smiles_to_coati(model.xformer.encode(raw_tokens, tok))                  # [B, E]
    logits = model.xformer.forward_with_replacement(tokens, model.coati_to_token(h), tok)
    ar     = cross_entropy(logits.view(-1, V), y_next.view(-1), ignore_index=-1)           # mean over the targets, as forward_dist's AR loss
    total  = ar + (h * dh_ext).sum()                                                       # dh_ext: an external gradient w.r.t. h, or 0

then clip_grad_norm_(10) and torch.optim.AdamW(lr, weight_decay 0.1, betas (0.9, 0.99), eps 1e-8) over all parameters: gen_golden.py's
optimiser settings.  Rows are those of coati2_likelihood_golden.npz -- decoder [CLIP][UNK][SMILES] (+ [SUFFIX][MIDDLE]) <smi>[STOP] with its
masked targets -- and the encoder's [SMILES]<smi>[STOP] of the same strings.

Small part: the model of coati2_golden.npz (2 layers, d = 64, 4 heads of 16, n_seq 32), its three smiles_to_coati variants, the 16 small
rows (8 plain, 8 with the suffix pair).  Per variant: h, logits, ar; every parameter gradient with dh_ext = 0 ("g0.") and with one seeded
dh_ext ("g1."), the gradient norm clip_grad_norm_ returns for both; a 20-step loss curve on the fixed batch with the first lr of LRS whose
curve's last-4 mean is below 0.85 x its first-4 mean (recorded); for swiglu_resnet the parameters after 1 and 3 of those steps.
Self-check: the directional derivative of `total` along its own gradient, |g|, agrees with the central difference of the float64 model
(eps 1e-3 along g / |g|) to 1e-3 of its value.

Edge part (swiglu_resnet, dh_ext = 0; gradients stored like the full part's): "one" -- one row alone, B = 1, the 3-token body C#N; "fail" --
the first three small rows with a failure row between them as the data pipeline leaves it: the decoder's row all [PAD] (no target, no
[UNK]), the encoder's row a lone [STOP].

Full part: FULL of tests/coati2_full_weights.py (12 layers, d = 512, 16 heads of 32, V = 4266, swiglu_resnet), the 16 full rows, dh_ext = 0.
The gradients are ~ 170 MB: stored are, per parameter, the gradient's 2-norm and every ceil(numel / 1024)-th element of the flat gradient;
h, ar, the total norm.

No committed file may exceed 1 MiB and one set of the small model's gradients is 0.44 MB of float32, so the per-parameter arrays live in
companions of coati2_train_golden.npz: coati2_train_golden_<variant>.npz ("g0.<name>", "g1.<name>") and coati2_train_golden_steps.npz
("after1.<name>", "after3.<name>" of swiglu_resnet).  Everything else is in coati2_train_golden.npz.

    python tests/golden/gen_golden_coati2_train.py            # (re)write tests/golden/coati2_train_golden*.npz
    python tests/golden/gen_golden_coati2_train.py --verify   # regenerate into a scratch directory and compare contents
"""
import copy
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.environ.get("GOLDEN_OUT", HERE)
sys.path.insert(0, HERE)
sys.path.insert(1, ROOT)

NAME = "coati2_train_golden.npz"
LRS = (5e-4, 1e-3, 2e-3, 5e-3, 1e-2)      # gen_golden.py's 5e-4 first
OPT = dict(weight_decay=0.1, betas=(0.9, 0.99), eps=1e-8)
MAX_NORM = 10.0
N_CURVE = 20
CD_EPS, CD_TOL = 1e-3, 1e-3
N_SAMPLE = 1024


class _Logger:
    def setLevel(self, level):
        pass


class _Tok:
    """what encode / forward_with_replacement read of a tokenizer"""

    def __init__(self, stop, unk):
        self.stop_token = stop
        self.vocab = {"[UNK]": unk}


def raw_rows(tokens, stop, smiles_token, pad):
    """[SMILES]<smi>[STOP] of every decoder row [CLIP][UNK][SMILES] (+ [SUFFIX][MIDDLE]) <smi>[STOP]: what follows the row's [SMILES]"""
    rows = []
    for r in tokens.tolist():
        i, j = r.index(smiles_token), r.index(stop)
        rows.append(r[i:j + 1])
    out = torch.full((len(rows), max(len(r) for r in rows)), pad, dtype=torch.long)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.tensor(r)
    return out


def step_loss(model, tok, raw, tokens, y_next, dh_ext=None):
    h = model.smiles_to_coati(model.xformer.encode(raw, tok))
    logits = model.xformer.forward_with_replacement(tokens, model.coati_to_token(h), tok)
    ar = torch.nn.functional.cross_entropy(logits.view(-1, logits.size(-1)), y_next.view(-1), ignore_index=-1)
    total = ar if dh_ext is None else ar + (h * dh_ext.to(h.dtype)).sum()
    return h, logits, ar, total


def grads_of(model, tok, raw, tokens, y_next, dh_ext):
    model.zero_grad(set_to_none=True)
    h, logits, ar, total = step_loss(model, tok, raw, tokens, y_next, dh_ext)
    total.backward()
    g = {n: p.grad.clone() for n, p in model.named_parameters()}
    gn = torch.nn.utils.clip_grad_norm_(model.parameters(), MAX_NORM)
    return h.detach(), logits.detach(), ar.detach(), g, gn.detach()


def check_direction(model, tok, raw, tokens, y_next, dh_ext, g, what):
    """|g| against the central difference of the float64 model along g / |g|"""
    norm = torch.sqrt(sum((v.double() ** 2).sum() for v in g.values()))
    m64 = copy.deepcopy(model).double()
    base = {n: p.detach().clone() for n, p in m64.named_parameters()}
    val = []
    for sign in (1.0, -1.0):
        with torch.no_grad():
            for n, p in m64.named_parameters():
                p.copy_(base[n] + sign * CD_EPS * g[n].double() / norm)
            val.append(float(step_loss(m64, tok, raw, tokens, y_next, None if dh_ext is None else dh_ext.double())[3]))
    cd = (val[0] - val[1]) / (2 * CD_EPS)
    rel = abs(cd - float(norm)) / float(norm)
    print(f"{what}: |g| {float(norm):.6f}, float64 central difference {cd:.6f}, relative difference {rel:.2e}")
    assert rel <= CD_TOL, (what, float(norm), cd)
    return cd


def curve(model0, tok, raw, tokens, y_next, lr, keep=()):
    model = copy.deepcopy(model0)
    opt = torch.optim.AdamW(model.parameters(), lr=lr, **OPT)
    losses, norms, kept = [], [], {}
    for step in range(N_CURVE):
        opt.zero_grad()
        _, _, ar, total = step_loss(model, tok, raw, tokens, y_next)
        total.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), MAX_NORM)))
        opt.step()
        losses.append(float(ar.detach()))
        if step + 1 in keep:
            kept[step + 1] = {n: p.detach().clone() for n, p in model.named_parameters()}
    return np.array(losses, dtype=np.float64), np.array(norms, dtype=np.float64), kept


def main():
    import gen_golden as G   # inserts the stubs, imports the reference
    import gen_golden_coati2 as G2
    sys.modules["rdkit.RDLogger"].logger = lambda: _Logger()   # transformer_only.py:14-16
    from coati.models.simple_coati2.transformer_only import COATI_Smiles_Inference
    from tests.coati2_full_weights import FULL, checksums, full_param_shapes, full_weights
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))

    g = np.load(os.path.join(HERE, "coati2_golden.npz"))
    lk = np.load(os.path.join(HERE, "coati2_likelihood_golden.npz"))
    voc = json.load(open(os.path.join(HERE, "coati2_vocab.json")))
    special = voc["special_tokens"]
    ids = {n: special.index(n) for n in ("[PAD]", "[STOP]", "[UNK]", "[SMILES]")}
    assert ids["[PAD]"] == int(lk["pad_token"]) and ids["[STOP]"] == int(lk["stop_token"])
    tok = _Tok(ids["[STOP]"], ids["[UNK]"])
    n_tok = len(special) + len(voc["smiles_tokens"])
    out = dict(max_norm=np.float64(MAX_NORM), weight_decay=np.float64(OPT["weight_decay"]), betas=np.array(OPT["betas"]), eps=np.float64(OPT["eps"]),
               lrs=np.array(LRS))
    side = {}

    tokens, y_next = torch.from_numpy(lk["small.tokens"]), torch.from_numpy(lk["small.y_next"])
    raw = raw_rows(tokens, ids["[STOP]"], ids["[SMILES]"], ids["[PAD]"])
    dh_ext = 0.05 * torch.randn(tokens.shape[0], G2.D, generator=torch.Generator().manual_seed(2064))
    out.update({"small.raw_tokens": raw, "small.tokens": tokens, "small.y_next": y_next, "small.dh_ext": dh_ext})
    kw = dict(n_layer_xformer=G2.N_LAYER, n_hidden_xformer=G2.D, embed_dim=G2.D, n_head=G2.N_HEAD, mlp_dropout=0.0, n_direct_clr=16,
              n_tok=n_tok, biases=True, device=torch.device("cpu"))
    for variant in G2.VARIANTS:
        torch.manual_seed(0)
        model = COATI_Smiles_Inference(n_seq=G2.N_SEQ, enc_to_coati=variant, **kw)
        sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}
        sd.update({k[len(variant) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(variant + ".w.")})
        missing, unexpected = model.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith(".attn.bias") for k in missing), (missing, unexpected)
        model.train()   # (dropout 0: the same function as eval())
        h, logits, ar, g0, gn0 = grads_of(model, tok, raw, tokens, y_next, None)
        _, _, _, g1, gn1 = grads_of(model, tok, raw, tokens, y_next, dh_ext)
        cd0 = check_direction(model, tok, raw, tokens, y_next, None, g0, f"{variant} dh_ext = 0")
        cd1 = check_direction(model, tok, raw, tokens, y_next, dh_ext, g1, f"{variant} seeded dh_ext")
        out.update({f"{variant}.h": h, f"{variant}.logits": logits, f"{variant}.ar": ar, f"{variant}.gradnorm0": gn0, f"{variant}.gradnorm1": gn1,
                    f"{variant}.cd0": np.float64(cd0), f"{variant}.cd1": np.float64(cd1)})
        side[f"coati2_train_golden_{variant}.npz"] = {**{f"g0.{n}": v for n, v in g0.items()}, **{f"g1.{n}": v for n, v in g1.items()}}
        for lr in LRS:
            losses, norms, kept = curve(model, tok, raw, tokens, y_next, lr, keep=(1, 3) if variant == "swiglu_resnet" else ())
            if losses[-4:].mean() < 0.85 * losses[:4].mean():
                break
        else:
            raise AssertionError(f"{variant}: no lr of {LRS} brings the curve's last-4 mean below 0.85 x its first-4 mean")
        print(f"{variant}: lr {lr}, curve {losses[0]:.4f} -> {losses[-1]:.4f}")
        out.update({f"{variant}.lr": np.float64(lr), f"{variant}.curve": losses, f"{variant}.curve_gradnorm": norms})
        if kept:
            side["coati2_train_golden_steps.npz"] = {f"after{k}.{n}": v for k, params in kept.items() for n, v in params.items()}

    # ---- edge shapes (the model left in `model` is swiglu_resnet, the last variant) ----
    assert variant == "swiglu_resnet"
    from coati.models.simple_coati2.trie_tokenizer import TrieTokenizer
    tt = TrieTokenizer(n_seq=voc["n_seq"], special_tokens=special, smiles_tokens=voc["smiles_tokens"])
    one = torch.tensor([tt.tokenize_text("[CLIP][UNK][SMILES]C#N[STOP]", pad=False)])
    assert one.shape[1] == 3 + 3 + 1
    masked = [int(t) for t in lk["masked_ids"]]
    y_one = torch.full_like(one, ids["[PAD]"])
    y_one[:, :-1] = one[:, 1:]
    for t in masked:
        y_one[y_one == t] = -1
    fail_tok = torch.cat([tokens[0:1], torch.full_like(tokens[0:1], ids["[PAD]"]), tokens[1:3]])
    fail_y = torch.cat([y_next[0:1], torch.full_like(y_next[0:1], -1), y_next[1:3]])
    fail_raw = torch.cat([raw[0:1], torch.full_like(raw[0:1], ids["[PAD]"]), raw[1:3]])
    fail_raw[1, 0] = ids["[STOP]"]
    for tag, (r_, t_, y_) in (("one", (raw_rows(one, ids["[STOP]"], ids["[SMILES]"], ids["[PAD]"]), one, y_one)), ("fail", (fail_raw, fail_tok, fail_y))):
        h, _, ar, ge, gne = grads_of(model, tok, r_, t_, y_, None)
        pn = list(ge)
        out.update({f"{tag}.raw_tokens": r_, f"{tag}.tokens": t_, f"{tag}.y_next": y_, f"{tag}.h": h, f"{tag}.ar": ar, f"{tag}.gradnorm": gne,
                    f"{tag}.names": np.array(pn), f"{tag}.gnorm": np.array([float(ge[n].double().norm()) for n in pn])})
        for n in pn:
            flat = ge[n].flatten()
            out[f"{tag}.gs.{n}"] = flat[::-(-flat.numel() // N_SAMPLE)].clone()

    # ---- full shape ----
    W = full_weights()
    names = [n for n, _ in full_param_shapes()]
    torch.manual_seed(0)
    big = COATI_Smiles_Inference(n_layer_xformer=FULL["n_layer_xformer"], n_hidden_xformer=FULL["n_hidden_xformer"], embed_dim=FULL["embed_dim"],
                                 n_head=FULL["n_head"], n_seq=FULL["n_seq"], n_tok=FULL["n_tok"], mlp_dropout=0.0, enc_to_coati="swiglu_resnet",
                                 biases=True, device=torch.device("cpu"))
    missing, unexpected = big.load_state_dict(W, strict=False)
    assert not unexpected and all(k.endswith(".attn.bias") for k in missing), (missing, unexpected)
    ftok, fy = torch.from_numpy(lk["full.tokens"]), torch.from_numpy(lk["full.y_next"])
    fraw = raw_rows(ftok, ids["[STOP]"], ids["[SMILES]"], ids["[PAD]"])
    h, _, ar, gf, gnf = grads_of(big, tok, fraw, ftok, fy, None)
    ws, wa = checksums(W, names)
    out.update({"full.raw_tokens": fraw, "full.tokens": ftok, "full.y_next": fy, "full.h": h, "full.ar": ar, "full.gradnorm": gnf,
                "full.names": np.array(names), "full.wsum": np.array(ws), "full.wabs": np.array(wa),
                "full.gnorm": np.array([float(gf[n].double().norm()) for n in names])})
    for n in names:
        flat = gf[n].flatten()
        out[f"full.gs.{n}"] = flat[::-(-flat.numel() // N_SAMPLE)].clone()
    side[NAME] = out
    for name, d in side.items():
        np.savez_compressed(os.path.join(OUT, name), **G.npify(d))
        print("written", os.path.join(OUT, name), os.path.getsize(os.path.join(OUT, name)), "bytes")
        assert os.path.getsize(os.path.join(OUT, name)) < (1 << 20), name


def verify():
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, GOLDEN_OUT=tmp), check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        names = sorted(os.listdir(tmp))
        ok = names == sorted(f for f in os.listdir(HERE) if f.startswith("coati2_train_golden") and f.endswith(".npz"))
        for name in names:
            x, y = np.load(os.path.join(tmp, name)), np.load(os.path.join(HERE, name))
            ok = ok and x.files == y.files
            for k in x.files:
                if x[k].dtype.kind == "f":   # (CPU sums re-associate across thread counts: 1e-5 of scale, as gen_golden_coati2_likelihood.py;
                    sc = max(float(np.abs(y[k]).max()), 1e-30)   # the 20-step curve and the stepped parameters carry up to 20 steps of it: 1e-4)
                    tol = 1e-4 if (".curve" in k or k.startswith("after")) else 1e-5
                    same = x[k].shape == y[k].shape and float(np.abs(x[k] - y[k]).max()) <= tol * sc
                else:
                    same = np.array_equal(x[k], y[k])
                if not same:
                    print("DIFFERENT", name, k)
                    ok = False
        print(NAME, "and companions", "same" if ok else "DIFFERENT")
        return ok


if __name__ == "__main__":
    if "--verify" in sys.argv:
        sys.exit(0 if verify() else 1)
    main()
