"""
Golden vectors for COATI2 likelihood scoring and its gradient w.r.t. the embedding, produced by IMPORTING THE REFERENCE in the build
container (stubs of gen_golden.py).  The reference has no COATI2 likelihood method: the fixture is built from its own modules, every row
unpadded,

    logits = model.xformer.forward_with_replacement(tk, model.coati_to_token(h[None]), tok)
    nll    = cross_entropy(logits[0], y_next, ignore_index=-1, reduction="sum")

on rows [CLIP][UNK][SMILES] (+ [SUFFIX][MIDDLE]) <smi>[STOP] -- the prompt hcoati_to_2d decodes from -- with the targets masked as
clip_e2e.py:647-654 masks them ([CLIP] / [PAD] / [SMILES] / [UNK] / [SUFFIX] / [MIDDLE] -> -1; nothing behind [STOP]).

Small part: the model, vocabulary and weights of coati2_golden.npz / coati2_vocab.json (gen_golden_coati2.py), its three smiles_to_coati
variants.  Per variant 16 rows: the 8 SMILES without the suffix pair, scored under the stored "<variant>.encode" rows, and the same 8
with it, scored under one seeded random [8, 64].  Per row: tokens / y_next (padded with [PAD] / -1), h, nll, dh = d nll / d h from
autograd, the central difference of nll along dh / |dh| (eps 1e-2, the model and h in float64), and the NLLs of ten plain gradient-descent
steps h <- h - step dh (entry 0 = the start).  "<variant>.step": of the STEPS for which every row's trajectory falls strictly, the one
whose smallest single-step drop over the 16 rows is largest -- the trajectory furthest from flat: a step near the stability edge, or one
that has converged after a few iterations, ends in drops that any rounding of the forward pass outweighs.  Per variant also the round trip: encode_tokens of [SMILES]<smi>[STOP] -> the same likelihood (no suffix pair), for the 8
SMILES and two strings that must be dropped (one too long behind the prompt, one that does not tokenize), with the mask.

Full part: FULL of tests/coati2_full_weights.py (12 layers, d = 512, 16 heads of 32, n_seq 250, V = 4266, swiglu_resnet) with that
module's seeded weights (not stored: per-parameter checksums), 16 rows: the prompt (odd rows with the suffix pair) + a random body of
8..57 non-special ids + [STOP], a seeded h [16, 512].  Stored: tokens, y_next, h, nll, dh, the central difference.

    python tests/golden/gen_golden_coati2_likelihood.py            # (re)write tests/golden/coati2_likelihood_golden.npz  (a minute of CPU)
    python tests/golden/gen_golden_coati2_likelihood.py --verify   # regenerate into a scratch directory and compare contents
"""
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

EPS = 1e-2
N_DESCENT = 10
STEPS = (20.0, 10.0, 5.0, 2.0, 1.0)
S2S_EXTRA = ["C" * 59, "CC%O"]      # 31 ids with [STOP]: inside n_seq = 32, too long behind the 3 prompt ids; a piece without an id
B_FULL, BODY_LO, BODY_HI, N_SPECIAL_FULL = 16, 8, 57, 330
NAME = "coati2_likelihood_golden.npz"


class _Logger:
    def setLevel(self, level):
        pass


class _UnkOnly:
    """what forward_with_replacement reads of a tokenizer"""

    def __init__(self, unk):
        self.vocab = {"[UNK]": unk}


def masked_targets(tokens, ids, pad):
    """the next token per position, [PAD] behind the last one; the ids of clip_e2e.py:647-654 -> -1"""
    y = torch.full_like(tokens, pad)
    y[:, :-1] = tokens[:, 1:]
    for t in ids:
        y[y == t] = -1
    return y


def make_fn(model, tok, tk, yn):
    def fn(x):
        logits = model.xformer.forward_with_replacement(tk, model.coati_to_token(x.unsqueeze(0)), tok)
        return torch.nn.functional.cross_entropy(logits[0], yn, ignore_index=-1, reduction="sum")
    fn.model = model
    return fn


def pad_rows(rows, fill):
    out = torch.full((len(rows), max(len(r) for r in rows)), fill, dtype=torch.long)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.as_tensor(r, dtype=torch.long)
    return out


def main():
    import gen_golden as G   # inserts the stubs, imports the reference
    import gen_golden_coati2 as G2
    from gen_golden_score_grad import EPS as _EPS, central_difference, nll_and_grad
    assert _EPS == EPS
    sys.modules["rdkit.RDLogger"].logger = lambda: _Logger()   # transformer_only.py:14-16
    from coati.models.simple_coati2.transformer_only import COATI_Smiles_Inference
    from coati.models.simple_coati2.trie_tokenizer import TrieTokenizer
    from tests.coati2_full_weights import FULL, SEED, checksums, full_param_shapes, full_weights
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))

    g = np.load(os.path.join(HERE, "coati2_golden.npz"))
    voc = json.load(open(os.path.join(HERE, "coati2_vocab.json")))
    tok = TrieTokenizer(n_seq=voc["n_seq"], special_tokens=voc["special_tokens"], smiles_tokens=voc["smiles_tokens"])
    masked = (tok.clip_token, tok.pad_token, tok.smiles_token, tok.unk_token, tok.suffix_token, tok.middle_token)
    kw = dict(n_layer_xformer=G2.N_LAYER, n_hidden_xformer=G2.D, embed_dim=G2.D, n_head=G2.N_HEAD, mlp_dropout=0.0, n_direct_clr=16,
              n_tok=tok.n_token, biases=True, device=torch.device("cpu"))
    out = dict(eps=np.float64(EPS), smiles=np.array(G2.SMILES), masked_ids=np.array(masked), stop_token=np.int64(tok.stop_token),
               pad_token=np.int64(tok.pad_token))
    out["s2s.smiles"] = np.array(G2.SMILES + S2S_EXTRA)

    rows = []
    for sfx in (False, True):
        for smi in G2.SMILES:
            rows.append(tok.tokenize_text("[CLIP][UNK][SMILES]" + ("[SUFFIX][MIDDLE]" if sfx else "") + smi + "[STOP]", pad=False))
    tokens = pad_rows(rows, tok.pad_token)
    y_next = masked_targets(tokens, masked, tok.pad_token)
    out.update({"small.tokens": tokens, "small.y_next": y_next, "small.do_suffix": np.array([False] * 8 + [True] * 8)})
    h_rand = torch.randn(len(G2.SMILES), G2.D, generator=torch.Generator().manual_seed(64))

    models = {}
    for variant in G2.VARIANTS:
        torch.manual_seed(0)
        model = COATI_Smiles_Inference(n_seq=G2.N_SEQ, enc_to_coati=variant, **kw)
        sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}
        sd.update({k[len(variant) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(variant + ".w.")})
        missing, unexpected = model.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith(".attn.bias") for k in missing), (missing, unexpected)
        model.eval()
        for p in model.parameters():
            p.requires_grad_(False)
        models[variant] = model
        h = torch.cat([torch.from_numpy(g[f"{variant}.encode"]), h_rand])
        fns = []
        nll, dh, cd = [], [], []
        for b in range(len(rows)):
            L = len(rows[b])
            fn = make_fn(model, tok, tokens[b:b + 1, :L], y_next[b, :L])
            fns.append(fn)
            n, gr = nll_and_grad(fn, h[b])
            nll.append(n); dh.append(gr); cd.append(central_difference(fn, h[b], gr))
        out.update({f"{variant}.h": h, f"{variant}.nll": torch.stack(nll), f"{variant}.dh": torch.stack(dh), f"{variant}.cd": torch.stack(cd)})
        models[variant + ".fns"] = fns
        # ---- the round trip: encode_tokens -> the likelihood of the same string ----
        s2s, mask = [], []
        for smi in G2.SMILES + S2S_EXTRA:
            try:
                body = tok.tokenize_text(smi + "[STOP]", pad=False)
            except Exception:   # KeyError: a piece without an id; the oversized-string exception
                body = None
            ok = body is not None and len(body) <= tok.n_seq - 3
            mask.append(ok)
            if not ok:
                continue
            with torch.no_grad():
                hs = model.encode_tokens(torch.tensor([[tok.smiles_token] + body]), tok)[0]
                tk = torch.tensor([[tok.clip_token, tok.unk_token, tok.smiles_token] + body])
                s2s.append(make_fn(model, tok, tk, masked_targets(tk, masked, tok.pad_token)[0])(hs))
        out.update({f"{variant}.s2s.nll": torch.stack(s2s), "s2s.mask": np.array(mask)})

    # ---- descent, per variant: of the steps whose every trajectory falls strictly, the one whose smallest single-step drop is largest ----
    for variant in G2.VARIANTS:
        h, best = out[f"{variant}.h"], None
        for cand in STEPS:
            traj = []
            for b, fn in enumerate(models[variant + ".fns"]):
                t, x = [out[f"{variant}.nll"][b]], h[b].clone()
                for _ in range(N_DESCENT):
                    _, gx = nll_and_grad(fn, x)
                    x = x - cand * gx
                    with torch.no_grad():
                        t.append(fn(x))
                traj.append(torch.stack(t))
            traj = torch.stack(traj)
            least = float((traj[:, :-1] - traj[:, 1:]).min())
            if least > 0 and (best is None or least > best[0]):
                best = (least, cand, traj)
        assert best is not None, f"{variant}: no step of STEPS gives strictly decreasing trajectories"
        print(f"{variant}: step {best[1]}, smallest single-step drop {best[0]:.4f}")
        out[f"{variant}.step"], out[f"{variant}.traj"] = np.float64(best[1]), best[2]

    # ---- full shape ----
    W = full_weights()
    names = [n for n, _ in full_param_shapes()]
    torch.manual_seed(0)
    big = COATI_Smiles_Inference(n_layer_xformer=FULL["n_layer_xformer"], n_hidden_xformer=FULL["n_hidden_xformer"], embed_dim=FULL["embed_dim"],
                                 n_head=FULL["n_head"], n_seq=FULL["n_seq"], n_tok=FULL["n_tok"], mlp_dropout=0.0, enc_to_coati="swiglu_resnet",
                                 biases=True, device=torch.device("cpu"))
    assert [k for k in big.state_dict().keys() if not k.endswith(".attn.bias")] == names
    missing, unexpected = big.load_state_dict(W, strict=False)
    assert not unexpected and all(k.endswith(".attn.bias") for k in missing), (missing, unexpected)
    big.eval()
    for p in big.parameters():
        p.requires_grad_(False)
    gen = torch.Generator().manual_seed(5120)
    frows = []
    for b in range(B_FULL):
        n_body = int(torch.randint(BODY_LO, BODY_HI + 1, (1,), generator=gen))
        body = torch.randint(N_SPECIAL_FULL, FULL["n_tok"], (n_body,), generator=gen).tolist()
        prefix = [tok.clip_token, tok.unk_token, tok.smiles_token] + ([tok.suffix_token, tok.middle_token] if b % 2 else [])
        frows.append(prefix + body + [tok.stop_token])
    ftok = pad_rows(frows, tok.pad_token)
    fy = masked_targets(ftok, masked, tok.pad_token)
    hf = torch.randn(B_FULL, FULL["embed_dim"], generator=gen)
    unk = _UnkOnly(tok.unk_token)
    nll, dh, cd = [], [], []
    for b in range(B_FULL):
        L = len(frows[b])
        fn = make_fn(big, unk, ftok[b:b + 1, :L], fy[b, :L])
        n, gr = nll_and_grad(fn, hf[b])
        nll.append(n); dh.append(gr); cd.append(central_difference(fn, hf[b], gr))
    ws, wa = checksums(W, names)
    out.update({"full.tokens": ftok, "full.y_next": fy, "full.h": hf, "full.nll": torch.stack(nll), "full.dh": torch.stack(dh),
                "full.cd": torch.stack(cd), "full.seed": np.array(SEED), "full.names": np.array(names), "full.wsum": np.array(ws),
                "full.wabs": np.array(wa)})
    np.savez_compressed(os.path.join(OUT, NAME), **G.npify(out))
    print("written", os.path.join(OUT, NAME))


def verify():
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, GOLDEN_OUT=tmp), check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        x, y = np.load(os.path.join(tmp, NAME)), np.load(os.path.join(HERE, NAME))
        ok = x.files == y.files
        for k in x.files:
            if x[k].dtype.kind == "f":   # (CPU sums re-associate across thread counts: 1e-5 of scale, as gen_golden_score_grad.py)
                sc = max(float(np.abs(y[k]).max()), 1e-30)
                same = x[k].shape == y[k].shape and float(np.abs(x[k] - y[k]).max()) <= 1e-5 * sc
            else:
                same = np.array_equal(x[k], y[k])
            if not same:
                print("DIFFERENT", k)
                ok = False
        print(NAME, "same" if ok else "DIFFERENT")
        return ok


if __name__ == "__main__":
    if "--verify" in sys.argv:
        sys.exit(0 if verify() else 1)
    main()
