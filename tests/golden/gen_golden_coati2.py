"""
Golden vectors for the COATI2 inference model (simple_coati2/transformer_only.py:43-200: COATI_Smiles_Inference with its three
smiles_to_coati variants, encode_tokens, coati_to_token, hcoati_to_2d_batch and hcoati_to_2d), produced by IMPORTING THE
REFERENCE in the build container (stubs of gen_golden.py, plus an RDLogger.logger() whose result has setLevel).

Model: d = 64, 2 layers, 4 heads, n_seq = 32, biases on, V = 74.  Vocabulary (coati2_vocab.json): the first 45 special names
of coati2_12_12, which keep the real vocabulary's ids ([CLIP] = 2, [MASK] = 20, [MIDDLE] = 21, [PAD] = 31, [SMILES] = 39,
[STOP] = 40, [SUFFIX] = 41, [UNK] = 44), and 29 SMILES pieces of tokenizer.json.  The JSON also records the reference
tokenizer's ids and decodings of a few strings.  Seeded weights, the LayerNorms perturbed away from 1 / 0: one transformer
("w.xformer.*", every entry but the causal-mask buffers) shared by the three variants.  Per variant (npz keys "<variant>.*"): the
head weights, the reference's state_dict() key list, the
encode_tokens outputs of 8 [SMILES]..[STOP] rows, coati_to_token of a fixed [5, E] input, and the generated rows:
hcoati_to_2d_batch (k = 2, inv_temp = 1e4: greedy in effect, the reference asserts k > 1) of the 8 embeddings, and
hcoati_to_2d (k = 1) of one [1, E] row and of one 1-D [E] vector (whose payload is the scalar h_token[0]).  With every
generated step the top-2 margin of the logits it was drawn from, relative to the row's largest |logit|, so that a test can
tell near-ties from real differences.  hcoati_to_2d raises on a sequence that does not stop within n_seq positions: those
calls run on a copy with a 2 * n_seq causal-mask buffer (same weights) and the first n_seq positions are kept
(gen_golden_generation.py's recipe).

    python tests/golden/gen_golden_coati2.py            # (re)write coati2_golden.npz and coati2_vocab.json
    python tests/golden/gen_golden_coati2.py --verify   # regenerate into a scratch directory and compare contents
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("GOLDEN_OUT", HERE)
sys.path.insert(0, HERE)

N_SEQ, D, N_LAYER, N_HEAD = 32, 64, 2, 4
VARIANTS = ("linear", "swiglu_mlp", "swiglu_resnet")
STOP_SCALE = 0.85   # lm_head's [STOP] row: some rows stop at once, others run to the forced [STOP]
SMILES = ["CCO", "c1ccccc1N", "CC(=O)O", "N(C)C(=O)OCc1ccccc1Cl", "ClCC(=O)OCC(=O)OC1CC", "C#N", "OC(=O)c1ccccc1", "c1ccccc1Br"]
TOK_CASES = ["[SMILES]CCO[STOP]", "[CLIP][UNK][SMILES]c1ccccc1N[STOP]", "[SMILES]CC[SUFFIX]O[MIDDLE]C(=O)[STOP][PAD][PAD]",
             "[MASK]C(=O)O[SET][FORMULA]", "[GRAPH]N(C)CBr[STOP]"]


class _Logger:
    def setLevel(self, level):
        pass


def _vocab(G):
    voc = json.load(open(os.path.join(HERE, "tokenizer.json")))
    special = json.load(open(os.path.join(G.REF, "coati/models/encoding/tokenizers/vocabs/coati2_12_12.json")))["special_tokens"][:45]
    return {"special_tokens": special, "smiles_tokens": voc["smiles"][:29]}


def _margins(lg):
    """relative top-2 margin of every row of lg [B, V]"""
    top2 = torch.topk(lg, 2, dim=1).values
    return ((top2[:, 0] - top2[:, 1]) / lg.abs().max(dim=1).values).numpy()


def main():
    import gen_golden as G   # inserts the stubs, imports the reference
    sys.modules["rdkit.RDLogger"].logger = lambda: _Logger()   # transformer_only.py:14-16
    from coati.models.simple_coati2.transformer_only import COATI_Smiles_Inference
    from coati.models.simple_coati2.trie_tokenizer import TrieTokenizer
    voc = _vocab(G)
    tok = TrieTokenizer(n_seq=N_SEQ, **voc)
    V = tok.n_token
    assert (tok.clip_token, tok.mask_token, tok.middle_token, tok.pad_token, tok.smiles_token, tok.stop_token, tok.suffix_token,
            tok.unk_token) == (2, 20, 21, 31, 39, 40, 41, 44)
    cases = [{"text": t, "ids": tok.tokenize_text(t, pad=False)} for t in TOK_CASES]
    for c in cases:
        c["decode"] = tok.decode(c["ids"])
        c["decode_plain"] = tok.decode(c["ids"], special=False)
    ids = {n: getattr(tok, n) for n in ("pad_token", "stop_token", "unk_token", "clip_token", "smiles_token", "suffix_token",
                                        "middle_token", "mask_token", "graph_token", "formula_token", "set_token", "n_special", "n_token")}
    doc = dict(voc, n_seq=N_SEQ, ids=ids, cases=cases)
    with open(os.path.join(OUT, "coati2_vocab.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")

    kw = dict(n_layer_xformer=N_LAYER, n_hidden_xformer=D, embed_dim=D, n_head=N_HEAD, mlp_dropout=0.0, n_direct_clr=16, n_tok=V,
              biases=True, device=torch.device("cpu"))
    rows = [tok.tokenize_text("[SMILES]" + s + "[STOP]", pad=False) for s in SMILES]
    T = max(len(r) for r in rows)
    tokens = torch.full((len(rows), T), tok.pad_token, dtype=torch.long)
    for i, r in enumerate(rows):
        tokens[i, : len(r)] = torch.tensor(r)
    x_tok = torch.randn(5, D, generator=torch.Generator().manual_seed(7))
    out = {"n_seq": np.int64(N_SEQ), "tokens": tokens.numpy(), "token_head.in": x_tok.numpy()}
    calls = []
    xformer = None     # one transformer for the three variants (w.xformer.*), the heads per variant (<variant>.w.*)
    for vi, variant in enumerate(VARIANTS):
        torch.manual_seed(100 + vi)
        model = COATI_Smiles_Inference(n_seq=N_SEQ, enc_to_coati=variant, **kw)
        g = torch.Generator().manual_seed(200 + vi)
        with torch.no_grad():
            for name, p in model.named_parameters():
                if p.dim() == 1 and (".ln_" in name or name.endswith("coati.0.weight") or name.endswith("coati.0.bias") or ".net.0." in name):
                    p.copy_((1.0 if name.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
        if xformer is None:
            xformer = {k: v.clone() for k, v in model.state_dict().items() if k.startswith("xformer.") and not k.endswith(".attn.bias")}
            xformer["xformer.lm_head.weight"][tok.stop_token] *= STOP_SCALE   # rows that stop after a few tokens, not at once
            out.update({f"w.{k}": v.numpy() for k, v in xformer.items()})
        model.load_state_dict(xformer, strict=False)
        model.eval()
        sd = model.state_dict()
        out[f"{variant}.keys"] = np.array(list(sd.keys()))
        for k, v in sd.items():
            if not k.startswith("xformer."):
                out[f"{variant}.w.{k}"] = v.numpy()
        with torch.no_grad():
            h = model.encode_tokens(tokens, tok)
            out[f"{variant}.encode"] = h.numpy()
            out[f"{variant}.token_head"] = model.coati_to_token(x_tok).numpy()
            # ---- hcoati_to_2d_batch (k = 2, inv_temp = 1e4) ----
            hook = model.xformer.lm_head.register_forward_hook(lambda mod, inp, o: calls.append(o.detach().clone()))
            calls.clear()
            torch.manual_seed(300 + vi)
            _, gen = model.hcoati_to_2d_batch(h.clone(), tok, k=2, inv_temp=1e4, return_tokens=True)
            hook.remove()
            gen = torch.tensor(gen, dtype=torch.long)
            marg = np.stack([_margins(lg[:, -1]) for lg in calls], 1)
            out[f"{variant}.batch.tokens"] = gen.numpy()
            out[f"{variant}.batch.margin"] = marg.astype(np.float32)
            # ---- hcoati_to_2d (k = 1) on the wide copy ----
            wide = COATI_Smiles_Inference(n_seq=2 * N_SEQ, enc_to_coati=variant, **kw)
            wide.load_state_dict({k: v for k, v in sd.items() if not k.endswith(".attn.bias")}, strict=False)
            wide.eval()
            wide.xformer.lm_head.register_forward_hook(lambda mod, inp, o: calls.append(o.detach().clone()))
            for name, x in (("row", h[2:3].clone()), ("vec", h[3].clone())):
                calls.clear()
                try:
                    wide.hcoati_to_2d(x, tok, k=1)
                except RuntimeError:
                    pass
                prefix = tok.tokenize_text("[CLIP][UNK][SMILES]", pad=False)
                got = prefix + [int(torch.argmax(lg[0, -1])) for lg in calls]
                n = min(len(got), N_SEQ)
                row = np.zeros(N_SEQ, dtype=np.int64)
                row[:n] = got[:n]
                m = np.zeros(N_SEQ, dtype=np.float32)
                for i, lg in enumerate(calls):
                    if len(prefix) + i < N_SEQ:
                        m[len(prefix) + i] = _margins(lg[0, -1:])[0]
                out.update({f"{variant}.{name}.in": x.numpy(), f"{variant}.{name}.tokens": row, f"{variant}.{name}.len": np.int64(n),
                            f"{variant}.{name}.stopped": np.bool_(tok.stop_token in got[:n]), f"{variant}.{name}.margin": m})
    np.savez_compressed(os.path.join(OUT, "coati2_golden.npz"), **out)


def verify():
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, GOLDEN_OUT=tmp), check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        x, y = np.load(os.path.join(tmp, "coati2_golden.npz")), np.load(os.path.join(HERE, "coati2_golden.npz"))
        ok = x.files == y.files and all(np.array_equal(x[k], y[k]) and x[k].dtype == y[k].dtype for k in x.files)
        print(("same     " if ok else "DIFFERENT") + " coati2_golden.npz")
        same_vocab = open(os.path.join(tmp, "coati2_vocab.json")).read() == open(os.path.join(HERE, "coati2_vocab.json")).read()
        print(("same     " if same_vocab else "DIFFERENT") + " coati2_vocab.json")
        return ok and same_vocab


if __name__ == "__main__":
    if "--verify" in sys.argv:
        sys.exit(0 if verify() else 1)
    main()
