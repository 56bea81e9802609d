"""
Golden vectors for coati.generative (coati_purifications.py, coati_density.py) and the xformer logits (smiles_xformer.py:375-382,
426-454), produced by IMPORTING THE REFERENCE in the build container (stubs of gen_golden.py).

Model: the small model of gen_golden.py (d = 64, 2 + 2 layers, V = 48) with the weights of small_model_after3.npz.  Tokenizer: the
reference TrieTokenizer over tokenizer.json, n_seq = 24.  rdkit is stubbed with a deterministic rule (canon() below): a string holding
"X" (or empty) is invalid, the canonical form of s is min(s, reversed s) -- "CCO" and "OCC" share one --, and "x" is valid but not in
the vocabulary (it fails tokenization).  hclip_to_2d_batch / hclip_to_2d are replaced by scripted lists: no sampling.  Recorded:
embed_smiles, embed_smiles_batch, purify_vector (with the canonical strings it encoded), force_decode_valid(_batch), xformer.forward /
forward_with_replacement logits, and estimate_density_batchwise's scale_tril per batch with the embeddings it saw.

    python tests/golden/gen_golden_generative.py            # (re)write tests/golden/generative_golden.npz
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("GOLDEN_OUT", HERE)
sys.path.insert(0, HERE)

N_SEQ = 24
EMBED = ["OCC", "CCO", "C=CC#N", "NCCO", "FC(F)(F)S", "CC(=O)O"]
BATCH = ["CCO", "c1ccccc1N", "C=CC#N", "ClCCBr", "CC(=O)O", "N(C)C(=O)OC", "OC(=O)c1ccccc1"]
# purify_vector decodes (n_rep = 8): invalid ("X"), untokenizable ("x"), two raw forms of one canonical string, repeats
PURIFY = [
    ["OCC", "CX", "CCO", "CxC", "CCN", "OCC", "", "NCC"],
    ["CX", "XC", "", "CX", "CxC", "X", "CXC", "xC"],             # nothing kept: V returned
]
FORCE_ONE = [["CX", "", "xX", "OCC", "CCN"], ["CX", "X", "XX"]]  # force_decode_valid: first valid raw string; "C" after 3 attempts
# force_decode_valid_batch (batch_size = 6): attempt 1 has nothing valid, attempt 2 a 2-2 tie (CCO first in decode order)
FORCE_BATCH = [[["CX", "X", "", "XC", "CXX", "X"], ["NCC", "OCC", "CCN", "CCO", "CX", "C"]],
               [["CX"] * 6, ["X"] * 6]]
DENSITY = ["CCO", "OCC", "CCN", "C=CC#N", "CX", "CC(=O)O", "NCCO", "CxC", "FC(F)(F)S", "CCOC", "OCCN", "C#N"]
LOGIT_ROWS = ["[CLIP][UNK][SMILES]CCO[STOP]", "[SMILES]C=CC#N[STOP]", "[CLIP][UNK][SMILES]NCC(=O)O[STOP]"]


def canon(s):
    if not s or "X" in s:
        return None
    return min(s, s[::-1])


def main():
    import gen_golden as G   # inserts the stubs, imports the reference
    from rdkit import Chem
    Chem.MolFromSmiles = lambda s: None if canon(s) is None else ("mol", s)
    Chem.MolToSmiles = lambda m: canon(m[1])
    from coati.models.encoding.tokenizers.trie_tokenizer import TrieTokenizer
    from coati.generative import coati_purifications as RP, coati_density as RD
    ref_clip = G.ref_clip
    voc = json.load(open(os.path.join(HERE, "tokenizer.json")))
    tok = TrieTokenizer(n_seq=N_SEQ, smiles_tokens=voc["smiles"], special_tokens=voc["special"])
    torch.manual_seed(0)
    model = ref_clip.e3gnn_smiles_clip_e2e(**G.SMALL, device=torch.device("cpu"))
    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(HERE, "small_model_after3.npz")).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(".attn.bias") for k in missing), (missing, unexpected)
    model.eval()
    E = G.SMALL["n_embd_common"]
    gen = torch.Generator().manual_seed(11)
    V = torch.randn(2, E, generator=gen)

    rec, script = {}, []
    real_enc = ref_clip.e3gnn_smiles_clip_e2e.encode_tokens

    def enc(self, token_indices, tokenizer):
        rec.setdefault("tokens", []).append(token_indices.clone())
        out = real_enc(self, token_indices, tokenizer)
        rec.setdefault("embeds", []).append(out.detach().clone())
        return out

    def scripted_batch(self, h, tokenizer, *a, **k):
        item = script.pop(0)
        if isinstance(item, Exception):
            raise item
        assert len(item) == h.shape[0], (len(item), h.shape)
        return list(item)

    def scripted_one(self, h, tokenizer, *a, **k):
        return script.pop(0)

    ref_clip.e3gnn_smiles_clip_e2e.encode_tokens = enc
    ref_clip.e3gnn_smiles_clip_e2e.hclip_to_2d_batch = scripted_batch
    ref_clip.e3gnn_smiles_clip_e2e.hclip_to_2d = scripted_one
    out = dict(n_seq=np.int64(N_SEQ), V=V, embed_smiles_in=np.array(EMBED), batch_in=np.array(BATCH))
    with torch.no_grad():
        out["embed_smiles"] = torch.stack([RP.embed_smiles(s, model, tok) for s in EMBED])
        out["embed_smiles_batch"] = RP.embed_smiles_batch(BATCH, model, tok)
        for i, strings in enumerate(PURIFY):
            rec.clear()
            script[:] = [strings]
            out[f"purify.{i}.in"] = np.array(strings)
            out[f"purify.{i}.out"] = RP.purify_vector(V[i], model, tok, n_rep=len(strings))
            toks = rec.get("tokens", [])
            out[f"purify.{i}.encoded"] = np.array([tok.decode(r.tolist(), special=False) for r in toks[0]] if toks else [], dtype=str)
        script[:] = [RuntimeError("decoder failure")]
        out["purify.raise.out"] = RP.purify_vector(V[0], model, tok, n_rep=8)
        for i, strings in enumerate(FORCE_ONE):
            script[:] = list(strings)
            out[f"force_one.{i}.in"] = np.array(strings)
            out[f"force_one.{i}.out"] = np.array(RP.force_decode_valid(V[0], model, tok, max_attempts=len(strings) if i else 2000))
            out[f"force_one.{i}.left"] = np.int64(len(script))
        for i, attempts in enumerate(FORCE_BATCH):
            script[:] = [list(a) for a in attempts]
            for j, a in enumerate(attempts):
                out[f"force_batch.{i}.in.{j}"] = np.array(a)
            out[f"force_batch.{i}.out"] = np.array(RP.force_decode_valid_batch(V[0], model, tok, batch_size=6, max_attempts=len(attempts)))
        # xformer logits: forward, and forward_with_replacement with the special token of V
        rows = [tok.tokenize_text(t, pad=True) for t in LOGIT_ROWS]
        idx = torch.tensor(rows, dtype=torch.long)
        out["logits.tokens"] = idx
        out["logits.forward"] = model.xformer.forward(idx)
        inj = model.point_clip_to_special_tokens(torch.cat([V, V[:1]]))
        out["logits.injection"] = inj
        out["logits.replacement"] = model.xformer.forward_with_replacement(idx, inj, tok)
    # estimate_density_batchwise: scale_tril of every batch's distribution and the embeddings it scored
    trils = []
    real_mvn = RD.MultivariateNormal

    def mvn(loc, scale_tril=None, **k):
        trils.append(scale_tril.detach().clone())
        return real_mvn(loc, scale_tril=scale_tril, **k)

    RD.MultivariateNormal = mvn
    rec.clear()
    res = RD.estimate_density_batchwise(DENSITY, model, tok, batch_size=4, epochs=2)
    RD.MultivariateNormal = real_mvn
    assert res is None
    out["density.in"] = np.array(DENSITY)
    out["density.scale_tril"] = torch.stack(trils)
    out["density.embeds"] = torch.cat(rec["embeds"])
    out["density.batch_rows"] = np.array([e.shape[0] for e in rec["embeds"]], dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "generative_golden.npz"), **G.npify(out))


if __name__ == "__main__":
    main()
