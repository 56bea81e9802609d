"""
Golden vectors for likelihood scoring (clip_e2e.py:333-347 _tokenize_smiles, :634-665 hclip_and_tokens_to_likelihood,
:667-742 batch_smiles_to_s2s_likelihood), produced by IMPORTING THE REFERENCE in the build container (stubs of gen_golden.py).

Model: the small model of gen_golden.py (d = 64, 2 + 2 layers, V = 48) with the weights of small_model_after3.npz.  Tokenizer: the
reference TrieTokenizer over the special + smiles vocabulary of tokenizer.json (43 ids; the special ids are gen_golden.Tok's), n_seq = 24.
Inputs: SMILES built from that vocabulary, one longer than n_seq - 5 tokens and one with a piece outside it (both False in the s2s
mask), and a seeded hclip [6, 64].  Recorded per method: the outputs, and -- by wrapping forward_with_replacement, encode_tokens and
torch.nn.functional.cross_entropy during the call -- the tokens, encoder tokens, targets and per-token cross-entropy it computed.

    python tests/golden/gen_golden_likelihood.py            # (re)write tests/golden/likelihood_golden.npz
    python tests/golden/gen_golden_likelihood.py --verify   # regenerate into a scratch directory and compare contents
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

N_SEQ = 24
SMILES = [
    "CC(=O)O", "c1ccccc1N", "CCO", "N(C)C(=O)OC", "c1cc[nH]c1", "CC[C@@H](N)C(=O)O", "ClCCBr", "OC(=O)c1ccccc1",
    "CN" * 10,                  # 20 tokens + [STOP] > n_seq - 5: too long for the s2s rows
    "CxC",                      # 'x' is not in the vocabulary
    "C=CC#N", "FC(F)(F)S", "c1ccccc1c1ccccc1",
]
HCLIP_SMILES = ["CC(=O)O", "c1ccccc1N", "CCO", "N(C)C(=O)OC", "ClCCBr", "OC(=O)c1ccccc1"]


def main():
    import gen_golden as G   # inserts the stubs, imports the reference
    from coati.models.encoding.tokenizers.trie_tokenizer import TrieTokenizer
    ref_clip, ref_sx = G.ref_clip, G.ref_sx
    voc = json.load(open(os.path.join(HERE, "tokenizer.json")))
    tok = TrieTokenizer(n_seq=N_SEQ, smiles_tokens=voc["smiles"], special_tokens=voc["special"])
    for k in ("pad_token", "stop_token", "smiles_token", "suffix_token", "middle_token", "unk_token", "clip_token"):
        assert getattr(tok, k) == getattr(G.Tok, k), k
    torch.manual_seed(0)
    model = ref_clip.e3gnn_smiles_clip_e2e(**G.SMALL, device=torch.device("cpu"))
    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(HERE, "small_model_after3.npz")).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(".attn.bias") for k in missing), (missing, unexpected)
    model.eval()
    hclip = torch.randn(len(HCLIP_SMILES), G.SMALL["n_embd_common"], generator=torch.Generator().manual_seed(7))

    rec = {}
    real_ce = torch.nn.functional.cross_entropy
    real_fwr = ref_sx.RotarySmilesTransformer.forward_with_replacement
    real_enc = ref_clip.e3gnn_smiles_clip_e2e.encode_tokens

    def ce(input, target, *a, **k):
        out = real_ce(input, target, *a, **k)
        rec["targets"], rec["ce"] = target.clone(), out.detach().clone()
        return out

    def fwr(self, idx, injection, tokenizer, *a, **k):
        rec["tokens"], rec["injection"] = idx.clone(), injection.detach().clone()
        return real_fwr(self, idx, injection, tokenizer, *a, **k)

    def enc(self, token_indices, tokenizer):
        rec["raw_tokens"] = token_indices.clone()
        out = real_enc(self, token_indices, tokenizer)
        rec["hclip"] = out.detach().clone()
        return out

    out = dict(smiles=np.array(SMILES), hclip_smiles=np.array(HCLIP_SMILES), hclip_in=hclip, n_seq=np.int64(N_SEQ))
    torch.nn.functional.cross_entropy = ce
    ref_sx.RotarySmilesTransformer.forward_with_replacement = fwr
    ref_clip.e3gnn_smiles_clip_e2e.encode_tokens = enc
    try:
        with torch.no_grad():
            # hclip_and_tokens_to_likelihood: one row per call (the reference's form); rows of different length, kept per row
            for i, (h, smi) in enumerate(zip(hclip, HCLIP_SMILES)):
                rec.clear()
                nll = model.hclip_and_tokens_to_likelihood(h, smi, tok)
                out.update({f"hclip.{i}.nll": nll, f"hclip.{i}.tokens": rec["tokens"], f"hclip.{i}.targets": rec["targets"],
                            f"hclip.{i}.ce": rec["ce"]})
            # batch_smiles_to_s2s_likelihood
            rec.clear()
            nll, mask = model.batch_smiles_to_s2s_likelihood(SMILES, tok)
            out.update({"s2s.nll": nll, "s2s.mask": mask, "s2s.raw_tokens": rec["raw_tokens"], "s2s.hclip": rec["hclip"],
                        "s2s.tokens": rec["tokens"], "s2s.targets": rec["targets"], "s2s.ce": rec["ce"]})
    finally:
        torch.nn.functional.cross_entropy = real_ce
        ref_sx.RotarySmilesTransformer.forward_with_replacement = real_fwr
        ref_clip.e3gnn_smiles_clip_e2e.encode_tokens = real_enc
    np.savez_compressed(os.path.join(OUT, "likelihood_golden.npz"), **G.npify(out))


def verify():
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, GOLDEN_OUT=tmp), check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        x, y = np.load(os.path.join(tmp, "likelihood_golden.npz")), np.load(os.path.join(HERE, "likelihood_golden.npz"))
        ok = x.files == y.files and all(np.array_equal(x[k], y[k]) and x[k].dtype == y[k].dtype for k in x.files)
        print(("same     " if ok else "DIFFERENT") + " likelihood_golden.npz")
        return ok


if __name__ == "__main__":
    if "--verify" in sys.argv:
        sys.exit(0 if verify() else 1)
    main()
