"""
Golden vectors for the likelihood's gradient w.r.t. the injected embedding: autograd through the reference's
e3gnn_smiles_clip_e2e.hclip_and_tokens_to_likelihood (clip_e2e.py:634-665), produced by IMPORTING THE REFERENCE in the build container
(stubs of gen_golden.py).

Small part: the small model of gen_golden.py with the weights of small_model_after3.npz, the TrieTokenizer of tokenizer.json and the six
(hclip_in, hclip_smiles) rows of likelihood_golden.npz.  Per row: nll, dh = d nll / d hclip from autograd, the central difference of nll
along dh / |dh| (eps 1e-2, evaluated in float64; it equals |dh| up to the difference's own error), and the NLLs of ten plain gradient-descent steps
h <- h - 20 dh (entry 0 = the start).

Grande part: the grande_closed architecture with the weights of oracle.coati_oracle.init_params(cfg, seed = 16) (not stored: per-parameter
checksums, as in grande_golden.npz), 16 rows [CLIP][UNK][SMILES][SUFFIX][MIDDLE] + a random body of 8..57 ids + [STOP], targets masked
as clip_e2e.py:647-654 does, a seeded hclip [16, 256].  The reference's method takes one row per call: every row runs unpadded through
forward_with_replacement(point_clip_to_special_tokens(h)).  Stored: tokens / y_next (padded with [PAD] / -1), hclip, nll, dh, the
central difference.

    python tests/golden/gen_golden_score_grad.py            # (re)write tests/golden/score_grad_golden.npz  (under a minute of CPU)
    python tests/golden/gen_golden_score_grad.py --verify   # regenerate into a scratch directory and compare contents
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

GRANDE = dict(n_layer_e3gnn=5, n_layer_xformer=16, n_hidden_xformer=256, n_hidden_e3nn=256, n_embd_common=256, n_head=16,
              n_seq=250, n_tok=10322)
SEED = 16
EPS = 1e-2
STEP, N_DESCENT = 20.0, 10
B_GRANDE, BODY_LO, BODY_HI, FIRST_BODY_ID = 16, 8, 57, 1596


def nll_and_grad(fn, h):
    """fn(h [E]) -> nll (0-dim); returns (nll, d nll / d h) from autograd"""
    h = h.detach().clone().requires_grad_(True)
    nll = fn(h)
    (g,) = torch.autograd.grad(nll, h)
    return nll.detach(), g


def central_difference(fn, h, g):
    """along g / |g|, with the model and h in float64: in float32 the difference of two NLLs of a few hundred loses 4e-3 of |g| to their
    rounding alone (`fn` reads the model it is called with through `fn.model`, which is switched to float64 for the two calls)"""
    h, g = h.double(), g.double()
    u = g / g.norm()
    fn.model.double()
    try:
        with torch.no_grad():
            return (fn(h + EPS * u) - fn(h - EPS * u)) / (2 * EPS)
    finally:
        fn.model.float()


def main():
    import gen_golden as G   # inserts the stubs, imports the reference
    from coati.models.encoding.tokenizers.trie_tokenizer import TrieTokenizer
    from oracle import coati_oracle as O
    ref_clip = G.ref_clip
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    out = dict(eps=np.float64(EPS), step=np.float64(STEP))

    # ---- small model, the six rows of likelihood_golden.npz ----------------------------------------------------------------
    lk = np.load(os.path.join(HERE, "likelihood_golden.npz"))
    voc = json.load(open(os.path.join(HERE, "tokenizer.json")))
    tok = TrieTokenizer(n_seq=int(lk["n_seq"]), smiles_tokens=voc["smiles"], special_tokens=voc["special"])
    torch.manual_seed(0)
    model = ref_clip.e3gnn_smiles_clip_e2e(**G.SMALL, device=torch.device("cpu"))
    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(HERE, "small_model_after3.npz")).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(".attn.bias") for k in missing), (missing, unexpected)
    model.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    hclip = torch.from_numpy(lk["hclip_in"])
    smiles = [str(s) for s in lk["hclip_smiles"]]
    nll, dh, cd, traj = [], [], [], []
    for h, smi in zip(hclip, smiles):
        fn = lambda x, smi=smi: model.hclip_and_tokens_to_likelihood(x, smi, tok)[0]   # noqa: E731
        fn.model = model
        n, g = nll_and_grad(fn, h)
        assert abs(float(n) - float(lk[f"hclip.{len(nll)}.nll"][0])) <= 1e-5 * abs(float(n))
        nll.append(n); dh.append(g); cd.append(central_difference(fn, h, g))
        t, x = [n], h.clone()
        for _ in range(N_DESCENT):
            _, gx = nll_and_grad(fn, x)
            x = x - STEP * gx
            with torch.no_grad():
                t.append(fn(x))
        traj.append(torch.stack(t))
    out.update({"small.smiles": np.array(smiles), "small.hclip": hclip, "small.nll": torch.stack(nll), "small.dh": torch.stack(dh),
                "small.cd": torch.stack(cd), "small.traj": torch.stack(traj)})

    # ---- grande shape ------------------------------------------------------------------------------------------------------
    ocfg = O.OracleConfig(**GRANDE)
    P = O.init_params(ocfg, seed=SEED)
    torch.manual_seed(0)
    big = ref_clip.e3gnn_smiles_clip_e2e(biases=True, torch_emb=False, residual=False, norm_clips=True, norm_embed=False,
                                         token_mlp=True, **GRANDE)
    missing, unexpected = big.load_state_dict(P, strict=False)
    assert not unexpected and all(k.endswith(".attn.bias") for k in missing), (missing, unexpected)
    big.eval()
    names = [n for n, _ in big.named_parameters()]
    for p in big.parameters():
        p.requires_grad_(False)
    tz = G.Tok(GRANDE["n_tok"], GRANDE["n_seq"])
    gen = torch.Generator().manual_seed(1616)
    T = 5 + BODY_HI + 1
    tokens = torch.full((B_GRANDE, T), tz.pad_token, dtype=torch.long)
    for b in range(B_GRANDE):
        n_body = int(torch.randint(BODY_LO, BODY_HI + 1, (1,), generator=gen))
        body = torch.randint(FIRST_BODY_ID, GRANDE["n_tok"], (n_body,), generator=gen)
        row = torch.cat([torch.tensor([tz.clip_token, tz.unk_token, tz.smiles_token, tz.suffix_token, tz.middle_token]), body,
                         torch.tensor([tz.stop_token])])
        tokens[b, :len(row)] = row
    y_next = torch.zeros_like(tokens)
    y_next[:, :-1] = tokens[:, 1:]
    for t in (tz.clip_token, tz.pad_token, tz.smiles_token, tz.unk_token, tz.suffix_token, tz.middle_token):
        y_next[y_next == t] = -1
    hg = torch.randn(B_GRANDE, GRANDE["n_embd_common"], generator=gen)
    nll, dh, cd = [], [], []
    for b in range(B_GRANDE):
        L = int((tokens[b] != tz.pad_token).sum())
        tk, yn = tokens[b:b + 1, :L], y_next[b, :L]

        def fn(x, tk=tk, yn=yn):
            logits = big.xformer.forward_with_replacement(tk, big.point_clip_to_special_tokens(x.unsqueeze(0)), tz)
            return torch.nn.functional.cross_entropy(logits[0], yn, ignore_index=-1, reduction="sum")
        fn.model = big
        n, g = nll_and_grad(fn, hg[b])
        nll.append(n); dh.append(g); cd.append(central_difference(fn, hg[b], g))
    out.update({"grande.tokens": tokens, "grande.y_next": y_next, "grande.hclip": hg, "grande.nll": torch.stack(nll),
                "grande.dh": torch.stack(dh), "grande.cd": torch.stack(cd), "grande.seed": np.array(SEED),
                "grande.names": np.array(names), "grande.wsum": np.array([float(P[n].double().sum()) for n in names]),
                "grande.wabs": np.array([float(P[n].double().abs().sum()) for n in names])})
    np.savez_compressed(os.path.join(OUT, "score_grad_golden.npz"), **G.npify(out))
    print("written", os.path.join(OUT, "score_grad_golden.npz"))


def verify():
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, GOLDEN_OUT=tmp), check=True,
                       stdout=subprocess.DEVNULL)
        x, y = np.load(os.path.join(tmp, "score_grad_golden.npz")), np.load(os.path.join(HERE, "score_grad_golden.npz"))
        ok = x.files == y.files
        for k in x.files:
            if x[k].dtype.kind == "f":   # (CPU sums re-associate across thread counts: 1e-5 of scale, as gen_golden_grande.py)
                sc = max(float(np.abs(y[k]).max()), 1e-30)
                same = x[k].shape == y[k].shape and float(np.abs(x[k] - y[k]).max()) <= 1e-5 * sc
            else:
                same = np.array_equal(x[k], y[k])
            if not same:
                print("DIFFERENT", k)
                ok = False
        print("score_grad_golden.npz", "same" if ok else "DIFFERENT")
        return ok


if __name__ == "__main__":
    if "--verify" in sys.argv:
        sys.exit(0 if verify() else 1)
    main()
