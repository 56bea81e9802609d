"""
Golden vectors for generation (clip_e2e.py:744-770 complete_batch -> smiles_xformer.py:157-198 generate_topk_batch, :590-632
points_to_2d_batch, :465-501 points_to_2d and :503-542 hclip_to_2d -> smiles_xformer.py:215-270 generate_topk_with_inj), produced by
IMPORTING THE REFERENCE in the build container (stubs of gen_golden.py).

Model: the small model of gen_golden.py (d = 64, 2 + 2 layers, V = 48) with the weights of small_model_after3.npz.  Tokenizer: the
reference TrieTokenizer over tokenizer.json (43 ids; special ids as gen_golden.Tok) and EXTRA, five pieces that give the model's
ids 43..47 a string (the small model was trained on ids up to 47, and the reference's decode fails on an id it has no piece for),
n_seq = 24.  Greedy (k = 1): the reference's
draws are deterministic.  Recorded per method: the inputs, the token rows, the decoded strings and -- by a forward hook on
xformer.lm_head -- the logits each generated column was drawn from ([B, n_seq, V], zero for prompt columns), so that a test can
tell near-ties from real differences.

The reference's generate_topk_batch has quirks the engine deliberately does not copy: a [STOP] drawn over a
prompt position, a stop count of occurrences rather than rows, a prompt of n_seq tokens.  This script asserts that none of them
fires on its inputs.  generate_topk_with_inj raises when a sequence does not stop within n_seq positions (the small model's greedy
sequences rarely stop): those calls run on a copy of the model with a wider causal-mask buffer and only the first n_seq positions,
which the engine returns, are kept.  So the fixture pins only behaviour the two implementations share.

    python tests/golden/gen_golden_generation.py            # (re)write tests/golden/generation_golden.npz
    python tests/golden/gen_golden_generation.py --verify   # regenerate into a scratch directory and compare contents
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
EXTRA = ["[He]", "[Ne]", "[Ar]", "[Kr]", "[Xe]"]
PROMPTS = [
    "[SMILES]C",                              # 2 tokens: the shortest prompt sets the reference's first position
    "[SMILES]CC(=O)",
    "[SMILES]c1ccccc1N",
    "[SMILES]CC[SUFFIX]O[MIDDLE]",            # fill-in-middle
    "[SMILES]CCO[STOP]",                      # a prompt with [STOP]: pads behind it
    "[SMILES]N(C)C(=O)OCc1ccccc1Cl",
    "[SMILES]ClCC(=O)OCC(=O)OC1CC",           # 12 tokens
]


def main():
    import gen_golden as G   # inserts the stubs, imports the reference
    from coati.models.encoding.tokenizers.trie_tokenizer import TrieTokenizer
    ref_clip = G.ref_clip
    voc = json.load(open(os.path.join(HERE, "tokenizer.json")))
    tok = TrieTokenizer(n_seq=N_SEQ, smiles_tokens=voc["smiles"] + EXTRA, special_tokens=voc["special"])
    assert len(tok.keys) == G.SMALL["n_tok"]
    for k in ("pad_token", "stop_token", "smiles_token", "suffix_token", "middle_token", "unk_token", "clip_token"):
        assert getattr(tok, k) == getattr(G.Tok, k), k
    torch.manual_seed(0)
    model = ref_clip.e3gnn_smiles_clip_e2e(**G.SMALL, device=torch.device("cpu"))
    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(HERE, "small_model_after3.npz")).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(".attn.bias") for k in missing), (missing, unexpected)
    model.eval()
    V, E, stop = G.SMALL["n_tok"], G.SMALL["n_embd_common"], tok.stop_token

    calls = []
    model.xformer.lm_head.register_forward_hook(lambda mod, inp, out: calls.append(out.detach().clone()))

    out = dict(n_seq=np.int64(N_SEQ), prompts=np.array(PROMPTS), extra_tokens=np.array(EXTRA))
    with torch.no_grad():
        # ---- complete_batch ----
        rows = [tok.tokenize_text(p, pad=False) for p in PROMPTS]
        plen = [len(r) for r in rows]
        assert min(plen) == 2 and max(plen) == 12 and max(plen) < N_SEQ, plen
        calls.clear()
        strings = model.complete_batch(PROMPTS, tok, k=1)
        B, m = len(rows), min(plen)
        pred = torch.zeros(B, N_SEQ, V)
        drawn = []
        for i, lg in enumerate(calls):              # call i draws column m - 1 + i from position m - 2 + i
            idx = m - 2 + i
            pred[:, idx + 1] = lg[:, idx]
            drawn.append(torch.topk(lg[:, idx], 1, dim=1).indices[:, 0])
        toks = torch.tensor(_regen_batch(rows, drawn, m, tok.pad_token, stop))
        for b in range(B):   # no [STOP] drawn over a prompt position (the reference would then pad the row's first real draw)
            for i, d in enumerate(drawn):
                assert not (m + i < plen[b] and int(d[b]) == stop), ("stop drawn over a prompt position", b, m + i)
        for b, r in enumerate(toks.tolist()):
            assert r[: plen[b]] == rows[b]                        # prompts verbatim
            assert r.count(stop) <= 1                             # stop occurrences == stopped rows
        out.update({"complete.tokens": toks, "complete.plen": np.array(plen), "complete.strings": np.array(strings),
                    "complete.logits": pred})
        # the same call with the reference's other decode flags (keep_special, no de_fim): the strings only
        out["complete.strings_special"] = np.array(model.complete_batch(PROMPTS, tok, k=1, keep_special=True, de_fim=False))

        # ---- points_to_2d_batch / points_to_2d ----
        _, _, atoms, coords = G.synth_batch(4, 16, 8, 48, seed=21, bad_row=False, far_atom=False)
        out.update({"points.atoms": atoms, "points.coords": coords})
        calls.clear()
        strings = model.points_to_2d_batch(atoms, coords, tok, k=1, keep_special=True)
        prefix = tok.tokenize_text("[CLIP][UNK][SMILES]", pad=False)
        pred = torch.zeros(atoms.shape[0], N_SEQ, V)
        gen = []
        for i, lg in enumerate(calls):
            pred[:, len(prefix) + i] = lg[:, -1]
            gen.append(torch.topk(lg[:, -1], 1, dim=1).indices[:, 0])
        out.update({"points_batch.strings": np.array(strings), "points_batch.logits": pred, "points_batch.prefix": np.array(prefix)})
        out["points_batch.tokens"] = torch.tensor(_regen_inj_batch(prefix, gen, stop, tok.pad_token, N_SEQ))
        # ---- points_to_2d and hclip_to_2d ([1, E]: the row is injected; [E]: its first channel, a scalar over all C) ----
        # generate_topk_with_inj raises on a sequence that has not stopped within n_seq positions (its causal-mask buffer is n_seq
        # wide); the engine returns those n_seq positions.  The one-sequence calls therefore run on a copy of the model with a
        # 2 * n_seq buffer (same weights; the rotary tables of the first n_seq positions are the same), the fixture keeps the
        # first n_seq positions, and the decoded string only of a sequence that stopped within them.
        wide = ref_clip.e3gnn_smiles_clip_e2e(**dict(G.SMALL, n_seq=2 * N_SEQ), device=torch.device("cpu"))
        wide.load_state_dict(sd, strict=False)
        wide.eval()
        wide.xformer.lm_head.register_forward_hook(lambda mod, inp, out: calls.append(out.detach().clone()))
        for i in range(2):
            r = _one(wide, calls, lambda: wide.points_to_2d(atoms[i:i + 1], coords[i:i + 1], tok, k=1),
                     tok.tokenize_text("[CLIP][UNK][SMILES][SUFFIX][MIDDLE]", pad=False))
            out.update(_single(f"points.{i}", *r, V, stop))
        h = torch.randn(2, E, generator=torch.Generator().manual_seed(5))
        out["hclip.in"] = h
        for name, x, sfx in (("hclip.row", h[0:1].clone(), False), ("hclip.vec", h[1].clone(), False),
                             ("hclip.row_suffix", h[0:1].clone(), True)):
            r = _one(wide, calls, lambda: wide.hclip_to_2d(x, tok, k=1, do_suffix=sfx),
                     tok.tokenize_text("[CLIP][UNK][SMILES]" + ("[SUFFIX][MIDDLE]" if sfx else ""), pad=False))
            out.update(_single(name, *r, V, stop))
    np.savez_compressed(os.path.join(OUT, "generation_golden.npz"), **G.npify(out))


def _regen_batch(rows, drawn, m, pad, stop):
    """the reference's final current_t from its draws (the loop of smiles_xformer.py:183-198, with the checks above)"""
    B = len(rows)
    cur = [[0] * N_SEQ for _ in range(B)]
    for b, r in enumerate(rows):
        cur[b][: len(r)] = r
    stopped = set()
    for i, d in enumerate(drawn):
        col = m - 1 + i
        for b in range(B):
            if col >= len(rows[b]):
                cur[b][col] = pad if b in stopped else int(d[b])
        stopped = {b for b in range(B) if stop in cur[b]}
    return cur


def _regen_inj_batch(prefix, gen, stop, pad, n_seq):
    """generate_top_k_with_inj_batch's token rows (smiles_xformer.py:294-351) from its draws"""
    B = gen[0].shape[0]
    rows = [list(prefix) for _ in range(B)]
    stopped = set()
    for d in gen:
        for b in range(B):
            rows[b].append(pad if b in stopped else int(d[b]))
        stopped = {b for b in range(B) if stop in rows[b][len(prefix):]}
    for b in range(B):
        if b not in stopped:
            rows[b][-1] = stop
    assert all(len(r) <= n_seq for r in rows)
    return rows


def _one(model, calls, fn, prefix):
    """(tokens, string or None, lm_head outputs) of the one generate_topk_with_inj call fn makes.  Where the call raises (the
    sequence outgrew the causal-mask buffer), the tokens are the prefix + the greedy draws of the forwards that ran."""
    calls.clear()
    try:
        s = fn()
    except RuntimeError:
        s = None
    got = list(prefix) + [int(torch.argmax(lg[0, -1])) for lg in calls]
    return got, s, list(calls)


def _single(name, tokens, string, calls, V, stop):
    """one generate_topk_with_inj call (on the wide model): its first n_seq positions, the logits they were drawn from, and the
    decoded string when the sequence stopped within them"""
    n_gen = len(calls)
    p = len(tokens) - n_gen
    n = min(len(tokens), N_SEQ)
    pred = torch.zeros(1, N_SEQ, V)
    for i, lg in enumerate(calls):
        if p + i < N_SEQ:
            pred[0, p + i] = lg[0, -1]
    row = torch.zeros(1, N_SEQ, dtype=torch.long)
    row[0, :n] = torch.tensor(tokens[:n])
    stopped = stop in tokens[:n]
    assert not stopped or string is not None
    return {f"{name}.tokens": row, f"{name}.len": np.int64(n), f"{name}.plen": np.int64(p), f"{name}.stopped": np.bool_(stopped),
            f"{name}.string": np.array(string if stopped else ""), f"{name}.logits": pred}


def verify():
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, GOLDEN_OUT=tmp), check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        x, y = np.load(os.path.join(tmp, "generation_golden.npz")), np.load(os.path.join(HERE, "generation_golden.npz"))
        ok = x.files == y.files and all(np.array_equal(x[k], y[k]) and x[k].dtype == y[k].dtype for k in x.files)
        print(("same     " if ok else "DIFFERENT") + " generation_golden.npz")
        return ok


if __name__ == "__main__":
    if "--verify" in sys.argv:
        sys.exit(0 if verify() else 1)
    main()
