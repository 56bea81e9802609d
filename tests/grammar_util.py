"""Shared by tests/test_grammar_cpu.py and tests/test_gpu_grammar.py: the real `may_closedparen` slice of
tests/golden/tokenizer_real.json (320 special + 2377 SMILES tokens, V = 2697: odd, so the kernel's vector tail is exercised), its
grammar, and states reached by random walks."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tokenizer_real.json")
_CACHE = {}


def fixture():
    if "g" not in _CACHE:
        with open(GOLDEN) as f:
            _CACHE["g"] = json.load(f)
    return _CACHE["g"]


def tokenizer():
    if "tk" not in _CACHE:
        from coati_amd.models.encoding.tokenizers import TrieTokenizer
        g = fixture()
        _CACHE["tk"] = TrieTokenizer(n_seq=g["n_seq"], smiles_tokens=g["smiles"], special_tokens=g["special"])
    return _CACHE["tk"]


def grammar():
    if "gr" not in _CACHE:
        from coati_amd.grammar import SmilesGrammar
        _CACHE["gr"] = SmilesGrammar.from_tokenizer(tokenizer())
    return _CACHE["gr"]


def text(tokens):
    """the SMILES text of a token list: special tokens dropped, ends at the first [STOP]"""
    tk = tokenizer()
    n_special = len(tk.special_tokens)
    out = []
    for t in tokens:
        if t == tk.stop_token:
            break
        if t >= n_special:
            out.append(tk.keys[t])
    return "".join(out)


def random_states(n, seed, max_len=12):
    """n states behind walks of 0 .. max_len tokens: every fourth walk draws uniformly among all SMILES tokens (most of these go dead),
    the others among the admitted ones (alive); every eighth state is then advanced by [STOP] (finished, and dead where something is
    still open), some by one to three `(` (open branches) and by `[` (inside a bracket atom: the table's
    second row)."""
    gr, tk = grammar(), tokenizer()
    rng = np.random.default_rng(seed)
    n_special = len(tk.special_tokens)
    out = []
    for i in range(n):
        length = int(rng.integers(0, max_len + 1))
        st = (0, 0, 0)
        for _ in range(length):
            if i % 4 == 0:
                st = gr.advance(st, int(rng.integers(n_special, gr.n_token)))
            else:
                ok = np.flatnonzero(gr.admitted(st, 40))
                ok = ok[ok != gr.stop_token]
                st = gr.advance(st, int(rng.choice(ok)))
        if i % 8 == 1:
            st = gr.advance(st, gr.stop_token)
        for _ in range({3: 1, 6: 2, 7: 3}.get(i % 8, 0)):
            st = gr.advance(st, tk.vocab["("])
        if i % 8 in (2, 5, 7):
            st = gr.advance(st, tk.vocab["["])
        out.append(st)
    return out
