"""Syntax-constrained decoding, host side (no GPU): include/coati_grammar.h parses against coati_hip.h and the library exports what it
declares, the entry refuses bad arguments with a code before any device call, hand-checked table entries of the real vocabulary slice,
the token-level walk against the string-level balanced() on the tokenizer fixture's rows, and the never-empty invariant."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import grammar_util as U  # noqa: E402

SAMPLE, END_INBR, NEUTRAL = 1, 2, 4
INBR, DEAD, FINISHED = 1, 2, 4


# ---- the fourth header ------------------------------------------------------------------------------------------------------
def test_grammar_header_parses_into_a_table_of_its_own():
    from coati_amd import _abi, _lib, build
    assert sorted(_lib.GRAMMAR_PROTOTYPES) == ["coati_grammar_step"]
    for other in (_lib.PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.SEARCH_PROTOTYPES):
        assert not set(_lib.GRAMMAR_PROTOTYPES) & set(other)
    assert len(_lib.PROTOTYPES) == 121 and _lib.ABI_VERSION == 5 and len(_lib.BEAM_PROTOTYPES) == 4 and len(_lib.SEARCH_PROTOTYPES) == 2
    I, P, L = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert _lib.GRAMMAR_PROTOTYPES["coati_grammar_step"] == (I, [P, L, I, I, P, P, P, P, P, I, I, P])
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.GRAMMAR_HEADER) as f:
        text = f.read()
    again = _abi.parse(text, guard="COATI_GRAMMAR_H", name="coati_grammar.h", base=base)
    assert again.prototypes == _lib.GRAMMAR_PROTOTYPES and again.version == 5 and not again.experimental
    marker = "#endif /* COATI_GRAMMAR_H */"
    with pytest.raises(ValueError, match=r"coati_grammar\.h: coati_gemm_nt is already declared in coati_hip\.h"):
        _abi.parse(text.replace(marker, "int coati_gemm_nt(int a);\n" + marker), guard="COATI_GRAMMAR_H", name="coati_grammar.h", base=base)


def test_library_exports_the_grammar_entry():
    from coati_amd import _lib, build
    l = _lib.lib()
    assert l.coati_abi_version() == 5
    for name, (restype, argtypes) in _lib.GRAMMAR_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert "coati_grammar_step" not in _lib.exported_symbols()
    assert "grammar.hip" in build.HIP_UNITS
    # exactly what the header declares: no other coati_grammar* symbol in the library
    with open(build.LIB, "rb") as f:
        blob = f.read()
    import re
    assert set(re.findall(rb"coati_grammar\w*", blob)) == {b"coati_grammar_step"}


def test_grammar_step_refuses_bad_arguments_with_a_code():
    """decided on the host before any device call: the pointers are host buffers that a refusal never looks at"""
    from coati_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def step(logits=p, ldl=10, B=2, V=10, table=p, sin=p, sout=p, tok=None, parent=None, remaining=3, stop=1):
        rc = l.coati_grammar_step(logits, ldl, B, V, table, sin, sout, tok, parent, remaining, stop, None)
        return rc, l.coati_last_error().decode()

    for kw in (dict(logits=None), dict(table=None), dict(sin=None), dict(sout=None)):
        rc, msg = step(**kw)
        assert rc < 0 and "null" in msg, (kw, rc, msg)
    for kw, word in ((dict(B=0), "B=0"), (dict(V=0), "V=0"), (dict(ldl=9), "ldl=9"), (dict(remaining=0), "remaining=0"),
                     (dict(stop=-1), "stop_token=-1"), (dict(stop=10), "stop_token=10")):
        rc, msg = step(**kw)
        assert rc < 0 and word in msg, (kw, rc, msg)
    rc, msg = step(parent=p)                 # parent needs ping-pong buffers
    assert rc < 0 and "ping-pong" in msg, (rc, msg)


# ---- the table --------------------------------------------------------------------------------------------------------------
def test_hand_checked_entries():
    """(need, delta, toggle, flags) from both entry states; flags: 1 sampleable, 2 ends inside a bracket, 4 neutral"""
    gr, tk = U.grammar(), U.tokenizer()
    assert gr.n_token == 2697 and gr.stop_token == tk.stop_token == 1
    e = lambda s, inbr: gr.entry(tk.vocab[s], inbr)   # noqa: E731
    assert e("c1ccccc1", 0) == (0, 0, 0, SAMPLE)                     # opens and closes ring 1
    assert e("c1ccccc1", 1) == (0, 0, 0, SAMPLE | END_INBR)          # inside a bracket the digits flip nothing, the bracket stays open
    assert e("(=O)c1", 0) == (0, 0, 1 << 1, SAMPLE)
    assert e("(=O)c1", 1) == (0, 0, 0, 0)                            # `(` inside a bracket: invalid
    assert e(")", 0) == (1, -1, 0, SAMPLE) and e(")", 1) == (0, 0, 0, 0)
    assert e("(", 0) == (0, 1, 0, SAMPLE) and e("(", 1) == (0, 0, 0, 0)
    assert e("3", 0) == (0, 0, 1 << 3, SAMPLE) and e("3", 1) == (0, 0, 0, SAMPLE | END_INBR)
    assert e("[C@@H](C)C", 0) == (0, 0, 0, SAMPLE) and e("[C@@H](C)C", 1) == (0, 0, 0, 0)
    assert e("[", 0) == (0, 0, 0, SAMPLE | END_INBR) and e("[", 1) == (0, 0, 0, 0)
    assert e("]", 0) == (0, 0, 0, 0) and e("]", 1) == (0, 0, 0, SAMPLE)
    assert e("%", 0) == (0, 0, 0, 0) and e("%", 1) == (0, 0, 0, 0)   # never sampled; forced, it kills the row
    for s in ("[PAD]", "[SMILES]", "[SET]", "[STOP]", "[UNK]"):
        assert e(s, 0) == e(s, 1) == (0, 0, 0, NEUTRAL), s
    # the packed 8-byte entry: need | delta << 8 | toggle << 16 | flags << 32, little-endian
    t = tk.vocab[")"]
    assert int(gr.table[0, t]) == 1 | (0xff << 8) | (SAMPLE << 32) and gr.table.shape == (2, 2697)
    assert int(gr.table[0, tk.vocab["(=O)c1"]]) == (2 << 16) | (SAMPLE << 32)


def test_advance_rules():
    gr, tk = U.grammar(), U.tokenizer()
    v = tk.vocab
    s = gr.walk([v["[SMILES]"], v["c1"], v["cc"], v["("]])
    assert s == (1, 1 << 1, 0) and gr.walk([v["["]]) == (0, 0, INBR)
    assert gr.advance(s, v["[PAD]"]) == s                                        # neutral
    assert gr.advance(s, 1) == (1, 2, FINISHED | DEAD)                           # [STOP] with something open
    assert gr.advance((0, 0, 0), 1) == (0, 0, FINISHED)
    assert gr.advance((0, 0, 0), v[")"]) == (0, 0, DEAD) and gr.advance((0, 0, 0), v["%"]) == (0, 0, DEAD)
    assert gr.advance((0, 0, DEAD), v["C"]) == (0, 0, DEAD) and gr.advance((0, 0, FINISHED), v["("]) == (0, 0, FINISHED)
    assert gr.advance((0, 0, 0), v["("], remaining=2) == (1, 0, 0)               # `)` and [STOP] still fit
    assert gr.advance((0, 0, 0), v["("], remaining=1) == (1, 0, DEAD)            # only [STOP] fits
    adm = gr.admitted((0, 0, 0), 2)
    assert adm[1] and adm[v["C"]] and not adm[v["("]] and not adm[v["c1"]] and adm[v["c1ccccc1"]] and not adm[v["[PAD]"]]
    adm = gr.admitted((1, 0, 0), 2)
    assert adm.nonzero()[0].tolist() == [v[")"]]
    assert gr.admitted((0, 0, 0), 1).nonzero()[0].tolist() == [1]
    assert gr.admitted((0, 0, INBR), 3)[v["]"]] and not gr.admitted((0, 0, INBR), 3)[1]


def test_from_tokenizer_refusals():
    from coati_amd.grammar import SmilesGrammar
    from coati_amd.models.encoding.tokenizers import TrieTokenizer
    from coati_amd.models.simple_coati2.trie_tokenizer import TrieTokenizer as Trie2
    g = U.fixture()
    for drop in (")", "]", "7"):
        tk = TrieTokenizer(n_seq=64, smiles_tokens=[t for t in g["smiles"] if t != drop], special_tokens=g["special"])
        with pytest.raises(ValueError, match="lacks the single-symbol tokens"):
            SmilesGrammar.from_tokenizer(tk)
    for tok, word in (("(" * 300, "need 0 / delta 300"), ("C" + ")" * 130, "need 130 / delta -130"), (")" * 256 + "(" * 256, "need 256")):
        tk = TrieTokenizer(n_seq=64, smiles_tokens=g["smiles"] + [tok], special_tokens=g["special"])
        with pytest.raises(ValueError, match=word):
            SmilesGrammar.from_tokenizer(tk)
    tk2 = Trie2(n_seq=64, smiles_tokens=g["smiles"], special_tokens=g["special"])     # the COATI2 tokenizer
    assert (SmilesGrammar.from_tokenizer(tk2).table == U.grammar().table).all()


# ---- walk against the string level --------------------------------------------------------------------------------------------
def test_walk_agrees_with_balanced_on_the_fixture_rows():
    from coati_amd.grammar import balanced, cost
    gr = U.grammar()
    seen = {(True, False): 0, (False, False): 0, (False, True): 0}
    for c in U.fixture()["cases"]:
        if c["result"][0] != "ok" or "%" in c["row"]:
            continue
        ids = c["result"][1]                                     # [SMILES] ... [STOP]
        ok, dead = balanced(c["row"], detail=True)
        s = gr.walk(ids[:-1])
        assert bool(s[2] & DEAD) == dead, (c["row"], s)
        assert (not s[2] & DEAD and cost(s) == 0) == ok == balanced(c["row"]), (c["row"], s)
        f = gr.walk(ids)                                         # with the [STOP]: finished, dead unless balanced
        assert bool(f[2] & FINISHED) or dead
        assert bool(f[2] & DEAD) == (not ok), (c["row"], f)
        seen[(ok, dead)] += 1
    assert min(seen.values()) >= 5, seen                         # balanced, open and broken rows are all there
    assert balanced("") and balanced("C[NH3+]") and balanced("[13C]1CC1") and not balanced("C1CC") and not balanced("C(")
    assert balanced("C)", detail=True) == (False, True) and balanced("C[N(]", detail=True) == (False, True)
    assert balanced("C]", detail=True) == (False, True) and balanced("C%10CC%10", detail=True) == (False, True)
    assert balanced("C[N", detail=True) == (False, False) and balanced("C1CC2", detail=True) == (False, False)


# ---- the never-empty invariant ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 3, 8, 24])
def test_random_admitted_walks_always_close(R):
    """2000 walks over the five budgets (400 each, fixed seeds): from the empty state, a uniformly random admitted token per draw; the
    admitted set is never empty, [STOP] comes within R draws, the string is balanced."""
    from coati_amd.grammar import balanced
    gr = U.grammar()
    rng = np.random.default_rng(1000 + R)
    lengths = []
    for _ in range(400):
        state, toks = (0, 0, 0), []
        for r in range(R, 0, -1):
            ok = np.flatnonzero(gr.admitted(state, r))
            assert len(ok) > 0, (state, r, toks)
            t = int(rng.choice(ok))
            toks.append(t)
            state = gr.advance(state, t, r - 1)
            assert not state[2] & DEAD, (state, toks)
            if t == gr.stop_token:
                break
        assert toks[-1] == gr.stop_token and state[2] == FINISHED and len(toks) <= R, (state, toks)
        assert balanced(U.text(toks)), U.text(toks)
        lengths.append(len(toks))
    assert max(lengths) == R or R > 8
