"""COATI2 (coati.models.simple_coati2) host-side pieces, no GPU: the import alias, the COATI2 tokenizer against the reference's ids
(tests/golden/coati2_vocab.json, written by gen_golden_coati2.py), the C ABI's new symbols, and the engine's COATI2 parameter table
in the reference's state_dict order."""
import ctypes
import json
import os
import pickle

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def _vocab():
    with open(os.path.join(GOLDEN, "coati2_vocab.json")) as f:
        return json.load(f)


def _tokenizer():
    from coati_amd.models.simple_coati2.trie_tokenizer import TrieTokenizer
    v = _vocab()
    return TrieTokenizer(n_seq=v["n_seq"], special_tokens=v["special_tokens"], smiles_tokens=v["smiles_tokens"])


def test_coati_alias_resolves_simple_coati2():
    import coati  # noqa: F401
    from coati.models.simple_coati2.io import load_coati2
    from coati.models.simple_coati2.transformer_only import COATI_Smiles_Inference, SwiGLU, SwiGLUResNet  # noqa: F401
    from coati.models.simple_coati2.trie_tokenizer import TrieTokenizer
    assert load_coati2.__module__ == "coati_amd.models.simple_coati2.io"
    assert COATI_Smiles_Inference.__module__ == "coati_amd.models.simple_coati2.transformer_only"
    assert TrieTokenizer.__module__ == "coati_amd.models.simple_coati2.trie_tokenizer"


def test_tokenizer_ids_match_reference():
    tok = _tokenizer()
    ids = _vocab()["ids"]
    for name, want in ids.items():
        assert getattr(tok, name) == want, name
    assert (tok.pad_token, tok.stop_token, tok.unk_token, tok.clip_token) == (31, 40, 44, 2)


def test_tokenizer_text_and_decode_match_reference():
    tok = _tokenizer()
    for case in _vocab()["cases"]:
        assert tok.tokenize_text(case["text"], pad=False) == case["ids"], case["text"]
        assert tok.decode(case["ids"]) == case["decode"], case["text"]
        assert tok.decode(case["ids"], special=False) == case["decode_plain"], case["text"]
    padded = tok.tokenize_text("[SMILES]CCO[STOP]")
    assert len(padded) == tok.n_seq and padded[-1] == tok.pad_token == 31


def test_tokenizer_requires_mask():
    from coati_amd.models.simple_coati2.trie_tokenizer import TrieTokenizer
    v = _vocab()
    special = [t for t in v["special_tokens"] if t != "[MASK]"]
    with pytest.raises(KeyError):
        TrieTokenizer(n_seq=v["n_seq"], special_tokens=special, smiles_tokens=v["smiles_tokens"])


def test_tokenizer_pickles():
    tok = _tokenizer()
    back = pickle.loads(pickle.dumps(tok))
    assert type(back) is type(tok)
    assert (back.mask_token, back.n_special, back.n_seq) == (tok.mask_token, tok.n_special, tok.n_seq)
    text = _vocab()["cases"][1]["text"]
    assert back.tokenize_text(text, pad=False) == tok.tokenize_text(text, pad=False)


def test_header_declares_and_library_exports_coati2_entries():
    from coati_amd import _lib
    l = _lib.lib()
    for name in ("coati_swiglu", "coati_engine_create_coati2", "coati_engine_token_head"):
        assert name in _lib.PROTOTYPES and _lib.PROTOTYPES[name][0] is ctypes.c_int, name
        assert hasattr(l, name), name
        assert name in _lib.exported_symbols()


def _layout(variant, **over):
    """(names, shapes) of the engine's COATI2 parameter table (host-only: creating an engine does not touch the device)"""
    from coati_amd import _lib
    from coati_amd.engine import ENC_TO_COATI
    l = _lib.lib()
    g = np.load(os.path.join(GOLDEN, "coati2_golden.npz"))
    V = int(g["w.xformer.lm_head.weight"].shape[0])
    f = dict(n_layer_xformer=2, n_layer_e3gnn=5, n_hidden_xformer=64, n_hidden_e3nn=128, n_embd_common=64, n_head=4, n_seq=32, n_tok=V,
             msg_cutoff=5.0, pad_token=31, stop_token=40, unk_token=44, use_fp8=0, norm_clips=0, token_mlp=1, use_point_encoder=0,
             biases=1, norm_embed=0, torch_emb=0, old_architecture=0, residual=0)
    f.update(over)
    c = _lib.CoatiConfig(*[f[n] for n, _ in _lib.CoatiConfig._fields_])
    h = ctypes.c_void_p()
    rc = l.coati_engine_create_coati2(ctypes.byref(c), ENC_TO_COATI[variant], ctypes.byref(h))
    if rc != 0:
        return None
    try:
        names, shapes = [], {}
        buf = ctypes.create_string_buffer(256)
        off, rows, cols = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        for i in range(l.coati_engine_n_entries(h)):
            _lib.check(l.coati_engine_entry(h, i, buf, 256, ctypes.byref(off), ctypes.byref(rows), ctypes.byref(cols)), "entry")
            names.append(buf.value.decode())
            shapes[names[-1]] = (rows.value, cols.value) if cols.value > 0 else (rows.value,)
        return names, shapes
    finally:
        l.coati_engine_destroy(h)


@pytest.mark.parametrize("variant", ["linear", "swiglu_mlp", "swiglu_resnet"])
def test_parameter_table_is_the_reference_state_dict(variant):
    from coati_amd.models.simple_coati2.transformer_only import coati2_parameter_order
    g = np.load(os.path.join(GOLDEN, "coati2_golden.npz"))
    names, shapes = _layout(variant)
    ref_keys = [k for k in g[f"{variant}.keys"].tolist() if not k.endswith(".attn.bias")]
    assert coati2_parameter_order(names) == ref_keys
    for k in ref_keys:
        assert shapes[k] == g[f"w.{k}" if k.startswith("xformer.") else f"{variant}.w.{k}"].shape, k


def test_create_coati2_refusals():
    assert _layout("linear") is not None
    assert _layout("linear", use_point_encoder=1) is None
    assert _layout("linear", use_fp8=1) is None
    assert _layout("linear", n_embd_common=128) is None
    assert _layout("linear", norm_embed=1) is None
    assert _layout("linear", n_seq=300) is None
