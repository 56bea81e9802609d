"""Likelihood scoring, host side: the rows e3gnn_smiles_clip_e2e.hclip_and_tokens_to_likelihood / batch_smiles_to_s2s_likelihood build
from SMILES (tokens, encoder tokens, targets, tokenize mask) against what the reference computed inside the same calls
(tests/golden/likelihood_golden.npz, gen_golden_likelihood.py).  Needs no GPU: the builders run on host tensors."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def golden(golden_dir):
    from coati_amd.models.encoding.tokenizers import TrieTokenizer
    g = np.load(os.path.join(golden_dir, "likelihood_golden.npz"))
    voc = json.load(open(os.path.join(golden_dir, "tokenizer.json")))
    tk = TrieTokenizer(n_seq=int(g["n_seq"]), smiles_tokens=voc["smiles"], special_tokens=voc["special"])
    return g, tk


def test_tokenize_smiles_matches_reference_rule(golden):
    from coati_amd.models.encoding.clip_e2e import _tokenize_smiles
    g, tk = golden
    with contextlib.redirect_stdout(io.StringIO()):
        rows = [_tokenize_smiles(s, tk, prefix="", suffix="[STOP]", max_size=tk.n_seq - 5) for s in g["smiles"].tolist()]
        assert _tokenize_smiles("CC", tk).shape == (tk.n_seq,)                  # default: [SMILES]..[STOP] in n_seq positions
        assert int(_tokenize_smiles("CC", tk)[0]) == tk.smiles_token
    assert [r is not None for r in rows] == g["s2s.mask"].tolist()
    assert torch.equal(torch.stack([r for r in rows if r is not None]), torch.from_numpy(g["s2s.raw_tokens"][:, 1:]))


def test_s2s_rows_match_reference(golden):
    """tokens, encoder tokens, targets and mask of batch_smiles_to_s2s_likelihood, bit for bit"""
    from coati_amd.models.encoding.clip_e2e import s2s_likelihood_tokens
    g, tk = golden
    with contextlib.redirect_stdout(io.StringIO()):
        raw, tok, y, mask = s2s_likelihood_tokens(g["smiles"].tolist(), tk)
    assert mask.dtype == torch.bool and mask.tolist() == g["s2s.mask"].tolist()
    assert mask.tolist().count(False) == 2            # the oversize row and the row with a piece outside the vocabulary
    assert torch.equal(raw, torch.from_numpy(g["s2s.raw_tokens"]))
    assert torch.equal(tok, torch.from_numpy(g["s2s.tokens"]))
    assert torch.equal(y.reshape(-1), torch.from_numpy(g["s2s.targets"]))
    # the reference's per-token cross-entropy is zero exactly where the targets are masked
    ce = torch.from_numpy(g["s2s.ce"])
    assert bool((ce[y.reshape(-1) < 0] == 0).all()) and bool((ce[y.reshape(-1) >= 0] > 0).all())


def test_hclip_rows_match_reference(golden):
    """one padded batch of hclip_and_tokens_to_likelihood rows == the reference's single-row tokens / targets, row by row; the
    [PAD] tail of the shorter rows carries no target"""
    from coati_amd.models.encoding.clip_e2e import hclip_likelihood_tokens
    g, tk = golden
    smiles = g["hclip_smiles"].tolist()
    tok, y = hclip_likelihood_tokens(smiles, tk)
    assert tok.shape == (len(smiles), max(g[f"hclip.{i}.tokens"].shape[1] for i in range(len(smiles))))
    for i in range(len(smiles)):
        rt, ry = torch.from_numpy(g[f"hclip.{i}.tokens"][0]), torch.from_numpy(g[f"hclip.{i}.targets"])
        n = rt.shape[0]
        assert torch.equal(tok[i, :n], rt) and torch.equal(y[i, :n], ry), i
        assert bool((tok[i, n:] == tk.pad_token).all()) and bool((y[i, n:] == -1).all())
    # single-row form: exactly the reference's row
    t1, y1 = hclip_likelihood_tokens(smiles[:1], tk)
    assert torch.equal(t1, torch.from_numpy(g["hclip.0.tokens"])) and torch.equal(y1[0], torch.from_numpy(g["hclip.0.targets"]))


def test_hclip_rows_raise_like_reference(golden):
    """a piece outside the vocabulary raises KeyError, an oversize row the reference's 'Oversized String' (range_check=True)"""
    from coati_amd.models.encoding.clip_e2e import hclip_likelihood_tokens
    _, tk = golden
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(KeyError):
            hclip_likelihood_tokens(["CxC"], tk)
        with pytest.raises(Exception, match="Oversized"):
            hclip_likelihood_tokens(["CN" * 10], tk)


def test_methods_exist_on_the_model_and_the_alias():
    """code written against the reference finds both methods (and the module-level helper) under coati.* as well"""
    import coati  # noqa: F401
    from coati.models.encoding import clip_e2e as alias
    from coati_amd.models.encoding import clip_e2e as real
    assert alias is real
    for name in ("hclip_and_tokens_to_likelihood", "batch_smiles_to_s2s_likelihood"):
        assert callable(getattr(alias.e3gnn_smiles_clip_e2e, name))
    assert callable(alias._tokenize_smiles)
