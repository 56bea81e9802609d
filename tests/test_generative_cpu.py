"""coati.generative / coati.common.util on the host: the modules import under the reference's names with its parameters and defaults,
batch_indexable slices as the reference's does, and the host logic of the purification and forced-decoding functions (drop rules,
deduplication, tie-break, "C" fallback, V returned unchanged) reproduces tests/golden/generative_golden.npz against a stub encoder
with scripted decodes (tests/golden/gen_golden_generative.py)."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import coati  # noqa: E402,F401  (the coati.* alias)

# the reference's signatures (coati/generative/coati_purifications.py, coati_density.py, coati/common/util.py): (name, default) pairs
REF_SIGS = {
    "coati.generative.coati_purifications": {
        "embed_points": [("s", None), ("encoder", None)],
        "embed_smiles": [("s", None), ("encoder", None), ("tokenizer", None)],
        "embed_smiles_batch": [("smiles_list", None), ("encoder", None), ("tokenizer", None)],
        "purify_vector": [("V", None), ("encoder", None), ("tokenizer", None), ("n_rep", 128)],
        "force_decode_valid": [("V", None), ("encoder", None), ("tokenizer", None), ("max_attempts", 2000)],
        "force_decode_valid_batch": [("V", None), ("encoder", None), ("tokenizer", None), ("batch_size", 128), ("max_attempts", 4)],
    },
    "coati.generative.coati_density": {
        "estimate_density_batchwise": [("iterable", None), ("encoder", None), ("tokenizer", None), ("batch_size", 1024), ("epochs", 10),
                                       ("entropy_limit", -100)],
    },
    "coati.common.util": {
        "batch_indexable": [("iterable", None), ("n", 128)],
        "dir_or_file_exists": [("d", None)],
        "tensor_of_dict_of_lists": [("d", None)],
        "colored_background": [("r", None), ("g", None), ("b", None), ("text", None)],
        "json_valid_dict": [("obj", None)],
        "utc_epoch_now": [],
        "makedir": [("path", None), ("isfile", False)],
        "rmdir": [("path", None)],
        "records_mp": [("recs", None), ("func", None), ("args", None), ("n", None)],
        "execute_with_timeout": [("method", None), ("args", None), ("timeout", None)],
        "get_tnet_dir": [],
        "dicts_to_keyval": [("list_of_dicts", None), ("key", None), ("value", None)],
        "query_yes_no": [("question", None), ("default", None)],
        "get_all_allocated_torch_tensors": [],
    },
}


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "generative_golden.npz"))


def _canon(s):
    """the golden's rdkit rule (gen_golden_generative.canon)"""
    if not s or "X" in s:
        return None
    return min(s, s[::-1])


@pytest.fixture(scope="module")
def tok(golden_dir):
    from coati_amd.models.encoding.tokenizers import TrieTokenizer
    voc = json.load(open(os.path.join(golden_dir, "tokenizer.json")))
    return TrieTokenizer(n_seq=24, smiles_tokens=voc["smiles"], special_tokens=voc["special"])


class StubEncoder:
    """no engine: scripted hclip_to_2d_batch / hclip_to_2d ("X", invalid, once the script is used up)"""

    def __init__(self, batches=(), singles=()):
        self.batches, self.singles = list(batches), list(singles)
        self.device = torch.device("cpu")
        self.batch_calls = []

    def hclip_to_2d_batch(self, h, tokenizer):
        self.batch_calls.append(int(h.shape[0]))
        item = self.batches.pop(0)
        if isinstance(item, Exception):
            raise item
        assert len(item) == h.shape[0]
        return list(item)

    def hclip_to_2d(self, h, tokenizer):
        return self.singles.pop(0) if self.singles else "X"


@pytest.mark.parametrize("mod", sorted(REF_SIGS))
def test_reference_names_parameters_and_defaults(mod):
    import importlib
    m = importlib.import_module(mod)
    for name, params in REF_SIGS[mod].items():
        fn = getattr(m, name)
        sig = list(inspect.signature(fn).parameters.values())
        got = [(p.name, None if p.default is inspect.Parameter.empty else p.default) for p in sig[:len(params)]]
        assert got == params, (mod, name, got)
        assert all(p.default is not inspect.Parameter.empty for p in sig[len(params):]), (mod, name, sig)   # additions keep defaults
    if mod == "coati.common.util":
        for cls in ("NpEncoder", "OnlineEstimator"):
            assert inspect.isclass(getattr(m, cls))
        assert not hasattr(m, "s3")


def test_batch_indexable():
    from coati.common.util import batch_indexable
    assert list(batch_indexable(list(range(7)), 3)) == [[0, 1, 2], [3, 4, 5], [6]]
    assert list(batch_indexable("abcdef", 2)) == ["ab", "cd", "ef"]
    assert list(batch_indexable([], 4)) == []
    assert [len(b) for b in batch_indexable(list(range(300)))] == [128, 128, 44]
    t = torch.arange(10)
    parts = list(batch_indexable(t, 4))
    assert [p.tolist() for p in parts] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert inspect.isgenerator(batch_indexable([1], 1))


def test_util_helpers():
    from coati.common import util as U
    assert U.tensor_of_dict_of_lists({"a": [1, 2], "b": ["x"]}) == [{"a": 1, "b": "x"}, {"a": 2, "b": "x"}]
    assert U.json_valid_dict({"a": np.int64(3), "b": np.float32(0.5), "c": torch.tensor([1, 2])}) == {"a": 3, "b": 0.5, "c": [1, 2]}
    assert U.dicts_to_keyval([{"k": 1, "v": 2}, {"k": 3, "v": 4}], "k", "v") == {1: 2, 3: 4}
    est = U.OnlineEstimator(np.array(1.0))
    est(np.array(2.0))
    mean, var = est(np.array(6.0))
    assert np.isclose(mean, 3.0) and np.isclose(var, np.var([1.0, 2.0, 6.0], ddof=1))
    assert U.colored_background(1, 2, 3, "t") == "\033[48;2;1;2;3mt\033[0m"


def test_purification_plan_matches_golden(golden_dir, tok):
    from coati.generative import coati_purifications as P
    g = _golden(golden_dir)
    decoded = [g["purify.0.in"].tolist(), g["purify.1.in"].tolist()]
    plan = P.purification_plan(decoded, tok, _canon)
    # the reference encoded these canonical strings for vector 0 (in decode order), and nothing for vector 1
    assert sorted(plan.expanded(0)) == sorted(g["purify.0.encoded"].tolist())
    assert plan.expanded(1) == [] and g["purify.1.encoded"].size == 0
    assert plan.strings == ["CCO", "CCN"]
    assert plan.members[0] == [(0, 3), (1, 2)]
    assert plan.failed == [False, False]
    # one canonicaliser call per distinct raw string: 7 in vector 0, and the 4 of vector 1 that vector 0 did not have
    assert plan.canon_calls == 7 + 4
    assert plan.rows[0] == tok.tokenize_text("[SMILES]CCO[STOP]", pad=False)


def test_purify_vector_returns_V_unchanged(golden_dir, tok):
    from coati.generative import coati_purifications as P
    g = _golden(golden_dir)
    V = torch.from_numpy(g["V"][1].copy())
    enc = StubEncoder(batches=[g["purify.1.in"].tolist()])
    assert P.purify_vector(V, enc, tok, n_rep=8, canon_smiles=_canon) is V
    assert enc.batch_calls == [8]
    assert torch.equal(V, torch.from_numpy(g["purify.1.out"]))
    enc = StubEncoder(batches=[RuntimeError("decoder failure")])
    V0 = torch.from_numpy(g["V"][0].copy())
    assert P.purify_vector(V0, enc, tok, n_rep=8, canon_smiles=_canon) is V0
    assert torch.equal(V0, torch.from_numpy(g["purify.raise.out"]))


def test_force_decode_valid_matches_golden(golden_dir, tok):
    from coati.generative import coati_purifications as P
    g = _golden(golden_dir)
    V = torch.from_numpy(g["V"][0].copy())
    assert P.force_decode_valid(V, StubEncoder(singles=g["force_one.0.in"].tolist()), tok, canon_smiles=_canon) == str(g["force_one.0.out"])
    assert str(g["force_one.0.out"]) == "OCC"          # the raw string, not its canonical form
    ones = g["force_one.1.in"].tolist()
    assert P.force_decode_valid(V, StubEncoder(singles=ones), tok, max_attempts=len(ones), canon_smiles=_canon) == str(g["force_one.1.out"]) == "C"


def test_force_decode_valid_batch_matches_golden(golden_dir, tok):
    from coati.generative import coati_purifications as P
    g = _golden(golden_dir)
    V = torch.from_numpy(g["V"][0].copy())
    for i in range(2):
        attempts = [g[f"force_batch.{i}.in.{j}"].tolist() for j in range(2)]
        enc = StubEncoder(batches=attempts)
        got = P.force_decode_valid_batch(V, enc, tok, batch_size=6, max_attempts=2, canon_smiles=_canon)
        assert got == str(g[f"force_batch.{i}.out"]), (i, got)
        assert enc.batch_calls == [6, 6]
    assert str(g["force_batch.0.out"]) == "CCN"          # the 2-2 tie goes to the first in decode order
    # a decode call that raises spends the attempt
    enc = StubEncoder(batches=[RuntimeError("x"), ["OCC"] * 6])
    assert P.force_decode_valid_batch(V, enc, tok, batch_size=6, max_attempts=2, canon_smiles=_canon) == "CCO"


def test_most_frequent_valid_and_module_canonicaliser():
    from coati.generative import coati_purifications as P
    assert P.most_frequent_valid(["A", "B", "B", "A", "C"]) == "A"
    assert P.most_frequent_valid(["A", "B", "B"]) == "B"
    assert P.most_frequent_valid([]) is None and P.most_frequent_valid(None) is None
    old = P.canon_smiles
    try:
        P.canon_smiles = _canon
        assert P.most_frequent_valid(["NCC", "CCN", "X", "OCC"]) == "CCN"
        assert P.most_frequent_valid(["X", ""]) is None
    finally:
        P.canon_smiles = old


def test_force_decode_valid_batches_resolves_per_vector(tok):
    from coati.generative import coati_purifications as P
    V = torch.zeros(3, 4)
    # attempt 1: vector 0 resolves, 1 and 2 do not; attempt 2 decodes only vectors 1 and 2, together
    enc = StubEncoder(batches=[["CCO", "X"] + ["X", "X"] + ["X", ""], ["NCC", "CCN"] + ["X", "X"]])
    got = P.force_decode_valid_batches(V, enc, tok, batch_size=2, max_attempts=3, canon_smiles=_canon)
    assert got == ["CCO", "CCN", "C"]
    assert enc.batch_calls == [6, 4, 2]


def test_embed_points_needs_mol_to_atoms_coords():
    from coati.generative import coati_purifications as P
    with pytest.raises(RuntimeError, match="mol_to_atoms_coords"):
        P.embed_points("CCO", StubEncoder())


def test_embed_smiles_rejects_invalid_and_untokenizable(tok):
    from coati.generative import coati_purifications as P
    with pytest.raises(ValueError):
        P.embed_smiles("CX", StubEncoder(), tok, canon_smiles=_canon)
    with pytest.raises(KeyError):
        P.embed_smiles("CxC", StubEncoder(), tok, canon_smiles=_canon)


def test_encode_rows_matches_tokenize_text(tok):
    texts = ["[SMILES]CCO[STOP]", "[SMILES]CxC[STOP]", "[SMILES]" + "CN" * 20 + "[STOP]", "[SMILES]c1ccccc1N[STOP]"]
    ids, lens = tok.encode_rows(texts)
    assert lens.tolist()[1:3] == [-1, -2]
    for i in (0, 3):
        assert ids[i].tolist() == tok.tokenize_text(texts[i], pad=True)
        assert int(lens[i]) == len(tok.tokenize_text(texts[i], pad=False))
