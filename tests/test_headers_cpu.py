"""The feature headers as a set (no GPU): build.FEATURE_HEADERS is the one table that coati_amd/build.py and coati_amd/_lib.py walk.  It
lists exactly the headers under include/, every header's path and table are the module attributes the per-feature tests use, no name is
declared twice, and every declared name is a bound symbol of the loaded library -- for whichever header comes next as well."""
import glob
import importlib
import itertools
import os
import shutil

import pytest


def _stems():
    from coati_amd import build
    return [stem for stem, _ in build.FEATURE_HEADERS]


def test_table_lists_exactly_the_headers_under_include():
    from coati_amd import build
    include = os.path.dirname(build.HEADER)
    there = sorted(p for p in glob.glob(os.path.join(include, "coati_*.h")) if p != build.HEADER)
    assert there == sorted(os.path.join(include, f"coati_{stem}.h") for stem in _stems())
    assert len(set(_stems())) == len(_stems()) >= 19
    assert all(what and "\n" not in what for _, what in build.FEATURE_HEADERS)


def test_every_stem_has_its_path_and_table_attributes():
    from coati_amd import _lib, build
    assert list(_lib.HEADER_PROTOTYPES) == _stems()
    for stem in _stems():
        assert getattr(_lib, f"{stem.upper()}_PROTOTYPES") is _lib.HEADER_PROTOTYPES[stem], stem
        assert _lib.HEADER_PROTOTYPES[stem], stem
        path = getattr(build, f"{stem.upper()}_HEADER")
        assert path.endswith(os.path.join("include", f"coati_{stem}.h")) and path in build._sources(), stem
    assert build.HEADER in build._sources()


def test_all_tables_are_disjoint_and_required_symbols_is_their_union():
    from coati_amd import _lib, build
    tables = {"hip": _lib.PROTOTYPES, **_lib.HEADER_PROTOTYPES}
    assert len(tables) == 1 + len(build.FEATURE_HEADERS) >= 20
    for (a, ta), (b, tb) in itertools.combinations(tables.items(), 2):
        assert not set(ta) & set(tb), (a, b)
    required = _lib.required_symbols()
    assert len(required) == len(set(required)) == len(_lib.exported_symbols()) + sum(len(t) for t in _lib.HEADER_PROTOTYPES.values())
    assert required[:len(_lib.exported_symbols())] == _lib.exported_symbols()
    assert set(required) == set(_lib.exported_symbols()).union(*_lib.HEADER_PROTOTYPES.values())


def test_a_name_declared_in_two_feature_headers_is_refused(tmp_path, monkeypatch):
    from coati_amd import _lib, build
    twice = str(tmp_path / "coati_tsne.h")
    shutil.copy(build.TSNE_HEADER, twice)
    with open(twice) as f:
        text = f.read()
    assert text.count("int coati_tsne_chunk(void);") == 1
    with open(twice, "w") as f:
        f.write(text.replace("int coati_tsne_chunk(void);", "int coati_search_slices(int64_t N, int Q, int k);\nint coati_tsne_chunk(void);"))
    monkeypatch.setattr(build, "TSNE_HEADER", twice)
    try:
        with pytest.raises(ValueError) as e:
            importlib.reload(_lib)
        assert "coati_tsne.h" in str(e.value) and "coati_search.h" in str(e.value) and "coati_search_slices" in str(e.value)
    finally:
        monkeypatch.undo()
        importlib.reload(_lib)
    assert "coati_search_slices" in _lib.SEARCH_PROTOTYPES and "coati_search_slices" not in _lib.TSNE_PROTOTYPES


def test_every_declared_entry_is_bound_as_parsed():
    from coati_amd import _lib
    l = _lib.lib()
    for stem, table in _lib.HEADER_PROTOTYPES.items():
        for name, (restype, argtypes) in table.items():
            fn = getattr(l, name)
            assert fn.restype is restype and list(fn.argtypes) == list(argtypes), (stem, name)
    for name in _lib.exported_symbols():
        restype, argtypes = _lib.PROTOTYPES[name]
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
