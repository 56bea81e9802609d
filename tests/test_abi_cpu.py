"""The ctypes binding is derived from include/coati_hip.h (coati_amd/_abi.py): what the reader makes of the header, that it refuses
what it does not know instead of skipping it, and that the loaded library's functions carry exactly the parsed signatures.  No GPU."""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int64, c_void_p

import pytest

from coati_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, L, F = c_void_p, c_int, c_int64, c_float


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "coati_hip.h")) as f:
        return f.read()


@pytest.fixture(scope="module")
def abi(header):
    return _abi.parse(header)


def test_counts_move_with_the_header(header, abi):
    assert len(abi.prototypes) == 121 and len(abi.experimental) == 5 and abi.version == 5
    assert abi.experimental <= set(abi.prototypes)
    plain = _abi.parse(header, experimental=False)
    assert set(plain.prototypes) == set(abi.prototypes) - abi.experimental and not plain.experimental


# one signature per kind of type the header uses: name -> (restype, argtypes); None in argtypes = POINTER(CoatiConfig)
SPOT = {
    "coati_gemm_nt": (I, [P, I, L, P, L, I, I, I, P, L, I, P, P, P, L, I, P]),              # mixed int / int64_t
    "coati_sgemm": (I, [P, L, L, P, L, L, P, L, I, I, I, P, F, I, P]),                      # a float scalar
    "coati_adamw": (I, [P, P, P, P, P, L, F, F, F, F, F, I, P, F, P]),                      # five floats in a row
    "coati_tokenizer_encode": (L, [P, c_char_p, L, P, I]),                                   # long long, const char*
    "coati_engine_entry": (I, [P, I, c_char_p, I, P, P, P]),                                 # char* out
    "coati_engine_site_name": (c_char_p, [I]),                                               # const char* return
    "coati_engine_destroy": (None, [P]),                                                     # void
    "coati_wgrad_grouped": (I, [I, P, P, P, P, I, P, P, P, P, P, I, P, L, P]),              # T* const*
    "coati_engine_decode_graph_step": (I, [P, P, P, P, P, P]),                               # float**
    "coati_engine_workspace_bytes": (L, [P, I, I, I, I, I]),                                 # int64_t return
    "coati_ab_trace_read": (I, [P]),                                                         # experimental, unsigned long long*
    "coati_engine_create_coati2": (I, [None, I, P]),                                         # const coati_config*, coati_engine**
    "coati_abi_version": (I, []),                                                            # (void)
}


@pytest.mark.parametrize("name", sorted(SPOT))
def test_spot_signatures(abi, name):
    restype, argtypes = SPOT[name]
    assert abi.prototypes[name] == (restype, [POINTER(abi.CoatiConfig) if a is None else a for a in argtypes])
    assert (name in abi.experimental) == (name == "coati_ab_trace_read")


def test_config_struct(abi):
    fields = abi.config_fields
    assert len(fields) == 21 and ctypes.sizeof(abi.CoatiConfig) == 84 and abi.CoatiConfig._fields_ == fields
    assert [i for i, (_, t) in enumerate(fields) if t is c_float] == [8] and fields[8][0] == "msg_cutoff"
    assert all(t is c_int for i, (_, t) in enumerate(fields) if i != 8)
    assert (fields[0][0], fields[-1][0]) == ("n_layer_xformer", "residual")
    assert [n for n, _ in fields[9:12]] == ["pad_token", "stop_token", "unk_token"]          # three fields of one declaration


@pytest.mark.parametrize("line", ["int coati_x(double v);", "int coati_y(struct foo s);", "static int z;",
                                  "#if 0", "int coati_w(int);", "int coati_v(int a)"])
def test_reader_refuses_what_it_does_not_know(header, line):
    """a scalar type outside the list, a struct by value, a statement that is no prototype; and, beyond those three: a preprocessor
    condition it cannot evaluate, a parameter without a name, a statement that never ends"""
    marker = "typedef struct coati_tokenizer coati_tokenizer;"
    assert header.count(marker) == 1
    _abi.parse(header.replace(marker, marker + "\nint coati_fine(int a);"))                   # the insertion point itself is sound
    with pytest.raises(ValueError, match="coati_hip.h"):
        _abi.parse(header.replace(marker, marker + "\n" + line))


def test_exported_symbols_follow_the_build_variant(abi, monkeypatch):
    from coati_amd import _lib, build
    monkeypatch.setattr(build, "EXPERIMENTAL", False)
    assert _lib.exported_symbols() == sorted(set(abi.prototypes) - abi.experimental)
    monkeypatch.setattr(build, "EXPERIMENTAL", True)
    assert _lib.exported_symbols() == sorted(abi.prototypes)


def test_missing_header_is_an_error_that_names_the_path(monkeypatch, tmp_path):
    import importlib
    from coati_amd import _lib, build
    before = _lib.PROTOTYPES
    monkeypatch.setattr(build, "HEADER", str(tmp_path / "coati_hip.h"))
    with pytest.raises(RuntimeError, match=str(tmp_path / "coati_hip.h")):
        importlib.reload(_lib)              # (fails in the module's first statement: nothing of the loaded module is replaced)
    assert _lib.PROTOTYPES is before


def test_loaded_library_carries_the_parsed_signatures():
    from coati_amd import _lib
    l = _lib.lib()
    assert _lib.ABI_VERSION == l.coati_abi_version() and _lib.CoatiConfig is _lib._ABI.CoatiConfig
    bound = [n for n in _lib.PROTOTYPES if hasattr(l, n)]
    assert set(_lib.exported_symbols()) <= set(bound)
    for name in bound:
        restype, argtypes = _lib.PROTOTYPES[name]
        assert getattr(l, name).restype is restype and list(getattr(l, name).argtypes) == argtypes, name
    for name in set(_lib.PROTOTYPES) - set(bound):      # operators of csrc/experimental/ the loaded library was built without
        with pytest.raises(RuntimeError, match="COATI_AMD_EXPERIMENTAL=1"):
            _lib.call(name, None)
