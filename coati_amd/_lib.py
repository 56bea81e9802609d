"""ctypes binding of libcoati_hip.so.  Every signature, the config struct and the ABI version are read from the C ABI's own header
(include/coati_hip.h, _abi.py), and the entries of every feature header of build.FEATURE_HEADERS (include/coati_<stem>.h) the same way:
nothing of it is restated here.  There is no CPU fallback: if the library is missing or a call fails, a RuntimeError is raised."""
import ctypes
import os

from . import _abi
from . import build as _build

try:
    with open(_build.HEADER) as _f:
        _ABI = _abi.parse(_f.read())
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.HEADER}, which the binding of libcoati_hip.so is derived from: {e}") from e

PROTOTYPES = _ABI.prototypes        # name -> (restype, argtypes), the operators of csrc/experimental/ included
CoatiConfig = _ABI.CoatiConfig
ABI_VERSION = _ABI.version
# stem -> the entries of include/coati_<stem>.h, in the same library (tables of their own: PROTOTYPES is coati_hip.h's); each is also the
# module attribute <STEM>_PROTOTYPES (BEAM_PROTOTYPES ... TSNE_PROTOTYPES)
HEADER_PROTOTYPES = {}
for _stem, _what in _build.FEATURE_HEADERS:
    _path = getattr(_build, f"{_stem.upper()}_HEADER")      # through the attribute: a path set there after import counts
    try:
        with open(_path) as _f:
            _table = _abi.parse(_f.read(), guard=f"COATI_{_stem.upper()}_H", name=f"coati_{_stem}.h", base=_ABI).prototypes
    except OSError as e:
        raise RuntimeError(f"coati_amd: cannot read {_path}, which the binding of {_what} is derived from: {e}") from e
    for _other, _theirs in HEADER_PROTOTYPES.items():
        if set(_table) & set(_theirs):
            raise ValueError(f"coati_{_stem}.h: {min(set(_table) & set(_theirs))} is already declared in coati_{_other}.h")
    HEADER_PROTOTYPES[_stem] = globals()[f"{_stem.upper()}_PROTOTYPES"] = _table

_lib = None


def has_experimental():
    return hasattr(lib(), "coati_attn_block_fwd")


def lib():
    """Loads (building if the sources are newer) the HIP library.  Raises if it cannot be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB
    # build() is a no-op unless a source under csrc/ or include/ is newer than the library (build.needs_build); when no
    # compiler is around (a box that only received the prebuilt .so) a stale-looking timestamp must not be fatal
    try:
        _build.build(force=os.environ.get("COATI_AMD_REBUILD") == "1", verbose=False)
    except Exception:
        if not os.path.exists(path):
            raise
    if not os.path.exists(path):
        raise RuntimeError(f"coati_amd: {path} is missing and could not be built; there is no CPU fallback")
    # torch first: its wheel carries its own ROCm runtime; loading this library before torch would bind it to the system
    # libamdhip64 and leave the process with two HIP runtimes (one of which then reports "no ROCm-capable device")
    import torch  # noqa: F401
    l = ctypes.CDLL(path)
    # operators of csrc/experimental/ are only in libcoati_hip_x.so (COATI_AMD_EXPERIMENTAL=1, build.py): bound when the loaded library has them
    for name, (restype, argtypes) in [item for table in [PROTOTYPES, *HEADER_PROTOTYPES.values()] for item in table.items()]:
        if hasattr(l, name):
            getattr(l, name).restype = restype
            getattr(l, name).argtypes = argtypes
    if l.coati_abi_version() != ABI_VERSION:
        raise RuntimeError(f"coati_amd: {path} has ABI version {l.coati_abi_version()}, this package expects {ABI_VERSION}; "
                           "rebuild with `python -m coati_amd.build --force`")
    missing = [n for n in required_symbols() if not hasattr(l, n)]
    if missing:
        raise RuntimeError(f"coati_amd: {path} lacks symbols {missing[:6]}; rebuild with `python -m coati_amd.build --force`")
    _lib = l
    return l


def exported_symbols():
    return sorted(n for n in PROTOTYPES if _build.EXPERIMENTAL or n not in _ABI.experimental)


def required_symbols():
    """what the loaded library must export: exported_symbols() and every entry of every feature header"""
    return exported_symbols() + [n for table in HEADER_PROTOTYPES.values() for n in sorted(table)]


def check(rc, what=""):
    if rc != 0:
        msg = lib().coati_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"libcoati_hip: {what} failed (code {rc}): {msg}")


def call(name, *args):
    if name in _ABI.experimental and not hasattr(lib(), name):
        raise RuntimeError(f"libcoati_hip: {name} is an operator of csrc/experimental/ -- build and load with COATI_AMD_EXPERIMENTAL=1")
    check(getattr(lib(), name)(*args), name)
