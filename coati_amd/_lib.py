"""ctypes binding of libcoati_hip.so.  Every signature, the config struct and the ABI version are read from the C ABI's own header
(include/coati_hip.h, _abi.py), the beam-search entries from include/coati_beam.h, the library-search entries from include/coati_search.h,
the constrained-decoding entry from include/coati_grammar.h, the property-head entry from include/coati_screen.h, its input gradient from include/coati_guide.h, the GP head from include/coati_gp.h, the gradient of its acquisition from include/coati_acq.h, library clustering from include/coati_cluster.h, IVF approximate search from include/coati_ivf.h, radius search from include/coati_radius.h, the point encoder's kernels one by one from include/coati_gnn_ops.h, quantised search from include/coati_search8.h, IVF search over fp8 lists from include/coati_ivf8.h, radius search over inverted lists from include/coati_ivf_radius.h, product-quantised search from include/coati_pq.h, IVF search over lists of residual PQ codes from include/coati_ivfpq.h, four-bit search from include/coati_search4.h, embedding maps from include/coati_tsne.h: nothing of it is restated here.  There is no CPU fallback: if the library is missing or a call fails, a
RuntimeError is raised."""
import ctypes
import os

from . import _abi
from . import build as _build

try:
    with open(_build.HEADER) as _f:
        _ABI = _abi.parse(_f.read())
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.HEADER}, which the binding of libcoati_hip.so is derived from: {e}") from e
try:
    with open(_build.BEAM_HEADER) as _f:
        _BEAM_ABI = _abi.parse(_f.read(), guard="COATI_BEAM_H", name="coati_beam.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.BEAM_HEADER}, which the beam-search binding is derived from: {e}") from e
try:
    with open(_build.SEARCH_HEADER) as _f:
        _SEARCH_ABI = _abi.parse(_f.read(), guard="COATI_SEARCH_H", name="coati_search.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.SEARCH_HEADER}, which the library-search binding is derived from: {e}") from e
try:
    with open(_build.GRAMMAR_HEADER) as _f:
        _GRAMMAR_ABI = _abi.parse(_f.read(), guard="COATI_GRAMMAR_H", name="coati_grammar.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.GRAMMAR_HEADER}, which the constrained-decoding binding is derived from: {e}") from e
try:
    with open(_build.SCREEN_HEADER) as _f:
        _SCREEN_ABI = _abi.parse(_f.read(), guard="COATI_SCREEN_H", name="coati_screen.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.SCREEN_HEADER}, which the property-head binding is derived from: {e}") from e
try:
    with open(_build.GUIDE_HEADER) as _f:
        _GUIDE_ABI = _abi.parse(_f.read(), guard="COATI_GUIDE_H", name="coati_guide.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.GUIDE_HEADER}, which the head-gradient binding is derived from: {e}") from e
try:
    with open(_build.LN_XHAT_HEADER) as _f:
        _LN_XHAT_ABI = _abi.parse(_f.read(), guard="COATI_LN_XHAT_H", name="coati_ln_xhat.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.LN_XHAT_HEADER}, which the saved-xhat binding is derived from: {e}") from e
try:
    with open(_build.GP_HEADER) as _f:
        _GP_ABI = _abi.parse(_f.read(), guard="COATI_GP_H", name="coati_gp.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.GP_HEADER}, which the GP-head binding is derived from: {e}") from e
try:
    with open(_build.ACQ_HEADER) as _f:
        _ACQ_ABI = _abi.parse(_f.read(), guard="COATI_ACQ_H", name="coati_acq.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.ACQ_HEADER}, which the acquisition-gradient binding is derived from: {e}") from e
try:
    with open(_build.CLUSTER_HEADER) as _f:
        _CLUSTER_ABI = _abi.parse(_f.read(), guard="COATI_CLUSTER_H", name="coati_cluster.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.CLUSTER_HEADER}, which the library-clustering binding is derived from: {e}") from e
try:
    with open(_build.IVF_HEADER) as _f:
        _IVF_ABI = _abi.parse(_f.read(), guard="COATI_IVF_H", name="coati_ivf.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.IVF_HEADER}, which the IVF-search binding is derived from: {e}") from e
try:
    with open(_build.RADIUS_HEADER) as _f:
        _RADIUS_ABI = _abi.parse(_f.read(), guard="COATI_RADIUS_H", name="coati_radius.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.RADIUS_HEADER}, which the radius-search binding is derived from: {e}") from e
try:
    with open(_build.GNN_OPS_HEADER) as _f:
        _GNN_OPS_ABI = _abi.parse(_f.read(), guard="COATI_GNN_OPS_H", name="coati_gnn_ops.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.GNN_OPS_HEADER}, which the binding of the point encoder's single kernels is derived from: {e}") from e
try:
    with open(_build.SEARCH8_HEADER) as _f:
        _SEARCH8_ABI = _abi.parse(_f.read(), guard="COATI_SEARCH8_H", name="coati_search8.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.SEARCH8_HEADER}, which the quantised-search binding is derived from: {e}") from e
try:
    with open(_build.IVF8_HEADER) as _f:
        _IVF8_ABI = _abi.parse(_f.read(), guard="COATI_IVF8_H", name="coati_ivf8.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.IVF8_HEADER}, which the binding of the IVF search over fp8 lists is derived from: {e}") from e
try:
    with open(_build.IVF_RADIUS_HEADER) as _f:
        _IVF_RADIUS_ABI = _abi.parse(_f.read(), guard="COATI_IVF_RADIUS_H", name="coati_ivf_radius.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.IVF_RADIUS_HEADER}, which the binding of the radius search over inverted lists is derived from: {e}") from e
try:
    with open(_build.PQ_HEADER) as _f:
        _PQ_ABI = _abi.parse(_f.read(), guard="COATI_PQ_H", name="coati_pq.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.PQ_HEADER}, which the binding of the product-quantised search is derived from: {e}") from e
try:
    with open(_build.IVFPQ_HEADER) as _f:
        _IVFPQ_ABI = _abi.parse(_f.read(), guard="COATI_IVFPQ_H", name="coati_ivfpq.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.IVFPQ_HEADER}, which the binding of the IVF-PQ search is derived from: {e}") from e
try:
    with open(_build.SEARCH4_HEADER) as _f:
        _SEARCH4_ABI = _abi.parse(_f.read(), guard="COATI_SEARCH4_H", name="coati_search4.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.SEARCH4_HEADER}, which the binding of the four-bit search is derived from: {e}") from e
try:
    with open(_build.TSNE_HEADER) as _f:
        _TSNE_ABI = _abi.parse(_f.read(), guard="COATI_TSNE_H", name="coati_tsne.h", base=_ABI)
except OSError as e:
    raise RuntimeError(f"coati_amd: cannot read {_build.TSNE_HEADER}, which the binding of the embedding maps is derived from: {e}") from e

PROTOTYPES = _ABI.prototypes        # name -> (restype, argtypes), the operators of csrc/experimental/ included
CoatiConfig = _ABI.CoatiConfig
ABI_VERSION = _ABI.version
BEAM_PROTOTYPES = _BEAM_ABI.prototypes   # the entries of include/coati_beam.h, in the same library (a table of their own: PROTOTYPES is coati_hip.h's)
SEARCH_PROTOTYPES = _SEARCH_ABI.prototypes   # the entries of include/coati_search.h, likewise
GRAMMAR_PROTOTYPES = _GRAMMAR_ABI.prototypes   # the entry of include/coati_grammar.h, likewise
SCREEN_PROTOTYPES = _SCREEN_ABI.prototypes   # the entry of include/coati_screen.h, likewise
GUIDE_PROTOTYPES = _GUIDE_ABI.prototypes   # the entry of include/coati_guide.h, likewise
LN_XHAT_PROTOTYPES = _LN_XHAT_ABI.prototypes   # the entries of include/coati_ln_xhat.h, likewise
GP_PROTOTYPES = _GP_ABI.prototypes   # the entry of include/coati_gp.h, likewise
ACQ_PROTOTYPES = _ACQ_ABI.prototypes   # the entry of include/coati_acq.h, likewise
CLUSTER_PROTOTYPES = _CLUSTER_ABI.prototypes   # the entries of include/coati_cluster.h, likewise
IVF_PROTOTYPES = _IVF_ABI.prototypes   # the entries of include/coati_ivf.h, likewise
RADIUS_PROTOTYPES = _RADIUS_ABI.prototypes   # the entries of include/coati_radius.h, likewise
GNN_OPS_PROTOTYPES = _GNN_OPS_ABI.prototypes   # the entries of include/coati_gnn_ops.h, likewise
SEARCH8_PROTOTYPES = _SEARCH8_ABI.prototypes   # the entries of include/coati_search8.h, likewise
IVF8_PROTOTYPES = _IVF8_ABI.prototypes   # the entry of include/coati_ivf8.h, likewise
IVF_RADIUS_PROTOTYPES = _IVF_RADIUS_ABI.prototypes   # the entries of include/coati_ivf_radius.h, likewise
PQ_PROTOTYPES = _PQ_ABI.prototypes   # the entries of include/coati_pq.h, likewise
IVFPQ_PROTOTYPES = _IVFPQ_ABI.prototypes   # the entries of include/coati_ivfpq.h, likewise
SEARCH4_PROTOTYPES = _SEARCH4_ABI.prototypes   # the entries of include/coati_search4.h, likewise
TSNE_PROTOTYPES = _TSNE_ABI.prototypes   # the entries of include/coati_tsne.h, likewise

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
    for name, (restype, argtypes) in list(PROTOTYPES.items()) + list(BEAM_PROTOTYPES.items()) + list(SEARCH_PROTOTYPES.items()) + list(GRAMMAR_PROTOTYPES.items()) + list(SCREEN_PROTOTYPES.items()) + list(GUIDE_PROTOTYPES.items()) + list(LN_XHAT_PROTOTYPES.items()) + list(GP_PROTOTYPES.items()) + list(ACQ_PROTOTYPES.items()) + list(CLUSTER_PROTOTYPES.items()) + list(IVF_PROTOTYPES.items()) + list(RADIUS_PROTOTYPES.items()) + list(GNN_OPS_PROTOTYPES.items()) + list(SEARCH8_PROTOTYPES.items()) + list(IVF8_PROTOTYPES.items()) + list(IVF_RADIUS_PROTOTYPES.items()) + list(PQ_PROTOTYPES.items()) + list(IVFPQ_PROTOTYPES.items()) + list(SEARCH4_PROTOTYPES.items()) + list(TSNE_PROTOTYPES.items()):
        if hasattr(l, name):
            getattr(l, name).restype = restype
            getattr(l, name).argtypes = argtypes
    if l.coati_abi_version() != ABI_VERSION:
        raise RuntimeError(f"coati_amd: {path} has ABI version {l.coati_abi_version()}, this package expects {ABI_VERSION}; "
                           "rebuild with `python -m coati_amd.build --force`")
    missing = [n for n in exported_symbols() + sorted(BEAM_PROTOTYPES) + sorted(SEARCH_PROTOTYPES) + sorted(GRAMMAR_PROTOTYPES) + sorted(SCREEN_PROTOTYPES) + sorted(GUIDE_PROTOTYPES) + sorted(LN_XHAT_PROTOTYPES) + sorted(GP_PROTOTYPES) + sorted(ACQ_PROTOTYPES) + sorted(CLUSTER_PROTOTYPES) + sorted(IVF_PROTOTYPES) + sorted(RADIUS_PROTOTYPES) + sorted(GNN_OPS_PROTOTYPES) + sorted(SEARCH8_PROTOTYPES) + sorted(IVF8_PROTOTYPES) + sorted(IVF_RADIUS_PROTOTYPES) + sorted(PQ_PROTOTYPES) + sorted(IVFPQ_PROTOTYPES) + sorted(SEARCH4_PROTOTYPES) + sorted(TSNE_PROTOTYPES) if not hasattr(l, n)]
    if missing:
        raise RuntimeError(f"coati_amd: {path} lacks symbols {missing[:6]}; rebuild with `python -m coati_amd.build --force`")
    _lib = l
    return l


def exported_symbols():
    return sorted(n for n in PROTOTYPES if _build.EXPERIMENTAL or n not in _ABI.experimental)


def check(rc, what=""):
    if rc != 0:
        msg = lib().coati_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"libcoati_hip: {what} failed (code {rc}): {msg}")


def call(name, *args):
    if name in _ABI.experimental and not hasattr(lib(), name):
        raise RuntimeError(f"libcoati_hip: {name} is an operator of csrc/experimental/ -- build and load with COATI_AMD_EXPERIMENTAL=1")
    check(getattr(lib(), name)(*args), name)
