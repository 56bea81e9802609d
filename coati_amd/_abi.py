"""Reads include/coati_hip.h into ctypes signatures, so that the Python binding cannot disagree with the C ABI.  No C parser: the header
is one extern "C" block of prototypes over a handful of scalar types, one struct, one anonymous enum and opaque typedefs, and anything
else at file scope is an error here, never skipped.  A feature header of the same library (the table build.FEATURE_HEADERS lists them) is read the same way,
against the first one's coati_config and scalar types (parse(..., base=)).  Imports neither torch nor the library."""
import ctypes
import re
from collections import namedtuple
from ctypes import POINTER, c_char_p, c_float, c_int, c_int64, c_void_p

SCALARS = {"int": c_int, "int32_t": c_int, "int64_t": c_int64, "long long": c_int64, "float": c_float}
# what the header is read under: its include guard, the experimental operators (flagged), and as C (the extern "C" braces are left out)
GUARD, NAME = "COATI_HIP_H", "coati_hip.h"
CONDITIONS = ("ifdef COATI_EXPERIMENTAL", "ifdef __cplusplus")      # next to the header's own "ifndef <guard>"

# prototypes: name -> (restype, argtypes); experimental: the names declared under #ifdef COATI_EXPERIMENTAL;
# config_fields: [(name, ctype)] of coati_config in order, CoatiConfig the Structure made of them; version: COATI_ABI_VERSION
Abi = namedtuple("Abi", "prototypes experimental config_fields CoatiConfig version")


def strip_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)


def _statements(code, name=NAME):
    """the pieces of `code` between the ';' that are outside braces"""
    depth = start = 0
    for i, ch in enumerate(code):
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            yield " ".join(code[start:i].split())
            start = i + 1
    if code[start:].strip():
        raise ValueError(f"{name}: unfinished statement {' '.join(code[start:].split())!r}")


def _ctype(decl, config, void_ok=False, name=NAME):
    """ctypes type of a C type as the header spells it"""
    t = " ".join(decl.replace("*", " * ").split())
    if "*" not in t:
        if t == "void" and void_ok:
            return None
        if t not in SCALARS:
            raise ValueError(f"{name}: type {decl!r} is not one the binding knows")
        return SCALARS[t]
    if not re.fullmatch(r"[\w ]+( \*( const)?)+", t):
        raise ValueError(f"{name}: {decl!r} is not a pointer type")
    if t in ("char *", "const char *"):
        return c_char_p
    if t == "const coati_config *":
        if config is None:
            raise ValueError(f"{name}: coati_config is used before it is defined")
        return POINTER(config)
    return c_void_p


def parse(text, experimental=True, guard=GUARD, name=NAME, base=None):
    """The Abi of the header `text`; experimental = False leaves the prototypes under #ifdef COATI_EXPERIMENTAL out.
    guard / name: the header's include guard, and its file name for the error messages.  base: the Abi of coati_hip.h when `text` is a
    further header of the library: coati_config and the version are base's, the header defines neither, and declaring one of base's
    names again is an error."""
    conditions = (f"ifndef {guard}",) + CONDITIONS
    chunks, open_ifs, defines = [[False, ""]], [], {}          # chunks: [experimental?, code between two preprocessor lines]
    for line in strip_comments(text).splitlines():
        m = re.match(r"\s*#\s*(\w+)\s*(.*?)\s*$", line)
        if not m:
            if "ifdef __cplusplus" not in open_ifs:
                chunks[-1][1] += line + "\n"
            continue
        word, rest = m.groups()
        if word in ("ifdef", "ifndef") and f"{word} {rest}" in conditions:
            open_ifs.append(f"{word} {rest}")
        elif word == "endif" and open_ifs:
            open_ifs.pop()
        elif word == "define":
            defines[rest.split()[0]] = rest.split()[1:]
        elif word != "include":
            raise ValueError(f"{name}: preprocessor line {line.strip()!r} is not one the binding knows")
        chunks.append(["ifdef COATI_EXPERIMENTAL" in open_ifs, ""])
    if open_ifs:
        raise ValueError(f"{name}: #{open_ifs[-1]} is never closed")
    protos, flagged, fields, config = {}, set(), [], None
    if base is not None:
        fields, config = base.config_fields, base.CoatiConfig
    for is_exp, code in chunks:
        for s in _statements(code, name):
            struct = re.fullmatch(r"typedef struct coati_config \{(.*)\} coati_config", s)
            proto = re.fullmatch(r"([\w\s*]+?)\b(coati_\w+) ?\((.*)\)", s)
            if struct and config is None:
                for decl in _statements(struct.group(1), name):
                    ctype, _, names = decl.partition(" ")
                    fields += [(n.strip(), _ctype(ctype, None, name=name)) for n in names.split(",")]
                config = type("CoatiConfig", (ctypes.Structure,), {"_fields_": fields})
            elif proto and proto.group(2) not in protos:
                ret, fn, params = proto.groups()
                params = [] if params.strip() == "void" else [re.fullmatch(r"(.*?)\w+", p.strip()) for p in params.split(",")]
                if None in params:
                    raise ValueError(f"{name}: cannot read the parameters of {s!r}")
                if base is not None and proto.group(2) in base.prototypes:
                    raise ValueError(f"{name}: {proto.group(2)} is already declared in {NAME}")
                sig = (_ctype(ret, config, void_ok=True, name=name), [_ctype(p.group(1), config, name=name) for p in params])
                if experimental or not is_exp:
                    protos[fn] = sig
                    flagged.update([fn] if is_exp else [])
            elif not re.fullmatch(r"typedef struct (\w+) \1|enum \{[\w\s=,]*\}", s):
                raise ValueError(f"{name}: statement {s!r} is neither a prototype, coati_config, the enum nor an opaque typedef")
    if base is not None:
        return Abi(protos, frozenset(flagged), fields, config, base.version)
    version = defines.get("COATI_ABI_VERSION", [])
    if config is None or len(version) != 1 or not version[0].isdigit():
        raise ValueError(f"{name}: coati_config or a numeric COATI_ABI_VERSION is missing")
    return Abi(protos, frozenset(flagged), fields, config, int(version[0]))
