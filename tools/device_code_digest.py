"""Digest of the device code of every object file of a build: for each .o under the given directory (default coati_amd/build), the sha256 of
the .text, .rodata and .note sections of its gfx950 code object.  Two builds with equal digests hold the same kernels, constants and kernel
descriptors, so a host-side change can be shown to have changed no device code -- on a machine without a GPU.  It hashes bytes and reads
no instruction.  (The whole code object is not compared: its __hip_cuid_<hash> symbol follows the source text.)

    python tools/device_code_digest.py [objdir] > digest.txt      # then diff two of them"""
import hashlib
import os
import subprocess
import sys
import tempfile

SECTIONS = (".text", ".rodata", ".note")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _llvm_bin():
    hipcc = os.path.realpath(os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc")
    for d in (os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin"), os.path.dirname(hipcc)):
        if os.path.exists(os.path.join(d, "llvm-objcopy")):
            return d
    raise RuntimeError(f"no llvm-objcopy next to {hipcc}")


def _dump(llvm, obj, section, out):
    """the bytes of `section` of `obj` (through the file `out`), or None when the object has no such section"""
    if os.path.exists(out):
        os.remove(out)
    r = subprocess.run([os.path.join(llvm, "llvm-objcopy"), f"--dump-section={section}={out}", obj, os.devnull], capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(out):
        return None
    with open(out, "rb") as f:
        return f.read()


def digest(obj, llvm, tmp):
    """{section: sha256 hex} of the gfx950 code object inside the host object `obj`; {} for a unit without device code"""
    fatbin, code = os.path.join(tmp, "fatbin"), os.path.join(tmp, "code.o")
    if not _dump(llvm, obj, ".hip_fatbin", fatbin):
        return {}
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", f"--targets={TARGET}", f"--input={fatbin}", f"--output={code}",
                    "--unbundle"], check=True)
    out = {}
    for section in SECTIONS:
        data = _dump(llvm, code, section, os.path.join(tmp, "section"))
        out[section] = hashlib.sha256(data).hexdigest() if data is not None else "-"
    return out


if __name__ == "__main__":
    objdir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "coati_amd", "build")
    llvm = _llvm_bin()
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(f for f in os.listdir(objdir) if f.endswith(".o")):
            d = digest(os.path.join(objdir, name), llvm, tmp)
            print(name, *(f"{s}={d[s]}" for s in SECTIONS) if d else ("(no device code)",))
