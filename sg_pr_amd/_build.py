"""Build libsgpr_hip.so (the C-ABI in include/sgpr.h) for gfx950 with hipcc, in-tree.

Every HIP source is compiled to its own object (up to MAX_COMPILERS at once) and the objects are linked into
sg_pr_amd/lib/libsgpr_hip.so.  Staleness is decided by CONTENT, never by timestamps or by where the code runs: the
sha256 of every source, header and the compiler flags is stored next to each object and next to the library
(`*.srchash`); an artefact is reused only while its recorded hash equals the hash of what is on disk now.
`force=True` (or SGPR_FORCE_BUILD=1 in the environment) recompiles everything from scratch.
"""
import collections
import concurrent.futures
import ctypes
import hashlib
import os
import re
import shutil
import subprocess

PKG = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIB_DIR = os.path.join(PKG, "lib")
OBJ_DIR = os.path.join(LIB_DIR, "obj")
LIB_PATH = os.path.join(LIB_DIR, "libsgpr_hip.so")
SOURCES = ["sgpr_embed.hip", "sgpr_score.hip", "sgpr_metrics.hip", "sgpr_modules.hip", "sgpr_cluster.hip",
           "sgpr_generic.hip", "sgpr_wide.hip", "sgpr_prep.hip", "sgpr_train.hip", "sgpr_train_pairs.hip", "sgpr_select.hip",
           "sgpr_seq.hip", "sgpr_peak.hip", "sgpr_verify.hip", "sgpr_consistency.hip", "sgpr_api.hip", "sgpr_posegraph.hip",
           "sgpr_localize.hip", "sgpr_landmarks.hip", "sgpr_landmark_refine.hip", "sgpr_landmark_align.hip",
           "sgpr_landmark_update.hip", "sgpr_landmark_persist.hip", "sgpr_landmark_track.hip", "sgpr_landmark_relocalize.hip",
           "sgpr_landmark_merge.hip"]
HEADERS = [os.path.join(REPO, "include", "sgpr.h"), os.path.join(CSRC, "sgpr_internal.hpp"),
           os.path.join(CSRC, "sgpr_model.hpp"), os.path.join(CSRC, "sgpr_map.hpp"), os.path.join(CSRC, "sgpr_map_grid.hpp"), os.path.join(CSRC, "sgpr_eval.hpp"),
           os.path.join(REPO, "include", "sgpr_localize.h"), os.path.join(REPO, "include", "sgpr_landmarks.h"),
           os.path.join(REPO, "include", "sgpr_landmark_refine.h"), os.path.join(REPO, "include", "sgpr_landmark_align.h"),
           os.path.join(REPO, "include", "sgpr_landmark_update.h"), os.path.join(CSRC, "sgpr_landmark_core.hpp"),
           os.path.join(REPO, "include", "sgpr_landmark_persist.h"), os.path.join(CSRC, "sgpr_landmark_align_core.hpp"),
           os.path.join(REPO, "include", "sgpr_landmark_track.h"), os.path.join(REPO, "include", "sgpr_landmark_relocalize.h"),
           os.path.join(REPO, "include", "sgpr_landmark_merge.h"), os.path.join(REPO, "include", "sgpr_posegraph.h")]
MAX_COMPILERS = 16     # compilers at once: one per source, up to this many
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed"]


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: cannot build libsgpr_hip.so")
    return exe


def _sources():
    return [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]


def _obj(src):
    return os.path.join(OBJ_DIR, os.path.splitext(src)[0] + ".o")


def _hash_of(paths):
    h = hashlib.sha256(" ".join(FLAGS).encode())
    for p in paths:
        h.update(os.path.basename(p).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def source_hash():
    """sha256 over every HIP source, the shared headers and the compiler flags (what the library is a function of)."""
    return _hash_of([os.path.join(CSRC, s) for s in _sources()] + HEADERS)


HeaderAbi = collections.namedtuple("HeaderAbi", "functions constants errors")
_VALUE_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
                "double": ctypes.c_double}
_RETURN_TYPES = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "void": None, "const char*": ctypes.c_char_p}


def parse_header(text):
    """What a C header in the style of include/sgpr.h declares -> HeaderAbi(functions, constants, errors):
    functions [(name, restype, argtypes)] in ctypes terms, one per `ret sgpr_name(args);` - every pointer parameter is
    c_void_p, values are int / int64_t / size_t / float / double, returns int / size_t / void / const char*;
    constants {name: value} of the `#define SGPR_* <integer>` lines; errors {name: value} of the SGPR_OK / SGPR_E_*
    enum.  Only that style is read: comments, preprocessor lines, struct typedefs and the extern "C" brace are dropped.
    A declaration with any other type raises ImportError naming it (ctypes would otherwise pass it as an int)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {m.group(1): int(m.group(2), 0)
                 for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(SGPR_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    errors = {}
    for body in re.findall(r"\benum\s*\{(.*?)\}\s*;", text, re.S):
        for name, value in re.findall(r"(SGPR_\w+)\s*=\s*(-?\d+)", body):
            errors[name] = int(value)
    text = re.sub(r"\benum\s*\{.*?\}\s*;|\btypedef\s+struct\s+\w+\s*(\{.*?\})?\s*\w+\s*;|\bextern\s+\"C\"\s*\{", " ", text,
                  flags=re.S)
    functions = []
    for decl in text.split(";"):
        decl = " ".join(decl.split()).strip("} ")                      # (the closing brace of extern "C")
        if not decl:
            continue
        m = re.fullmatch(r"(.+?) ?\b(sgpr_\w+) ?\((.*)\)", decl)
        if m is None or m.group(1) not in _RETURN_TYPES:
            raise ImportError("C header: cannot bind `%s`: not `int | size_t | void | const char* sgpr_name(...)`" % decl)
        argtypes = []
        for param in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
            words = param.replace("*", " * ").split()
            kind = " ".join(w for w in words[:-1] if w != "const")   # (the last word is the parameter's name)
            if "*" in words[:-1]:
                argtypes.append(ctypes.c_void_p)
            elif kind in _VALUE_TYPES:
                argtypes.append(_VALUE_TYPES[kind])
            else:
                raise ImportError("C header: cannot bind `%s`: parameter `%s` is neither a pointer nor one of %s"
                                  % (decl, param.strip(), ", ".join(_VALUE_TYPES)))
        functions.append((m.group(2), _RETURN_TYPES[m.group(1)], argtypes))
    return HeaderAbi(functions, constants, errors)


def header_abi():
    """parse_header of include/sgpr.h: the one declaration the Python binding follows."""
    with open(HEADERS[0]) as f:
        return parse_header(f.read())


def header_abi_version():
    """SGPR_ABI_VERSION of include/sgpr.h - what a loaded library must answer from sgpr_abi_version()."""
    return header_abi().constants["SGPR_ABI_VERSION"]


def _recorded(path):
    try:
        with open(path + ".srchash") as f:
            return f.read().strip()
    except OSError:
        return None


def is_stale():
    return not os.path.exists(LIB_PATH) or _recorded(LIB_PATH) != source_hash()


def build_library(force=False, verbose=False):
    """Compile every HIP source for gfx950 into sg_pr_amd/lib/libsgpr_hip.so."""
    force = force or os.environ.get("SGPR_FORCE_BUILD", "") not in ("", "0")
    if not force and not is_stale():
        return LIB_PATH
    os.makedirs(OBJ_DIR, exist_ok=True)
    hipcc = _hipcc()
    inc = ["-I" + os.path.join(REPO, "include"), "-I" + CSRC]

    def compile_one(src):
        path, obj = os.path.join(CSRC, src), _obj(src)
        want = _hash_of([path] + HEADERS)
        if not force and os.path.exists(obj) and _recorded(obj) == want:
            return obj
        cmd = [hipcc] + FLAGS + inc + ["-c", path, "-o", obj + ".tmp"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        os.replace(obj + ".tmp", obj)
        with open(obj + ".srchash", "w") as f:
            f.write(want)
        return obj

    total = source_hash()
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(_sources()), MAX_COMPILERS)) as pool:
        objs = list(pool.map(compile_one, _sources()))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB_PATH + ".tmp"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(LIB_PATH + ".tmp", LIB_PATH)
    with open(LIB_PATH + ".srchash", "w") as f:
        f.write(total)
    return LIB_PATH


if __name__ == "__main__":
    import sys
    print(build_library(force="--force" in sys.argv, verbose=True))
