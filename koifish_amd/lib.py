"""ctypes loader for libkf_hip.so / libkf_host.so (built in-tree by koifish_amd/build.py)."""
import ctypes as C
import functools
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
# KF_LIB_DIR (development only: scratch/build_variant.py): a directory holding an A/B build of the two libraries
LIB_HIP = os.path.join(os.environ.get("KF_LIB_DIR", HERE), "libkf_hip.so")
LIB_HOST = os.path.join(os.environ.get("KF_LIB_DIR", HERE), "libkf_host.so")

# typNUMBER (src/g_float.hpp:84-117)
F32, F64, F16, BF16, F8E5M2, F8E4M3, U8, I8, U16, I16, U32, I32, U64, I64, Q4, Q3, Q2, T_SIGN, T_SEQ, BOOL1, T_BINARY, T_BINARY_3, T_BINARY_TILE = range(23)
BITS = {BF16: 16, F8E5M2: 8, Q4: 4, T_SIGN: 2, BOOL1: 1, T_BINARY: 1}
KF_EPI_RESIDUAL = 1
EVO_PSO, EVO_MIX, EVO_PSO_GA = 1, 2, 4   # enum kf_evo_algorithm = the live members of Fuyou_params::ALGORITHM
EVO_ALGORITHMS = {"pso": EVO_PSO, "mix": EVO_MIX, "pso_ga": EVO_PSO_GA}   # Fuyou_params::Algo2Name
ENSEMBLE_AGGREGATION, ENSEMBLE_BRANCH = 0, 1   # kfh_gpt2_eval's mode
QUANT_GROUP, QUANT_ROW_LUT, QUANT_ROW_RTN = 0, 1, 2  # kf_weight.quant
CLIP_OFF, CLIP_REPORT, CLIP_TENSOR, CLIP_GLOBAL = 0, 1, 2, 3   # enum kf_clip_mode (0: the trainers' "off"; kf_grad_norms itself has no such mode)
CLIP_MODES = {None: CLIP_OFF, "report": CLIP_REPORT, "tensor": CLIP_TENSOR, "global": CLIP_GLOBAL}
MODES = ("TP", "ACT_INT8", "ADAPTERS", "KV_INT8", "HOT_MASK", "FUSE0")  # enum koifish::Mode (host/kf_host_modes.hpp), in precedence order
NF4 = 1000  # not a typNUMBER: "Q4 with the normal-float quant card" (QUANT_MODE::RTNf) for the helpers that take a storage type
NF3 = 1001  # the same card at 3 bits (RT_NormalF with bits == 3): layer matrices only, multiplied from the packed stream with kf_set_row_unpack
FMT_Q3R, FMT_Q2R, FMT_Q2N = 9, 10, 11   # kf_kernels.h: the kernel formats of the 3- / 2-bit row forms (kfdbg_rowq_standin)

INCLUDE = os.path.join(HERE, "..", "include")   # kf_abi.h (libkf_hip.so) and kf_host_abi.h (libkf_host.so): the one statement of every signature


class KFError(RuntimeError):
    pass


class Weight(C.Structure):
    """struct kf_weight (include/kf_abi.h)"""
    _fields_ = [("data", C.c_void_p), ("gama", C.c_void_p), ("type", C.c_int32), ("ne0", C.c_int32), ("ne1", C.c_int32), ("nGroup", C.c_int32),
                ("lGroup", C.c_int32), ("qMin", C.c_int32), ("qMax", C.c_int32), ("qBias", C.c_int32), ("qzeros", C.c_void_p), ("qscales", C.c_void_p), ("quant", C.c_int32), ("reserved_", C.c_int32)]


class AttnDocsHeader(C.Structure):
    """struct kf_attn_docs_header (include/kf_abi.h): the first 64 bytes of a table kf_attn_docs_plan wrote; off / n: the forward, dQ and dK/dV tables in entries"""
    _fields_ = ([(f, C.c_int32) for f in ("magic", "n_rows", "n_head", "n_kv", "head_dim", "n_doc", "max_len")] + [("off", C.c_int32 * 3), ("n", C.c_int32 * 3)]
                + [(f, C.c_int32) for f in ("doc_rows", "gap_rows", "reserved_")])


ATTN_DOCS_MAGIC = 0x53434F44
F_IGNORE_LOSS = 0x10000   # MASK_FLAG::F_IGNORE_LOSS: the mask word of a row whose target does not count


class LoraPlan(C.Structure):
    """struct kf::LoraPlan (csrc/kf_lora_plan.h), as kfdbg_lora_plan fills it"""
    _fields_ = ([(f, C.c_int) for f in ("status", "tm", "rows_gx", "rows_block", "rows_lds", "tr_gx", "SA", "SB", "tilesA", "tilesB", "w_gx", "w_block", "w_lds", "fin_gx")]
                + [(f, C.c_longlong) for f in ("off_adelta", "off_aT", "off_bT", "off_partA", "off_partB", "scratch")])


class GradNormPlan(C.Structure):
    """struct kf::GradNormPlan (csrc/kf_gradnorm_plan.h), as kfdbg_gradnorm_plan fills it"""
    _fields_ = [("status", C.c_int), ("bad", C.c_int), ("n_tensors", C.c_int), ("total_wg", C.c_int), ("off_table", C.c_size_t), ("off_part", C.c_size_t), ("bytes", C.c_size_t), ("stamp", C.c_ulonglong)]


# a host drafter of generate_speculative: (ids, n, k, out, user) -> the number of ids proposed (koifish::SpecDecoder::DraftFn)
SPEC_DRAFT_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p)
# what a prototype's text cannot say: (function, parameter index) -> ctypes type
EXPLICIT_ARGTYPES = {("kfh_spec_set_callback", 1): SPEC_DRAFT_FN}
_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "long": C.c_long, "long long": C.c_longlong, "unsigned": C.c_uint,
            "unsigned long long": C.c_ulonglong, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint8_t": C.c_uint8,
            "uint16_t": C.c_uint16, "kf_bf16": C.c_uint16}
_MIRRORS = {"kf_weight": Weight}   # structs with a ctypes mirror here: a T* parameter is POINTER(mirror), so that callers may pass an instance


def _ctype(text, what, mirrors=_MIRRORS):
    """the ctypes type of one parameter ("const kf_weight* w", "int n", "unsigned char handle[64]") or return type ("const char*"; mirrors = {}: a pointer comes
    back as c_void_p); raises on a type it does not know"""
    text, array = re.subn(r"\[\w*\]", "", re.sub(r"\bconst\b", "", text))
    base, stars = " ".join(text.split("*")[0].split()), text.count("*")
    if stars == 0 and base not in _SCALARS:   # a named parameter: the last word is its name
        base = base.rpartition(" ")[0]
    if stars + array:
        return C.c_char_p if (base, stars + array) == ("char", 1) else C.POINTER(mirrors[base]) if base in mirrors and stars + array == 1 else C.c_void_p
    if base not in _SCALARS:
        raise KFError("%s: unknown type %r" % (what, text.strip()))
    return _SCALARS[base]


def parse_header(text):
    """{name: (argtypes, restype)} of every `ret name(params);` a C header declares.  Comments, preprocessor lines, everything inside braces and the typedef / enum /
    struct statements around them are skipped; any other statement that is not a prototype, and any type outside the rule of _ctype, raises."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text.replace("\\\n", " "), flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M).replace('extern "C" {', "")
    while re.search(r"\{[^{}]*\}", text):
        text = re.sub(r"\{[^{}]*\}", "", text)
    out = {}
    for stmt in text.replace("}", "").split(";"):
        stmt = " ".join(stmt.split())
        if not stmt or stmt.split()[0] in ("typedef", "enum", "struct"):
            continue
        m = re.fullmatch(r"([\w\s*]+?)\b(\w+) ?\(([^()]*)\)", stmt)
        if not m:
            raise KFError("not a prototype: %r" % stmt)
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        params = [] if params in ("", "void") else params.split(",")
        out[name] = ([EXPLICIT_ARGTYPES.get((name, i)) or _ctype(p, "%s, parameter %d" % (name, i)) for i, p in enumerate(params)],
                     None if ret == "void" else _ctype(ret, name + ", return type", {}))
    return out


@functools.lru_cache(maxsize=None)
def header_signatures(name):
    """parse_header of include/<name>.  No fallback: a missing header is an error that names the path."""
    path = os.path.join(INCLUDE, name)
    if not os.path.exists(path):
        raise KFError("%s is missing: the ctypes signatures are read from it" % path)
    with open(path) as f:
        return parse_header(f.read())


def __getattr__(name):
    if name == "ABI_SYMBOLS":   # every symbol include/kf_abi.h declares (tests/test_abi_symbols.py checks its own reading of the header against this list and the .so)
        return sorted(header_signatures("kf_abi.h"))
    raise AttributeError(name)


_libs = None


def load():
    """Returns (hip, host) CDLLs, every function a header declares typed from its prototype.  No fallback: a missing library or header is an error the caller must see."""
    global _libs
    if _libs is None:
        for p in (LIB_HIP, LIB_HOST):
            if not os.path.exists(p):
                raise KFError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
                              "koifish_amd has no CPU fallback." % p)
        hip = C.CDLL(LIB_HIP, mode=C.RTLD_GLOBAL)
        host = C.CDLL(os.environ.get("KF_HOST_LIB", LIB_HOST))   # KF_HOST_LIB: the sanitizer build of the host library (tests/test_host_asan_cpu.py)
        for lib, header in ((hip, "kf_abi.h"), (host, "kf_host_abi.h")):
            for name, (argtypes, restype) in header_signatures(header).items():   # getattr raises on a name the library lacks
                f = getattr(lib, name)
                f.argtypes, f.restype = argtypes, restype
        # diagnostics that include/kf_abi.h deliberately leaves out
        hip.kfdbg_gradnorm_plan.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        hip.kfdbg_lora_plan.argtypes = [C.c_int] * 4 + [C.POINTER(LoraPlan)]
        hip.kfdbg_gemv_rows_plan.argtypes = [C.c_void_p, C.c_void_p]
        hip.kfdbg_kv8_plan.argtypes = [C.c_int] * 5 + [C.c_void_p]
        _libs = (hip, host)
    return _libs


def check(rc, what=""):
    if rc != 0:
        hip, _ = load()
        raise KFError("%s failed: code %d: %s" % (what, rc, hip.kf_last_error().decode()))
    return rc
