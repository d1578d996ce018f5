"""The ctypes signatures without a GPU: koifish_amd/lib.py reads them from the two C headers (include/kf_abi.h for libkf_hip.so, include/kf_host_abi.h for
libkf_host.so, which the host sources include, so the compiler holds the definitions to the same text).  Every declared function is typed, the type rule is pinned on
signatures written out here by hand from the headers, an unknown type is an error, and the host library exports what its header declares -- no more, no less."""
import ctypes as C
import os
import re

import pytest

from koifish_amd import lib as L
from test_abi_symbols import exported

P, I, F, D, Z, W = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t, C.POINTER(L.Weight)
HEADERS = ("kf_abi.h", "kf_host_abi.h")


def test_every_declared_function_is_typed():
    for lib, header in zip(L.load(), HEADERS):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(L.INCLUDE, header)).read(), flags=re.S)
        sigs = L.header_signatures(header)
        assert len(sigs) > 150
        for name, (argtypes, restype) in sigs.items():
            f = getattr(lib, name)
            assert f.argtypes is not None and list(f.argtypes) == argtypes and f.restype == restype, name
            (params,) = re.findall(r"\b%s\(([^()]*)\)" % name, text)   # one prototype each, none with a parenthesis among its parameters
            assert len(f.argtypes) == (0 if params.strip() in ("", "void") else params.count(",") + 1), name


def test_pinned_signatures():
    hip, host = L.load()
    for f, argtypes, restype in (
            (hip.kf_linear, [P, W, P, P, P, I, F, F, C.c_uint32, P], I),
            (hip.kf_adamw, [P] * 5 + [Z, I] + [F] * 8 + [C.c_uint32, P], I),
            (hip.kf_attn_backward, [P] * 4 + [C.c_longlong, P, P, C.c_longlong, P, P, P, C.c_longlong, I, I, I, I, I, P], I),
            (hip.kf_memset, [P, P, I, Z], I),
            (hip.kf_tp_recv_bytes, [I, I], Z),
            (hip.kf_xengine_workspace_bytes, [P], Z),
            (hip.kf_last_error, [], C.c_char_p),
            (hip.kf_tp_ipc_export, [P, P, P], I),   # unsigned char handle[64]
            (hip.kf_norm_linear, [P, P, P, F, I, P, P, P, I, P], I),   # const kf_weight* const* is no single-level pointer
            (host.kfh_create, [I, P] + [I] * 8 + [F] * 3 + [P], P),
            (host.kfh_destroy, [P], None),
            (host.kfh_qwen3t_step, [P, P, P, F, D, D, F, F, C.c_uint32], I),
            (host.kfh_gpt2_step, [P, P, P, F, D, D, F, F, C.c_uint32], I),
            (host.kfh_qwen3t_set_param_gama, [P, I, P, P, P, W], I),
            (host.kfh_st_info, [P, I, C.c_char_p, I, C.c_char_p, I, P, P, P, P], I),
            (host.kfh_spec_set_callback, [P, L.SPEC_DRAFT_FN, P], I)):
        assert list(f.argtypes) == argtypes and f.restype == restype, f.__name__


def test_type_rule():
    sigs = L.parse_header("""
        /* a comment with a call(in, it); */
        #define KF_MACRO(x) \\
            int not_a_prototype(x);
        typedef struct kf_s { int a; struct { int b; } c; } kf_s;
        enum { KF_A = 1 };
        typedef int (*fn_t)(int);
        const char* f_text(const char* s, char** out);
        void f_none(void);
        unsigned long long f_wide(long long a, unsigned b, uint8_t c, uint16_t d, kf_bf16 e, int64_t f, uint64_t g, int32_t h, long i, double j, int);
        kf_weight* f_ptr(const kf_weight* w, kf_weight** ws, const kf_s* s, float x[4]);
    """)
    assert sigs == {"f_text": ([C.c_char_p, P], C.c_char_p), "f_none": ([], None),
                    "f_wide": ([C.c_longlong, C.c_uint, C.c_uint8, C.c_uint16, C.c_uint16, C.c_int64, C.c_uint64, C.c_int32, C.c_long, D, I], C.c_ulonglong),
                    "f_ptr": ([W, P, P, P], P)}


@pytest.mark.parametrize("text", ["int f(kf_unknown_t x);", "kf_unknown_t f(int x);", "int f(int x, short y);", "int f(fn_t cb);", "int x = 3;"])
def test_unknown_type_raises(text):
    """never a default: a by-value type outside the rule (a function pointer's typedef among them: those go into L.EXPLICIT_ARGTYPES) and a statement that is no
    prototype are errors"""
    with pytest.raises(L.KFError):
        L.parse_header(text)


def test_missing_header_is_an_error_that_names_the_path():
    with pytest.raises(L.KFError, match="no_such_header.h"):
        L.header_signatures("no_such_header.h")


def test_host_header_and_library_agree():
    """test_abi_symbols.test_header_and_library_agree for libkf_host.so: the exported kfh* symbols are the header's names, in both directions"""
    decl = set(L.header_signatures("kf_host_abi.h"))
    exp = {f for f in exported(L.LIB_HOST) if f.startswith("kfh")}
    assert decl and not decl - exp, "declared in kf_host_abi.h but not exported: %s" % sorted(decl - exp)
    assert not exp - decl, "exported but not declared in kf_host_abi.h: %s" % sorted(exp - decl)
