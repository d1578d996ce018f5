"""Shared by tests/test_fixed_exponent_cpu.py and tests/test_gpu_engine_fixed_exponent.py: builds tests/fixed_exponent_ref.c -- the CPU oracle's source plus a restatement of
its canonical attention against the fixed exponent, and a record of the largest |n| the oracle's own canonical attention meets."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_CFLAGS = "-O2 -std=c11 -fPIC -fopenmp -ffp-contract=off -fno-fast-math -mavx2 -mfma -mf16c -Wall -Wextra -fvisibility=hidden".split()   # oracle/Makefile
LIM = 448.0   # KF_CANON_FIX_LIM (koifish_amd/csrc/kf_attn_common.h)


def build_ref(directory):
    """the helper library inside `directory` (a temporary one); returns its path"""
    so = os.path.join(str(directory), "libfixed_exponent_ref.so")
    subprocess.check_call(["gcc"] + ORACLE_CFLAGS + ["-shared", "-o", so, os.path.join(HERE, "fixed_exponent_ref.c"), "-lm"])
    return so


def load_ref(so):
    lib = C.CDLL(so)
    lib.kfx_attn_decode_fixed.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.POINTER(C.c_float)]
    lib.kfx_attn_decode_fixed.restype = C.c_int
    lib.kfx_max_abs_n.argtypes = [C.c_int]
    lib.kfx_max_abs_n.restype = C.c_float
    return lib
