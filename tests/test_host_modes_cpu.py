"""The host decoder's mode table (koifish_amd/host/kf_host_modes.hpp) without a GPU: for every set of active modes and every mode asked for, whether the call is
refused, with which status, naming which mode, and with the phrases the GPU tests match; the engines' refusals; the eager-only set.  The ten excluded pairs, the
precedence order and the texts are written out HERE, not read from the library: the table is checked against them, through kfhdbg_mode_refusal /
kfhdbg_engine_refusal / kfhdbg_eager_only of the host library (which loads without a device).  Last, the header alone in a stand-alone program under
AddressSanitizer + UBSan: it needs nothing but the ABI header's status codes."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from koifish_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("TP", "ACT_INT8", "ADAPTERS", "KV_INT8", "HOT_MASK", "FUSE0")   # the precedence order
PAIRS = {frozenset(p) for p in (
    ("TP", "ACT_INT8"), ("TP", "ADAPTERS"), ("TP", "KV_INT8"), ("ACT_INT8", "ADAPTERS"), ("ACT_INT8", "KV_INT8"), ("ACT_INT8", "HOT_MASK"),
    ("ADAPTERS", "KV_INT8"), ("ADAPTERS", "HOT_MASK"), ("KV_INT8", "HOT_MASK"), ("KV_INT8", "FUSE0"))}
ALLOWED = {frozenset(p) for p in (("TP", "HOT_MASK"), ("TP", "FUSE0"), ("ACT_INT8", "FUSE0"), ("ADAPTERS", "FUSE0"), ("HOT_MASK", "FUSE0"))}
IS_ON = {"TP": "tensor-parallel rank", "ACT_INT8": "int8 activations are on", "ADAPTERS": "adapters are attached", "KV_INT8": "the int8 KV cache is on",
         "HOT_MASK": "hot-row mask", "FUSE0": "fuse_level 0"}   # what a refusal says of the active mode it names: the substrings the GPU tests match
ENGINE_WHY = {"ACT_INT8": "int8 activations run on the per-layer launches", "ADAPTERS": "adapters", "KV_INT8": "int8 KV cache runs on the per-layer launches"}
EAGER_ONLY = {"ACT_INT8", "ADAPTERS"}
KF_OK, INVALID_ARGS, UNSUPPORTED, ENGINE_NOT_SERVED = 0, -20, -1000, 1


@pytest.fixture(scope="module")
def host():
    return L.load()[1]


def active_sets():
    for bits in range(1 << len(MODES)):
        yield bits, [m for i, m in enumerate(MODES) if bits >> i & 1]


def refusal(host, bits, asked):
    buf = C.create_string_buffer(512)
    return host.kfhdbg_mode_refusal(bits, MODES.index(asked), buf, 512), buf.value.decode()


def test_the_pairs_written_here_are_the_fifteen():
    assert len(PAIRS) == 10 and len(ALLOWED) == 5 and not PAIRS & ALLOWED
    assert PAIRS | ALLOWED == {frozenset(p) for p in itertools.combinations(MODES, 2)}
    assert L.MODES == MODES


def test_every_active_set_and_every_mode_asked(host):
    """64 active sets x 6 modes asked: refused exactly when an active mode is paired with the one asked; the status; the mode named; its phrase"""
    n_refused = 0
    for bits, active in active_sets():
        for asked in MODES:
            rc, why = refusal(host, bits, asked)
            excluders = [m for m in active if frozenset((m, asked)) in PAIRS]
            if not excluders:
                assert rc == KF_OK and why == "", (active, asked, rc, why)
                continue
            n_refused += 1
            named = excluders[0]   # active is in precedence order
            assert rc == (UNSUPPORTED if "TP" in (named, asked) else INVALID_ARGS), (active, asked, rc)
            assert why.startswith("kfhdbg: ") and IS_ON[named] in why, (active, asked, why)
            for m in excluders[1:]:   # only the first is named
                assert IS_ON[m] not in why, (active, asked, why)
    assert n_refused == sum(1 for _, active in active_sets() for asked in MODES if any(frozenset((m, asked)) in PAIRS for m in active))


def test_the_relation_is_symmetric_and_no_mode_excludes_itself(host):
    for a in MODES:
        assert refusal(host, 1 << MODES.index(a), a)[0] == KF_OK
        for b in MODES:
            ab, ba = refusal(host, 1 << MODES.index(a), b)[0], refusal(host, 1 << MODES.index(b), a)[0]
            assert ab == ba and (ab != KF_OK) == (frozenset((a, b)) in PAIRS), (a, b, ab, ba)


def test_the_phrases_the_gpu_tests_match(host):
    one = lambda m: 1 << MODES.index(m)
    for asked in ("ACT_INT8", "ADAPTERS", "HOT_MASK", "FUSE0", "TP"):
        assert "the int8 KV cache is on" in refusal(host, one("KV_INT8"), asked)[1]
    assert "fuse_level 0 has no int8 KV cache form" in refusal(host, one("KV_INT8"), "FUSE0")[1]
    for active, phrase in IS_ON.items():
        if active != "KV_INT8":
            assert phrase in refusal(host, one(active), "KV_INT8")[1], active
    for active in ("ADAPTERS", "KV_INT8", "HOT_MASK"):   # kfh_set_hot / kfh_set_act_int8 against each other and the rest
        assert IS_ON[active] in refusal(host, one(active), "ACT_INT8")[1]
    assert IS_ON["ACT_INT8"] in refusal(host, one("ACT_INT8"), "HOT_MASK")[1]
    for active in MODES:   # every refusal kfh_set_adapter returns says "adapters"
        rc, why = refusal(host, one(active), "ADAPTERS")
        assert (rc == KF_OK) or "adapters" in why, (active, why)
    assert host.kfhdbg_mode_refusal(0, len(MODES), None, 0) == INVALID_ARGS and host.kfhdbg_mode_refusal(0, -1, None, 0) == INVALID_ARGS   # no such mode


def test_engines_and_eager_only(host):
    for bits, active in active_sets():
        buf = C.create_string_buffer(256)
        rc = host.kfhdbg_engine_refusal(bits, buf, 256)
        blockers = [m for m in active if m in ENGINE_WHY]
        if blockers:
            assert rc == ENGINE_NOT_SERVED and ENGINE_WHY[blockers[0]] in buf.value.decode(), (active, buf.value)
        else:
            assert rc == KF_OK and buf.value == b"", (active, buf.value)
        assert host.kfhdbg_eager_only(bits) == int(any(m in EAGER_ONLY for m in active)), active


def test_the_header_stands_alone_under_sanitizers(tmp_path):
    src = tmp_path / "modes.cpp"
    src.write_text('#include "kf_host_modes.hpp"\n#include <cstdio>\nint main() {\n  std::string why;\n'
                   '  int n = 0;\n  for (unsigned a = 0; a < 64; a++) for (int m = 0; m < koifish::N_MODES; m++) n += koifish::mode_refusal(a, (koifish::Mode)m, "t", why) != 0;\n'
                   '  n += koifish::engine_refusal(63, why) + koifish::eager_only(6);\n  std::printf("%d %s\\n", n, why.c_str());\n  return 0;\n}\n')
    exe = tmp_path / "modes"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "koifish_amd", "host"),
                           str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split(" ", 1)
    refused = sum(1 for _, active in active_sets() for asked in MODES if any(frozenset((m, asked)) in PAIRS for m in active))
    assert int(out[0]) == refused + ENGINE_NOT_SERVED + 1 and out[1].strip() == ENGINE_WHY["ACT_INT8"]
