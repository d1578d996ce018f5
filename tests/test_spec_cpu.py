"""The host rules of speculative decoding (koifish_amd/host/kf_spec.hpp) without a GPU, through kfhdbg_spec_* / kfhdbg_verify_refusal of the host library (which loads
without a device): how a round is sized, the accept rule, the lookup drafter, and what the verify pass says while a mode it has no form for is on.  Every expected
value is written out here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from koifish_amd import lib as L

MODES = ("TP", "ACT_INT8", "ADAPTERS", "KV_INT8", "HOT_MASK", "FUSE0")   # the precedence order of the mode table
IS_ON = {"TP": "tensor-parallel rank", "ACT_INT8": "int8 activations are on", "ADAPTERS": "adapters are attached", "KV_INT8": "the int8 KV cache is on",
         "HOT_MASK": "hot-row mask", "FUSE0": "fuse_level 0"}
UNDO = {"TP": "kfh_tp_init was not called", "ACT_INT8": "kfh_set_act_int8", "ADAPTERS": "clear the adapters", "KV_INT8": "kfh_set_kv_int8 off", "HOT_MASK": "clear the masks",
        "FUSE0": "kfh_set_fuse_level(1)"}
KF_OK, INVALID_ARGS, UNSUPPORTED = 0, -20, -1000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    return L.load()[1]


def arr(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the round's size: k drafts emit up to k + 1 ids, and row pos + k is the last cache row the round writes
@pytest.mark.parametrize("k,n_left,pos,n_ctx,want", [
    (4, 100, 10, 256, 4),     # nothing clips
    (7, 100, 10, 256, 7),
    (9, 100, 10, 256, 7),     # never more than 7 drafts: 8 rows
    (4, 5, 10, 256, 4),       # 5 ids wanted: 4 drafts + the target's own id
    (4, 4, 10, 256, 3),       # clipped by n_new
    (4, 2, 10, 256, 1),
    (4, 1, 10, 256, 0),       # one id wanted: a plain one-row step
    (4, 100, 251, 256, 4),    # rows 251 .. 255: the last cache row
    (4, 100, 252, 256, 3),    # clipped by max_seq
    (4, 100, 254, 256, 1),
    (4, 100, 255, 256, 0),
    (4, 3, 254, 256, 1),      # both
])
def test_clip_k(host, k, n_left, pos, n_ctx, want):
    assert host.kfhdbg_spec_clip_k(k, n_left, pos, n_ctx) == want


# ---- the accept rule: the leading drafts the target agrees with; top1 has one id more than there are drafts
@pytest.mark.parametrize("drafts,top1,want", [
    ([5, 6, 7, 8], [9, 6, 7, 8, 1], 0),     # none: the first draft is wrong, what follows does not count
    ([5, 6, 7, 8], [5, 6, 9, 8, 1], 2),     # some
    ([5, 6, 7, 8], [5, 6, 7, 9, 1], 3),
    ([5, 6, 7, 8], [5, 6, 7, 8, 1], 4),     # all
    ([5], [5, 3], 1),
    ([5], [4, 3], 0),
    ([], [4], 0),                           # a round without drafts
])
def test_accept(host, drafts, top1, want):
    d, t = arr(drafts), arr(top1)
    assert host.kfhdbg_spec_accept(p(d) if d.size else None, d.size, p(t)) == want


def lookup(host, ids, ngram, k):
    a, out = arr(ids), np.full(max(k, 1), -1, dtype=np.int32)
    n = host.kfhdbg_spec_lookup(p(a), a.size, ngram, k, p(out))
    return out[:n].tolist()


def test_lookup_no_match(host):
    assert lookup(host, [1, 2, 3, 4, 5], 3, 4) == []
    assert lookup(host, [7], 3, 4) == [] and lookup(host, [], 3, 4) == []
    assert lookup(host, [1, 2, 1], 3, 0) == []


def test_lookup_match_at_the_very_start(host):
    # the suffix (1, 2, 3) stands at 0: what followed it there is proposed, as far as k and the context go
    ids = [1, 2, 3, 9, 8, 7, 6, 1, 2, 3]
    assert lookup(host, ids, 3, 4) == [9, 8, 7, 6]
    assert lookup(host, ids, 3, 2) == [9, 8]
    assert lookup(host, ids, 3, 7) == [9, 8, 7, 6, 1, 2, 3]   # the context ends first: fewer than k


def test_lookup_longest_of_several_matches(host):
    # (3) alone stands at 2, 5 and 8; (2, 3) at 4 and 7; (1, 2, 3) only at 6: the longest suffix decides, not the nearest place
    ids = [0, 5, 3, 4, 2, 3, 1, 2, 3, 6, 1, 2, 3]
    assert lookup(host, ids, 3, 2) == [6, 1]
    assert lookup(host, ids, 2, 2) == [6, 1]     # (2, 3): the most recent earlier place is 7
    assert lookup(host, ids, 1, 2) == [6, 1]     # (3): the most recent earlier place is 8
    # several places of the SAME length: the most recent one
    ids = [1, 2, 7, 7, 1, 2, 8, 8, 1, 2]
    assert lookup(host, ids, 2, 2) == [8, 8]
    # a shorter suffix is taken only when no longer one matches
    ids = [4, 2, 9, 9, 3, 2]
    assert lookup(host, ids, 3, 3) == [9, 9, 3]


def test_lookup_context_shorter_than_ngram(host):
    assert lookup(host, [5, 5], 3, 3) == [5]          # the suffix is cut to n - 1 = 1 id: (5) stands at 0, one id follows it
    assert lookup(host, [5, 6, 5], 8, 3) == [6, 5]    # suffixes of 2 and 1 ids are tried: (5) stands at 0


# ---- what the verify pass says: every mode of the table is refused, the first active one named in the table's own words
def refusal(host, bits, greedy=1):
    buf = C.create_string_buffer(512)
    return host.kfhdbg_verify_refusal(bits, greedy, buf, 512), buf.value.decode()


def test_verify_refuses_every_mode_and_names_the_first(host):
    assert refusal(host, 0) == (KF_OK, "")
    for bits in range(1, 1 << len(MODES)):
        first = next(m for i, m in enumerate(MODES) if bits >> i & 1)
        rc, why = refusal(host, bits)
        assert rc == (UNSUPPORTED if first == "TP" else INVALID_ARGS), (bits, why)
        assert IS_ON[first] in why and UNDO[first] in why and "the verify pass has no" in why, why
        for other in MODES:
            if other != first:
                assert IS_ON[other] not in why, why


def test_verify_refuses_a_sampler(host):
    rc, why = refusal(host, 0, greedy=0)
    assert rc == INVALID_ARGS and "a sampler is set" in why and "temperature 0" in why
    rc, why = refusal(host, 1 << MODES.index("KV_INT8"), greedy=0)   # a mode is named before the sampler
    assert rc == INVALID_ARGS and IS_ON["KV_INT8"] in why and "sampler" not in why


def test_the_header_stands_alone_under_sanitizers(tmp_path):
    """kf_spec.hpp alone in a stand-alone program under AddressSanitizer + UBSan: the lookup drafter's index arithmetic at every context length, ngram and k of a small
    range, with the output array sized exactly k and the context exactly n, and the other rules beside it"""
    src = tmp_path / "spec.cpp"
    src.write_text('''#include "kf_spec.hpp"
#include <cstdio>
#include <vector>
int main() {
    long sum = 0;
    for (int n = 0; n <= 12; n++)
        for (int ngram = 0; ngram <= 5; ngram++)
            for (int k = 0; k <= 8; k++)
                for (int period = 1; period <= 4; period++) {
                    std::vector<int> ids(n), out(k);
                    for (int i = 0; i < n; i++) ids[i] = i % period;
                    const int m = koifish::spec_lookup(ids.data(), n, ngram, k, out.data());
                    if (m < 0 || m > k) return 1;
                    for (int i = 0; i < m; i++) sum += out[i];
                    sum += m + koifish::spec_clip_k(k, n, n, 12) + koifish::spec_accept(out.data(), m, ids.data() + (n > m ? 0 : n));
                }
    std::string why;
    for (unsigned a = 0; a < 64; a++) sum += koifish::verify_refusal(a, a & 1, "t", why) != 0;
    std::printf("%ld %s\\n", sum, why.c_str());
    return 0;
}
''')
    exe = tmp_path / "spec"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "koifish_amd", "host"),
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode()
    assert "tensor-parallel rank" in out   # the last refusal composed: every mode on
