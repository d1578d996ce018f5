// kf_spec.hpp -- the host rules of speculative decoding, pure: no device, no HIP, not kf_host.hpp -- only the status codes of the C ABI and the mode table.
// A round proposes k drafted ids d[0 .. k) behind the sequence's last token t (at position pos), the target verifies [t, d ...] in one pass over its weights
// (Fish::Verify: top1[i] = the target's greedy id behind row i) and the longest prefix of the drafts the target agrees with is kept: spec_clip_k sizes the round,
// spec_accept is the accept rule, spec_lookup the model-free drafter, verify_refusal what Fish::Verify says while a mode it has no form for is on.
// (tests/test_spec_cpu.py reaches them through kfhdbg_spec_*.)
#pragma once
#include <string>

#include "kf_host_modes.hpp"

namespace koifish {

constexpr int KF_SPEC_MAX_K = 7; /* drafted ids per round: with the token in front of them the 8 rows of kf_linear_rows */

// the drafts of a round: k clipped so that the round emits at most the n_left ids still wanted (a round emits up to k + 1) and its last row stays inside the caches
// (rows pos .. pos + k, n_ctx rows); 0: a plain one-row step
inline int spec_clip_k(int k, int n_left, int pos, int n_ctx) {
    if (k > KF_SPEC_MAX_K) k = KF_SPEC_MAX_K;
    if (k > n_left - 1) k = n_left - 1;
    if (k > n_ctx - 1 - pos) k = n_ctx - 1 - pos;
    return k > 0 ? k : 0;
}

// the accept rule: the number of leading drafts with drafts[i] == top1[i] (top1[i]: the target's id behind row i, row 0 = the token in front of the drafts).
// The round then emits top1[0 .. n_acc] -- the accepted drafts and the target's own id behind the last of them -- n_acc + 1 ids
inline int spec_accept(const int* drafts, int k, const int* top1) {
    int n = 0;
    while (n < k && drafts[n] == top1[n]) n++;
    return n;
}

// the lookup drafter: the longest suffix of ids [0, n), at most ngram tokens, that also stands EARLIER in ids proposes the tokens that followed it there -- the most
// recent such place when there are several of that length.  out [k]; returns the number of ids proposed, 0 .. k (fewer than k when the context ends first)
inline int spec_lookup(const int* ids, int n, int ngram, int k, int* out) {
    if (!ids || !out || n < 2 || ngram < 1 || k < 1) return 0;
    for (int g = ngram < n - 1 ? ngram : n - 1; g >= 1; g--) {
        const int* suf = ids + n - g;
        for (int s = n - g - 1; s >= 0; s--) { /* the match ends at s + g <= n - 1: at least one token follows it */
            int j = 0;
            while (j < g && ids[s + j] == suf[j]) j++;
            if (j < g) continue;
            int m = 0;
            while (m < k && s + g + m < n) out[m] = ids[s + g + m], m++;
            return m;
        }
    }
    return 0;
}

// Fish::Verify runs the fused per-layer launches of the plain decode step, R rows at a time: every mode of the table changes what a layer runs, and the verify pass has
// a form for none of them.  KF_OK, or the refusal in the table's own words, naming the first active mode: KF_UNSUPPORTED_DATATYPE for a tensor-parallel rank,
// KF_INVALID_ARGS otherwise; a sampler that is not greedy is refused the same way (acceptance compares greedy ids; rejection sampling is not built)
inline int verify_refusal(unsigned active, bool greedy, const char* entry, std::string& why) {
    for (int m = 0; m < N_MODES; m++) {
        if (!(active & mode_bit(m))) continue;
        why = std::string(entry) + ": " + kModes[m].is_on + " and the verify pass has no " + kModes[m].form + " form: " + kModes[m].undo;
        return m == MODE_TP ? KF_UNSUPPORTED_DATATYPE : KF_INVALID_ARGS;
    }
    if (!greedy) {
        why = std::string(entry) + ": a sampler is set and the verify pass accepts greedy ids only: kfh_set_sampler with temperature 0 first";
        return KF_INVALID_ARGS;
    }
    return KF_OK;
}

}  // namespace koifish
