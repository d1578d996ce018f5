// kf_host_modes.hpp -- the ways koifish::Fish can run a layer, which of them combine, and what a refusal says.  Pure host logic: no device, no HIP, not
// kf_host.hpp -- only the status codes of the C ABI.  Every setter asks mode_refusal, every engine builder engine_refusal, the step sequencing eager_only; nothing
// else in the host library states which modes exclude each other ("Modes").
#pragma once
#include <string>

#include "../../include/kf_abi.h"

namespace koifish {

// In precedence order: when several active modes exclude the one asked for, the first of them is the one a refusal names.
enum Mode { MODE_TP = 0, MODE_ACT_INT8, MODE_ADAPTERS, MODE_KV_INT8, MODE_HOT_MASK, MODE_FUSE0, N_MODES };
constexpr unsigned mode_bit(int m) { return 1u << m; }

struct ModeRow {
    const char* is_on;       // "<this mode> is on"
    const char* subject;     // what runs when this mode is asked for: the thing that "has no <form> form"
    const char* form;        // "... has no <this mode's> form"
    const char* undo;        // how to leave this mode
    unsigned excludes;       // the modes this one does not combine with
    const char* engine_why;  // the persistent engine and the XCD objects do not run this mode, and say this; NULL: they do
    bool eager_only;         // steps run as eager per-layer launches with the position resolved on the host: no engine, no captured graphs
};

namespace mode_bits {
constexpr unsigned TP = mode_bit(MODE_TP), A8 = mode_bit(MODE_ACT_INT8), AD = mode_bit(MODE_ADAPTERS), KV = mode_bit(MODE_KV_INT8), HOT = mode_bit(MODE_HOT_MASK),
                   F0 = mode_bit(MODE_FUSE0);
}
// clang-format off
constexpr ModeRow kModes[N_MODES] = {
    /* TP        tp.world > 1     */ {"this Fish is a tensor-parallel rank", "the tensor-parallel step", "tensor-parallel", "use a Fish that kfh_tp_init was not called on",
                                      mode_bits::A8 | mode_bits::AD | mode_bits::KV, nullptr, false},
    /* ACT_INT8  either switch    */ {"int8 activations are on", "the int8-activation layer body", "int8-activation", "switch kfh_set_act_int8 / kfh_set_act_int8_q4 off first",
                                      mode_bits::TP | mode_bits::AD | mode_bits::KV | mode_bits::HOT, "int8 activations run on the per-layer launches", true},
    /* ADAPTERS  n_adapters > 0   */ {"low-rank adapters are attached", "the layer body that applies adapters", "adapter", "clear the adapters first",
                                      mode_bits::TP | mode_bits::A8 | mode_bits::KV | mode_bits::HOT, "low-rank adapters are attached: they run on the per-layer launches", true},
    /* KV_INT8   kv_int8          */ {"the int8 KV cache is on", "the int8 KV cache", "int8 KV cache", "switch kfh_set_kv_int8 off first",
                                      mode_bits::TP | mode_bits::A8 | mode_bits::AD | mode_bits::HOT | mode_bits::F0, "int8 KV cache runs on the per-layer launches", false},
    /* HOT_MASK  masked_layers > 0*/ {"a hot-row mask is set", "the sparse forward", "sparse", "clear the masks (kfh_set_hot with NULL) first",
                                      mode_bits::A8 | mode_bits::AD | mode_bits::KV, nullptr, false},
    /* FUSE0     fuse_level == 0  */ {"fuse_level 0 is set", "fuse_level 0", "one-launch-per-kernel", "kfh_set_fuse_level(1) first",
                                      mode_bits::KV, nullptr, false},
};
// clang-format on
constexpr bool modes_symmetric() {
    for (int a = 0; a < N_MODES; a++)
        for (int b = 0; b < N_MODES; b++)
            if (((kModes[a].excludes >> b) & 1u) != ((kModes[b].excludes >> a) & 1u) || (a == b && (kModes[a].excludes >> a) & 1u)) return false;
    return true;
}
static_assert(modes_symmetric(), "the exclusion relation is symmetric and no mode excludes itself");

// KF_OK when no active mode excludes `asked`.  Otherwise the refusal, naming the first active mode that does: KF_UNSUPPORTED_DATATYPE when the pair involves a
// tensor-parallel rank, KF_INVALID_ARGS for every other pair; why = "<entry>: <that mode> is on and <what was asked> has no <that mode's> form: <how to leave it>".
inline int mode_refusal(unsigned active, Mode asked, const char* entry, std::string& why) {
    for (int m = 0; m < N_MODES; m++) {
        if (!(active & kModes[asked].excludes & mode_bit(m))) continue;
        why = std::string(entry) + ": " + kModes[m].is_on + " and " + kModes[asked].subject + " has no " + kModes[m].form + " form: " + kModes[m].undo;
        return (m == MODE_TP || asked == MODE_TP) ? KF_UNSUPPORTED_DATATYPE : KF_INVALID_ARGS;
    }
    return KF_OK;
}
// KF_OK, or KF_ENGINE_NOT_SERVED with the first active engine-excluding mode's reason: what EnsureEngine, XcdReplicas and XcdTP ask before they build anything
inline int engine_refusal(unsigned active, std::string& why) {
    for (int m = 0; m < N_MODES; m++)
        if ((active & mode_bit(m)) && kModes[m].engine_why) {
            why = kModes[m].engine_why;
            return KF_ENGINE_NOT_SERVED;
        }
    return KF_OK;
}
inline bool eager_only(unsigned active) {
    for (int m = 0; m < N_MODES; m++)
        if ((active & mode_bit(m)) && kModes[m].eager_only) return true;
    return false;
}

}  // namespace koifish
