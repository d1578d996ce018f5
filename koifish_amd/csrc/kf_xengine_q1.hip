// kf_xengine_q1.hip -- the XCD-confined decode engines on 1-bit and 2-bit PackedQ layers (round 6; 1-bit: BASELINE config 5's storage): the kernel of kf_xengine_kernel.h
// instantiated for FMT_Q1T / FMT_Q2T -- a lane takes ONE DWORD of a 128-element 1-bit block, resp. one 8-byte half of a 64-element 2-bit block (32 weights either way: the
// lanes, slots and canonical chains of a 4-bit matrix, kf_engine.hip's dealing), BlockPrep<FMT> turns it into 16 bf16 pair words through the 256-entry LDS selector table, and
// every sequence of the decoder takes its chain pair over them.  A translation unit of its own, so that the storages' instantiations compile side by side.
#include "kf_xengine_kernel.h"

namespace kf {

template <int FMT, int NWV, int DEPTH, int NB>
using XL1 = XCfg<FMT, 2, 128, NWV, 1024, 2048, 1024, 3072, DEPTH, false, 1, 2, false, NB>; /* Qwen3-0.6B */
template <int FMT, int NWV, int DEPTH, int NB>
using XL2 = XCfg<FMT, 2, 64, NWV, 256, 256, 128, 512, DEPTH, false, 1, 2, false, NB>;       /* the 256-wide test shape */

// the low-bit entries of the table of forms (kf_xengine.hip xengine_form picks among them): one / two / four sequences per decoder, the default forms of the 4-bit engines
#define XE_LOWBIT_FORMS(F) xe_form<XL1<F, 12, 2, 1>>(1), xe_form<XL1<F, 12, 4, 2>>(1), xe_form<XL1<F, 12, 2, 4>>(1), xe_form<XL2<F, 12, 2, 1>>(2), xe_form<XL2<F, 12, 4, 2>>(2), xe_form<XL2<F, 12, 2, 4>>(2)
const XForm* xe_forms_lowbit(int* n) {
    static const XForm forms[] = {XE_LOWBIT_FORMS(FMT_Q1T), XE_LOWBIT_FORMS(FMT_Q2T)};
    *n = sizeof(forms) / sizeof(forms[0]);
    return forms;
}
#undef XE_LOWBIT_FORMS

}  // namespace kf
