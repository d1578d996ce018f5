// kf_gemm_awq.hip -- token batches on the AutoAWQ GEMM-format tensors as they are stored (Qwen3-*-AWQ checkpoints), gfx950 / wave64.
//
//   y[t, o] = sum_i x[t, i] W[i, o],   W[i, o] = bf16((q[i, o] - z[i / 128, o]) * float(s[i / 128, o]))      (CU_Q42X_awq; kf_awq.hip forms the same bits)
//
// qweight is int32 [in, out / 8]: the matrix lies k-major, a dword holds eight OUTPUTS of one input row (output 8 c + j in nibble ORDER[j], ORDER = {0,4,1,5,2,6,3,7}),
// while an operand of v_mfma_f32_16x16x32_bf16 wants eight consecutive k of one output per lane.  The transpose costs nothing: it is the choice of the output a lane
// stands for.  In an MFMA step over input rows k0 .. k0 + 31 and word columns c0 .. c0 + 15, lane (r16, q4) gathers the eight words of rows k0 + 8 q4 .. + 7 at word
// column c0 + r16 and takes nibble ORDER[j] of each: fragment j = eight consecutive k of output 8 (c0 + r16) + j.  The eight fragments are the B operands (columns =
// outputs) of eight accumulator tiles against the same x fragment (rows = tokens), so column r16 of tile j is output 8 (c0 + r16) + j: a lane ends with EIGHT
// CONSECUTIVE outputs of each of its token rows 4 q4 + i -- one 16-byte store a row, and bias / residual / prior y are read at the same eight places.  No weight moves
// between lanes.
//
// A workgroup owns 8 WC outputs x BT tokens over the whole of K (AwqCfg, kf_gemm_plan.h: no split over k between workgroups, no atomics, one launch): it reads every
// packed word of its WC word columns once, VW words a load (16 bytes where a row has a multiple of four words, single words otherwise), and stages the RAW words and the
// x rows through two LDS buffers -- the next stage's global loads are in flight while a stage is multiplied, one barrier a stage.
//
// Dequantised per wave, in registers, not once per workgroup into a bf16 LDS image: the waves of a workgroup are dealt over the outputs first (wide form: 2 x 2, a wave
// holds 128 outputs x 64 tokens = 32 accumulator tiles), so a word is unpacked by two waves, not by all -- and the image would cost an LDS write and a read per
// weight plus a second barrier per stage, eight times the raw words' LDS bytes.  z and s of a lane's eight outputs are unpacked once per 128-row group into sixteen
// registers; a weight is then one byte -> fp32 conversion (v_cvt_f32_ubyteN of the nibble-masked word), the subtract, the multiply (exact in fp32: 5 bits x 11 bits)
// and half a v_cvt_pk_bf16_f32: ONE rounding.
//
// Forms (kf_gemm_plan.h awq_kern chooses; resources: DESIGN.md):
//   narrow  16 outputs x 32 tokens, the four waves take the four 32-row k-steps of a 128-row group and are summed in wave order through LDS; two of a step's sixteen
//           word columns are used -- batches of 16 .. 127 rows are bound by the stream of qweight and by workgroups over `out`, not by MFMA issue
//   wide    256 outputs x 128 tokens, 64-row stages
// fp32 accumulation in MFMA order, a fixed function of the operands and the plan: same call, same bits.
#include "kf_gemm_common.h"

namespace kf {

struct AwqArgs {
    const uint32_t *qw, *qz;
    const uint16_t *sc, *x;
    uint16_t* y;
    const uint16_t *bias, *res;
    float alpha, beta;
    int K, out, n;
};

template <class C>
__global__ void __launch_bounds__(C::NTH) awq_tile_kernel(const AwqArgs a) {
    constexpr int KS = C::KS, WS = C::WS, XS = C::XS, VW = C::VW, TT = C::TT, NTH = C::NTH;
    constexpr int XCH = C::BT * (KS / 8) / NTH;                 /* 16-byte chunks of x per thread and stage */
    constexpr int NWCH = KS * (C::WC / VW), WCH = (NWCH + NTH - 1) / NTH; /* VW-word chunks of qweight per stage; per thread */
    static_assert(C::BT * (KS / 8) % NTH == 0, "x chunks");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, q4 = lane >> 4;
    const int wk = wave % C::WK, wt = (wave / C::WK) % C::WT, wo = wave / (C::WK * C::WT);
    const int w8 = a.out >> 3, col0 = blockIdx.x * C::WC, tok0 = blockIdx.y * C::BT;
    const bool used = r16 < C::WCU;                              /* an idle column repeats the last used one: its products are dropped */
    const int lc = wo * C::WCU + (used ? r16 : C::WCU - 1), cg = col0 + lc;
    const bool colok = cg < w8;                                  /* past `out`: zero words in LDS, zero scales, nothing stored */
    const bool vec = w8 % VW == 0;                               /* a row segment starts on a VW-word boundary */

    uint32_t wreg[WCH][VW];
    u32x4 xreg[XCH];
    uint32_t zpend = 0;
    u32x4 spend = u32x4{0u, 0u, 0u, 0u};
    auto fetch = [&](int st) { /* stage st: global -> registers */
        const int k0 = st * KS;
#pragma unroll
        for (int u = 0; u < WCH; u++) {
            const int i = tid + u * NTH, row = i / (C::WC / VW), c = (i % (C::WC / VW)) * VW;
#pragma unroll
            for (int v = 0; v < VW; v++) wreg[u][v] = 0u;
            if (NWCH % NTH != 0 && i >= NWCH) continue;
            const uint32_t* p = a.qw + (size_t)(k0 + row) * w8 + col0 + c;
            if (vec) {
                if (col0 + c < w8) {
                    if constexpr (VW == 4) {
                        const u32x4 t = *reinterpret_cast<const u32x4*>(p);
                        wreg[u][0] = t.x, wreg[u][1] = t.y, wreg[u][2] = t.z, wreg[u][3] = t.w;
                    } else if constexpr (VW == 2) {
                        const u32x2 t = *reinterpret_cast<const u32x2*>(p);
                        wreg[u][0] = t.x, wreg[u][1] = t.y;
                    } else {
                        wreg[u][0] = p[0];
                    }
                }
            } else {
#pragma unroll
                for (int v = 0; v < VW; v++)
                    if (col0 + c + v < w8) wreg[u][v] = p[v];
            }
        }
#pragma unroll
        for (int u = 0; u < XCH; u++) {
            const int i = tid + u * NTH, tok = tok0 + i / (KS / 8), kc = (i % (KS / 8)) * 8;
            xreg[u] = tok < a.n ? *reinterpret_cast<const u32x4*>(a.x + (size_t)tok * a.K + k0 + kc) : u32x4{0u, 0u, 0u, 0u};
        }
        if ((k0 & 127) == 0 && colok) { /* the stage opens a group: its zeros word and eight fp16 scales */
            const int g = k0 >> 7;
            zpend = a.qz[(size_t)g * w8 + cg];
            spend = *reinterpret_cast<const u32x4*>(a.sc + (size_t)g * a.out + (size_t)cg * 8);
        }
    };
    auto stash = [&](int buf) { /* registers -> LDS buffer buf */
        uint32_t* wl = reinterpret_cast<uint32_t*>(smem + buf * C::STAGE);
        uint16_t* xl = reinterpret_cast<uint16_t*>(smem + buf * C::STAGE + C::W_BYTES);
#pragma unroll
        for (int u = 0; u < WCH; u++) {
            const int i = tid + u * NTH, row = i / (C::WC / VW), c = (i % (C::WC / VW)) * VW;
            if (NWCH % NTH != 0 && i >= NWCH) continue;
            if constexpr (VW >= 2) { /* WS and c are even: 8-byte stores */
#pragma unroll
                for (int v = 0; v < VW; v += 2) *reinterpret_cast<u32x2*>(wl + row * WS + c + v) = u32x2{wreg[u][v], wreg[u][v + 1]};
            } else {
                wl[row * WS + c] = wreg[u][0];
            }
        }
#pragma unroll
        for (int u = 0; u < XCH; u++) {
            const int i = tid + u * NTH;
            *reinterpret_cast<u32x4*>(xl + (i / (KS / 8)) * XS + (i % (KS / 8)) * 8) = xreg[u];
        }
    };

    f32x4 acc[8][TT];
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
        for (int tt = 0; tt < TT; tt++) acc[j][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float zf[8], sf[8]; /* the group's zeros and scales of this lane's eight outputs, j order */
#pragma unroll
    for (int j = 0; j < 8; j++) zf[j] = 0.f, sf[j] = 0.f;

    const int nst = a.K / KS;
    fetch(0);
    stash(0);
    __syncthreads();
    for (int st = 0; st < nst; st++) {
        if (((st * KS) & 127) == 0) { /* before the next fetch overwrites them */
            const uint32_t zl = zpend & 0x0F0F0F0Fu, zh = (zpend >> 4) & 0x0F0F0F0Fu;
            const uint32_t sw[4] = {spend.x, spend.y, spend.z, spend.w};
#pragma unroll
            for (int j = 0; j < 8; j++) {
                zf[j] = (float)((((j >> 1) & 1 ? zh : zl) >> (8 * ((j & 1) * 2 + (j >> 2)))) & 0xffu);
                sf[j] = half_bits_to_f32((j & 1) ? sw[j >> 1] >> 16 : sw[j >> 1] & 0xffffu);
            }
        }
        if (st + 1 < nst) fetch(st + 1);
        const uint32_t* wl = reinterpret_cast<const uint32_t*>(smem + (st & 1) * C::STAGE);
        const uint16_t* xl = reinterpret_cast<const uint16_t*>(smem + (st & 1) * C::STAGE + C::W_BYTES);
#pragma unroll
        for (int ks0 = 0; ks0 < KS / 32; ks0 += C::WK) {
            const int ks = ks0 + wk;
            uint32_t lo[8], hi[8]; /* byte b of lo: nibble 2 b, of hi: nibble 2 b + 1 */
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const uint32_t w = wl[(ks * 32 + 8 * q4 + r) * WS + lc];
                lo[r] = w & 0x0F0F0F0Fu, hi[r] = (w >> 4) & 0x0F0F0F0Fu;
                asm("" : "+v"(lo[r])); /* opaque masks keep the byte extractions as v_cvt_f32_ubyteN (see kf_gemv.hip) */
                asm("" : "+v"(hi[r]));
            }
            bf16x8 xf[TT];
#pragma unroll
            for (int tt = 0; tt < TT; tt++) xf[tt] = *reinterpret_cast<const bf16x8*>(xl + ((wt * TT + tt) * 16 + r16) * XS + ks * 32 + 8 * q4);
#pragma unroll
            for (int j = 0; j < 8; j++) { /* output 8 cg + j: nibble ORDER[j] = byte (j & 1) * 2 + (j >> 2) of lo (j & 2 == 0) or hi */
                const int sh = 8 * ((j & 1) * 2 + (j >> 2));
                float f[8];
#pragma unroll
                for (int r = 0; r < 8; r++) f[r] = ((float)((((j >> 1) & 1 ? hi[r] : lo[r]) >> sh) & 0xffu) - zf[j]) * sf[j];
                const u32x4 frag = u32x4{pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7])};
#pragma unroll
                for (int tt = 0; tt < TT; tt++) acc[j][tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[tt], __builtin_bit_cast(bf16x8, frag), acc[j][tt], 0, 0, 0);
            }
        }
        if (st + 1 < nst) stash((st + 1) & 1); /* the buffer stage st - 1 was read from: every wave passed the barrier that closed it */
        __syncthreads();
    }

    if constexpr (C::WK > 1) { /* the k-slices of a tile, summed in wave order: ((w0 + w1) + w2) + w3 */
        float* red = reinterpret_cast<float*>(smem);
        const int slot = ((wo * C::WT + wt) * 4 + q4) * C::WCU + r16; /* used lanes only */
        constexpr int PER = 8 * TT * 4, SLICE = C::WO * C::WT * 4 * C::WCU * PER;
        if (wk > 0 && used) {
#pragma unroll
            for (int j = 0; j < 8; j++)
#pragma unroll
                for (int tt = 0; tt < TT; tt++) *reinterpret_cast<f32x4*>(red + (wk - 1) * SLICE + slot * PER + (j * TT + tt) * 4) = acc[j][tt];
        }
        __syncthreads();
        if (wk > 0) return;
        if (used) {
#pragma unroll
            for (int s = 1; s < C::WK; s++)
#pragma unroll
                for (int j = 0; j < 8; j++)
#pragma unroll
                    for (int tt = 0; tt < TT; tt++) acc[j][tt] += *reinterpret_cast<const f32x4*>(red + (s - 1) * SLICE + slot * PER + (j * TT + tt) * 4);
        }
    }

    // lane (r16, q4): token rows 4 q4 + i of its TT tiles, outputs 8 cg .. 8 cg + 7 (tile j = output 8 cg + j)
    if (!used || !colok) return;
    const bool vec_y = (reinterpret_cast<uintptr_t>(a.y) & 15) == 0;
    const size_t o0 = (size_t)cg * 8;
#pragma unroll
    for (int tt = 0; tt < TT; tt++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int tok = tok0 + (wt * TT + tt) * 16 + 4 * q4 + i;
            if (tok >= a.n) continue;
            uint16_t* yp = a.y + (size_t)tok * a.out;
            uint16_t o[8];
#pragma unroll
            for (int j = 0; j < 8; j++) o[j] = linear_out_bf16(acc[j][tt][i], a.alpha, a.beta, yp, o0 + j, a.bias, o0 + j, a.res, (size_t)tok * a.out + o0 + j);
            if (vec_y) {
                *reinterpret_cast<u32x4*>(yp + o0) = u32x4{(uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16),
                                                            (uint32_t)o[4] | ((uint32_t)o[5] << 16), (uint32_t)o[6] | ((uint32_t)o[7] << 16)};
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++) yp[o0 + j] = o[j];
            }
        }
}

template <class C>
static int awq_run(hipStream_t st, const GemmKern& k, const AwqArgs& a) {
    static_assert(C::LDS <= 64 * 1024, "more dynamic LDS than a launch gets without hipFuncSetAttribute");
    hipLaunchKernelGGL(awq_tile_kernel<C>, dim3(k.gx, k.gy), dim3(k.block), k.lds, st, a);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

int awq_tile_launch(hipStream_t st, const GemmKern& k, const kf_weight* w, const uint16_t* x, int n, uint16_t* y, const uint16_t* bias, float alpha, float beta,
                    const uint16_t* residual) {
    int r = awq_check(w);
    if (r) return r;
    if (k.fam != GK_AWQ) return KF_INVALID_ARGS;
    const AwqArgs a = {(const uint32_t*)w->data, (const uint32_t*)w->qzeros, (const uint16_t*)w->qscales, x, y, bias, residual, alpha, beta, w->ne1, w->ne0, n};
    return k.form == AWQ_WIDE.bt ? awq_run<AwqWide>(st, k, a) : awq_run<AwqNarrow>(st, k, a);
}

}  // namespace kf
