/* The canonical decode attention restated against the FIXED reference exponent 0 (koifish_amd/csrc/kf_attn_common.h, KF_CANON_FIX_LIM), with the sums dealt as the
 * persistent engine deals them: 64-key slices; inside a slice 8 waves x 4 key groups, the keys interleaved (wave w, group g: t0 + 4 w + g + 32 u); a lane's keys in
 * order, the four groups joined pairwise, the waves in order, the slices in four quarters joined by two quad adds.  No maximum anywhere: p = ldexp(f, n).
 * Built by tests/fixed_exponent.py with the oracle's flags; it includes the oracle's source and changes nothing there.
 * The library is also a whole oracle whose canonical attention reports the largest |n| it has met (kfx_max_abs_n): the oracle's only use of kfo_exp2_parts is the
 * softmax weight of mode CANON, and it is routed through a recording twin here -- same values out. */
#include "../oracle/kfo_math.h"
static float kfx_seen_max_abs_n;
static inline void kfx_exp2_parts_recording(float y, float* f, float* n) {
    kfo_exp2_parts(y, f, n);
    const float a = *n != *n ? INFINITY : fabsf(*n);
#pragma omp critical(kfx_seen)
    if (a > kfx_seen_max_abs_n) kfx_seen_max_abs_n = a;
}
#define kfo_exp2_parts kfx_exp2_parts_recording
#include "../oracle/kf_oracle.c"

/* the largest |n| (NaN counts as +inf) of every valid key since the last reset */
KFO_API float kfx_max_abs_n(int reset) {
    const float r = kfx_seen_max_abs_n;
    if (reset) kfx_seen_max_abs_n = 0.f;
    return r;
}

#define FX_LIM 448.0f
#define FX_CHUNK 64
#define FX_MAXSP 32

/* returns 1 when a valid key's exponent lies outside [-FX_LIM, FX_LIM] (the guard); *max_abs_n: the largest |n| met (NaN counts as +inf) */
KFO_API int kfx_attn_decode_fixed(const uint16_t* q, const uint16_t* kc, const uint16_t* vc, uint16_t* out, int pos, int n_head, int n_kv, int hd, int kv_stride,
                                  float* max_abs_n) {
    const int kv_mul = n_head / n_kv, len = pos + 1, LPK = hd / 8, KPW = 64 / LPK, NW = 8, nsp = (len + FX_CHUNK - 1) / FX_CHUNK;
    const float rden = 1.0f / sqrtf((float)hd);
    int guard = 0;
    float amax = 0.f;
    if (nsp > FX_MAXSP || hd > 128) return -1;
    for (int h = 0; h < n_head; h++) {
        const int kvh = h / kv_mul;
        float qf[128];
        for (int i = 0; i < hd; i++) qf[i] = kfo_bf16_to_f32(q[(size_t)h * hd + i]);
        double So[FX_MAXSP][128];
        double Sl[FX_MAXSP];
        for (int sp = 0; sp < FX_MAXSP; sp++) { /* slices behind the position publish zeros */
            Sl[sp] = 0.0;
            for (int i = 0; i < hd; i++) So[sp][i] = 0.0;
        }
        for (int sp = 0; sp < nsp; sp++) {
            const int t0 = sp * FX_CHUNK, t1 = t0 + FX_CHUNK < len ? t0 + FX_CHUNK : len;
            double Wo[128], Wl = 0.0; /* the eight waves' sums, in order */
            for (int i = 0; i < hd; i++) Wo[i] = 0.0;
            for (int w = 0; w < NW; w++) {
                double Go[8][128], Gl[8]; /* per key group of the wave (KPW <= 8) */
                for (int g = 0; g < KPW; g++) {
                    Gl[g] = 0.0;
                    for (int i = 0; i < hd; i++) Go[g][i] = 0.0;
                    for (int t = t0 + w * KPW + g; t < t1; t += NW * KPW) {
                        const uint16_t* kt = kc + (size_t)t * kv_stride + (size_t)kvh * hd;
                        const uint16_t* vt = vc + (size_t)t * kv_stride + (size_t)kvh * hd;
                        float lane[16];
                        for (int j = 0; j < LPK; j++) {
                            float acc = 0.f;
                            for (int i = 0; i < 8; i++) acc = fmaf(qf[8 * j + i], kfo_bf16_to_f32(kt[8 * j + i]), acc);
                            lane[j] = acc;
                        }
                        for (int s = 1; s < LPK; s <<= 1)
                            for (int j = 0; j < LPK; j += 2 * s) lane[j] = lane[j] + lane[j + s];
                        const float sc = kfo_round_bf16(lane[0] * rden);
                        float f, n;
                        kfo_exp2_parts(sc * 1.44269502162933349609375f, &f, &n);
                        if (!(fabsf(n) <= FX_LIM)) guard = 1;
                        const float an = n != n ? INFINITY : fabsf(n);
                        if (an > amax) amax = an;
                        const double p = ldexp((double)f, (int)n);
                        Gl[g] += p;
                        for (int i = 0; i < hd; i++) Go[g][i] = fma(p, (double)kfo_bf16_to_f32(vt[i]), Go[g][i]);
                    }
                }
                for (int s = KPW / 2; s >= 1; s >>= 1) /* pairwise: g with g + s */
                    for (int g = 0; g < s; g++) {
                        Gl[g] += Gl[g + s];
                        for (int i = 0; i < hd; i++) Go[g][i] += Go[g + s][i];
                    }
                Wl += Gl[0];
                for (int i = 0; i < hd; i++) Wo[i] += Go[0][i];
            }
            Sl[sp] = Wl;
            for (int i = 0; i < hd; i++) So[sp][i] = Wo[i];
        }
        if (nsp == 1) {
            for (int i = 0; i < hd; i++) out[(size_t)h * hd + i] = kfo_f32_to_bf16((float)(So[0][i] / Sl[0]));
        } else {
            double Lq[FX_MAXSP];
            for (int sp = 0; sp < FX_MAXSP; sp++) Lq[sp] = Sl[sp];
            for (int s = FX_MAXSP / 2; s >= 1; s >>= 1) /* the slices' L: a balanced tree */
                for (int sp = 0; sp < s; sp++) Lq[sp] += Lq[sp + s];
            for (int i = 0; i < hd; i++) {
                double qs[4];
                for (int k = 0; k < 4; k++) {
                    qs[k] = 0.0;
                    for (int sp = k * (FX_MAXSP / 4); sp < (k + 1) * (FX_MAXSP / 4); sp++) qs[k] += So[sp][i];
                }
                const double o = (qs[0] + qs[1]) + (qs[2] + qs[3]);
                out[(size_t)h * hd + i] = kfo_f32_to_bf16((float)(o / Lq[0]));
            }
        }
    }
    *max_abs_n = amax;
    return guard;
}
