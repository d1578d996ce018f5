// kf_gama_plan.h -- how kf_gama_backward runs: kf::gama_plan, one pure host function, picks the tile form, the cut of the n token rows into slabs, the grids, the LDS
// and the scratch; kf_gama_bwd.hip and the entry in kf_abi.hip execute what it returns and decide nothing.
//   The product is the weight-gradient GEMM of kf_linear_backward (both operands k-major, contraction over the n token rows), but what leaves a workgroup is two fp32
//   numbers per 128-column group of its tile, not the tile: a slab's partials are [2][nGroup] floats.  So a cut over n costs 8 bytes per group and slab -- not the
//   64 / 256 KiB partial tiles of gemm3_sk_kernel -- and needs no flags: every (slab, tile) is its own workgroup, a second launch adds the slabs in index order.
//   * form: the tile's IC extent must be whole groups: 128 x 128 (G3_SMALL) or 256 x 256 (G3_BIG: a wave's 128 columns are one group); 256 x 256 from G3_BIG_MIN
//     tiles, as the forward rule.
//   * slabs: S in 1 .. GAMA_MAX_SLABS, each at least GAMA_MIN_STEPS k-steps of G3_BK rows deep, chosen to fill the most of the last round of resident workgroups
//     (tiles S / (rounds x resident)); ties go to the smaller S.  Slab s owns k-steps [nkt s / S, nkt (s + 1) / S).
#pragma once
#include "kf_gemm_plan.h"

namespace kf {

constexpr int GAMA_GROUP = 128;    /* lGroup served: a tile's IC extent is a whole number of these */
constexpr int GAMA_MAX_SLABS = 8;  /* cut of the n token rows */
constexpr int GAMA_MIN_STEPS = 2;  /* k-steps (of G3_BK rows) per slab: the prologue of a piece is one step's loads */
constexpr int GAMA_FIN_BLOCK = 256; /* threads of the finish launch, one gGama element each */

struct GamaPlan {
    int status;          /* KF_OK, or KF_INVALID_ARGS for a shape the entry refuses */
    int form;            /* G3_SMALL / G3_BIG */
    int nbx, nby;        /* tiles along IC and OC */
    int S;               /* slabs over n */
    int gx, block, lds;  /* the tile launch: nbx nby S workgroups */
    int fin_gx;          /* the finish launch: 2 nGroup elements */
    long long scratch;   /* bytes: S slabs of [2][nGroup] fp32 */
};

// the shapes served: IC whole groups, OC and n as kf_linear_backward's weight gradient wants them
inline bool gama_shape_ok(int OC, int IC, int n) { return OC >= 128 && OC % 64 == 0 && IC >= GAMA_GROUP && IC % GAMA_GROUP == 0 && n >= G3_BK && n % G3_BK == 0; }

inline GamaPlan gama_plan(int OC, int IC, int n) {
    GamaPlan p = {};
    if (!gama_shape_ok(OC, IC, n)) {
        p.status = KF_INVALID_ARGS;
        return p;
    }
    const long nbig = cdiv(IC, G3_BM) * cdiv(OC, G3_BN);
    p.form = nbig >= G3_BIG_MIN ? G3_BIG : G3_SMALL;
    const G3Form& c = G3_FORMS[p.form];
    p.nbx = (int)cdiv(IC, c.bm), p.nby = (int)cdiv(OC, c.bn);
    const long tiles = (long)p.nbx * p.nby, resident = 256L * c.wgs;
    const int nkt = n / G3_BK;
    p.S = 1;
    for (int s = 2; s <= GAMA_MAX_SLABS && nkt / s >= GAMA_MIN_STEPS; s++) {
        /* fill of the rounds: tiles s / (rounds(s) resident) > tiles S / (rounds(S) resident), in integers */
        if (tiles * s * cdiv(tiles * p.S, resident) > tiles * p.S * cdiv(tiles * s, resident)) p.S = s;
    }
    const long long nGroup = (long long)OC * IC / GAMA_GROUP;
    p.gx = (int)(tiles * p.S), p.block = c.nth, p.lds = c.lds;
    p.fin_gx = (int)cdiv(2 * nGroup, GAMA_FIN_BLOCK);
    p.scratch = up256((long long)p.S * 2 * nGroup * 4);
    return p;
}

// ---- the launcher (kf_gama_bwd.hip): executes a plan, nothing else; KF_OK or KF_HIP_CHECK.  fmt: FMT_Q4 / FMT_Q2 / FMT_Q1 of the packed stream
int gama_backward_launch(hipStream_t st, const GamaPlan& p, const unsigned char* packed, int fmt, int qBias, int OC, int IC, const uint16_t* deltaIn, const uint16_t* inp, int n,
                         uint16_t* gGama, float scale, float* scratch);

}  // namespace kf
