// cc_assign.h — gfx950 kernels of the read-only assignment (cc_assign): for every point, on its own, what the online phase
// would decide if the point were the very next one (hddstream.py:288-430) against the table as it stands.  Nothing is
// speculated and nothing is written to the table, so neither the windows nor their validation kernels take part:
//
//   k_assign_scan    per point and kind the nearest row by (projected distance, list-order key) - for the pcore kind the
//                    nearest ADMISSIBLE one (pdim filter of the tentative add, hddstream.py:317-321)
//   k_assign_decide  the radius test of the enlarged pcore row, failing that of the enlarged outlier row with its promotion
//                    flag (:416-419), failing that "new"; uid, path and distance per point
//
// Arithmetic: the reference's.  A distance is the left-to-right sum over all d dimensions of (p_i - cen_i)^2 / pref_i with
// the STORED entry (Table::pref, never the operand column, which a tainted table may not hold in this form); POW2 - Ctl::pow2:
// k a power of two and every stored entry 1 or k - multiplies by 1 or 1 / k instead, the same double.  No contraction, no
// pruning.  (included by cc_api.hip behind cc_online.h, whose helpers it uses: Par, Cand, cc_tentative_radius, cc_div_pref)
#pragma once

#define CC_ASSIGN_NW 4   // waves per workgroup: the rows of a workgroup's segment are split over them
#define CC_ASSIGN_TR 8   // rows per tile: one accumulator each while the dimensions are walked
#define CC_ASSIGN_DB 8   // dimensions per block: the point's coordinates held at a time

// the columns of the table the two kernels read
struct AssignRows {
    const double* cen;
    const double* pref;
    const double* cf1;
    const double* cf2;
    const double* w;
    const int* kind;
    const int* key;
    const long long* uid;
    int m_rows;
};

// (dist, key, slot) beats the running best: a row, and nearer or equally near and earlier in its list
__device__ __forceinline__ bool cc_assign_beats(double dist, int key, const Cand& best)
{
    return best.slot < 0 || cand_less(dist, key, best.dist, best.key);
}
__device__ __forceinline__ void cc_assign_merge(Cand& best, const Cand& x)
{
    const bool take = x.slot >= 0 && cc_assign_beats(x.dist, x.key, best);
    best.dist = take ? x.dist : best.dist;
    best.key = take ? x.key : best.key;
    best.slot = take ? x.slot : best.slot;
}

// ---------------------------------------------------------------------------------
// k_assign_scan: one point per lane (grid.x tiles of 64 points of the chunk), the rows of segment blockIdx.y of gridDim.y
// split over the workgroup's waves.  A row's centroid and stored entries are the same for all 64 points of a wave: their
// addresses are wave-uniform (scalar loads, as in k_scan_u).  Rows are taken in tiles of CC_ASSIGN_TR with one accumulator
// each while the dimensions are walked in blocks of CC_ASSIGN_DB - the point's coordinates of a block are read once per tile
// from the chunk's dimension-major copy (coalesced) - so that every row's sum stays left to right and the registers held do
// not grow with d: one kernel serves d = 1 .. CC_MAX_DIM.  The pdim filter is evaluated lazily, by the lanes for which a
// pcore row would become the best (cc_tentative_radius over the row's CF1, CF2 and the point's row-major coordinates).
// part[(point * S + segment) * 2 + kind]: the segment's best per kind; slot -1: none.
// ---------------------------------------------------------------------------------
template <bool FILTER, bool POW2>
__global__ __launch_bounds__(64 * CC_ASSIGN_NW) void k_assign_scan(AssignRows t, Par par, const double* __restrict__ X,
                                                                  const double* __restrict__ Xt, int cn,
                                                                  Cand* __restrict__ part)
{
    constexpr int NW = CC_ASSIGN_NW, TR = CC_ASSIGN_TR, DB = CC_ASSIGN_DB;
    const int d = par.d;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int S = gridDim.y;
    const int nsub = S * NW;
    const int sub = blockIdx.y * NW + wv;
    const int per = (t.m_rows + nsub - 1) / nsub;
    const int r0 = min(t.m_rows, sub * per);
    const int r1 = r0 + min(per, t.m_rows - r0);
    const int j = (int)blockIdx.x * 64 + lane;
    const bool valid = j < cn;
    const int jc = valid ? j : cn - 1;  // (lanes beyond the chunk read its last point and keep nothing)
    const double* __restrict__ g_cen = t.cen;
    const double* __restrict__ g_pref = t.pref;

    Cand best[2];
    best[0] = Cand{CC_INF, CC_IDX_INF, -1};
    best[1] = Cand{CC_INF, CC_IDX_INF, -1};

    for (int rt = r0; rt < r1; rt += TR) {
        const int tm = __builtin_amdgcn_readfirstlane(min(TR, r1 - rt));
        double acc[TR];
#pragma unroll
        for (int r = 0; r < TR; ++r) acc[r] = 0.0;
        for (int i0 = 0; i0 < d; i0 += DB) {
            const int nb = min(DB, d - i0);
            double p[DB];
#pragma unroll
            for (int i = 0; i < DB; ++i) p[i] = (i < nb) ? Xt[(size_t)(i0 + i) * (size_t)cn + (size_t)jc] : 0.0;
#pragma unroll
            for (int r = 0; r < TR; ++r) {
                if (r < tm) {
                    const double* __restrict__ c = g_cen + (size_t)(rt + r) * (size_t)d + (size_t)i0;
                    const double* __restrict__ f = g_pref + (size_t)(rt + r) * (size_t)d + (size_t)i0;
#pragma unroll
                    for (int i = 0; i < DB; ++i) {
                        if (i < nb) {
                            double x = p[i] - c[i];
                            x = x * x;
                            // mc_functions.py:39 + :41
                            if (POW2) acc[r] = acc[r] + x * (f[i] == 1.0 ? 1.0 : par.inv_k);
                            else acc[r] = acc[r] + cc_div_pref(x, f[i], par);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            if (r < tm) {
                const int rowg = rt + r;
                const int kd = t.kind[rowg];  // (wave-uniform: the branches below are)
                const int key = t.key[rowg];
                if (kd == CC_KIND_PCORE) {
                    bool take = valid && cc_assign_beats(acc[r], key, best[0]);
                    if (FILTER && take) {
                        int ne1 = 0;
                        (void)cc_tentative_radius(t.cf1 + (size_t)rowg * d, t.cf2 + (size_t)rowg * d, t.w[rowg],
                                                  X + (size_t)jc * d, d, par, nullptr, &ne1);
                        take = ne1 <= par.pi;  // hddstream.py:319-321
                    }
                    best[0].dist = take ? acc[r] : best[0].dist;
                    best[0].key = take ? key : best[0].key;
                    best[0].slot = take ? rowg : best[0].slot;
                } else if (kd == CC_KIND_OUTLIER) {
                    const bool take = valid && cc_assign_beats(acc[r], key, best[1]);
                    best[1].dist = take ? acc[r] : best[1].dist;
                    best[1].key = take ? key : best[1].key;
                    best[1].slot = take ? rowg : best[1].slot;
                }
            }
        }
    }

    // the waves' bests merged through LDS by (distance, key), as in the snapshot scans
    __shared__ Cand s_m[(NW - 1) * 2 * 64];
    if (wv > 0) {
        s_m[((wv - 1) * 2 + 0) * 64 + lane] = best[0];
        s_m[((wv - 1) * 2 + 1) * 64 + lane] = best[1];
    }
    __syncthreads();
    if (wv != 0 || !valid) return;
#pragma unroll
    for (int w = 0; w < NW - 1; ++w) {
        cc_assign_merge(best[0], s_m[(w * 2 + 0) * 64 + lane]);
        cc_assign_merge(best[1], s_m[(w * 2 + 1) * 64 + lane]);
    }
    Cand* o = part + ((size_t)j * S + blockIdx.y) * 2;
    o[0] = best[0];
    o[1] = best[1];
}

// ---------------------------------------------------------------------------------
// k_assign_decide: one lane per point.  The segments' bests merged by (distance, key), then hddstream.py:330-343 for the
// pcore row and :378-395 with :416-419 for the outlier row.  path 0 / 1 / 5 with the row's creation number and its distance,
// or 2 with -1 and -1.0 (no creation number is consumed).  A point costs two tentative adds here against its share of
// m_rows distances in the scan: no lane group per point.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_assign_decide(AssignRows t, Par par, const double* __restrict__ X, int cn,
                                                       const Cand* __restrict__ part, int S,
                                                       long long* __restrict__ out_uid, int8_t* __restrict__ out_path,
                                                       double* __restrict__ out_dist)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= cn) return;
    const int d = par.d;
    Cand b0 = Cand{CC_INF, CC_IDX_INF, -1}, b1 = b0;
    for (int s = 0; s < S; ++s) {
        cc_assign_merge(b0, part[((size_t)j * S + s) * 2 + 0]);
        cc_assign_merge(b1, part[((size_t)j * S + s) * 2 + 1]);
    }
    const double* p = X + (size_t)j * d;
    int path = 2;
    long long uid = -1;
    double dist = -1.0;
    if (b0.slot >= 0) {
        const size_t r = (size_t)b0.slot;
        const double r2 = cc_tentative_radius(t.cf1 + r * d, t.cf2 + r * d, t.w[r], p, d, par, nullptr, nullptr);
        if (r2 <= par.eps_sq) {  // hddstream.py:337
            path = 0;
            uid = t.uid[r];
            dist = b0.dist;
        }
    }
    if (path == 2 && b1.slot >= 0) {
        const size_t r = (size_t)b1.slot;
        int gt1 = 0;
        const double w = t.w[r];
        const double r2 = cc_tentative_radius(t.cf1 + r * d, t.cf2 + r * d, w, p, d, par, &gt1, nullptr);
        if (r2 <= par.eps_sq) {  // hddstream.py:386
            path = 1;
            if (w + 1.0 >= par.beta_mu && gt1 <= par.pi) path |= 4;  // hddstream.py:416-419
            uid = t.uid[r];
            dist = b1.dist;
        }
    }
    out_uid[j] = uid;
    if (out_path) out_path[j] = (int8_t)path;
    if (out_dist) out_dist[j] = dist;
}
