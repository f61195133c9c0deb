// chronoclust_amd/csrc: the fused ingest of list-mode event records WITH a transform (cc_points_upload_list_xf and its kin):
// what k_ingest_list does (cc_ingest_list.h), and between the decoding and the scaling the compensation by the inverse
// spillover matrix and arcsinh(v / cofactor) - the preparation every cytometry file takes before it is clustered - or, for
// the `_list_xl` entry points, the logicle scale of fluorescence flow cytometry, solved per value (cc_logicle_value).
// (included by cc_online.h behind cc_ingest_list.h; one translation unit, cc_api.hip)
#pragma once

// ---------------------------------------------------------------------------------
// The transform on the device: cc_list_xf, built by list_check_xf (cc_api_list.inc) and laid behind the descriptors in the
// same device buffer.  All pointers are device pointers.
//   m          compensated source columns, 0: none
//   comp       [m][m] row-major, the inverse spillover matrix; read from global memory through the caches: every workgroup
//              reads the same at most 32 KiB, a wave reads one row segment comp[j][sel ..] per step - consecutive addresses
//              where the selected dimensions follow the matrix order - and the LDS stays with the events
//   ccol       [m] the compensated source columns, cmask[m] the AND mask each is decoded with (integers: the mask of the
//              first selected dimension that names the column, 0xFFFFFFFF for a column no selected dimension names)
//   sel        [d] per selected dimension: its index into ccol / comp's columns, -1: not compensated
//   cof        [d] cofactors, null: none; an entry of 0 passes the value through
// The value of (event, selected dimension c), cc_xf_value - THE one device function both kernels below call, on the same
// operands, so that the scaler's min_ (fitted from k_col_minmax_list_xf) maps the minimum k_ingest_list_xf holds to exactly
// 0.0:
//   sel[c] = i >= 0:  v = ((x[0] * comp[0][i]) + x[1] * comp[1][i]) + ... ascending, x[j] the decoded element of ccol[j],
//                     every product and every sum rounded to double (the build's -ffp-contract=off: nothing is fused)
//   else              v = the decoded element of the dimension's own column
//   cof[c] > 0:       v = asinh(v / cof[c]) - one double division, the device maths library's asinh
//   LG, pa[c] > 0:    v = logicle(v) (cc_logicle_value); never on a dimension with a cofactor > 0 (refused: list_check_lg)
// The logicle instances (LG, the third template parameter) find their coefficients behind the cofactors, which the host then
// always lays: lg = cof + d, [d][5] row-major x1, b, d, pa, pc (cc_logicle.h); a row of zeros is off the scale.  The kernels'
// arguments are the same with and without: an instance without LG is, instruction for instruction, what it was.
// ---------------------------------------------------------------------------------
struct cc_list_xf {
    int m;
    const double* comp;
    const int* ccol;
    const unsigned* cmask;
    const int* sel;
    const double* cof;
};

// The coefficients of one dimension as the solve takes them: kc = pc / pa (one division where they are loaded), so that
// the equation is solved for r = |v| / pa and no intermediate exceeds r b^2 - a T of any size and a |v| of any size stay in range.
struct cc_lgc {
    double x1, b, d, pa, kc;
};

__device__ __forceinline__ cc_lgc cc_lgc_load(const double* __restrict__ row)
{
    cc_lgc g;
    g.x1 = row[0]; g.b = row[1]; g.d = row[2]; g.pa = row[3];
    g.kc = g.pa > 0.0 ? row[4] / g.pa : 0.0;
    return g;
}

// Halley steps of cc_logicle_value: a compile-time count, every lane takes them all - no exit depends on the data.  From the
// start below three steps reach the floor of double arithmetic over |v| from the smallest subnormal to 1e300 for every
// parameter set of tests/logicle_util.py; the fourth is the margin.
#ifndef CC_LOGICLE_STEPS
#define CC_LOGICLE_STEPS 4
#endif

// logicle(v) = x1 + sign(v) u, u the root of g(u) = expm1(b u) - kc expm1(-d u) - r = 0, r = |v| / pa  (G / pa of cc_logicle.h).
// g is increasing and convex on u >= 0, so both starts - the tangent at 0, r / g'(0), exact to O(u^3) near zero, and
// ln(r + 1) / b, exact but for the decaying term far out - lie at or above the root; the smaller is taken and Halley's
// iteration falls onto the root from there, 1 - g g'' / (2 g'^2) staying above 1/2.  The expm1 form loses nothing at small u;
// the step is formed from the quotients g / g' and g'' / g', never from a square.  Beyond r = 2^900 (and for Inf and NaN, which
// give a non-finite result) the decaying term and the constants are below the last place: u = (ln |v| - ln pa) / b.
// logicle(+-0) = x1, bit for bit.  -ffp-contract=off: nothing is fused.
__device__ __forceinline__ double cc_logicle_value(double v, const cc_lgc g)
{
    const double y = __builtin_fabs(v);
    const double r = y / g.pa;
    double u;
    if (r <= 0x1p900) {
        const double kd = g.kc * g.d;
        const double lin = r / (g.b + kd);
        const double far = log(r + 1.0) / g.b;
        u = lin < far ? lin : far;
#pragma clang loop unroll(disable)
        for (int i = 0; i < CC_LOGICLE_STEPS; ++i) {
            const double e1 = expm1(g.b * u);
            const double e2 = expm1(-(g.d * u));
            const double f = (e1 - g.kc * e2) - r;
            const double p1 = g.b * (e1 + 1.0);
            const double p2 = kd * (e2 + 1.0);
            const double f1 = p1 + p2;
            const double f2 = g.b * p1 - g.d * p2;
            const double q = f / f1;
            const double den = 1.0 - 0.5 * (q * (f2 / f1));
            u = u - q / den;
        }
    } else {
        u = (log(y) - log(g.pa)) / g.b;
    }
    return v < 0.0 ? g.x1 - u : g.x1 + u;
}

// x: the event's m compensated elements, decoded (LDS); own: the event's record in staging; lg: read by the LG instances only
template <typename T, bool SWAP, bool LG>
__device__ __forceinline__ double cc_xf_value(const T* __restrict__ x, const unsigned char* __restrict__ own, int col, unsigned mask,
                                              int sel, int m, const double* __restrict__ comp, double cof, const cc_lgc lg)
{
    double v;
    if (sel >= 0) {
        const double* __restrict__ k = comp + sel;
        v = (double)x[0] * k[0];
        for (int j = 1; j < m; ++j) {
            const double t = (double)x[j] * k[(size_t)j * m];
            v = v + t;
        }
    } else {
        v = (double)cc_list_decode<T, SWAP>(own + (size_t)col * sizeof(T), mask);
    }
    if (cof > 0.0) {
        const double q = v / cof;
        v = asinh(q);
    }
    if constexpr (LG) {
        if (lg.pa > 0.0) v = cc_logicle_value(v, lg);
    }
    return v;
}

// the tile's compensated source columns into LDS, decoded: xs[p * XP + j] = element ccol[j] of event p of the tile (np events)
template <typename T, bool SWAP, int XP>
__device__ __forceinline__ void cc_xf_stage(T* __restrict__ xs, const unsigned char* __restrict__ src, int src_cols, int np, int m,
                                            const int* __restrict__ ccol, const unsigned* __restrict__ cmask)
{
    const int tot = np * m;
    for (int e = (int)threadIdx.x; e < tot; e += 256) {
        const int p = e / m, j = e - p * m;
        xs[p * XP + j] = cc_list_decode<T, SWAP>(src + ((size_t)p * (size_t)src_cols + (size_t)ccol[j]) * sizeof(T), cmask[j]);
    }
}

// ---------------------------------------------------------------------------------
// k_ingest_list_xf<T, SWAP>: k_ingest_list's grid, addressing and results (X, Xt with its pad rows, bad[0], bad[2..3]); whether
// there is compensation (m > 0), cofactors (cof) or scaling (scale) are wave-uniform runtime branches.  A value is computed
// ONCE, written to X from the register and kept in LDS as a double; after the barrier a wave reads one dimension of 64
// events (lane = event, pitch 65 doubles: every bank once) and writes one 512-byte segment of Xt: the same doubles by
// construction.  The tile's compensated columns are staged once per workgroup, decoded, at cc_ingest_pitch<T>().
// LDS: 64 x 65 doubles (33 280 bytes) + 64 x pitch T (8 448 .. 33 280 bytes) + the block's descriptors.
// The finiteness test is always compiled in: a compensated sum of finite integers times a large matrix entry may overflow.
// LG: the block's logicle coefficients lie in LDS next to s_cof, one array per coefficient (5 x 64 doubles, 2 560 bytes):
// neighbouring lanes hold neighbouring dimensions and read neighbouring banks.
// ---------------------------------------------------------------------------------
template <typename T, bool SWAP, bool LG = false>
__global__ __launch_bounds__(256) void k_ingest_list_xf(const unsigned char* __restrict__ raw, int src_cols, int ns, long long s0,
                                                        long long n_total, int d, int xt_rows,
                                                        const cc_list_desc* __restrict__ desc, cc_list_xf xf,
                                                        double* __restrict__ X, double* __restrict__ Xt,
                                                        const double* __restrict__ scale, const double* __restrict__ mn,
                                                        int* __restrict__ bad)
{
    constexpr int XP = cc_ingest_pitch<T>();
    constexpr int VP = CC_INGEST_TILE + 1;
    __shared__ double val[CC_INGEST_TILE * VP];
    __shared__ T xs[CC_INGEST_TILE * XP];
    __shared__ int s_col[CC_INGEST_TILE];
    __shared__ unsigned s_mask[CC_INGEST_TILE];
    __shared__ int s_sel[CC_INGEST_TILE];
    __shared__ double s_cof[CC_INGEST_TILE];
    __shared__ double s_lg[LG ? 5 * CC_INGEST_TILE : 1];
    __shared__ unsigned long long s_m;
    const int p0 = (int)blockIdx.x * CC_INGEST_TILE;  // the tile's first point, in the slab
    const int np = ns - p0 < CC_INGEST_TILE ? ns - p0 : CC_INGEST_TILE;
    const int c0 = (int)blockIdx.y * CC_INGEST_TILE;
    const int db = d - c0 < CC_INGEST_TILE ? d - c0 : CC_INGEST_TILE;
    const int m = xf.m;
    const unsigned char* __restrict__ src = raw + (size_t)p0 * (size_t)src_cols * sizeof(T);  // the tile's first record
    if (threadIdx.x == 0) s_m = 0ull;
    if ((int)threadIdx.x < db) {
        const cc_list_desc e = desc[c0 + threadIdx.x];
        s_col[threadIdx.x] = e.col;
        s_mask[threadIdx.x] = e.mask;
        s_sel[threadIdx.x] = m > 0 ? xf.sel[c0 + threadIdx.x] : -1;
        s_cof[threadIdx.x] = xf.cof ? xf.cof[c0 + threadIdx.x] : 0.0;
        if constexpr (LG) {
            const cc_lgc g = cc_lgc_load(xf.cof + d + (size_t)5 * (c0 + threadIdx.x));
            s_lg[threadIdx.x] = g.x1;
            s_lg[CC_INGEST_TILE + threadIdx.x] = g.b;
            s_lg[2 * CC_INGEST_TILE + threadIdx.x] = g.d;
            s_lg[3 * CC_INGEST_TILE + threadIdx.x] = g.pa;
            s_lg[4 * CC_INGEST_TILE + threadIdx.x] = g.kc;
        }
    }
    if (m > 0) cc_xf_stage<T, SWAP, XP>(xs, src, src_cols, np, m, xf.ccol, xf.cmask);
    __syncthreads();
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    double* __restrict__ dst = X + (size_t)(s0 + p0) * d + c0;
    double* __restrict__ out = Xt + (size_t)c0 * n_total + (size_t)(s0 + p0) + lane;
    // rows c0 .. c0 + rows - 1 of Xt: this block's dimensions and, behind the last of them, the pad rows
    const int rows = xt_rows - c0 < CC_INGEST_TILE ? xt_rows - c0 : CC_INGEST_TILE;
    // element e of the tile in row order = (point e / db, dimension e % db); a thread's elements are 256 apart
    const int tot = np * db, step_p = 256 / db, step_c = 256 - step_p * db;
    int p = (int)threadIdx.x / db, c = (int)threadIdx.x - p * db;
    int b = 0;
    double mx = 0.0;
    for (int e = (int)threadIdx.x; e < tot; e += 256) {
        cc_lgc g{};
        if constexpr (LG)
            g = cc_lgc{s_lg[c], s_lg[CC_INGEST_TILE + c], s_lg[2 * CC_INGEST_TILE + c], s_lg[3 * CC_INGEST_TILE + c],
                       s_lg[4 * CC_INGEST_TILE + c]};
        double v = cc_xf_value<T, SWAP, LG>(xs + p * XP, src + (size_t)p * (size_t)src_cols * sizeof(T), s_col[c], s_mask[c], s_sel[c],
                                            m, xf.comp, s_cof[c], g);
        if (scale) {
            v = v * scale[c0 + c];
            v = v + mn[c0 + c];
        }
        val[p * VP + c] = v;
        dst[(size_t)p * d + c] = v;
        b |= !(v - v == 0.0);
        const double a = __builtin_fabs(v);
        mx = a > mx ? a : mx;  // (NaN never enters)
        p += step_p;
        c += step_c;
        if (c >= db) {
            c -= db;
            ++p;
        }
    }
    __syncthreads();
    if (lane < np)
        for (int i = wave; i < rows; i += 4) out[(size_t)i * n_total] = i < db ? val[lane * VP + i] : 0.0;
    if (__any(b) && lane == 0) atomicOr(bad, 1);
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(mx, off);
        mx = o > mx ? o : mx;
    }
    if (lane == 0) atomicMax(&s_m, (unsigned long long)__double_as_longlong(mx));
    __syncthreads();
    if (threadIdx.x == 0 && s_m != 0ull) atomicMax(reinterpret_cast<unsigned long long*>(bad + 2), s_m);
}

// Per-selected-column minimum / maximum of the TRANSFORMED values of a slab of event records in device staging (n records),
// NaN ignored: k_col_minmax_list's partials part[2][chunks][d], one workgroup per (row chunk, block of 64 selected columns).
// The chunk's rows go by in tiles of 64 events; a tile's compensated columns are staged as k_ingest_list_xf stages them and
// every value comes from cc_xf_value on the same operands.  Thread t keeps column c0 + t % db and the tile's events t / db,
// t / db + 256 / db, ...
template <typename T, bool SWAP, bool LG = false>
__global__ __launch_bounds__(256) void k_col_minmax_list_xf(const unsigned char* __restrict__ raw, long long n, int src_cols, int d,
                                                            const cc_list_desc* __restrict__ desc, cc_list_xf xf,
                                                            double* __restrict__ part, int chunks)
{
    constexpr int XP = cc_ingest_pitch<T>();
    __shared__ T xs[CC_INGEST_TILE * XP];
    __shared__ double smn[256], smx[256];
    const long long per = (n + chunks - 1) / chunks;
    const long long r0 = (long long)blockIdx.x * per, r1 = (r0 + per < n) ? r0 + per : n;
    double mn = CC_INF, mx = -CC_INF;
    const int c0 = (int)blockIdx.y * CC_INGEST_TILE;
    const int db = (d - c0) < CC_INGEST_TILE ? d - c0 : CC_INGEST_TILE;
    const int rows_per_pass = 256 / db;
    const int col = (int)(threadIdx.x % db);
    const int rsub = (int)(threadIdx.x / db);
    const int m = xf.m;
    const cc_list_desc e = desc[c0 + col];
    const int sel = m > 0 ? xf.sel[c0 + col] : -1;
    const double cof = xf.cof ? xf.cof[c0 + col] : 0.0;
    cc_lgc g{};
    if constexpr (LG) g = cc_lgc_load(xf.cof + d + (size_t)5 * (c0 + col));
    for (long long t0 = r0; t0 < r1; t0 += CC_INGEST_TILE) {
        const int np = r1 - t0 < CC_INGEST_TILE ? (int)(r1 - t0) : CC_INGEST_TILE;
        const unsigned char* __restrict__ src = raw + (size_t)t0 * (size_t)src_cols * sizeof(T);
        if (m > 0) {
            __syncthreads();  // (the previous tile's readers have left xs)
            cc_xf_stage<T, SWAP, XP>(xs, src, src_cols, np, m, xf.ccol, xf.cmask);
            __syncthreads();
        }
        if (rsub < rows_per_pass)
            for (int p = rsub; p < np; p += rows_per_pass) {
                const double v = cc_xf_value<T, SWAP, LG>(xs + p * XP, src + (size_t)p * (size_t)src_cols * sizeof(T), e.col, e.mask, sel,
                                                          m, xf.comp, cof, g);
                mn = __builtin_fmin(mn, v);  // fmin / fmax return the non-NaN operand
                mx = __builtin_fmax(mx, v);
            }
    }
    smn[threadIdx.x] = mn;
    smx[threadIdx.x] = mx;
    __syncthreads();
    if ((int)threadIdx.x < db) {
        for (int q = 1; q < rows_per_pass; ++q) {
            mn = __builtin_fmin(mn, smn[q * db + threadIdx.x]);
            mx = __builtin_fmax(mx, smx[q * db + threadIdx.x]);
        }
        part[(size_t)blockIdx.x * d + c0 + threadIdx.x] = mn;
        part[(size_t)(chunks + blockIdx.x) * d + c0 + threadIdx.x] = mx;
    }
}
