// chronoclust_amd/csrc: the fused ingest of a point view WITH a transform (cc_points_upload_view_xl and its kin): what k_ingest
// does (cc_ingest.h), and between the widening and the scaling the value cc_xf_value defines (cc_ingest_list_xf.h) - the
// compensation by the inverse spillover matrix, arcsinh(v / cofactor) or the logicle scale -, for the arrays a parsed CSV, a
// .npy file or a caller hands over.  (included by cc_online.h behind cc_ingest_list_xf.h; one translation unit, cc_api.hip)
#pragma once

// ---------------------------------------------------------------------------------
// The transform is the cc_list_xf of cc_ingest_list_xf.h, laid out on the device as list_desc_copy lays it out; ccol index the
// VIEW's columns 0 .. d - 1, so every compensated column is a selected dimension and no element is masked.
//
// Rows form: a row of a view is an event record of rp elements in native byte order, its dimensions the columns 0 .. d - 1.  That
// is k_ingest_list_xf<T, false, LG> / k_col_minmax_list_xf<T, false, LG> with src_cols = rp and the identity descriptors - the
// very kernels for float, double, uint8_t, uint16_t and uint32_t, new instances of the same text for the four view types
// list-mode data does not have, whose bit patterns follow here.
//
// Columns form (the CSV case): k_ingest_xf<T, LG> and k_col_minmax_view_xf<T, LG> below.  Every value comes from cc_xf_value -
// THE device function of the list kernels - on the same operands: x = the point's m compensated elements, point-major in LDS;
// the dimension's own element decoded in place (column 0 of a record that starts at the element, no mask, no swap).
// ---------------------------------------------------------------------------------
template <> struct cc_list_bits<_Float16> { typedef unsigned short type; };
template <> struct cc_list_bits<int8_t> { typedef unsigned char type; };
template <> struct cc_list_bits<int16_t> { typedef unsigned short type; };
template <> struct cc_list_bits<int32_t> { typedef unsigned int type; };

// the tile's m compensated strips into LDS point-major: xs[p * XP + j] = element (point p of the tile, column ccol[j]); a wave
// reads 64 consecutive elements of one strip (lane = point) and writes them a pitch apart: every bank of its lane group once
template <typename T, int XP>
__device__ __forceinline__ void cc_xf_stage_cols(T* __restrict__ xs, const T* __restrict__ tile0, long long rp, int lane, int wave, int np,
                                                 int m, const int* __restrict__ ccol)
{
    if (lane < np)
        for (int j = wave; j < m; j += 4) xs[lane * XP + j] = tile0[(size_t)ccol[j] * (size_t)rp];
}

// ---------------------------------------------------------------------------------
// k_ingest_xf<T, LG>: k_ingest's columns form - its grid, addressing and results (X row-major, Xt dimension-major with its pad
// rows +0.0, bad[0], bad[2..3]); staging holds d strips at a pitch of rp elements (a multiple of 64, rp >= ns).  Whether there
// is compensation (m > 0), cofactors (cof) or scaling (scale) are wave-uniform runtime branches, and so is everything that
// depends on the dimension alone: a wave walks one dimension at a time with lane = point, its index held in a scalar
// register, so sel, the cofactor and the logicle coefficients are scalar operands read once per (wave, dimension).
// A value is computed ONCE: the wave reads the dimension's own 64 consecutive elements from staging (or sums the point's
// compensated elements from LDS), forms the value, writes the 512-byte segment of Xt from the register and keeps the double
// in LDS at a pitch of 65; after the barrier the tile is walked in row order into X, a wave's stores consecutive: the same
// doubles by construction.
// LDS: 64 x 65 doubles (33 280 bytes) + 64 x cc_ingest_pitch<T>() elements (4 352 .. 33 280 bytes); the descriptors need none.
// Banks: xs is written and read with lane = point at the pitch of cc_ingest.h (every bank of the lane group once for the
// 8-, 4-, 2- and 1-byte walks); val is written with lane = point at 65 doubles (ds_write_b64: 16 lanes x 2 words on 32
// banks) and read with consecutive doubles.
// The finiteness test is always compiled in.
// ---------------------------------------------------------------------------------
template <typename T, bool LG>
__global__ __launch_bounds__(256) void k_ingest_xf(const T* __restrict__ raw, long long rp, int ns, long long s0, long long n_total,
                                                   int d, int xt_rows, cc_list_xf xf, double* __restrict__ X,
                                                   double* __restrict__ Xt, const double* __restrict__ scale,
                                                   const double* __restrict__ mn, int* __restrict__ bad)
{
    constexpr int XP = cc_ingest_pitch<T>();
    constexpr int VP = CC_INGEST_TILE + 1;
    __shared__ double val[CC_INGEST_TILE * VP];
    __shared__ T xs[CC_INGEST_TILE * XP];
    __shared__ unsigned long long s_m;
    const int p0 = (int)blockIdx.x * CC_INGEST_TILE;  // the tile's first point, in the slab
    const int np = ns - p0 < CC_INGEST_TILE ? ns - p0 : CC_INGEST_TILE;
    const int c0 = (int)blockIdx.y * CC_INGEST_TILE;
    const int db = d - c0 < CC_INGEST_TILE ? d - c0 : CC_INGEST_TILE;
    const int m = xf.m;
    if (threadIdx.x == 0) s_m = 0ull;
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const T* __restrict__ tile0 = raw + p0 + lane;  // this lane's point in strip 0 (read by lanes < np only)
    if (m > 0) cc_xf_stage_cols<T, XP>(xs, tile0, rp, lane, wave, np, m, xf.ccol);
    __syncthreads();
    double* __restrict__ dst = X + (size_t)(s0 + p0) * d + c0;
    double* __restrict__ out = Xt + (size_t)c0 * n_total + (size_t)(s0 + p0) + lane;
    // rows c0 .. c0 + rows - 1 of Xt: this block's dimensions and, behind the last of them, the pad rows
    const int rows = xt_rows - c0 < CC_INGEST_TILE ? xt_rows - c0 : CC_INGEST_TILE;
    int b = 0;
    double mx = 0.0;
    for (int i = wave; i < rows; i += 4) {
        double v = 0.0;
        if (i < db) {
            const int c = c0 + i;
            const int sel = m > 0 ? xf.sel[c] : -1;
            const double cof = xf.cof ? xf.cof[c] : 0.0;
            cc_lgc g{};
            if constexpr (LG) g = cc_lgc_load(xf.cof + d + (size_t)5 * c);
            if (lane < np) {
                v = cc_xf_value<T, false, LG>(xs + lane * XP, reinterpret_cast<const unsigned char*>(tile0 + (size_t)c * (size_t)rp), 0,
                                              0xFFFFFFFFu, sel, m, xf.comp, cof, g);
                if (scale) {
                    v = v * scale[c];
                    v = v + mn[c];
                }
                val[lane * VP + i] = v;
                b |= !(v - v == 0.0);
                const double a = __builtin_fabs(v);
                mx = a > mx ? a : mx;  // (NaN never enters)
            }
        }
        if (lane < np) out[(size_t)i * n_total] = v;
    }
    __syncthreads();
    // element e of the tile in row order = (point e / db, dimension e % db); a thread's elements are 256 apart
    const int tot = np * db, step_p = 256 / db, step_c = 256 - step_p * db;
    int p = (int)threadIdx.x / db, c = (int)threadIdx.x - p * db;
    for (int e = (int)threadIdx.x; e < tot; e += 256) {
        dst[(size_t)p * d + c] = val[p * VP + c];
        p += step_p;
        c += step_c;
        if (c >= db) {
            c -= db;
            ++p;
        }
    }
    if (__any(b) && lane == 0) atomicOr(bad, 1);
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(mx, off);
        mx = o > mx ? o : mx;
    }
    if (lane == 0) atomicMax(&s_m, (unsigned long long)__double_as_longlong(mx));
    __syncthreads();
    if (threadIdx.x == 0 && s_m != 0ull) atomicMax(reinterpret_cast<unsigned long long*>(bad + 2), s_m);
}

// Per-column minimum / maximum of the TRANSFORMED values of a slab of a columns-form view in device staging (n points, d
// strips at a pitch of rp elements), NaN ignored: k_col_minmax_view's partials part[2][chunks][d], one workgroup per (row chunk,
// block of CC_MINMAX_XF_DIMS columns).  The chunk's rows go by in tiles of 64 points; a tile's compensated strips are staged as
// k_ingest_xf stages them and every value comes from cc_xf_value on the same operands, a wave on one dimension at a time with
// lane = point.  A (dimension, lane) pair keeps its running extrema in LDS (one wave owns a dimension: no barrier between
// the tiles but the staging's); behind the last tile the wave folds its dimensions across the lanes.
// LDS: 2 x 16 x 64 doubles (16 384 bytes) + 64 x cc_ingest_pitch<T>() elements.
#define CC_MINMAX_XF_DIMS 16
template <typename T, bool LG>
__global__ __launch_bounds__(256) void k_col_minmax_view_xf(const T* __restrict__ raw, long long n, int d, long long rp, cc_list_xf xf,
                                                            double* __restrict__ part, int chunks)
{
    constexpr int XP = cc_ingest_pitch<T>();
    __shared__ T xs[CC_INGEST_TILE * XP];
    __shared__ double amn[CC_MINMAX_XF_DIMS * 64], amx[CC_MINMAX_XF_DIMS * 64];
    const long long per = (n + chunks - 1) / chunks;
    const long long r0 = (long long)blockIdx.x * per, r1 = (r0 + per < n) ? r0 + per : n;
    const int c0 = (int)blockIdx.y * CC_MINMAX_XF_DIMS;
    const int db = (d - c0) < CC_MINMAX_XF_DIMS ? d - c0 : CC_MINMAX_XF_DIMS;
    const int m = xf.m;
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    for (int i = wave; i < db; i += 4) {
        amn[i * 64 + lane] = CC_INF;
        amx[i * 64 + lane] = -CC_INF;
    }
    for (long long t0 = r0; t0 < r1; t0 += CC_INGEST_TILE) {
        const int np = r1 - t0 < CC_INGEST_TILE ? (int)(r1 - t0) : CC_INGEST_TILE;
        const T* __restrict__ tile0 = raw + t0 + lane;
        if (m > 0) {
            __syncthreads();  // (the previous tile's readers have left xs)
            cc_xf_stage_cols<T, XP>(xs, tile0, rp, lane, wave, np, m, xf.ccol);
            __syncthreads();
        }
        for (int i = wave; i < db; i += 4) {
            const int c = c0 + i;
            const int sel = m > 0 ? xf.sel[c] : -1;
            const double cof = xf.cof ? xf.cof[c] : 0.0;
            cc_lgc g{};
            if constexpr (LG) g = cc_lgc_load(xf.cof + d + (size_t)5 * c);
            if (lane < np) {
                const double v = cc_xf_value<T, false, LG>(xs + lane * XP, reinterpret_cast<const unsigned char*>(tile0 + (size_t)c * (size_t)rp),
                                                           0, 0xFFFFFFFFu, sel, m, xf.comp, cof, g);
                amn[i * 64 + lane] = __builtin_fmin(amn[i * 64 + lane], v);  // fmin / fmax return the non-NaN operand
                amx[i * 64 + lane] = __builtin_fmax(amx[i * 64 + lane], v);
            }
        }
    }
    for (int i = wave; i < db; i += 4) {
        double mn = amn[i * 64 + lane], mx = amx[i * 64 + lane];
        for (int off = 32; off >= 1; off >>= 1) {
            mn = __builtin_fmin(mn, __shfl_xor(mn, off));
            mx = __builtin_fmax(mx, __shfl_xor(mx, off));
        }
        if (lane == 0) {
            part[(size_t)blockIdx.x * d + c0 + i] = mn;
            part[(size_t)(chunks + blockIdx.x) * d + c0 + i] = mx;
        }
    }
}
