// chronoclust_amd/csrc: kernels over the uploaded points - transposed copy, finiteness check, MinMax scaler.  (included by cc_online.h; one translation unit, cc_api.hip)
#pragma once

// dimension-major copy of the points for the scan's coalesced loads: xt[i * n + r] = x[r * d + i]
__global__ void k_transpose_points(const double* __restrict__ x, double* __restrict__ xt, long long n, int d)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * d) return;
    const long long r = e / d;
    const int i = (int)(e - r * d);
    xt[(size_t)i * n + r] = x[e];
}

// NaN / Inf check of the uploaded points (cc_points_upload)
// bad[0]: 1 if any value is NaN or Inf; bad[2..3] (one 64-bit word): bits of the largest |value| (Ctl::x_absmax: the
// single-precision prefix of the pruned scans needs a bound on the magnitudes it converts)
__global__ __launch_bounds__(256) void k_check_finite(const double* __restrict__ x, long long n, int* __restrict__ bad)
{
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    int b = 0;
    double m = 0.0;
    for (; i < n; i += stride) {
        const double v = x[i];
        b |= !(v - v == 0.0);
        const double a = __builtin_fabs(v);
        m = a > m ? a : m;  // (NaN never enters)
    }
    if (b) atomicOr(bad, 1);
    __shared__ unsigned long long s_m;
    if (threadIdx.x == 0) s_m = 0ull;
    __syncthreads();
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(m, off);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(&s_m, (unsigned long long)__double_as_longlong(m));
    __syncthreads();
    if (threadIdx.x == 0 && s_m != 0ull) atomicMax(reinterpret_cast<unsigned long long*>(bad + 2), s_m);
}

// ---------------------------------------------------------------------------------
// MinMax scaling on the device (scaling/scaler.py:27-47 = scikit-learn's MinMaxScaler restated, see
// chronoclust_amd/scaling/scaler.py): HBM-bound elementwise passes and one column reduction.
// ---------------------------------------------------------------------------------

// per-column minimum / maximum ignoring NaN (np.nanmin / np.nanmax): one workgroup per row chunk, coalescing is across the
// columns of a row (consecutive threads read consecutive doubles), partials in part[2][chunks][d].  BLOCKED (d > 256): one
// workgroup per (row chunk, block of 256 columns: blockIdx.y), each block reduced like a table of at most 256 columns.
// T: the element type of x, double or float (cc_col_minmax_f32) - widened at the load, which is exact, so that order, fmin /
// fmax and the NaN rule are one reduction's for both.
template <bool BLOCKED, typename T>
__global__ __launch_bounds__(256) void k_col_minmax(const T* __restrict__ x, long long n, int d,
                                                    double* __restrict__ part, int chunks)
{
    // this workgroup's columns c0 .. c0 + db - 1: thread t handles column c0 + t % db of rows t / db, t / db + rows_per_pass, ...
    const int c0 = BLOCKED ? (int)blockIdx.y * 256 : 0;
    const int db = BLOCKED ? ((d - c0) < 256 ? d - c0 : 256) : d;
    const int rows_per_pass = 256 / db > 0 ? 256 / db : 1;
    const int col = (db <= 256) ? (int)(threadIdx.x % db) : 0;
    const int rsub = (int)(threadIdx.x / db);
    const long long per = (n + chunks - 1) / chunks;
    const long long r0 = (long long)blockIdx.x * per, r1 = (r0 + per < n) ? r0 + per : n;
    double mn = CC_INF, mx = -CC_INF;
    if (rsub < rows_per_pass && db <= 256)
        for (long long r = r0 + rsub; r < r1; r += rows_per_pass) {
            const double v = (double)x[r * d + c0 + col];
            mn = __builtin_fmin(mn, v);  // fmin / fmax return the non-NaN operand
            mx = __builtin_fmax(mx, v);
        }
    __shared__ double smn[256], smx[256];
    smn[threadIdx.x] = mn;
    smx[threadIdx.x] = mx;
    __syncthreads();
    if ((int)threadIdx.x < db && db <= 256) {
        for (int q = 1; q < rows_per_pass; ++q) {
            mn = __builtin_fmin(mn, smn[q * db + threadIdx.x]);
            mx = __builtin_fmax(mx, smx[q * db + threadIdx.x]);
        }
        part[(size_t)blockIdx.x * d + c0 + threadIdx.x] = mn;
        part[(size_t)(chunks + blockIdx.x) * d + c0 + threadIdx.x] = mx;
    }
}

// MinMaxScaler.transform: X * scale_ + min_ (two roundings, in place); inverse: (X - min_) / scale_
__global__ void k_scale_points(double* __restrict__ x, long long tot, int d, const double* __restrict__ scale,
                               const double* __restrict__ mn)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= tot) return;
    const int c = (int)(e % d);
    double v = x[e];
    v = v * scale[c];
    v = v + mn[c];
    x[e] = v;
}

__global__ void k_unscale_points(const double* __restrict__ x, double* __restrict__ out, long long tot, int d,
                                 const double* __restrict__ scale, const double* __restrict__ mn)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= tot) return;
    const int c = (int)(e % d);
    double v = x[e];
    v = v - mn[c];
    v = v / scale[c];
    out[e] = v;
}

// ---------------------------------------------------------------------------------
// Single-precision points (cc_points_upload_f32 and its kin): one pass over raw float [ns, d] - a slab of a timepoint of
// n_total points that starts at point s0, in device staging - leaves what k_scale_points, k_check_finite and
// k_transpose_points leave of a float64 upload:
//   X  [n_total, d]        row-major, (double)v - exact - or, SCALED, (double)v * scale[c], then + mn[c] (two roundings)
//   Xt [xt_rows, n_total]  dimension-major, the same doubles; rows d .. xt_rows - 1 (the padded scan widths) +0.0
//   bad[0] |= 1 for a NaN / Inf among the stored values, bad[2..3] max= the bits of the largest stored magnitude
// One workgroup per tile of 64 points x block of at most 64 dimensions (grid: tiles of the slab x blocks of d).  The tile
// is read as rows of db consecutive floats - for d <= 64 that is one contiguous range of 64 d floats - and each value is
// written to X from the register it was loaded into, at the position it was read from: loads and stores of a wave are
// consecutive.  The floats are staged in LDS at a pitch of 65 words, so that a wave that reads one dimension of 64 points
// (lane = point) meets 32 banks per half; it widens (and scales) them again - the same operations on the same operands give
// the same doubles - and writes one 512-byte row segment of Xt per (wave, dimension).  The pad rows belong to the workgroups
// of the last block (they exist only where d <= 64: one block).
// ---------------------------------------------------------------------------------
#define CC_INGEST_TILE 64
#define CC_INGEST_PITCH 65

template <bool SCALED>
__device__ __forceinline__ double cc_ingest_value(float f, const double* __restrict__ scale, const double* __restrict__ mn, int c)
{
    double v = (double)f;
    if (SCALED) {
        v = v * scale[c];
        v = v + mn[c];
    }
    return v;
}

template <bool SCALED>
__global__ __launch_bounds__(256) void k_ingest_f32(const float* __restrict__ raw, int ns, long long s0, long long n_total, int d,
                                                    int xt_rows, double* __restrict__ X, double* __restrict__ Xt,
                                                    const double* __restrict__ scale, const double* __restrict__ mn,
                                                    int* __restrict__ bad)
{
    __shared__ float tile[CC_INGEST_TILE * CC_INGEST_PITCH];
    __shared__ unsigned long long s_m;
    const int p0 = (int)blockIdx.x * CC_INGEST_TILE;  // the tile's first point, in the slab
    const int np = ns - p0 < CC_INGEST_TILE ? ns - p0 : CC_INGEST_TILE;
    const int c0 = (int)blockIdx.y * CC_INGEST_TILE;
    const int db = d - c0 < CC_INGEST_TILE ? d - c0 : CC_INGEST_TILE;
    if (threadIdx.x == 0) s_m = 0ull;
    const float* __restrict__ src = raw + (size_t)p0 * d + c0;
    double* __restrict__ dst = X + (size_t)(s0 + p0) * d + c0;
    // element e of the tile = (point e / db, dimension e % db); a thread's elements are 256 apart
    const int tot = np * db, step_p = 256 / db, step_c = 256 - step_p * db;
    int p = (int)threadIdx.x / db, c = (int)threadIdx.x - p * db;
    int b = 0;
    double m = 0.0;
    for (int e = (int)threadIdx.x; e < tot; e += 256) {
        const size_t g = (size_t)p * d + c;
        const float f = src[g];
        tile[p * CC_INGEST_PITCH + c] = f;
        const double v = cc_ingest_value<SCALED>(f, scale, mn, c0 + c);
        dst[g] = v;
        b |= !(v - v == 0.0);
        const double a = __builtin_fabs(v);
        m = a > m ? a : m;  // (NaN never enters)
        p += step_p;
        c += step_c;
        if (c >= db) {
            c -= db;
            ++p;
        }
    }
    __syncthreads();
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    if (__any(b) && lane == 0) atomicOr(bad, 1);
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(m, off);
        m = o > m ? o : m;
    }
    if (lane == 0) atomicMax(&s_m, (unsigned long long)__double_as_longlong(m));
    // rows c0 .. c0 + rows - 1 of Xt: this block's dimensions and, behind the last of them, the pad rows
    const int rows = xt_rows - c0 < CC_INGEST_TILE ? xt_rows - c0 : CC_INGEST_TILE;
    if (lane < np) {
        double* __restrict__ out = Xt + (size_t)c0 * n_total + (size_t)(s0 + p0) + lane;
        for (int i = wave; i < rows; i += 4)
            out[(size_t)i * n_total] = i < db ? cc_ingest_value<SCALED>(tile[lane * CC_INGEST_PITCH + i], scale, mn, c0 + i) : 0.0;
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_m != 0ull) atomicMax(reinterpret_cast<unsigned long long*>(bad + 2), s_m);
}
