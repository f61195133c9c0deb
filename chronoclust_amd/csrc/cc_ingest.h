// chronoclust_amd/csrc: the fused ingest of a point view (cc_points_upload_view and its kin) - any accepted element type,
// points stored by rows or by columns.  (included by cc_online.h behind cc_points.h; one translation unit, cc_api.hip)
#pragma once

// ---------------------------------------------------------------------------------
// k_ingest<T, COLS, SCALED>: one pass over a slab of raw T in device staging - ns points of a timepoint of n_total that
// start at point s0 - leaves what k_ingest_f32 leaves (cc_points.h): X row-major, Xt dimension-major with its pad rows +0.0,
// bad[0] |= 1 for a NaN / Inf among the stored values, bad[2..3] max= the bits of the largest stored magnitude.
// One workgroup per tile of 64 points x block of at most 64 dimensions, the raw elements staged in LDS point-major.
//   rows form (COLS = false): staging holds ns rows at a pitch of rp elements (rp >= d: the source's own pitch, or d).  This
//     is k_ingest_f32's scheme: the tile is read as rows of db consecutive elements and written to X from the register, at
//     the position it was read from; after the barrier a wave reads one dimension of 64 points from LDS (lane = point) and
//     writes one 512-byte segment of Xt.
//   columns form (COLS = true): staging holds d strips at a pitch of rp elements (a multiple of 64, rp >= ns).  The mirror:
//     a wave reads one dimension's 64 consecutive elements (lane = point), writes that 512-byte segment of Xt from the
//     register and stages the raw element; after the barrier the tile is walked in row order and written to X, a wave's
//     stores consecutive.
// Either way a value is converted twice - once from the register, once from LDS - by the same operations on the same
// operands: the same doubles.  (double) of every T is exact.
// LDS pitch, in elements, per element size: 65 (8 and 4 bytes), 66 (2 bytes: 33 words), 68 (1 byte: 17 words) - an odd number
// of words, or twice an odd number for the 8-byte type.  The walk with lane = point (stride = the pitch) then meets every bank
// of its lane group once: ds_read_b32 / ds_write_b32 and the sub-word forms 32 lanes on 32 banks, ds_read_b64 32 lanes x 2 words
// on 64 banks, ds_write_b64 16 lanes x 2 words on 32 banks.  The walk with consecutive elements is consecutive words.  What
// remains: in that second walk two (2 bytes) or four (1 byte) neighbouring lanes meet in one word; for the loads that is one
// address, a broadcast, for the stores of the rows form (ds_write_b16 / ds_write_b8) DESIGN.md section 4 says what is known.
// The finiteness test is compiled in for the floating types and for every SCALED instance (an integer times an overflowing
// scale is Inf on the float64 route too); the magnitude maximum for all.
// ---------------------------------------------------------------------------------

template <typename T> struct cc_ingest_elem { static constexpr bool floating = false; };
template <> struct cc_ingest_elem<double> { static constexpr bool floating = true; };
template <> struct cc_ingest_elem<float> { static constexpr bool floating = true; };
template <> struct cc_ingest_elem<_Float16> { static constexpr bool floating = true; };

template <typename T>
constexpr int cc_ingest_pitch()
{
    return sizeof(T) == 1 ? 68 : sizeof(T) == 2 ? 66 : 65;
}

template <bool SCALED, typename T>
__device__ __forceinline__ double cc_ingest_widen(T t, const double* __restrict__ scale, const double* __restrict__ mn, int c)
{
    double v = (double)t;
    if (SCALED) {
        v = v * scale[c];
        v = v + mn[c];
    }
    return v;
}

template <typename T, bool COLS, bool SCALED>
__global__ __launch_bounds__(256) void k_ingest(const T* __restrict__ raw, long long rp, int ns, long long s0, long long n_total,
                                                int d, int xt_rows, double* __restrict__ X, double* __restrict__ Xt,
                                                const double* __restrict__ scale, const double* __restrict__ mn,
                                                int* __restrict__ bad)
{
    constexpr int PITCH = cc_ingest_pitch<T>();
    constexpr bool CHECK = cc_ingest_elem<T>::floating || SCALED;
    __shared__ T tile[CC_INGEST_TILE * PITCH];
    __shared__ unsigned long long s_m;
    const int p0 = (int)blockIdx.x * CC_INGEST_TILE;  // the tile's first point, in the slab
    const int np = ns - p0 < CC_INGEST_TILE ? ns - p0 : CC_INGEST_TILE;
    const int c0 = (int)blockIdx.y * CC_INGEST_TILE;
    const int db = d - c0 < CC_INGEST_TILE ? d - c0 : CC_INGEST_TILE;
    if (threadIdx.x == 0) s_m = 0ull;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    double* __restrict__ dst = X + (size_t)(s0 + p0) * d + c0;
    double* __restrict__ out = Xt + (size_t)c0 * n_total + (size_t)(s0 + p0) + lane;
    // rows c0 .. c0 + rows - 1 of Xt: this block's dimensions and, behind the last of them, the pad rows
    const int rows = xt_rows - c0 < CC_INGEST_TILE ? xt_rows - c0 : CC_INGEST_TILE;
    // element e of the tile in row order = (point e / db, dimension e % db); a thread's elements are 256 apart
    const int tot = np * db, step_p = 256 / db, step_c = 256 - step_p * db;
    int p = (int)threadIdx.x / db, c = (int)threadIdx.x - p * db;
    int b = 0;
    double m = 0.0;
    if (!COLS) {
        const T* __restrict__ src = raw + (size_t)p0 * rp + c0;
        for (int e = (int)threadIdx.x; e < tot; e += 256) {
            const T f = src[(size_t)p * rp + c];
            tile[p * PITCH + c] = f;
            const double v = cc_ingest_widen<SCALED>(f, scale, mn, c0 + c);
            dst[(size_t)p * d + c] = v;
            if (CHECK) b |= !(v - v == 0.0);
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
        if (lane < np)
            for (int i = wave; i < rows; i += 4)
                out[(size_t)i * n_total] = i < db ? cc_ingest_widen<SCALED>(tile[lane * PITCH + i], scale, mn, c0 + i) : 0.0;
    } else {
        if (lane < np) {
            const T* __restrict__ src = raw + (size_t)c0 * rp + p0 + lane;
            for (int i = wave; i < rows; i += 4) {
                double v = 0.0;
                if (i < db) {
                    const T f = src[(size_t)i * rp];
                    tile[lane * PITCH + i] = f;
                    v = cc_ingest_widen<SCALED>(f, scale, mn, c0 + i);
                    if (CHECK) b |= !(v - v == 0.0);
                    const double a = __builtin_fabs(v);
                    m = a > m ? a : m;
                }
                out[(size_t)i * n_total] = v;
            }
        }
        __syncthreads();
        for (int e = (int)threadIdx.x; e < tot; e += 256) {
            dst[(size_t)p * d + c] = cc_ingest_widen<SCALED>(tile[p * PITCH + c], scale, mn, c0 + c);
            p += step_p;
            c += step_c;
            if (c >= db) {
                c -= db;
                ++p;
            }
        }
    }
    if (CHECK && __any(b) && lane == 0) atomicOr(bad, 1);
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(m, off);
        m = o > m ? o : m;
    }
    if (lane == 0) atomicMax(&s_m, (unsigned long long)__double_as_longlong(m));
    __syncthreads();
    if (threadIdx.x == 0 && s_m != 0ull) atomicMax(reinterpret_cast<unsigned long long*>(bad + 2), s_m);
}

// Per-column minimum / maximum of a slab of a view in device staging (n rows), NaN ignored: k_col_minmax's partials
// part[2][chunks][d] over the slab's row chunks.  Minimum and maximum do not depend on the order of the reduction (but for the sign of a zero).
//   rows form: k_col_minmax's own walk, one workgroup per (row chunk, block of 256 columns), rows at a pitch of `pitch` elements
//   columns form: one workgroup per (row chunk, column: blockIdx.y), the column's strip at c * pitch read 256 rows at a time
template <typename T, bool COLS>
__global__ __launch_bounds__(256) void k_col_minmax_view(const T* __restrict__ x, long long n, int d, long long pitch,
                                                         double* __restrict__ part, int chunks)
{
    const long long per = (n + chunks - 1) / chunks;
    const long long r0 = (long long)blockIdx.x * per, r1 = (r0 + per < n) ? r0 + per : n;
    double mn = CC_INF, mx = -CC_INF;
    __shared__ double smn[256], smx[256];
    if (COLS) {
        const int col = (int)blockIdx.y;
        const T* __restrict__ strip = x + (size_t)col * pitch;
        for (long long r = r0 + threadIdx.x; r < r1; r += 256) {
            const double v = (double)strip[r];
            mn = __builtin_fmin(mn, v);  // fmin / fmax return the non-NaN operand
            mx = __builtin_fmax(mx, v);
        }
        for (int off = 32; off >= 1; off >>= 1) {
            mn = __builtin_fmin(mn, __shfl_xor(mn, off));
            mx = __builtin_fmax(mx, __shfl_xor(mx, off));
        }
        if ((threadIdx.x & 63) == 0) {
            smn[threadIdx.x >> 6] = mn;
            smx[threadIdx.x >> 6] = mx;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int q = 1; q < 4; ++q) {
                mn = __builtin_fmin(mn, smn[q]);
                mx = __builtin_fmax(mx, smx[q]);
            }
            part[(size_t)blockIdx.x * d + col] = mn;
            part[(size_t)(chunks + blockIdx.x) * d + col] = mx;
        }
    } else {
        // this workgroup's columns c0 .. c0 + db - 1: thread t handles column c0 + t % db of rows t / db, t / db + rows_per_pass, ...
        const int c0 = (int)blockIdx.y * 256;
        const int db = (d - c0) < 256 ? d - c0 : 256;
        const int rows_per_pass = 256 / db;
        const int col = (int)(threadIdx.x % db);
        const int rsub = (int)(threadIdx.x / db);
        if (rsub < rows_per_pass)
            for (long long r = r0 + rsub; r < r1; r += rows_per_pass) {
                const double v = (double)x[(size_t)r * pitch + c0 + col];
                mn = __builtin_fmin(mn, v);
                mx = __builtin_fmax(mx, v);
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
}
