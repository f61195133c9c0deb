// chronoclust_amd/csrc: the fused ingest of list-mode event records (cc_points_upload_list and its kin) - the DATA segment of
// an FCS file as the bytes it holds: either byte order, the clustered channels a list of columns of the record.
// (included by cc_online.h behind cc_ingest.h; one translation unit, cc_api.hip)
#pragma once

// ---------------------------------------------------------------------------------
// k_ingest_list<T, SWAP, SCALED>: k_ingest's rows form (cc_ingest.h) with another source addressing.  One pass over a slab of
// whole event records in device staging - ns events of a timepoint of n_total that start at event s0 - leaves what k_ingest
// leaves: X row-major, Xt dimension-major with its pad rows +0.0, bad[0] |= 1 for a NaN / Inf among the stored values,
// bad[2..3] max= the bits of the largest stored magnitude.  One workgroup of 256 threads per tile of 64 points x block of at
// most 64 SELECTED dimensions; the block's descriptors {source column, AND mask} are read once into LDS.
//   address   the element of (point p, selected dimension c) is at raw + (p * src_cols + col[c]) * sizeof(T): a record is
//             src_cols elements, col[] in any order, repeats allowed.  The staging buffer starts aligned and a record is a
//             whole multiple of the element size, so every element is naturally aligned.  A channel no descriptor names is
//             never read: what it holds - a NaN pattern, say - does not reach the finiteness check.
//   decoding  the element is loaded as an unsigned integer of its width; SWAP reverses its bytes (__builtin_bswap16 / 32 /
//             64); an integer type is ANDed with the descriptor's mask (0xFFFFFFFF: none); a floating type is bit-cast from
//             the integer - a swapped float pattern is never held in a floating register before the swap, where a signalling
//             NaN pattern could be quieted -; then (double), exact for every T.
// What is staged in LDS is the decoded T, so that the second conversion (from LDS, for Xt) runs the same operations on the
// same operand as the first (from the register, for X): the same doubles, cc_ingest.h's argument.  LDS pitch and walks:
// cc_ingest_pitch<T>(), as there.  cc_ingest_widen<SCALED> is reused as it is; the finiteness test is compiled in for the
// floating types and for every SCALED instance, the magnitude maximum for all.
// T: float, double, uint8_t, uint16_t, uint32_t - the element types list-mode FCS data has; 20 instances.
// ---------------------------------------------------------------------------------

struct cc_list_desc {
    int col;        // source column of this selected dimension, 0 .. src_cols - 1
    unsigned mask;  // AND mask of an integer element (0xFFFFFFFF: none); unused for the floating types
};

template <typename T> struct cc_list_bits;
template <> struct cc_list_bits<double> { typedef unsigned long long type; };
template <> struct cc_list_bits<float> { typedef unsigned int type; };
template <> struct cc_list_bits<uint32_t> { typedef unsigned int type; };
template <> struct cc_list_bits<uint16_t> { typedef unsigned short type; };
template <> struct cc_list_bits<uint8_t> { typedef unsigned char type; };

// the decoded element at `at` (naturally aligned): load as an integer, swap, mask (integers) or bit-cast (floating)
template <typename T, bool SWAP>
__device__ __forceinline__ T cc_list_decode(const void* __restrict__ at, unsigned mask)
{
    typedef typename cc_list_bits<T>::type U;
    U u = *static_cast<const U*>(at);
    if (SWAP) {
        if (sizeof(U) == 8) u = (U)__builtin_bswap64((unsigned long long)u);
        else if (sizeof(U) == 4) u = (U)__builtin_bswap32((unsigned int)u);
        else if (sizeof(U) == 2) u = (U)__builtin_bswap16((unsigned short)u);
    }
    if (!cc_ingest_elem<T>::floating) u = (U)(u & (U)mask);
    T t;
    __builtin_memcpy(&t, &u, sizeof(T));
    return t;
}

template <typename T, bool SWAP, bool SCALED>
__global__ __launch_bounds__(256) void k_ingest_list(const unsigned char* __restrict__ raw, int src_cols, int ns, long long s0,
                                                     long long n_total, int d, int xt_rows,
                                                     const cc_list_desc* __restrict__ desc, double* __restrict__ X,
                                                     double* __restrict__ Xt, const double* __restrict__ scale,
                                                     const double* __restrict__ mn, int* __restrict__ bad)
{
    constexpr int PITCH = cc_ingest_pitch<T>();
    constexpr bool CHECK = cc_ingest_elem<T>::floating || SCALED;
    __shared__ T tile[CC_INGEST_TILE * PITCH];
    __shared__ int s_col[CC_INGEST_TILE];
    __shared__ unsigned s_mask[CC_INGEST_TILE];
    __shared__ unsigned long long s_m;
    const int p0 = (int)blockIdx.x * CC_INGEST_TILE;  // the tile's first point, in the slab
    const int np = ns - p0 < CC_INGEST_TILE ? ns - p0 : CC_INGEST_TILE;
    const int c0 = (int)blockIdx.y * CC_INGEST_TILE;
    const int db = d - c0 < CC_INGEST_TILE ? d - c0 : CC_INGEST_TILE;
    if (threadIdx.x == 0) s_m = 0ull;
    if ((int)threadIdx.x < db) {
        const cc_list_desc e = desc[c0 + threadIdx.x];
        s_col[threadIdx.x] = e.col;
        s_mask[threadIdx.x] = e.mask;
    }
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
    double m = 0.0;
    const unsigned char* __restrict__ src = raw + (size_t)p0 * (size_t)src_cols * sizeof(T);  // the tile's first record
    for (int e = (int)threadIdx.x; e < tot; e += 256) {
        const T f = cc_list_decode<T, SWAP>(src + ((size_t)p * (size_t)src_cols + (size_t)s_col[c]) * sizeof(T), s_mask[c]);
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
    if (CHECK && __any(b) && lane == 0) atomicOr(bad, 1);
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(m, off);
        m = o > m ? o : m;
    }
    if (lane == 0) atomicMax(&s_m, (unsigned long long)__double_as_longlong(m));
    __syncthreads();
    if (threadIdx.x == 0 && s_m != 0ull) atomicMax(reinterpret_cast<unsigned long long*>(bad + 2), s_m);
}

// Per-selected-column minimum / maximum of a slab of event records in device staging (n records), NaN ignored:
// k_col_minmax_view's rows form (cc_ingest.h) with k_ingest_list's addressing and decoding - partials part[2][chunks][d] over
// the slab's row chunks, one workgroup per (row chunk, block of 256 selected columns); a thread keeps one descriptor.
template <typename T, bool SWAP>
__global__ __launch_bounds__(256) void k_col_minmax_list(const unsigned char* __restrict__ raw, long long n, int src_cols, int d,
                                                         const cc_list_desc* __restrict__ desc, double* __restrict__ part,
                                                         int chunks)
{
    const long long per = (n + chunks - 1) / chunks;
    const long long r0 = (long long)blockIdx.x * per, r1 = (r0 + per < n) ? r0 + per : n;
    double mn = CC_INF, mx = -CC_INF;
    __shared__ double smn[256], smx[256];
    // this workgroup's columns c0 .. c0 + db - 1: thread t handles column c0 + t % db of rows t / db, t / db + rows_per_pass, ...
    const int c0 = (int)blockIdx.y * 256;
    const int db = (d - c0) < 256 ? d - c0 : 256;
    const int rows_per_pass = 256 / db;
    const int col = (int)(threadIdx.x % db);
    const int rsub = (int)(threadIdx.x / db);
    if (rsub < rows_per_pass) {
        const cc_list_desc e = desc[c0 + col];
        for (long long r = r0 + rsub; r < r1; r += rows_per_pass) {
            const double v = (double)cc_list_decode<T, SWAP>(raw + ((size_t)r * (size_t)src_cols + (size_t)e.col) * sizeof(T), e.mask);
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
