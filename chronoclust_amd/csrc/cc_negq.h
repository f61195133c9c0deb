// chronoclust_amd/csrc: an exact order statistic per selected column over the NEGATIVE compensated values of list-mode events
// that stream through staging (cc_negq_begin / _add_list / _select / _end, cc_api_negq.inc): what the rule of Parks, Roederer
// and Moore 2006 takes the logicle width W from - the 5th percentile of the negative values of a channel, pooled over every
// timepoint of a series.  The values are those of cc_xf_value<T, SWAP, false> with cofactor 0: decoded, masked, compensated by
// the source's own inverse spillover matrix (the left-to-right sum of k_ingest_list_xf, bit for bit), nothing else.
// (included by cc_online.h behind cc_ingest_list_xf.h; one translation unit, cc_api.hip)
//
// The plan is dense and has no global atomics: every result is a function of the values alone, whatever the order the
// workgroups run in.
//   k_negq_stage<T, SWAP>  per staged slab: the value of every WANTED dimension into val[wanted dimension][capacity] at the
//                          slab's event offset - k_ingest_list_xf's tiling, staging and LDS transpose, one 512-byte segment per
//                          wave and dimension.  Nothing else is written.
//   the selection          a most-significant-digit radix select over the 64-bit pattern, 8 passes of 8 bits.  For v < 0 the
//                          complement of the bits orders as the values do (the key; NaN and +-0 are not negative, so keys and
//                          values are one to one; -Inf has the smallest key).  A pass is two launches: k_negq_hist - grid
//                          (chunks, wanted dimensions), a 256-bin LDS histogram of the negative elements that match the prefix
//                          found so far, stored with plain stores to hist[dimension][chunk][256] - and k_negq_pick - one
//                          workgroup per wanted dimension folds the chunks, finds the digit that holds the rank and updates
//                          prefix, remaining rank and the count below in the dimension's state on the device.  Pass 0's total
//                          is cnt: the rank j = floor((cnt - 1) q) and frac are formed there, in double.
//   the successor          k_negq_next (per chunk the smallest key above lo's) and k_negq_done (folds them, decides whether hi
//                          is lo again - a tie that reaches rank j + 1, or j the last rank - and writes cnt, lo, hi, frac).
// Every launch is made whatever the data holds, every loop's trip count is a function of the sizes alone: cnt == 0 runs the
// same eighteen launches and yields cnt = 0, lo = hi = frac = 0.  Nothing waits on a flag, nothing is retried.
#pragma once

#define CC_NEGQ_THREADS 256   // threads of a workgroup of the selection
#define CC_NEGQ_CHUNK 8192    // elements of a column a workgroup of k_negq_hist / k_negq_next takes: 32 per thread
#define CC_NEGQ_STATE 8       // words of a dimension's state

// a dimension's state, unsigned 64-bit words: st[dimension][CC_NEGQ_STATE]
enum { CC_NQ_PREFIX = 0, CC_NQ_RANK, CC_NQ_BELOW, CC_NQ_CNT, CC_NQ_J, CC_NQ_FRAC, CC_NQ_MULT };

__device__ __forceinline__ unsigned long long cc_negq_key(double v)
{
    return ~(unsigned long long)__double_as_longlong(v);
}

// ---------------------------------------------------------------------------------
// k_negq_stage<T, SWAP>: grid (tiles of 64 events of the slab, blocks of 64 selected dimensions), 256 threads.  wmap[d]: the
// row of `val` a selected dimension is written to, -1: not wanted (its value is not computed).  The slab's ns events start at
// event s0 of the pooled `cap` (s0 + ns <= cap: the host's check).  LDS: k_ingest_list_xf's without the cofactors.
// ---------------------------------------------------------------------------------
template <typename T, bool SWAP>
__global__ __launch_bounds__(256) void k_negq_stage(const unsigned char* __restrict__ raw, int src_cols, int ns, long long s0,
                                                    long long cap, int d, const cc_list_desc* __restrict__ desc, cc_list_xf xf,
                                                    const int* __restrict__ wmap, double* __restrict__ val)
{
    constexpr int XP = cc_ingest_pitch<T>();
    constexpr int VP = CC_INGEST_TILE + 1;
    __shared__ double vs[CC_INGEST_TILE * VP];
    __shared__ T xs[CC_INGEST_TILE * XP];
    __shared__ int s_col[CC_INGEST_TILE];
    __shared__ unsigned s_mask[CC_INGEST_TILE];
    __shared__ int s_sel[CC_INGEST_TILE];
    __shared__ int s_row[CC_INGEST_TILE];
    const int p0 = (int)blockIdx.x * CC_INGEST_TILE;  // the tile's first event, in the slab
    const int np = ns - p0 < CC_INGEST_TILE ? ns - p0 : CC_INGEST_TILE;
    const int c0 = (int)blockIdx.y * CC_INGEST_TILE;
    const int db = d - c0 < CC_INGEST_TILE ? d - c0 : CC_INGEST_TILE;
    const int m = xf.m;
    const unsigned char* __restrict__ src = raw + (size_t)p0 * (size_t)src_cols * sizeof(T);  // the tile's first record
    if ((int)threadIdx.x < db) {
        const cc_list_desc e = desc[c0 + threadIdx.x];
        s_col[threadIdx.x] = e.col;
        s_mask[threadIdx.x] = e.mask;
        s_sel[threadIdx.x] = m > 0 ? xf.sel[c0 + threadIdx.x] : -1;
        s_row[threadIdx.x] = wmap[c0 + threadIdx.x];
    }
    if (m > 0) cc_xf_stage<T, SWAP, XP>(xs, src, src_cols, np, m, xf.ccol, xf.cmask);
    __syncthreads();
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    // element e of the tile in row order = (event e / db, dimension e % db); a thread's elements are 256 apart
    const int tot = np * db, step_p = 256 / db, step_c = 256 - step_p * db;
    int p = (int)threadIdx.x / db, c = (int)threadIdx.x - p * db;
    for (int e = (int)threadIdx.x; e < tot; e += 256) {
        if (s_row[c] >= 0)
            vs[p * VP + c] = cc_xf_value<T, SWAP, false>(xs + p * XP, src + (size_t)p * (size_t)src_cols * sizeof(T), s_col[c], s_mask[c],
                                                         s_sel[c], m, xf.comp, 0.0, cc_lgc{});
        p += step_p;
        c += step_c;
        if (c >= db) {
            c -= db;
            ++p;
        }
    }
    __syncthreads();
    if (lane < np)
        for (int i = wave; i < db; i += 4) {
            const int row = s_row[i];
            if (row >= 0) val[(size_t)row * (size_t)cap + (size_t)(s0 + p0) + lane] = vs[lane * VP + i];
        }
}

// ---------------------------------------------------------------------------------
// k_negq_hist: grid (chunks, wanted dimensions).  The workgroup's CC_NEGQ_CHUNK elements of column blockIdx.y, 256 at a time: an
// element counts where it is negative and its key matches the prefix above this pass's digit.  The high digits of values that
// share sign and exponent are all but one value: where every counting lane of a wave holds the same digit, one lane adds the
// ballot's population count; else every counting lane adds 1 (LDS atomics: no loop behind them).  The 256 counts leave with one
// plain store per thread.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_NEGQ_THREADS) void k_negq_hist(const double* __restrict__ val, long long cap, long long n,
                                                               const unsigned long long* __restrict__ st, int pass,
                                                               unsigned* __restrict__ hist, int chunks)
{
    __shared__ unsigned h[256];
    const int w = (int)blockIdx.y;
    h[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned long long prefix = pass ? st[(size_t)w * CC_NEGQ_STATE + CC_NQ_PREFIX] : 0ull;
    const unsigned long long above = pass ? ~0ull << (64 - 8 * pass) : 0ull;  // the digits already found
    const int shift = 56 - 8 * pass;
    const double* __restrict__ col = val + (size_t)w * (size_t)cap;
    const long long e0 = (long long)blockIdx.x * CC_NEGQ_CHUNK + (long long)threadIdx.x;
    const int lane = (int)threadIdx.x & 63;
#pragma unroll 4
    for (int it = 0; it < CC_NEGQ_CHUNK / CC_NEGQ_THREADS; ++it) {
        const long long i = e0 + (long long)it * CC_NEGQ_THREADS;
        const double v = i < n ? col[i] : 0.0;
        const unsigned long long key = cc_negq_key(v);
        const bool counts = v < 0.0 && ((key ^ prefix) & above) == 0ull;
        const unsigned dig = (unsigned)(key >> shift) & 255u;
        const unsigned long long who = __ballot(counts);
        if (who == 0ull) continue;  // (wave-uniform)
        const int first = __ffsll((long long)who) - 1;
        const unsigned d0 = (unsigned)__shfl((int)dig, first);
        const unsigned long long same = __ballot(counts && dig == d0);
        if (same == who) {
            if (lane == first) atomicAdd(&h[d0], (unsigned)__popcll(who));
        } else if (counts) {
            atomicAdd(&h[dig], 1u);
        }
    }
    __syncthreads();
    hist[((size_t)w * (size_t)chunks + blockIdx.x) * 256 + threadIdx.x] = h[threadIdx.x];
}

// ---------------------------------------------------------------------------------
// k_negq_pick: one workgroup per wanted dimension.  Thread t folds bin t over the chunks; thread 0 then walks the 256 totals
// (always all of them) to the digit that holds the remaining rank.  Pass 0: cnt is the total, h = (cnt - 1) q in double,
// j = floor(h), frac = h - j (cnt == 0: all zero).  The last pass leaves lo's key in PREFIX, the count of smaller keys in BELOW
// and lo's multiplicity in MULT.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_NEGQ_THREADS) void k_negq_pick(const unsigned* __restrict__ hist, int chunks, int pass, double q,
                                                               unsigned long long* __restrict__ st)
{
    __shared__ unsigned long long tot[256];
    const int w = (int)blockIdx.x;
    const unsigned* __restrict__ hw = hist + (size_t)w * (size_t)chunks * 256 + threadIdx.x;
    unsigned long long sum = 0ull;
    for (int c = 0; c < chunks; ++c) sum += hw[(size_t)c * 256];
    tot[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long* __restrict__ s = st + (size_t)w * CC_NEGQ_STATE;
    unsigned long long prefix = 0ull, rank = 0ull, below = 0ull;
    if (pass == 0) {
        unsigned long long cnt = 0ull;
        for (int b = 0; b < 256; ++b) cnt += tot[b];
        double frac = 0.0;
        if (cnt > 0ull) {
            const double hq = (double)(cnt - 1ull) * q;
            const double fl = floor(hq);
            rank = (unsigned long long)fl;
            if (rank > cnt - 1ull) rank = cnt - 1ull;  // (q <= 1: never; the selection below relies on it)
            frac = hq - fl;
        }
        s[CC_NQ_CNT] = cnt;
        s[CC_NQ_J] = rank;
        s[CC_NQ_FRAC] = (unsigned long long)__double_as_longlong(frac);
    } else {
        prefix = s[CC_NQ_PREFIX];
        rank = s[CC_NQ_RANK];
        below = s[CC_NQ_BELOW];
    }
    unsigned long long cum = 0ull, mult = 0ull;
    unsigned dig = 0u;
    bool found = false;
    for (int b = 0; b < 256; ++b) {
        const unsigned long long c = tot[b];
        if (!found && cum + c > rank) {
            found = true;
            dig = (unsigned)b;
            mult = c;
        }
        if (!found) cum += c;
    }
    if (!found) cum = 0ull;  // (cnt == 0: every total is zero)
    s[CC_NQ_PREFIX] = prefix | ((unsigned long long)dig << (56 - 8 * pass));
    s[CC_NQ_RANK] = rank - cum;
    s[CC_NQ_BELOW] = below + cum;
    s[CC_NQ_MULT] = mult;
}

// the smallest of a workgroup's keys: the waves by shuffles, the four of them through LDS; the result on thread 0
__device__ __forceinline__ unsigned long long cc_negq_block_min(unsigned long long k, unsigned long long* __restrict__ sm)
{
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off);
        k = o < k ? o : k;
    }
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < CC_NEGQ_THREADS / 64; ++i) k = sm[i] < k ? sm[i] : k;
    return k;
}

// k_negq_next: grid (chunks, wanted dimensions): the smallest key of the chunk's negative elements above lo's key, all ones where
// there is none (no negative value has that key: it is +0.0's) - nxt[dimension][chunk]
__global__ __launch_bounds__(CC_NEGQ_THREADS) void k_negq_next(const double* __restrict__ val, long long cap, long long n,
                                                               const unsigned long long* __restrict__ st,
                                                               unsigned long long* __restrict__ nxt, int chunks)
{
    __shared__ unsigned long long sm[CC_NEGQ_THREADS / 64];
    const int w = (int)blockIdx.y;
    const unsigned long long lo = st[(size_t)w * CC_NEGQ_STATE + CC_NQ_PREFIX];
    const double* __restrict__ col = val + (size_t)w * (size_t)cap;
    const long long e0 = (long long)blockIdx.x * CC_NEGQ_CHUNK + (long long)threadIdx.x;
    unsigned long long best = ~0ull;
#pragma unroll 4
    for (int it = 0; it < CC_NEGQ_CHUNK / CC_NEGQ_THREADS; ++it) {
        const long long i = e0 + (long long)it * CC_NEGQ_THREADS;
        const double v = i < n ? col[i] : 0.0;
        const unsigned long long key = cc_negq_key(v);
        if (v < 0.0 && key > lo && key < best) best = key;
    }
    best = cc_negq_block_min(best, sm);
    if (threadIdx.x == 0) nxt[(size_t)w * (size_t)chunks + blockIdx.x] = best;
}

// k_negq_done: one workgroup per wanted dimension: out[dimension] = {cnt, bits of lo, bits of hi, bits of frac}.  hi is lo
// again where lo's tie reaches rank j + 1 (BELOW + MULT >= j + 2) or j is the last rank; else the smallest key above lo's.
__global__ __launch_bounds__(CC_NEGQ_THREADS) void k_negq_done(const unsigned long long* __restrict__ nxt, int chunks,
                                                               const unsigned long long* __restrict__ st,
                                                               unsigned long long* __restrict__ out)
{
    __shared__ unsigned long long sm[CC_NEGQ_THREADS / 64];
    const int w = (int)blockIdx.x;
    unsigned long long best = ~0ull;
    for (int c = (int)threadIdx.x; c < chunks; c += CC_NEGQ_THREADS) {
        const unsigned long long k = nxt[(size_t)w * (size_t)chunks + c];
        best = k < best ? k : best;
    }
    best = cc_negq_block_min(best, sm);
    if (threadIdx.x != 0) return;
    const unsigned long long* __restrict__ s = st + (size_t)w * CC_NEGQ_STATE;
    const unsigned long long cnt = s[CC_NQ_CNT], j = s[CC_NQ_J];
    unsigned long long lo = 0ull, hi = 0ull, frac = 0ull;
    if (cnt > 0ull) {
        lo = ~s[CC_NQ_PREFIX];
        const bool again = s[CC_NQ_BELOW] + s[CC_NQ_MULT] >= j + 2ull || j + 1ull > cnt - 1ull;
        hi = again ? lo : ~best;
        frac = s[CC_NQ_FRAC];
    }
    out[(size_t)w * 4] = cnt;
    out[(size_t)w * 4 + 1] = lo;
    out[(size_t)w * 4 + 2] = hi;
    out[(size_t)w * 4 + 3] = frac;
}
