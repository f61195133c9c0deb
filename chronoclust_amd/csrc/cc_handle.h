// cc_handle.h — the handle behind the C-ABI and what every part of the host side needs of it: the RAII device buffers,
// the microcluster table's columns, the members of cc_handle in groups by concern, error handling (guarded), the control
// block's push / pull, and the growth of the table and the window buffers.  (included by cc_api.hip, the one translation unit)
#pragma once
#include "cc_knobs.h"
#include "cc_ingest_src.h"

namespace {

struct HipErr {
    hipError_t e;
    const char* what;
};

#define HIPCHK(call)                                  \
    do {                                              \
        hipError_t _e = (call);                       \
        if (_e != hipSuccess) throw HipErr{_e, #call}; \
    } while (0)

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    void ensure(size_t count)
    {
        if (count <= n && p) return;
        release();
        size_t want = std::max<size_t>(count, 1);
        if (hipMalloc((void**)&p, want * sizeof(T)) != hipSuccess) {
            p = nullptr;
            throw HipErr{hipErrorOutOfMemory, "hipMalloc"};
        }
        n = want;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { release(); swap(o); }
        return *this;
    }
    void swap(DevBuf& o) noexcept
    {
        std::swap(p, o.p);
        std::swap(n, o.n);
    }
};

// The microcluster table, one device buffer per column.  for_each_column names every column once, with what a row holds of
// it and what becomes of it when the table grows (ensure_table); a column added there is allocated, grown and - the buffers
// are movable - swapped with the rest.  view() alone spells them out again: its order is Table's.
struct TableStore {
    DevBuf<double> cf1, cf2, cen, pref, scl, w;
    DevBuf<int> kind, key;
    DevBuf<long long> id, uid;
    DevBuf<unsigned long long> touch, last, carry_of, cnt;
    DevBuf<int> memb, clen, heavy;
    size_t cap = 0;
    int d = 0;
    // a column of a grown table: the first m_rows rows copied from the old one, the whole column cleared, both (cleared, then
    // the live rows copied), or left as allocated (scratch that is written before it is read)
    enum Grow { KEPT, CLEARED, CLEARED_KEPT, SCRATCH };
    // f(pointer to the member, elements per row, Grow) for a table of `dims` dimensions
    template <typename F>
    static void for_each_column(int dims, F&& f)
    {
        const size_t dim = (size_t)dims;
        f(&TableStore::cf1, dim, KEPT); f(&TableStore::cf2, dim, KEPT); f(&TableStore::cen, dim, KEPT);
        f(&TableStore::pref, dim, KEPT); f(&TableStore::scl, dim, KEPT);
        f(&TableStore::w, (size_t)1, KEPT); f(&TableStore::kind, (size_t)1, KEPT); f(&TableStore::key, (size_t)1, KEPT);
        f(&TableStore::id, (size_t)1, KEPT); f(&TableStore::uid, (size_t)1, KEPT);
        f(&TableStore::touch, (size_t)2, CLEARED); f(&TableStore::last, (size_t)2, CLEARED);
        // (the carry marks of the last commit are live state: the next window may be a lookahead window)
        f(&TableStore::carry_of, (size_t)1, CLEARED_KEPT);
        f(&TableStore::cnt, (size_t)1, CLEARED); f(&TableStore::memb, (size_t)CC_CHAIN_MEMB, SCRATCH);
        f(&TableStore::clen, (size_t)1, CLEARED);
        // (heavy marks index rows like the list in the control block: they move with the table)
        f(&TableStore::heavy, (size_t)1, CLEARED_KEPT);
    }
    void alloc(size_t rows, int dim)
    {
        for_each_column(dim, [&](auto col, size_t per_row, Grow) { (this->*col).ensure(rows * per_row); });
        // (only once every column is there: an allocation that fails part way leaves a table that will be allocated again)
        cap = rows;
        d = dim;
    }
    Table view() const { return Table{cf1.p, cf2.p, cen.p, pref.p, scl.p, w.p, kind.p, key.p, id.p, uid.p, touch.p, last.p, carry_of.p, cnt.p, memb.p, clen.p, heavy.p, cap}; }
};

// The clusters of the last offline phase, flat: cluster c = members [off[c], off[c + 1]) of `mem`, pcore list positions in
// merge order (a vector per cluster cost 5 000 allocations per call at C2: 350 us of the ordered expansion's 380)
struct HostClusters {
    std::vector<int> mem, off{0};
    size_t size() const { return off.size() - 1; }
    void clear() { mem.clear(); off.assign(1, 0); }
};

}  // namespace

// Page-locked host scratch for the small read-backs and uploads of a call (offline phase: row order, flags, counts, lists):
// a copy to or from pageable memory is driven by the host thread - it first waits for the stream to drain -, one to or from
// page-locked memory is a stream operation; six to ten of them per cc_offline call were 300 us of idle device.  Bump
// allocation per call (`reset`), never freed in between; growing it (rare) drains the stream first.
struct PinArena {
    char* p = nullptr;
    size_t cap = 0, used = 0;
    void reset() { used = 0; }
    void reserve(size_t bytes)
    {
        if (bytes <= cap) return;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = std::max<size_t>(bytes, (size_t)1 << 20);
        if (hipHostMalloc((void**)&p, want, hipHostMallocDefault) != hipSuccess) {
            p = nullptr;
            throw HipErr{hipErrorOutOfMemory, "hipHostMalloc"};
        }
        cap = want;
    }
    template <typename T>
    T* take(size_t n)  // (within what reserve() was given)
    {
        used = (used + 63) & ~(size_t)63;
        T* r = reinterpret_cast<T*>(p + used);
        used += std::max<size_t>(n, 1) * sizeof(T);
        if (used > cap) throw HipErr{hipErrorOutOfMemory, "page-locked scratch exhausted"};
        return r;
    }
    ~PinArena() { if (p) (void)hipHostFree(p); }
    PinArena() = default;
    PinArena(const PinArena&) = delete;
    PinArena& operator=(const PinArena&) = delete;
};

// How the clean snapshot scans of an online call run for the handle's d, pdim filter, k and knobs (scan_plan(): read by the
// dispatcher, the window policy's configuration and the partial counts).  Two thresholds are in table rows, which grow.
struct ScanPlan {
    int dp = 0;            // padded dimensionality: the ladder 4 / 8 / 14 / 16 / 20 / 32 / 40 / 64 (0: not planned yet)
    // the plain scan is k_scan_u (k a power of two, no pdim filter; d on the ladder, or 9 <= d <= 64 over padded operands),
    // else k_scan<FILTER, POW2>.  cc::scan_width (cc_batch.h) is the rule for this and for the chain, before the knobs.
    bool scan_u = false;
    // d is off the ladder: every snapshot scan reads the rows' centroids and operands from a mirror at stride dp that
    // k_pad_rows rebuilds in front of it (padded_rows(), cc_api.hip); the points' dimension-major copy has dp rows
    bool pad_rows = false;
    // the pruned chain: COMMON where k_scan_u applies and d > 8; GENERAL (k_scan_p3<GENERAL>) where the pdim filter is on or k
    // is not a power of two (on the ladder only)
    enum Chain { NONE, COMMON, GENERAL } chain = NONE;
    // its scan of a window: k_scan_p3, k_scan_p2 or k_scan_p - the split form k_scan_a + k_scan_p<MASKED> from split_rows table
    // rows on -; k_scan_p3 LISTED from listed_rows table rows on
    enum Form { P3, P2, P1 } form = P1;
    long long split_rows = std::numeric_limits<long long>::max(), listed_rows = 0;
    bool seed16 = false;  // the window's seeded chain: seeds from k_seed16 with the tight threshold, not from k_seed
    int prune_applicable = 0, allow_guess = 0, allow_probe = 0, force_prune_rows = 0;  // (cc_policy_config)
    int waves = 4, dirty_waves = 4;  // waves per workgroup of the clean / dirty scans
    int plain_wgs_per_cu = 1, prune_wgs_per_cu = 1;  // resident workgroups of the plain scan / those a pruned one is split into
    bool split(long long m_rows) const { return m_rows >= split_rows; }
    bool listed(long long m_rows) const { return m_rows >= listed_rows; }
};

// ---- the members of cc_handle, in groups by concern.  cc_handle inherits from them, so a member is h->name whatever its group.

// what the window policy decided for the batch of windows being enqueued, as the scan dispatcher reads it
struct BatchScanState {
    bool prune_now = false;   // this batch's snapshot scans are pruned ones (set per batch by online_range)
    bool group_guess_now = false;     // ... and the missed points derived from the gathered records (k_missed_g), see timed_scan
    bool lean_now = false;    // ... guessed thresholds without k_missed / the seeded chain for missed points (cc_policy_decision::prune == 3)
    bool guess_now = false;   // ... with guessed thresholds (k_scan_p + k_missed + the seeded chain for the missed points)
    bool probe_now = false;   // the next plain scan also runs the pruned chain on 128 points (cc_policy_decision::probe)
    ScanPlan scan_plan;       // how this call's snapshot scans run (set per online call by OnlineRun::prepare)
    // the policy's cc_policy_decision::prune as the three flags above
    void set_prune(int prune)
    {
        prune_now = prune != 0;
        guess_now = prune >= 2;
        lean_now = prune == 3;
    }
};

// buffers of the pruned snapshot scans (sized by ensure_window_buffers, ensure_prefix16, ensure_pad_rows and the dispatcher)
struct PrunedScanBuffers {
    DevBuf<Cand> probe_part;  // the probe's scratch partials (BatchScanState::probe_now)
    DevBuf<unsigned long long> found;  // [2][CC_MAX_WINDOW / 64] per point tile: the points a guessed-threshold scan found a pcore MC for
    DevBuf<int> missed;                // [2][CC_MISSED_CAP] the others, listed by k_missed (two window parities)
    DevBuf<SeedCand> spart;   // [2][window, S, 2]  prefix-score winners per workgroup sub-range and kind (two window parities)
    DevBuf<double> thr;       // [2][window, 2]     abandon thresholds per point and kind
    DevBuf<float> thr32;      // [2][window, 2]     ... and what phase A's single-precision prefix sums are compared with
    DevBuf<unsigned long long> cmax;  // [2]        largest |centroid coordinate| of the scanned prefixes (bits of a double)
    DevBuf<cc_h8> a16;        // [2][(table capacity + 64) x 4]  k_prefix16: the table rows as half-precision operands of the MFMA prefix test (two window parities)
    DevBuf<Prefix16Hdr> hdr16;  // [2]              ... origin and scale they were converted with
    size_t a16_stride = 0;
    DevBuf<unsigned> masks;   // [2][tiles of 128 points, sub-ranges, words per sub-range]  k_scan_a's survivor masks (two window parities)
    size_t mask_stride = 0;
    DevBuf<double> pad_cen, pad_scl;  // [2][(table capacity + 16) x dp]  k_pad_rows: the scanned rows' centroids / operands at stride dp (two window parities)
    size_t pad_stride = 0;
    size_t spart_stride = 0, thr_stride = 0;
};

// window buffers: the versions of a window's rows, the scans' partials, the carry set, the validation kernels' lists, and the
// scan copies of the table (sized by ensure_window_buffers / scan_copy_sync)
struct WindowBuffers {
    int win_alloc = 0, seg_alloc = 0, d_alloc = 0;
    DevBuf<double> v_cf1, v_cf2, v_cen, v_pref, v_scl, v_w, v_dsq, v_tau;
    DevBuf<unsigned long long> v_tile_dsq;
    DevBuf<int> v_kind, v_key, v_next, v_upg, v_acc, v_tgt, v_skip, v_skip_car, v_unsafe;
    DevBuf<Cand> part, clean, dpart, dpart2, dseed;  // part: two copies (window parity), dpart2: carry-set scan
    size_t part_stride = 0;
    // carry set of the previous window (lookahead)
    DevBuf<double> c_cf1v, c_cf2v, c_cenv, c_prefv, c_sclv, c_wv, c_c0, c_w0, c_dsq;
    DevBuf<int> c_kind, c_key, c_slot, c_kind0;
    DevBuf<unsigned long long> c_tile_dsq;
    DevBuf<int> T0, T1, rk;
    DevBuf<int> link_near;    // [window] k_link_scan: per window point that decided "create", the earliest such point before it that would absorb it
    DevBuf<int> sp_list;      // [window] the round's list of points for the sparse dirty scans
    DevBuf<int> long_list;    // [2][CC_LONG_CAP] MCs whose chain k_chain_long replays (tables beyond k_claims' reach)
    DevBuf<unsigned long long> lstat, lprev;  // [2][CC_LSTAT_ROWS] / [CC_MAX_WINDOW]: long chains laid out ahead of k_chain (k_chain_long<.., true>)
    bool prep_launched = false;  // (this call: the counters behind lstat are worth reading)
    DevBuf<CommitRec> rec;
    // scan copy of the table for lookahead scans (see ScanCopy)
    DevBuf<double> sh_cen[2], sh_scl[2], sh_cf1[2], sh_cf2[2], sh_w[2];
    DevBuf<int> sh_kind[2], sh_key[2];
    DevBuf<int8_t> dpath;
};

// results of the last offline phase and the scratch it runs on
struct OfflineResults {
    DevBuf<double> pv_cf1, pv_cf2, pv_cen, pv_pref, pv_w, wvec;
    DevBuf<long long> pv_id;
    DevBuf<int> prow, nn, pdim, mem_dev, off_dev, nw_cnt, nw_nbr;
    DevBuf<long long> nw_off;
    DevBuf<int8_t> core;
    DevBuf<unsigned long long> adj, adjw;
    DevBuf<double> c_cf1, c_cf2, c_cen, c_pref, c_w;
    HostClusters clusters;
    PinArena pin;  // page-locked scratch of the current call
    std::vector<long long> pcore_ids_host, pcore_uid_host;  // ids / creation numbers of the pcores, list order
    DevBuf<int32_t> pc_map, pc_out;                         // cc_point_clusters: creation number -> cluster, result
    int n_core = 0;
};

// association scratch
struct AssocScratch {
    DevBuf<double> a_cur_cen, a_cur_pref, a_prev_cen, a_dist, a_pdist;
    DevBuf<int> a_idx, a_pidx;
    DevBuf<int> flags;
};

// relaxed multi-GPU mode (events sharded over the ranks)
struct RelaxedState {
    int relaxed_minibatch = 0;     // points per rank and super-step (0: the exact path)
    bool shard_suspended = false;  // inside a relaxed super-step the ranks cluster different points: no split scans
    DevBuf<double> rs_cf1, rs_cf2, rs_w, r_delta, r_gather;   // snapshot of the shared table, deltas, all-reduce scratch
    DevBuf<int> rs_kind, rs_key, r_didx, r_didx_all, r_cnt_all;
    DevBuf<long long> rs_id;
    DevBuf<double> rg_X, rg_Xt;                               // the set-aside points of a super-step, gathered
    DevBuf<long long> rg_uid;
    DevBuf<int8_t> rg_path;
    cc_relaxed_stats rstats{};
};

// cc_assign: the chunk buffers of the read-only assignment, two sets (one per stream; cc_api_assign.inc) - the points of a
// chunk row-major and dimension-major, the segments' partial bests, the chunk's results, k_check_finite's words; raw: the
// chunk as it arrives in single precision (cc_assign_f32: k_ingest_f32 fills X and Xt from it)
struct AssignBuffers {
    struct Set {
        DevBuf<double> X, Xt, dist;
        DevBuf<float> raw;
        DevBuf<long long> uid;
        DevBuf<int8_t> path;
        DevBuf<Cand> part;
        DevBuf<int> bad;
    } asg[2];
};

struct cc_handle : Knobs, BatchScanState, PrunedScanBuffers, WindowBuffers, OfflineResults, AssocScratch, RelaxedState, AssignBuffers {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // lookahead scans
    std::string err;
    cc_params par{};
    bool have_par = false;
    cc_tuning tun{};
    cc_stats stats{};

    int d = 0;
    TableStore tab, tab2;
    Ctl hc{};  // host mirror of the device control block
    Ctl* hc_pin = nullptr;  // two page-locked staging blocks for it (read-back between batches / restart push)
    DevBuf<Ctl> ctl;
    // a pruned scan's sample {rows visited, rows completed} per window parity: Ctl::pstat, as the kernels take it
    unsigned long long* pstat_p() const { return (unsigned long long*)((char*)ctl.p + offsetof(Ctl, pstat)); }
    // a stored preference entry outside {1, k} may be present (cc_set_params with another k on a table that holds rows,
    // cc_inject_mc / cc_inject_bulk; cleared by cc_reset).  Two consequences: never the x * (1/k) shortcut (Ctl::pow2 = 0,
    // refresh_ctl_params), and no pruned chain (scan_plan, cc_api.hip): the prefix bounds of cc_tau16, cc_tau32 and cc_thr32
    // take min(1, 1 / k) for the smallest weight of a dimension, which a stored entry above max(k, 1) undercuts
    bool tainted = false;
    int adapt_win = 0;      // window size the last call settled at (0: none yet)
    int clean_batches = 0;  // consecutive batches without a truncated window
    int since_shrink = 1000;  // batches since the window was last shrunk
    DevBuf<int> seq_lists;      // [2][table capacity] k_seq_g: rows of the pcore MCs / of the outlier MCs
    DevBuf<double> seq_img;     // [4][d][table capacity] k_seq_g: dimension-major copy of the rows it scans (centroid, operand, CF1, CF2)
    bool seq_sticky = false;    // the last call ended on the sequential kernel (k_seq): the next one starts there
    int n_cus = 256;            // compute units of the device (hipDeviceProp_t::multiProcessorCount)
    int wall_khz = 0;           // rate of the device's constant clock (hipDeviceAttributeWallClockRate; 0: unknown, no stamps)

    // points + labels of the current call
    DevBuf<double> X, Xt;
    long long n_points = 0;
    double x_absmax = 0.0;     // the largest |coordinate| of the resident points (k_check_finite)
    DevBuf<long long> lab_uid;
    DevBuf<int8_t> lab_path;
    DevBuf<int> badflag;
    DevBuf<double> scr, scr2;  // scaler scratch
    DevBuf<float> ingest_raw[2];  // a staged source (IngestSrc): the two slabs of device staging of an upload / a column reduction, in bytes
    long long f32_points = 0;     // cc_f32_points: points taken in single precision since cc_create
    long long view_points = 0;    // cc_view_points: points taken through the `_view` entry points since cc_create (they share ingest_raw, in bytes)
    long long list_points = 0;    // cc_list_points: events taken through the `_list` entry points since cc_create (ingest_raw again)
    DevBuf<int> list_desc;        // ... their descriptors {source column, mask} on the device, uploaded once per call (k_ingest_list)

    // cc_negq_begin .. cc_negq_end: the pooled selection of negative compensated values (cc_negq.h, cc_api_negq.inc); scratch
    // of its own, freed by cc_negq_end and with the handle, left alone by cc_reset
    struct NegQ {
        bool open = false;
        int d = 0, nw = 0;            // selected dimensions of every source / how many of them are wanted
        long long cap = 0, n = 0;     // events to come, pooled / events added so far
        std::vector<int> wmap;        // [d] the row of `val` a selected dimension has, -1: not wanted
        DevBuf<int> wdev;             // ... on the device
        DevBuf<double> val;           // [nw][cap] the values, dimension-major
        DevBuf<unsigned> hist;        // [nw][chunks][256] a pass's digit counts per chunk
        DevBuf<unsigned long long> st, nxt, out;  // [nw][CC_NEGQ_STATE] / [nw][chunks] successor candidates / [nw][4] the results
    } nq;

    // cc_points_prefetch: the next timepoint's points, uploaded by a worker thread through page-locked staging
    struct Prefetch {
        std::thread worker;
        bool active = false;            // a worker was started and has not been adopted / discarded yet
        IngestSrc src;                  // what it uploads, and how it is read (compared by the adopting upload)
        bool scaled = false;
        long long piece = 0;            // a staged source: points per piece, whole 64-point tiles that fit a page-locked buffer
        DevBuf<int> desc;               // event records: their descriptors on the device (k_ingest_list)
        DevBuf<float> raw[2];           // a staged source: the two pieces of device staging
        std::vector<double> scale, mn;
        DevBuf<double> X, Xt, sm;       // destination buffers (swapped with the handle's on adoption), scale / min
        DevBuf<int> bad;
        hipStream_t stream = nullptr;
        void* pin[2] = {nullptr, nullptr};
        size_t pin_bytes = 0;
        int bad_host[4] = {0, 0, 0, 0};  // k_check_finite's words: [0] non-finite flag, [2..3] bits of the largest |value|
        int rc = 0;                     // hipError_t of the worker (0: fine)
        const char* what = "";
    } pf;

    std::vector<hipEvent_t> ev_pool, sync_pool;

    // exact multi-GPU path: this handle is rank comm.rank of comm.world replicas of one stream
    cc::Comm comm;
    // a snapshot scan is split over the ranks when the table holds at least this many (row, dim) entries
    // (below that a window's scan is shorter than the all-gather that would follow it)
    long long shard_min_row_dims = 400000;
    long long shard_min_row_dims_pruned = 0;  // ... while the scans are pruned chains (0: the same; set by cc_comm_calibrate)
    double calib_ag_us = 0.0, calib_scan_ns = 0.0;  // what cc_comm_calibrate measured (group maxima)
    int offline_shard_min_rows = 8192;  // the pair matrices of the offline phase / association tracker likewise
    DevBuf<Cand> gsend, gpart;  // one merged record per window point (two parities) / the gathered records of all ranks
    DevBuf<Cand> gsend2, gpart2;  // guessed thresholds in a group: the missed points' new records, compact / gathered
    size_t gsend_stride = 0, gpart_stride = 0;
    DevBuf<int> g_i32;          // gather scratch of the offline phase
};

namespace {

// Run-time bools as compile-time ones: with_bools(f, a, b) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}), so a
// kernel's template flags are picked by one launch expression in a generic lambda instead of a ladder of ifs.
template <typename F>
void with_bools(F&& f)
{
    f();
}
template <typename F, typename... Rest>
void with_bools(F&& f, bool b, Rest... rest)
{
    if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// a device buffer the library refuses to size (ensure_table): CC_ERR_OOM with the reason
struct CapacityErr {
    std::string what;
};

int fail(cc_handle* h, int code, const std::string& msg)
{
    if (h) h->err = msg;
    return code;
}

// Every non-OK way out of a call made while the handle belongs to a group leaves the peers waiting for a rank that
// will not come: the group is given up (in-process peers are released, RCCL communicators aborted) and the peers
// get CC_ERR_COMM instead of hanging.
void group_lost(cc_handle* h)
{
    if (h && h->comm.active()) h->comm.fail_group();
}

template <typename F>
int guarded(cc_handle* h, F&& f)
{
    try {
        if (h) HIPCHK(hipSetDevice(h->device));
        const int rc = f();
        if (rc < 0) group_lost(h);
        return rc;
    } catch (const HipErr& e) {
        char buf[512];
        snprintf(buf, sizeof buf, "HIP error %d (%s) in %s", (int)e.e, hipGetErrorString(e.e), e.what);
        group_lost(h);
        return fail(h, e.e == hipErrorOutOfMemory ? CC_ERR_OOM : CC_ERR_NO_DEVICE, buf);
    } catch (const cc::CommErr& e) {
        group_lost(h);
        return fail(h, CC_ERR_COMM, "exchange between ranks failed: " + e.what);
    } catch (const std::bad_alloc&) {
        group_lost(h);
        return fail(h, CC_ERR_OOM, "host allocation failed");
    } catch (const CapacityErr& e) {
        group_lost(h);
        return fail(h, CC_ERR_OOM, e.what);
    }
}

// hipStreamSynchronize of a stream that may hold a collective of the handle's group: bounded (cc::Comm::wait_stream)
void sync_stream(cc_handle* h, hipStream_t st)
{
    if (h->comm.rccl() || h->comm.broken) h->comm.wait_stream(st);
    else HIPCHK(hipStreamSynchronize(st));
}

bool is_pow2(double k)
{
    if (!(k > 0.0) || !std::isfinite(k)) return false;
    int e;
    double m = std::frexp(k, &e);
    return m == 0.5 && e > -1000 && e < 1000;
}

void refresh_ctl_params(cc_handle* h)
{
    Ctl& c = h->hc;
    const cc_params& p = h->par;
    c.eps_sq = p.eps_sq;
    c.delta_sq = p.delta_sq;
    c.k = p.k;
    c.pow2 = (is_pow2(p.k) && !h->tainted) ? 1 : 0;
    c.inv_k = c.pow2 ? 1.0 / p.k : 0.0;
    c.beta_mu = p.beta * p.mu;  // hddstream.py:416, 529
    c.mu = p.mu;
    c.omicron = p.omicron;
    c.pi = p.pi;
    c.filter = (h->d > 0 && p.pi < h->d) ? 1 : 0;
    c.d = h->d;
}

// (Every push opens a fresh window chain - start of a call, back from the sequential kernel, a restart -: whatever scans
// left per window parity belongs to windows that will be scanned again, and the host's copy of it may be a half-summed one.)
// (The scan stamps go with it: the host has counted those of every window that ran before it writes the block, so no stamp
// outlives the batch - or the call - it was taken in.)
void clear_window_chain(Ctl& c)
{
    memset(c.pstat, 0, sizeof(c.pstat));
    c.n_missed_all[0] = c.n_missed_all[1] = 0;
    memset(c.scan_t0, 0, sizeof(c.scan_t0));
    memset(c.scan_t1, 0, sizeof(c.scan_t1));
}
void push_ctl(cc_handle* h)
{
    clear_window_chain(h->hc);
    HIPCHK(hipMemcpyAsync(h->ctl.p, &h->hc, sizeof(Ctl), hipMemcpyHostToDevice, h->stream));
}
void pull_ctl(cc_handle* h)
{
    HIPCHK(hipMemcpyAsync(&h->hc, h->ctl.p, sizeof(Ctl), hipMemcpyDeviceToHost, h->stream));
    sync_stream(h, h->stream);
}
// The same between the batches of a call, through page-locked staging blocks: a copy to or from pageable memory is driven
// by the host - it waits for the stream to drain and only then starts the copy (30 us of idle device before the copy
// kernel at every read-back, profiles/r06_tool_startup_gaps_before.txt) -, one from page-locked memory is a stream
// operation like any other.  pull: the block is read once the stream has drained.  push: only ever called right after a
// pull (the stream is idle, the previous push's copy has completed), so one block serves.
void pull_ctl_pinned(cc_handle* h)
{
    if (!h->hc_pin) { pull_ctl(h); return; }
    HIPCHK(hipMemcpyAsync(h->hc_pin, h->ctl.p, sizeof(Ctl), hipMemcpyDeviceToHost, h->stream));
    sync_stream(h, h->stream);
    memcpy(&h->hc, h->hc_pin, sizeof(Ctl));
}
void push_ctl_pinned(cc_handle* h)
{
    if (!h->hc_pin) { push_ctl(h); return; }
    clear_window_chain(h->hc);
    memcpy(h->hc_pin + 1, &h->hc, sizeof(Ctl));
    HIPCHK(hipMemcpyAsync(h->ctl.p, h->hc_pin + 1, sizeof(Ctl), hipMemcpyHostToDevice, h->stream));
}

// The kernels over the table index its elements with an int (row * d + dimension, up to a block of threads past the end):
// a capacity of more than CC_MAX_TABLE_ELEMS / d rows is refused rather than overflowed (2 M rows at d = 1 024).
#define CC_MAX_TABLE_ELEMS ((size_t)INT_MAX - 1023)

// grow the table to at least `rows` rows, keeping the first m_rows rows
void ensure_table(cc_handle* h, size_t rows)
{
    if (h->tab.cap >= rows && h->tab.d == h->d) return;
    const size_t max_rows = CC_MAX_TABLE_ELEMS / (size_t)std::max(h->d, 1);
    if (rows > max_rows)
        throw CapacityErr{"a table of " + std::to_string(rows) + " rows of " + std::to_string(h->d) + " dimensions: more than " +
                          std::to_string(max_rows) + " rows (" + std::to_string(CC_MAX_TABLE_ELEMS) + " elements) at this width"};
    // (a table of another width is a new table - set_dim admits the change only while no row is held -: sized by what is asked
    // for.  Twice the capacity of the old width, per change of width, took a handle that met a dozen widths out of memory.)
    const size_t doubled = h->tab.d == h->d ? h->tab.cap * 2 : 0;
    size_t want = std::min(max_rows, std::max<size_t>(rows, std::max<size_t>(1024, doubled)));
    TableStore nt;
    nt.alloc(want, h->d);
    const size_t m = (size_t)h->hc.m_rows;
    TableStore& old = h->tab;
    TableStore::for_each_column(h->d, [&](auto col, size_t per_row, TableStore::Grow grow) {
        auto& to = nt.*col;
        const size_t elem = sizeof(*to.p);
        if (grow == TableStore::CLEARED || grow == TableStore::CLEARED_KEPT)
            HIPCHK(hipMemsetAsync(to.p, 0, want * per_row * elem, h->stream));
        // (a table that holds rows has every column: alloc() is all or nothing)
        if ((grow == TableStore::KEPT || grow == TableStore::CLEARED_KEPT) && m > 0)
            HIPCHK(hipMemcpyAsync(to.p, (old.*col).p, m * per_row * elem, hipMemcpyDeviceToDevice, h->stream));
    });
    sync_stream(h, h->stream);
    std::swap(h->tab, nt);
}

int set_dim(cc_handle* h, int d)
{
    if (d <= 0 || d > CC_MAX_DIM) return fail(h, CC_ERR_BAD_ARG, "d must be in 1.." + std::to_string(CC_MAX_DIM));
    if (h->d == 0) h->d = d;
    if (h->d != d) {
        if (h->hc.m_rows == 0) h->d = d;
        else return fail(h, CC_ERR_BAD_ARG, "dimensionality differs from the microclusters already held");
    }
    return CC_OK;
}

// (Known limitation: sized by the largest window times the largest width the handle has seen, also for the 64 points the wide
// path asks for - DESIGN.md section 3.)
void ensure_window_buffers(cc_handle* h, int win, int seg)
{
    if (win <= h->win_alloc && seg <= h->seg_alloc && h->d <= h->d_alloc) return;
    win = std::max(win, h->win_alloc);
    seg = std::max(seg, h->seg_alloc);
    const size_t w = (size_t)win, d = (size_t)std::max(h->d, h->d_alloc);
    h->v_cf1.ensure(w * d); h->v_cf2.ensure(w * d); h->v_cen.ensure(w * d); h->v_pref.ensure(w * d); h->v_scl.ensure(w * d); h->v_w.ensure(w);
    h->v_kind.ensure(w); h->v_key.ensure(w); h->v_next.ensure(w); h->v_upg.ensure(w); h->v_acc.ensure(w);
    h->v_dsq.ensure(w); h->v_tau.ensure(CC_TAU_STRIDE * w); h->v_tile_dsq.ensure(CC_DSQ_STRIDE * (w / 16 + 2));
    h->v_tgt.ensure(w);
    h->v_skip.ensure(w / 64 + 2); h->v_skip_car.ensure(w / 64 + 2); h->v_unsafe.ensure(w);
    h->part_stride = w * seg * 4;
    h->spart_stride = w * seg * 2;
    h->thr_stride = w * 2;
    h->spart.ensure(2 * h->spart_stride);
    h->thr.ensure(2 * h->thr_stride);
    h->thr32.ensure(2 * h->thr_stride);
    h->cmax.ensure(2);
    h->found.ensure(2 * (CC_MAX_WINDOW / 64));
    h->missed.ensure(2 * CC_MISSED_CAP);
    h->part.ensure(2 * h->part_stride); h->dpart.ensure(w * seg * 2); h->dpart2.ensure(w * seg * 2);
    h->clean.ensure(w * 4); h->dseed.ensure(w * 4);
    h->c_cf1v.ensure(w * d); h->c_cf2v.ensure(w * d); h->c_cenv.ensure(w * d); h->c_prefv.ensure(w * d);
    h->c_sclv.ensure(w * d); h->c_wv.ensure(w); h->c_c0.ensure(w * d); h->c_w0.ensure(w * d);
    h->c_kind.ensure(w); h->c_key.ensure(w); h->c_slot.ensure(w); h->c_kind0.ensure(w); h->c_dsq.ensure(w); h->c_tile_dsq.ensure(CC_DSQ_STRIDE * (w / 16 + 2));
    h->T0.ensure(w + 128); h->T1.ensure(w + 128);  // k_chain reads the claims in 128-entry blocks
    h->long_list.ensure(2 * CC_LONG_CAP);
    h->lstat.ensure(2 * CC_LSTAT_ROWS + 2);
    h->lprev.ensure(CC_MAX_WINDOW);
    h->dpath.ensure(w); h->rk.ensure(w); h->rec.ensure(1); h->sp_list.ensure(w); h->link_near.ensure(w);
    h->win_alloc = win; h->seg_alloc = seg; h->d_alloc = (int)d;
}

Carry carry_view(cc_handle* h)
{
    return Carry{h->c_cf1v.p, h->c_cf2v.p, h->c_cenv.p, h->c_prefv.p, h->c_sclv.p, h->c_wv.p, h->c_kind.p, h->c_key.p,
                 h->c_slot.p, h->c_c0.p, h->c_w0.p, h->c_kind0.p, h->c_dsq.p, h->c_tile_dsq.p};
}

// bring both scan copies in line with the table (rows [0, m_rows)); enqueued on the main stream
void scan_copy_sync(cc_handle* h, ScanCopy (&out)[2])
{
    const size_t cap = h->tab.cap, d = (size_t)h->d, m = (size_t)h->hc.m_rows;
    const bool filter = h->hc.filter != 0;
    const TableStore& t = h->tab;
    for (int q = 0; q < 2; ++q) {
        h->sh_cen[q].ensure(cap * d); h->sh_scl[q].ensure(cap * d); h->sh_kind[q].ensure(cap); h->sh_key[q].ensure(cap);
        if (filter) { h->sh_cf1[q].ensure(cap * d); h->sh_cf2[q].ensure(cap * d); h->sh_w[q].ensure(cap); }
        if (m > 0) {
            HIPCHK(hipMemcpyAsync(h->sh_cen[q].p, t.cen.p, m * d * 8, hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(h->sh_scl[q].p, t.scl.p, m * d * 8, hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(h->sh_kind[q].p, t.kind.p, m * 4, hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(h->sh_key[q].p, t.key.p, m * 4, hipMemcpyDeviceToDevice, h->stream));
            if (filter) {
                HIPCHK(hipMemcpyAsync(h->sh_cf1[q].p, t.cf1.p, m * d * 8, hipMemcpyDeviceToDevice, h->stream));
                HIPCHK(hipMemcpyAsync(h->sh_cf2[q].p, t.cf2.p, m * d * 8, hipMemcpyDeviceToDevice, h->stream));
                HIPCHK(hipMemcpyAsync(h->sh_w[q].p, t.w.p, m * 8, hipMemcpyDeviceToDevice, h->stream));
            }
        }
        out[q] = ScanCopy{h->sh_cen[q].p, h->sh_scl[q].p, h->sh_cf1[q].p, h->sh_cf2[q].p, h->sh_w[q].p, h->sh_kind[q].p,
                          h->sh_key[q].p};
    }
}

Versions versions_view(cc_handle* h)
{
    return Versions{h->v_cf1.p, h->v_cf2.p, h->v_cen.p, h->v_pref.p, h->v_scl.p, h->v_w.p, h->v_kind.p,
                    h->v_key.p, h->v_next.p, h->v_upg.p, h->v_acc.p, h->v_tgt.p, h->v_dsq.p, h->v_tile_dsq.p,
                    h->v_tau.p, h->v_skip.p, h->v_skip_car.p, h->v_unsafe.p};
}

// the table rows as half-precision operands of the MFMA prefix test (k_prefix16): two window parities, whole tiles of 32 rows
// (grown between batches only: a scan in flight on the other stream may be reading it)
void ensure_prefix16(cc_handle* h)
{
    const size_t a16_rows = h->tab.cap + 2 * CC_P16_TM;
    if (h->a16_stride >= a16_rows * 4) return;
    sync_stream(h, h->stream);
    sync_stream(h, h->stream2);
    h->a16.ensure(2 * a16_rows * 4);
    h->a16_stride = a16_rows * 4;
    h->hdr16.ensure(2);
}

// the scanned rows' centroids and operands at the padded stride (k_pad_rows; d off the ladder): two window parities - an
// in-place scan on the first stream and a lookahead scan on the second can be in flight together.  The scan kernels read
// rows below the scanned row count only (k_scan_u's request for the next row stays inside its tile, cc_load_prefix and the
// row walks of the pruned kernels are bounded by their sub-range, k_prefix16's extra rows are rows of its own buffer, not
// of this one); a tile of rows of slack all the same.  (grown between batches only, like ensure_prefix16)
void ensure_pad_rows(cc_handle* h, int dp)
{
    const size_t stride = (h->tab.cap + CC_SCAN_TM) * (size_t)dp;
    if (h->pad_stride >= stride) return;
    sync_stream(h, h->stream);
    sync_stream(h, h->stream2);
    h->pad_cen.ensure(2 * stride);
    h->pad_scl.ensure(2 * stride);
    h->pad_stride = stride;
}

hipEvent_t get_event(cc_handle* h, size_t i)
{
    while (h->ev_pool.size() <= i) {
        hipEvent_t e;
        // (timestamps are all the host reads from these: no system-scope release when one is recorded)
        HIPCHK(hipEventCreateWithFlags(&e, h->light_sync_events ? hipEventReleaseToDevice : hipEventDefault));
        h->ev_pool.push_back(e);
    }
    return h->ev_pool[i];
}

// events that only order the two streams (never read back): no timestamp, device-scope release
hipEvent_t get_sync_event(cc_handle* h, size_t i)
{
    if (!h->light_sync_events) return get_event(h, i);
    while (h->sync_pool.size() <= i) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventReleaseToDevice));
        h->sync_pool.push_back(e);
    }
    return h->sync_pool[i];
}


}  // namespace
