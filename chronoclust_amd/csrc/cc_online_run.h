// cc_online_run.h — one call of the exact windowed online phase: OnlineRun (prepare, stints of the sequential kernel, batches
// of windows enqueued and read back, finish), the trace of the window policy's decisions, and online_range(), its only
// user.  Needs cc_handle.h, cc_policy.h, cc_batch.h and the scan dispatcher of cc_api.hip (launch_scan, scan_plan).
// (included by cc_api.hip, the one translation unit)
#pragma once

namespace {

// CHRONOCLUST_HIP_POLICY_TRACE=<file>: the observations and decisions of the window policy, one JSON object per line
struct PolicyTrace {
    FILE* f = nullptr;
    static void obs_json(FILE* f, const cc_policy_obs& o)
    {
        fprintf(f, "{\"cursor\": %lld, \"m_rows\": %d, \"stall_b\": %d, \"stat_windows\": %lld, \"stat_truncated\": %lld, "
                   "\"stat_trunc_unknown\": %lld, \"stat_tiles\": %lld, \"stat_dirty_tiles\": %lld, \"stat_unsafe\": %lld, \"stat_missed\": %lld, \"tg_ok\": %d, \"round_hist\": [",
                (long long)o.cursor, o.m_rows, o.stall_b, (long long)o.stat_windows, (long long)o.stat_truncated,
                (long long)o.stat_trunc_unknown, (long long)o.stat_tiles, (long long)o.stat_dirty_tiles, (long long)o.stat_unsafe,
                (long long)o.stat_missed, o.tg_ok);
        for (int r = 0; r < CC_POLICY_MAX_ROUNDS + 2; ++r) fprintf(f, "%s%lld", r ? ", " : "", (long long)o.round_hist[r]);
        fprintf(f, "], \"prune_rows\": %llu, \"prune_full\": %llu, \"after_sequential\": %d}", (unsigned long long)o.prune_rows,
                (unsigned long long)o.prune_full, o.after_sequential);
    }
    static void dec_json(FILE* f, const cc_policy_decision& d)
    {
        fprintf(f, "{\"win_cfg\": %d, \"want\": %d, \"rounds\": %d, \"batch_windows\": %d, \"lookahead\": %d, \"nodirty\": %d, "
                   "\"prune\": %d, \"shard\": %d, \"restart\": %d, \"bad\": %d, \"stalled\": %d, \"sparse\": %d, \"probe\": %d}",
                d.win_cfg, d.want, d.rounds, d.batch_windows, d.lookahead, d.nodirty, d.prune, d.shard, d.restart, d.bad, d.stalled, d.sparse, d.probe);
    }
    // rank >= 0: the handle is rank `rank` of a group and writes <file>.rank<rank>
    PolicyTrace(const cc_policy_config& c, const cc_policy_carry& k, long long cursor, int rows, const cc_policy_decision& d0,
                int rank)
    {
        const char* path = getenv("CHRONOCLUST_HIP_POLICY_TRACE");
        if (!path || !path[0]) return;
        const std::string name = rank >= 0 ? std::string(path) + ".rank" + std::to_string(rank) : std::string(path);
        f = fopen(name.c_str(), "a");
        if (!f) return;
        fprintf(f, "{\"call\": {\"config\": {\"window\": %d, \"rounds_max\": %d, \"windows_per_sync\": %d, \"early_window\": %d, "
                   "\"lookahead\": %d, \"allow_nodirty\": %d, \"prune_mode\": %d, \"prune_applicable\": %d, \"can_shard\": %d, \"d\": %d, "
                   "\"resume\": %d, \"allow_sparse\": %d, \"allow_guess\": %d, \"allow_probe\": %d, \"shard_min_row_dims\": %lld, \"n_end\": %lld, \"shard_min_row_dims_pruned\": %lld, \"lookahead_pruned\": %d, \"force_prune_rows\": %d}, \"carry\": [%d, %d, %d], \"start\": [%lld, %d], \"dec\": ",
                c.window, c.rounds_max, c.windows_per_sync, c.early_window, c.lookahead, c.allow_nodirty, c.prune_mode,
                c.prune_applicable, c.can_shard, c.d, c.resume, c.allow_sparse, c.allow_guess, c.allow_probe, (long long)c.shard_min_row_dims, (long long)c.n_end, (long long)c.shard_min_row_dims_pruned, c.lookahead_pruned, c.force_prune_rows,
                k.adapt_win, k.clean_batches, k.since_shrink, cursor, rows);
        dec_json(f, d0);
        fprintf(f, "}}\n");
    }
    void batch(const cc_policy_obs& o, const cc_policy_decision& d)
    {
        if (!f) return;
        fprintf(f, "{\"obs\": ");
        obs_json(f, o);
        fprintf(f, ", \"dec\": ");
        dec_json(f, d);
        fprintf(f, "}\n");
    }
    void sequential(long long cursor, int rows, const cc_policy_decision& d)
    {
        cc_policy_obs o{};
        o.cursor = cursor;
        o.m_rows = rows;
        o.after_sequential = 1;
        batch(o, d);
    }
    ~PolicyTrace()
    {
        if (f) fclose(f);
    }
    PolicyTrace(const PolicyTrace&) = delete;
    PolicyTrace& operator=(const PolicyTrace&) = delete;
};

// k_link_scan over the padded dimensionality (the scans' ladder)
void launch_link_scan(cc_handle* h, hipStream_t st, int win)
{
    const dim3 grid((win + 63) / 64, (win + 4 * CC_LINK_SUB - 1) / (4 * CC_LINK_SUB)), block(256);
    const int d = h->d;
#define CC_LINK_DP(DP) hipLaunchKernelGGL((k_link_scan<DP>), grid, block, 0, st, (const Ctl*)h->ctl.p, (const double*)h->X.p, \
                                          (const double*)h->Xt.p, (const int*)h->T0.p, h->link_near.p)
    if (d <= 4) CC_LINK_DP(4);
    else if (d <= 8) CC_LINK_DP(8);
    else if (d <= 14) CC_LINK_DP(14);
    else if (d <= 16) CC_LINK_DP(16);
    else if (d <= 20) CC_LINK_DP(20);
    else if (d <= 32) CC_LINK_DP(32);
    else if (d <= 40) CC_LINK_DP(40);
    else CC_LINK_DP(64);
#undef CC_LINK_DP
}

static_assert(cc::kMaxWindow == CC_MAX_WINDOW && cc::kLongCap == CC_LONG_CAP, "cc_batch.h repeats two constants of cc_common.h");

// The views the scans walk (Rows, cc_common.h), field by field on a zeroed struct: what a view does not have stays null
Rows rows_of_table(const Table& t)
{
    Rows r{};
    r.cen = t.cen; r.scl = t.scl; r.pref = t.pref; r.cf1 = t.cf1; r.cf2 = t.cf2; r.w = t.w; r.kind = t.kind; r.key = t.key;
    return r;
}
Rows rows_of_versions(const Versions& v)
{
    Rows r{};
    r.cen = v.cen; r.scl = v.scl; r.pref = v.pref; r.cf1 = v.cf1; r.cf2 = v.cf2; r.w = v.w; r.kind = v.kind; r.key = v.key;
    r.next = v.next; r.tile_dsq = v.tile_dsq; r.dsq = v.dsq; r.tau = v.tau; r.skip = v.skip;
    return r;
}
Rows rows_of_carry(const Carry& c, const Versions& v, const Table& t)
{
    Rows r{};
    r.cen = c.cen; r.scl = c.scl; r.pref = c.pref; r.cf1 = c.cf1; r.cf2 = c.cf2; r.w = c.w; r.kind = c.kind; r.key = c.key;
    r.tile_dsq = c.tile_dsq; r.dsq = c.dsq; r.tau = v.tau; r.skip = v.skip_car;
    r.slot = c.slot; r.touch = t.touch; r.cap = t.cap;
    return r;
}
// (lookahead scans read a scan copy of the table, see ScanCopy)
Rows rows_of_scan_copy(const ScanCopy& s)
{
    Rows r{};
    r.cen = s.cen; r.scl = s.scl; r.cf1 = s.cf1; r.cf2 = s.cf2; r.w = s.w; r.kind = s.kind; r.key = s.key;
    return r;
}
// the sparse dirty scans: the same rows for the round's list of points instead of the window's tiles
Rows sparse_rows(Rows r, const int* plist)
{
    r.skip = nullptr;
    r.plist = plist;
    return r;
}

// the counters of a call in the host mirror of the control block, before its first batch
void reset_call_counters(Ctl& c)
{
    c.last_round = 0;
    c.fc[0] = 0;
    for (int i = 1; i < CC_MAX_ROUNDS + 2; ++i) c.fc[i] = CC_IDX_INF;
    c.stat_windows = c.stat_rounds = c.stat_truncated = 0;
    c.stat_lookahead = 0;
    c.stat_tiles = c.stat_dirty_tiles = 0;
    c.stat_unprovable = c.stat_unsafe = 0;
    c.stat_long = 0;
    for (int i = 0; i < CC_MAX_ROUNDS + 2; ++i) c.n_long[i] = 0;
    c.stat_trunc_unknown = 0;
    c.stat_table_rows = 0;
    c.stat_seq_points = 0;
    c.stat_seq_r_points = 0;
#ifdef CC_LONG_TIMERS
    for (int i = 0; i < 8; ++i) c.dbg_long[i] = 0;
#endif
#ifdef CC_ROUND_DEBUG
    for (int i = 0; i < CC_MAX_ROUNDS + 2; ++i)
        for (int q = 0; q < 6; ++q) c.dbg_round[i][q] = 0;
#endif
    c.n_heavy = c.n_heavy_new = 0;  // (rows are renumbered between calls: the marks of the last call are void)
    c.stat_seq_clk = c.stat_seq_wall = 0;
    c.stat_prune_rows = c.stat_prune_full = 0;
    c.stat_missed = 0;
    c.seed_at = -1;
    for (int q = 0; q < 2; ++q) {
        c.n_missed[q] = 0;
        for (int K = 0; K < 2; ++K) { c.tg[q][K] = 0.0; c.tg_ok[q][K] = 0; }
    }
    c.cen_absmax = 0ull;            // (k_rebuild_scl takes the table's maximum into it)
    c.stat_pair_rows = 0.0;
    for (int i = 0; i < CC_MAX_ROUNDS + 2; ++i) c.round_hist[i] = 0;
}

// One call of the exact windowed online phase over the resident points [range_a, range_e): the state that lives across its
// batches of windows, and what happens to it - prepare(), then per iteration either a stint of the sequential kernel or a
// batch of windows enqueued (enqueue_batch) and read back (after_batch: the policy's decision for the next one) -, finish().
// How a batch runs is decided in four places, none of them here: ScanPlan (cc_api.hip), cc::BatchPlan (cc_batch.h),
// cc::WindowPolicy and cc::SeqHandover (cc_policy.h); this struct measures, carries the decisions out and launches.
// online_range() below is its only user.
struct OnlineRun {
    cc_handle* const h;
    const long long range_a, N;
    const bool no_create, resume;
    Ctl& c;  // the host mirror of the control block (h->hc)

    // ---- constants of the call ----
    int win = 0, R = 0;
    int S_cfg = 1, Sd_full = 1, Sd = 1;  // partials per point: clean scans (refined per batch) / dirty scans
    int world = 1, myrank = 0;
    bool grouped = false;
    size_t batch_max = 2;
    bool timing = false;
    int seq_cap = 0;
    Versions ver{};
    Carry car{};
    hipStream_t sA = nullptr, sB = nullptr;
    static constexpr size_t ev_base = 4;

    // ---- the window policy and its current decision ----
    std::optional<cc::WindowPolicy> policy;
    std::optional<PolicyTrace> ptrace;
    cc_policy_decision dec{};
    // While k_dseed rules the dirty scans out for every tile they are not launched at all (beside a lookahead scan
    // even a launch whose workgroups all return at once waits for registers until the scan has dispatched its last
    // workgroup); k_decide then refuses points that would have needed them, the device idles the rest of the batch
    // if that stops a window at its first point, and the next batch launches them again.
    bool nodirty = false;
    bool sparse_now = false;  // with nodirty: sparse dirty scans for the round's list of points
    bool la_on = false;       // lookahead scans are being enqueued
    bool shard_on = false;    // snapshot scans are split over the ranks of the group
    bool link_now = false;    // round 0 of this batch's windows links the points that decide "create" (cc_link.h)
    int Rcur = 1;             // validation rounds enqueued per window of the batch
    int batch_windows = 2;

    // ---- progress ----
    long long done = 0;       // the device's cursor as last read back
    int m_known = 0;          // table rows as last read back
    unsigned long long seq_host = 0;  // sequence number of the window the next iteration validates
    long long cursor_prev = 0;
    double batch_t0 = 0.0;

    // ---- events, timing, statistics ----
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evCommit = nullptr, evScan = nullptr;
    size_t ev_used = 2, ev_sync = ev_base;
    std::vector<std::pair<size_t, double>> timed;  // (event index, 1.0 for a pruned chain)
    std::vector<size_t> timed_comm;                // event index of every timed merge + all-gather
    // In-place scans (one stream, not split, no lookahead) are timed without events: two stamps of the device's constant
    // clock per window, taken inside kernels that run anyway (Ctl::scan_t0 / scan_t1) and read with the control block after
    // the batch.  An event record costs the stream ~6 us of idle device at each of the two places, a stamp nothing.
    bool stamps = false;                                      // this call's control block has stamp_on set
    std::vector<std::pair<unsigned long long, int>> stamped;  // the batch's windows timed that way: (sequence number, 1 for a pruned chain)
    int64_t stamped_n = 0, stamped_n_p = 0;                   // launches so timed in this call / of those, pruned chains
    double stamped_ms = 0.0, stamped_ms_p = 0.0;              // their intervals, of the windows that ran
    double pair_rows_eff = 0.0, pair_rows_prev = 0.0;  // (window points x table rows) this rank's scans covered
    double pair_rows_pruned = 0.0;                     // ... of those, by pruned chains
    long long sharded_windows = 0;

    cc::SeqHandover seq;    // the sequential kernel's wall-clock rule (off inside a group)
    cc::LongChains longs;   // long chains as the previous batch saw them (k_chain_long over the list k_decide keeps)
    long long long_launches = 0;

    // ---- the batch being enqueued: its plan and the views its launches read ----
    cc::BatchPlan bp{};
    Table tab{};
    Rows trows{}, vrows{}, crows{}, vrows_sp{}, crows_sp{}, srows[2] = {};
    ScanCopy scopy[2] = {};
    int* long_list = nullptr;       // the list k_decide keeps for the listed long chains and k_claims_heavy
    int probe_left = 0;             // scans of the batch that still carry the pruned chain's probe
    hipEvent_t scan_end = nullptr;  // the event recorded right behind the last timed scan (nothing after it yet)

    OnlineRun(cc_handle* handle, long long a, long long e, bool no_create_, bool resume_)
        : h(handle), range_a(a), N(e), no_create(no_create_), resume(resume_), c(handle->hc) {}

    static double now_ms()
    {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    // points per ms the sequential kernel is assumed to manage before it has been measured in this call (k_seq on its LDS
    // image: ~0.9 us per point; k_seq_r, rows in registers, d <= 4: ~0.6 us)
    bool seq_r_applies() const { return h->allow_seq_r && h->d >= 2 && h->d <= 4; }
    // (k_seq_g, beyond the LDS image: 3-5 us per point at a few hundred rows)
    // d > CC_WINDOW_MAX_DIM: the windowed path (two dimensions per lane of a 32-lane group, 2 d registers per point in the scans)
    // does not take such points; k_seq_g does, from the first one on
    bool wide() const { return h->d > CC_WINDOW_MAX_DIM; }
    // table rows a batch of windows may create (none beyond CC_WINDOW_MAX_DIM: k_seq_g's chunks are reserved in run())
    size_t window_rows() const { return wide() ? 0 : (size_t)win * batch_max; }
    bool seq_g_applies() const { return h->allow_seq_g && h->hc.m_rows >= seq_cap; }
    double seq_rate_guess() const { return cc::seq_rate_guess(h->d, h->hc.m_rows, seq_cap, h->allow_seq_r, h->allow_seq_g); }
    // (`possible` of cc::SeqHandover: never in a group, never with no_create, while the table fits k_seq's image or k_seq_g may run)
    bool seq_possible() const { return !h->comm.active() && !no_create && (h->hc.m_rows < seq_cap || h->allow_seq_g); }

    // lookahead (re)start: the current window is a fresh one (scanned in place), the lookahead scan enqueued next covers
    // the one after it
    void set_lookahead(bool on)
    {
        la_on = on;
        c.la_on = on ? 1 : 0;
        c.stall_b = 0;
        c.mode = 0;
        c.car_n = 0;
        const int q = (int)((c.window_seq + 1ull) & 1ull);
        const long long c1 = c.cursor + c.win_b;
        const long long left1 = c.n_points - c1;
        c.la_cursor[q] = c1;
        c.la_b[q] = (on && left1 > 0) ? (int)std::min<long long>(left1, c.win_cfg) : 0;
        c.la_rows[q] = c.m_rows;
        c.la_cursor[q ^ 1] = 0;
        c.la_b[q ^ 1] = 0;
        c.la_rows[q ^ 1] = 0;
    }

    // How the batches of windows run - window size, validation rounds, windows per batch, lookahead, dirty scans,
    // pruned or plain scans, split over the ranks - is decided by cc::WindowPolicy (cc_policy.h) from the device
    // counters alone; OnlineRun carries the decisions out.  The constants of the call it decides on:
    cc_policy_config policy_config() const
    {
        const ScanPlan& plan = h->scan_plan;
        cc_policy_config p{};
        p.window = win; p.rounds_max = R; p.n_end = N; p.d = h->d; p.resume = resume ? 1 : 0;
        p.windows_per_sync = h->tun.windows_per_sync; p.early_window = h->tun.early_window; p.lookahead = h->tun.lookahead;
        p.allow_nodirty = h->allow_nodirty ? 1 : 0; p.allow_sparse = h->allow_sparse; p.lookahead_pruned = h->la_pruned ? 1 : 0;
        p.prune_mode = h->prune_mode; p.prune_applicable = plan.prune_applicable; p.force_prune_rows = plan.force_prune_rows;
        p.allow_guess = plan.allow_guess; p.allow_probe = plan.allow_probe;
        p.can_shard = (grouped && !h->shard_suspended) ? 1 : 0;
        p.shard_min_row_dims = h->shard_min_row_dims; p.shard_min_row_dims_pruned = h->shard_min_row_dims_pruned;
        return p;
    }

    // buffers, control block, policy: everything before the first batch
    void prepare()
    {
        refresh_ctl_params(h);
        // how this call's snapshot scans run (the pdim filter and k are fixed for the call)
        h->scan_plan = scan_plan(h);
        const ScanPlan& plan = h->scan_plan;
        win = h->tun.window; R = h->tun.rounds;
        // `segments` MC sub-ranges per point tile = S workgroups of `waves` waves -> S partials per point
        S_cfg = std::max(1, h->tun.segments / plan.waves);
        Sd_full = std::max(1, (h->tun.dirty_segments > 0 ? h->tun.dirty_segments : h->tun.segments) / plan.dirty_waves);
        // while the dirty scans are ruled out tile by tile (k_dseed) their launches only have to be scheduled: a
        // few workgroups per point tile then, the full split while they really run (set per batch below)
        Sd = Sd_full;
        nodirty = false;
        // (beyond CC_WINDOW_MAX_DIM no window runs: the window buffers, w d doubles each, are kept at their smallest)
        ensure_window_buffers(h, wide() ? 64 : win, std::max(S_cfg, Sd_full));
        // Exact multi-GPU path: while the table is large enough, every rank scans its share of the table rows and
        // the ranks all-gather one merged candidate record per window point; the rest of the window runs replicated.
        // All ranks take the same decision: it depends on the row count only, which is the same everywhere.
        world = h->comm.world; myrank = h->comm.rank;
        // (a communicator of one rank takes the same path: that is how the RCCL calls are exercised on one GPU)
        grouped = h->comm.active();
        if (grouped) {
            // (+ 4: the record behind the last point's carries the rank's pruned-scan sample, see k_merge_partials)
            // (grids cover at least 64 points, see BatchPlan::gw: the blocks are sized for that even when the window is smaller)
            const size_t gmax = (size_t)std::max(64, h->win_alloc);
            h->gsend_stride = gmax * 4 + 4;
            h->gpart_stride = (size_t)world * (gmax * 4 + 4);
            h->gsend.ensure(2 * h->gsend_stride);
            h->gpart.ensure(2 * h->gpart_stride);
            h->gsend2.ensure((size_t)2 * CC_MISSED_CAP * 4);  // (per window parity, like the lists they serve)
            h->gpart2.ensure((size_t)2 * world * CC_MISSED_CAP * 4);
        }
        // every window of a batch may create one MC per point: rows for the largest batch that can be enqueued
        batch_max = (size_t)std::max(2, h->tun.windows_per_sync);
        ensure_table(h, (size_t)h->hc.m_rows + window_rows() + 1);

        c.cursor = range_a;
        c.n_points = N;
        c.xt_stride = h->n_points;
        c.no_create = no_create ? 1 : 0;
        const cc_policy_config pcfg = policy_config();
        const cc_policy_carry pcarry{h->adapt_win, h->clean_batches, h->since_shrink, 0};
        policy.emplace(pcfg, pcarry);
        dec = policy->start(range_a, c.m_rows);
        ptrace.emplace(pcfg, pcarry, range_a, c.m_rows, dec, grouped ? myrank : -1);
        c.win_cfg = dec.win_cfg;
        c.win_b = (int)std::min<long long>(c.win_cfg, N - range_a);
        c.max_rounds = R;
        reset_call_counters(c);
        HIPCHK(hipMemsetAsync(h->tab.heavy.p, 0, h->tab.cap * sizeof(int), h->stream));  // (the marks behind Ctl::n_heavy)
        c.x_absmax = h->x_absmax;
        set_lookahead(dec.lookahead != 0);
        timing = h->tun.time_kernels != 0;
        // (a batch must fit the ring of stamp slots, and the clock's rate must be known: else the events time every scan)
        stamps = timing && h->wall_khz > 0 && batch_max < (size_t)CC_STAMP_SLOTS;
        c.stamp_on = stamps ? 1 : 0;
        push_ctl(h);

        // no carry set yet: the commit record of an earlier call describes rows that may have moved since
        HIPCHK(hipMemsetAsync(h->rec.p, 0, sizeof(CommitRec), h->stream));
        HIPCHK(hipMemsetAsync(h->cmax.p, 0, 2 * sizeof(unsigned long long), h->stream));  // (k_seed takes maxima into it)
        HIPCHK(hipMemsetAsync(h->found.p, 0, h->found.n * sizeof(unsigned long long), h->stream));
        // (marks of long chains laid out in an earlier call - another table, perhaps another numbering of the windows)
        HIPCHK(hipMemsetAsync(h->lstat.p, 0, h->lstat.n * sizeof(unsigned long long), h->stream));
        HIPCHK(hipMemsetAsync(h->lprev.p, 0, h->lprev.n * sizeof(unsigned long long), h->stream));
        if (c.m_rows > 0)
            hipLaunchKernelGGL(k_rebuild_scl, dim3((c.m_rows * h->d + 255) / 256), dim3(256), 0, h->stream, h->ctl.p, h->tab.view(),
                               c.m_rows, h->d, c.pow2, c.inv_k);
        ev0 = get_event(h, 0); ev1 = get_event(h, 1);
        HIPCHK(hipEventRecord(ev0, h->stream));
        ev_used = 2;
        shard_on = dec.shard != 0;

        ver = versions_view(h);
        car = carry_view(h);
        sA = h->stream; sB = h->stream2;
        // cross-stream hand-offs: a fresh event per hand-off (the pool is reused from batch to batch)
        evCommit = get_event(h, 2); evScan = nullptr;
        ev_sync = ev_base;
        ev_used = ev_base + 3 * (batch_max + 2);

        done = range_a;
        m_known = c.m_rows;
        // the sequential kernel (cc::SeqHandover): forced beyond CC_WINDOW_MAX_DIM, else as the caller's tuning says
        seq_cap = wide() ? 0 : cc_seq_cap_rows(h->d);
        seq.start(wide() ? 2 : h->tun.sequential, seq_possible(), h->seq_sticky);
        Rcur = dec.rounds;
        batch_windows = dec.batch_windows;
        h->set_prune(dec.prune);
        nodirty = dec.nodirty != 0;
        sparse_now = dec.sparse != 0;
        cursor_prev = range_a;
        seq_host = c.window_seq;
        // (a call starts with whatever is new since the last one: the first batch links, the later ones while the table grows)
        link_now = h->allow_link && !no_create && !wide();
    }

    // a stint of the sequential kernel (k_seq): one chunk of points, then back to the windows if the table outgrew its LDS
    // image or the stint is over
    void sequential_stint()
    {
        const int chunk = 8192;
        const double t0 = now_ms();
        const bool use_g = seq_g_applies();
        const bool f = h->hc.filter != 0, p2 = h->hc.pow2 != 0;
        if (use_g) {
            // the table has outgrown the LDS image: the same loop on the table where it lies, one workgroup
            const int list_cap = (int)std::min<size_t>(h->tab.cap, (size_t)INT_MAX / 2);
            h->seq_lists.ensure(2 * (size_t)list_cap);
            h->seq_img.ensure(4 * (size_t)list_cap * (size_t)h->d);
            // (W, the wide form: a point's dimensions in blocks of 64)
            with_bools([&](auto F, auto P, auto W) {
                hipLaunchKernelGGL((k_seq_g<decltype(F)::value, decltype(P)::value, decltype(W)::value>), dim3(1), dim3(CC_SEQG_THREADS), 0, sA, h->ctl.p, h->X.p, tab,
                                   h->lab_uid.p, h->lab_path.p, chunk, h->seq_lists.p, list_cap, h->seq_img.p);
            }, f, p2, h->d > CC_SEQG_NARROW_DIM);
        } else {
            // d <= 4: the register-resident kernel first; what it cannot hold (Ctl::seq_rest) is left to the LDS kernel
            int follow = 0;
            auto seq_r = [&](auto D) {
                with_bools([&](auto P) {
                    hipLaunchKernelGGL((k_seq_r<decltype(D)::value, decltype(P)::value>), dim3(1), dim3(64), 0, sA, h->ctl.p, h->X.p, tab, h->lab_uid.p,
                                       h->lab_path.p, chunk);
                }, p2);
                follow = 1;
            };
            if (h->allow_seq_r) {
                if (h->d == 2) seq_r(std::integral_constant<int, 2>{});
                else if (h->d == 3) seq_r(std::integral_constant<int, 3>{});
                else if (h->d == 4) seq_r(std::integral_constant<int, 4>{});
            }
            with_bools([&](auto F, auto P) {
                hipLaunchKernelGGL((k_seq<decltype(F)::value, decltype(P)::value>), dim3(1), dim3(64), 0, sA, h->ctl.p, h->X.p, tab, h->lab_uid.p,
                                   h->lab_path.p, chunk, follow);
            }, f, p2);
        }
        HIPCHK(hipGetLastError());
        pull_ctl(h);
        const double dt = now_ms() - t0;
        const long long got = h->hc.cursor - done;
        done = h->hc.cursor;
        m_known = h->hc.m_rows;
        seq_host = h->hc.window_seq;
        cursor_prev = h->hc.cursor;
        const double seq_rate = got > 0 ? (double)got / std::max(dt, 1e-3) : 0.0;
        if (h->trace)
            fprintf(stderr, "[cc] done %lld rows %d | sequential kernel: %lld points in %.3f ms (so far %lld shader cycles, %.3f ms of kernel time)\n",
                    done, h->hc.m_rows, got, dt, (long long)h->hc.stat_seq_clk, (double)h->hc.stat_seq_wall / 1e5);
        if (use_g) h->stats.seq_g_points += got;
        if (seq.after_chunk(got, seq_rate, chunk, use_g, h->allow_seq_g, seq_possible(), done < N, wide()) != cc::SeqHandover::kContinue) {
            // back to the windows: a fresh window at the cursor, no carry set, no pending lookahead scan
            HIPCHK(hipMemsetAsync(h->rec.p, 0, sizeof(CommitRec), h->stream));
            h->hc.win_b = (int)std::min<long long>(h->hc.win_cfg, N - done);
            dec = policy->after_sequential(h->hc.cursor, h->hc.m_rows);
            ptrace->sequential(h->hc.cursor, h->hc.m_rows, dec);
            nodirty = dec.nodirty != 0;
            sparse_now = dec.sparse != 0;
            set_lookahead(dec.lookahead != 0);
            push_ctl(h);
        }
    }

    // what cc::batch_plan decides on: settings, the scan plan, and the control block as last read back
    cc::BatchInputs batch_inputs() const
    {
        const ScanPlan& plan = h->scan_plan;
        cc::BatchInputs in{};
        in.window = win; in.win_cfg = h->hc.win_cfg; in.batch_windows = batch_windows; in.points_left = N - done;
        in.S_cfg = S_cfg; in.n_cus = h->n_cus; in.prune_wgs_per_cu = plan.prune_wgs_per_cu; in.plain_wgs_per_cu = plan.plain_wgs_per_cu;
        // (h->prune_now was set for this batch at the end of the previous one, together with the lookahead restart a
        // change of it needs: a pruned scan leaves fewer partials per point than a plain one)
        in.prune_now = h->prune_now ? 1 : 0;
        in.decide_threads = h->decide_threads; in.chain_threads = h->chain_threads; in.commit_threads = h->commit_threads;
        in.allow_claims = h->allow_claims ? 1 : 0; in.allow_long = h->allow_long ? 1 : 0;
        in.allow_heavy = h->allow_heavy ? 1 : 0; in.allow_prep = h->allow_prep ? 1 : 0;
        in.m_rows = h->hc.m_rows; in.n_heavy = h->hc.n_heavy;
        in.long_seen = longs.seen ? 1 : 0; in.long_few = longs.few ? 1 : 0; in.long_avg = longs.avg;
        return in;
    }

    // ---- the launches of a window, each kernel from one place ----

    // the claims of round `round`: T0 and T1 in turn (round 0 writes T0)
    int* claims_of(int round) const { return (round & 1) ? h->T1.p : h->T0.p; }
    const ScanCopy& sc_now() const { return scopy[seq_host & 1ull]; }  // the scan copy of this window's parity
    int quiet_ok() const { return h->allow_quiet ? 1 : 0; }
    bool sparse_round() const { return nodirty && sparse_now; }

    // the missed points of a guessed-thresholds scan split over ranks (a function of the gathered records: the same list
    // everywhere) go through the seeded chain on every rank's rows, their new records are exchanged in a second, small
    // all-gather of fixed size and take the place of the old ones
    void exchange_missed(hipStream_t st, const Rows& rws, int mode, int round, int q, int srank, int sworld)
    {
        launch_scan<false>(h, st, bp.gw, rws, nullptr, h->part.p, bp.S, round, mode, srank, sworld, 1);
        Cand* const send2 = h->gsend2.p + (size_t)q * CC_MISSED_CAP * 4;
        Cand* const recv2 = h->gpart2.p + (size_t)q * sworld * CC_MISSED_CAP * 4;
        hipLaunchKernelGGL(k_merge_partials, dim3((CC_MISSED_CAP + 255) / 256), dim3(256), 0, st, h->ctl.p,
                           h->part.p, h->part_stride, bp.S, send2, (size_t)0, round, mode,
                           (const unsigned long long*)nullptr, 0, (const int*)h->missed.p);
        h->comm.all_gather(send2, recv2, (size_t)CC_MISSED_CAP * 4 * sizeof(Cand), st, st == h->stream2 ? 1 : 0);
        hipLaunchKernelGGL(k_scatter_missed, dim3((CC_MISSED_CAP * sworld + 255) / 256), dim3(256), 0, st,
                           (const Ctl*)h->ctl.p, (const int*)h->missed.p, (const Cand*)recv2, sworld,
                           h->gpart.p, h->gpart_stride, (size_t)bp.gw * 4 + 4, round, mode);
    }

    // a snapshot scan (mode 0: this window, in place; 1: the window after it, against the scan copy of parity `round`),
    // timed on request, and in a group the exchange of its records; leaves scan_end
    void snapshot_scan(hipStream_t st, int mode, int round)
    {
        const int gw = bp.gw, S = bp.S;
        const int q = (mode == 1) ? (round & 1) : (int)(seq_host & 1ull);  // the window's parity
        const Rows& src = (mode == 1) ? srows[round & 1] : trows;
        // (d off the ladder: the scan, its probe and the relaunch for missed points in a group walk padded operands)
        const Rows rws = h->scan_plan.pad_rows ? padded_rows(h, st, src, q, round, mode) : src;
        h->probe_now = probe_left > 0 && !h->prune_now;  // (the batch's first scan carries the probe)
        if (h->probe_now) --probe_left;
        const int srank = shard_on ? myrank : 0, sworld = shard_on ? world : 1;
        // guessed thresholds with the missed points agreed on from the gathered records: whenever the scan is split
        // over more than one rank (a group of one rank takes the same steps on request, CHRONOCLUST_HIP_GROUP_GUESS=1:
        // that is how the second all-gather is exercised over RCCL on one GPU)
        h->group_guess_now = shard_on && (sworld > 1 || h->group_guess_always);
        scan_end = nullptr;
        if (stamps && mode == 0 && !shard_on && !la_on && stamped.size() + 1 < (size_t)CC_STAMP_SLOTS) {
            // in place, one stream: the chain's first kernel and k_decide stamp the device clock (cc_stamp_begin / cc_stamp_end)
            launch_scan<false>(h, st, gw, rws, nullptr, h->part.p, S, round, mode, srank, sworld);
            stamped.push_back({seq_host, h->prune_now ? 1 : 0});
            ++stamped_n;
            if (h->prune_now) ++stamped_n_p;
            return;
        }
        if (timing) {
            hipEvent_t a = get_event(h, ev_used), b = get_event(h, ev_used + 1);
            HIPCHK(hipEventRecord(a, st));
            launch_scan<false>(h, st, gw, rws, nullptr, h->part.p, S, round, mode, srank, sworld);
            HIPCHK(hipEventRecord(b, st));
            timed.push_back({ev_used, h->prune_now ? 1.0 : 0.0});  // (second: a pruned chain or a plain scan)
            ev_used += 2;
            if (!shard_on) scan_end = b;
        } else {
            launch_scan<false>(h, st, gw, rws, nullptr, h->part.p, S, round, mode, srank, sworld);
        }
        if (!shard_on) return;
        // the rank's S partials per point -> one record per point -> the records of all ranks, in rank
        // order, in the gathered buffer of the window's parity (what k_decide round 0 reads)
        if (timing) HIPCHK(hipEventRecord(get_event(h, ev_used), st));
        hipLaunchKernelGGL(k_merge_partials, dim3((gw + 255) / 256), dim3(256), 0, st, h->ctl.p, h->part.p,
                           h->part_stride, S, h->gsend.p, h->gsend_stride, round, mode,
                           (const unsigned long long*)h->pstat_p(), gw * 4,
                           (const int*)nullptr);
        h->comm.all_gather(h->gsend.p + (size_t)q * h->gsend_stride, h->gpart.p + (size_t)q * h->gpart_stride,
                           ((size_t)gw * 4 + 4) * sizeof(Cand), st, st == h->stream2 ? 1 : 0);
        if (h->prune_now && h->guess_now && h->group_guess_now && h->lean_now) ++h->stats.scan_lean_launches;
        if (h->prune_now && h->guess_now && h->group_guess_now && !h->lean_now) exchange_missed(st, rws, mode, round, q, srank, sworld);
        if (timing) {
            HIPCHK(hipEventRecord(get_event(h, ev_used + 1), st));
            timed_comm.push_back(ev_used);
            ev_used += 2;
        }
    }

    // the snapshot scans of a window: its own in place, or - with lookahead - the next window's on the second stream
    void launch_snapshot_scans(bool first_window)
    {
        if (!la_on) return snapshot_scan(sA, 0, 0);
        // first stream: this window's snapshot scan (enqueued one iteration ago on the second stream)
        if (evScan) HIPCHK(hipStreamWaitEvent(sA, evScan, 0));
        // second stream: the snapshot scan of the window after this one, against the scan copy of its
        // parity (= the table as the previous commit left it), while this window is validated on the first
        HIPCHK(hipStreamWaitEvent(sB, evCommit, 0));
        snapshot_scan(sB, 1, (int)((seq_host + 1ull) & 1ull));
        if (scan_end) evScan = scan_end;  // the timing event already marks the end of the scan: no second record
        else {
            evScan = get_sync_event(h, ev_sync++);
            HIPCHK(hipEventRecord(evScan, sB));
        }
        // only the first window of a lookahead batch can need an in-place scan (the device idles the
        // rest of a batch whose lookahead chain breaks, see Ctl::stall_b)
        if (first_window && h->hc.mode == 0) snapshot_scan(sA, 0, 0);
    }

    // k_decide.  Round 0 reads the snapshot candidates alone and carries, as extra workgroups, the previous commit's rows
    // into the scan copy of this window's parity (cc_apply_carry: the copy was last read by this window's own snapshot
    // scan, and this window's commit overwrites the carry set); round r > 0 replays against the claims of round r - 1.
    void launch_decide(int round)
    {
        const bool first = round == 0;
        // where k_decide finds the snapshot candidates of a point
        const Cand* const dec_part = shard_on ? h->gpart.p : h->part.p;
        const size_t dec_stride = shard_on ? h->gpart_stride : h->part_stride;
        const int dec_S = shard_on ? world : bp.S, dec_inner = shard_on ? 1 : bp.S;
        const size_t dec_outer = shard_on ? (size_t)bp.gw * 4 + 4 : 0;
        const int dec_tail = (first && shard_on) ? bp.gw * 4 : -1;  // where each rank's pruned-scan sample sits in its block
        const int ac_blocks = (first && la_on) ? bp.rblocks : 0;
        const int dirty_mode = (first || !nodirty) ? 0 : (sparse_round() ? 2 : 1);
        // lanes per point: 16 while a lane's two dimensions cover the point (d <= 32), else 32.  The grid is derived here -
        // bp.dblocks counts workgroups at 32 lanes per point -, with the cc_apply_carry workgroups last
        const int group = (h->d <= 32 && h->decide_group == 16) ? 16 : 32;
        const int per_wg = h->decide_threads / group;
        const dim3 grid((bp.gw + per_wg - 1) / per_wg + ac_blocks);
        hipLaunchKernelGGL(group == 16 ? k_decide<16> : k_decide<32>, grid, dim3(h->decide_threads), 0, sA, h->ctl.p, h->X.p, tab, ver, car,
                           dec_part, dec_stride, h->clean.p, h->dpart.p, h->dpart2.p, h->dseed.p,
                           first ? (const int*)nullptr : (const int*)claims_of(round - 1), claims_of(round), h->dpath.p, dec_S, Sd,
                           round, dirty_mode, bp.scan_rows, dec_inner, dec_outer,
                           first ? (const CommitRec*)h->rec.p : (const CommitRec*)nullptr, first ? sc_now() : ScanCopy{}, ac_blocks,
                           long_list, bp.long_cap, dec_tail, (!first && round == Rcur) ? 1 : 0, bp.heavy_on ? 1 : 0,
                           first ? 0 : quiet_ok(), (first && link_now) ? h->link_near.p : (int*)nullptr);
    }

    // the window's own creators (cc_link.h): points that decided "create" and would be absorbed by an earlier
    // such point claim the microcluster that one creates - before the first chain replay, not after two of them
    void launch_link()
    {
        launch_link_scan(h, sA, bp.gw);
        hipLaunchKernelGGL(k_link_apply, dim3((bp.gw + 255) / 256), dim3(256), 0, sA, h->ctl.p, tab, h->T0.p,
                           (const int*)h->link_near.p, h->dpath.p);
        ++h->stats.link_launches;
    }

    // the claims round `round` decided, gathered per microcluster: k_claims while it serves the table, k_claims_heavy for
    // the heavy rows of a larger one
    void launch_claims(int round)
    {
        if (bp.scan_rows > 0)
            hipLaunchKernelGGL(k_claims, dim3(bp.scan_rows), dim3(256), 0, sA, h->ctl.p, tab, (const int*)claims_of(round), round,
                               bp.scan_rows, round ? quiet_ok() : 0);
    }
    void launch_claims_heavy(int round)
    {
        if (!bp.heavy_on) return;
        ++h->stats.heavy_launches;
        hipLaunchKernelGGL(k_claims_heavy, dim3(CC_HEAVY_CAP), dim3(256), 0, sA, h->ctl.p, tab, (const int*)claims_of(round), round,
                           long_list, bp.long_cap, round ? quiet_ok() : 0);
    }

    // k_chain_long in the form the plan names (CC_LONG_*: one workgroup per table row or per entry of the round's list; SPLIT:
    // the large workgroups), as the preparing launch ahead of k_chain (prep_kernel) or as the replay behind it
    void launch_chain_long(int form, bool prep_kernel, int round)
    {
        if (form == CC_LONG_NONE) return;
        const bool by_list = form == CC_LONG_LIST_SPLIT || form == CC_LONG_LIST_SMALL;
        const bool split = form == CC_LONG_ROWS_SPLIT || form == CC_LONG_LIST_SPLIT;
        if (prep_kernel) h->prep_launched = true;
        else if (by_list) ++long_launches;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(by_list ? bp.long_cap : bp.long_rows), dim3(split ? CC_LONG_THREADS : 256), 0, sA, h->ctl.p,
                               h->X.p, tab, ver, car, (const int*)claims_of(round - 1), round, by_list ? 0 : bp.long_rows,
                               by_list ? (const int*)long_list : (const int*)nullptr, bp.prep ? h->lstat.p : nullptr,
                               bp.prep ? h->lprev.p : nullptr);
        };
        if (prep_kernel) launch(k_chain_long<true, true>);
        else if (split) launch(k_chain_long<true, false>);
        else launch(k_chain_long<false, false>);
    }

    void launch_chain(int round)
    {
        hipLaunchKernelGGL(k_chain, dim3(bp.cblocks), dim3(h->chain_threads), 0, sA, h->ctl.p, h->X.p, tab, ver, car,
                           (const int*)claims_of(round - 1), round, bp.long_rows, (const unsigned long long*)(bp.prep ? h->lprev.p : nullptr),
                           bp.prep ? h->lstat.p : nullptr);
    }

    void launch_dseed(int round)
    {
        hipLaunchKernelGGL(k_dseed, dim3((bp.gw + 63) / 64), dim3(64), 0, sA, h->ctl.p, h->X.p, tab, ver, car,
                           h->clean.p, h->dseed.p, (const int*)claims_of(round - 1), round, (const int8_t*)h->dpath.p, h->sp_list.p,
                           sparse_round() ? bp.sparse_cap : 0);
    }

    // the dirty scans of a round: over the version rows and, with lookahead, the carry set - the window's tiles, or (sparse)
    // the round's list of points, or not at all while k_dseed rules them out (nodirty)
    void launch_dirty_scans(int round)
    {
        if (nodirty && !sparse_round()) return;
        const bool sp = nodirty;
        // (sparse: the grid covers the list's capacity; workgroups beyond the round's count return at once)
        const int pts = sp ? bp.sparse_cap : bp.gw;
        launch_scan<true>(h, sA, pts, sp ? vrows_sp : vrows, h->dseed.p, h->dpart.p, Sd, round, 0);
        if (la_on) launch_scan<true>(h, sA, pts, sp ? crows_sp : crows, h->dseed.p, h->dpart2.p, Sd, round, 1);
    }

    void launch_commit()
    {
        hipLaunchKernelGGL(k_commit_a, dim3(1), dim3(1024), 0, sA, h->ctl.p, tab, ver, car, h->T0.p, h->T1.p,
                           h->rk.p, h->rec.p, (const Cand*)h->clean.p, (const int8_t*)h->dpath.p);
        hipLaunchKernelGGL(k_commit_b, dim3(bp.rblocks), dim3(h->commit_threads), 0, sA, h->rec.p, tab, ver, car, h->rk.p, h->dpath.p,
                           h->lab_uid.p, h->lab_path.p, h->d, sc_now(), h->hc.filter);
    }

    // one batch of windows: per window the snapshot scan (in place or one window ahead on the second stream), round 0 of
    // the decisions, the validation rounds, the commit - all enqueued without a host round-trip
    void enqueue_batch()
    {
        batch_t0 = now_ms();
        bp = cc::batch_plan(batch_inputs());
        trows = rows_of_table(tab);
        vrows = rows_of_versions(ver);
        crows = rows_of_carry(car, ver, tab);
        vrows_sp = sparse_rows(vrows, h->sp_list.p);
        crows_sp = sparse_rows(crows, h->sp_list.p);
        long_list = bp.long_listed ? h->long_list.p : nullptr;
        ev_sync = ev_base;
        // lookahead scans read a scan copy of the table (see ScanCopy): both in line with the table at the start of
        // a batch, then kept up commit by commit
        scopy[0] = scopy[1] = ScanCopy{};
        if (la_on) scan_copy_sync(h, scopy);
        for (int q = 0; q < 2; ++q) srows[q] = rows_of_scan_copy(scopy[q]);
        evScan = nullptr;  // the scan of the batch's first window is complete (the second stream was drained)
        if (la_on) HIPCHK(hipEventRecord(evCommit, sA));  // everything so far (table, control block) is in place
        probe_left = (dec.probe != 0) ? 1 : 0;
        for (int wv = 0; wv < bp.windows_now; ++wv, ++seq_host) {
            launch_snapshot_scans(wv == 0);
            launch_decide(0);
            if (link_now) launch_link();
            launch_claims(0);
            launch_claims_heavy(0);
            for (int r = 1; r <= Rcur; ++r) {
                if (bp.prep) launch_chain_long(bp.prep_form, true, r);
                launch_chain(r);
                launch_chain_long(bp.long_form, false, r);
                launch_dseed(r);
                launch_dirty_scans(r);
                launch_decide(r);
                // (the claims of the last round are not replayed: nothing to gather either)
                if (r < Rcur) {
                    launch_claims(r);
                    launch_claims_heavy(r);
                }
            }
            launch_commit();
            if (la_on) {
                evCommit = get_sync_event(h, ev_sync++);
                HIPCHK(hipEventRecord(evCommit, sA));
            }
        }
    }

    // the batch has been enqueued: wait for it, read the control block back, let the policy decide how the next one runs
    int after_batch()
    {
        HIPCHK(hipGetLastError());
        pull_ctl_pinned(h);
        if (la_on) sync_stream(h, sB);
        // the stamped scans of the windows that ran (a prefix of the batch: the device's sequence number has passed them); a
        // window the device idled left its begin stamp at 0
        for (const auto& s : stamped) {
            if (s.first >= h->hc.window_seq) break;
            const size_t slot = (size_t)(s.first & (unsigned long long)(CC_STAMP_SLOTS - 1));
            const unsigned long long t0 = h->hc.scan_t0[slot], t1 = h->hc.scan_t1[slot];
            if (t0 == 0ull || t1 <= t0) continue;
            const double ms = (double)(t1 - t0) / (double)h->wall_khz;
            stamped_ms += ms;
            if (s.second) stamped_ms_p += ms;
        }
        stamped.clear();
        seq_host = h->hc.window_seq;
        done = h->hc.cursor;
        const double dt = now_ms() - batch_t0;
        const long long pts_b = h->hc.cursor - cursor_prev;
        link_now = cc::link_after_batch(h->allow_link && !no_create, h->hc.m_rows - m_known, pts_b);
        m_known = h->hc.m_rows;
        cursor_prev = h->hc.cursor;
        longs.after_batch(h->hc.stat_long, h->hc.stat_rounds);
        const bool shard_was = shard_on;
        // what the device counted, and the policy's decision for the next batch
        cc_policy_obs o{};
        o.cursor = h->hc.cursor;
        o.m_rows = h->hc.m_rows;
        o.stall_b = h->hc.stall_b;
        o.stat_windows = h->hc.stat_windows;
        o.stat_truncated = h->hc.stat_truncated;
        o.stat_trunc_unknown = h->hc.stat_trunc_unknown;
        o.stat_tiles = h->hc.stat_tiles;
        o.stat_dirty_tiles = h->hc.stat_dirty_tiles;
        o.stat_unsafe = h->hc.stat_unsafe;
        o.stat_missed = h->hc.stat_missed;
        o.tg_ok = (h->hc.tg_ok[0][0] != 0 && h->hc.tg_ok[1][0] != 0) ? 1 : 0;  // (a mean for the pcore kind in both slots)
        for (int r = 0; r < CC_MAX_ROUNDS + 2; ++r) o.round_hist[r] = h->hc.round_hist[r];
        o.prune_rows = h->hc.stat_prune_rows;
        o.prune_full = h->hc.stat_prune_full;
        dec = policy->after_batch(o);
        ptrace->batch(o, dec);
        const cc_policy_carry& k = policy->carry();
        h->adapt_win = k.adapt_win; h->clean_batches = k.clean_batches; h->since_shrink = k.since_shrink;
        if (dec.stalled)
            return fail(h, CC_ERR_INTERNAL, "the online phase made no progress in five consecutive batches of windows");
        if (h->trace && dec.prune_rows > 0)
            fprintf(stderr, "[cc] pruned scans of the batch%s (sample): %lld (wave, row) pairs, %.1f %% evaluated in full; points missed by guessed thresholds so far: %lld\n",
                    h->guess_now ? ", guessed thresholds" : "", (long long)dec.prune_rows,
                    100.0 * (double)dec.prune_full / (double)dec.prune_rows, (long long)h->hc.stat_missed);
        pair_rows_eff += (h->hc.stat_pair_rows - pair_rows_prev) / (shard_was ? (double)world : 1.0);
        if (h->prune_now) pair_rows_pruned += (h->hc.stat_pair_rows - pair_rows_prev) / (shard_was ? (double)world : 1.0);
        pair_rows_prev = h->hc.stat_pair_rows;
        if (shard_was) sharded_windows += dec.wins;
        Rcur = dec.rounds;
        Sd = Sd_full;
        nodirty = dec.nodirty != 0;
        sparse_now = dec.sparse != 0;
        shard_on = dec.shard != 0;
        h->set_prune(dec.prune);
        if (dec.restart) {
            h->hc.win_cfg = dec.win_cfg;
            h->hc.win_b = (int)std::min<long long>(dec.win_cfg, N - done);
            set_lookahead(dec.lookahead != 0);
            push_ctl_pinned(h);
        }
#ifdef CC_ROUND_DEBUG
        for (int r = 1; r <= CC_MAX_ROUNDS; ++r)
            if (h->hc.dbg_round[r][5] != 0)
                fprintf(stderr, "[cc]    round %d so far: %llu decisions, %llu refused, create->join new %llu, create->join row %llu, join->create %llu, other MC %llu | windows ended in round %d: %lld\n",
                        r, h->hc.dbg_round[r][5], h->hc.dbg_round[r][0], h->hc.dbg_round[r][1], h->hc.dbg_round[r][2], h->hc.dbg_round[r][3],
                        h->hc.dbg_round[r][4], r, (long long)h->hc.round_hist[r]);
#endif
        if (h->trace)
            fprintf(stderr, "[cc] %.2f ms done %lld rows %d | batch: %lld windows %lld points trunc %lld (%lld at an undecidable point) lookahead %lld dirty tiles %lld / %lld (points so far: %lld unlocated, %lld unsafe) | next window %d rounds %d\n",
                    now_ms() - batch_t0, done, h->hc.m_rows, (long long)dec.wins, (long long)dec.pts, (long long)dec.trunc, (long long)dec.unk, (long long)h->hc.stat_lookahead, (long long)dec.dtiles, (long long)dec.tiles,
                    (long long)h->hc.stat_unprovable, (long long)h->hc.stat_unsafe, dec.want, Rcur);
        batch_windows = dec.batch_windows;
        // the batch's wall-clock rate (none when it committed nothing) against the sequential kernel's: cc::SeqHandover
        seq.after_batch(dec.bad != 0, pts_b > 0 ? (double)pts_b / std::max(dt, 1e-3) : 0.0, seq_possible(), done < N, seq_r_applies(),
                        seq_rate_guess());
        return (int)CC_OK;
    }

    // statistics of the call
    void finish()
    {
        HIPCHK(hipEventRecord(ev1, h->stream));
        HIPCHK(hipEventSynchronize(ev1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
        h->stats.run_ms += ms;
        h->stats.points += N - range_a;
        h->stats.windows += h->hc.stat_windows;
        h->stats.rounds += h->hc.stat_rounds;
        h->stats.truncated += h->hc.stat_truncated;
        h->stats.rows = h->hc.m_rows;
        h->stats.scan_pair_dims += pair_rows_eff * (double)h->d;
        h->stats.scan_pair_dims_pruned += pair_rows_pruned * (double)h->d;
        h->stats.sharded_windows += sharded_windows;
        h->stats.seq_points += h->hc.stat_seq_points;
        h->stats.seq_r_points += h->hc.stat_seq_r_points;
#ifdef CC_SEQG_TIMERS
        fprintf(stderr, "[cc] k_seq_g (shader cycles, thread 0): scan %llu minimum %llu add %llu barrier %llu rest %llu chunk %llu | points %llu\n",
                h->hc.dbg_long[0], h->hc.dbg_long[1], h->hc.dbg_long[2], h->hc.dbg_long[3], h->hc.dbg_long[4], h->hc.dbg_long[5], h->hc.dbg_long[7]);
#endif
#ifdef CC_LONG_TIMERS
        fprintf(stderr, "[cc] k_chain_long, workgroup 0 (shader cycles): collect %llu stage %llu chains %llu step-dim %llu step %llu rows %llu state %llu | batches %llu\n",
                h->hc.dbg_long[0], h->hc.dbg_long[1], h->hc.dbg_long[2], h->hc.dbg_long[3], h->hc.dbg_long[4], h->hc.dbg_long[5], h->hc.dbg_long[6], h->hc.dbg_long[7]);
#endif
        h->seq_sticky = seq.on();
        h->stats.table_rows_scanned += h->hc.stat_table_rows;
        h->stats.lookahead_windows += h->hc.stat_lookahead;
        h->stats.pruned_scan_rows += (int64_t)h->hc.stat_prune_rows;
        h->stats.pruned_scan_full_rows += (int64_t)h->hc.stat_prune_full;
        h->stats.long_chains += (int64_t)h->hc.stat_long;
        h->stats.long_chain_launches += long_launches;
        if (h->prep_launched) {
            h->prep_launched = false;
            unsigned long long lp[2] = {0ull, 0ull};
            HIPCHK(hipMemcpy(lp, h->lstat.p + 2 * CC_LSTAT_ROWS, sizeof(lp), hipMemcpyDeviceToHost));
            h->stats.long_prepared += (int64_t)lp[0];
            h->stats.long_replayed += (int64_t)lp[1];
        }
        h->stats.tiles += h->hc.stat_tiles;
        h->stats.dirty_tiles += h->hc.stat_dirty_tiles;
        h->stats.missed_points += h->hc.stat_missed;
        h->probe_now = false;
        if (timing) {
            double tot = 0.0, tot_p = 0.0;
            int64_t n_p = 0;
            for (auto& t : timed) {
                float e = 0.f;
                HIPCHK(hipEventElapsedTime(&e, h->ev_pool[t.first], h->ev_pool[t.first + 1]));
                tot += e;
                if (t.second != 0.0) { tot_p += e; ++n_p; }
            }
            // (the stamped scans were summed batch by batch, after_batch; launches are counted as enqueued either way)
            h->stats.scan_launches += (int64_t)timed.size() + stamped_n;
            h->stats.scan_ms += tot + stamped_ms;
            h->stats.scan_launches_pruned += n_p + stamped_n_p;
            h->stats.scan_ms_pruned += tot_p + stamped_ms_p;
            double ctot = 0.0;
            for (size_t i : timed_comm) {
                float e = 0.f;
                HIPCHK(hipEventElapsedTime(&e, h->ev_pool[i], h->ev_pool[i + 1]));
                ctot += e;
            }
            h->stats.comm_launches += (int64_t)timed_comm.size();
            h->stats.comm_ms += ctot;
        }
    }

    int run()
    {
        prepare();
        while (done < N) {
            ensure_table(h, (size_t)m_known + std::max<size_t>(window_rows(), seq.on() ? 8192 : 0) + 1);
            tab = h->tab.view();
            if (seq.on()) {
                sequential_stint();
                continue;
            }
            enqueue_batch();
            const int rc = after_batch();
            if (rc != CC_OK) return rc;
        }
        finish();
        return (int)CC_OK;
    }
};

// The exact windowed online phase over the resident points [range_a, range_e), in row order.  no_create: a point that
// no MC absorbs does not create one; it is set aside (label -1, path code 8) and changes nothing - the first half of a
// super-step of the relaxed multi-GPU mode (section 6 of DESIGN.md).  Statistics are added to h->stats.
// resume: the range continues a stream this handle was clustering a moment ago (a later mini-batch of a timepoint): the
// window size carries over as it is instead of restarting small.
int online_range(cc_handle* h, long long range_a, long long range_e, bool no_create, bool resume)
{
    if (range_e <= range_a) return (int)CC_OK;
    if (h->d > CC_WINDOW_MAX_DIM && (h->comm.active() || no_create || !h->allow_seq_g))
        return fail(h, CC_ERR_BAD_ARG, "more than " + std::to_string(CC_WINDOW_MAX_DIM) + " dimensions: the online phase runs on the sequential "
                    "workgroup kernel (k_seq_g) only - not in a multi-GPU group, not with CHRONOCLUST_HIP_SEQG=0");
    if (h->d == 0) return fail(h, CC_ERR_BAD_ARG, "no points uploaded");
    OnlineRun run(h, range_a, range_e, no_create, resume);
    return run.run();
}

}  // namespace
