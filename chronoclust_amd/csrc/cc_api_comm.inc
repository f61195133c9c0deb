// cc_api_comm.inc — the host side of the multi-GPU paths: the all-reduce of the relaxed mode and its super-steps
// (online_relaxed), the communicator set-up (RCCL, in-process), the calibration of the split thresholds, the relaxed
// mode's and the thresholds' setters and getters.  (included by cc_api.hip, the one translation unit, behind
// cc_online_run.h and the scan dispatcher of cc_api.hip: online_relaxed runs online_range, cc_comm_calibrate times k_scan_u at
// the residency scan_u_wgs_per_cu reports)

namespace {

// sum over the ranks of buf[0 .. count), the same result on every rank, ordered on `st`
void comm_all_reduce_sum(cc_handle* h, double* buf, size_t count, hipStream_t st)
{
    cc::Comm& cm = h->comm;
    // (fail_group() drops the communicators, so a broken group no longer looks like an RCCL one: ask first)
    if (cm.broken) throw cc::CommErr{"the group has failed earlier"};
    if (cm.rccl()) {
        cm.check(cc::RcclApi::get().AllReduce(buf, buf, count, ncclDouble, ncclSum, cm.lane(0), st), "ncclAllReduce");
        return;
    }
    if (!cm.local || cm.world == 1) return;
    h->r_gather.ensure((size_t)cm.world * count);
    cm.all_gather(buf, h->r_gather.p, count * 8, st);
    hipLaunchKernelGGL(k_sum_ranks, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, h->r_gather.p, cm.world, count, buf);
}

// Relaxed multi-GPU mode: the points of the timepoint are sharded over the ranks in contiguous blocks; per super-step
// every rank clusters `relaxed_minibatch` of its points against the shared table (exact path, no MC creation), the CF
// changes are all-reduced, and the set-aside points of all ranks are clustered redundantly on every rank (exact path).
int online_relaxed(cc_handle* h)
{
    const long long N = h->n_points;
    const int W = h->comm.world, rank = h->comm.rank, d = h->d;
    if (N == 0) return (int)CC_OK;
    if (d == 0) return fail(h, CC_ERR_BAD_ARG, "no points uploaded");
    const long long L = (N + W - 1) / W;  // shard length
    const long long a0 = std::min(N, (long long)rank * L), e0 = std::min(N, a0 + L);
    const long long b = h->relaxed_minibatch;
    // Mini-batches grow from 2 048 points per rank by doubling: while the table is (nearly) empty every point is set
    // aside and clustered by all ranks redundantly, so the first super-steps are kept small; the schedule depends on
    // nothing but the shard length, hence is the same on every rank.
    std::vector<long long> starts(1, 0);
    for (long long sz = std::min<long long>(b, 2048); starts.back() < L; sz = std::min(b, sz * 2)) starts.push_back(std::min(L, starts.back() + sz));
    const long long steps = (long long)starts.size() - 1;
    hipStream_t st = h->stream;
    memset(&h->rstats, 0, sizeof(h->rstats));
    struct Suspend {  // (restored on every way out)
        cc_handle* h;
        explicit Suspend(cc_handle* hh) : h(hh) { h->shard_suspended = true; }
        ~Suspend() { h->shard_suspended = false; }
    } suspend(h);
    // labels: room for every rank's padded shard (the final all-gather is in place); -1 = not clustered yet
    if (h->lab_uid.n < (size_t)(L * W)) { h->lab_uid.ensure((size_t)(L * W)); h->lab_path.ensure((size_t)(L * W)); }
    HIPCHK(hipMemsetAsync(h->lab_uid.p, 0xFF, (size_t)(L * W) * 8, st));
    HIPCHK(hipMemsetAsync(h->lab_path.p, 0, (size_t)(L * W), st));
    h->r_didx.ensure((size_t)b + 1);
    h->r_didx_all.ensure((size_t)W * (b + 1));
    std::vector<int> didx_host((size_t)W * (b + 1)), list;
    for (long long sidx = 0; sidx < steps; ++sidx) {
        const long long a = std::min(e0, a0 + starts[sidx]), e = std::min(e0, a0 + starts[sidx + 1]);
        // ---- snapshot of the table all ranks share ----
        refresh_ctl_params(h);
        const int M = h->hc.m_rows;
        const int n_pkeys0 = h->hc.n_pkeys;
        const long long pid0 = h->hc.pcore_last_id;
        const size_t md = (size_t)M * d, dl = (size_t)M * (2 * d + 1);
        if (M > 0) {
            h->rs_cf1.ensure(md); h->rs_cf2.ensure(md); h->rs_w.ensure(M); h->rs_kind.ensure(M); h->rs_key.ensure(M);
            h->rs_id.ensure(M); h->r_delta.ensure(dl);
            HIPCHK(hipMemcpyAsync(h->rs_cf1.p, h->tab.cf1.p, md * 8, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync(h->rs_cf2.p, h->tab.cf2.p, md * 8, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync(h->rs_w.p, h->tab.w.p, (size_t)M * 8, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync(h->rs_kind.p, h->tab.kind.p, (size_t)M * 4, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync(h->rs_key.p, h->tab.key.p, (size_t)M * 4, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync(h->rs_id.p, h->tab.id.p, (size_t)M * 8, hipMemcpyDeviceToDevice, st));
        }
        // ---- A: this rank's mini-batch, no MC creation ----
        const auto tA0 = std::chrono::steady_clock::now();
        if (h->trace) sync_stream(h, st);
        const auto tA1 = std::chrono::steady_clock::now();
        int rc = online_range(h, a, e, true, sidx > 0);
        const auto tA2 = std::chrono::steady_clock::now();
        if (rc != CC_OK) return rc;
        if (h->hc.m_rows != M) return fail(h, CC_ERR_INTERNAL, "relaxed mode: a mini-batch created microclusters");
        // ---- M: merge the changes of the existing rows ----
        if (M > 0) {
            const Table tab = h->tab.view();  // (online_range may have moved the table)
            hipLaunchKernelGGL(k_rel_delta, dim3((unsigned)((md + 255) / 256)), dim3(256), 0, st, tab, h->rs_cf1.p, h->rs_cf2.p,
                               h->rs_w.p, M, d, h->r_delta.p);
            comm_all_reduce_sum(h, h->r_delta.p, dl, st);
            hipLaunchKernelGGL(k_rel_merge, dim3((unsigned)((md + 255) / 256)), dim3(256), 0, st, tab, h->rs_cf1.p, h->rs_cf2.p,
                               h->rs_w.p, h->rs_kind.p, h->rs_key.p, h->rs_id.p, M, d, h->r_delta.p, h->hc.delta_sq, h->hc.k,
                               h->hc.pow2, h->hc.inv_k);
            hipLaunchKernelGGL(k_rel_promote, dim3(1), dim3(1024), 0, st, h->ctl.p, tab, M, d, h->r_delta.p, h->hc.beta_mu,
                               h->hc.pi, n_pkeys0, pid0);
        }
        // ---- B: the set-aside points of all ranks, in rank order, on every rank ----
        hipLaunchKernelGGL(k_rel_collect, dim3(1), dim3(1024), 0, st, h->lab_uid.p, a, e, h->r_didx.p);
        // their numbers first (4 bytes per rank); the index lists only travel when there are any - in the steady state
        // there are none
        h->r_cnt_all.ensure((size_t)W);
        h->comm.all_gather(h->r_didx.p, h->r_cnt_all.p, 4, st);
        std::vector<int> cnt_host((size_t)W);
        HIPCHK(hipMemcpyAsync(cnt_host.data(), h->r_cnt_all.p, (size_t)W * 4, hipMemcpyDeviceToHost, st));
        pull_ctl(h);  // (synchronises the stream; the counters k_rel_promote left)
        long long total = 0;
        for (int r = 0; r < W; ++r) total += cnt_host[r];
        list.clear();
        if (total > 0) {  // (the same decision on every rank: the counts are the gathered ones)
            h->comm.all_gather(h->r_didx.p, h->r_didx_all.p, (size_t)(b + 1) * 4, st);
            HIPCHK(hipMemcpyAsync(didx_host.data(), h->r_didx_all.p, didx_host.size() * 4, hipMemcpyDeviceToHost, st));
            sync_stream(h, st);
            for (int r = 0; r < W; ++r) {
                const int* blk = didx_host.data() + (size_t)r * (b + 1);
                list.insert(list.end(), blk + 1, blk + 1 + blk[0]);
            }
        }
        if (h->trace) {
            const auto tA3 = std::chrono::steady_clock::now();
            auto ms = [](auto x, auto y) { return std::chrono::duration<double, std::milli>(y - x).count(); };
            fprintf(stderr, "[cc] relaxed super-step %lld: %lld points | snapshot %.3f ms, sharded half %.3f ms, merge + collect %.3f ms, set aside %lld\n",
                    sidx, e - a, ms(tA0, tA1), ms(tA1, tA2), ms(tA2, tA3), total);
        }
        h->rstats.super_steps += 1;
        h->rstats.minibatch_points += e - a;
        const long long K = (long long)list.size();
        if (K > 0) {
            h->rstats.deferred_points += K;
            h->r_didx_all.ensure((size_t)std::max<long long>((long long)W * (b + 1), K));
            HIPCHK(hipMemcpyAsync(h->r_didx_all.p, list.data(), (size_t)K * 4, hipMemcpyHostToDevice, st));
            h->rg_X.ensure((size_t)K * d); h->rg_Xt.ensure((size_t)K * xt_dims(d)); h->rg_uid.ensure((size_t)K); h->rg_path.ensure((size_t)K);
            hipLaunchKernelGGL(k_rel_gather_points, dim3((unsigned)(((size_t)K * d + 255) / 256)), dim3(256), 0, st, h->X.p,
                               h->r_didx_all.p, (int)K, d, h->rg_X.p);
            HIPCHK(transpose_points_padded(st, h->rg_X.p, h->rg_Xt.p, K, d));  // (the exact run below may scan over padded operands)
            // the gathered points take the place of the resident ones for one exact run
            auto swap_in = [&]() {
                h->X.swap(h->rg_X);
                h->Xt.swap(h->rg_Xt);
                h->lab_uid.swap(h->rg_uid);
                h->lab_path.swap(h->rg_path);
            };
            swap_in();
            h->n_points = K;
            // (the window policy this rank's mini-batches settled on is not the business of the replicated half)
            const int keep_win = h->adapt_win, keep_clean = h->clean_batches, keep_shrink = h->since_shrink;
            auto restore_policy = [&]() { h->adapt_win = keep_win; h->clean_batches = keep_clean; h->since_shrink = keep_shrink; };
            try {
                rc = online_range(h, 0, K, false, false);
            } catch (...) {
                swap_in();
                h->n_points = N;
                restore_policy();
                throw;
            }
            swap_in();
            h->n_points = N;
            restore_policy();
            if (rc != CC_OK) return rc;
            hipLaunchKernelGGL(k_rel_scatter_labels, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, h->rg_uid.p,
                               h->rg_path.p, h->r_didx_all.p, (int)K, h->lab_uid.p, h->lab_path.p);
        }
    }
    // every rank's shard of the labels to every rank (in place, shards padded to the same length)
    h->comm.all_gather(h->lab_uid.p + (size_t)rank * L, h->lab_uid.p, (size_t)L * 8, st);
    h->comm.all_gather(h->lab_path.p + (size_t)rank * L, h->lab_path.p, (size_t)L, st);
    sync_stream(h, st);
    HIPCHK(hipGetLastError());
    h->stats.points = N;
    return (int)CC_OK;
}

}  // namespace

extern "C" {

// ---- exact multi-GPU path: communicator set-up -------------------------------------------------------

int cc_comm_unique_id(void* out_id)
{
    if (!out_id) return CC_ERR_BAD_ARG;
    cc::RcclApi& api = cc::RcclApi::get();
    if (!api.ok()) return CC_ERR_COMM;
    ncclUniqueId id;
    if (api.GetUniqueId(&id) != ncclSuccess) return CC_ERR_COMM;
    static_assert(sizeof(id) == CC_COMM_ID_BYTES, "ncclUniqueId size");
    memcpy(out_id, &id, sizeof(id));
    return CC_OK;
}

int cc_comm_init_rccl(cc_handle* h, const void* id_bytes, int rank, int world)
{
    if (!h || !id_bytes || world < 1 || rank < 0 || rank >= world) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() {
        if (h->comm.active()) return fail(h, CC_ERR_BAD_ARG, "the handle already belongs to a group");
        cc::RcclApi& api = cc::RcclApi::get();
        if (!api.ok()) return fail(h, CC_ERR_COMM, std::string("librccl could not be loaded: ") + (dlerror() ? dlerror() : "missing symbol"));
        ncclUniqueId id;
        memcpy(&id, id_bytes, sizeof(id));
        ncclComm_t comm = nullptr;
        ncclResult_t r = api.CommInitRank(&comm, world, id, rank);  // (the handle's device is current)
        if (r != ncclSuccess) return fail(h, CC_ERR_COMM, std::string("ncclCommInitRank: ") + api.GetErrorString(r));
        h->comm.nccl[0] = comm;
        h->comm.rank = rank;
        h->comm.world = world;
        h->comm.broken = false;
        const char* to = getenv("CHRONOCLUST_HIP_COMM_TIMEOUT_S");
        if (to && atof(to) > 0.0) h->comm.timeout_s = atof(to);
        // ONE communicator serves both streams by default: RCCL then orders the lookahead scans' all-gathers (second
        // stream) with those of the validation stream, which costs some overlap but is the mode every RCCL user runs.
        // CHRONOCLUST_HIP_TWO_COMMS=1: a second communicator for the lookahead stream (its id is made by rank 0 and
        // travels through the first one), so that the two streams' collectives are independent - concurrent
        // communicators need both collective kernels co-resident on every rank and have never run on more than one
        // GPU in a build session: opt-in until a multi-GPU run has confirmed them
        const char* two = getenv("CHRONOCLUST_HIP_TWO_COMMS");
        if (two && two[0] == '1') {
            DevBuf<char> ids;
            ids.ensure((size_t)world * sizeof(ncclUniqueId) + sizeof(ncclUniqueId));
            ncclUniqueId id2;
            memset(&id2, 0, sizeof id2);
            if (rank == 0) {
                r = api.GetUniqueId(&id2);
                if (r != ncclSuccess) return fail(h, CC_ERR_COMM, std::string("ncclGetUniqueId: ") + api.GetErrorString(r));
            }
            char* send = ids.p + (size_t)world * sizeof(ncclUniqueId);
            HIPCHK(hipMemcpyAsync(send, &id2, sizeof id2, hipMemcpyHostToDevice, h->stream));
            h->comm.all_gather(send, ids.p, sizeof id2, h->stream, 0);
            HIPCHK(hipMemcpyAsync(&id2, ids.p, sizeof id2, hipMemcpyDeviceToHost, h->stream));  // rank 0's block
            sync_stream(h, h->stream);
            ncclComm_t comm2 = nullptr;
            r = api.CommInitRank(&comm2, world, id2, rank);
            if (r != ncclSuccess) return fail(h, CC_ERR_COMM, std::string("ncclCommInitRank (second communicator): ") + api.GetErrorString(r));
            h->comm.nccl[1] = comm2;
        }
        // the split thresholds from a measurement of this group's own exchange (collective: every rank is here)
        const char* cal = getenv("CHRONOCLUST_HIP_CALIBRATE");
        if (!(cal && cal[0] == '0')) {
            const int rc = cc_comm_calibrate(h);
            if (rc != CC_OK) return rc;
        }
        return (int)CC_OK;
    });
}

int cc_comm_calibrate(cc_handle* h)
{
    if (!h) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() {
        if (!h->comm.active()) return fail(h, CC_ERR_BAD_ARG, "cc_comm_calibrate: the handle belongs to no group");
        const int world = h->comm.world, rank = h->comm.rank;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        auto timed3 = [&](auto&& fn) {  // one untimed pass, then the minimum of three
            fn();
            sync_stream(h, h->stream);
            float best = 1e30f;
            for (int i = 0; i < 3; ++i) {
                HIPCHK(hipEventRecord(e0, h->stream));
                fn();
                HIPCHK(hipEventRecord(e1, h->stream));
                sync_stream(h, h->stream);
                float ms = 0.f;
                HIPCHK(hipEventElapsedTime(&ms, e0, e1));
                best = std::min(best, ms);
            }
            return (double)best * 1e3;  // us
        };
        // (1) the exchange of a split window: one full window's records from every rank
        const int win = std::min(h->tun.window, CC_MAX_WINDOW);
        const size_t rec = ((size_t)win * 4 + 4) * sizeof(Cand);
        DevBuf<char> sbuf, rbuf;
        sbuf.ensure(rec);
        rbuf.ensure(rec * (size_t)world);
        HIPCHK(hipMemsetAsync(sbuf.p, 0, rec, h->stream));
        const double ag_us = timed3([&]() { h->comm.all_gather(sbuf.p, rbuf.p, rec, h->stream, 0); });
        // (2) what a table row costs: the plain snapshot scan of a full window over 4 096 synthetic rows x 20 dimensions, on
        // scratch buffers and a control block of its own (the handle's state is not touched)
        constexpr int DPc = 20, Rc = 4096;
        constexpr int NWc = ScanShape<DPc, false>::NW;
        DevBuf<Ctl> cctl;
        DevBuf<double> cxt, ccen, cscl;
        DevBuf<int> ckind, ckey;
        DevBuf<Cand> cpart;
        const int tiles = (win + 63) / 64;
        const int Sc = std::max(1, std::min(16, (h->n_cus * scan_u_wgs_per_cu<DPc>()) / std::max(1, tiles)));
        cctl.ensure(1); cxt.ensure((size_t)win * DPc); ccen.ensure((size_t)Rc * DPc); cscl.ensure((size_t)Rc * DPc);
        ckind.ensure(Rc); ckey.ensure(Rc); cpart.ensure((size_t)2 * win * Sc * 4);
        {
            std::vector<double> x((size_t)win * DPc), cen((size_t)Rc * DPc), scl((size_t)Rc * DPc, 0.25);
            unsigned long long st = 0x9E3779B97F4A7C15ull;
            auto rnd = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (double)(st >> 11) * 0x1p-53; };
            for (auto& v : x) v = 0.1 + 0.8 * rnd();
            for (auto& v : cen) v = 0.1 + 0.8 * rnd();
            std::vector<int> kind(Rc, CC_KIND_PCORE), key(Rc);
            for (int i = 0; i < Rc; ++i) key[i] = i;
            Ctl c;
            memset(&c, 0, sizeof c);
            c.d = DPc; c.m_rows = Rc; c.win_b = win; c.win_cfg = win; c.n_points = win; c.xt_stride = win;
            c.k = 4.0; c.inv_k = 0.25; c.pow2 = 1;
            HIPCHK(hipMemcpyAsync(cctl.p, &c, sizeof c, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(cxt.p, x.data(), x.size() * 8, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(ccen.p, cen.data(), cen.size() * 8, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(cscl.p, scl.data(), scl.size() * 8, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(ckind.p, kind.data(), (size_t)Rc * 4, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(ckey.p, key.data(), (size_t)Rc * 4, hipMemcpyHostToDevice, h->stream));
            sync_stream(h, h->stream);  // (the host vectors go out of scope)
        }
        const double scan_us = timed3([&]() {
            hipLaunchKernelGGL((k_scan_u<DPc, NWc>), dim3(tiles, Sc), dim3(64 * NWc), 0, h->stream, (const Ctl*)cctl.p, (const double*)cxt.p,
                               (const double*)ccen.p, (const double*)cscl.p, (const int*)ckind.p, (const int*)ckey.p, cpart.p, 0, 0,
                               (size_t)win * Sc * 4, 0, 1);
        });
        HIPCHK(hipGetLastError());
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        // (3) every rank takes the group's maxima: the thresholds decide the sequence of collectives and must be the same
        // everywhere (an all-gather of two doubles per rank through the transport itself)
        double mine[2] = {ag_us, scan_us * 1e3 / ((double)Rc * DPc)};  // us, ns per (row, dim)
        DevBuf<double> dsend, drecv;
        dsend.ensure(2);
        drecv.ensure((size_t)2 * world);
        HIPCHK(hipMemcpyAsync(dsend.p, mine, sizeof mine, hipMemcpyHostToDevice, h->stream));
        h->comm.all_gather(dsend.p, drecv.p, sizeof mine, h->stream, 0);
        std::vector<double> all((size_t)2 * world);
        HIPCHK(hipMemcpyAsync(all.data(), drecv.p, all.size() * 8, hipMemcpyDeviceToHost, h->stream));
        sync_stream(h, h->stream);
        double ag = 0.0, sc = 0.0;
        for (int r = 0; r < world; ++r) { ag = std::max(ag, all[(size_t)2 * r]); sc = std::max(sc, all[(size_t)2 * r + 1]); }
        h->calib_ag_us = ag;
        h->calib_scan_ns = sc;
        if (world > 1 && sc > 0.0) {
            // time saved by the split = scan x (1 - 1 / world); it pays from scan >= exchange x world / (world - 1) on
            const double row_dims = ag * 1e3 * (double)world / (double)(world - 1) / sc;
            h->shard_min_row_dims = (long long)std::min(row_dims, 1e15);
            h->shard_min_row_dims_pruned = (long long)std::min(row_dims * 3.3, 1e15);
        }
        if (h->trace)
            fprintf(stderr, "[cc] rank %d of %d: all-gather of a %d-point window's records %.1f us, plain scan %.3f ns per (row, dim) "
                    "(group maxima) -> scans split from %lld (plain) / %lld (pruned) row-dims on\n", rank, world, win, ag, sc,
                    (long long)h->shard_min_row_dims, (long long)(h->shard_min_row_dims_pruned > 0 ? h->shard_min_row_dims_pruned : h->shard_min_row_dims));
        return (int)CC_OK;
    });
}

int cc_comm_init_local(cc_handle** handles, int world)
{
    if (!handles || world < 1) return CC_ERR_BAD_ARG;
    for (int r = 0; r < world; ++r)
        if (!handles[r] || handles[r]->comm.active()) return CC_ERR_BAD_ARG;
    auto grp = std::make_shared<cc::LocalGroup>(world);
    // every member's events first: a failure leaves no handle half inside a group
    for (int r = 0; r < world; ++r) {
        cc_handle* h = handles[r];
        int rc = guarded(h, [&]() {
            HIPCHK(hipEventCreateWithFlags(&h->comm.ev_ready, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&h->comm.ev_done, hipEventDisableTiming));
            return (int)CC_OK;
        });
        if (rc != CC_OK) {
            for (int q = 0; q <= r; ++q) handles[q]->comm.destroy();
            return rc;
        }
    }
    for (int r = 0; r < world; ++r) {
        handles[r]->comm.local = grp;
        handles[r]->comm.rank = r;
        handles[r]->comm.world = world;
    }
    return CC_OK;
}

int cc_comm_destroy(cc_handle* h)
{
    if (!h) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() {
        try {
            sync_stream(h, h->stream);
            sync_stream(h, h->stream2);
        } catch (const cc::CommErr&) {  // (the group is already lost: nothing left to drain)
        }
        h->comm.destroy();
        return (int)CC_OK;
    });
}

int cc_comm_info(cc_handle* h, int32_t* rank, int32_t* world, int32_t* transport)
{
    if (!h) return CC_ERR_BAD_ARG;
    if (rank) *rank = h->comm.rank;
    if (world) *world = h->comm.world;
    if (transport) *transport = h->comm.rccl() ? 1 : (h->comm.local ? 2 : 0);
    return CC_OK;
}

int cc_comm_set_relaxed(cc_handle* h, int32_t minibatch_points)
{
    if (!h || minibatch_points < 0) return CC_ERR_BAD_ARG;
    if (minibatch_points > 0 && !h->comm.active()) return fail(h, CC_ERR_BAD_ARG, "the relaxed mode needs a group (cc_comm_init_*)");
    h->relaxed_minibatch = minibatch_points;
    return CC_OK;
}

int cc_get_relaxed_stats(cc_handle* h, cc_relaxed_stats* out)
{
    if (!h || !out) return CC_ERR_BAD_ARG;
    *out = h->rstats;
    return CC_OK;
}

int cc_set_shard_thresholds(cc_handle* h, int64_t min_row_dims, int32_t offline_min_rows)
{
    if (!h) return CC_ERR_BAD_ARG;
    if (min_row_dims >= 0) { h->shard_min_row_dims = min_row_dims; h->shard_min_row_dims_pruned = 0; }  // (one threshold for both kinds of scan)
    if (offline_min_rows >= 0) h->offline_shard_min_rows = offline_min_rows;
    return CC_OK;
}

}  // extern "C"
