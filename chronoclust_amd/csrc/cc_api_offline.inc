// cc_api_offline.inc — the table in list order, the decay / downgrade pass, the offline phase (pair matrices on the device,
// the breadth-first merge on the host), the export of its clusters, the association tracker's argmin and the per-point
// cluster index.  (included by cc_api.hip, the one translation unit, behind cc_handle.h)

namespace {

struct RowList {
    std::vector<int> pcore, outlier;  // table rows in Python list order
};

// list order = ascending key within a kind
RowList list_order(cc_handle* h, std::vector<int>* kind_out = nullptr, std::vector<int>* key_out = nullptr)
{
    const int m = h->hc.m_rows;
    std::vector<int> kind(m), key(m);
    if (m) {
        HIPCHK(hipMemcpyAsync(kind.data(), h->tab.kind.p, (size_t)m * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(key.data(), h->tab.key.p, (size_t)m * 4, hipMemcpyDeviceToHost, h->stream));
        sync_stream(h, h->stream);
    }
    RowList rl;
    for (int r = 0; r < m; ++r) {
        if (kind[r] == CC_KIND_PCORE) rl.pcore.push_back(r);
        else if (kind[r] == CC_KIND_OUTLIER) rl.outlier.push_back(r);
    }
    auto by_key = [&](int a, int b) { return key[a] < key[b]; };
    std::sort(rl.pcore.begin(), rl.pcore.end(), by_key);
    std::sort(rl.outlier.begin(), rl.outlier.end(), by_key);
    if (kind_out) *kind_out = kind;
    if (key_out) *key_out = key;
    return rl;
}

}  // namespace

extern "C" {

int cc_decay_downgrade(cc_handle* h, double factor)
{
    if (!h) return CC_ERR_BAD_ARG;
    if (!h->have_par) return fail(h, CC_ERR_BAD_ARG, "cc_set_params has not been called");
    return guarded(h, [&]() {
        const int m = h->hc.m_rows, d = h->d;
        if (m == 0) return (int)CC_OK;
        refresh_ctl_params(h);
        const Table tab = h->tab.view();
        hipLaunchKernelGGL(k_decay, dim3((m * d + 255) / 256), dim3(256), 0, h->stream, tab, m, d, factor);
        h->flags.ensure((size_t)m);
        hipLaunchKernelGGL(k_downgrade_flags, dim3((m + 255) / 256), dim3(256), 0, h->stream, tab, m, d,
                           h->hc.beta_mu, h->hc.pi, h->hc.omicron, h->flags.p);
        std::vector<int> flags(m);
        std::vector<long long> id(m), uid(m);
        HIPCHK(hipMemcpyAsync(flags.data(), h->flags.p, (size_t)m * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(id.data(), tab.id, (size_t)m * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(uid.data(), tab.uid, (size_t)m * 8, hipMemcpyDeviceToHost, h->stream));
        RowList rl = list_order(h);  // synchronises the stream

        // hddstream.py:528-537 and :545-549: Python removes from the list it iterates, so the element that
        // slides into the freed position is skipped.  Integer work over the flags only.
        std::vector<int> pl = rl.pcore, ol = rl.outlier;
        std::vector<char> downgraded(m, 0);
        for (size_t i = 0; i < pl.size(); ++i) {
            const int r = pl[i];
            if (flags[r] & 1) {
                downgraded[r] = 1;
                pl.erase(pl.begin() + (long)i);
                ol.push_back(r);
            }
        }
        for (size_t i = 0; i < ol.size(); ++i) {
            if (flags[ol[i]] & 2) ol.erase(ol.begin() + (long)i);
        }
        const int np = (int)pl.size(), no = (int)ol.size(), n = np + no;
        std::vector<int> perm(n), nkind(n), nkey(n);
        std::vector<long long> nid(n);
        for (int i = 0; i < np; ++i) { perm[i] = pl[i]; nkind[i] = CC_KIND_PCORE; nkey[i] = i; nid[i] = id[pl[i]]; }
        for (int i = 0; i < no; ++i) {
            const int r = ol[i];
            perm[np + i] = r; nkind[np + i] = CC_KIND_OUTLIER; nkey[np + i] = i;
            nid[np + i] = downgraded[r] ? uid[r] : id[r];  // hddstream.py:535
        }
        if (h->tab2.cap < h->tab.cap || h->tab2.d != d) {
            h->tab2.alloc(h->tab.cap, d);
            // stamps are compared with atomic max: fresh memory must not hold anything that looks newer
            HIPCHK(hipMemsetAsync(h->tab2.touch.p, 0, 2 * h->tab2.cap * 8, h->stream));
            HIPCHK(hipMemsetAsync(h->tab2.last.p, 0, 2 * h->tab2.cap * 8, h->stream));
            HIPCHK(hipMemsetAsync(h->tab2.carry_of.p, 0, h->tab2.cap * 8, h->stream));
            HIPCHK(hipMemsetAsync(h->tab2.cnt.p, 0, h->tab2.cap * 8, h->stream));
        }
        DevBuf<int> dperm, dkind, dkey;
        DevBuf<long long> dnid;
        dperm.ensure(n); dkind.ensure(n); dkey.ensure(n); dnid.ensure(n);
        if (n) {
            HIPCHK(hipMemcpyAsync(dperm.p, perm.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(dkind.p, nkind.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(dkey.p, nkey.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(dnid.p, nid.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
            hipLaunchKernelGGL(k_gather_rows, dim3((n * d + 255) / 256), dim3(256), 0, h->stream, tab, h->tab2.view(),
                               dperm.p, dkind.p, dkey.p, dnid.p, n, d);
        }
        sync_stream(h, h->stream);
        std::swap(h->tab, h->tab2);
        h->hc.m_rows = n;
        h->hc.n_pkeys = np;
        h->hc.n_okeys = no;
        push_ctl(h);
        sync_stream(h, h->stream);
        return (int)CC_OK;
    });
}

int cc_offline(cc_handle* h, int32_t* n_clusters, int8_t* out_core, int32_t* out_pdim, int32_t* out_nn,
               int32_t* out_nw)
{
    if (!h) return CC_ERR_BAD_ARG;
    if (!h->have_par) return fail(h, CC_ERR_BAD_ARG, "cc_set_params has not been called");
    return guarded(h, [&]() {
        refresh_ctl_params(h);
        h->clusters.clear();
        h->pcore_ids_host.clear();
        h->pcore_uid_host.clear();
        h->n_core = 0;
        if (n_clusters) *n_clusters = 0;
        // (CHRONOCLUST_HIP_TRACE=1: host wall time per phase of the call)
        auto now_us = []() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        double tph[8] = {now_us(), 0, 0, 0, 0, 0, 0, 0};
        // the pcore rows in list order (ascending key), from page-locked copies of the kind / key columns; creation numbers
        // of all rows beside them (cc_point_clusters joins the per-point labels to the clusters through the pcores')
        const int m_all = h->hc.m_rows;
        h->pin.reset();
        h->pin.reserve((size_t)m_all * 72 + ((size_t)1 << 16));  // (everything below but the neighbour lists: 49 B per row)
        std::vector<int> prow_host;
        const long long* uid_all = nullptr;
        if (m_all > 0) {
            int* kind = h->pin.take<int>((size_t)m_all);
            int* key = h->pin.take<int>((size_t)m_all);
            long long* uid = h->pin.take<long long>((size_t)m_all);
            HIPCHK(hipMemcpyAsync(kind, h->tab.kind.p, (size_t)m_all * 4, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipMemcpyAsync(key, h->tab.key.p, (size_t)m_all * 4, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipMemcpyAsync(uid, h->tab.uid.p, (size_t)m_all * 8, hipMemcpyDeviceToHost, h->stream));
            sync_stream(h, h->stream);
            uid_all = uid;
            std::vector<unsigned long long> order;  // (key, row) packed: one plain sort, no indirection
            order.reserve((size_t)m_all);
            for (int r = 0; r < m_all; ++r)
                if (kind[r] == CC_KIND_PCORE) order.push_back(((unsigned long long)((unsigned)key[r] ^ 0x80000000u) << 32) | (unsigned)r);  // (signed order)
            std::sort(order.begin(), order.end());
            prow_host.resize(order.size());
            for (size_t i = 0; i < order.size(); ++i) prow_host[i] = (int)(order[i] & 0xFFFFFFFFull);
        }
        tph[1] = now_us();
        const int mp = (int)prow_host.size(), d = h->d;
        if (mp == 0) return (int)CC_OK;
        const size_t md = (size_t)mp * d;
        const int words = (mp + 63) / 64;
        // Multi-GPU: a rank evaluates a block of p rows (whole 64-row blocks) of the M x M pair matrices and the ranks
        // all-gather what the ordered expansion needs of them: subspace preference vectors, neighbour counts, the
        // weighted-reachability bitmask.  The eps-neighbour bitmask stays local (a row is only read by its owner).
        const int world = h->comm.world, rank = h->comm.rank;
        const bool shard = h->comm.active() && mp >= h->offline_shard_min_rows;
        const int share = shard ? cc_shard_share(mp, world, 64) : words * 64;  // p rows per rank
        const size_t rows_pad = shard ? (size_t)share * world : (size_t)mp;     // buffers hold every rank's block
        int p_lo = 0, p_hi = mp;
        if (shard) cc_shard_range(mp, world, rank, 64, &p_lo, &p_hi);
        h->pv_cf1.ensure(md); h->pv_cf2.ensure(md); h->pv_cen.ensure(md); h->pv_pref.ensure(md); h->pv_w.ensure(mp);
        h->pv_id.ensure(mp); h->prow.ensure(mp); h->wvec.ensure(rows_pad * d); h->nn.ensure(rows_pad); h->pdim.ensure(mp);
        h->core.ensure(mp); h->adj.ensure(rows_pad * words); h->adjw.ensure(rows_pad * words);
        int* const prow_pin = h->pin.take<int>((size_t)mp);
        memcpy(prow_pin, prow_host.data(), (size_t)mp * 4);
        HIPCHK(hipMemcpyAsync(h->prow.p, prow_pin, (size_t)mp * 4, hipMemcpyHostToDevice, h->stream));
        PcoreView pv{h->pv_cf1.p, h->pv_cf2.p, h->pv_cen.p, h->pv_pref.p, h->pv_w.p, h->pv_id.p};
        const Ctl& c = h->hc;
        const cc_params& p = h->par;
        hipLaunchKernelGGL(k_gather_pcores, dim3((unsigned)((md + 255) / 256)), dim3(256), 0, h->stream, h->tab.view(),
                           pv, h->prow.p, mp, d);
        hipLaunchKernelGGL(k_core_flags, dim3((mp + 255) / 256), dim3(256), 0, h->stream, pv, mp, d, p.eps_sq, p.mu,
                           p.pi, p.k, c.inv_k, c.pow2, h->core.p);
        const int my_rows = p_hi - p_lo;
        if (my_rows > 0) {
            {
                // p rows per workgroup: CC_EPS_PCH on large tables; a table of a few thousand rows would be a few hundred
                // workgroups of one wave per SIMD each (5 000 rows: 400 workgroups, 141 us for 46 us of arithmetic) - whole
                // staging passes (CC_EPS_TP rows), at least ~8 workgroups per CU
                int pch = CC_EPS_PCH;
                while (pch > CC_EPS_TP && (long long)((words + 3) / 4) * ((my_rows + pch - 1) / pch) < 8ll * h->n_cus) pch /= 2;
                const dim3 grid((words + 3) / 4, (my_rows + pch - 1) / pch), block(256);
#define CC_EPS(DP) hipLaunchKernelGGL((k_eps_neighbours<DP>), grid, block, 0, h->stream, pv.cen, mp, d, p.ups_eps, h->adj.p, words, p_lo, p_hi, pch)
                if (d <= 4) CC_EPS(4);
                else if (d <= 8) CC_EPS(8);
                else if (d <= 16) CC_EPS(16);
                else if (d <= 20) CC_EPS(20);
                else if (d <= 24) CC_EPS(24);
                else if (d <= 40) CC_EPS(40);
                else if (d <= 64) CC_EPS(64);
                else if (d <= 128) CC_EPS(128);
                else hipLaunchKernelGGL(k_eps_neighbours_blk, grid, block, 0, h->stream, pv.cen, mp, d, p.ups_eps, h->adj.p, words,
                                        p_lo, p_hi, pch);
#undef CC_EPS
            }
            hipLaunchKernelGGL(k_subspace_pref, dim3((unsigned)(((size_t)my_rows * d + 255) / 256)), dim3(256), 0, h->stream,
                               pv.cen, h->adj.p, words, mp, d, p.delta, p.k, h->wvec.p, h->nn.p, p_lo, p_hi);
        }
        if (shard) {
            // in place: rank r's block sits at r * share rows of the same buffer on every rank
            h->comm.all_gather(h->wvec.p + (size_t)rank * share * d, h->wvec.p, (size_t)share * d * 8, h->stream);
            h->comm.all_gather(h->nn.p + (size_t)rank * share, h->nn.p, (size_t)share * 4, h->stream);
        }
        hipLaunchKernelGGL(k_pdim, dim3((mp + 255) / 256), dim3(256), 0, h->stream, h->wvec.p, mp, d, h->pdim.p);
        if (my_rows > 0)
            hipLaunchKernelGGL(k_weighted_reach, dim3(my_rows), dim3(64), 0, h->stream, pv.cen, h->wvec.p, h->adj.p,
                               h->adjw.p, words, mp, d, p.ups_eps_sq, p_lo, p_hi);
        if (shard)
            h->comm.all_gather(h->adjw.p + (size_t)rank * share * words, h->adjw.p, (size_t)share * words * 8, h->stream);
        // the reachability rows as neighbour lists: counts -> offsets (host prefix sums) -> ascending positions
        h->nw_cnt.ensure(mp);
        hipLaunchKernelGGL(k_adj_counts, dim3(mp), dim3(64), 0, h->stream, h->adjw.p, words, mp, h->nw_cnt.p);
        h->pcore_uid_host.resize(mp);
        for (int i = 0; i < mp; ++i) h->pcore_uid_host[(size_t)i] = uid_all[(size_t)prow_host[(size_t)i]];
        int8_t* const core = h->pin.take<int8_t>((size_t)mp);
        int* const pdim = h->pin.take<int>((size_t)mp);
        int* const nn = h->pin.take<int>((size_t)mp);
        int* const nw_cnt = h->pin.take<int>((size_t)mp);
        long long* const ids_pin = h->pin.take<long long>((size_t)mp);
        long long* const nw_off = h->pin.take<long long>((size_t)mp + 1);
        HIPCHK(hipMemcpyAsync(core, h->core.p, mp, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(pdim, h->pdim.p, (size_t)mp * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(nn, h->nn.p, (size_t)mp * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(nw_cnt, h->nw_cnt.p, (size_t)mp * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(ids_pin, h->pv_id.p, (size_t)mp * 8, hipMemcpyDeviceToHost, h->stream));
        sync_stream(h, h->stream);
        HIPCHK(hipGetLastError());
        h->pcore_ids_host.assign(ids_pin, ids_pin + mp);
        tph[2] = now_us();
        nw_off[0] = 0;
        for (int i = 0; i < mp; ++i) nw_off[(size_t)i + 1] = nw_off[i] + nw_cnt[i];
        const long long n_edges = nw_off[mp];
        // (the lists go into a block of their own: the first one must stay where it is)
        std::vector<int> nbr_pageable;
        const int* nbr = nullptr;
        if (n_edges > 0) {
            h->nw_off.ensure((size_t)mp + 1);
            h->nw_nbr.ensure((size_t)n_edges);
            HIPCHK(hipMemcpyAsync(h->nw_off.p, nw_off, ((size_t)mp + 1) * 8, hipMemcpyHostToDevice, h->stream));
            hipLaunchKernelGGL(k_adj_fill, dim3(mp), dim3(64), 0, h->stream, h->adjw.p, words, mp, h->nw_off.p, h->nw_nbr.p);
            int* dst;
            if (h->pin.used + (size_t)n_edges * 4 + 128 <= h->pin.cap) dst = h->pin.take<int>((size_t)n_edges);
            else {  // (dense neighbourhoods: more edges than the scratch was sized for)
                nbr_pageable.resize((size_t)n_edges);
                dst = nbr_pageable.data();
            }
            HIPCHK(hipMemcpyAsync(dst, h->nw_nbr.p, (size_t)n_edges * 4, hipMemcpyDeviceToHost, h->stream));
            sync_stream(h, h->stream);
            HIPCHK(hipGetLastError());
            nbr = dst;
        }

        tph[3] = now_us();
        // ---- ordered expansion on the host: predecon.py:62-120, 242-267 (integer / graph work only) ----
        auto for_each_nw = [&](int q, auto&& fn) {  // the weighted neighbours of q in ascending (= dict) order
            for (long long e = nw_off[q]; e < nw_off[(size_t)q + 1]; ++e) fn(nbr[(size_t)e]);
        };
        std::vector<int8_t> cls(mp, 0);  // 0 'u', 1 'c', 2 'n'
        std::vector<int> queue;
        h->clusters.mem.reserve((size_t)mp);
        h->clusters.off.reserve((size_t)mp + 1);
        const int lam = p.pi;
        for (int seed = 0; seed < mp; ++seed) {
            if (cls[seed] != 0) continue;
            if (!core[seed]) { cls[seed] = 2; continue; }
            const size_t cl_begin = h->clusters.mem.size();
            queue.clear();
            for_each_nw(seed, [&](int x) { queue.push_back(x); });
            size_t head = 0;
            while (head < queue.size()) {
                const int q = queue[head++];
                if (!core[q]) continue;
                for_each_nw(q, [&](int x) {
                    if (pdim[x] > lam) return;
                    if (cls[x] == 0) queue.push_back(x);
                    if (cls[x] == 0 || cls[x] == 2) {
                        cls[x] = 1;
                        h->clusters.mem.push_back(x);
                    }
                });
            }
            if (h->clusters.mem.size() > cl_begin) h->clusters.off.push_back((int)h->clusters.mem.size());  // predecon.py:83 (W > 0)
        }
        for (int i = 0; i < mp; ++i) h->n_core += core[i];

        tph[4] = now_us();
        // ---- cluster CF sums in merge order + preferred dimensions on the device ----
        const int nc = (int)h->clusters.size();
        if (nc) {
            const std::vector<int>&mem = h->clusters.mem, &off = h->clusters.off;
            const size_t cd = (size_t)nc * d;
            h->mem_dev.ensure(mem.size()); h->off_dev.ensure(off.size());
            h->c_cf1.ensure(cd); h->c_cf2.ensure(cd); h->c_cen.ensure(cd); h->c_pref.ensure(cd); h->c_w.ensure(nc);
            HIPCHK(hipMemcpyAsync(h->mem_dev.p, mem.data(), mem.size() * 4, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(h->off_dev.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, h->stream));
            hipLaunchKernelGGL(k_cluster_merge, dim3((unsigned)((cd + 255) / 256)), dim3(256), 0, h->stream, pv,
                               h->mem_dev.p, h->off_dev.p, nc, d, p.delta_sq, p.k, h->c_cf1.p, h->c_cf2.p, h->c_cen.p,
                               h->c_pref.p, h->c_w.p);
            sync_stream(h, h->stream);
        }
        tph[5] = now_us();
        if (h->trace)
            fprintf(stderr, "[cc] offline phase, host wall time: list order %.0f us, pair kernels + read-back %.0f, neighbour lists %.0f, "
                    "ordered expansion %.0f, cluster sums %.0f (%d pcores, %d clusters)\n", tph[1] - tph[0], tph[2] - tph[1], tph[3] - tph[2],
                    tph[4] - tph[3], tph[5] - tph[4], mp, nc);
        if (out_core) memcpy(out_core, core, mp);
        if (out_pdim) memcpy(out_pdim, pdim, (size_t)mp * 4);
        if (out_nn) memcpy(out_nn, nn, (size_t)mp * 4);
        if (out_nw) memcpy(out_nw, nw_cnt, (size_t)mp * 4);
        if (n_clusters) *n_clusters = nc;
        return (int)CC_OK;
    });
}

int cc_num_core(cc_handle* h) { return h ? h->n_core : CC_ERR_BAD_ARG; }

int cc_cluster_size(cc_handle* h, int32_t c)
{
    if (!h || c < 0 || c >= (int)h->clusters.size()) return CC_ERR_BAD_ARG;
    return h->clusters.off[(size_t)c + 1] - h->clusters.off[(size_t)c];
}

int cc_cluster_export(cc_handle* h, int32_t c, int64_t* members, double* w, double* cf1, double* cf2, double* cen,
                      double* pref)
{
    if (!h || c < 0 || c >= (int)h->clusters.size()) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() {
        const size_t d = (size_t)h->d;
        const int a = h->clusters.off[(size_t)c], e = h->clusters.off[(size_t)c + 1];
        if (members)
            for (int i = a; i < e; ++i) members[i - a] = h->pcore_ids_host[(size_t)h->clusters.mem[(size_t)i]];
        if (w) HIPCHK(hipMemcpyAsync(w, h->c_w.p + c, 8, hipMemcpyDeviceToHost, h->stream));
        if (cf1) HIPCHK(hipMemcpyAsync(cf1, h->c_cf1.p + (size_t)c * d, d * 8, hipMemcpyDeviceToHost, h->stream));
        if (cf2) HIPCHK(hipMemcpyAsync(cf2, h->c_cf2.p + (size_t)c * d, d * 8, hipMemcpyDeviceToHost, h->stream));
        if (cen) HIPCHK(hipMemcpyAsync(cen, h->c_cen.p + (size_t)c * d, d * 8, hipMemcpyDeviceToHost, h->stream));
        if (pref) HIPCHK(hipMemcpyAsync(pref, h->c_pref.p + (size_t)c * d, d * 8, hipMemcpyDeviceToHost, h->stream));
        sync_stream(h, h->stream);
        return (int)CC_OK;
    });
}

int cc_clusters_total_members(cc_handle* h)
{
    if (!h) return CC_ERR_BAD_ARG;
    size_t tot = 0;
    tot = h->clusters.mem.size();
    return (int)tot;
}

int cc_clusters_export(cc_handle* h, int64_t* members, int32_t* offsets, double* w, double* cf1, double* cf2,
                       double* cen, double* pref)
{
    if (!h) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() {
        const size_t nc = h->clusters.size(), d = (size_t)h->d;
        const size_t tot = h->clusters.mem.size();
        if (offsets)
            for (size_t c = 0; c <= nc; ++c) offsets[c] = (int32_t)h->clusters.off[c];
        if (members)
            for (size_t i = 0; i < tot; ++i) members[i] = h->pcore_ids_host[(size_t)h->clusters.mem[i]];
        if (nc == 0) return (int)CC_OK;
        if (w) HIPCHK(hipMemcpyAsync(w, h->c_w.p, nc * 8, hipMemcpyDeviceToHost, h->stream));
        if (cf1) HIPCHK(hipMemcpyAsync(cf1, h->c_cf1.p, nc * d * 8, hipMemcpyDeviceToHost, h->stream));
        if (cf2) HIPCHK(hipMemcpyAsync(cf2, h->c_cf2.p, nc * d * 8, hipMemcpyDeviceToHost, h->stream));
        if (cen) HIPCHK(hipMemcpyAsync(cen, h->c_cen.p, nc * d * 8, hipMemcpyDeviceToHost, h->stream));
        if (pref) HIPCHK(hipMemcpyAsync(pref, h->c_pref.p, nc * d * 8, hipMemcpyDeviceToHost, h->stream));
        sync_stream(h, h->stream);
        return (int)CC_OK;
    });
}

int cc_assoc_argmin(cc_handle* h, const double* cur_cen, const double* cur_pref, int32_t mc, const double* prev_cen,
                    int32_t mp, int32_t d, int32_t* out_idx, double* out_dist)
{
    if (!h || !cur_cen || !cur_pref || !out_idx || mc < 0 || mp < 0 || d <= 0) return CC_ERR_BAD_ARG;
    if (mp > 0 && !prev_cen) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() {
        if (mc == 0) return (int)CC_OK;
        const size_t cd = (size_t)mc * d, pd = (size_t)mp * d;
        // multi-GPU: a rank takes a block of current pcores; indices and distances are all-gathered
        const int world = h->comm.world, rank = h->comm.rank;
        const bool shard = h->comm.active() && mc >= h->offline_shard_min_rows;
        const int share = shard ? cc_shard_share(mc, world, 1) : mc;
        int c_lo = 0, c_hi = mc;
        if (shard) cc_shard_range(mc, world, rank, 1, &c_lo, &c_hi);
        h->a_cur_cen.ensure(cd); h->a_cur_pref.ensure(cd); h->a_prev_cen.ensure(pd);
        h->a_idx.ensure(shard ? (size_t)share * world : (size_t)mc);
        h->a_dist.ensure(shard ? (size_t)share * world : (size_t)mc);
        // the distance operand per (current pcore, dim): 1 or 1/k when every preference entry is 1 or k and k is a power
        // of two (x / k == x * (1/k) bit for bit), else the preference entry itself (the kernel divides)
        const double k = h->have_par ? h->par.k : 1.0;
        bool unit = is_pow2(k);
        for (size_t i = 0; unit && i < cd; ++i) unit = cur_pref[i] == 1.0 || cur_pref[i] == k;
        std::vector<double> op(cd);
        const double inv_k = unit ? 1.0 / k : 0.0;
        for (size_t i = 0; i < cd; ++i) op[i] = unit ? (cur_pref[i] == 1.0 ? 1.0 : inv_k) : cur_pref[i];
        HIPCHK(hipMemcpyAsync(h->a_cur_cen.p, cur_cen, cd * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->a_cur_pref.p, op.data(), cd * 8, hipMemcpyHostToDevice, h->stream));
        if (pd) HIPCHK(hipMemcpyAsync(h->a_prev_cen.p, prev_cen, pd * 8, hipMemcpyHostToDevice, h->stream));
        if (c_hi > c_lo && mp > 0) {
            const int ctiles = (c_hi - c_lo + 255) / 256;  // workgroups of 4 x 64 current pcores
            // previous pcores in S sub-ranges so that the launch fills the machine (>= ~1024 workgroups)
            const int S = std::max(1, std::min((mp + CC_ASSOC_TQ - 1) / CC_ASSOC_TQ, (1024 + ctiles - 1) / ctiles));
            h->a_pdist.ensure((size_t)S * mc);
            h->a_pidx.ensure((size_t)S * mc);
            const dim3 grid(ctiles, S), block(256);
            // k_assoc_tiled over the padded dimensionality (beyond 128: in blocks), `unit` as a template flag
            auto assoc = [&](auto DP) {
                with_bools([&](auto UNIT) {
                    hipLaunchKernelGGL((k_assoc_tiled<decltype(DP)::value, decltype(UNIT)::value>), grid, block, 0, h->stream,
                                       h->a_cur_cen.p, h->a_cur_pref.p, h->a_prev_cen.p, mc, mp, d, c_lo, c_hi, h->a_pdist.p, h->a_pidx.p);
                }, unit);
            };
            if (d <= 4) assoc(std::integral_constant<int, 4>{});
            else if (d <= 8) assoc(std::integral_constant<int, 8>{});
            else if (d <= 16) assoc(std::integral_constant<int, 16>{});
            else if (d <= 24) assoc(std::integral_constant<int, 24>{});
            else if (d <= 40) assoc(std::integral_constant<int, 40>{});
            else if (d <= 64) assoc(std::integral_constant<int, 64>{});
            else if (d <= 128) assoc(std::integral_constant<int, 128>{});
            else
                with_bools([&](auto UNIT) {
                    hipLaunchKernelGGL((k_assoc_tiled_blk<decltype(UNIT)::value>), grid, block, 0, h->stream, h->a_cur_cen.p,
                                       h->a_cur_pref.p, h->a_prev_cen.p, mc, mp, d, c_lo, c_hi, h->a_pdist.p, h->a_pidx.p);
                }, unit);
            hipLaunchKernelGGL(k_assoc_merge, dim3((c_hi - c_lo + 255) / 256), dim3(256), 0, h->stream, h->a_pdist.p,
                               h->a_pidx.p, S, mc, c_lo, c_hi, h->a_idx.p, h->a_dist.p);
        } else if (c_hi > c_lo) {
            // no previous pcores: index -1, distance +inf (what the argmin kernel starts from)
            HIPCHK(hipMemsetAsync(h->a_idx.p + c_lo, 0xFF, (size_t)(c_hi - c_lo) * 4, h->stream));
            const std::vector<double> inf((size_t)(c_hi - c_lo), std::numeric_limits<double>::infinity());
            HIPCHK(hipMemcpyAsync(h->a_dist.p + c_lo, inf.data(), inf.size() * 8, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));  // (`inf` is a local)
        }
        if (shard) {
            h->comm.all_gather(h->a_idx.p + (size_t)rank * share, h->a_idx.p, (size_t)share * 4, h->stream);
            h->comm.all_gather(h->a_dist.p + (size_t)rank * share, h->a_dist.p, (size_t)share * 8, h->stream);
        }
        HIPCHK(hipMemcpyAsync(out_idx, h->a_idx.p, (size_t)mc * 4, hipMemcpyDeviceToHost, h->stream));
        if (out_dist) HIPCHK(hipMemcpyAsync(out_dist, h->a_dist.p, (size_t)mc * 8, hipMemcpyDeviceToHost, h->stream));
        sync_stream(h, h->stream);
        HIPCHK(hipGetLastError());
        return (int)CC_OK;
    });
}

// ---- per-point output: cluster index of every point (device), text of the per-point file (host) ----------

int cc_point_clusters(cc_handle* h, int32_t* out_idx)
{
    if (!h || !out_idx) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() {
        const long long n = h->n_points;
        if (n == 0) return (int)CC_OK;
        // creation number -> cluster index, for the pcores the last cc_offline put into clusters (everything else,
        // outlier microclusters included: -1), built from the merge lists and uploaded as one dense table
        const long long n_uid = h->hc.outlier_last_id;
        std::vector<int32_t> map((size_t)std::max<long long>(n_uid, 1), -1);
        for (size_t c = 0; c < h->clusters.size(); ++c)
            for (int i = h->clusters.off[c]; i < h->clusters.off[c + 1]; ++i) {
                const long long u = h->pcore_uid_host[(size_t)h->clusters.mem[(size_t)i]];
                if (u >= 0 && u < n_uid) map[(size_t)u] = (int32_t)c;
            }
        h->pc_map.ensure(map.size());
        h->pc_out.ensure((size_t)n);
        HIPCHK(hipMemcpyAsync(h->pc_map.p, map.data(), map.size() * 4, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_point_clusters, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->lab_uid.p, n,
                           h->pc_map.p, n_uid, h->pc_out.p);
        HIPCHK(hipMemcpyAsync(out_idx, h->pc_out.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
        sync_stream(h, h->stream);  // (`map` is a local)
        HIPCHK(hipGetLastError());
        return (int)CC_OK;
    });
}

}  // extern "C"
