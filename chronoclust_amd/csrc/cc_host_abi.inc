// cc_host_abi.inc - the C-ABI entry points that are plain host code (no handle, no HIP).  Included inside the extern "C"
// block of cc_api.hip (the product) and of tests/host_san/host_abi.cpp (the same text under -fsanitize=address,undefined
// and -fsanitize=thread, g++ only: sanitizers never touch the GPU build).  Needs chronoclust_hip.h, cc_host.h,
// cc_policy.h, cc_batch.h, cc_csv.h.

int cc_shard_rows(int32_t n, int32_t world, int32_t rank, int32_t unit, int32_t* lo, int32_t* hi)
{
    if (n < 0 || world < 1 || rank < 0 || rank >= world || unit < 1 || !lo || !hi) return CC_ERR_BAD_ARG;
    int a = 0, b = 0;
    cc_shard_range(n, world, rank, unit, &a, &b);
    *lo = a;
    *hi = b;
    return CC_OK;
}

int64_t cc_format_points_csv(const double* values, int64_t n, int32_t d, int64_t first_id, const int32_t* label_idx,
                             const char* label_bytes, const int32_t* label_offsets, int32_t n_labels, char* out,
                             int64_t cap)
{
    if (!values || n < 0 || d < 0 || !label_idx || !label_bytes || !label_offsets || n_labels < 1 || !out) return CC_ERR_BAD_ARG;
    char* o = out;
    char* const end = out + cap;
    int max_label = 0;
    for (int i = 0; i < n_labels; ++i) max_label = std::max(max_label, label_offsets[i + 1] - label_offsets[i]);
    const int64_t row_max = 24 + 1 + max_label + (int64_t)d * 33 + 2;
    for (int64_t r = 0; r < n; ++r) {
        if (end - o < row_max) return CC_ERR_OOM;  // the caller's buffer is too small
        o += cc::format_i64(first_id + r, o);
        *o++ = ',';
        int li = label_idx[r];
        if (li < 0 || li >= n_labels) li = n_labels - 1;  // (-1: the last entry, "None")
        const int ll = label_offsets[li + 1] - label_offsets[li];
        memcpy(o, label_bytes + label_offsets[li], (size_t)ll);
        o += ll;
        const double* v = values + r * d;
        for (int i = 0; i < d; ++i) {
            *o++ = ',';
            if (v[i] == v[i]) o += cc::format_repr(v[i], o);  // (NaN: an empty field, DataFrame.to_csv's na_rep)
        }
        *o++ = '\n';
    }
    return (int64_t)(o - out);
}

int cc_policy_replay(const cc_policy_config* cfg, cc_policy_carry* carry, int64_t start_cursor, int32_t start_rows,
                     const cc_policy_obs* obs, int32_t n, cc_policy_decision* out)
{
    if (!cfg || !carry || n < 0 || (n > 0 && !obs) || !out) return CC_ERR_BAD_ARG;
    cc::WindowPolicy policy(*cfg, *carry);
    out[0] = policy.start(start_cursor, start_rows);
    for (int i = 0; i < n; ++i)
        out[i + 1] = obs[i].after_sequential ? policy.after_sequential(obs[i].cursor, obs[i].m_rows) : policy.after_batch(obs[i]);
    *carry = policy.carry();
    return CC_OK;
}

double cc_policy_seq_rate_guess(int32_t d, int32_t m_rows, int32_t allow_seq_r, int32_t allow_seq_g)
{
    if (d < 1 || d > CC_MAX_DIM || m_rows < 0) return -1.0;
    const int seq_cap = d > CC_WINDOW_MAX_DIM ? 0 : cc_seq_cap_rows(d);
    return cc::seq_rate_guess(d, m_rows, seq_cap, allow_seq_r != 0, allow_seq_g != 0);
}

int cc_seq_handover_replay(int32_t mode, int32_t possible, int32_t sticky, const cc_seq_event* ev, int32_t n, int32_t* outcome,
                           int64_t* stint_len)
{
    if (mode < 0 || mode > 2 || n < 0 || (n > 0 && !ev) || !outcome || !stint_len) return CC_ERR_BAD_ARG;
    cc::SeqHandover rule;
    outcome[0] = rule.start(mode, possible != 0, sticky != 0) ? 1 : 0;
    stint_len[0] = rule.stint_len();
    for (int i = 0; i < n; ++i) {
        const cc_seq_event& e = ev[i];
        outcome[i + 1] = e.chunk_event
                             ? (int32_t)rule.after_chunk(e.got, e.rate, e.chunk, e.use_g != 0, e.allow_seq_g != 0, e.possible != 0,
                                                         e.more != 0, e.wide != 0)
                             : (rule.after_batch(e.bad != 0, e.rate, e.possible != 0, e.more != 0, e.seq_r_applies != 0, e.rate_guess) ? 1 : 0);
        stint_len[i + 1] = rule.stint_len();
    }
    return CC_OK;
}

int cc_batch_plan(const cc_batch_inputs* in, cc_batch_geometry* out)
{
    if (!in || !out) return CC_ERR_BAD_ARG;
    for (int t : {in->decide_threads, in->chain_threads, in->commit_threads})
        if (t != 64 && t != 128 && t != 256) return CC_ERR_BAD_ARG;
    if (in->window < 1 || in->win_cfg < 0 || in->S_cfg < 1 || in->n_cus < 1 || in->prune_wgs_per_cu < 1 || in->plain_wgs_per_cu < 1 ||
        in->m_rows < 0 || in->long_avg < 0 || in->points_left < 0)
        return CC_ERR_BAD_ARG;
    *out = cc::batch_plan(*in);
    return CC_OK;
}

int cc_scan_width(int32_t d, int32_t filter_on, int32_t k_pow2, int32_t* padded, int32_t* scan_u, int32_t* chain)
{
    if (d < 1 || d > CC_MAX_DIM || !padded || !scan_u || !chain) return CC_ERR_BAD_ARG;
    const cc::ScanWidth w = cc::scan_width(d, filter_on != 0, k_pow2 != 0);
    *padded = w.padded;
    *scan_u = w.scan_u ? 1 : 0;
    *chain = w.chain;
    return CC_OK;
}

