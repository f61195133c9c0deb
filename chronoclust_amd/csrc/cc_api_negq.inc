// cc_api_negq.inc — cc_negq_begin / _add_list / _select / _end: an exact order statistic per selected column over the negative
// compensated values of list-mode events, pooled over any number of sources (the kernels and the plan: cc_negq.h).  The events
// stream slab by slab through the handle's upload staging, as a column reduction's do (col_minmax_slabs): the same stage_slab,
// the same refusals (list_check, list_check_xf), CHRONOCLUST_HIP_INGEST_SLAB honoured.  The state (cc_handle::nq) is scratch of
// its own: the resident points, the flag words, the scaler scratch, the counters and a pending prefetch are not touched.
// (included by cc_api.hip, the one translation unit, behind cc_api_ingest.inc)

namespace {

int negq_chunks(int64_t n) { return (int)std::max<int64_t>(1, (n + CC_NEGQ_CHUNK - 1) / CC_NEGQ_CHUNK); }

// k_negq_stage on `st` for the ns records of a slab in device staging (`raw`) that starts at pooled event s0
void negq_stage_launch(hipStream_t st, const void* raw, const ListSrc& v, const int* desc, int64_t ns, int64_t s0, int64_t cap,
                       const int* wmap, double* val)
{
    const int d = v.d;
    cc_list_xf xf{};  // (no transform: m = 0, nothing behind it is read)
    if (v.xf) xf = list_xf_device(v, desc);
    xf.cof = nullptr;  // cofactors are not applied here
    const dim3 grid((unsigned)((ns + CC_INGEST_TILE - 1) / CC_INGEST_TILE), (unsigned)((d + CC_INGEST_TILE - 1) / CC_INGEST_TILE));
    with_list_dtype(v.dtype, [&](auto t) {
        using T = decltype(t);
        with_bools([&](auto W) {
            hipLaunchKernelGGL((k_negq_stage<T, decltype(W)::value>), grid, dim3(256), 0, st, static_cast<const unsigned char*>(raw),
                               v.src_cols, (int)ns, (long long)s0, (long long)cap, d, reinterpret_cast<const cc_list_desc*>(desc), xf,
                               wmap, val);
        }, v.swapped());
    });
}

int negq_add(cc_handle* h, const IngestSrc& src)
{
    cc_handle::NegQ& nq = h->nq;
    const int64_t n = src.n;
    const size_t pb = src.point_bytes(false);
    const int64_t slab = std::min<int64_t>(slab_points(h, pb, CC_UPLOAD_STAGING), tiles_up(n));
    for (int q = 0; q < (n > slab ? 2 : 1); ++q) h->ingest_raw[q].ensure(slab_floats(pb, slab));
    list_desc_upload(h->stream, src.list, h->list_desc);
    std::vector<char> pack;
    int k = 0;
    for (int64_t off = 0; off < n; off += slab, k ^= 1) {
        const int64_t ns = std::min<int64_t>(slab, n - off);
        stage_slab(h->stream, src, off, ns, h->ingest_raw[k].p, pack);
        negq_stage_launch(h->stream, h->ingest_raw[k].p, src.list, h->list_desc.p, ns, nq.n + off, nq.cap, nq.wdev.p, nq.val.p);
    }
    HIPCHK(hipGetLastError());
    sync_stream(h, h->stream);  // (the descriptors and the caller's records have been read)
    nq.n += n;
    return (int)CC_OK;
}

int negq_select(cc_handle* h, double q, int64_t* out_count, double* out_lo, double* out_hi, double* out_frac)
{
    cc_handle::NegQ& nq = h->nq;
    if (nq.nw > 0) {
        const int chunks = negq_chunks(nq.n);
        const dim3 wide((unsigned)chunks, (unsigned)nq.nw), one((unsigned)nq.nw), block(CC_NEGQ_THREADS);
        for (int pass = 0; pass < 8; ++pass) {
            hipLaunchKernelGGL(k_negq_hist, wide, block, 0, h->stream, (const double*)nq.val.p, (long long)nq.cap, (long long)nq.n,
                               (const unsigned long long*)nq.st.p, pass, nq.hist.p, chunks);
            hipLaunchKernelGGL(k_negq_pick, one, block, 0, h->stream, (const unsigned*)nq.hist.p, chunks, pass, q, nq.st.p);
        }
        hipLaunchKernelGGL(k_negq_next, wide, block, 0, h->stream, (const double*)nq.val.p, (long long)nq.cap, (long long)nq.n,
                           (const unsigned long long*)nq.st.p, nq.nxt.p, chunks);
        hipLaunchKernelGGL(k_negq_done, one, block, 0, h->stream, (const unsigned long long*)nq.nxt.p, chunks,
                           (const unsigned long long*)nq.st.p, nq.out.p);
        HIPCHK(hipGetLastError());
    }
    std::vector<unsigned long long> got((size_t)4 * std::max(nq.nw, 1));
    if (nq.nw > 0) HIPCHK(hipMemcpyAsync(got.data(), nq.out.p, (size_t)4 * nq.nw * 8, hipMemcpyDeviceToHost, h->stream));
    sync_stream(h, h->stream);
    for (int c = 0; c < nq.d; ++c) {
        const int w = nq.wmap[c];
        out_count[c] = w < 0 ? -1 : (int64_t)got[(size_t)4 * w];
        unsigned long long word[3] = {0ull, 0ull, 0ull};
        if (w >= 0) memcpy(word, &got[(size_t)4 * w + 1], sizeof word);
        memcpy(out_lo + c, &word[0], 8);
        memcpy(out_hi + c, &word[1], 8);
        memcpy(out_frac + c, &word[2], 8);
    }
    return (int)CC_OK;
}

}  // namespace

extern "C" {

int cc_negq_begin(cc_handle* h, int32_t d, const uint8_t* want, int64_t capacity)
{
    if (!h) return CC_ERR_BAD_ARG;
    if (d <= 0 || d > CC_MAX_DIM) return fail(h, CC_ERR_BAD_ARG, "negative quantiles: d must be in 1.." + std::to_string(CC_MAX_DIM));
    if (capacity < 0) return fail(h, CC_ERR_BAD_ARG, "negative quantiles: capacity must be non-negative");
    return guarded(h, [&]() {
        // a new state beside the old one: an allocation that fails leaves the handle as it was
        cc_handle::NegQ nw;
        nw.d = d;
        nw.cap = capacity;
        nw.wmap.assign((size_t)d, -1);
        for (int c = 0; c < d; ++c)
            if (!want || want[c]) nw.wmap[c] = nw.nw++;
        const size_t rows = (size_t)std::max(nw.nw, 1), chunks = (size_t)negq_chunks(capacity);
        nw.val.ensure(rows * (size_t)capacity);
        nw.hist.ensure(rows * chunks * 256);
        nw.nxt.ensure(rows * chunks);
        nw.st.ensure(rows * CC_NEGQ_STATE);
        nw.out.ensure(rows * 4);
        nw.wdev.ensure((size_t)d);
        HIPCHK(hipMemcpyAsync(nw.wdev.p, nw.wmap.data(), (size_t)d * sizeof(int), hipMemcpyHostToDevice, h->stream));
        sync_stream(h, h->stream);
        nw.open = true;
        h->nq = std::move(nw);
        return (int)CC_OK;
    });
}

int cc_negq_add_list(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf)
{
    if (!h) return CC_ERR_BAD_ARG;
    if (!h->nq.open) return fail(h, CC_ERR_BAD_ARG, "negative quantiles: cc_negq_add_list without cc_negq_begin");
    ListSrc v;
    int rc = list_check(h, lm, false, &v);
    if (rc == CC_OK) rc = list_check_xf(h, xf, &v);
    if (rc != CC_OK) return rc;
    if (v.d != h->nq.d)
        return fail(h, CC_ERR_BAD_ARG, "negative quantiles: the list mode selects " + std::to_string(v.d) + " dimensions, cc_negq_begin was given " +
                                           std::to_string(h->nq.d));
    if (v.n > h->nq.cap - h->nq.n)
        return fail(h, CC_ERR_BAD_ARG, "negative quantiles: " + std::to_string(h->nq.n) + " + " + std::to_string(v.n) +
                                           " events exceed the capacity of " + std::to_string(h->nq.cap));
    if (v.n == 0) return CC_OK;
    return guarded(h, [&]() { return negq_add(h, IngestSrc::of(v)); });
}

int cc_negq_select(cc_handle* h, double q, int64_t* out_count, double* out_lo, double* out_hi, double* out_frac)
{
    if (!h || !out_count || !out_lo || !out_hi || !out_frac) return fail(h, CC_ERR_BAD_ARG, "negative quantiles: an output is null");
    if (!h->nq.open) return fail(h, CC_ERR_BAD_ARG, "negative quantiles: cc_negq_select without cc_negq_begin");
    if (!(q >= 0.0 && q <= 1.0)) return fail(h, CC_ERR_BAD_ARG, "negative quantiles: q must be in [0, 1]");
    return guarded(h, [&]() { return negq_select(h, q, out_count, out_lo, out_hi, out_frac); });
}

int cc_negq_end(cc_handle* h)
{
    if (!h) return CC_ERR_BAD_ARG;
    if (!h->nq.open) return fail(h, CC_ERR_BAD_ARG, "negative quantiles: cc_negq_end without cc_negq_begin");
    return guarded(h, [&]() {
        sync_stream(h, h->stream);
        h->nq = cc_handle::NegQ();
        return (int)CC_OK;
    });
}

}  // extern "C"
