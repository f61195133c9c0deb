// cc_api_list.inc — the `_list` entry points: list-mode event records (cc_list_mode: the DATA segment of an FCS file) to the
// device as the bytes they hold.  Whole records travel in slabs through the staging buffers of the `_f32` route - byte copies,
// no packing pass on the host whatever src_cols / d is - and k_ingest_list (cc_ingest_list.h) swaps, gathers the selected
// channels, masks, widens, scales, checks and writes both resident copies; cc_col_minmax_list reduces the same slabs.
// cc_assign_list is in cc_api_assign.inc.  (included by cc_api.hip, the one translation unit, behind cc_api_views.inc)

namespace {

// a checked cc_list_mode: the descriptors with their defaults filled in
struct ListSrc {
    const char* data = nullptr;
    int64_t n = 0;
    int src_cols = 0, dtype = 0, sz = 0, flags = 0, d = 0;
    std::vector<cc_list_desc> desc;  // d of them
    bool swapped() const { return (flags & CC_LM_SWAPPED) != 0; }
    size_t record_bytes() const { return (size_t)src_cols * (size_t)sz; }
    const char* at(int64_t r) const { return data + (size_t)r * record_bytes(); }
};

bool same_desc(const std::vector<cc_list_desc>& a, const std::vector<cc_list_desc>& b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].col != b[i].col || a[i].mask != b[i].mask) return false;
    return true;
}

// f(T{}) for the element type of a list-mode dtype code (checked before: list_check)
template <typename F>
void with_list_dtype(int dtype, F&& f)
{
    switch (dtype) {
    case CC_DT_F64: f(double{}); break;
    case CC_DT_F32: f(float{}); break;
    case CC_DT_U8: f(uint8_t{}); break;
    case CC_DT_U16: f(uint16_t{}); break;
    default: f(uint32_t{}); break;
    }
}

// The descriptor's refusals, before anything is read, launched or allocated.  `need_points`: n = 0 is refused too.
int list_check(cc_handle* h, const cc_list_mode* lm, bool need_points, ListSrc* out)
{
    if (!h) return CC_ERR_BAD_ARG;
    if (!lm) return fail(h, CC_ERR_BAD_ARG, "list mode: the descriptor is null");
    if (lm->n < 0 || (need_points && lm->n == 0))
        return fail(h, CC_ERR_BAD_ARG, "list mode: n must be " + std::string(need_points ? "positive" : "non-negative"));
    if (!lm->data) return fail(h, CC_ERR_BAD_ARG, "list mode: data is null");
    if (lm->d <= 0 || lm->d > CC_MAX_DIM) return fail(h, CC_ERR_BAD_ARG, "list mode: d must be in 1.." + std::to_string(CC_MAX_DIM));
    if (lm->src_cols <= 0 || lm->src_cols > CC_MAX_SRC_COLS)
        return fail(h, CC_ERR_BAD_ARG, "list mode: src_cols must be in 1.." + std::to_string(CC_MAX_SRC_COLS));
    const bool floating = lm->dtype == CC_DT_F32 || lm->dtype == CC_DT_F64;
    if (!floating && lm->dtype != CC_DT_U8 && lm->dtype != CC_DT_U16 && lm->dtype != CC_DT_U32)
        return fail(h, CC_ERR_BAD_ARG, "list mode: dtype " + std::to_string(lm->dtype) + " is none of F32, F64, U8, U16, U32");
    if (lm->flags & ~(int32_t)CC_LM_SWAPPED) return fail(h, CC_ERR_BAD_ARG, "list mode: unknown flag bits " + std::to_string(lm->flags));
    if (lm->masks && floating) return fail(h, CC_ERR_BAD_ARG, "list mode: masks are for the integer dtypes only");
    if (!lm->cols && lm->d > lm->src_cols)
        return fail(h, CC_ERR_BAD_ARG, "list mode: column " + std::to_string(lm->src_cols) + " (no column list: 0 .. d - 1) is outside 0.." +
                                           std::to_string(lm->src_cols - 1));
    for (int i = 0; lm->cols && i < lm->d; ++i)
        if (lm->cols[i] < 0 || lm->cols[i] >= lm->src_cols)
            return fail(h, CC_ERR_BAD_ARG, "list mode: column " + std::to_string(lm->cols[i]) + " (entry " + std::to_string(i) +
                                               ") is outside 0.." + std::to_string(lm->src_cols - 1));
    const int sz = dtype_size(lm->dtype);
    if (lm->n > std::numeric_limits<int64_t>::max() / ((int64_t)lm->src_cols * sz))
        return fail(h, CC_ERR_BAD_ARG, "list mode: the extent overflows int64");
    out->data = static_cast<const char*>(lm->data);
    out->n = lm->n; out->src_cols = lm->src_cols; out->dtype = lm->dtype; out->sz = sz; out->flags = lm->flags; out->d = lm->d;
    out->desc.resize((size_t)lm->d);
    for (int i = 0; i < lm->d; ++i) {
        out->desc[i].col = lm->cols ? lm->cols[i] : i;
        out->desc[i].mask = lm->masks ? lm->masks[i] : 0xFFFFFFFFu;
    }
    return (int)CC_OK;
}

// Events per slab in a staging buffer of `cap_bytes`: whole 64-point tiles, at least one; CHRONOCLUST_HIP_INGEST_SLAB
// shortens it.  (At most 32 KiB a record: 4 096 elements of 8 bytes.)
int64_t list_slab_points(const cc_handle* h, const ListSrc& v, size_t cap_bytes)
{
    int64_t pts = (int64_t)(cap_bytes / v.record_bytes()) & ~(int64_t)63;
    if (h->ingest_slab > 0) pts = std::min<int64_t>(pts, ((int64_t)h->ingest_slab + 63) & ~(int64_t)63);
    return std::max<int64_t>(CC_INGEST_TILE, pts);
}
// floats of a DevBuf<float> that hold a slab of `pts` records
size_t list_slab_floats(const ListSrc& v, int64_t pts)
{
    return ((size_t)pts * v.record_bytes() + 3) / 4;
}

// the descriptors to the device on `st` (`v` outlives the stream's next synchronisation)
void list_desc_upload(hipStream_t st, const ListSrc& v, DevBuf<int>& dev)
{
    static_assert(sizeof(cc_list_desc) == 8, "cc_list_desc is two words");
    dev.ensure((size_t)2 * v.d);
    HIPCHK(hipMemcpyAsync(dev.p, v.desc.data(), (size_t)v.d * sizeof(cc_list_desc), hipMemcpyHostToDevice, st));
}

// k_ingest_list on `st` for the ns records of a slab in device staging (`raw`) that starts at event s0 of n_total;
// desc: device; scale / mn: device, or both null
void ingest_list_launch(hipStream_t st, const void* raw, const ListSrc& v, const int* desc, int64_t ns, int64_t s0, int64_t n_total,
                        size_t xt_rows, double* X, double* Xt, const double* scale, const double* mn, int* bad)
{
    const int d = v.d;
    const dim3 grid((unsigned)((ns + CC_INGEST_TILE - 1) / CC_INGEST_TILE), (unsigned)((d + CC_INGEST_TILE - 1) / CC_INGEST_TILE));
    with_list_dtype(v.dtype, [&](auto t) {
        using T = decltype(t);
        with_bools([&](auto W, auto S) {
            hipLaunchKernelGGL((k_ingest_list<T, decltype(W)::value, decltype(S)::value>), grid, dim3(256), 0, st,
                               static_cast<const unsigned char*>(raw), v.src_cols, (int)ns, (long long)s0, (long long)n_total, d,
                               (int)xt_rows, reinterpret_cast<const cc_list_desc*>(desc), X, Xt, scale, mn, bad);
        }, v.swapped(), scale != nullptr);
    });
}

int upload_list(cc_handle* h, const ListSrc& v, const double* scale, const double* mn)
{
    const int64_t n = v.n;
    const int d = v.d;
    int rc = set_dim(h, d);
    if (rc != CC_OK) return rc;
    h->list_points += n;
    if (h->pf.active) {
        // the events may already be on their way (cc_points_prefetch_list): adopt them if it is this very upload
        cc_handle::Prefetch& pf = h->pf;
        bool same = pf.list && pf.x == v.data && pf.n == n && pf.d == d && pf.dtype == v.dtype && pf.src_cols == v.src_cols &&
                    pf.flags == v.flags && same_desc(pf.ldesc, v.desc) && pf.scaled == (scale != nullptr);
        for (int i = 0; same && scale && i < d; ++i) same = pf.scale[i] == scale[i] && pf.mn[i] == mn[i];
        const bool ok = prefetch_join(h);
        pf.active = false;
        if (same && ok) {
            h->X.swap(pf.X);
            h->Xt.swap(pf.Xt);
            h->lab_uid.ensure((size_t)n);
            h->lab_path.ensure((size_t)n);
            h->n_points = n;
            if (pf.bad_host[0]) {
                h->n_points = 0;
                return fail(h, CC_ERR_NONFINITE, "input points contain NaN or Inf");
            }
            h->x_absmax = absmax_of(pf.bad_host);
            return (int)CC_OK;
        }
    }
    h->X.ensure((size_t)n * d);
    h->Xt.ensure((size_t)n * xt_dims(d));
    h->lab_uid.ensure((size_t)n);
    h->lab_path.ensure((size_t)n);
    h->n_points = n;
    if (n == 0) return (int)CC_OK;
    // slab by slab through the two staging buffers, all on the handle's stream: the flag words are cleared once and
    // accumulate over the slabs
    const int64_t slab = std::min<int64_t>(list_slab_points(h, v, (size_t)32 << 20), (n + 63) & ~(int64_t)63);
    for (int q = 0; q < (n > slab ? 2 : 1); ++q) h->ingest_raw[q].ensure(list_slab_floats(v, slab));
    HIPCHK(hipMemsetAsync(h->badflag.p, 0, 16, h->stream));
    list_desc_upload(h->stream, v, h->list_desc);
    if (scale) {
        h->scr2.ensure((size_t)2 * d);
        HIPCHK(hipMemcpyAsync(h->scr2.p, scale, (size_t)d * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->scr2.p + d, mn, (size_t)d * 8, hipMemcpyHostToDevice, h->stream));
    }
    int k = 0;
    for (int64_t off = 0; off < n; off += slab, k ^= 1) {
        const int64_t ns = std::min<int64_t>(slab, n - off);
        HIPCHK(hipMemcpyAsync(h->ingest_raw[k].p, v.at(off), (size_t)ns * v.record_bytes(), hipMemcpyHostToDevice, h->stream));
        ingest_list_launch(h->stream, h->ingest_raw[k].p, v, h->list_desc.p, ns, off, n, xt_dims(d), h->X.p, h->Xt.p,
                           scale ? h->scr2.p : nullptr, scale ? h->scr2.p + d : nullptr, h->badflag.p);
    }
    HIPCHK(hipGetLastError());
    int bad[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(bad, h->badflag.p, 16, hipMemcpyDeviceToHost, h->stream));
    sync_stream(h, h->stream);
    if (bad[0]) {
        h->n_points = 0;
        return fail(h, CC_ERR_NONFINITE, "input points contain NaN or Inf");
    }
    h->x_absmax = absmax_of(bad);
    return (int)CC_OK;
}

// the prefetch worker of event records: piece by piece, whole records into page-locked staging -> device staging ->
// k_ingest_list into place, all on the worker's stream
void prefetch_list_worker(cc_handle::Prefetch& pf, ListSrc v, int device, size_t xt_rows)
{
    auto chk = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && pf.rc == 0) { pf.rc = (int)e; pf.what = what; }
        return e == hipSuccess;
    };
    if (!chk(hipSetDevice(device), "hipSetDevice")) return;
    hipEvent_t ev[2] = {nullptr, nullptr};
    for (int q = 0; q < 2; ++q)
        if (!chk(hipEventCreateWithFlags(&ev[q], hipEventDisableTiming), "hipEventCreate")) return;
    const double* sc = pf.scaled ? pf.sm.p : nullptr;
    chk(hipMemsetAsync(pf.bad.p, 0, 16, pf.stream), "hipMemsetAsync");
    chk(hipMemcpyAsync(pf.desc.p, v.desc.data(), (size_t)v.d * sizeof(cc_list_desc), hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
    if (pf.scaled) {
        chk(hipMemcpyAsync(pf.sm.p, pf.scale.data(), (size_t)pf.d * 8, hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
        chk(hipMemcpyAsync(pf.sm.p + pf.d, pf.mn.data(), (size_t)pf.d * 8, hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
    }
    long long it = 0;
    int k = 0;
    for (long long off = 0; off < pf.n && pf.rc == 0; off += pf.piece, k ^= 1, ++it) {
        const long long ns = std::min(pf.piece, pf.n - off);
        const size_t len = (size_t)ns * v.record_bytes();
        if (it >= 2) chk(hipEventSynchronize(ev[k]), "hipEventSynchronize");  // the staging buffer is free again
        memcpy(pf.pin[k], v.at(off), len);
        chk(hipMemcpyAsync(pf.raw[k].p, pf.pin[k], len, hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
        chk(hipEventRecord(ev[k], pf.stream), "hipEventRecord");
        if (pf.rc == 0)
            ingest_list_launch(pf.stream, pf.raw[k].p, v, pf.desc.p, ns, off, pf.n, xt_rows, pf.X.p, pf.Xt.p, sc,
                               sc ? sc + pf.d : nullptr, pf.bad.p);
    }
    if (pf.rc == 0) {
        chk(hipMemcpyAsync(pf.bad_host, pf.bad.p, 16, hipMemcpyDeviceToHost, pf.stream), "hipMemcpyAsync");
        chk(hipGetLastError(), "kernel launch");
    }
    chk(hipStreamSynchronize(pf.stream), "hipStreamSynchronize");
    for (int q = 0; q < 2; ++q) (void)hipEventDestroy(ev[q]);
}

int prefetch_list(cc_handle* h, const ListSrc& v, const double* scale, const double* min_)
{
    prefetch_discard(h);
    cc_handle::Prefetch& pf = h->pf;
    const int64_t n = v.n;
    const int d = v.d;
    pf.x = v.data; pf.f32 = false; pf.view = false; pf.list = true; pf.dtype = v.dtype; pf.src_cols = v.src_cols; pf.flags = v.flags;
    pf.ldesc = v.desc;
    pf.n = n; pf.d = d; pf.scaled = scale != nullptr;
    pf.scale.assign(scale, scale ? scale + d : scale);
    pf.mn.assign(min_, min_ ? min_ + d : min_);
    pf.rc = 0; pf.what = ""; pf.bad_host[0] = pf.bad_host[1] = pf.bad_host[2] = pf.bad_host[3] = 0;
    if (!pf.stream) HIPCHK(hipStreamCreateWithFlags(&pf.stream, hipStreamNonBlocking));
    const size_t chunk = (size_t)16 << 20;
    if (pf.pin_bytes < chunk) {
        for (int q = 0; q < 2; ++q) {
            if (pf.pin[q]) (void)hipHostFree(pf.pin[q]);
            pf.pin[q] = nullptr;
            HIPCHK(hipHostMalloc(&pf.pin[q], chunk, hipHostMallocDefault));
        }
        pf.pin_bytes = chunk;
    }
    pf.X.ensure((size_t)n * d); pf.Xt.ensure((size_t)n * xt_dims(d)); pf.sm.ensure((size_t)2 * d); pf.bad.ensure(4);
    pf.desc.ensure((size_t)2 * d);
    // a piece: the whole point tiles of whole records that fit a page-locked buffer (at most 32 KiB a record)
    pf.piece = std::min<int64_t>(list_slab_points(h, v, chunk), (n + 63) & ~(int64_t)63);
    for (int q = 0; q < (n > pf.piece ? 2 : 1); ++q) pf.raw[q].ensure(list_slab_floats(v, pf.piece));
    pf.active = true;
    const int device = h->device;
    const size_t xt_rows = xt_dims(d);
    pf.worker = std::thread([&pf, v, device, xt_rows]() { prefetch_list_worker(pf, v, device, xt_rows); });
    return (int)CC_OK;
}

int col_minmax_list(cc_handle* h, const ListSrc& v, double* out_min, double* out_max)
{
    const int64_t n = v.n;
    const int d = v.d;
    // slab by slab through the two staging buffers, as the upload: every slab leaves k_col_minmax's partials of its own row
    // chunks, part[2][chunks][d], one block per slab behind the other in the scaler scratch
    const int64_t slab = std::min<int64_t>(list_slab_points(h, v, (size_t)32 << 20), (n + 63) & ~(int64_t)63);
    const auto chunks_of = [](int64_t ns) { return (int)std::min<long long>(1024, (ns + 255) / 256); };
    const int64_t slabs = (n + slab - 1) / slab;
    const size_t per_slab = (size_t)2 * chunks_of(slab) * d;
    for (int q = 0; q < (n > slab ? 2 : 1); ++q) h->ingest_raw[q].ensure(list_slab_floats(v, slab));
    h->scr2.ensure(per_slab * (size_t)slabs);
    list_desc_upload(h->stream, v, h->list_desc);
    int k = 0;
    int64_t si = 0;
    for (int64_t off = 0; off < n; off += slab, k ^= 1, ++si) {
        const int64_t ns = std::min<int64_t>(slab, n - off);
        const int chunks = chunks_of(ns);
        double* part = h->scr2.p + per_slab * (size_t)si;
        HIPCHK(hipMemcpyAsync(h->ingest_raw[k].p, v.at(off), (size_t)ns * v.record_bytes(), hipMemcpyHostToDevice, h->stream));
        with_list_dtype(v.dtype, [&](auto t) {
            using T = decltype(t);
            with_bools([&](auto W) {
                hipLaunchKernelGGL((k_col_minmax_list<T, decltype(W)::value>), dim3(chunks, (d + 255) / 256), dim3(256), 0, h->stream,
                                   reinterpret_cast<const unsigned char*>(h->ingest_raw[k].p), (long long)ns, v.src_cols, d,
                                   reinterpret_cast<const cc_list_desc*>(h->list_desc.p), part, chunks);
            }, v.swapped());
        });
    }
    HIPCHK(hipGetLastError());
    std::vector<double> part(per_slab * (size_t)slabs);
    HIPCHK(hipMemcpyAsync(part.data(), h->scr2.p, part.size() * 8, hipMemcpyDeviceToHost, h->stream));
    sync_stream(h, h->stream);
    for (int c = 0; c < d; ++c) {
        double mn = std::numeric_limits<double>::infinity(), mx = -mn;
        si = 0;
        for (int64_t off = 0; off < n; off += slab, ++si) {
            const int chunks = chunks_of(std::min<int64_t>(slab, n - off));
            const double* p = part.data() + per_slab * (size_t)si;
            for (int b = 0; b < chunks; ++b) {
                mn = std::fmin(mn, p[(size_t)b * d + c]);
                mx = std::fmax(mx, p[(size_t)(chunks + b) * d + c]);
            }
        }
        out_min[c] = mn;
        out_max[c] = mx;
    }
    return (int)CC_OK;
}

}  // namespace

extern "C" {

int cc_points_upload_list(cc_handle* h, const cc_list_mode* lm, const double* scale, const double* min_)
{
    if (!h) return CC_ERR_BAD_ARG;
    if ((scale == nullptr) != (min_ == nullptr)) return fail(h, CC_ERR_BAD_ARG, "list mode: scale and min_ go together");
    ListSrc v;
    const int rc = list_check(h, lm, false, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return upload_list(h, v, scale, min_); });
}

int cc_points_prefetch_list(cc_handle* h, const cc_list_mode* lm, const double* scale, const double* min_)
{
    if (!h) return CC_ERR_BAD_ARG;
    if ((scale == nullptr) != (min_ == nullptr)) return fail(h, CC_ERR_BAD_ARG, "list mode: scale and min_ go together");
    ListSrc v;
    const int rc = list_check(h, lm, true, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return prefetch_list(h, v, scale, min_); });
}

int cc_col_minmax_list(cc_handle* h, const cc_list_mode* lm, double* out_min, double* out_max)
{
    if (!h || !out_min || !out_max) return CC_ERR_BAD_ARG;
    ListSrc v;
    const int rc = list_check(h, lm, true, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return col_minmax_list(h, v, out_min, out_max); });
}

int cc_online_list(cc_handle* h, const cc_list_mode* lm, int64_t* out_uid, int8_t* out_path)
{
    int rc = cc_points_upload_list(h, lm, nullptr, nullptr);
    if (rc != CC_OK) return rc;
    rc = cc_online_run(h);
    if (rc != CC_OK) return rc;
    return cc_labels_download(h, out_uid, out_path);
}

int cc_list_points(cc_handle* h, int64_t* out)
{
    if (!h || !out) return CC_ERR_BAD_ARG;
    *out = h->list_points;
    return CC_OK;
}

}  // extern "C"
