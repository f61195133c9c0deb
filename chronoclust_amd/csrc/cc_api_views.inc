// cc_api_views.inc — the `_view` entry points: points where they lie on the host (cc_points_view: rows or columns form, nine
// element types) to the device without a copy there.  The bytes travel in slabs through the staging buffers of the `_f32`
// route and k_ingest (cc_ingest.h) widens, scales, checks and writes both resident copies; cc_col_minmax_view reduces the
// same slabs.  cc_assign_view is in cc_api_assign.inc.  (included by cc_api.hip, the one translation unit,
// behind cc_api_points.inc)

namespace {

// a checked cc_points_view
struct ViewSrc {
    const char* data = nullptr;
    int64_t n = 0;
    int d = 0, dtype = 0, sz = 0;
    int64_t rs = 0, cs = 0;
    bool cols = false;
    // rows form whose pitch would waste the bus (beyond 8 d elements): the slab's rows are packed on the host first
    bool packed() const { return !cols && rs > 8 * (int64_t)d; }
    // elements from a staged point to the next (rows form) / from a staged strip to the next (columns form) for ns points
    int64_t pitch(int64_t ns) const { return cols ? ((ns + 63) & ~(int64_t)63) : (packed() ? d : rs); }
    // bytes of staging a point takes
    size_t point_bytes() const { return (size_t)(cols || packed() ? d : rs) * sz; }
    const char* at(int64_t r, int64_t c) const { return data + (r * rs + c * cs) * sz; }
};

int dtype_size(int dtype)
{
    switch (dtype) {
    case CC_DT_F64: return 8;
    case CC_DT_F32: case CC_DT_I32: case CC_DT_U32: return 4;
    case CC_DT_F16: case CC_DT_I16: case CC_DT_U16: return 2;
    case CC_DT_I8: case CC_DT_U8: return 1;
    default: return 0;
    }
}

// f(T{}) for the element type of a dtype code (checked before: view_check)
template <typename F>
void with_dtype(int dtype, F&& f)
{
    switch (dtype) {
    case CC_DT_F64: f(double{}); break;
    case CC_DT_F32: f(float{}); break;
    case CC_DT_F16: f(_Float16{}); break;
    case CC_DT_I8: f(int8_t{}); break;
    case CC_DT_U8: f(uint8_t{}); break;
    case CC_DT_I16: f(int16_t{}); break;
    case CC_DT_U16: f(uint16_t{}); break;
    case CC_DT_I32: f(int32_t{}); break;
    default: f(uint32_t{}); break;
    }
}

// The descriptor's refusals, before anything is read, launched or allocated.  `need_points`: n = 0 is refused too.
int view_check(cc_handle* h, const cc_points_view* v, bool need_points, ViewSrc* out)
{
    if (!h || !v) return CC_ERR_BAD_ARG;
    if (v->n < 0 || (need_points && v->n == 0)) return fail(h, CC_ERR_BAD_ARG, "view: n must be " + std::string(need_points ? "positive" : "non-negative"));
    if (!v->data && v->n > 0) return fail(h, CC_ERR_BAD_ARG, "view: data is null");
    if (v->d <= 0 || v->d > CC_MAX_DIM) return fail(h, CC_ERR_BAD_ARG, "d must be in 1.." + std::to_string(CC_MAX_DIM));
    const int sz = dtype_size(v->dtype);
    if (sz == 0) return fail(h, CC_ERR_BAD_ARG, "view: unknown dtype " + std::to_string(v->dtype));
    if (v->row_stride <= 0 || v->col_stride <= 0)
        return fail(h, CC_ERR_BAD_ARG, "view: strides must be positive (row_stride " + std::to_string(v->row_stride) +
                                           ", col_stride " + std::to_string(v->col_stride) + ")");
    // (the stride of an axis of length 1 says nothing: one column or one point satisfies both forms, and is the rows form)
    const int64_t rs = v->n <= 1 ? (v->col_stride == 1 || v->d == 1 ? (int64_t)v->d : 1) : v->row_stride;
    const int64_t cs = v->d == 1 ? 1 : v->col_stride;
    const bool rows = cs == 1 && rs >= v->d;
    const bool cols = rs == 1 && cs >= v->n;
    if (!rows && !cols) {
        if (v->row_stride != 1 && v->col_stride != 1)
            return fail(h, CC_ERR_BAD_ARG, "view: neither stride is 1 (row_stride " + std::to_string(v->row_stride) +
                                               ", col_stride " + std::to_string(v->col_stride) + ")");
        return fail(h, CC_ERR_BAD_ARG, "view: the strides overlap (row_stride " + std::to_string(v->row_stride) + " for d = " +
                                           std::to_string(v->d) + ", col_stride " + std::to_string(v->col_stride) + " for n = " +
                                           std::to_string(v->n) + ")");
    }
    // the extent in bytes: (outer - 1) * stride + inner elements
    const int64_t outer = rows ? v->n : v->d, inner = rows ? v->d : v->n, stride = rows ? rs : cs;
    const int64_t most = std::numeric_limits<int64_t>::max() / sz;
    if (outer > 1 && (stride > (most - inner) / (outer - 1)))
        return fail(h, CC_ERR_BAD_ARG, "view: the extent overflows int64");
    out->data = static_cast<const char*>(v->data);
    out->n = v->n; out->d = v->d; out->dtype = v->dtype; out->sz = sz;
    out->rs = rs; out->cs = cs;
    out->cols = !rows;
    return (int)CC_OK;
}

// Points per slab of a view in a staging buffer of `cap_bytes`: whole 64-point tiles, at least one;
// CHRONOCLUST_HIP_INGEST_SLAB shortens it.  (At most 64 KiB a point: 8 d elements of 8 bytes, d <= 1 024.)
int64_t view_slab_points(const cc_handle* h, const ViewSrc& v, size_t cap_bytes)
{
    int64_t pts = (int64_t)(cap_bytes / v.point_bytes()) & ~(int64_t)63;
    if (h->ingest_slab > 0) pts = std::min<int64_t>(pts, ((int64_t)h->ingest_slab + 63) & ~(int64_t)63);
    return std::max<int64_t>(CC_INGEST_TILE, pts);
}
// floats of a DevBuf<float> that hold a slab of `pts` points (pts: whole tiles)
size_t view_slab_floats(const ViewSrc& v, int64_t pts)
{
    return ((size_t)pts * v.point_bytes() + 3) / 4;
}

// Points off .. off + ns - 1 of the view into device staging `raw` on `st`, as view.pitch(ns) lays them out: whole pitched
// rows in one copy (the last row only as far as its d elements), rows of a wasteful pitch packed on the host first (`pack`;
// the copy has left it when this returns), or d strips.
void view_stage(hipStream_t st, const ViewSrc& v, int64_t off, int64_t ns, void* raw, std::vector<char>& pack)
{
    const size_t sz = (size_t)v.sz;
    if (v.cols) {
        const size_t rp = (size_t)v.pitch(ns);
        for (int c = 0; c < v.d; ++c)
            HIPCHK(hipMemcpyAsync(static_cast<char*>(raw) + (size_t)c * rp * sz, v.at(off, c), (size_t)ns * sz, hipMemcpyHostToDevice, st));
    } else if (v.packed()) {
        const size_t row = (size_t)v.d * sz;
        pack.resize((size_t)ns * row);
        for (int64_t r = 0; r < ns; ++r) memcpy(pack.data() + (size_t)r * row, v.at(off + r, 0), row);
        HIPCHK(hipMemcpyAsync(raw, pack.data(), pack.size(), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    } else {
        HIPCHK(hipMemcpyAsync(raw, v.at(off, 0), ((size_t)(ns - 1) * v.rs + v.d) * sz, hipMemcpyHostToDevice, st));
    }
}

// k_ingest on `st` for the ns points of a slab in device staging (`raw`, laid out by view_stage or by the prefetch worker at
// a pitch of rp elements) that starts at point s0 of n_total; scale / mn: device, or both null
void ingest_view_launch(hipStream_t st, const void* raw, int dtype, bool cols, int64_t rp, int64_t ns, int64_t s0, int64_t n_total,
                        int d, size_t xt_rows, double* X, double* Xt, const double* scale, const double* mn, int* bad)
{
    const dim3 grid((unsigned)((ns + CC_INGEST_TILE - 1) / CC_INGEST_TILE), (unsigned)((d + CC_INGEST_TILE - 1) / CC_INGEST_TILE));
    with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        with_bools([&](auto C, auto S) {
            hipLaunchKernelGGL((k_ingest<T, decltype(C)::value, decltype(S)::value>), grid, dim3(256), 0, st,
                               static_cast<const T*>(raw), (long long)rp, (int)ns, (long long)s0, (long long)n_total, d,
                               (int)xt_rows, X, Xt, scale, mn, bad);
        }, cols, scale != nullptr);
    });
}

int upload_view(cc_handle* h, const ViewSrc& v, const double* scale, const double* mn)
{
    const int64_t n = v.n;
    const int d = v.d;
    int rc = set_dim(h, d);
    if (rc != CC_OK) return rc;
    h->view_points += n;
    if (h->pf.active) {
        // the points may already be on their way (cc_points_prefetch_view): adopt them if it is this very upload
        cc_handle::Prefetch& pf = h->pf;
        bool same = pf.view && pf.x == v.data && pf.n == n && pf.d == d && pf.dtype == v.dtype && pf.rs == v.rs && pf.cs == v.cs &&
                    pf.scaled == (scale != nullptr);
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
    const int64_t slab = std::min<int64_t>(view_slab_points(h, v, (size_t)32 << 20), (n + 63) & ~(int64_t)63);
    for (int q = 0; q < (n > slab ? 2 : 1); ++q) h->ingest_raw[q].ensure(view_slab_floats(v, slab));
    HIPCHK(hipMemsetAsync(h->badflag.p, 0, 16, h->stream));
    if (scale) {
        h->scr2.ensure((size_t)2 * d);
        HIPCHK(hipMemcpyAsync(h->scr2.p, scale, (size_t)d * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->scr2.p + d, mn, (size_t)d * 8, hipMemcpyHostToDevice, h->stream));
    }
    std::vector<char> pack;
    int k = 0;
    for (int64_t off = 0; off < n; off += slab, k ^= 1) {
        const int64_t ns = std::min<int64_t>(slab, n - off);
        view_stage(h->stream, v, off, ns, h->ingest_raw[k].p, pack);
        ingest_view_launch(h->stream, h->ingest_raw[k].p, v.dtype, v.cols, v.pitch(ns), ns, off, n, d, xt_dims(d), h->X.p, h->Xt.p,
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

// the prefetch worker of a view: piece by piece, page-locked staging filled strip by strip (columns form) or row by row
// (rows form, the pitch stripped) -> device staging -> k_ingest into place, all on the worker's stream
void prefetch_view_worker(cc_handle::Prefetch& pf, ViewSrc v, int device, size_t xt_rows)
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
    if (pf.scaled) {
        chk(hipMemcpyAsync(pf.sm.p, pf.scale.data(), (size_t)pf.d * 8, hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
        chk(hipMemcpyAsync(pf.sm.p + pf.d, pf.mn.data(), (size_t)pf.d * 8, hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
    }
    const size_t sz = (size_t)v.sz;
    long long it = 0;
    int k = 0;
    for (long long off = 0; off < pf.n && pf.rc == 0; off += pf.piece, k ^= 1, ++it) {
        const long long ns = std::min(pf.piece, pf.n - off);
        const size_t rp = v.cols ? (size_t)((ns + 63) & ~63ll) : (size_t)v.d;
        const size_t len = (v.cols ? (size_t)v.d * rp : (size_t)ns * rp) * sz;
        if (it >= 2) chk(hipEventSynchronize(ev[k]), "hipEventSynchronize");  // the staging buffer is free again
        char* pin = static_cast<char*>(pf.pin[k]);
        if (v.cols) {
            for (int c = 0; c < v.d; ++c) memcpy(pin + (size_t)c * rp * sz, v.at(off, c), (size_t)ns * sz);
        } else if (v.rs == v.d) {
            memcpy(pin, v.at(off, 0), len);
        } else {
            for (long long r = 0; r < ns; ++r) memcpy(pin + (size_t)r * rp * sz, v.at(off + r, 0), rp * sz);
        }
        chk(hipMemcpyAsync(pf.raw[k].p, pin, len, hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
        chk(hipEventRecord(ev[k], pf.stream), "hipEventRecord");
        if (pf.rc == 0)
            ingest_view_launch(pf.stream, pf.raw[k].p, v.dtype, v.cols, (int64_t)rp, ns, off, pf.n, pf.d, xt_rows, pf.X.p, pf.Xt.p, sc,
                               sc ? sc + pf.d : nullptr, pf.bad.p);
    }
    if (pf.rc == 0) {
        chk(hipMemcpyAsync(pf.bad_host, pf.bad.p, 16, hipMemcpyDeviceToHost, pf.stream), "hipMemcpyAsync");
        chk(hipGetLastError(), "kernel launch");
    }
    chk(hipStreamSynchronize(pf.stream), "hipStreamSynchronize");
    for (int q = 0; q < 2; ++q) (void)hipEventDestroy(ev[q]);
}

int prefetch_view(cc_handle* h, const ViewSrc& v, const double* scale, const double* min_)
{
    prefetch_discard(h);
    cc_handle::Prefetch& pf = h->pf;
    const int64_t n = v.n;
    const int d = v.d;
    pf.x = v.data; pf.f32 = false; pf.view = true; pf.list = false; pf.dtype = v.dtype; pf.rs = v.rs; pf.cs = v.cs;
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
    // a piece: the whole point tiles that fit a page-locked buffer, the rows without their pitch (at most 8 KiB a point)
    ViewSrc tight = v;
    if (!v.cols) tight.rs = d;
    pf.piece = std::min<int64_t>(view_slab_points(h, tight, chunk), (n + 63) & ~(int64_t)63);
    for (int q = 0; q < (n > pf.piece ? 2 : 1); ++q) pf.raw[q].ensure(view_slab_floats(tight, pf.piece));
    pf.active = true;
    const int device = h->device;
    const size_t xt_rows = xt_dims(d);
    pf.worker = std::thread([&pf, v, device, xt_rows]() { prefetch_view_worker(pf, v, device, xt_rows); });
    return (int)CC_OK;
}

int col_minmax_view(cc_handle* h, const ViewSrc& v, double* out_min, double* out_max)
{
    const int64_t n = v.n;
    const int d = v.d;
    // slab by slab through the two staging buffers, as the upload: every slab leaves k_col_minmax's partials of its own row
    // chunks, part[2][chunks][d], one block per slab behind the other in the scaler scratch
    const int64_t slab = std::min<int64_t>(view_slab_points(h, v, (size_t)32 << 20), (n + 63) & ~(int64_t)63);
    const auto chunks_of = [](int64_t ns) { return (int)std::min<long long>(1024, (ns + 255) / 256); };
    const int64_t slabs = (n + slab - 1) / slab;
    const size_t per_slab = (size_t)2 * chunks_of(slab) * d;
    for (int q = 0; q < (n > slab ? 2 : 1); ++q) h->ingest_raw[q].ensure(view_slab_floats(v, slab));
    h->scr2.ensure(per_slab * (size_t)slabs);
    std::vector<char> pack;
    int k = 0;
    int64_t si = 0;
    for (int64_t off = 0; off < n; off += slab, k ^= 1, ++si) {
        const int64_t ns = std::min<int64_t>(slab, n - off);
        const int chunks = chunks_of(ns);
        double* part = h->scr2.p + per_slab * (size_t)si;
        view_stage(h->stream, v, off, ns, h->ingest_raw[k].p, pack);
        with_dtype(v.dtype, [&](auto t) {
            using T = decltype(t);
            const T* xd = reinterpret_cast<const T*>(h->ingest_raw[k].p);
            if (v.cols)
                hipLaunchKernelGGL((k_col_minmax_view<T, true>), dim3(chunks, d), dim3(256), 0, h->stream, xd, (long long)ns, d,
                                   (long long)v.pitch(ns), part, chunks);
            else
                hipLaunchKernelGGL((k_col_minmax_view<T, false>), dim3(chunks, (d + 255) / 256), dim3(256), 0, h->stream, xd,
                                   (long long)ns, d, (long long)v.pitch(ns), part, chunks);
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

int cc_points_upload_view(cc_handle* h, const cc_points_view* view, const double* scale, const double* min_)
{
    if (!h || !view || ((scale == nullptr) != (min_ == nullptr))) return CC_ERR_BAD_ARG;
    ViewSrc v;
    const int rc = view_check(h, view, false, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return upload_view(h, v, scale, min_); });
}

int cc_points_prefetch_view(cc_handle* h, const cc_points_view* view, const double* scale, const double* min_)
{
    if (!h || !view || ((scale == nullptr) != (min_ == nullptr))) return CC_ERR_BAD_ARG;
    ViewSrc v;
    const int rc = view_check(h, view, true, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return prefetch_view(h, v, scale, min_); });
}

int cc_col_minmax_view(cc_handle* h, const cc_points_view* view, double* out_min, double* out_max)
{
    if (!h || !view || !out_min || !out_max) return CC_ERR_BAD_ARG;
    ViewSrc v;
    const int rc = view_check(h, view, true, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return col_minmax_view(h, v, out_min, out_max); });
}

int cc_online_view(cc_handle* h, const cc_points_view* view, int64_t* out_uid, int8_t* out_path)
{
    int rc = cc_points_upload_view(h, view, nullptr, nullptr);
    if (rc != CC_OK) return rc;
    rc = cc_online_run(h);
    if (rc != CC_OK) return rc;
    return cc_labels_download(h, out_uid, out_path);
}

}  // extern "C"
