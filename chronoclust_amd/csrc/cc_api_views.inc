// cc_api_views.inc — the `_view` entry points: points where they lie on the host (cc_points_view: rows or columns form, nine
// element types) to the device without a copy there.  Here: the descriptor's check (view_check -> ViewSrc, cc_ingest_src.h),
// how a slab of a view is staged (view_stage) and the launches of k_ingest and k_col_minmax_view (cc_ingest.h) for a staged
// slab.  The upload, the prefetch and the column reduction themselves are those of every staged source (cc_api_ingest.inc);
// cc_assign_view is in cc_api_assign.inc.  (included by cc_api.hip, the one translation unit, behind cc_api_points.inc)

namespace {

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

// k_col_minmax_view on `st` for the ns points of a slab in device staging (`raw`, laid out by view_stage): its partials
// part[2][chunks][d]
void minmax_view_launch(hipStream_t st, const ViewSrc& v, const void* raw, int64_t ns, double* part, int chunks)
{
    const int d = v.d;
    with_dtype(v.dtype, [&](auto t) {
        using T = decltype(t);
        const T* xd = static_cast<const T*>(raw);
        if (v.cols)
            hipLaunchKernelGGL((k_col_minmax_view<T, true>), dim3(chunks, d), dim3(256), 0, st, xd, (long long)ns, d,
                               (long long)v.pitch(ns), part, chunks);
        else
            hipLaunchKernelGGL((k_col_minmax_view<T, false>), dim3(chunks, (d + 255) / 256), dim3(256), 0, st, xd,
                               (long long)ns, d, (long long)v.pitch(ns), part, chunks);
    });
}

}  // namespace

extern "C" {

int cc_points_upload_view(cc_handle* h, const cc_points_view* view, const double* scale, const double* min_)
{
    if (!h || !view || ((scale == nullptr) != (min_ == nullptr))) return CC_ERR_BAD_ARG;
    ViewSrc v;
    const int rc = view_check(h, view, false, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return upload_source(h, IngestSrc::of(v), scale, min_); });
}

int cc_points_prefetch_view(cc_handle* h, const cc_points_view* view, const double* scale, const double* min_)
{
    if (!h || !view || ((scale == nullptr) != (min_ == nullptr))) return CC_ERR_BAD_ARG;
    ViewSrc v;
    const int rc = view_check(h, view, true, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return prefetch_source(h, IngestSrc::of(v), scale, min_); });
}

int cc_col_minmax_view(cc_handle* h, const cc_points_view* view, double* out_min, double* out_max)
{
    if (!h || !view || !out_min || !out_max) return CC_ERR_BAD_ARG;
    ViewSrc v;
    const int rc = view_check(h, view, true, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return col_minmax_slabs(h, IngestSrc::of(v), out_min, out_max); });
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
