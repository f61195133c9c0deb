// cc_api_views.inc — the `_view` entry points: points where they lie on the host (cc_points_view: rows or columns form, nine
// element types) to the device without a copy there.  Here: the descriptor's check (view_check -> ViewSrc, cc_ingest_src.h),
// how a slab of a view is staged (view_stage) and the launches of k_ingest and k_col_minmax_view (cc_ingest.h) for a staged
// slab.  The upload, the prefetch and the column reduction themselves are those of every staged source (cc_api_ingest.inc);
// cc_assign_view is in cc_api_assign.inc.  With a transform (the `_view_xl` entry points: cc_list_transform, cc_list_logicle,
// checked by the list mode's own list_check_xf / list_check_lg over the view's d columns) the launches are those of
// cc_ingest_xf.h: k_ingest_xf / k_col_minmax_view_xf for the columns form, the list kernels for the rows form, whose rows are
// event records.  (included by cc_api.hip, the one translation unit, behind cc_api_points.inc)

namespace {

// (cc_api_list.inc, behind this file)
int list_check_xf(cc_handle* h, const cc_list_transform* xf, ListSrc* out);
int list_check_lg(cc_handle* h, const cc_list_logicle* lg, ListSrc* out);
cc_list_xf list_xf_device(const ListSrc& v, const int* desc);

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

// view_check, then the transform's and the logicle rows' refusals as a list mode's: what every `_view_xl` entry point begins
// with.  The compensated columns index the view's columns, so one outside 0 .. d - 1 is refused as one outside a record is.
// xf and lg null, or a transform that asks for nothing: no transform - the `_view` sibling.
int view_check(cc_handle* h, const cc_points_view* v, const cc_list_transform* xf, const cc_list_logicle* lg, bool need_points,
               ViewSrc* out)
{
    int rc = view_check(h, v, need_points, out);
    if (rc != CC_OK || (!xf && !lg)) return rc;
    ListSrc& t = out->tr;
    t.n = out->n; t.src_cols = out->d; t.dtype = out->dtype; t.sz = out->sz; t.flags = 0; t.d = out->d;
    t.desc.resize((size_t)out->d);
    for (int i = 0; i < out->d; ++i) {
        t.desc[i].col = i;
        t.desc[i].mask = 0xFFFFFFFFu;
    }
    rc = list_check_xf(h, xf, &t);
    return rc != CC_OK ? rc : list_check_lg(h, lg, &t);
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
// a pitch of rp elements) that starts at point s0 of n_total; scale / mn: device, or both null.  tr: the view's transform, with
// one (tr.xf; desc: where list_desc_copy laid it on the device) k_ingest_xf for the columns form and k_ingest_list_xf over
// records of rp elements for the rows form
void ingest_view_launch(hipStream_t st, const void* raw, int dtype, bool cols, int64_t rp, int64_t ns, int64_t s0, int64_t n_total,
                        int d, size_t xt_rows, double* X, double* Xt, const double* scale, const double* mn, int* bad,
                        const ListSrc& tr, const int* desc)
{
    const dim3 grid((unsigned)((ns + CC_INGEST_TILE - 1) / CC_INGEST_TILE), (unsigned)((d + CC_INGEST_TILE - 1) / CC_INGEST_TILE));
    if (tr.xf) {
        const cc_list_xf xf = list_xf_device(tr, desc);
        with_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            with_bools([&](auto L) {
                if (cols)
                    hipLaunchKernelGGL((k_ingest_xf<T, decltype(L)::value>), grid, dim3(256), 0, st, static_cast<const T*>(raw),
                                       (long long)rp, (int)ns, (long long)s0, (long long)n_total, d, (int)xt_rows, xf, X, Xt, scale, mn,
                                       bad);
                else
                    hipLaunchKernelGGL((k_ingest_list_xf<T, false, decltype(L)::value>), grid, dim3(256), 0, st,
                                       static_cast<const unsigned char*>(raw), (int)rp, (int)ns, (long long)s0, (long long)n_total, d,
                                       (int)xt_rows, reinterpret_cast<const cc_list_desc*>(desc), xf, X, Xt, scale, mn, bad);
            }, tr.lg);
        });
        return;
    }
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
// part[2][chunks][d]; with a transform (v.tr.xf; desc: where it lies on the device) over the transformed values:
// k_col_minmax_view_xf for the columns form, k_col_minmax_list_xf over records of the staged pitch for the rows form
void minmax_view_launch(hipStream_t st, const ViewSrc& v, const void* raw, const int* desc, int64_t ns, double* part, int chunks)
{
    const int d = v.d;
    if (v.tr.xf) {
        const cc_list_xf xf = list_xf_device(v.tr, desc);
        with_dtype(v.dtype, [&](auto t) {
            using T = decltype(t);
            with_bools([&](auto L) {
                if (v.cols)
                    hipLaunchKernelGGL((k_col_minmax_view_xf<T, decltype(L)::value>),
                                       dim3(chunks, (d + CC_MINMAX_XF_DIMS - 1) / CC_MINMAX_XF_DIMS), dim3(256), 0, st,
                                       static_cast<const T*>(raw), (long long)ns, d, (long long)v.pitch(ns), xf, part, chunks);
                else
                    hipLaunchKernelGGL((k_col_minmax_list_xf<T, false, decltype(L)::value>),
                                       dim3(chunks, (d + CC_INGEST_TILE - 1) / CC_INGEST_TILE), dim3(256), 0, st,
                                       static_cast<const unsigned char*>(raw), (long long)ns, (int)v.pitch(ns), d,
                                       reinterpret_cast<const cc_list_desc*>(desc), xf, part, chunks);
            }, v.tr.lg);
        });
        return;
    }
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

int cc_points_upload_view_xl(cc_handle* h, const cc_points_view* view, const cc_list_transform* xf, const cc_list_logicle* lg,
                             const double* scale, const double* min_)
{
    if (!h || !view || ((scale == nullptr) != (min_ == nullptr))) return CC_ERR_BAD_ARG;
    ViewSrc v;
    const int rc = view_check(h, view, xf, lg, false, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return upload_source(h, IngestSrc::of(v), scale, min_); });
}

int cc_points_prefetch_view_xl(cc_handle* h, const cc_points_view* view, const cc_list_transform* xf, const cc_list_logicle* lg,
                               const double* scale, const double* min_)
{
    if (!h || !view || ((scale == nullptr) != (min_ == nullptr))) return CC_ERR_BAD_ARG;
    ViewSrc v;
    const int rc = view_check(h, view, xf, lg, true, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return prefetch_source(h, IngestSrc::of(v), scale, min_); });
}

int cc_col_minmax_view_xl(cc_handle* h, const cc_points_view* view, const cc_list_transform* xf, const cc_list_logicle* lg,
                          double* out_min, double* out_max)
{
    if (!h || !view || !out_min || !out_max) return CC_ERR_BAD_ARG;
    ViewSrc v;
    const int rc = view_check(h, view, xf, lg, true, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return col_minmax_slabs(h, IngestSrc::of(v), out_min, out_max); });
}

int cc_online_view_xl(cc_handle* h, const cc_points_view* view, const cc_list_transform* xf, const cc_list_logicle* lg,
                      int64_t* out_uid, int8_t* out_path)
{
    int rc = cc_points_upload_view_xl(h, view, xf, lg, nullptr, nullptr);
    if (rc != CC_OK) return rc;
    rc = cc_online_run(h);
    if (rc != CC_OK) return rc;
    return cc_labels_download(h, out_uid, out_path);
}

// the `_view` entry points: their `_xl` siblings without a transform
int cc_points_upload_view(cc_handle* h, const cc_points_view* view, const double* scale, const double* min_)
{
    return cc_points_upload_view_xl(h, view, nullptr, nullptr, scale, min_);
}

int cc_points_prefetch_view(cc_handle* h, const cc_points_view* view, const double* scale, const double* min_)
{
    return cc_points_prefetch_view_xl(h, view, nullptr, nullptr, scale, min_);
}

int cc_col_minmax_view(cc_handle* h, const cc_points_view* view, double* out_min, double* out_max)
{
    return cc_col_minmax_view_xl(h, view, nullptr, nullptr, out_min, out_max);
}

int cc_online_view(cc_handle* h, const cc_points_view* view, int64_t* out_uid, int8_t* out_path)
{
    return cc_online_view_xl(h, view, nullptr, nullptr, out_uid, out_path);
}

}  // extern "C"
