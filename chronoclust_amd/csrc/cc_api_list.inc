// cc_api_list.inc — the `_list` entry points: list-mode event records (cc_list_mode: the DATA segment of an FCS file) to the
// device as the bytes they hold.  Whole records travel in slabs - byte copies, no packing pass on the host whatever
// src_cols / d is - and k_ingest_list (cc_ingest_list.h) swaps, gathers the selected channels, masks, widens, scales, checks and
// writes both resident copies.  Here: the descriptor's check (list_check -> ListSrc, cc_ingest_src.h), the descriptors' way to
// the device and the launches of k_ingest_list and k_col_minmax_list for a staged slab.  The upload, the prefetch and the column
// reduction themselves are those of every staged source (cc_api_ingest.inc); cc_assign_list is in cc_api_assign.inc.
// (included by cc_api.hip, the one translation unit, behind cc_api_views.inc)

namespace {

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

// k_col_minmax_list on `st` for the ns records of a slab in device staging (`raw`): its partials part[2][chunks][d]; desc: device
void minmax_list_launch(hipStream_t st, const ListSrc& v, const void* raw, const int* desc, int64_t ns, double* part, int chunks)
{
    const int d = v.d;
    with_list_dtype(v.dtype, [&](auto t) {
        using T = decltype(t);
        with_bools([&](auto W) {
            hipLaunchKernelGGL((k_col_minmax_list<T, decltype(W)::value>), dim3(chunks, (d + 255) / 256), dim3(256), 0, st,
                               static_cast<const unsigned char*>(raw), (long long)ns, v.src_cols, d,
                               reinterpret_cast<const cc_list_desc*>(desc), part, chunks);
        }, v.swapped());
    });
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
    return guarded(h, [&]() { return upload_source(h, IngestSrc::of(v), scale, min_); });
}

int cc_points_prefetch_list(cc_handle* h, const cc_list_mode* lm, const double* scale, const double* min_)
{
    if (!h) return CC_ERR_BAD_ARG;
    if ((scale == nullptr) != (min_ == nullptr)) return fail(h, CC_ERR_BAD_ARG, "list mode: scale and min_ go together");
    ListSrc v;
    const int rc = list_check(h, lm, true, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return prefetch_source(h, IngestSrc::of(v), scale, min_); });
}

int cc_col_minmax_list(cc_handle* h, const cc_list_mode* lm, double* out_min, double* out_max)
{
    if (!h || !out_min || !out_max) return CC_ERR_BAD_ARG;
    ListSrc v;
    const int rc = list_check(h, lm, true, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return col_minmax_slabs(h, IngestSrc::of(v), out_min, out_max); });
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
