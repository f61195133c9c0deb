// cc_api_list.inc — the `_list`, `_list_xf` and `_list_xl` entry points: list-mode event records (cc_list_mode: the DATA segment of an FCS file) to the
// device as the bytes they hold.  Whole records travel in slabs - byte copies, no packing pass on the host whatever
// src_cols / d is - and k_ingest_list (cc_ingest_list.h) swaps, gathers the selected channels, masks, widens, scales, checks and
// writes both resident copies.  Here: the descriptor's check (list_check -> ListSrc, cc_ingest_src.h), the descriptors' way to
// the device and the launches of k_ingest_list and k_col_minmax_list for a staged slab - with a transform (cc_list_transform,
// checked by list_check_xf) those of k_ingest_list_xf and k_col_minmax_list_xf (cc_ingest_list_xf.h).  The upload, the prefetch and the column
// reduction themselves are those of every staged source (cc_api_ingest.inc); cc_assign_list is in cc_api_assign.inc.
// With logicle rows (cc_list_logicle, checked by list_check_lg; the coefficients from cc_logicle.h) the same two kernels run as
// their logicle instances; cc_logicle_coefficients hands the coefficients out.
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

// The transform's refusals (cc_list_transform), behind list_check's and like them before anything is read, launched or
// allocated; its copy into `out` as the kernels read it.  xf null, or m = 0 without cofactors: no transform - the `_list` sibling.
int list_check_xf(cc_handle* h, const cc_list_transform* xf, ListSrc* out)
{
    if (!xf) return (int)CC_OK;
    if (xf->reserved != 0) return fail(h, CC_ERR_BAD_ARG, "list transform: reserved must be 0");
    const int m = xf->m, d = out->d;
    if (m < 0 || m > CC_MAX_COMP) return fail(h, CC_ERR_BAD_ARG, "list transform: m must be in 0.." + std::to_string(CC_MAX_COMP));
    if (m > 0 && (!xf->comp_cols || !xf->comp)) return fail(h, CC_ERR_BAD_ARG, "list transform: comp_cols or comp is null with m > 0");
    for (int j = 0; j < m; ++j) {
        if (xf->comp_cols[j] < 0 || xf->comp_cols[j] >= out->src_cols)
            return fail(h, CC_ERR_BAD_ARG, "list transform: compensated column " + std::to_string(xf->comp_cols[j]) + " (entry " +
                                               std::to_string(j) + ") is outside 0.." + std::to_string(out->src_cols - 1));
        for (int i = 0; i < j; ++i)
            if (xf->comp_cols[i] == xf->comp_cols[j])
                return fail(h, CC_ERR_BAD_ARG, "list transform: compensated column " + std::to_string(xf->comp_cols[j]) + " repeats");
    }
    for (int i = 0; i < m * m; ++i)
        if (!std::isfinite(xf->comp[i]))
            return fail(h, CC_ERR_BAD_ARG, "list transform: matrix entry " + std::to_string(i) + " is not finite");
    for (int c = 0; xf->cofactor && c < d; ++c)
        if (!std::isfinite(xf->cofactor[c]) || xf->cofactor[c] < 0.0)
            return fail(h, CC_ERR_BAD_ARG, "list transform: cofactor " + std::to_string(c) + " is negative or not finite");
    if (m == 0 && !xf->cofactor) return (int)CC_OK;
    out->xf = true;
    out->m = m;
    out->has_cof = xf->cofactor != nullptr;
    out->xf_f.assign(xf->comp, xf->comp + (size_t)m * m);
    if (xf->cofactor) out->xf_f.insert(out->xf_f.end(), xf->cofactor, xf->cofactor + d);
    out->xf_i.assign((size_t)2 * m + d, -1);
    for (int j = 0; j < m; ++j) {
        out->xf_i[j] = xf->comp_cols[j];
        // decoded under the mask of the first selected dimension that names the column; none where none does
        bool named = false;
        for (int c = 0; c < d; ++c) {
            if (out->desc[c].col != xf->comp_cols[j]) continue;
            if (!named) out->xf_i[m + j] = (int)out->desc[c].mask;
            named = true;
            out->xf_i[2 * m + c] = j;
        }
    }
    return (int)CC_OK;
}

// The logicle rows' refusals (cc_list_logicle), behind list_check_xf's and like them before anything is read, launched or
// allocated; the coefficients (cc_logicle_derive: the one place they are computed) into `out` behind the cofactors.  lg null, or
// every T == 0: no logicle scale - the `_list_xf` sibling, untouched.
int list_check_lg(cc_handle* h, const cc_list_logicle* lg, ListSrc* out)
{
    if (!lg) return (int)CC_OK;
    if (lg->reserved != 0) return fail(h, CC_ERR_BAD_ARG, "list logicle: reserved must be 0");
    const int d = out->d, m = out->m;
    if (lg->d != d)
        return fail(h, CC_ERR_BAD_ARG, "list logicle: d is " + std::to_string(lg->d) + ", the list mode selects " + std::to_string(d));
    if (!lg->twma) return fail(h, CC_ERR_BAD_ARG, "list logicle: twma is null with d > 0");
    std::vector<double> coef((size_t)5 * d, 0.0);
    bool on = false;
    for (int c = 0; c < d; ++c) {
        double k[8];
        const double* row = lg->twma + (size_t)4 * c;
        const char* why = cc_logicle_derive(row, k);
        if (why) return fail(h, CC_ERR_BAD_ARG, "list logicle: dimension " + std::to_string(c) + ": " + why);
        if (row[0] == 0.0) continue;
        if (out->has_cof && out->xf_f[(size_t)m * m + c] > 0.0)
            return fail(h, CC_ERR_BAD_ARG, "list logicle: dimension " + std::to_string(c) + " has a cofactor and a logicle scale");
        on = true;
        std::copy(k, k + 5, coef.begin() + (size_t)5 * c);
    }
    if (!on) return (int)CC_OK;
    if (!out->xf) {  // (no transform beside it: none compensated, no cofactors)
        out->xf = true;
        out->m = 0;
        out->xf_f.clear();
        out->xf_i.assign((size_t)d, -1);
    }
    if (!out->has_cof) {
        out->has_cof = true;
        out->xf_f.insert(out->xf_f.end(), (size_t)d, 0.0);
    }
    out->lg = true;
    out->lg_twma.assign(lg->twma, lg->twma + (size_t)4 * d);
    out->xf_f.insert(out->xf_f.end(), coef.begin(), coef.end());
    return (int)CC_OK;
}

// list_check, then list_check_xf, then list_check_lg: what every `_list_xl` entry point begins with
int list_check(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, const cc_list_logicle* lg, bool need_points,
               ListSrc* out)
{
    int rc = list_check(h, lm, need_points, out);
    if (rc == CC_OK) rc = list_check_xf(h, xf, out);
    return rc != CC_OK ? rc : list_check_lg(h, lg, out);
}

// the descriptors, and behind them the transform, into `dev` (ListSrc::desc_words() ints) on `st`
hipError_t list_desc_copy(hipStream_t st, const ListSrc& v, int* dev)
{
    static_assert(sizeof(cc_list_desc) == 8, "cc_list_desc is two words");
    hipError_t e = hipMemcpyAsync(dev, v.desc.data(), (size_t)v.d * sizeof(cc_list_desc), hipMemcpyHostToDevice, st);
    if (e != hipSuccess || !v.xf) return e;
    int* at = dev + (size_t)2 * v.d;  // (8-byte aligned: the buffer is, and a descriptor is two words)
    e = hipMemcpyAsync(at, v.xf_f.data(), v.xf_f.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(at + 2 * v.xf_f.size(), v.xf_i.data(), v.xf_i.size() * sizeof(int), hipMemcpyHostToDevice, st);
}

// the transform as the kernels take it, from where list_desc_copy laid it
cc_list_xf list_xf_device(const ListSrc& v, const int* desc)
{
    const double* f = reinterpret_cast<const double*>(desc + (size_t)2 * v.d);
    const int* i = desc + (size_t)2 * v.d + 2 * v.xf_f.size();
    cc_list_xf x;
    x.m = v.m;
    x.comp = f;
    x.cof = v.has_cof ? f + (size_t)v.m * v.m : nullptr;
    x.ccol = i;
    x.cmask = reinterpret_cast<const unsigned*>(i + v.m);
    x.sel = i + 2 * v.m;
    return x;
}

// the descriptors to the device on `st` (`v` outlives the stream's next synchronisation)
void list_desc_upload(hipStream_t st, const ListSrc& v, DevBuf<int>& dev)
{
    dev.ensure(v.desc_words());
    HIPCHK(list_desc_copy(st, v, dev.p));
}

// k_ingest_list on `st` for the ns records of a slab in device staging (`raw`) that starts at event s0 of n_total;
// desc: device; scale / mn: device, or both null
void ingest_list_launch(hipStream_t st, const void* raw, const ListSrc& v, const int* desc, int64_t ns, int64_t s0, int64_t n_total,
                        size_t xt_rows, double* X, double* Xt, const double* scale, const double* mn, int* bad)
{
    const int d = v.d;
    const dim3 grid((unsigned)((ns + CC_INGEST_TILE - 1) / CC_INGEST_TILE), (unsigned)((d + CC_INGEST_TILE - 1) / CC_INGEST_TILE));
    if (v.xf) {
        const cc_list_xf xf = list_xf_device(v, desc);
        with_list_dtype(v.dtype, [&](auto t) {
            using T = decltype(t);
            with_bools([&](auto W, auto L) {
                hipLaunchKernelGGL((k_ingest_list_xf<T, decltype(W)::value, decltype(L)::value>), grid, dim3(256), 0, st,
                                   static_cast<const unsigned char*>(raw), v.src_cols, (int)ns, (long long)s0, (long long)n_total, d,
                                   (int)xt_rows, reinterpret_cast<const cc_list_desc*>(desc), xf, X, Xt, scale, mn, bad);
            }, v.swapped(), v.lg);
        });
        return;
    }
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
    if (v.xf) {
        const cc_list_xf xf = list_xf_device(v, desc);
        with_list_dtype(v.dtype, [&](auto t) {
            using T = decltype(t);
            with_bools([&](auto W, auto L) {
                hipLaunchKernelGGL((k_col_minmax_list_xf<T, decltype(W)::value, decltype(L)::value>),
                                   dim3(chunks, (d + CC_INGEST_TILE - 1) / CC_INGEST_TILE), dim3(256), 0, st,
                                   static_cast<const unsigned char*>(raw), (long long)ns, v.src_cols, d,
                                   reinterpret_cast<const cc_list_desc*>(desc), xf, part, chunks);
            }, v.swapped(), v.lg);
        });
        return;
    }
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

int cc_points_upload_list_xl(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, const cc_list_logicle* lg,
                             const double* scale, const double* min_)
{
    if (!h) return CC_ERR_BAD_ARG;
    if ((scale == nullptr) != (min_ == nullptr)) return fail(h, CC_ERR_BAD_ARG, "list mode: scale and min_ go together");
    ListSrc v;
    const int rc = list_check(h, lm, xf, lg, false, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return upload_source(h, IngestSrc::of(v), scale, min_); });
}

int cc_points_prefetch_list_xl(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, const cc_list_logicle* lg,
                               const double* scale, const double* min_)
{
    if (!h) return CC_ERR_BAD_ARG;
    if ((scale == nullptr) != (min_ == nullptr)) return fail(h, CC_ERR_BAD_ARG, "list mode: scale and min_ go together");
    ListSrc v;
    const int rc = list_check(h, lm, xf, lg, true, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return prefetch_source(h, IngestSrc::of(v), scale, min_); });
}

int cc_col_minmax_list_xl(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, const cc_list_logicle* lg,
                          double* out_min, double* out_max)
{
    if (!h || !out_min || !out_max) return CC_ERR_BAD_ARG;
    ListSrc v;
    const int rc = list_check(h, lm, xf, lg, true, &v);
    if (rc != CC_OK) return rc;
    return guarded(h, [&]() { return col_minmax_slabs(h, IngestSrc::of(v), out_min, out_max); });
}

int cc_online_list_xl(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, const cc_list_logicle* lg, int64_t* out_uid,
                      int8_t* out_path)
{
    int rc = cc_points_upload_list_xl(h, lm, xf, lg, nullptr, nullptr);
    if (rc != CC_OK) return rc;
    rc = cc_online_run(h);
    if (rc != CC_OK) return rc;
    return cc_labels_download(h, out_uid, out_path);
}

int cc_logicle_coefficients(const double twma[4], double out[8])
{
    if (!twma || !out) return CC_ERR_BAD_ARG;
    return cc_logicle_derive(twma, out) ? (int)CC_ERR_BAD_ARG : (int)CC_OK;
}

// the `_list_xf` entry points: their `_xl` siblings without a logicle scale
int cc_points_upload_list_xf(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, const double* scale,
                             const double* min_)
{
    return cc_points_upload_list_xl(h, lm, xf, nullptr, scale, min_);
}

int cc_points_prefetch_list_xf(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, const double* scale,
                               const double* min_)
{
    return cc_points_prefetch_list_xl(h, lm, xf, nullptr, scale, min_);
}

int cc_col_minmax_list_xf(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, double* out_min, double* out_max)
{
    return cc_col_minmax_list_xl(h, lm, xf, nullptr, out_min, out_max);
}

int cc_online_list_xf(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, int64_t* out_uid, int8_t* out_path)
{
    return cc_online_list_xl(h, lm, xf, nullptr, out_uid, out_path);
}

// the `_list` entry points: their `_xf` siblings without a transform
int cc_points_upload_list(cc_handle* h, const cc_list_mode* lm, const double* scale, const double* min_)
{
    return cc_points_upload_list_xf(h, lm, nullptr, scale, min_);
}

int cc_points_prefetch_list(cc_handle* h, const cc_list_mode* lm, const double* scale, const double* min_)
{
    return cc_points_prefetch_list_xf(h, lm, nullptr, scale, min_);
}

int cc_col_minmax_list(cc_handle* h, const cc_list_mode* lm, double* out_min, double* out_max)
{
    return cc_col_minmax_list_xf(h, lm, nullptr, out_min, out_max);
}

int cc_online_list(cc_handle* h, const cc_list_mode* lm, int64_t* out_uid, int8_t* out_path)
{
    return cc_online_list_xf(h, lm, nullptr, out_uid, out_path);
}

int cc_list_points(cc_handle* h, int64_t* out)
{
    if (!h || !out) return CC_ERR_BAD_ARG;
    *out = h->list_points;
    return CC_OK;
}

}  // extern "C"
