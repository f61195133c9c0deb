// cc_api_points.inc — the C-ABI entry points that bring points to the device and back: upload (plain, scaled, adopted from a
// prefetch), the column minima / maxima of the scaler, the prefetch, download.  Each taker of points has a float64 and a
// float32 form.  float64 rows are copied whole and taken in where they land (dense_take_in); `_f32` rows are one kind of
// staged source (IngestSrc, cc_ingest_src.h): they cross the bus in single precision, in slabs, and k_ingest_f32 widens, scales,
// checks and transposes a slab in one pass (cc_points.h).  The upload, the prefetch and its worker are written once for every
// kind, in cc_api_ingest.inc.  (included by cc_api.hip, the one translation unit, behind cc_handle.h)

namespace {
// cc_api_ingest.inc, behind the view's and the event records' helpers that they dispatch to
int upload_source(cc_handle* h, const IngestSrc& src, const double* scale, const double* mn);
int prefetch_source(cc_handle* h, const IngestSrc& src, const double* scale, const double* min_);
int col_minmax_slabs(cc_handle* h, const IngestSrc& src, double* out_min, double* out_max);
}  // namespace

extern "C" {

// Rows of the dimension-major copy of points of d dimensions: the padded width where a snapshot scan may run over padded
// operands (9 <= d <= 64, d no compiled width: cc::scan_width) - k_scan_u, k_seed, k_seed16, k_scan_a, k_scan_p, k_scan_p2 and
// k_scan_p3 read a point's coordinates i < DP of that copy without a bound on d -, else d.  Whatever the pdim filter and k are
// at the time: they may change between the upload and the run.
static size_t xt_dims(int d)
{
    return (d > 8 && d <= CC_WINDOW_MAX_DIM) ? (size_t)cc::scan_width(d, false, false).padded : (size_t)d;
}
// X [n, d] -> Xt [xt_dims(d), n] on `st`: the transpose, then the trailing rows zeroed (zero bytes are +0.0)
static hipError_t transpose_points_padded(hipStream_t st, const double* X, double* Xt, long long n, int d)
{
    const size_t tot = (size_t)n * d, pad = xt_dims(d) - (size_t)d;
    hipLaunchKernelGGL(k_transpose_points, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, X, Xt, n, d);
    return pad > 0 ? hipMemsetAsync(Xt + tot, 0, pad * (size_t)n * 8, st) : hipSuccess;
}

// The float64 route behind its copy, on `st`: X [n, d] on the device scaled in place (sc: scale then min_ on the device, or
// null), checked (k_check_finite into `bad`) and transposed into Xt.
static hipError_t dense_take_in(hipStream_t st, double* X, double* Xt, long long n, int d, const double* sc, int* bad)
{
    const long long tot = n * d;
    if (sc) hipLaunchKernelGGL(k_scale_points, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, X, tot, d, sc, sc + d);
    const int blocks = (int)std::min<long long>((tot + 255) / 256, 4096);
    hipLaunchKernelGGL(k_check_finite, dim3(blocks), dim3(256), 0, st, X, tot, bad);
    return transpose_points_padded(st, X, Xt, n, d);
}

// k_ingest_f32 on `st` for the ns points of a slab in device staging (`raw`) that starts at point s0 of n_total: rows s0 ..
// of X [n_total, d], columns s0 .. of Xt [xt_rows, n_total]; scale / mn: device, or both null
static void ingest_f32_launch(hipStream_t st, const float* raw, int64_t ns, int64_t s0, int64_t n_total, int d, size_t xt_rows,
                              double* X, double* Xt, const double* scale, const double* mn, int* bad)
{
    const dim3 grid((unsigned)((ns + CC_INGEST_TILE - 1) / CC_INGEST_TILE), (unsigned)((d + CC_INGEST_TILE - 1) / CC_INGEST_TILE));
    with_bools([&](auto S) {
        hipLaunchKernelGGL(k_ingest_f32<decltype(S)::value>, grid, dim3(256), 0, st, raw, (int)ns, (long long)s0,
                           (long long)n_total, d, (int)xt_rows, X, Xt, scale, mn, bad);
    }, scale != nullptr);
}

int cc_points_upload(cc_handle* h, const double* x, int64_t n, int32_t d)
{
    if (!h || (!x && n > 0) || n < 0) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() { return upload_source(h, IngestSrc::rows(x, false, n, d), nullptr, nullptr); });
}

int cc_points_upload_f32(cc_handle* h, const float* x, int64_t n, int32_t d)
{
    if (!h || (!x && n > 0) || n < 0) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() { return upload_source(h, IngestSrc::rows(x, true, n, d), nullptr, nullptr); });
}

// MinMax scaling on the device (scaling/scaler.py:27-47).  cc_col_minmax: per-column min / max of a host buffer,
// NaN ignored (what MinMaxScaler.partial_fit takes from one file); cc_points_upload_scaled: cc_points_upload of
// x * scale + min_; cc_points_download_unscaled: (resident points - min_) / scale back to the host.
}  // extern "C"

// column c's minimum / maximum over k_col_minmax's partials of one launch, part[2][chunks][d], folded into mn / mx
static void fold_chunks(const double* part, int chunks, int d, int c, double& mn, double& mx)
{
    for (int b = 0; b < chunks; ++b) {
        mn = std::fmin(mn, part[(size_t)b * d + c]);
        mx = std::fmax(mx, part[(size_t)(chunks + b) * d + c]);
    }
}

// T = double or float: the whole array goes to the scaler scratch as it is (a float takes half a double's room there) and one
// launch reduces it, so that the partition into row chunks - the order of the reduction - is the same for both
template <typename T>
static int col_minmax(cc_handle* h, const T* x, int64_t n, int32_t d, double* out_min, double* out_max)
{
    if (!h || !x || n <= 0 || !out_min || !out_max) return CC_ERR_BAD_ARG;
    if (d <= 0 || d > CC_MAX_DIM) return fail(h, CC_ERR_BAD_ARG, "d must be in 1.." + std::to_string(CC_MAX_DIM));
    return guarded(h, [&]() {
        h->scr.ensure(((size_t)n * d * sizeof(T) + 7) / 8);
        const int chunks = (int)std::min<long long>(1024, (n + 255) / 256);
        h->scr2.ensure((size_t)2 * chunks * d);
        const T* xd = reinterpret_cast<const T*>(h->scr.p);
        HIPCHK(hipMemcpyAsync(h->scr.p, x, (size_t)n * d * sizeof(T), hipMemcpyHostToDevice, h->stream));
        if (d <= 256)
            hipLaunchKernelGGL((k_col_minmax<false, T>), dim3(chunks), dim3(256), 0, h->stream, xd, (long long)n, (int)d,
                               h->scr2.p, chunks);
        else
            hipLaunchKernelGGL((k_col_minmax<true, T>), dim3(chunks, (d + 255) / 256), dim3(256), 0, h->stream, xd,
                               (long long)n, (int)d, h->scr2.p, chunks);
        std::vector<double> part((size_t)2 * chunks * d);
        HIPCHK(hipMemcpyAsync(part.data(), h->scr2.p, part.size() * 8, hipMemcpyDeviceToHost, h->stream));
        sync_stream(h, h->stream);
        for (int c = 0; c < d; ++c) {
            double mn = std::numeric_limits<double>::infinity(), mx = -mn;
            fold_chunks(part.data(), chunks, d, c, mn, mx);
            out_min[c] = mn;
            out_max[c] = mx;
        }
        return (int)CC_OK;
    });
}

extern "C" {

int cc_col_minmax(cc_handle* h, const double* x, int64_t n, int32_t d, double* out_min, double* out_max)
{
    return col_minmax(h, x, n, d, out_min, out_max);
}

int cc_col_minmax_f32(cc_handle* h, const float* x, int64_t n, int32_t d, double* out_min, double* out_max)
{
    return col_minmax(h, x, n, d, out_min, out_max);
}

// waits for a running prefetch; returns true if it finished without an error
static bool prefetch_join(cc_handle* h)
{
    if (h->pf.worker.joinable()) h->pf.worker.join();
    return h->pf.active && h->pf.rc == 0;
}

static void prefetch_discard(cc_handle* h)
{
    (void)prefetch_join(h);
    h->pf.active = false;
}

// the largest |value| k_check_finite saw (words 2..3 of its flag buffer)
static double absmax_of(const int* flag_words)
{
    double m;
    memcpy(&m, flag_words + 2, 8);
    return m;
}

}  // extern "C"

static int points_prefetch(cc_handle* h, const void* x, bool f32, int64_t n, int32_t d, const double* scale, const double* min_)
{
    if (!h || !x || n <= 0 || ((scale == nullptr) != (min_ == nullptr))) return CC_ERR_BAD_ARG;
    if (d <= 0 || d > CC_MAX_DIM) return fail(h, CC_ERR_BAD_ARG, "d must be in 1.." + std::to_string(CC_MAX_DIM));
    return guarded(h, [&]() { return prefetch_source(h, IngestSrc::rows(x, f32, n, d), scale, min_); });
}

extern "C" {

int cc_points_prefetch(cc_handle* h, const double* x, int64_t n, int32_t d, const double* scale, const double* min_)
{
    return points_prefetch(h, x, false, n, d, scale, min_);
}

int cc_points_prefetch_f32(cc_handle* h, const float* x, int64_t n, int32_t d, const double* scale, const double* min_)
{
    return points_prefetch(h, x, true, n, d, scale, min_);
}

int cc_points_upload_scaled(cc_handle* h, const double* x, int64_t n, int32_t d, const double* scale, const double* min_)
{
    if (!h || (!x && n > 0) || n < 0 || !scale || !min_) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() { return upload_source(h, IngestSrc::rows(x, false, n, d), scale, min_); });
}

int cc_points_upload_scaled_f32(cc_handle* h, const float* x, int64_t n, int32_t d, const double* scale, const double* min_)
{
    if (!h || (!x && n > 0) || n < 0 || !scale || !min_) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() { return upload_source(h, IngestSrc::rows(x, true, n, d), scale, min_); });
}

// the resident dimension-major copy as the scans read it: xt_dims(d) rows of n points, the padded rows included
int cc_points_download_xt(cc_handle* h, double* out)
{
    if (!h || !out) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() {
        if (h->n_points == 0 || h->d == 0) return (int)CC_OK;
        HIPCHK(hipMemcpyAsync(out, h->Xt.p, (size_t)h->n_points * xt_dims(h->d) * 8, hipMemcpyDeviceToHost, h->stream));
        sync_stream(h, h->stream);
        return (int)CC_OK;
    });
}

int cc_points_download(cc_handle* h, double* out, const double* scale, const double* min_)
{
    if (!h || !out || ((scale == nullptr) != (min_ == nullptr))) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() {
        const long long tot = h->n_points * (long long)h->d;
        if (tot == 0) return (int)CC_OK;
        const int d = h->d;
        if (!scale) {
            HIPCHK(hipMemcpyAsync(out, h->X.p, (size_t)tot * 8, hipMemcpyDeviceToHost, h->stream));
        } else {
            h->scr.ensure((size_t)tot);
            h->scr2.ensure((size_t)2 * d);
            HIPCHK(hipMemcpyAsync(h->scr2.p, scale, (size_t)d * 8, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(h->scr2.p + d, min_, (size_t)d * 8, hipMemcpyHostToDevice, h->stream));
            hipLaunchKernelGGL(k_unscale_points, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->X.p, h->scr.p,
                               tot, d, h->scr2.p, h->scr2.p + d);
            HIPCHK(hipMemcpyAsync(out, h->scr.p, (size_t)tot * 8, hipMemcpyDeviceToHost, h->stream));
        }
        sync_stream(h, h->stream);
        return (int)CC_OK;
    });
}

}  // extern "C"
