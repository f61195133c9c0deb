// cc_api_points.inc — the C-ABI entry points that bring points to the device and back: upload (plain, scaled, adopted from a
// prefetch), the column minima / maxima of the scaler, the prefetch worker, download.  Each taker of points has a float64 and
// a float32 form (`_f32`: the points cross the bus in single precision, in slabs, and k_ingest_f32 widens, scales, checks and
// transposes a slab in one pass; cc_points.h).  (included by cc_api.hip, the one translation unit, behind cc_handle.h)

extern "C" {

static int upload_points(cc_handle* h, const void* x, bool f32, int64_t n, int32_t d, const double* scale, const double* mn);

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

// Points per slab of raw float32 of d dimensions in a staging buffer of `cap_bytes`: whole 64-point tiles, at least one;
// CHRONOCLUST_HIP_INGEST_SLAB shortens it.
static int64_t ingest_slab_points(const cc_handle* h, int d, size_t cap_bytes)
{
    int64_t pts = (int64_t)(cap_bytes / (4 * (size_t)d)) & ~(int64_t)63;
    if (h->ingest_slab > 0) pts = std::min<int64_t>(pts, ((int64_t)h->ingest_slab + 63) & ~(int64_t)63);
    return std::max<int64_t>(CC_INGEST_TILE, pts);
}
// k_ingest_f32 on `st` for the ns points of a slab in device staging (`raw`) that starts at point s0 of n_total: rows s0 ..
// of X [n_total, d], columns s0 .. of Xt [xt_rows, n_total]; scale / mn: device, or both null
static void ingest_launch(hipStream_t st, const float* raw, int64_t ns, int64_t s0, int64_t n_total, int d, size_t xt_rows,
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
    return guarded(h, [&]() { return upload_points(h, x, false, n, d, nullptr, nullptr); });
}

int cc_points_upload_f32(cc_handle* h, const float* x, int64_t n, int32_t d)
{
    if (!h || (!x && n > 0) || n < 0) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() { return upload_points(h, x, true, n, d, nullptr, nullptr); });
}

// MinMax scaling on the device (scaling/scaler.py:27-47).  cc_col_minmax: per-column min / max of a host buffer,
// NaN ignored (what MinMaxScaler.partial_fit takes from one file); cc_points_upload_scaled: cc_points_upload of
// x * scale + min_; cc_points_download_unscaled: (resident points - min_) / scale back to the host.
}  // extern "C"

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
            for (int b = 0; b < chunks; ++b) {
                mn = std::fmin(mn, part[(size_t)b * d + c]);
                mx = std::fmax(mx, part[(size_t)(chunks + b) * d + c]);
            }
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

static int upload_points(cc_handle* h, const void* x, bool f32, int64_t n, int32_t d, const double* scale, const double* mn)
{
    int rc = set_dim(h, d);
    if (rc != CC_OK) return rc;
    if (f32) h->f32_points += n;
    if (h->pf.active) {
        // the points may already be on their way (cc_points_prefetch): adopt them if it is this very upload
        cc_handle::Prefetch& pf = h->pf;
        bool same = !pf.view && !pf.list && pf.x == x && pf.f32 == f32 && pf.n == n && pf.d == d && pf.scaled == (scale != nullptr);
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
    if (f32) {
        // slab by slab through the two staging buffers, all on the handle's stream: the flag words are cleared once and
        // accumulate over the slabs
        const float* xf = static_cast<const float*>(x);
        const int64_t slab = std::min<int64_t>(ingest_slab_points(h, d, (size_t)32 << 20), (n + 63) & ~(int64_t)63);
        for (int q = 0; q < (n > slab ? 2 : 1); ++q) h->ingest_raw[q].ensure((size_t)slab * d);
        HIPCHK(hipMemsetAsync(h->badflag.p, 0, 16, h->stream));
        if (scale) {
            h->scr2.ensure((size_t)2 * d);
            HIPCHK(hipMemcpyAsync(h->scr2.p, scale, (size_t)d * 8, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(h->scr2.p + d, mn, (size_t)d * 8, hipMemcpyHostToDevice, h->stream));
        }
        int k = 0;
        for (int64_t off = 0; off < n; off += slab, k ^= 1) {
            const int64_t ns = std::min<int64_t>(slab, n - off);
            HIPCHK(hipMemcpyAsync(h->ingest_raw[k].p, xf + (size_t)off * d, (size_t)ns * d * 4, hipMemcpyHostToDevice, h->stream));
            ingest_launch(h->stream, h->ingest_raw[k].p, ns, off, n, (int)d, xt_dims(d), h->X.p, h->Xt.p,
                          scale ? h->scr2.p : nullptr, scale ? h->scr2.p + d : nullptr, h->badflag.p);
        }
        HIPCHK(hipGetLastError());
    } else {
        HIPCHK(hipMemcpyAsync(h->X.p, x, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemsetAsync(h->badflag.p, 0, 16, h->stream));
        const long long tot = (long long)n * d;
        if (scale) {
            h->scr2.ensure((size_t)2 * d);
            HIPCHK(hipMemcpyAsync(h->scr2.p, scale, (size_t)d * 8, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(h->scr2.p + d, mn, (size_t)d * 8, hipMemcpyHostToDevice, h->stream));
            hipLaunchKernelGGL(k_scale_points, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->X.p, tot, (int)d,
                               h->scr2.p, h->scr2.p + d);
        }
        int blocks = (int)std::min<long long>((tot + 255) / 256, 4096);
        hipLaunchKernelGGL(k_check_finite, dim3(blocks), dim3(256), 0, h->stream, h->X.p, tot, h->badflag.p);
        HIPCHK(transpose_points_padded(h->stream, h->X.p, h->Xt.p, (long long)n, (int)d));
    }
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

}  // extern "C"

static int points_prefetch(cc_handle* h, const void* x, bool f32, int64_t n, int32_t d, const double* scale, const double* min_)
{
    if (!h || !x || n <= 0 || ((scale == nullptr) != (min_ == nullptr))) return CC_ERR_BAD_ARG;
    if (d <= 0 || d > CC_MAX_DIM) return fail(h, CC_ERR_BAD_ARG, "d must be in 1.." + std::to_string(CC_MAX_DIM));
    return guarded(h, [&]() {
        prefetch_discard(h);
        cc_handle::Prefetch& pf = h->pf;
        pf.x = x; pf.f32 = f32; pf.view = false; pf.list = false; pf.n = n; pf.d = d; pf.scaled = scale != nullptr;
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
        if (f32) {
            // a piece: the whole point tiles that fit a page-locked buffer (at most 4 KiB a point: 4 096 of them at least)
            pf.piece = std::min<int64_t>(ingest_slab_points(h, d, chunk), (n + 63) & ~(int64_t)63);
            for (int q = 0; q < (n > pf.piece ? 2 : 1); ++q) pf.raw[q].ensure((size_t)pf.piece * d);
        }
        pf.active = true;
        const int device = h->device;
        const size_t xt_rows = xt_dims(d);
        pf.worker = std::thread([&pf, device, chunk, xt_rows]() {
            auto chk = [&](hipError_t e, const char* what) {
                if (e != hipSuccess && pf.rc == 0) { pf.rc = (int)e; pf.what = what; }
                return e == hipSuccess;
            };
            if (!chk(hipSetDevice(device), "hipSetDevice")) return;
            const size_t bytes = (size_t)pf.n * pf.d * 8;
            hipEvent_t ev[2] = {nullptr, nullptr};
            for (int q = 0; q < 2; ++q)
                if (!chk(hipEventCreateWithFlags(&ev[q], hipEventDisableTiming), "hipEventCreate")) return;
            int k = 0;
            if (pf.f32) {
                // piece by piece: page-locked staging -> device staging -> k_ingest_f32 into place, all on the worker's stream
                // (a piece's device buffer is free again once the kernel two pieces back has run: stream order)
                const float* xf = static_cast<const float*>(pf.x);
                const double* sc = pf.scaled ? pf.sm.p : nullptr;
                chk(hipMemsetAsync(pf.bad.p, 0, 16, pf.stream), "hipMemsetAsync");
                if (pf.scaled) {
                    chk(hipMemcpyAsync(pf.sm.p, pf.scale.data(), (size_t)pf.d * 8, hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
                    chk(hipMemcpyAsync(pf.sm.p + pf.d, pf.mn.data(), (size_t)pf.d * 8, hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
                }
                long long it = 0;
                for (long long off = 0; off < pf.n && pf.rc == 0; off += pf.piece, k ^= 1, ++it) {
                    const long long ns = std::min(pf.piece, pf.n - off);
                    const size_t len = (size_t)ns * pf.d * 4;
                    if (it >= 2) chk(hipEventSynchronize(ev[k]), "hipEventSynchronize");  // the staging buffer is free again
                    memcpy(pf.pin[k], xf + (size_t)off * pf.d, len);
                    chk(hipMemcpyAsync(pf.raw[k].p, pf.pin[k], len, hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
                    chk(hipEventRecord(ev[k], pf.stream), "hipEventRecord");
                    if (pf.rc == 0)
                        ingest_launch(pf.stream, pf.raw[k].p, ns, off, pf.n, pf.d, xt_rows, pf.X.p, pf.Xt.p, sc,
                                      sc ? sc + pf.d : nullptr, pf.bad.p);
                }
                if (pf.rc == 0) {
                    chk(hipMemcpyAsync(pf.bad_host, pf.bad.p, 16, hipMemcpyDeviceToHost, pf.stream), "hipMemcpyAsync");
                    chk(hipGetLastError(), "kernel launch");
                }
                chk(hipStreamSynchronize(pf.stream), "hipStreamSynchronize");
                for (int q = 0; q < 2; ++q) (void)hipEventDestroy(ev[q]);
                return;
            }
            for (size_t off = 0; off < bytes && pf.rc == 0; off += chunk, k ^= 1) {
                const size_t len = std::min(chunk, bytes - off);
                if (off >= 2 * chunk) chk(hipEventSynchronize(ev[k]), "hipEventSynchronize");  // the staging buffer is free again
                memcpy(pf.pin[k], (const char*)pf.x + off, len);
                chk(hipMemcpyAsync((char*)pf.X.p + off, pf.pin[k], len, hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
                chk(hipEventRecord(ev[k], pf.stream), "hipEventRecord");
            }
            const long long tot = pf.n * (long long)pf.d;
            if (pf.rc == 0) {
                chk(hipMemsetAsync(pf.bad.p, 0, 16, pf.stream), "hipMemsetAsync");
                if (pf.scaled) {
                    chk(hipMemcpyAsync(pf.sm.p, pf.scale.data(), (size_t)pf.d * 8, hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
                    chk(hipMemcpyAsync(pf.sm.p + pf.d, pf.mn.data(), (size_t)pf.d * 8, hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
                    hipLaunchKernelGGL(k_scale_points, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, pf.stream, pf.X.p, tot,
                                       pf.d, pf.sm.p, pf.sm.p + pf.d);
                }
                const int blocks = (int)std::min<long long>((tot + 255) / 256, 4096);
                hipLaunchKernelGGL(k_check_finite, dim3(blocks), dim3(256), 0, pf.stream, pf.X.p, tot, pf.bad.p);
                chk(transpose_points_padded(pf.stream, pf.X.p, pf.Xt.p, pf.n, pf.d), "hipMemsetAsync");
                chk(hipMemcpyAsync(pf.bad_host, pf.bad.p, 16, hipMemcpyDeviceToHost, pf.stream), "hipMemcpyAsync");
                chk(hipGetLastError(), "kernel launch");
            }
            chk(hipStreamSynchronize(pf.stream), "hipStreamSynchronize");
            for (int q = 0; q < 2; ++q) (void)hipEventDestroy(ev[q]);
        });
        return (int)CC_OK;
    });
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
    return guarded(h, [&]() { return upload_points(h, x, false, n, d, scale, min_); });
}

int cc_points_upload_scaled_f32(cc_handle* h, const float* x, int64_t n, int32_t d, const double* scale, const double* min_)
{
    if (!h || (!x && n > 0) || n < 0 || !scale || !min_) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() { return upload_points(h, x, true, n, d, scale, min_); });
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
