// cc_api_ingest.inc — the one way of points to the device, whatever their source (IngestSrc, cc_ingest_src.h): what differs by
// kind - how a slab is staged, how page-locked staging is filled, which kernel takes a staged slab in or reduces it, which
// counter the source feeds - in one small function each, and once for all kinds the upload (adoption of a prefetch, the slab
// loop, the refusal of non-finite input), the prefetch with its worker, and the column reduction over slabs.  float64 rows are
// no staged source: their whole-array copy and dense_take_in (cc_api_points.inc) are the other branch of the upload and of the
// worker.  (included by cc_api.hip, the one translation unit, behind cc_api_list.inc)

namespace {

constexpr size_t CC_UPLOAD_STAGING = (size_t)32 << 20;    // a slab of an upload or of a column reduction
constexpr size_t CC_PREFETCH_STAGING = (size_t)16 << 20;  // a page-locked buffer of the prefetch: a piece, or as much of float64 rows
constexpr size_t CC_ASSIGN_STAGING = (size_t)16 << 20;    // a sub-slab of a view's or of event records' chunk in cc_assign

int64_t tiles_up(int64_t n) { return (n + 63) & ~(int64_t)63; }

// Points per slab in a staging buffer of `cap_bytes`: whole 64-point tiles, at least one; CHRONOCLUST_HIP_INGEST_SLAB shortens
// it.  (A point takes 64 KiB at the most: a view's 8 d elements of 8 bytes, d <= 1 024.)
int64_t slab_points(const cc_handle* h, size_t bytes_per_point, size_t cap_bytes)
{
    int64_t pts = (int64_t)(cap_bytes / bytes_per_point) & ~(int64_t)63;
    if (h->ingest_slab > 0) pts = std::min<int64_t>(pts, tiles_up(h->ingest_slab));
    return std::max<int64_t>(CC_INGEST_TILE, pts);
}
// floats of a DevBuf<float> that hold a slab of `pts` points (pts: whole tiles)
size_t slab_floats(size_t bytes_per_point, int64_t pts)
{
    return ((size_t)pts * bytes_per_point + 3) / 4;
}

// the handle's counter that a source feeds (float64 rows: none)
long long* points_counter(cc_handle* h, const IngestSrc& s)
{
    switch (s.kind) {
    case IngestSrc::F32: return &h->f32_points;
    case IngestSrc::VIEW: return &h->view_points;
    case IngestSrc::LIST: return &h->list_points;
    default: return nullptr;
    }
}

// Points off .. off + ns - 1 of a staged source into device staging `raw` on `st`: a view as view_stage lays it out (`pack`:
// its host scratch), rows and whole event records in one copy.
void stage_slab(hipStream_t st, const IngestSrc& s, int64_t off, int64_t ns, void* raw, std::vector<char>& pack)
{
    if (s.kind == IngestSrc::VIEW) return view_stage(st, s.view, off, ns, raw, pack);
    const size_t pb = s.point_bytes(false);
    HIPCHK(hipMemcpyAsync(raw, static_cast<const char*>(s.x) + (size_t)off * pb, (size_t)ns * pb, hipMemcpyHostToDevice, st));
}

// The same points into page-locked staging, tight (the prefetch worker): a view strip by strip (columns form) or row by row
// (rows form, the pitch stripped), rows and whole event records as they lie.  Returns the bytes to copy on.
size_t fill_pinned(const IngestSrc& s, int64_t off, int64_t ns, char* pin)
{
    if (s.kind != IngestSrc::VIEW) {
        const size_t pb = s.point_bytes(true);
        memcpy(pin, static_cast<const char*>(s.x) + (size_t)off * pb, (size_t)ns * pb);
        return (size_t)ns * pb;
    }
    const ViewSrc& v = s.view;
    const size_t sz = (size_t)v.sz, rp = (size_t)s.view_pitch(ns, true);
    if (v.cols) {
        for (int c = 0; c < v.d; ++c) memcpy(pin + (size_t)c * rp * sz, v.at(off, c), (size_t)ns * sz);
        return (size_t)v.d * rp * sz;
    }
    if (v.rs == v.d) {
        memcpy(pin, v.at(off, 0), (size_t)ns * rp * sz);
    } else {
        for (int64_t r = 0; r < ns; ++r) memcpy(pin + (size_t)r * rp * sz, v.at(off + r, 0), rp * sz);
    }
    return (size_t)ns * rp * sz;
}

// The source's ingest kernel on `st` for the ns points of a slab in device staging (`raw`: as stage_slab laid it out, or
// `tight`, as fill_pinned did) that starts at point s0 of n_total: rows s0 .. of X [n_total, d], columns s0 .. of
// Xt [xt_rows, n_total].  desc: the event records' descriptors / a view's transform on the device (IngestSrc::described);
// scale / mn: device, or both null.
void ingest_launch(hipStream_t st, const IngestSrc& s, const void* raw, bool tight, const int* desc, int64_t ns, int64_t s0,
                   int64_t n_total, size_t xt_rows, double* X, double* Xt, const double* scale, const double* mn, int* bad)
{
    switch (s.kind) {
    case IngestSrc::VIEW:
        return ingest_view_launch(st, raw, s.view.dtype, s.view.cols, s.view_pitch(ns, tight), ns, s0, n_total, s.d, xt_rows, X, Xt,
                                  scale, mn, bad, s.view.tr, desc);
    case IngestSrc::LIST: return ingest_list_launch(st, raw, s.list, desc, ns, s0, n_total, xt_rows, X, Xt, scale, mn, bad);
    default: return ingest_f32_launch(st, static_cast<const float*>(raw), ns, s0, n_total, s.d, xt_rows, X, Xt, scale, mn, bad);
    }
}

int upload_source(cc_handle* h, const IngestSrc& src, const double* scale, const double* mn)
{
    const int64_t n = src.n;
    const int d = src.d;
    int rc = set_dim(h, d);
    if (rc != CC_OK) return rc;
    if (long long* taken = points_counter(h, src)) *taken += n;
    cc_handle::Prefetch& pf = h->pf;
    bool adopted = false;
    if (pf.active) {
        // the points may already be on their way (cc_points_prefetch and its kin): adopt them if it is this very upload
        bool same = pf.src.same(src) && pf.scaled == (scale != nullptr);
        for (int i = 0; same && scale && i < d; ++i) same = pf.scale[i] == scale[i] && pf.mn[i] == mn[i];
        const bool ok = prefetch_join(h);
        pf.active = false;
        adopted = same && ok;
    }
    int bad[4] = {0, 0, 0, 0};  // k_check_finite's words, as the worker or this upload read them back
    if (adopted) {
        h->X.swap(pf.X);
        h->Xt.swap(pf.Xt);
        memcpy(bad, pf.bad_host, sizeof bad);
    } else {
        h->X.ensure((size_t)n * d);
        h->Xt.ensure((size_t)n * xt_dims(d));
    }
    h->lab_uid.ensure((size_t)n);
    h->lab_path.ensure((size_t)n);
    h->n_points = n;
    if (!adopted) {
        if (n == 0) return (int)CC_OK;
        // all on the handle's stream: the flag words are cleared once and accumulate over the slabs
        HIPCHK(hipMemsetAsync(h->badflag.p, 0, 16, h->stream));
        const double* sc = nullptr;
        if (scale) {
            h->scr2.ensure((size_t)2 * d);
            HIPCHK(hipMemcpyAsync(h->scr2.p, scale, (size_t)d * 8, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(h->scr2.p + d, mn, (size_t)d * 8, hipMemcpyHostToDevice, h->stream));
            sc = h->scr2.p;
        }
        if (!src.staged()) {
            HIPCHK(hipMemcpyAsync(h->X.p, src.x, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
            HIPCHK(dense_take_in(h->stream, h->X.p, h->Xt.p, (long long)n, d, sc, h->badflag.p));
        } else {
            // slab by slab through the two staging buffers
            const size_t pb = src.point_bytes(false);
            const int64_t slab = std::min<int64_t>(slab_points(h, pb, CC_UPLOAD_STAGING), tiles_up(n));
            for (int q = 0; q < (n > slab ? 2 : 1); ++q) h->ingest_raw[q].ensure(slab_floats(pb, slab));
            if (const ListSrc* ds = src.described()) list_desc_upload(h->stream, *ds, h->list_desc);
            std::vector<char> pack;
            int k = 0;
            for (int64_t off = 0; off < n; off += slab, k ^= 1) {
                const int64_t ns = std::min<int64_t>(slab, n - off);
                stage_slab(h->stream, src, off, ns, h->ingest_raw[k].p, pack);
                ingest_launch(h->stream, src, h->ingest_raw[k].p, false, h->list_desc.p, ns, off, n, xt_dims(d), h->X.p, h->Xt.p, sc,
                              sc ? sc + d : nullptr, h->badflag.p);
            }
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(bad, h->badflag.p, 16, hipMemcpyDeviceToHost, h->stream));
        sync_stream(h, h->stream);
    }
    if (bad[0]) {
        h->n_points = 0;
        return fail(h, CC_ERR_NONFINITE, "input points contain NaN or Inf");
    }
    h->x_absmax = absmax_of(bad);
    return (int)CC_OK;
}

// The prefetch worker, all on its own stream.  A staged source piece by piece: page-locked staging -> device staging -> the
// ingest kernel into place (a piece's device buffer is free again once the kernel two pieces back has run: stream order).
// float64 rows 16 MiB by 16 MiB through the same page-locked buffers straight into pf.X, taken in as a whole behind the last.
void prefetch_worker(cc_handle::Prefetch& pf, int device, size_t xt_rows)
{
    auto chk = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && pf.rc == 0) { pf.rc = (int)e; pf.what = what; }
        return e == hipSuccess;
    };
    if (!chk(hipSetDevice(device), "hipSetDevice")) return;
    hipEvent_t ev[2] = {nullptr, nullptr};
    for (int q = 0; q < 2; ++q)
        if (!chk(hipEventCreateWithFlags(&ev[q], hipEventDisableTiming), "hipEventCreate")) return;
    const IngestSrc& s = pf.src;
    const int d = s.d;
    const double* sc = pf.scaled ? pf.sm.p : nullptr;
    chk(hipMemsetAsync(pf.bad.p, 0, 16, pf.stream), "hipMemsetAsync");
    if (const ListSrc* ds = s.described()) chk(list_desc_copy(pf.stream, *ds, pf.desc.p), "hipMemcpyAsync");
    if (pf.scaled) {
        chk(hipMemcpyAsync(pf.sm.p, pf.scale.data(), (size_t)d * 8, hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
        chk(hipMemcpyAsync(pf.sm.p + d, pf.mn.data(), (size_t)d * 8, hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
    }
    // (a step of the loop: a piece of points, or that many bytes of float64 rows)
    const bool staged = s.staged();
    const long long total = staged ? (long long)s.n : (long long)s.n * d * 8;
    const long long step = staged ? pf.piece : (long long)CC_PREFETCH_STAGING;
    long long it = 0;
    int k = 0;
    for (long long off = 0; off < total && pf.rc == 0; off += step, k ^= 1, ++it) {
        const long long ns = std::min(step, total - off);
        if (it >= 2) chk(hipEventSynchronize(ev[k]), "hipEventSynchronize");  // the staging buffer is free again
        char* pin = static_cast<char*>(pf.pin[k]);
        if (staged) {
            const size_t len = fill_pinned(s, off, ns, pin);
            chk(hipMemcpyAsync(pf.raw[k].p, pin, len, hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
        } else {
            memcpy(pin, static_cast<const char*>(s.x) + off, (size_t)ns);
            chk(hipMemcpyAsync((char*)pf.X.p + off, pin, (size_t)ns, hipMemcpyHostToDevice, pf.stream), "hipMemcpyAsync");
        }
        chk(hipEventRecord(ev[k], pf.stream), "hipEventRecord");
        if (staged && pf.rc == 0)
            ingest_launch(pf.stream, s, pf.raw[k].p, true, pf.desc.p, ns, off, s.n, xt_rows, pf.X.p, pf.Xt.p, sc, sc ? sc + d : nullptr,
                          pf.bad.p);
    }
    if (!staged && pf.rc == 0) chk(dense_take_in(pf.stream, pf.X.p, pf.Xt.p, s.n, d, sc, pf.bad.p), "hipMemsetAsync");
    if (pf.rc == 0) {
        chk(hipMemcpyAsync(pf.bad_host, pf.bad.p, 16, hipMemcpyDeviceToHost, pf.stream), "hipMemcpyAsync");
        chk(hipGetLastError(), "kernel launch");
    }
    chk(hipStreamSynchronize(pf.stream), "hipStreamSynchronize");
    for (int q = 0; q < 2; ++q) (void)hipEventDestroy(ev[q]);
}

int prefetch_source(cc_handle* h, const IngestSrc& src, const double* scale, const double* min_)
{
    prefetch_discard(h);
    cc_handle::Prefetch& pf = h->pf;
    const int64_t n = src.n;
    const int d = src.d;
    pf.src = src;
    pf.scaled = scale != nullptr;
    pf.scale.assign(scale, scale ? scale + d : scale);
    pf.mn.assign(min_, min_ ? min_ + d : min_);
    pf.rc = 0; pf.what = ""; pf.bad_host[0] = pf.bad_host[1] = pf.bad_host[2] = pf.bad_host[3] = 0;
    if (!pf.stream) HIPCHK(hipStreamCreateWithFlags(&pf.stream, hipStreamNonBlocking));
    if (pf.pin_bytes < CC_PREFETCH_STAGING) {
        for (int q = 0; q < 2; ++q) {
            if (pf.pin[q]) (void)hipHostFree(pf.pin[q]);
            pf.pin[q] = nullptr;
            HIPCHK(hipHostMalloc(&pf.pin[q], CC_PREFETCH_STAGING, hipHostMallocDefault));
        }
        pf.pin_bytes = CC_PREFETCH_STAGING;
    }
    pf.X.ensure((size_t)n * d); pf.Xt.ensure((size_t)n * xt_dims(d)); pf.sm.ensure((size_t)2 * d); pf.bad.ensure(4);
    if (const ListSrc* ds = src.described()) pf.desc.ensure(ds->desc_words());
    if (src.staged()) {
        // a piece: the whole point tiles that fit a page-locked buffer, a view's rows without their pitch
        const size_t pb = src.point_bytes(true);
        pf.piece = std::min<int64_t>(slab_points(h, pb, CC_PREFETCH_STAGING), tiles_up(n));
        for (int q = 0; q < (n > pf.piece ? 2 : 1); ++q) pf.raw[q].ensure(slab_floats(pb, pf.piece));
    }
    pf.active = true;
    pf.worker = std::thread(prefetch_worker, std::ref(pf), h->device, xt_dims(d));
    return (int)CC_OK;
}

// Column minima / maxima of a view or of event records: slab by slab through the two staging buffers, as the upload.  Every
// slab leaves k_col_minmax's partials of its own row chunks, part[2][chunks][d], one block per slab behind the other in the
// scaler scratch.
int col_minmax_slabs(cc_handle* h, const IngestSrc& src, double* out_min, double* out_max)
{
    const int64_t n = src.n;
    const int d = src.d;
    const size_t pb = src.point_bytes(false);
    const int64_t slab = std::min<int64_t>(slab_points(h, pb, CC_UPLOAD_STAGING), tiles_up(n));
    const auto chunks_of = [](int64_t ns) { return (int)std::min<long long>(1024, (ns + 255) / 256); };
    const int64_t slabs = (n + slab - 1) / slab;
    const size_t per_slab = (size_t)2 * chunks_of(slab) * d;
    for (int q = 0; q < (n > slab ? 2 : 1); ++q) h->ingest_raw[q].ensure(slab_floats(pb, slab));
    h->scr2.ensure(per_slab * (size_t)slabs);
    if (const ListSrc* ds = src.described()) list_desc_upload(h->stream, *ds, h->list_desc);
    std::vector<char> pack;
    int k = 0;
    int64_t si = 0;
    for (int64_t off = 0; off < n; off += slab, k ^= 1, ++si) {
        const int64_t ns = std::min<int64_t>(slab, n - off);
        double* part = h->scr2.p + per_slab * (size_t)si;
        stage_slab(h->stream, src, off, ns, h->ingest_raw[k].p, pack);
        if (src.kind == IngestSrc::LIST)
            minmax_list_launch(h->stream, src.list, h->ingest_raw[k].p, h->list_desc.p, ns, part, chunks_of(ns));
        else
            minmax_view_launch(h->stream, src.view, h->ingest_raw[k].p, h->list_desc.p, ns, part, chunks_of(ns));
    }
    HIPCHK(hipGetLastError());
    std::vector<double> part(per_slab * (size_t)slabs);
    HIPCHK(hipMemcpyAsync(part.data(), h->scr2.p, part.size() * 8, hipMemcpyDeviceToHost, h->stream));
    sync_stream(h, h->stream);
    for (int c = 0; c < d; ++c) {
        double mn = std::numeric_limits<double>::infinity(), mx = -mn;
        si = 0;
        for (int64_t off = 0; off < n; off += slab, ++si)
            fold_chunks(part.data() + per_slab * (size_t)si, chunks_of(std::min<int64_t>(slab, n - off)), d, c, mn, mx);
        out_min[c] = mn;
        out_max[c] = mx;
    }
    return (int)CC_OK;
}

}  // namespace
