// cc_api_assign.inc — cc_assign: the read-only assignment of points to the table as it stands (kernels: cc_assign.h).
// The points travel in chunks through buffers of the call's own (AssignBuffers, cc_handle.h) - two sets, even chunks on the
// first stream and odd ones on the second, so that a chunk's upload runs beside the previous chunk's scan.  Nothing of the
// handle's state is written: not the table, the control block, the resident points or their labels, the window buffers, the
// scan copies or the policy's carried state; of cc_stats only assign_points and assign_launches.  No collective is called:
// on a handle of a group the rank's own table is read.  float64 rows are copied, checked and transposed chunk by chunk; every
// other source (IngestSrc: cc_assign_f32, cc_assign_view, cc_assign_view_xl, cc_assign_list, cc_assign_list_xf, cc_assign_list_xl) takes the same chunks, each staged through the set's
// raw buffer and taken in by its ingest kernel (stage_slab, ingest_launch: cc_api_ingest.inc) - float32 rows a chunk at once, a
// view or event records in sub-slabs of at most 16 MiB.  (included by cc_api.hip, the one translation unit, behind
// cc_api_ingest.inc)

namespace {

// points per chunk: CHRONOCLUST_HIP_ASSIGN_CHUNK, else 32 MiB of coordinates (at most 262 144 points: a few thousand
// workgroups per launch), whole point tiles - in 8-byte terms also for single-precision points: both routes take the same chunks
int64_t assign_chunk_points(const cc_handle* h, int d)
{
    if (h->assign_chunk > 0) return h->assign_chunk;
    const int64_t by_bytes = ((int64_t)32 << 20) / (8 * (int64_t)d);
    return std::max<int64_t>(64, std::min<int64_t>(262144, by_bytes & ~(int64_t)63));
}

// row segments per point tile: CHRONOCLUST_HIP_ASSIGN_SEGMENTS, else one while the chunk's point tiles alone fill the device
// (four workgroups per CU), more for small chunks against large tables - never fewer than one tile of rows per wave
int assign_segments(const cc_handle* h, int64_t chunk, int m_rows)
{
    if (h->assign_segments > 0) return h->assign_segments;
    const int64_t tiles = (chunk + 63) / 64;
    const int64_t want = (4 * (int64_t)h->n_cus + tiles - 1) / tiles;
    const int64_t most = std::max<int64_t>(1, m_rows / (CC_ASSIGN_NW * CC_ASSIGN_TR));
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, most), 64));
}

int assign_run(cc_handle* h, const IngestSrc& src, int64_t* out_uid, int8_t* out_path, double* out_dist, bool* nonfinite)
{
    const int64_t n = src.n;
    const int d = src.d;
    if (long long* taken = points_counter(h, src)) *taken += n;
    h->stats.assign_points = n;
    h->stats.assign_launches = 0;
    if (n == 0) return (int)CC_OK;
    const Ctl& c = h->hc;
    Par par;
    par.delta_sq = c.delta_sq; par.k = c.k; par.inv_k = c.inv_k; par.eps_sq = c.eps_sq; par.beta_mu = c.beta_mu;
    par.pow2 = c.pow2; par.pi = c.pi;
    par.filter = c.pi < d ? 1 : 0;  // (of the points' d: an empty table has none of its own)
    par.d = d;
    const TableStore& tb = h->tab;
    const AssignRows rows{tb.cen.p, tb.pref.p, tb.cf1.p, tb.cf2.p, tb.w.p, tb.kind.p, tb.key.p, tb.uid.p, c.m_rows};
    const int64_t chunk = std::min<int64_t>(assign_chunk_points(h, d), n);
    const int S = assign_segments(h, chunk, c.m_rows);
    hipStream_t st[2] = {h->stream, h->stream2};
    const int sets = n > chunk ? 2 : 1;
    // a staged chunk goes through the set's raw buffer: float32 rows at once, a view or event records in sub-slabs of at most
    // 16 MiB of staging, whatever the view's pitch
    const size_t pb = src.staged() ? src.point_bytes(false) : 0;
    const int64_t sub = !src.staged() ? 0 : src.kind == IngestSrc::F32 ? chunk
                      : std::min<int64_t>(slab_points(h, pb, CC_ASSIGN_STAGING), tiles_up(chunk));
    for (int q = 0; q < sets; ++q) {
        AssignBuffers::Set& b = h->asg[q];
        b.X.ensure((size_t)chunk * d); b.Xt.ensure((size_t)chunk * d);
        if (src.staged()) b.raw.ensure(slab_floats(pb, sub));
        b.uid.ensure((size_t)chunk); b.path.ensure((size_t)chunk); b.dist.ensure((size_t)chunk);
        b.part.ensure((size_t)chunk * S * 2);
        b.bad.ensure(4);
        HIPCHK(hipMemsetAsync(b.bad.p, 0, 16, st[q]));
    }
    if (const ListSrc* ds = src.described()) {
        // the descriptors (a view's transform) once, for both streams
        list_desc_upload(h->stream, *ds, h->list_desc);
        sync_stream(h, h->stream);
    }
    std::vector<char> pack;
    int64_t off = 0;
    for (int64_t ci = 0; off < n; ++ci, off += chunk) {
        const int q = (int)(ci & 1);
        const int cn = (int)std::min<int64_t>(chunk, n - off);
        if (ci >= 2) sync_stream(h, st[q]);  // (the set's previous chunk has left its buffers)
        AssignBuffers::Set& b = h->asg[q];
        const long long tot = (long long)cn * d;
        if (src.staged()) {
            // (one buffer: the next sub-slab's copy follows this one's kernel in stream order)
            for (int64_t s0 = 0; s0 < cn; s0 += sub) {
                const int64_t ns = std::min<int64_t>(sub, cn - s0);
                stage_slab(st[q], src, off + s0, ns, b.raw.p, pack);
                ingest_launch(st[q], src, b.raw.p, false, h->list_desc.p, ns, s0, cn, (size_t)d, b.X.p, b.Xt.p, nullptr, nullptr, b.bad.p);
            }
        } else {
            HIPCHK(hipMemcpyAsync(b.X.p, static_cast<const double*>(src.x) + (size_t)off * d, (size_t)tot * 8, hipMemcpyHostToDevice, st[q]));
            hipLaunchKernelGGL(k_check_finite, dim3((unsigned)std::min<long long>((tot + 255) / 256, 4096)), dim3(256), 0, st[q],
                               (const double*)b.X.p, tot, b.bad.p);
            hipLaunchKernelGGL(k_transpose_points, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st[q], (const double*)b.X.p,
                               b.Xt.p, (long long)cn, d);
        }
        const dim3 grid((unsigned)((cn + 63) / 64), (unsigned)S), block(64 * CC_ASSIGN_NW);
        with_bools([&](auto F, auto P) {
            hipLaunchKernelGGL((k_assign_scan<decltype(F)::value, decltype(P)::value>), grid, block, 0, st[q], rows, par,
                               (const double*)b.X.p, (const double*)b.Xt.p, cn, b.part.p);
        }, par.filter != 0, par.pow2 != 0);
        ++h->stats.assign_launches;
        hipLaunchKernelGGL(k_assign_decide, dim3((unsigned)((cn + 255) / 256)), dim3(256), 0, st[q], rows, par,
                           (const double*)b.X.p, cn, (const Cand*)b.part.p, S, b.uid.p, out_path ? b.path.p : nullptr,
                           out_dist ? b.dist.p : nullptr);
        HIPCHK(hipGetLastError());
        static_assert(sizeof(long long) == sizeof(int64_t), "int64");
        HIPCHK(hipMemcpyAsync(out_uid + off, b.uid.p, (size_t)cn * 8, hipMemcpyDeviceToHost, st[q]));
        if (out_path) HIPCHK(hipMemcpyAsync(out_path + off, b.path.p, (size_t)cn, hipMemcpyDeviceToHost, st[q]));
        if (out_dist) HIPCHK(hipMemcpyAsync(out_dist + off, b.dist.p, (size_t)cn * 8, hipMemcpyDeviceToHost, st[q]));
    }
    int bad[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    for (int q = 0; q < sets; ++q) {
        HIPCHK(hipMemcpyAsync(bad[q], h->asg[q].bad.p, 16, hipMemcpyDeviceToHost, st[q]));
        sync_stream(h, st[q]);
    }
    *nonfinite = bad[0][0] != 0 || bad[1][0] != 0;
    return (int)CC_OK;
}

int assign_points(cc_handle* h, const IngestSrc& src, int64_t* out_uid, int8_t* out_path, double* out_dist)
{
    const int64_t n = src.n;
    const int d = src.d;
    if (!h || n < 0 || (n > 0 && (!src.x || !out_uid))) return CC_ERR_BAD_ARG;
    if (!h->have_par) return fail(h, CC_ERR_BAD_ARG, "cc_set_params has not been called");
    if (d <= 0 || d > CC_MAX_DIM) return fail(h, CC_ERR_BAD_ARG, "d must be in 1.." + std::to_string(CC_MAX_DIM));
    if (h->hc.m_rows > 0 && d != h->d) return fail(h, CC_ERR_BAD_ARG, "dimensionality differs from the microclusters already held");
    bool nonfinite = false;
    const int rc = guarded(h, [&]() { return assign_run(h, src, out_uid, out_path, out_dist, &nonfinite); });
    // (outside guarded: a refused query is no reason to give up the handle's group)
    if (rc == CC_OK && nonfinite) return fail(h, CC_ERR_NONFINITE, "input points contain NaN or Inf");
    return rc;
}

}  // namespace

extern "C" int cc_assign(cc_handle* h, const double* x, int64_t n, int32_t d, int64_t* out_uid, int8_t* out_path,
                         double* out_dist)
{
    return assign_points(h, IngestSrc::rows(x, false, n, d), out_uid, out_path, out_dist);
}

extern "C" int cc_assign_f32(cc_handle* h, const float* x, int64_t n, int32_t d, int64_t* out_uid, int8_t* out_path,
                             double* out_dist)
{
    return assign_points(h, IngestSrc::rows(x, true, n, d), out_uid, out_path, out_dist);
}

extern "C" int cc_assign_view_xl(cc_handle* h, const cc_points_view* view, const cc_list_transform* xf, const cc_list_logicle* lg,
                                 int64_t* out_uid, int8_t* out_path, double* out_dist)
{
    ViewSrc v;
    const int rc = view_check(h, view, xf, lg, false, &v);
    if (rc != CC_OK) return rc;
    return assign_points(h, IngestSrc::of(v), out_uid, out_path, out_dist);
}

extern "C" int cc_assign_view(cc_handle* h, const cc_points_view* view, int64_t* out_uid, int8_t* out_path, double* out_dist)
{
    return cc_assign_view_xl(h, view, nullptr, nullptr, out_uid, out_path, out_dist);
}

extern "C" int cc_assign_list_xl(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, const cc_list_logicle* lg,
                                 int64_t* out_uid, int8_t* out_path, double* out_dist)
{
    ListSrc v;
    const int rc = list_check(h, lm, xf, lg, false, &v);
    if (rc != CC_OK) return rc;
    return assign_points(h, IngestSrc::of(v), out_uid, out_path, out_dist);
}

extern "C" int cc_assign_list_xf(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, int64_t* out_uid,
                                 int8_t* out_path, double* out_dist)
{
    return cc_assign_list_xl(h, lm, xf, nullptr, out_uid, out_path, out_dist);
}

extern "C" int cc_assign_list(cc_handle* h, const cc_list_mode* lm, int64_t* out_uid, int8_t* out_path, double* out_dist)
{
    return cc_assign_list_xf(h, lm, nullptr, out_uid, out_path, out_dist);
}
