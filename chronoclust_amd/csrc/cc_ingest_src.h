// cc_ingest_src.h — what the host knows of points that reach the device through staging: IngestSrc, one description for
// float32 rows (`_f32`), a checked cc_points_view (`_view`; with a checked transform: `_view_xl`) and a checked cc_list_mode (`_list`, `_list_xf`, `_list_xl`), with float64 rows - a
// whole-array copy, not staged - as its fourth kind.  The upload, the prefetch and cc_assign (cc_api_ingest.inc,
// cc_api_assign.inc) are written once against it; cc_handle::Prefetch keeps one to tell which upload may adopt it.
// Host data only: the staging copies and the kernel launches per kind are in cc_api_ingest.inc.
// (included by cc_handle.h, behind the kernels' headers: cc_list_desc is cc_ingest_list.h's)
#pragma once

namespace {

// a checked cc_list_mode: the descriptors with their defaults filled in
struct ListSrc {
    const char* data = nullptr;
    int64_t n = 0;
    int src_cols = 0, dtype = 0, sz = 0, flags = 0, d = 0;
    std::vector<cc_list_desc> desc;  // d of them
    // the transform of the `_list_xf` entry points (cc_list_transform, checked), a copy: xf_f = comp[m][m], then the d
    // cofactors where there are any; xf_i = the m compensated columns, their m masks, then per selected dimension its index
    // into them or -1 (cc_list_xf, cc_ingest_list_xf.h).  On the device both lie behind the descriptors: xf_words() more ints.
    // The logicle rows of the `_list_xl` entry points (cc_list_logicle, checked): lg_twma = the d rows T, W, M, A as given, kept
    // for `same`; with one of them on (lg) the cofactors are always laid - zeros where none were given - and behind them, in
    // xf_f too, the coefficients [d][5] the kernels read (cc_logicle.h).
    bool xf = false, has_cof = false, lg = false;
    int m = 0;
    std::vector<double> xf_f, lg_twma;
    std::vector<int> xf_i;
    size_t xf_words() const { return xf ? 2 * xf_f.size() + xf_i.size() : 0; }
    size_t desc_words() const { return (size_t)2 * d + xf_words(); }
    bool swapped() const { return (flags & CC_LM_SWAPPED) != 0; }
    size_t record_bytes() const { return (size_t)src_cols * (size_t)sz; }
    const char* at(int64_t r) const { return data + (size_t)r * record_bytes(); }
};

// a checked cc_points_view
struct ViewSrc {
    const char* data = nullptr;
    int64_t n = 0;
    int d = 0, dtype = 0, sz = 0;
    int64_t rs = 0, cs = 0;
    bool cols = false;
    // the transform of the `_view_xl` entry points (cc_list_transform / cc_list_logicle, checked by list_check_xf / list_check_lg
    // as a list mode's are): carried as a ListSrc over the view's d columns - src_cols = d, the identity descriptors, no mask -, so
    // that it is laid out on the device, compared and read by the kernels as a list mode's is.  tr.xf: there is one.
    ListSrc tr;
    // rows form whose pitch would waste the bus (beyond 8 d elements): the slab's rows are packed on the host first
    bool packed() const { return !cols && rs > 8 * (int64_t)d; }
    // elements from a staged point to the next (rows form) / from a staged strip to the next (columns form) for ns points
    int64_t pitch(int64_t ns) const { return cols ? ((ns + 63) & ~(int64_t)63) : (packed() ? d : rs); }
    // bytes of staging a point takes
    size_t point_bytes() const { return (size_t)(cols || packed() ? d : rs) * sz; }
    const char* at(int64_t r, int64_t c) const { return data + (r * rs + c * cs) * sz; }
};

struct IngestSrc {
    enum Kind { F64, F32, VIEW, LIST };
    Kind kind = F64;
    const void* x = nullptr;  // point 0 / element (0, 0) of the view / event 0
    int64_t n = 0;
    int d = 0;
    ViewSrc view;  // kind == VIEW
    ListSrc list;  // kind == LIST

    static IngestSrc rows(const void* x, bool f32, int64_t n, int d)
    {
        IngestSrc s;
        s.kind = f32 ? F32 : F64; s.x = x; s.n = n; s.d = d;
        return s;
    }
    static IngestSrc of(const ViewSrc& v)
    {
        IngestSrc s;
        s.kind = VIEW; s.x = v.data; s.n = v.n; s.d = v.d; s.view = v;
        return s;
    }
    static IngestSrc of(const ListSrc& v)
    {
        IngestSrc s;
        s.kind = LIST; s.x = v.data; s.n = v.n; s.d = v.d; s.list = v;
        return s;
    }

    // float64 rows are copied whole and taken in where they land; every other kind travels in slabs through staging
    bool staged() const { return kind != F64; }
    // Bytes of staging a point takes: as an upload stages it (a view keeps a modest pitch), or `tight`, as the prefetch
    // worker lays it into page-locked memory (rows lose their pitch).
    size_t point_bytes(bool tight) const
    {
        switch (kind) {
        case VIEW: return tight ? (size_t)d * view.sz : view.point_bytes();
        case LIST: return list.record_bytes();
        default: return (size_t)d * (kind == F32 ? 4 : 8);
        }
    }
    // a view's staged pitch for a slab of ns points (ViewSrc::pitch; tight: rows at d elements)
    int64_t view_pitch(int64_t ns, bool tight) const { return tight && !view.cols ? d : view.pitch(ns); }
    // The same points read the same way: the kind first, then that kind's fields.  (The same address under another
    // descriptor is another source.)
    bool same(const IngestSrc& o) const
    {
        if (kind != o.kind || x != o.x || n != o.n || d != o.d) return false;
        if (kind == VIEW)
            return view.dtype == o.view.dtype && view.rs == o.view.rs && view.cs == o.view.cs && same_transform(view.tr, o.view.tr);
        if (kind != LIST) return true;
        if (list.dtype != o.list.dtype || list.src_cols != o.list.src_cols || list.flags != o.list.flags) return false;
        for (int i = 0; i < d; ++i)
            if (list.desc[i].col != o.list.desc[i].col || list.desc[i].mask != o.list.desc[i].mask) return false;
        return same_transform(list, o.list);
    }
    // the transform by content: m, the columns, the bits of every matrix entry, cofactor and logicle row
    static bool same_transform(const ListSrc& a, const ListSrc& b)
    {
        if (a.xf != b.xf || a.m != b.m || a.has_cof != b.has_cof || a.xf_i != b.xf_i || a.xf_f.size() != b.xf_f.size() || a.lg != b.lg ||
            a.lg_twma.size() != b.lg_twma.size())
            return false;
        if (!a.lg_twma.empty() && memcmp(a.lg_twma.data(), b.lg_twma.data(), a.lg_twma.size() * sizeof(double)) != 0) return false;
        return a.xf_f.empty() || memcmp(a.xf_f.data(), b.xf_f.data(), a.xf_f.size() * sizeof(double)) == 0;
    }
    // what lies on the device beside the points for the kernels to read, once per call: a list mode's descriptors with its
    // transform behind them, a view's transform (laid out the same way), else nothing
    const ListSrc* described() const { return kind == LIST ? &list : (kind == VIEW && view.tr.xf ? &view.tr : nullptr); }
};

}  // namespace
