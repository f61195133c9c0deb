/*
 * chronoclust_hip.h — C-ABI of the MI355X (gfx950) ChronoClust hot path.
 *
 * This is the drop-in boundary.  The upstream project is pure Python and has
 * no FFI of its own; the seam a maintainer would bind
 * is the HDDStream object (chronoclust/clustering/hddstream.py) and the
 * association tracker (chronoclust/tracking/cluster_tracker.py).  Each entry
 * point below names the reference code it replaces.  INTEGRATION.md shows the
 * ctypes stub that goes into the reference.
 *
 * Conventions
 *  - plain C: pointers + sizes, no C++/torch types; every function returns 0
 *    on success or a negative cc_status; cc_last_error() has the text;
 *  - host pointers unless the name says "device"; row-major float64 [N, d]
 *    (the `_f32` entry points: row-major float32 [N, d], widened on the device;
 *    the `_view` entry points: a cc_points_view - rows or columns, nine element
 *    types -, widened on the device; the `_list` entry points: a cc_list_mode -
 *    list-mode event records as an FCS file holds them, either byte order, a
 *    list of channels -, decoded on the device; the `_list_xf` entry points: the
 *    same with a cc_list_transform - spillover compensation and
 *    asinh(x / cofactor) -, applied on the device as the events are decoded; the
 *    `_list_xl` entry points: the same with a cc_list_logicle - the logicle
 *    display scale, solved per value on the device);
 *  - one handle = one HDDStream state on one GPU; a handle is not thread-safe;
 *  - all floating-point work is IEEE double, no FMA contraction, sums over
 *    dimensions strictly left to right, so results are bit-identical to the
 *    reference's numba functions (utilities/mc_functions.py,
 *    utilities/predeconmc_functions.py);
 *  - there is NO CPU fallback: without a HIP device cc_create fails.
 *
 * Derived parameters are computed by the caller with the reference's own
 * Python expressions and passed in finished (so libm's pow never enters a
 * comparison on the device):
 *    eps_sq      = epsilon ** 2                 hddstream.py:46
 *    delta_sq    = delta ** 2                   hddstream.py:49
 *    ups_eps     = upsilon * epsilon            hddstream.py:47
 *    ups_eps_sq  = (upsilon * epsilon) ** 2     predecon.py:40
 *    mu          = mu_cfg * N                   hddstream.py:126,164
 *    omicron     = omicron_cfg * previous N     hddstream.py:119
 *    pi          = d if pi_cfg <= 0 else round  hddstream.py:107-114
 *    decay factor= 2 ** (-lambda * interval)    hddstream.py:283
 */
#ifndef CHRONOCLUST_HIP_H
#define CHRONOCLUST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cc_handle cc_handle;

enum cc_status {
    CC_OK = 0,
    CC_ERR_NO_DEVICE = -1,   /* no HIP device / HIP runtime error            */
    CC_ERR_BAD_ARG = -2,     /* null pointer, d mismatch, d > CC_MAX_DIM ... */
    CC_ERR_NONFINITE = -3,   /* NaN/Inf in the input points                  */
    CC_ERR_OOM = -4,
    CC_ERR_INTERNAL = -5,
    CC_ERR_COMM = -6         /* RCCL / in-process exchange between ranks failed */
};

enum cc_kind { CC_PCORE = 0, CC_OUTLIER = 1 };

/* Dimensions of a point.  The reference takes any width (hddstream.py:107-114); this library takes d <= CC_MAX_DIM and
 * refuses wider data with CC_ERR_BAD_ARG.  Up to CC_WINDOW_MAX_DIM the online phase runs on the windowed, speculative path
 * (and the sequential kernels where the policy prefers them); from there to CC_MAX_DIM on the sequential workgroup kernel
 * alone (k_seq_g: the reference's loop on the table in HBM; beyond 128 dimensions its wide form walks a point in blocks of
 * 64 dimensions) - exact like every path, one GPU only (cc_online* in a multi-GPU group returns CC_ERR_BAD_ARG for such
 * data).  The offline phase and the trackers take any d <= CC_MAX_DIM.  (1 024: one point fits 8 KB of LDS, and a table
 * of fewer than 2 M rows keeps every rows * d element index below 2^31.) */
#define CC_MAX_DIM 1024
#define CC_WINDOW_MAX_DIM 64

typedef struct cc_params {
    double eps_sq;
    double delta_sq;
    double k;
    double beta;
    double mu;
    double omicron;
    double ups_eps;
    double ups_eps_sq;
    double delta;
    int32_t pi;
    int32_t pad;
} cc_params;

/* Tuning knobs of the exact windowed online path (0 = library default). */
typedef struct cc_tuning {
    int32_t window;          /* points speculated per window (<= 49152 = the default since round 6) */
    int32_t rounds;          /* max validation rounds per window                 */
    int32_t segments;        /* microcluster-range segments per point tile       */
    int32_t windows_per_sync;/* windows enqueued between host read-backs         */
    int32_t time_kernels;    /* 1: bracket every scan launch with HIP events     */
    int32_t dirty_segments;  /* sub-ranges of the version-row scan (0: = segments)*/
    int32_t early_window;    /* window while the table grows fast (0: 4096)       */
    int32_t lookahead;       /* 0 / 1: scan the next window on a second stream
                              * while this one is validated, as long as windows
                              * commit in full (default); 2: off; 3: always      */
    int32_t sequential;      /* the one-wavefront sequential kernel for small tables:
                              * 0 when the speculative windows keep being cut
                              * short and it measures faster (default); 1 never;
                              * 2 whenever the table fits its LDS image           */
} cc_tuning;

typedef struct cc_stats {
    int64_t points;          /* points processed by the last cc_online_run       */
    int64_t windows;         /* windows committed                                 */
    int64_t rounds;          /* validation rounds executed                        */
    int64_t truncated;       /* windows committed short of their full size       */
    int64_t scan_launches;   /* snapshot-scan launches timed (time_kernels = 1)  */
    double  scan_ms;         /* sum of their HIP-event durations                  */
    double  scan_pair_dims;  /* (point, microcluster, dim) triples they covered   */
    double  run_ms;          /* HIP-event time of the whole cc_online_run         */
    int64_t rows;            /* microcluster rows in the table after the run     */
    int64_t table_rows_scanned; /* sum over windows of the table rows a scan read  */
    int64_t lookahead_windows; /* windows whose snapshot scan ran ahead             */
    int64_t sharded_windows; /* windows whose snapshot scan was split over the ranks (multi-GPU) */
    int64_t comm_launches;   /* merge + all-gather steps timed (time_kernels = 1)  */
    double  comm_ms;         /* sum of their HIP-event durations                  */
    int64_t seq_points;      /* points taken by the sequential kernel             */
    int64_t scan_u_launches; /* snapshot scans launched as k_scan_u (rows as scalar
                              * operands) rather than the LDS-staged k_scan          */
    int64_t scan_p_launches; /* of those, pruned scans (k_seed + k_seed_merge + k_scan_p: rows
                              * abandoned as soon as their partial sums pass a threshold) */
    int64_t pruned_scan_rows;      /* (wave, row) pairs the pruned scans visited (sampled: the
                                    * first point tile of every window) ...              */
    int64_t pruned_scan_full_rows; /* ... and of those, pairs evaluated over all dimensions */
    int64_t window;          /* configured window of the run (cc_tuning.window or the default)  */
    int64_t long_chains;     /* chains of existing microclusters with more than 32 claimants in a window
                              * (per validation round) ...                                      */
    int64_t long_chain_launches; /* ... and launches of k_chain_long over the list of such chains (tables
                              * of more than 1 024 rows; smaller ones always run it)             */
    int64_t tiles;           /* 64-point tiles validated ...                                               */
    int64_t dirty_tiles;     /* ... and of those, tiles whose dirty scan had to run (last round of a window) */
    int64_t scan_launches_pruned;  /* of scan_launches: the timed launches that were pruned chains ...       */
    double  scan_ms_pruned;        /* ... their share of scan_ms ...                                          */
    double  scan_pair_dims_pruned; /* ... and of scan_pair_dims (the rest: plain scans)                       */
    int64_t scan_g_launches;       /* of scan_p_launches: with guessed thresholds (no seed pass over the window) */
    int64_t missed_points;         /* ... points those scans missed (the seeded chain ran for them alone)        */
    int64_t probe_launches;        /* plain scans that carried a probe of the pruned chain (128 points)          */
    int64_t seq_r_points;          /* of seq_points: taken by the register-resident sequential kernel (d <= 4)    */
    int64_t heavy_launches;        /* k_claims_heavy launches (claims of heavy rows gathered without k_decide's atomics) */
    int64_t scan_lean_launches;    /* of scan_g_launches: lean - no list of missed points, no seeded chain behind the scan */
    int64_t long_prepared;         /* of long_chains: chains of pcore microclusters whose running sums were laid out ahead of
                                    * k_chain, every step then evaluated by the step's own 32-lane group ...              */
    int64_t long_replayed;         /* ... and of those, chains replayed from the first step the radius test rejected */
    int64_t seq_g_points;          /* of seq_points: taken by k_seq_g (table in HBM: beyond the sequential kernel's LDS image) */
    int64_t link_launches;         /* windows whose round 0 linked the points that decided "create" among themselves
                                    * (k_link_scan + k_link_apply: while microclusters are being created)                  */
    int64_t scan_p2_launches;      /* of scan_p_launches: the window's pruned scan as k_scan_p2 (two points per lane in phase A,
                                    * phase B from the same residency) rather than k_scan_p                                */
    /* the split of the snapshot scans over the ranks of a group (cc_comm_calibrate): what was measured when the group
     * was formed and the thresholds in force - (table rows x d) from which a plain scan / a pruned chain is split */
    double  calib_allgather_us;    /* all-gather of one full window's records (64 B per point and rank); 0: not measured   */
    double  calib_scan_ns_per_row_dim;  /* plain snapshot scan of a full window: ns per (table row, dimension)             */
    int64_t split_threshold_row_dims;
    int64_t split_threshold_row_dims_pruned;
    int64_t missed_plain_launches; /* plain scans (k_scan_u over a point list) for the points a guessed-threshold scan missed */
    int64_t seed16_launches;       /* seeded pruned chains whose seeds came from the matrix cores (k_seed16) with the tight threshold */
    int64_t pad_rows_launches;     /* snapshot scans that ran over padded operands (k_pad_rows in front of them: 9 <= d <= 64, d no compiled width) */
    /* the last cc_assign (the only fields it writes; cc_online_run clears them with the rest) */
    int64_t assign_points;         /* points it was asked to assign */
    int64_t assign_launches;       /* k_assign_scan launches: one per chunk of points */
} cc_stats;

/* HDDStream.__init__ (hddstream.py:30-67): one state object on GPU `device`. */
int cc_create(int device, cc_handle** out);
void cc_destroy(cc_handle* h);
const char* cc_last_error(const cc_handle* h);
int cc_set_tuning(cc_handle* h, const cc_tuning* t);
/* Back to the state of a fresh HDDStream (no microclusters, id counters at 0); keeps buffers and parameters. */
int cc_reset(cc_handle* h);

/* hddstream.py:89-128 + 45-52: parameters in force for the following calls. */
int cc_set_params(cc_handle* h, const cc_params* p);

/* hddstream.py:199-213: _decay_clusters_weight(interval) (:247-286), then
 * downgrade_microclusters() (:512-549, including the skip-next-element
 * behaviour of removing from the list being iterated).  `factor` =
 * 2 ** (-lambda * interval). */
int cc_decay_downgrade(cc_handle* h, double factor);

/* The per-point loop of online_microcluster_maintenance (hddstream.py:220-237:
 * _add_to_pcore :288-343, _add_to_outlier :345-395 incl. upgrade :397-430,
 * _create_new_outlier_cluster :434-462), exact sequential semantics.
 *   cc_points_upload : copy X[N,d] to HBM (checks for NaN/Inf on the device)
 *   cc_online_run    : cluster the resident points in row order
 *   cc_labels_download: out_uid[r] = creation number (prev_outlier_id) of the
 *                      microcluster holding row r (microcluster.py:149);
 *                      out_path[r] (optional) = 0 pcore add, 1 outlier add,
 *                      2 new microcluster, |4 if the add promoted it
 *   cc_online        : the three of them in one call */
int cc_points_upload(cc_handle* h, const double* x, int64_t n, int32_t d);
/* Starts uploading the NEXT timepoint's points in the background (a worker thread copies them through page-locked
 * staging buffers on a stream of its own, then scales / checks / transposes them), while the caller still works on
 * the current timepoint (offline phase, trackers, writers - app.py:179-216).  scale / min_: as for
 * cc_points_upload_scaled, or both NULL.  The next cc_points_upload / cc_points_upload_scaled (or cc_online) with the
 * same pointer, shape and scaling adopts the result instead of copying; any other upload discards it.  x must stay
 * valid and unchanged until then.  The clustering results do not depend on whether an upload was prefetched. */
int cc_points_prefetch(cc_handle* h, const double* x, int64_t n, int32_t d, const double* scale, const double* min_);
int cc_online_run(cc_handle* h);
int cc_labels_download(cc_handle* h, int64_t* out_uid, int8_t* out_path);
int cc_online(cc_handle* h, const double* x, int64_t n, int32_t d, int64_t* out_uid, int8_t* out_path);

/* Read-only assignment: for each of the n points of x [n, d] (host, row-major), independently of every other point, what
 * the per-point loop above would do with it if it were the very next point - against the table exactly as it stands.
 *   out_uid[r]  = creation number of the microcluster the point would join, -1 if it would create one (no creation
 *                 number is consumed)
 *   out_path[r] (optional) = 0 nearest admissible pcore microcluster (pdim filter and radius test of the enlarged row,
 *                 hddstream.py:311-337), 1 nearest outlier microcluster (:371-386), |4 if that add would promote it
 *                 (:416-419), 2 new
 *   out_dist[r] (optional) = projected distance to the reported row (paths 0, 1, 5), -1.0 for path 2
 * i.e. the (uid, path) cc_online of that one point returns on a copy of the table, except that path 2 reports -1.
 * Nothing is modified: both lists, the id counters, the resident points and their labels, every other field of cc_stats.
 * The points travel in chunks through buffers of the call's own.  On a handle of a group the rank's table is read and no
 * collective is called.  Preconditions and errors as for cc_online: cc_set_params first; CC_ERR_BAD_ARG for d outside
 * 1..CC_MAX_DIM or different from the table's while it holds rows; CC_ERR_NONFINITE for NaN / Inf (the outputs are then
 * unspecified).  n = 0 succeeds; an empty table gives path 2 everywhere. */
int cc_assign(cc_handle* h, const double* x, int64_t n, int32_t d, int64_t* out_uid, int8_t* out_path, double* out_dist);

/* Single-precision points.  Cytometry events are 32-bit floats at the source (FCS files); each entry point below has the
 * contract of its float64 sibling - arguments, errors, what happens to a group - with x row-major float32 [N, d].  The
 * points cross the bus as they are, in slabs of whole 64-point tiles through two device staging buffers (at most 32 MiB
 * each; CHRONOCLUST_HIP_INGEST_SLAB=<points> shortens them), and one kernel per slab (k_ingest_f32) widens them - float to
 * double is exact -, applies scale_ / min_ in double (two roundings, as the float64 route), checks the stored values for
 * NaN / Inf and writes the row-major and the dimension-major copy.  What the device then holds is bit for bit what the
 * float64 entry point holds after the same values widened on the host, so every result is the same; scale, min_ and all
 * outputs stay double.  A prefetch is adopted by the upload of the same pointer, shape, scaling AND element type.
 * cc_assign_f32 takes the chunks cc_assign takes (cc_stats.assign_launches is the same).
 * cc_f32_points: *out = the points taken in single precision since cc_create - uploads (an adopted cc_points_prefetch_f32
 * included), cc_online_f32 and cc_assign_f32; no call clears it.  (A counter of its own, not a field of cc_stats: that
 * structure's layout and size stay what callers were compiled against.) */
int cc_points_upload_f32(cc_handle* h, const float* x, int64_t n, int32_t d);
int cc_points_upload_scaled_f32(cc_handle* h, const float* x, int64_t n, int32_t d, const double* scale,
                                const double* min_);
int cc_points_prefetch_f32(cc_handle* h, const float* x, int64_t n, int32_t d, const double* scale, const double* min_);
int cc_col_minmax_f32(cc_handle* h, const float* x, int64_t n, int32_t d, double* out_min, double* out_max);
int cc_online_f32(cc_handle* h, const float* x, int64_t n, int32_t d, int64_t* out_uid, int8_t* out_path);
int cc_assign_f32(cc_handle* h, const float* x, int64_t n, int32_t d, int64_t* out_uid, int8_t* out_path, double* out_dist);
/* The resident points' dimension-major copy as the snapshot scans read it, whichever route brought them: out [rows, n] with
 * rows = the padded scan width (cc_scan_width) for 9 <= d <= CC_WINDOW_MAX_DIM, else d; the rows beyond d hold +0.0. */
int cc_points_download_xt(cc_handle* h, double* out);
int cc_f32_points(cc_handle* h, int64_t* out);

/* Point views: points where they lie - column-major, pitched or narrow-typed - without a copy on the host.  Strides are in
 * ELEMENTS, not bytes; the elements are in native byte order. */
enum cc_dtype {
    CC_DT_F64 = 0, CC_DT_F32 = 1, CC_DT_F16 = 2,   /* IEEE binary64 / binary32 / binary16 */
    CC_DT_I8 = 3, CC_DT_U8 = 4, CC_DT_I16 = 5, CC_DT_U16 = 6, CC_DT_I32 = 7, CC_DT_U32 = 8
};

typedef struct cc_points_view {
    const void* data;     /* element (0, 0) */
    int64_t n;            /* points */
    int32_t d;            /* dimensions */
    int32_t dtype;        /* CC_DT_F64, _F32, _F16, _I8, _U8, _I16, _U16, _I32, _U32: native byte order */
    int64_t row_stride;   /* elements from a point to the next */
    int64_t col_stride;   /* elements from a dimension to the next */
} cc_points_view;

/* A view is taken in one of two layouts:
 *   rows form:    col_stride == 1 && row_stride >= d  (C order; a range of columns of a C-order array)
 *   columns form: row_stride == 1 && col_stride >= n  (Fortran order - what pandas hands out for a parsed CSV -; a range
 *                 of rows of a Fortran-order array; the transpose of a [d, N] array)
 * (The stride of an axis of length 1 says nothing and is ignored: one point or one dimension satisfies both, and is taken in
 * the rows form.)  Every other view - a zero or negative stride, both strides different
 * from 1, an unknown dtype, d outside 1..CC_MAX_DIM, an extent beyond int64 - is refused with CC_ERR_BAD_ARG and a message
 * that names the reason, before anything is read, launched or allocated.
 * Each entry point has the contract of its float64 sibling.  The bytes cross the bus as they are, in slabs of whole 64-point
 * tiles through the two device staging buffers of the `_f32` route (at most 32 MiB each, 16 MiB pieces in a prefetch;
 * CHRONOCLUST_HIP_INGEST_SLAB=<points> shortens a slab): the rows form as whole pitched rows in one copy (a pitch beyond 8 d
 * elements is stripped on the host, slab by slab, in elements of the source type), the columns form as d strips.  One kernel
 * per slab (k_ingest) widens - (double) of every accepted type is exact -, applies scale_ / min_ in double (two roundings),
 * checks the stored values for NaN / Inf and writes the row-major and the dimension-major copy: what the device then holds is
 * bit for bit what cc_points_upload holds after the same values widened and laid out on the host.
 * cc_points_upload_view / cc_points_prefetch_view: scale and min_ both NULL (plain) or both given (cc_points_upload_scaled).
 * A prefetch is adopted by the cc_points_upload_view (or cc_online_view) of the same pointer, shape, both strides, dtype and
 * scaling; any other upload discards it.
 * cc_col_minmax_view: the extrema compare equal to cc_col_minmax of the widened dense array (the sign of a zero extremum may
 * differ: the reduction's order does; MinMaxScaler's scale_ and min_ are the same for both signs).
 * cc_assign_view takes the chunks cc_assign takes (cc_stats.assign_launches is the same), each through sub-slabs of at most
 * 16 MiB of staging; cc_col_minmax_view reduces the upload's slabs in the upload's staging buffers: no staging is added.
 * cc_view_points: *out = the points taken through the `_view` entry points since cc_create (uploads, an adopted prefetch
 * included, cc_online_view, cc_assign_view); no call clears it.  cc_f32_points counts the `_f32` entry points only. */
int cc_points_upload_view(cc_handle* h, const cc_points_view* view, const double* scale, const double* min_);
int cc_points_prefetch_view(cc_handle* h, const cc_points_view* view, const double* scale, const double* min_);
int cc_col_minmax_view(cc_handle* h, const cc_points_view* view, double* out_min, double* out_max);
int cc_online_view(cc_handle* h, const cc_points_view* view, int64_t* out_uid, int8_t* out_path);
int cc_assign_view(cc_handle* h, const cc_points_view* view, int64_t* out_uid, int8_t* out_path, double* out_dist);
int cc_view_points(cc_handle* h, int64_t* out);

/* List-mode event records: the DATA segment of a list-mode FCS file as the bytes it holds.  An event is a record of src_cols
 * elements of one type, in the host's byte order or the other one; the dimensions to cluster on are a LIST of the record's
 * columns (Time, scatter and marker channels are interleaved: a list, not a range, so no cc_points_view describes them). */
#define CC_MAX_SRC_COLS 4096
enum { CC_LM_SWAPPED = 1 };      /* elements are in the other byte order than the host's */
typedef struct cc_list_mode {
    const void* data;       /* first byte of event 0; NO alignment is required */
    int64_t n;              /* events */
    int32_t src_cols;       /* elements per event record, 1 .. CC_MAX_SRC_COLS (4 096) */
    int32_t dtype;          /* CC_DT_F32, CC_DT_F64, CC_DT_U8, CC_DT_U16, CC_DT_U32 */
    int32_t flags;          /* 0 or CC_LM_SWAPPED */
    int32_t d;              /* selected columns, 1 .. CC_MAX_DIM */
    const int32_t* cols;    /* d source columns in output order, each in 0 .. src_cols - 1, repeats allowed; NULL: 0 .. d - 1 */
    const uint32_t* masks;  /* d AND masks, integer dtypes only; NULL: none */
} cc_list_mode;

/* Each entry point has the contract of its float64 sibling (arguments, errors, what happens to a group).  Refused with
 * CC_ERR_BAD_ARG and a message that names the reason, before anything is read, launched or allocated: a null descriptor or
 * null data, n < 0 (n == 0 where the sibling needs points: prefetch, col_minmax), d outside 1..CC_MAX_DIM, src_cols outside
 * 1..CC_MAX_SRC_COLS, a column index outside 0 .. src_cols - 1 (d > src_cols without a column list), another dtype code,
 * unknown flag bits, masks with a floating dtype, an extent n * src_cols * element size beyond int64.
 * The bytes travel as whole event records, in slabs of whole 64-point tiles through the two device staging buffers of the
 * `_f32` route (at most 32 MiB each, 16 MiB pieces in a prefetch; CHRONOCLUST_HIP_INGEST_SLAB=<events> shortens a slab).
 * The copies are byte copies, so `data` may sit at any address: the device staging buffer starts aligned and a record is a
 * whole multiple of its element size.  There is NO packing pass on the host, whatever src_cols / d is: a file of 60
 * channels of which 5 are clustered moves 12 times its payload across the bus - the caller's trade (select on the host and
 * use a `_view` or `_f32` entry point where that is the wrong one).  A channel that is not selected is never read on the
 * device: a NaN pattern in it is no error.
 * One kernel per slab (k_ingest_list) decodes an element - loaded as an unsigned integer of its width; with CC_LM_SWAPPED
 * its bytes reversed; an integer ANDed with its mask, a float bit-cast; (double), exact for every type -, applies scale_ /
 * min_ in double (two roundings), checks the stored values for NaN / Inf and writes the row-major and the dimension-major
 * copy: what the device then holds is bit for bit what cc_points_upload holds after the same values decoded on the host.
 * cc_points_upload_list / cc_points_prefetch_list: scale and min_ both NULL (plain) or both given (cc_points_upload_scaled).
 * A prefetch is adopted by the cc_points_upload_list (or cc_online_list) of the same pointer, n, src_cols, dtype, flags, d,
 * column list, masks (NULL and the defaults it stands for compare equal) and scaling; any other upload discards it.
 * cc_col_minmax_list reduces the upload's slabs in the upload's staging buffers (the sign of a zero extremum is free, as
 * for cc_col_minmax_view).  cc_assign_list takes the chunks cc_assign takes (cc_stats.assign_launches is the same), each
 * through sub-slabs of at most 16 MiB of staging.
 * cc_list_points: *out = the events taken through the `_list` entry points since cc_create (uploads, an adopted prefetch
 * included, cc_online_list, cc_assign_list); no call clears it.  cc_f32_points and cc_view_points do not count this route;
 * cc_stats keeps its layout. */
int cc_points_upload_list(cc_handle* h, const cc_list_mode* lm, const double* scale, const double* min_);
int cc_points_prefetch_list(cc_handle* h, const cc_list_mode* lm, const double* scale, const double* min_);
int cc_col_minmax_list(cc_handle* h, const cc_list_mode* lm, double* out_min, double* out_max);
int cc_online_list(cc_handle* h, const cc_list_mode* lm, int64_t* out_uid, int8_t* out_path);
int cc_assign_list(cc_handle* h, const cc_list_mode* lm, int64_t* out_uid, int8_t* out_path, double* out_dist);
int cc_list_points(cc_handle* h, int64_t* out);

/* List-mode event records, compensated and arcsinh-transformed on the device: what a cytometry file takes before it is
 * clustered, done where the events land.  For one event let x[s] be the decoded stored value of source column s (the decoding
 * of the `_list` entry points: swap, AND mask, bit-cast or widening; exact in double).
 *   compensation  m distinct source columns comp_cols[0 .. m - 1] and comp[m][m], row-major: the INVERSE of the spillover
 *                 matrix (the caller inverts).  A selected dimension whose source column is comp_cols[i] holds
 *                 v = ((x[comp_cols[0]] * comp[0][i]) + x[comp_cols[1]] * comp[1][i]) + ...  in ascending j, every product
 *                 and every sum rounded to double, nothing fused, the accumulator starting as the first product; any other
 *                 selected dimension holds v = x.  Compensated columns need not be selected, but they are read: a NaN in
 *                 one reaches the selected values and the upload is refused with CC_ERR_NONFINITE.  An integer compensated
 *                 column is decoded under the mask of the first selected dimension that names it; one that no selected
 *                 dimension names, under none.  m = 0: no compensation.
 *   cofactor      d entries, one per selected dimension, or NULL for none.  cofactor[c] > 0: v = asinh(v / cofactor[c]) - one
 *                 double division, the device maths library's asinh (its measured distance from the
 *                 correctly rounded value); cofactor[c] == 0: the value passes through untouched.
 * scale / min_, the finiteness flag, the magnitude maximum and both resident copies follow as for the `_list` entry points;
 * the two copies hold the same doubles (each value is computed once).  cc_col_minmax_list_xf reduces the transformed,
 * unscaled values - the very doubles the plain upload holds.
 * Each entry point is its `_list` sibling with a transform; xf == NULL (or m == 0 and cofactor == NULL) IS the sibling.  Refused
 * with CC_ERR_BAD_ARG and a message that names the reason, before anything is read or launched, beside the sibling's refusals:
 * m outside 0 .. CC_MAX_COMP, comp_cols or comp NULL with m > 0, a comp_cols entry outside 0 .. src_cols - 1 or one that
 * repeats, a matrix entry that is not finite, a cofactor that is negative or not finite, reserved != 0.
 * A prefetch is adopted only by the upload with the same transform: m, the columns, and the bits of every matrix entry and
 * cofactor.  cc_list_points counts these events too; a group of ranks behaves as with the `_list` siblings. */
#define CC_MAX_COMP 64
typedef struct cc_list_transform {
    int32_t m;                 /* compensated source columns, 0 .. CC_MAX_COMP; 0: no compensation */
    int32_t reserved;          /* 0 */
    const int32_t* comp_cols;  /* m distinct source columns, each in 0 .. src_cols - 1 */
    const double* comp;        /* [m][m] row-major: the inverse of the spillover matrix */
    const double* cofactor;    /* d entries (> 0: asinh(v / cofactor), 0: pass through), or NULL for none */
} cc_list_transform;
int cc_points_upload_list_xf(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, const double* scale,
                             const double* min_);
int cc_points_prefetch_list_xf(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, const double* scale,
                               const double* min_);
int cc_col_minmax_list_xf(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, double* out_min, double* out_max);
int cc_online_list_xf(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, int64_t* out_uid, int8_t* out_path);
int cc_assign_list_xf(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, int64_t* out_uid, int8_t* out_path,
                      double* out_dist);

/* List-mode event records on the logicle (biexponential) display scale, solved on the device: what fluorescence flow cytometry
 * is clustered on, as arcsinh is the scale of mass cytometry.  The scale of Parks, Roederer and Moore 2006 in the
 * parameterisation of Moore and Parks 2012; for one selected dimension with T > 0, M > 0, 0 <= W, 2 W <= M, -W <= A <= M - 2 W:
 *   w  = W / (M + A)      x2 = A / (M + A)      x1 = x2 + w      x0 = x2 + 2 w      b = (M + A) ln 10
 *   d  = the root in (0, b] of  2 (ln d - ln b) + w (d + b) = 0        (w == 0: d = b)
 *   ca = exp(x0 (b + d))          mf = exp(b x1) - ca exp(-d x1)       a = T / ((exp(b) - mf) - ca exp(-d))
 *   pa = a exp(b x1)              pc = a ca exp(-d x1)
 *   G(u) = pa (exp(b u) - 1) - pc (exp(-d u) - 1),  u >= 0:  G(0) = 0, G(1 - x1) = T, G''(0) = 0, G' > 0
 *   logicle(v) = x1 + sign(v) u,  u the root of G(u) = |v|;  logicle(+-0) = x1
 * The result is on the UNIT display scale: T maps to 1 and 0 to x1, it is not multiplied by M; values beyond +-T map beyond
 * [2 x1 - 1, 1] and are not clipped.  Per value: the decoding, then the compensation of the cc_list_transform (unchanged, bit
 * for bit), then the logicle scale OR the cofactor - a dimension that carries both is refused -, then scale / min_, then the
 * finiteness flag.  A finite v of any magnitude gives a finite result; the solve takes a fixed number of Halley steps, no loop
 * depends on the data.  A NaN or Inf v gives a non-finite result and the upload is refused with CC_ERR_NONFINITE, as ever.
 * There is no closed form: the result lies within a few units of np.spacing(max(|y|, 0.5)) of the root rounded once from
 * extended precision (DESIGN.md sections 5.3 and 8: the measured distance) - where the very values matter, read them back
 * (cc_points_download).
 * The coefficients are derived once per dimension on the host - w, x2, x1, x0 as the doubles of the formulas, everything behind
 * them in long double, rounded once - by the one function cc_logicle_coefficients also hands them out through:
 * out = {x1, b, d, pa, pc, 0, 0, 0} (all zeros for T == 0), CC_ERR_BAD_ARG for parameters outside the contract.  It needs no
 * handle and no GPU.
 * Each `_list_xl` entry point is its `_list_xf` sibling with logicle rows; lg == NULL, or every T == 0, IS the sibling.  Refused
 * with CC_ERR_BAD_ARG and a message that names the reason, before anything is read or launched, beside the siblings' refusals:
 * d other than the cc_list_mode's, twma NULL, a parameter that is not finite, T < 0, on a row with T > 0: M <= 0, W < 0,
 * 2 W > M, A < -W or A > M - 2 W (or coefficients beyond a double), a row with T > 0 on a dimension whose cofactor is > 0,
 * reserved != 0.  A prefetch is adopted only by the upload with the same logicle rows, bit for bit. */
typedef struct cc_list_logicle {
    int32_t d;           /* selected dimensions: must equal the cc_list_mode's */
    int32_t reserved;    /* 0 */
    const double* twma;  /* [d][4] row-major: T, W, M, A; a row with T == 0 leaves the dimension off the logicle scale */
} cc_list_logicle;
int cc_points_upload_list_xl(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, const cc_list_logicle* lg,
                             const double* scale, const double* min_);
int cc_points_prefetch_list_xl(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, const cc_list_logicle* lg,
                               const double* scale, const double* min_);
int cc_col_minmax_list_xl(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, const cc_list_logicle* lg,
                          double* out_min, double* out_max);
int cc_online_list_xl(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, const cc_list_logicle* lg, int64_t* out_uid,
                      int8_t* out_path);
int cc_assign_list_xl(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf, const cc_list_logicle* lg, int64_t* out_uid,
                      int8_t* out_path, double* out_dist);
int cc_logicle_coefficients(const double twma[4], double out[8]);

/* Point views, compensated and arcsinh- or logicle-transformed on the device: the transform contract of the `_list_xf` and
 * `_list_xl` entry points, unchanged, for the arrays a parsed CSV, a .npy file or a caller hands over.  Per value: (double) of
 * the element, exact for every view type; then the compensation - the same left-to-right sum in double, nothing fused -;
 * then asinh(v / cofactor) - one double division, the device maths library's asinh - OR the logicle scale - the same solve with
 * its compile-time step count -; then scale / min_, the finiteness flag, the magnitude maximum and both resident copies, which
 * hold the same doubles (each value is computed once).  A view's row of d elements is read as an event record whose selected
 * dimensions are its columns 0 .. d - 1: what the device then holds is bit for bit what the `_list_xl` entry points hold after
 * the same values laid out as float64 event records.
 * xf and lg are the structures of the list-mode entry points as they are: comp_cols index the VIEW's columns 0 .. d - 1 - every
 * compensated column is therefore a selected dimension, and there are no masks -; cofactor and twma hold one entry / one row
 * per column of the view.
 * Each entry point is its `_view` sibling with a transform; xf == NULL && lg == NULL, or a transform that asks for nothing
 * (m == 0, cofactor == NULL, every T == 0), IS the sibling.  Refused with CC_ERR_BAD_ARG and a message that names the reason,
 * before anything is read or launched, beside the sibling's refusals: everything the `_list_xf` / `_list_xl` entry points
 * refuse about xf and lg, with the view's d in the place of src_cols - so a compensated column outside 0 .. d - 1 - and of the
 * selected dimensions.  A NaN in a compensated column, or a compensated sum that overflows, refuses the upload with
 * CC_ERR_NONFINITE.  A prefetch is adopted only by the upload of the same view with the same transform: m, the columns and
 * the bits of every matrix entry, cofactor and logicle row.  cc_col_minmax_view_xl reduces the transformed, unscaled values -
 * the very doubles the plain upload holds.  cc_view_points counts these points too; a group of ranks behaves as with the
 * `_view` siblings. */
int cc_points_upload_view_xl(cc_handle* h, const cc_points_view* view, const cc_list_transform* xf, const cc_list_logicle* lg,
                             const double* scale, const double* min_);
int cc_points_prefetch_view_xl(cc_handle* h, const cc_points_view* view, const cc_list_transform* xf, const cc_list_logicle* lg,
                               const double* scale, const double* min_);
int cc_col_minmax_view_xl(cc_handle* h, const cc_points_view* view, const cc_list_transform* xf, const cc_list_logicle* lg,
                          double* out_min, double* out_max);
int cc_online_view_xl(cc_handle* h, const cc_points_view* view, const cc_list_transform* xf, const cc_list_logicle* lg,
                      int64_t* out_uid, int8_t* out_path);
int cc_assign_view_xl(cc_handle* h, const cc_points_view* view, const cc_list_transform* xf, const cc_list_logicle* lg,
                      int64_t* out_uid, int8_t* out_path, double* out_dist);

/* An exact order statistic per selected column over the NEGATIVE compensated values of list-mode events, pooled over any number
 * of sources and selected on the device: what the rule of Parks, Roederer and Moore 2006 takes the logicle width from
 * (W = (M - log10(T / |r|)) / 2, r the 5th percentile of a channel's negative values - the caller's arithmetic).
 * For one selected dimension, over every event added since cc_negq_begin:
 *   v      the value the `_list_xf` entry points compute with cofactor 0 - decoded, masked, compensated by the source's own
 *          comp (the same left-to-right sum, bit for bit) -, not put through a cofactor or a logicle scale, not scaled
 *   neg    the multiset of all v < 0 (NaN, +-0 and positive values are not in it; -Inf is);  cnt = |neg|
 *   h = (cnt - 1) * q in double;  j = floor(h);  frac = h - j
 *   lo = sorted(neg)[j],  hi = sorted(neg)[min(j + 1, cnt - 1)]: exact order statistics, bit for bit
 * cnt == 0 gives cnt = 0, lo = hi = frac = 0.  numpy's linear interpolation of (lo, hi) at frac is np.quantile(neg, q).
 * cc_negq_begin: d selected dimensions per source, want[d] non-zero for the dimensions to select (NULL: all), capacity = the
 * events to come, pooled; allocates want x capacity doubles of scratch (CC_ERR_OOM leaves the handle as it was); a begin while
 * one is open starts over.  cc_negq_add_list: appends one source's events, streamed through the upload's staging buffers in the
 * upload's slabs; xf as for cc_col_minmax_list_xf (NULL: no compensation) but its cofactors are not applied; any number of
 * calls, n == 0 adds nothing.  cc_negq_select: cnt, lo, hi, frac per selected dimension (each [d]; a dimension that is not
 * wanted: cnt = -1 and zeros) for one q in [0, 1]; any number of calls, nothing changes.  A radix select over the bit
 * patterns, 8 passes of 8 bits: the number of launches and every loop's trip count are functions of the sizes alone, one host
 * wait ends the call.  cc_negq_end frees the scratch; cc_destroy does too, cc_reset leaves it alone.
 * Refused with CC_ERR_BAD_ARG and a message that names the reason, before anything is read, launched or allocated: a null
 * handle or null outputs, d outside 1..CC_MAX_DIM, capacity < 0, add / select / end without begin, a cc_list_mode whose d is
 * not begin's, a running total beyond capacity, q outside [0, 1] or NaN, and everything cc_col_minmax_list_xf refuses about lm
 * and xf.  None of these calls changes what a later call can observe: resident points and labels, tables, counters,
 * cc_list_points, a pending prefetch and cc_stats stay as they are.  They are not collective: in a group every rank that
 * makes them gets the same answer. */
int cc_negq_begin(cc_handle* h, int32_t d, const uint8_t* want, int64_t capacity);
int cc_negq_add_list(cc_handle* h, const cc_list_mode* lm, const cc_list_transform* xf);
int cc_negq_select(cc_handle* h, double q, int64_t* out_count, double* out_lo, double* out_hi, double* out_frac);
int cc_negq_end(cc_handle* h);

/* HDDStream.pcore_MC / outlier_MC (hddstream.py:56-57) in list order.
 * Any output pointer may be NULL.  cf1/cf2/cen/pref are [count, d]. */
int cc_count(cc_handle* h, int kind);
int cc_dim(cc_handle* h);
int cc_counters(cc_handle* h, int64_t* pcore_last_id, int64_t* outlier_last_id);
/* Checkpoint restore: the id counters of hddstream.py:63-64 (the reference's own pickle drops them). */
int cc_set_counters(cc_handle* h, int64_t pcore_last_id, int64_t outlier_last_id);
int cc_export(cc_handle* h, int kind, int64_t* id, int64_t* uid, double* w,
              double* cf1, double* cf2, double* cen, double* pref);
/* Appends one microcluster to a list (tests, checkpoint restore). */
int cc_inject_mc(cc_handle* h, int kind, int32_t d, const double* cf1, const double* cf2, const double* cen,
                 const double* pref, double w, int64_t id, int64_t uid);

/* Appends n microclusters to a list in one upload (checkpoint restore of a whole table: what unpickling the
 * reference's pcore_MC / outlier_MC lists does, app.py:436-465).  cf1/cf2/cen/pref are [n, d]; w, id, uid [n]. */
int cc_inject_bulk(cc_handle* h, int kind, int32_t d, int32_t n, const double* cf1, const double* cf2,
                   const double* cen, const double* pref, const double* w, const int64_t* id, const int64_t* uid);

/* HDDStream.offline_clustering (hddstream.py:464-510) + PreDeCon.run
 * (clustering/predecon.py:49-267): core flags, eps-neighbourhoods, subspace
 * preference vectors and weighted reachability on the device; the ordered
 * expansion (predecon.py:89-120) on the host.  Returns the number of clusters
 * through *n_clusters.  Optional per-pcore dumps are indexed by list position. */
int cc_offline(cc_handle* h, int32_t* n_clusters, int8_t* out_core, int32_t* out_pdim, int32_t* out_nn,
               int32_t* out_nw);
int cc_num_core(cc_handle* h);
int cc_cluster_size(cc_handle* h, int32_t c);
/* members = pcore ids in merge order (predecon_mc.py:50-68) */
int cc_cluster_export(cc_handle* h, int32_t c, int64_t* members, double* w, double* cf1, double* cf2,
                      double* cen, double* pref);

/* All clusters in one call: offsets[n_clusters + 1] index members[] (pcore ids, merge order);
 * w is [n_clusters]; cf1 / cf2 / cen / pref are [n_clusters, d].  Any output pointer may be NULL. */
int cc_clusters_total_members(cc_handle* h);
int cc_clusters_export(cc_handle* h, int64_t* members, int32_t* offsets, double* w, double* cf1, double* cf2,
                       double* cen, double* pref);

/* MinMax scaling on the device (scaling/scaler.py:27-47, i.e. scikit-learn's
 * MinMaxScaler.partial_fit / transform / inverse_transform, feature range [0, 1]):
 *   cc_col_minmax              : per-column minimum / maximum of x[n, d], NaN ignored
 *                                (np.nanmin / np.nanmax); the caller folds the files of
 *                                all timepoints and forms scale_ = 1 / range
 *                                (range < 10 eps -> 1), min_ = 0 - data_min * scale_
 *   cc_points_upload_scaled    : cc_points_upload of x * scale_ + min_ (two roundings,
 *                                as numpy evaluates transform), scaled on the device
 *   cc_points_download         : the resident points back to the host; with scale_ / min_
 *                                given, (X - min_) / scale_ (inverse_transform), else as held */
int cc_col_minmax(cc_handle* h, const double* x, int64_t n, int32_t d, double* out_min, double* out_max);
int cc_points_upload_scaled(cc_handle* h, const double* x, int64_t n, int32_t d, const double* scale,
                            const double* min_);
int cc_points_download(cc_handle* h, double* out, const double* scale, const double* min_);

/* TrackByHistoricalAssociation.track_cluster_history (cluster_tracker.py:127-141):
 * for every current pcore (cur_cen/cur_pref [mc,d]) the index of the previous
 * pcore (prev_cen [mp,d], given in iteration order) with the smallest
 * sum_d (prev - cur)^2 / cur_pref; strict <, first minimum wins. */
int cc_assoc_argmin(cc_handle* h, const double* cur_cen, const double* cur_pref, int32_t mc,
                    const double* prev_cen, int32_t mp, int32_t d, int32_t* out_idx, double* out_dist);

/* Exact multi-GPU path for ONE event stream (the reference is a single Python thread and
 * has no counterpart).  `world` handles - one per GPU, each in its own process (RCCL) or, for verification on a
 * single GPU, several in one process with one host thread each (local) - hold the same state and receive the same
 * calls with the same arguments.  From then on cc_online_run, cc_offline and cc_assoc_argmin are collective:
 *   - the snapshot scan of a window (the loop of hddstream.py:311-328 / :371-375 over the microclusters) is
 *     split by table rows; the ranks all-gather one 64-byte candidate record per window point and every rank
 *     validates and commits the window redundantly and deterministically, so all ranks end with bit-identical
 *     tables, labels and clusters - identical to what one GPU computes;
 *   - the pair matrices of the offline phase (predecon.py:161-188, :219-239) and of the association tracker
 *     (cluster_tracker.py:127-141) are split by rows and all-gathered.
 * Small tables are not split (cc_set_shard_thresholds): below ~1 ms of scan per window the exchange costs more
 * than it saves.
 *   cc_comm_unique_id  : rank 0 obtains the 128-byte RCCL id and hands it to the other ranks (any channel)
 *   cc_comm_init_rccl  : joins the group (collective; librccl is loaded here, not before).  One communicator
 *                        serves both HIP streams of the handle; CHRONOCLUST_HIP_TWO_COMMS=1 adds a second one for
 *                        the lookahead stream (its id travels through the first), so that the all-gathers of
 *                        lookahead scans are not ordered with those of the validation stream - opt-in until a
 *                        multi-GPU run has confirmed it.  No wait for a collective is unbounded: host waits
 *                        poll ncclCommGetAsyncError and a deadline (CHRONOCLUST_HIP_COMM_TIMEOUT_S, default
 *                        120 s); on an error, a missed deadline or any failing call of a member the
 *                        communicators are aborted (ncclCommAbort) and calls return CC_ERR_COMM
 *   cc_comm_init_local : the in-process group of handles[0..world)
 *   cc_comm_info       : transport 0 none, 1 RCCL, 2 local */
#define CC_COMM_ID_BYTES 128
int cc_comm_unique_id(void* out_id);
int cc_comm_init_rccl(cc_handle* h, const void* id_bytes, int rank, int world);
int cc_comm_init_local(cc_handle** handles, int world);
/* Collective (every rank of the group, after joining it; cc_comm_init_rccl calls it itself unless
 * CHRONOCLUST_HIP_CALIBRATE=0; the members of an in-process group call it from their own threads): MEASURES what the split of
 * the snapshot scans over the ranks costs and what it saves, and derives the split thresholds from the measurement instead of
 * a constant -
 *   - three all-gathers of one full window's candidate records (64 B per point and rank) on the handle's stream: the exchange
 *     a split window pays, `calib_allgather_us` (minimum of the three);
 *   - three plain snapshot scans (k_scan_u) of a full window over 4 096 synthetic rows x 20 dimensions on scratch buffers:
 *     what a row costs, `calib_scan_ns_per_row_dim`;
 *   - both figures are exchanged and every rank takes the group's MAXIMUM, so that all ranks derive the same thresholds (they
 *     decide the sequence of collectives): a plain scan is split from rows x d >= allgather x world / (world - 1) / scan per
 *     (row, dim) on - where the time saved, scan x (1 - 1 / world), equals the exchange -, a pruned chain from 3.3 times
 *     that (it spends 0.3 of a plain scan's time on the same rows: 92 against 306 us per full window at 5 000 x 20).
 * A group of ONE rank measures and reports but keeps its thresholds (there is nothing to save; one-rank groups exist to
 * exercise the transport).  cc_set_shard_thresholds afterwards overrides both thresholds.  cc_get_stats reports all four. */
int cc_comm_calibrate(cc_handle* h);
int cc_comm_destroy(cc_handle* h);
int cc_comm_info(cc_handle* h, int32_t* rank, int32_t* world, int32_t* transport);
/* RELAXED multi-GPU mode - not the reference's semantics.  The events of a timepoint are sharded over the ranks in
 * contiguous blocks (what BASELINE.json's north_star sketches: "events within a timestep shard across the GPUs with
 * an RCCL all-reduce of the per-MC CF-vector deltas").  Per super-step every rank clusters `minibatch_points` of its
 * block against the table all ranks share (exact path, but a point that no MC absorbs is set aside instead of
 * creating one), the CF1 / CF2 / weight changes of the existing rows are all-reduced and written back with centroids
 * and preferred dimensions recomputed and promotions decided on the merged rows, and the set-aside points of all
 * ranks are clustered on every rank redundantly (exact path), so that new MCs are created once and all ranks keep
 * identical tables.  Within a super-step a rank does not see the other ranks' adds: labels, ids and CF sums differ
 * from the reference's; bench.py reports the agreement with the exact path beside the number.  Every rank must hold
 * the whole timepoint (cc_points_upload of the same array); cc_labels_download returns all labels on every rank
 * (path code 8 never remains: set-aside points are labelled by the second half of their super-step).
 * minibatch_points = 0 switches back to the exact path. */
int cc_comm_set_relaxed(cc_handle* h, int32_t minibatch_points);
typedef struct cc_relaxed_stats {
    int64_t super_steps;       /* of the last cc_online_run                                   */
    int64_t minibatch_points;  /* points this rank clustered in the sharded halves             */
    int64_t deferred_points;   /* set-aside points (all ranks) clustered in the replicated halves */
    int64_t reserved[5];
} cc_relaxed_stats;
int cc_get_relaxed_stats(cc_handle* h, cc_relaxed_stats* out);
/* The block [lo, hi) of n rows rank `rank` of `world` takes, in whole units of `unit` rows: the partition every
 * kernel of the multi-GPU path uses (unit 1: table rows of a scan, current pcores of the association argmin;
 * 64: rows of the offline pair matrices).  Pure host arithmetic, needs no handle and no GPU. */
int cc_shard_rows(int32_t n, int32_t world, int32_t rank, int32_t unit, int32_t* lo, int32_t* hi);
/* split the scan when rows * d >= min_row_dims, the offline / association pair matrices when rows >=
 * offline_min_rows; a negative value keeps the current setting (defaults 400 000 and 8 192) */
int cc_set_shard_thresholds(cc_handle* h, int64_t min_row_dims, int32_t offline_min_rows);

/* The join of app.py:303-332 (write_datapoints_details walks the `points` dicts of every cluster's pcores): for every
 * resident point the index of the cluster (order of cc_clusters_export, after cc_offline) its microcluster belongs
 * to, -1 for points in outlier microclusters and in pcores outside every cluster (the literal `None` of app.py:396).
 * A gather on the device from the per-point labels through a creation-number -> cluster table. */
int cc_point_clusters(cc_handle* h, int32_t* out_idx);

/* Text of n rows of cluster_points_D{t}.csv as DataFrame.to_csv(index=False) writes them (app.py:357-360):
 * "<first_id + r>,<label>,<v[r,0]>,...,<v[r,d-1]>\n", floats as repr(float) (shortest round-trip digits, CPython's
 * layout rules).  label_idx[r] selects one of n_labels CSV-ready label texts (label_bytes[label_offsets[i] ..
 * label_offsets[i + 1])); an index outside [0, n_labels) selects the last one.  Pure host work, no handle: callers
 * format chunks of rows on several threads.  Returns the number of bytes written to out, or CC_ERR_OOM when `cap`
 * cannot hold them (25 + longest label + 33 d + 2 bytes per row always suffice). */
int64_t cc_format_points_csv(const double* values, int64_t n, int32_t d, int64_t first_id, const int32_t* label_idx,
                             const char* label_bytes, const int32_t* label_offsets, int32_t n_labels, char* out,
                             int64_t cap);

/* Waits until everything the handle has enqueued on its HIP streams is done (the timing bracket of a harness: what
 * torch.cuda.synchronize() would be for work a framework had launched).  Inside a group the wait is bounded like
 * every wait of the library that may hold a collective: CC_ERR_COMM when a peer is gone. */
int cc_sync(cc_handle* h);

int cc_get_stats(cc_handle* h, cc_stats* out);

/* The window policy of the exact online phase as a pure function (csrc/cc_policy.h; no reference counterpart): between
 * two batches of windows the library reads the device's counters and decides window size, validation rounds, windows per
 * batch, lookahead / dirty / pruned scans and the split over the ranks of a group.  No decision can change a result, but
 * the ranks of a group must all take the same ones, so they depend on the counters alone.  cc_policy_replay runs the
 * policy over recorded observations - no handle, no GPU: out[0] is the decision for the first batch of a call that
 * starts at (start_cursor, start_rows), out[i + 1] the one taken after obs[i] (obs[i].after_sequential != 0: the stream
 * came back from the sequential kernel at obs[i].cursor / m_rows instead of finishing a batch).  *carry is updated to
 * what the handle would keep for its next call.  CHRONOCLUST_HIP_POLICY_TRACE=<file> makes the library append the
 * observations and decisions of every call as JSON lines (how the traces under tests/golden/policy/ were recorded). */
#define CC_POLICY_MAX_ROUNDS 8
typedef struct cc_policy_config {
    int32_t window, rounds_max, windows_per_sync, early_window;  /* cc_tuning values in force                        */
    int32_t lookahead;         /* cc_tuning.lookahead                                                              */
    int32_t allow_nodirty;     /* dirty scans may be left out while ruled out (CHRONOCLUST_HIP_NODIRTY != 0)       */
    int32_t prune_mode;        /* CHRONOCLUST_HIP_PRUNE: 0 never, 1 while it pays, 2 always                        */
    int32_t prune_applicable;  /* k = 2^e, pi >= d and d one of the widths the pruned scan is compiled for         */
    int32_t can_shard;         /* the handle belongs to a group and is not inside a relaxed super-step             */
    int32_t d;
    int32_t resume;            /* the call continues a stream this handle was clustering a moment ago              */
    int32_t allow_sparse;      /* sparse dirty scans while at most one point in this many needs them (0: never)     */
    int32_t allow_guess;       /* pruned scans may take table-wide guessed thresholds (CHRONOCLUST_HIP_GUESS != 0); 1: and
                                  run lean - without the list of missed points - after a batch without a miss, 2: never lean */
    int32_t allow_probe;       /* pruned scans come back on a probe's word (CHRONOCLUST_HIP_PROBE != 0), else after a
                                * stretch of points that doubles with every failed try                               */
    int64_t shard_min_row_dims;
    int64_t n_end;             /* end of the range of points the call clusters                                     */
    int64_t shard_min_row_dims_pruned;  /* the split threshold while the scans are pruned chains (0: shard_min_row_dims)   */
    int32_t lookahead_pruned;  /* 1: lookahead scans also while the scans are pruned chains on one GPU (CHRONOCLUST_HIP_LA_PRUNED=1;
                                * round 6: off - such a scan is too short to be worth a stream of its own, cc_policy.h)        */
    int32_t force_prune_rows;  /* > 0: pruned scans whenever the table has at least this many rows, whatever the samples said (round
                                * 6: behind k_seed16's seeds and the tight threshold a pruned chain returns what the plain scan returns,
                                * and from a few thousand rows on at a fraction of its time - also while the table still fills)  */
} cc_policy_config;
typedef struct cc_policy_carry {
    int32_t adapt_win, clean_batches, since_shrink, pad;
} cc_policy_carry;
typedef struct cc_policy_obs {   /* cumulative device counters of the call as read back after a batch              */
    int64_t cursor;
    int32_t m_rows, stall_b;
    int64_t stat_windows, stat_truncated, stat_trunc_unknown, stat_tiles, stat_dirty_tiles;
    int64_t stat_unsafe;       /* (point, round) pairs that needed rows only a dirty scan covers                  */
    int64_t stat_missed;       /* points a guessed threshold missed (the seeded chain ran for them)               */
    int64_t round_hist[CC_POLICY_MAX_ROUNDS + 2];
    uint64_t prune_rows, prune_full;
    int32_t after_sequential;
    int32_t tg_ok;             /* a mean join distance exists: guessed thresholds are available                   */
} cc_policy_obs;
typedef struct cc_policy_decision {
    int32_t win_cfg;        /* window size of the next batch (changes only with `restart`)                         */
    int32_t want;           /* the size the policy is heading for                                                  */
    int32_t rounds, batch_windows, lookahead, nodirty;
    int32_t prune;          /* 0: plain scans, 1: pruned with seeded thresholds, 2: pruned with guessed thresholds,
                             * 3: guessed thresholds, lean (no list of missed points, no seeded chain behind the scan) */
    int32_t shard;
    int32_t restart;        /* the chain of windows restarts: pending lookahead scan dropped, control block pushed */
    int32_t bad;            /* short, truncated windows at a small window size (input of the sequential-kernel rule) */
    int32_t stalled;        /* five batches without progress: the call fails with CC_ERR_INTERNAL                  */
    int32_t sparse;         /* with nodirty: the sparse dirty scans run for the points that need rows of their own  */
    int32_t probe;          /* plain scans, and the pruned chain runs beside the batch's first one on 128 points: its
                             * sample tells the policy whether pruned scans would pay, at 1 / 256 of a scan's cost    */
    int32_t pad;
    int64_t wins, pts, trunc, unk, tiles, dtiles, grew, prune_rows, prune_full;  /* what the batch did (deltas)     */
} cc_policy_decision;
int cc_policy_replay(const cc_policy_config* cfg, cc_policy_carry* carry, int64_t start_cursor, int32_t start_rows,
                     const cc_policy_obs* obs, int32_t n, cc_policy_decision* out);
/* The one wall-clock rule of the library (a stream of short, truncated windows is handed to the sequential kernel when that
 * is faster) compares the windows' measured rate with an ASSUMED rate of the sequential kernel until that has been measured
 * in the call: points per millisecond, as a function of the dimensionality and of the table size - k_seq_g, the kernel for
 * tables beyond the LDS image, slows down in proportion to the rows once they exceed its 1 024 threads.  Pure; < 0 on a
 * bad argument.  No reference counterpart. */
double cc_policy_seq_rate_guess(int32_t d, int32_t m_rows, int32_t allow_seq_r, int32_t allow_seq_g);
/* The rule itself (csrc/cc_policy.h, cc::SeqHandover) is pure: the library measures with its clock and hands the rates in.
 * cc_seq_handover_replay runs it over recorded events - no handle, no GPU, no clock.  outcome[0] / stint_len[0]: whether a call
 * in `mode` (cc_tuning.sequential; 2 also beyond CC_WINDOW_MAX_DIM) starts on the sequential kernel, and the length of its next
 * stint; outcome[i + 1] / stint_len[i + 1] after ev[i] - a batch of windows: 1 when the next iteration is a stint of the
 * sequential kernel; a chunk of the sequential kernel: 0 the stint continues, 1 back to the windows for one batch that is
 * measured against the stint (a probe), 2 back to the windows for good. */
typedef struct cc_seq_event {
    int32_t chunk_event;    /* 0: a batch of windows has been read back, 1: a chunk of the sequential kernel has run            */
    int32_t bad;            /* batch: cc_policy_decision.bad                                                                */
    int32_t possible;       /* the sequential kernel may run now: no group, points create, the table fits or k_seq_g is allowed */
    int32_t more;           /* points of the call are left                                                                  */
    int32_t seq_r_applies;  /* batch: the register kernel would take over (d = 2 .. 4 and allowed)                           */
    int32_t use_g;          /* chunk: k_seq_g ran it                                                                        */
    int32_t allow_seq_g, wide;  /* chunk: k_seq_g is allowed / more than CC_WINDOW_MAX_DIM dimensions (no windows to go back to) */
    int64_t got, chunk;     /* chunk: points it committed / was given                                                       */
    double rate;            /* points per millisecond measured: of the batch (<= 0: none, the last one stands) / of the chunk */
    double rate_guess;      /* batch: cc_policy_seq_rate_guess for the table as it is                                       */
} cc_seq_event;
int cc_seq_handover_replay(int32_t mode, int32_t possible, int32_t sticky, const cc_seq_event* ev, int32_t n, int32_t* outcome,
                           int64_t* stint_len);

/* How one batch of windows is launched (csrc/cc_batch.h; no reference counterpart): grids, partials per point, which kernels
 * gather the claims and replay the long chains - a pure function of the handle's settings and of what the last read-back of the
 * control block said, the same on every rank of a group.  cc_batch_plan computes it without a handle or a GPU. */
typedef struct cc_batch_inputs {
    int32_t window, win_cfg;   /* the configured window / the window size of this batch (Ctl::win_cfg)                       */
    int32_t S_cfg;             /* partials per point as configured (segments / waves per workgroup)                          */
    int32_t n_cus, prune_now;  /* CUs of the device / this batch's snapshot scans are pruned chains                          */
    int32_t prune_wgs_per_cu, plain_wgs_per_cu;  /* resident workgroups per CU of the scan plan's kernels                    */
    int32_t decide_threads, chain_threads, commit_threads;
    int32_t allow_claims, allow_long, allow_heavy, allow_prep;
    int32_t m_rows, n_heavy;   /* table rows / heavy rows as last read back                                                 */
    int32_t long_seen, long_few;  /* the previous batch had long chains / no more than 64 per validation round              */
    int64_t long_avg;          /* ... its average per round, + 1                                                            */
    int32_t batch_windows, pad;
    int64_t points_left;
} cc_batch_inputs;
enum { CC_LONG_NONE = 0, CC_LONG_ROWS_SPLIT = 1, CC_LONG_ROWS_SMALL = 2, CC_LONG_LIST_SPLIT = 3, CC_LONG_LIST_SMALL = 4 };
typedef struct cc_batch_geometry {
    int32_t gw;                /* points the grids cover: the window size of the batch, at least 64                          */
    int32_t S;                 /* partials per point of the batch's snapshot scans                                          */
    int32_t sparse_cap;        /* capacity of a round's list for the sparse dirty scans                                      */
    int32_t dblocks, cblocks, rblocks;  /* workgroups of k_decide, k_chain, k_commit_b                                      */
    int32_t scan_rows;         /* > 0: k_claims gathers the claims of these table rows                                       */
    int32_t long_rows;         /* > 0: k_chain_long runs one workgroup per table row                                         */
    int32_t long_listed;       /* k_chain_long runs over the list k_decide keeps                                            */
    int32_t heavy_on;          /* k_claims_heavy gathers the claims of the heavy rows                                        */
    int32_t long_cap;          /* entries k_decide may list per round = workgroups of the listed launches                    */
    int32_t windows_now;       /* windows to enqueue                                                                        */
    int32_t prep;              /* k_chain_long<.., PREP> runs ahead of k_chain                                               */
    int32_t prep_form;         /* ... CC_LONG_ROWS_SPLIT or CC_LONG_LIST_SPLIT (CC_LONG_NONE without prep)                    */
    int32_t long_form;         /* CC_LONG_*: the k_chain_long launch behind k_chain                                          */
    int32_t pad;
} cc_batch_geometry;
int cc_batch_plan(const cc_batch_inputs* in, cc_batch_geometry* out);

/* Which snapshot scans serve a stream of d dimensions (csrc/cc_batch.h, cc::scan_width; no reference counterpart), before any
 * CHRONOCLUST_HIP_* knob: the width the scan kernels run at (the smallest compiled one >= d: 4, 8, 14, 16, 20, 32, 40, 64),
 * whether the plain scan is the scalar-operand kernel (k a power of two, no pdim filter; at a compiled width, or from nine
 * dimensions on over padded operands) and which pruned chain exists.  No handle, no GPU.  CC_ERR_BAD_ARG unless
 * 1 <= d <= CC_MAX_DIM. */
enum { CC_CHAIN_NONE = 0, CC_CHAIN_COMMON = 1, CC_CHAIN_GENERAL = 2 };
int cc_scan_width(int32_t d, int32_t filter_on, int32_t k_pow2, int32_t* padded, int32_t* scan_u, int32_t* chain);

#ifdef __cplusplus
}
#endif
#endif
