// cc_api.hip — host side of the C-ABI declared in include/chronoclust_hip.h, the one translation unit of the library.
// The handle owns the HBM-resident state (microcluster table, window buffers, points, labels) and enqueues the gfx950
// kernels of cc_online.h / cc_offline.h on its HIP streams.  No CPU fallback exists for any kernel.
// Here: the snapshot scan's plan and dispatcher, the handle's life cycle and settings, the online and table entry points.
// Beside it, included below: cc_handle.h (the handle, its buffers and helpers; cc_knobs.h, cc_ingest_src.h), cc_online_run.h
// (one online call), cc_api_points.inc, cc_api_views.inc, cc_api_list.inc, cc_api_ingest.inc (the one upload, prefetch and
// column reduction behind those three), cc_api_offline.inc, cc_api_comm.inc and cc_api_assign.inc (the other entry points, by
// concern).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <optional>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/chronoclust_hip.h"
#include "cc_comm.h"
#include "cc_common.h"
#include "cc_csv.h"
#include "cc_offline.h"
#include "cc_online.h"
#include "cc_assign.h"
#include "cc_policy.h"
#include "cc_batch.h"

#include "cc_handle.h"  // (behind the kernels' headers: its buffers are typed by their records)

namespace {

// ---- scan dispatch over the padded dimensionality ---------------------------------

// From here to launch_scan: the scan plan, the launch helpers and the dispatcher - the host code that sets the snapshot
// scan's launch geometry (bench.py's scan_digest() hashes this text)
template <int DP, bool DIRTY>
void launch_scan_dp(cc_handle* h, hipStream_t st, int win, Rows rows, const Cand* clean, Cand* part, int S, int round,
                    int mode, int shard_rank, int shard_world, int phase);

// workgroups per CU of k_scan_u that are resident at once (what it is compiled for if the runtime does not say)
template <int DP>
int scan_u_wgs_per_cu()
{
    constexpr int NW = ScanShape<DP, false>::NW;
    static int blocks = 0;
    static const bool ok = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_scan_u<DP, NW>, 64 * NW, 0) == hipSuccess && blocks >= 1;
    return ok ? blocks : ScanUShape<DP>::WGS;
}

template <int DP>
ScanPlan scan_plan_dp(const cc_handle* h)
{
    ScanPlan p;
    p.dp = DP;
    // which scans exist at this width for this pdim filter and k (cc::scan_width, cc_batch.h), the knobs on top: the common
    // case (k a power of two, no pdim filter) has the rows as scalar operands - padded ones where d is no compiled width
    const cc::ScanWidth w = cc::scan_width(h->d, h->hc.filter != 0, h->hc.pow2 != 0);
    p.scan_u = h->allow_scan_u && w.scan_u;
    p.pad_rows = p.scan_u && h->d != DP;
    if (p.scan_u && w.chain == CC_CHAIN_COMMON) p.chain = ScanPlan::COMMON;
    // (no pruned chain on a tainted handle: phase A bounds a row's distance from below with min(1, 1 / k) as the smallest weight
    // of a dimension, phase B divides by the stored entry - one above max(k, 1) weighs less, and "abandoned implies beyond T"
    // no longer holds.  Taint has cleared pow2, so the common chain is gone already.)
    else if (h->allow_scan_p3 && h->allow_prune_general && !h->tainted && w.chain == CC_CHAIN_GENERAL) p.chain = ScanPlan::GENERAL;
    // the window's pruned scan: phase A on the matrix cores (k_scan_p3; GENERAL needs it), two points per lane (k_scan_p2) or
    // one (k_scan_p); CHRONOCLUST_HIP_SCANA: 0 never the split form, 2 always (even over k_scan_p3), 1 from 10 000 table rows
    // on where k_scan_p3 does not run.  The GENERAL chain is never split.
    const bool p3 = h->allow_scan_p3 && DP <= 40;
    p.form = p3 ? ScanPlan::P3 : (h->allow_scan_p2 && DP <= 40 ? ScanPlan::P2 : ScanPlan::P1);
    if (p.chain == ScanPlan::COMMON && h->split_a_mode == 2) p.split_rows = 0;
    else if (p.chain == ScanPlan::COMMON && h->split_a_mode == 1 && !p3) p.split_rows = 10000;
    p.listed_rows = h->p3_listed_rows;
    // (k_scan_p3 as SCANA sees it, on the GENERAL chain too: where the seeds come from the matrix cores, the pruned partials)
    const bool p3_sized = p3 && h->split_a_mode != 2;
    p.seed16 = h->allow_seed16 && (p.chain == ScanPlan::GENERAL || p3_sized);
    p.prune_applicable = p.chain != ScanPlan::NONE ? 1 : 0;
    // (GENERAL: seeded thresholds only - the points a guessed threshold misses would need a plain scan over a point list, which
    // exists for the common case alone (k_scan_u) -, no probes)
    p.allow_guess = (h->allow_guess && p.chain != ScanPlan::GENERAL) ? (h->allow_lean ? 1 : 2) : 0;  // (2: guessed thresholds, never lean)
    p.allow_probe = (h->allow_probe && p.chain != ScanPlan::GENERAL) ? 1 : 0;
    // (pruned scans from this many rows on whatever the phase: where the seeded chain runs behind k_seed16)
    p.force_prune_rows = (p.prune_applicable && h->allow_seed16 && p3_sized) ? h->force_prune_rows : 0;
    p.waves = ScanShape<DP, false>::NW;
    p.dirty_waves = ScanShape<DP, true>::NW;
    p.plain_wgs_per_cu = p.scan_u ? scan_u_wgs_per_cu<DP>() : ScanShape<DP, false>::WGS;
    // (measured, `profiles/r03_tool_prune_split.txt`: four rounds of the resident workgroups at d <= 20 - k_scan_p is
    // compiled for four per CU there -, eight of the three per CU beyond)
    // (round 6, k_scan_p3: the prefix test costs next to nothing on the matrix cores, what is left of a workgroup's time is its
    // prologue - the points staged, their constants - and the rows it completes: two rounds of the resident workgroups at
    // d <= 20, 54 against 63 us per C2 window running alone, half the partials per point)
    p.prune_wgs_per_cu = h->prune_rounds4 > 0 ? h->prune_rounds4 : (DP <= 20 ? (p3_sized ? 8 : 16) : 24);
    return p;
}

ScanPlan scan_plan(const cc_handle* h)
{
    switch (cc::scan_width(h->d, false, false).padded) {  // (the width is a function of d alone)
    case 4: return scan_plan_dp<4>(h);
    case 8: return scan_plan_dp<8>(h);
    case 14: return scan_plan_dp<14>(h);
    case 16: return scan_plan_dp<16>(h);
    case 20: return scan_plan_dp<20>(h);
    case 32: return scan_plan_dp<32>(h);
    case 40: return scan_plan_dp<40>(h);
    default: return scan_plan_dp<64>(h);
    }
}

// The clean scan's launches at padded width DP, one helper per kernel family: the window's `win` points, S partials per
// point into `part` (at the handle's part_stride), or lists of points
template <int DP>
struct ScanCall {
    static constexpr int NW = ScanShape<DP, false>::NW;
    cc_handle* h; hipStream_t st; const Rows& rows;
    int round, mode, win, S;
    Cand* part;

    // k_scan_u over the window (n_pts = win, plist == nullptr) or a list
    void scan_u(int n_pts, int srank, int sworld, const int* plist) const
    {
        hipLaunchKernelGGL((k_scan_u<DP, NW>), dim3((n_pts + 63) / 64, S), dim3(64 * NW), 0, st, h->ctl.p, h->Xt.p, rows.cen,
                           rows.scl, rows.kind, rows.key, part, round, mode, h->part_stride, srank, sworld, plist);
    }
    // the rows as half-precision operands of the MFMA prefix test (k_scan_p3, k_seed16)
    void prefix16() const
    {
        ensure_prefix16(h);
        const size_t a16_rows = h->tab.cap + 2 * CC_P16_TM;
        hipLaunchKernelGGL((k_prefix16<DP>), dim3((unsigned)((a16_rows + 255) / 256)), dim3(256), 0, st, (const Ctl*)h->ctl.p,
                           rows.cen, rows.kind, h->a16.p, h->hdr16.p, h->a16_stride, round, mode);
    }
    // seeds for n_pts points of the window or a list, Sp partials per point - k_seed (two points per lane: point tiles of 128)
    // or from the matrix cores (k_seed16, behind prefix16()) -, then the thresholds (k_seed_merge: F x the nearest seed; the
    // tight one, F <= 0, behind k_seed16)
    void seeds(int n_pts, int Sp, const int* plist, bool s16) const
    {
        const dim3 grid((n_pts + 127) / 128, Sp), block(64 * NW);
        if (s16) {
            if constexpr (DP <= 40) {
                hipLaunchKernelGGL((k_seed16<DP, NW>), grid, block, 0, st, (const Ctl*)h->ctl.p, (const double*)h->Xt.p, rows.cen, h->spart.p,
                                   round, mode, h->spart_stride, (const cc_h8*)h->a16.p, (const Prefix16Hdr*)h->hdr16.p, h->a16_stride);
                ++h->stats.seed16_launches;
            } else {
                throw HipErr{hipErrorInvalidValue, "k_seed16 is compiled up to 40 dimensions"};
            }
        } else {
            hipLaunchKernelGGL((k_seed<DP, NW>), grid, block, 0, st, h->ctl.p, h->Xt.p, rows.cen, rows.kind, h->spart.p, round, mode,
                               h->spart_stride, h->cmax.p, plist);
        }
        hipLaunchKernelGGL((k_seed_merge<DP>), dim3((2 * n_pts + 63) / 64), dim3(64), 0, st, h->ctl.p, h->X.p, rows.cen, rows.scl, h->spart.p,
                           h->spart_stride, Sp, h->thr.p, h->thr32.p, h->thr_stride, s16 ? 0.0 : h->prune_F, round, mode, h->cmax.p,
                           h->pstat_p(), plist, h->d);
    }
    // k_scan_p3 over the window (behind prefix16()); GENERAL evaluates the pdim filter (lazily, for rows that would enter a
    // list) and divides by k itself
    template <bool LISTED, bool GENERAL>
    void scan_p3(unsigned lds, int srank, int sworld, double gF, unsigned long long* found) const
    {
        hipLaunchKernelGGL((k_scan_p3<DP, NW, LISTED, GENERAL>), dim3((win + 127) / 128, S), dim3(64 * NW), lds, st, h->ctl.p, h->Xt.p,
                           rows.cen, rows.scl, rows.kind, rows.key, h->thr.p, h->thr_stride, part, round, mode, h->part_stride, srank,
                           sworld, h->pstat_p(), gF, found, (const cc_h8*)h->a16.p, (const Prefix16Hdr*)h->hdr16.p, h->a16_stride,
                           GENERAL ? (const double*)h->X.p : nullptr, GENERAL ? rows.cf1 : nullptr, GENERAL ? rows.cf2 : nullptr,
                           GENERAL ? rows.w : nullptr);
    }
    // k_scan_p, one point per lane with phase A inside: n_pts points of the window or a list, Sp partials per point into p
    void scan_p(int n_pts, int Sp, Cand* p, size_t p_stride, int srank, int sworld, const int* plist, double gF,
                unsigned long long* found) const
    {
        hipLaunchKernelGGL((k_scan_p<DP, NW, false>), dim3((n_pts + 63) / 64, Sp), dim3(64 * NW), 0, st, h->ctl.p, h->Xt.p, rows.cen,
                           rows.scl, rows.kind, rows.key, h->thr.p, h->thr32.p, h->thr_stride, p, round, mode, p_stride, srank, sworld,
                           h->pstat_p(), plist, gF, found, (const unsigned*)nullptr, (size_t)0, 0, 1);
    }
    // the window's pruned scan as two kernels: phase A (k_scan_a: two points per lane, survivor masks), phase B behind it
    void scan_split(int srank, int sworld, double gF, unsigned long long* found) const
    {
        const int nsub = S * NW;
        const int tps = cc_mask_tiles_per_sub((int)std::min<size_t>(h->tab.cap, (size_t)INT_MAX - 64), nsub);
        const size_t need = (size_t)((win + 127) / 128) * (size_t)nsub * (size_t)tps;
        if (need > h->mask_stride) { h->masks.ensure(2 * need); h->mask_stride = need; }
        hipLaunchKernelGGL((k_scan_a<DP, NW>), dim3((win + 127) / 128, S), dim3(64 * NW), 0, st, (const Ctl*)h->ctl.p,
                           (const double*)h->Xt.p, rows.cen, rows.kind, (const double*)h->thr.p, h->thr_stride, h->masks.p,
                           h->mask_stride, tps, round, mode, srank, sworld, gF);
        // phase B: about one and a half rounds of the resident workgroups, i.e. q of phase A's sub-ranges per wave
        // (its waves live on chains of memory round trips - prologue, masks, a few rows, merge -, not on arithmetic:
        // with phase A's own split - eight rounds at the C5 shape - the prologues dominate, with one round every
        // wave walks q times the rows; 2 M x 40, 50 000 rows: q = 1 / 2 / 3 / 4 / 6 / 12 -> 39.6 / 40.6 / 40.7 /
        // 41.2 / 39.9 / 39.8 M points/s.  CHRONOCLUST_HIP_SCANB_Q overrides.)
        int q = 1;
        const int tiles = (win + 63) / 64;
        const int resident = h->n_cus * (DP <= 20 ? CC_SCANP_WGS20 : (DP <= 40 ? 3 : 2));
        for (int c = 1; c <= S; ++c)
            if (S % c == 0 && 2 * tiles * (S / c) >= 3 * resident) q = c;
        static const int q_env = []() { const char* e = getenv("CHRONOCLUST_HIP_SCANB_Q"); return e ? atoi(e) : 0; }();
        if (q_env > 0 && S % q_env == 0) q = q_env;
        hipLaunchKernelGGL((k_scan_p<DP, NW, true>), dim3(tiles, S / q), dim3(64 * NW), 0, st, h->ctl.p, h->Xt.p, rows.cen, rows.scl,
                           rows.kind, rows.key, h->thr.p, h->thr32.p, h->thr_stride, part, round, mode, h->part_stride, srank, sworld,
                           h->pstat_p(), (const int*)nullptr, gF, found, (const unsigned*)h->masks.p, h->mask_stride, tps, q);
    }
};

template <int DP, bool DIRTY>
void launch_scan_dp(cc_handle* h, hipStream_t st, int win, Rows rows, const Cand* clean, Cand* part, int S, int round,
                    int mode, int shard_rank, int shard_world, int phase)
{
    constexpr int NW = ScanShape<DP, DIRTY>::NW;
    const dim3 block(64 * NW);
    constexpr int TILE = 64 * ScanShape<DP, DIRTY>::PT;  // window points per workgroup
    const dim3 grid((win + TILE - 1) / TILE, S);
    if constexpr (!DIRTY) {
        static_assert(ScanShape<DP, false>::PT == 1, "k_scan_u holds one window point per lane");
        const ScanPlan& pl = h->scan_plan;
        const ScanCall<DP> L{h, st, rows, round, mode, win, S, part};
        if (pl.scan_u) ++h->stats.scan_u_launches;  // (every window where k_scan_u applies, pruned or not)
        if constexpr (DP > 8) {
            // prefix scores -> thresholds -> the scan that abandons rows whose partial sums pass them.  The window's pruned
            // scan, against guessed thresholds (gF > 0; `found`: who found a pcore MC, per point tile) or seeded ones:
            auto window_scan = [&](int srank, int sworld, double gF, unsigned long long* found, bool have_prefix16) {
                if (pl.split(h->hc.m_rows)) return L.scan_split(srank, sworld, gF, found);
                if constexpr (DP <= 40) {
                    if (pl.form == ScanPlan::P3) {
                        if (!have_prefix16) L.prefix16();
                        // (LISTED: the kept rows listed per wave and walked with their operands prefetched)
                        const bool listed = pl.listed(h->hc.m_rows);
                        if (pl.chain == ScanPlan::GENERAL) {
                            if (listed) L.template scan_p3<true, true>(0, srank, sworld, gF, found);
                            else L.template scan_p3<false, true>(0, srank, sworld, gF, found);
                        } else {
                            // (unused dynamic LDS caps the workgroups a CU holds: CHRONOCLUST_HIP_SCAN_LDS_KB, an experiment knob)
                            static const char* const lds_kb = getenv("CHRONOCLUST_HIP_SCAN_LDS_KB");
                            static const unsigned p3_lds = lds_kb ? (unsigned)atoi(lds_kb) * 1024u : 0u;
                            if (listed) L.template scan_p3<true, false>(p3_lds, srank, sworld, gF, found);
                            else L.template scan_p3<false, false>(p3_lds, srank, sworld, gF, found);
                        }
                        ++h->stats.scan_p2_launches;
                        return;
                    }
                    if (pl.form == ScanPlan::P2) {  // (one kernel, two points per lane in phase A, phase B from the same residency)
                        hipLaunchKernelGGL((k_scan_p2<DP, NW>), dim3((win + 127) / 128, S), block, 0, st, h->ctl.p, h->Xt.p, rows.cen, rows.scl,
                                           rows.kind, rows.key, h->thr.p, h->thr_stride, part, round, mode, h->part_stride, srank, sworld,
                                           h->pstat_p(), gF, found);
                        ++h->stats.scan_p2_launches;
                        return;
                    }
                }
                L.scan_p(win, S, part, h->part_stride, srank, sworld, nullptr, gF, found);
            };
            // seeds and thresholds, then the pruned scan, for n_pts points of the window or a list (plist), Sp partials per point
            // into p.  (Split over the ranks of a group: seeds and thresholds over ALL rows on every rank - replicated, so that
            // every rank abandons against the same T -, phases A / B over the rank's own rows.)
            auto seeded_chain = [&](int n_pts, const int* plist, Cand* p, size_t p_stride, int Sp, int srank, int sworld) {
                const bool whole_window = plist == nullptr && n_pts == win && p_stride == h->part_stride && Sp == S;
                // (the rows' half-precision records first where k_seed16 or GENERAL's k_scan_p3 read them: they serve both)
                const bool s16 = whole_window && pl.seed16;
                const bool have_prefix16 = whole_window && (s16 || pl.chain == ScanPlan::GENERAL);
                if constexpr (DP <= 40) if (have_prefix16) L.prefix16();
                L.seeds(n_pts, Sp, plist, s16);
                if (whole_window) window_scan(srank, sworld, 0.0, nullptr, have_prefix16);
                else L.scan_p(n_pts, Sp, p, p_stride, srank, sworld, plist, 0.0, nullptr);
            };
            // the points a guessed threshold missed: the plain scan over their list (k_scan_u's header says why); the seeded
            // chain on request (CHRONOCLUST_HIP_MISSED_PLAIN=0)
            auto missed_scan = [&](const int* list) {
                if (!h->allow_missed_plain) return seeded_chain(CC_MISSED_CAP, list, part, h->part_stride, S, shard_rank, shard_world);
                ++h->stats.missed_plain_launches;
                L.scan_u(CC_MISSED_CAP, shard_rank, shard_world, list);
            };
            if (pl.chain == ScanPlan::GENERAL && h->prune_now && phase == 0) {
                ++h->stats.scan_p_launches;
                return seeded_chain(win, nullptr, part, h->part_stride, S, shard_rank, shard_world);
            }
            if (pl.chain == ScanPlan::COMMON) {
                if (phase == 1) {
                    // guessed thresholds on the exact multi-GPU path, after the ranks' records were gathered: the points
                    // whose merged pcore list starts with a bound (k_missed_g: the same list on every rank) go through the
                    // seeded chain - seeds over all rows on every rank, phases A / B over the rank's rows
                    hipLaunchKernelGGL(k_missed_g, dim3(1), dim3(1024), 0, st, h->ctl.p, (const Cand*)h->gpart.p, h->gpart_stride,
                                       (size_t)win * 4 + 4, shard_world, h->missed.p, CC_MISSED_CAP, round, mode, h->found.p);
                    return missed_scan(h->missed.p);
                }
                if (!h->prune_now) {
                    L.scan_u(win, shard_rank, shard_world, nullptr);
                    if (!h->probe_now) return;
                    // the probe: the pruned chain on the window's first 128 points, over all rows (the whole table on every
                    // rank: the same sample everywhere), into scratch partials - only its sample of completed rows
                    // (Ctl::stat_prune_*) is used, by the window policy.  (Few points, so many sub-ranges of rows: while the
                    // table fills most rows are completed, at the latency of scalar loads - 128 workgroups per point tile keep
                    // that to a hundred rows per wave.)
                    ++h->stats.probe_launches;
                    const int Sp = (int)std::max<size_t>(1, std::min<size_t>(128, h->spart_stride / 2 / 128));  // (what the seed buffer holds for 128 points)
                    h->probe_part.ensure((size_t)2 * 128 * Sp * 4);
                    return seeded_chain(std::min(win, 128), nullptr, h->probe_part.p, (size_t)128 * Sp * 4, Sp, 0, 1);
                }
                ++h->stats.scan_p_launches;
                if (!h->guess_now) return seeded_chain(win, nullptr, part, h->part_stride, S, shard_rank, shard_world);
                ++h->stats.scan_g_launches;
                unsigned long long* const found = h->lean_now ? nullptr : h->found.p;
                if (h->group_guess_now) {
                    // (split over ranks: every rank scans its rows against the same guess; who was missed is only known
                    // once the records are gathered - phase 1, enqueued by the caller behind the all-gather)
                    hipLaunchKernelGGL(k_pstat_zero, dim3(1), dim3(2), 0, st, (const Ctl*)h->ctl.p, h->pstat_p(), round, mode);
                    return window_scan(shard_rank, shard_world, h->prune_F, found, false);
                }
                // guessed thresholds: one scan, the list of the points it missed, the seeded chain for those (list of the
                // window's parity - the kernels take that half -: the lookahead scan of the next window fills the other one)
                window_scan(0, 1, h->prune_F, found, false);
                if (h->lean_now) { ++h->stats.scan_lean_launches; return; }  // (nobody is expected to be missed: see cc_policy.h)
                hipLaunchKernelGGL(k_missed, dim3(1), dim3(1024), 0, st, h->ctl.p, h->found.p, h->missed.p, CC_MISSED_CAP, round, mode);
                return missed_scan(h->missed.p);
            }
        }
        if (pl.scan_u) return L.scan_u(win, shard_rank, shard_world, nullptr);
    }
    // k_scan: the clean scan is compiled without the pdim filter for the common case pi >= d; the dirty scan (few rows
    // survive its pruning) tests the flag at run time
    const bool filter = DIRTY || h->hc.filter != 0;
#define CC_LAUNCH_SCAN(F, P) hipLaunchKernelGGL((k_scan<DP, F, P, DIRTY, NW>), grid, block, 0, st, h->ctl.p, h->X.p, h->Xt.p, rows, clean, \
                                          part, round, mode, h->part_stride, shard_rank, shard_world)
    if (filter) {
        if (h->hc.pow2) CC_LAUNCH_SCAN(true, true);
        else CC_LAUNCH_SCAN(true, false);
    } else if constexpr (!DIRTY) {
        if (h->hc.pow2) CC_LAUNCH_SCAN(false, true);
        else CC_LAUNCH_SCAN(false, false);
    }
#undef CC_LAUNCH_SCAN
}

// S = partials per point (workgroups per point tile); sub-ranges per tile = S * waves per workgroup.
// Clean scan: mode 0 = current window, 1 = lookahead (round = parity of that window's sequence number);
// dirty scan: mode 0 = version rows, 1 = carry set.
template <bool DIRTY>
void launch_scan(cc_handle* h, hipStream_t st, int win, Rows rows, const Cand* clean, Cand* part, int S, int round,
                 int mode, int shard_rank = 0, int shard_world = 1, int phase = 0)
{
#define CC_SCAN_DP(DP) return launch_scan_dp<DP, DIRTY>(h, st, win, rows, clean, part, S, round, mode, shard_rank, shard_world, phase)
    switch (h->scan_plan.dp) {
    case 4: CC_SCAN_DP(4);
    case 8: CC_SCAN_DP(8);
    case 14: CC_SCAN_DP(14);
    case 16: CC_SCAN_DP(16);
    case 20: CC_SCAN_DP(20);
    case 32: CC_SCAN_DP(32);
    case 40: CC_SCAN_DP(40);
    case 64: CC_SCAN_DP(64);
    }
    throw HipErr{hipErrorInvalidValue, "launch_scan before scan_plan() (OnlineRun::prepare)"};
#undef CC_SCAN_DP
}

// The rows of a snapshot scan where d is off the ladder (ScanPlan::pad_rows): k_pad_rows on the scan's stream, right in front
// of the scan and with its (round, mode), into the mirror of parity q - the window's parity, so that an in-place scan on the
// first stream and a lookahead scan on the second never share one.  Returns the view the scan chain walks: centroids and
// operands from the mirror, kinds and keys the source's.  (A full pass per scan, on purpose: nothing that changes the table
// in place between two scans has to know of the mirror.)
Rows padded_rows(cc_handle* h, hipStream_t st, Rows rows, int q, int round, int mode)
{
    const int dp = h->scan_plan.dp;
    ensure_pad_rows(h, dp);
    double* const cen = h->pad_cen.p + (size_t)q * h->pad_stride;
    double* const scl = h->pad_scl.p + (size_t)q * h->pad_stride;
    const dim3 grid((unsigned)((h->tab.cap * (size_t)(dp / 2) + 255) / 256));
#define CC_PAD_DP(DP) hipLaunchKernelGGL((k_pad_rows<DP>), grid, dim3(256), 0, st, (const Ctl*)h->ctl.p, rows.cen, rows.scl, cen, scl, \
                                         h->d, round, mode); break
    switch (dp) {
    case 14: CC_PAD_DP(14);
    case 16: CC_PAD_DP(16);
    case 20: CC_PAD_DP(20);
    case 32: CC_PAD_DP(32);
    case 40: CC_PAD_DP(40);
    case 64: CC_PAD_DP(64);
    default: throw HipErr{hipErrorInvalidValue, "padded_rows: no scan over padded operands at this width"};
    }
#undef CC_PAD_DP
    ++h->stats.pad_rows_launches;
    rows.cen = cen;
    rows.scl = scl;
    return rows;
}

}  // namespace

// one online call (OnlineRun, online_range), then the entry points by concern: points, point views, list-mode records, offline phase and
// tracker, multi-GPU,
// read-only assignment
#include "cc_online_run.h"
#include "cc_api_points.inc"
#include "cc_api_views.inc"
#include "cc_api_list.inc"
#include "cc_api_ingest.inc"
#include "cc_api_negq.inc"
#include "cc_api_offline.inc"
#include "cc_api_comm.inc"
#include "cc_api_assign.inc"

// =====================================================================================
// C-ABI
// =====================================================================================

extern "C" {

int cc_create(int device, cc_handle** out)
{
    if (!out) return CC_ERR_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return CC_ERR_NO_DEVICE;
    cc_handle* h = new (std::nothrow) cc_handle();
    if (!h) return CC_ERR_OOM;
    h->device = device;
    int rc = guarded(h, [&]() {
        // the validation kernels (first stream) are short latency chains, the lookahead scans (second stream) fill the
        // machine: when both have workgroups pending the validation ones go first
        int prio_lo = 0, prio_hi = 0;
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) h->n_cus = cus;
        int khz = 0;  // (what Ctl::scan_t0 / scan_t1 count in)
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0) h->wall_khz = khz;
        HIPCHK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        HIPCHK(hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, prio_hi));
        HIPCHK(hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, prio_lo));
        h->ctl.ensure(1);
        if (hipHostMalloc((void**)&h->hc_pin, 2 * sizeof(Ctl), hipHostMallocDefault) != hipSuccess) h->hc_pin = nullptr;
        h->badflag.ensure(4);
        memset(&h->hc, 0, sizeof(Ctl));
        // (round 6: the largest window - with the scans in place, what a window costs whatever its size (launches, prologues, the
        // validation kernels' chains of round trips: ~100 us) is a larger share of a shorter one: C2 13.98 -> 13.32 ms, the C5 shape
        // 75 -> 85 M points/s; the policy holds it at 32 768 while the table is small - cc_policy.h, `win`)
        h->tun.window = CC_MAX_WINDOW;
        h->tun.rounds = 3;
        h->tun.segments = 64;
        h->tun.windows_per_sync = 16;
        h->tun.time_kernels = 0;
        read_knobs(*h);
        push_ctl(h);
        sync_stream(h, h->stream);
        return CC_OK;
    });
    if (rc != CC_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return CC_OK;
}

void cc_destroy(cc_handle* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->pf.worker.joinable()) h->pf.worker.join();
    if (h->pf.stream) (void)hipStreamDestroy(h->pf.stream);
    if (h->hc_pin) (void)hipHostFree(h->hc_pin);
    for (int q = 0; q < 2; ++q)
        if (h->pf.pin[q]) (void)hipHostFree(h->pf.pin[q]);
    // (a pending collective whose peer is gone must not hang the destructor: bounded wait, then abort)
    auto drain = [&](hipStream_t st) {
        if (!st) return;
        try {
            if (h->comm.rccl() && !h->comm.broken) h->comm.wait_stream(st);
            else (void)hipStreamSynchronize(st);
        } catch (const cc::CommErr&) {
        }
    };
    drain(h->stream);
    drain(h->stream2);
    h->comm.destroy();
    if (h->stream) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipStreamDestroy(h->stream);
    }
    if (h->stream2) {
        (void)hipStreamSynchronize(h->stream2);
        (void)hipStreamDestroy(h->stream2);
    }
    for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->sync_pool) (void)hipEventDestroy(e);
    delete h;
}

const char* cc_last_error(const cc_handle* h) { return h ? h->err.c_str() : "null handle"; }

int cc_set_tuning(cc_handle* h, const cc_tuning* t)
{
    if (!h || !t) return CC_ERR_BAD_ARG;
    if (t->window > 0) h->tun.window = std::min(t->window, CC_MAX_WINDOW);
    if (t->rounds > 0) h->tun.rounds = std::min(t->rounds, CC_MAX_ROUNDS);
    if (t->segments > 0) h->tun.segments = std::min(t->segments, 1024);
    if (t->windows_per_sync > 0) h->tun.windows_per_sync = t->windows_per_sync;
    h->tun.time_kernels = t->time_kernels;
    if (t->dirty_segments > 0) h->tun.dirty_segments = std::min(t->dirty_segments, 1024);
    h->tun.lookahead = t->lookahead;
    h->tun.sequential = t->sequential;
    if (t->early_window > 0) h->tun.early_window = t->early_window;
    return CC_OK;
}

int cc_reset(cc_handle* h)
{
    if (!h) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() {
        Ctl& c = h->hc;
        c.m_rows = 0;
        c.n_pkeys = c.n_okeys = 0;
        c.pcore_last_id = c.outlier_last_id = 0;
        c.cursor = 0;
        h->tainted = false;
        h->adapt_win = 0;  // an empty table starts with small windows again
        h->seq_sticky = false;
        h->clean_batches = 0;
        h->since_shrink = 1000;
        h->clusters.clear();
        h->n_core = 0;
        refresh_ctl_params(h);
        push_ctl(h);
        sync_stream(h, h->stream);
        return (int)CC_OK;
    });
}

int cc_set_params(cc_handle* h, const cc_params* p)
{
    if (!h || !p) return CC_ERR_BAD_ARG;
    if (h->have_par && h->hc.m_rows > 0 && p->k != h->par.k) h->tainted = true;  // old rows keep their old k
    h->par = *p;
    h->have_par = true;
    refresh_ctl_params(h);
    return CC_OK;
}

int cc_dim(cc_handle* h) { return h ? h->d : CC_ERR_BAD_ARG; }

int cc_counters(cc_handle* h, int64_t* pcore_last_id, int64_t* outlier_last_id)
{
    if (!h) return CC_ERR_BAD_ARG;
    if (pcore_last_id) *pcore_last_id = h->hc.pcore_last_id;
    if (outlier_last_id) *outlier_last_id = h->hc.outlier_last_id;
    return CC_OK;
}

int cc_set_counters(cc_handle* h, int64_t pcore_last_id, int64_t outlier_last_id)
{
    if (!h || pcore_last_id < 0 || outlier_last_id < 0) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() {
        h->hc.pcore_last_id = pcore_last_id;
        h->hc.outlier_last_id = outlier_last_id;
        push_ctl(h);
        sync_stream(h, h->stream);
        return (int)CC_OK;
    });
}

int cc_online_run(cc_handle* h)
{
    if (!h) return CC_ERR_BAD_ARG;
    if (!h->have_par) return fail(h, CC_ERR_BAD_ARG, "cc_set_params has not been called");
    return guarded(h, [&]() {
        memset(&h->stats, 0, sizeof(h->stats));
        if (h->relaxed_minibatch > 0 && h->comm.active()) return online_relaxed(h);
        return online_range(h, 0, h->n_points, false, false);
    });
}

int cc_labels_download(cc_handle* h, int64_t* out_uid, int8_t* out_path)
{
    if (!h) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() {
        const size_t n = (size_t)h->n_points;
        if (n == 0) return (int)CC_OK;
        static_assert(sizeof(long long) == sizeof(int64_t), "int64");
        if (out_uid) HIPCHK(hipMemcpyAsync(out_uid, h->lab_uid.p, n * 8, hipMemcpyDeviceToHost, h->stream));
        if (out_path) HIPCHK(hipMemcpyAsync(out_path, h->lab_path.p, n, hipMemcpyDeviceToHost, h->stream));
        sync_stream(h, h->stream);
        return (int)CC_OK;
    });
}

int cc_online(cc_handle* h, const double* x, int64_t n, int32_t d, int64_t* out_uid, int8_t* out_path)
{
    int rc = cc_points_upload(h, x, n, d);
    if (rc != CC_OK) return rc;
    rc = cc_online_run(h);
    if (rc != CC_OK) return rc;
    return cc_labels_download(h, out_uid, out_path);
}

int cc_online_f32(cc_handle* h, const float* x, int64_t n, int32_t d, int64_t* out_uid, int8_t* out_path)
{
    int rc = cc_points_upload_f32(h, x, n, d);
    if (rc != CC_OK) return rc;
    rc = cc_online_run(h);
    if (rc != CC_OK) return rc;
    return cc_labels_download(h, out_uid, out_path);
}

int cc_count(cc_handle* h, int kind)
{
    if (!h) return CC_ERR_BAD_ARG;
    int n = 0;
    int rc = guarded(h, [&]() {
        RowList rl = list_order(h);
        n = (int)(kind == CC_PCORE ? rl.pcore.size() : rl.outlier.size());
        return (int)CC_OK;
    });
    return rc == CC_OK ? n : rc;
}

int cc_export(cc_handle* h, int kind, int64_t* id, int64_t* uid, double* w, double* cf1, double* cf2, double* cen,
              double* pref)
{
    if (!h) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() {
        RowList rl = list_order(h);
        const std::vector<int>& rows = kind == CC_PCORE ? rl.pcore : rl.outlier;
        const size_t m = (size_t)h->hc.m_rows, d = (size_t)h->d, n = rows.size();
        if (n == 0) return (int)CC_OK;
        auto fetch_vec = [&](const double* dev, double* out) {
            if (!out) return;
            std::vector<double> tmp(m * d);
            HIPCHK(hipMemcpyAsync(tmp.data(), dev, m * d * 8, hipMemcpyDeviceToHost, h->stream));
            sync_stream(h, h->stream);
            for (size_t i = 0; i < n; ++i) memcpy(out + i * d, tmp.data() + (size_t)rows[i] * d, d * 8);
        };
        fetch_vec(h->tab.cf1.p, cf1);
        fetch_vec(h->tab.cf2.p, cf2);
        fetch_vec(h->tab.cen.p, cen);
        fetch_vec(h->tab.pref.p, pref);
        if (w) {
            std::vector<double> tmp(m);
            HIPCHK(hipMemcpyAsync(tmp.data(), h->tab.w.p, m * 8, hipMemcpyDeviceToHost, h->stream));
            sync_stream(h, h->stream);
            for (size_t i = 0; i < n; ++i) w[i] = tmp[rows[i]];
        }
        auto fetch_i64 = [&](const long long* dev, int64_t* out) {
            if (!out) return;
            std::vector<long long> tmp(m);
            HIPCHK(hipMemcpyAsync(tmp.data(), dev, m * 8, hipMemcpyDeviceToHost, h->stream));
            sync_stream(h, h->stream);
            for (size_t i = 0; i < n; ++i) out[i] = tmp[rows[i]];
        };
        fetch_i64(h->tab.id.p, id);
        fetch_i64(h->tab.uid.p, uid);
        return (int)CC_OK;
    });
}

int cc_inject_mc(cc_handle* h, int kind, int32_t d, const double* cf1, const double* cf2, const double* cen,
                 const double* pref, double w, int64_t id, int64_t uid)
{
    if (!h || !cf1 || !cf2 || !cen || !pref) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() {
        int rc = set_dim(h, d);
        if (rc != CC_OK) return rc;
        ensure_table(h, (size_t)h->hc.m_rows + 1);
        const size_t r = (size_t)h->hc.m_rows, dd = (size_t)d;
        for (int i = 0; i < d; ++i)
            if (pref[i] != 1.0 && !(h->have_par && pref[i] == h->par.k)) h->tainted = true;
        HIPCHK(hipMemcpyAsync(h->tab.cf1.p + r * dd, cf1, dd * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->tab.cf2.p + r * dd, cf2, dd * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->tab.cen.p + r * dd, cen, dd * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->tab.pref.p + r * dd, pref, dd * 8, hipMemcpyHostToDevice, h->stream));
        const int knd = kind == CC_PCORE ? CC_KIND_PCORE : CC_KIND_OUTLIER;
        const int key = kind == CC_PCORE ? h->hc.n_pkeys++ : h->hc.n_okeys++;
        const long long lid = id, luid = uid;
        HIPCHK(hipMemcpyAsync(h->tab.w.p + r, &w, 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->tab.kind.p + r, &knd, 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->tab.key.p + r, &key, 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->tab.id.p + r, &lid, 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->tab.uid.p + r, &luid, 8, hipMemcpyHostToDevice, h->stream));
        sync_stream(h, h->stream);
        h->hc.m_rows += 1;
        if (kind == CC_PCORE && id >= h->hc.pcore_last_id) h->hc.pcore_last_id = id + 1;
        if (uid >= h->hc.outlier_last_id) h->hc.outlier_last_id = uid + 1;
        refresh_ctl_params(h);
        push_ctl(h);
        sync_stream(h, h->stream);
        return (int)CC_OK;
    });
}

int cc_inject_bulk(cc_handle* h, int kind, int32_t d, int32_t n, const double* cf1, const double* cf2,
                   const double* cen, const double* pref, const double* w, const int64_t* id, const int64_t* uid)
{
    if (!h || n < 0) return CC_ERR_BAD_ARG;
    if (n == 0) return CC_OK;
    if (!cf1 || !cf2 || !cen || !pref || !w || !id || !uid) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() {
        int rc = set_dim(h, d);
        if (rc != CC_OK) return rc;
        ensure_table(h, (size_t)h->hc.m_rows + (size_t)n);
        const size_t r = (size_t)h->hc.m_rows, dd = (size_t)d, nn = (size_t)n;
        for (size_t i = 0; i < nn * dd; ++i)
            if (pref[i] != 1.0 && !(h->have_par && pref[i] == h->par.k)) { h->tainted = true; break; }
        const int knd = kind == CC_PCORE ? CC_KIND_PCORE : CC_KIND_OUTLIER;
        int& nkeys = kind == CC_PCORE ? h->hc.n_pkeys : h->hc.n_okeys;
        std::vector<int> kinds(nn, knd), keys(nn);
        for (size_t i = 0; i < nn; ++i) keys[i] = nkeys + (int)i;
        static_assert(sizeof(long long) == sizeof(int64_t), "int64");
        HIPCHK(hipMemcpyAsync(h->tab.cf1.p + r * dd, cf1, nn * dd * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->tab.cf2.p + r * dd, cf2, nn * dd * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->tab.cen.p + r * dd, cen, nn * dd * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->tab.pref.p + r * dd, pref, nn * dd * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->tab.w.p + r, w, nn * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->tab.kind.p + r, kinds.data(), nn * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->tab.key.p + r, keys.data(), nn * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->tab.id.p + r, id, nn * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->tab.uid.p + r, uid, nn * 8, hipMemcpyHostToDevice, h->stream));
        sync_stream(h, h->stream);
        nkeys += n;
        h->hc.m_rows += n;
        for (size_t i = 0; i < nn; ++i) {
            if (kind == CC_PCORE && id[i] >= h->hc.pcore_last_id) h->hc.pcore_last_id = id[i] + 1;
            if (uid[i] >= h->hc.outlier_last_id) h->hc.outlier_last_id = uid[i] + 1;
        }
        refresh_ctl_params(h);
        push_ctl(h);
        sync_stream(h, h->stream);
        return (int)CC_OK;
    });
}

int cc_sync(cc_handle* h)
{
    if (!h) return CC_ERR_BAD_ARG;
    return guarded(h, [&]() {
        sync_stream(h, h->stream);
        sync_stream(h, h->stream2);
        HIPCHK(hipGetLastError());
        return (int)CC_OK;
    });
}

#include "cc_host_abi.inc"

int cc_f32_points(cc_handle* h, int64_t* out)
{
    if (!h || !out) return CC_ERR_BAD_ARG;
    *out = h->f32_points;
    return CC_OK;
}

int cc_view_points(cc_handle* h, int64_t* out)
{
    if (!h || !out) return CC_ERR_BAD_ARG;
    *out = h->view_points;
    return CC_OK;
}

int cc_get_stats(cc_handle* h, cc_stats* out)
{
    if (!h || !out) return CC_ERR_BAD_ARG;
    *out = h->stats;
    out->window = h->tun.window;
    out->calib_allgather_us = h->calib_ag_us;
    out->calib_scan_ns_per_row_dim = h->calib_scan_ns;
    out->split_threshold_row_dims = h->shard_min_row_dims;
    out->split_threshold_row_dims_pruned = h->shard_min_row_dims_pruned > 0 ? h->shard_min_row_dims_pruned : h->shard_min_row_dims;
    return CC_OK;
}

}  // extern "C"
