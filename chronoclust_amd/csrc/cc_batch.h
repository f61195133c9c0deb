// cc_batch.h — how one batch of windows of the exact online phase is launched, as plain C++ (no HIP, no handle).
//
// cc::WindowPolicy (cc_policy.h) decides HOW MANY windows of which size a batch has and which scans serve them; this file
// turns that, the handle's settings and the last read-back of the control block into the geometry of the batch's launches:
// grids, partials per point, and which kernels gather the claims and replay the long chains.  Like the policy it is a
// function of values that are identical on every rank of a group.  OnlineRun::enqueue_batch (cc_online_run.h) computes a
// BatchPlan once at its top and reads nothing else for geometry; cc_batch_plan (C-ABI) computes one on a machine without a
// GPU (tests/test_batch_plan.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/chronoclust_hip.h"

namespace cc {

using BatchInputs = cc_batch_inputs;
using BatchPlan = cc_batch_geometry;

// (CC_MAX_WINDOW and CC_LONG_CAP of cc_common.h, which needs HIP; cc_online_run.h asserts that they agree)
constexpr int kMaxWindow = 49152;
constexpr int kLongCap = 512;

// The widths the snapshot scans are compiled for, and which scans serve a stream of d dimensions (pdim filter on or off, k a
// power of two or not) before any knob is applied - scan_plan() (cc_api.hip) applies those on top; cc_scan_width (C-ABI)
// answers on a machine without a GPU (tests/test_scan_width_rule.py).
//   padded   the smallest compiled width >= d (padded dimensions cost full distance terms: the ladder follows the shapes of
//            BASELINE.json - d = 14, 20, 40); 64 beyond it, where no window runs
//   scan_u   the plain scan is k_scan_u, the rows as scalar operands: the common case (k a power of two, no pdim filter) at
//            a compiled width, and from nine dimensions on at any width up to 64 - there the kernels, which index rows as
//            row * padded, read a padded mirror of the rows (k_pad_rows, cc_scan.h) and points padded with zero rows.
//            Up to eight dimensions k_scan pads for itself and no pruned chain exists to gain.
//   chain    the pruned chain: COMMON behind k_scan_u beyond eight dimensions; GENERAL (k_scan_p3<GENERAL>, up to 40
//            dimensions) where the filter is on or k is not a power of two - at compiled widths only: its phase B evaluates
//            the pdim filter over the rows at the true d, where a padded dimension would count as preferred
constexpr int kScanWidths[8] = {4, 8, 14, 16, 20, 32, 40, 64};
struct ScanWidth {
    int padded = 0;
    bool scan_u = false;
    int chain = CC_CHAIN_NONE;
};
inline ScanWidth scan_width(int d, bool filter, bool pow2)
{
    ScanWidth w;
    w.padded = kScanWidths[7];
    for (int i = 7; i >= 0; --i)
        if (d <= kScanWidths[i]) w.padded = kScanWidths[i];
    const bool compiled = d == w.padded, common = !filter && pow2;
    w.scan_u = common && (compiled || (d > 8 && d < w.padded));
    if (w.scan_u && w.padded > 8) w.chain = CC_CHAIN_COMMON;
    else if (!common && compiled && w.padded > 8 && w.padded <= 40) w.chain = CC_CHAIN_GENERAL;
    return w;
}

// Partials per point for a batch whose windows have `tiles` point tiles: at most S, not less than S / 2, chosen so that
// the launch (tiles x S' workgroups) fills whole rounds of the resident workgroups - 1 024 workgroups on a machine that
// holds 768 at once (d = 40) run as long as 1 536 would.
inline int scan_partials_for(int tiles, int S, int resident)
{
    int best = S;
    double best_eff = 0.0;
    for (int s = S; s >= std::max(1, S / 2); --s) {
        const double x = (double)tiles * s / (double)resident;
        const double eff = x / std::ceil(x);
        if (eff > best_eff + 1e-9) { best_eff = eff; best = s; }
    }
    return best;
}

inline BatchPlan batch_plan(const BatchInputs& in)
{
    BatchPlan p{};
    // grids cover the window size of this batch (no window of the batch is larger), not the configured maximum
    const int gw = p.gw = std::max(64, std::min(in.window, in.win_cfg));
    // partials per point of this batch's clean scans (a pending lookahead scan was launched with the same value:
    // it only depends on the window size, and a change of that restarts the lookahead chain)
    // A pruned scan spends a few VALU instructions per row, so a wave must own many rows for its fixed costs
    // (points, thresholds, tile pipeline, candidate merge: microseconds) not to dominate: as few sub-ranges as fill
    // the machine once (about a fifth of the plain scan's partials at the full window).
    p.S = in.prune_now ? std::max(1, std::min(in.S_cfg, (in.n_cus * in.prune_wgs_per_cu) / std::max(1, (gw + 63) / 64)))
                       : scan_partials_for((gw + 63) / 64, in.S_cfg, in.n_cus * in.plain_wgs_per_cu);
    // capacity of the round's list for the sparse dirty scans: a sixteenth of the window (the policy's bound on
    // the batch's average), in whole tiles
    p.sparse_cap = std::min(kMaxWindow / 16, std::max(64, ((gw / 16 + 63) / 64) * 64));
    p.dblocks = (gw + in.decide_threads / 32 - 1) / (in.decide_threads / 32);  // one 32-lane group per point
    p.cblocks = (gw + in.chain_threads / 32 - 1) / (in.chain_threads / 32);    // 32-lane groups of k_chain per workgroup x 32
    p.rblocks = std::min((gw + in.commit_threads / 32 - 1) / (in.commit_threads / 32), 1024 * (256 / in.commit_threads));
    // few MCs: the claims of a window are gathered per MC by k_claims (rows beyond scan_rows, e.g. rows created
    // during the batch, keep k_decide's atomics)
    p.scan_rows = (in.allow_claims && in.m_rows > 0 && in.m_rows <= 1024) ? in.m_rows : 0;
    // ... and their long chains (more than CC_CHAIN_MEMB claimants; k_claims leaves the exact count) are replayed
    // by k_chain_long, one workgroup per MC, instead of one point after the other
    p.long_rows = in.allow_long ? p.scan_rows : 0;
    // On a larger table long chains are rare on evenly spread data and the rule on skewed data (one population
    // that takes a third of the events): k_chain_long is launched, over the list k_decide keeps, in the batches
    // that follow one in which such chains were seen (a function of device counters: every rank decides alike)
    p.long_listed = (in.allow_long && p.scan_rows == 0 && in.long_seen) ? 1 : 0;
    // heavy rows: their claims are gathered by k_claims_heavy instead of k_decide's atomics from the batch after the
    // one that marked them (the marks change between windows, on the device; what the host saw at the last sync
    // decides for the whole batch whether the gathering kernel is launched - k_decide is told the same)
    p.heavy_on = (in.allow_heavy && p.scan_rows == 0 && in.n_heavy > 0) ? 1 : 0;
    // workgroups of its launches = entries k_decide may list per round: a few more than the previous batch's
    // average when that was small (a launch of hundreds of workgroups that return at once is not free)
    p.long_cap = in.long_few ? (int)std::min<long long>(kLongCap, 2 * in.long_avg + 8) : kLongCap;
    // No window beyond the end of the range: when windows commit in full, ceil(left / window) of them finish the call (a
    // window that is cut short leaves its rest to the next batch, as anywhere else).  Every window enqueued past the end
    // is a dozen launches that find nothing to do - 50-100 us each, up to fifteen of them at the end of every call
    // (profiles/r06_tool_startup_timeline_before.txt: w36-w47).  A function of counters that are the same on every rank.
    const long long w = std::max(1, in.win_cfg);
    p.windows_now = (int)std::max<long long>(1, std::min<long long>(in.batch_windows, (in.points_left + w - 1) / w));
    // long chains of pcore MCs: running sums first, by one workgroup per chain (PREP); the steps themselves inside k_chain,
    // the fallback (rejected steps, outlier MCs) behind it
    // (while the chains are few and long: with 200 table rows a chain is one batch of k_chain_long and the rows' 200
    // workgroups are parallel enough - the extra launch cost 2 % there, measured)
    p.prep = (in.allow_prep && ((p.long_rows > 0 && p.long_rows <= 64) || (p.long_listed && in.long_few))) ? 1 : 0;
    p.prep_form = !p.prep ? CC_LONG_NONE : p.long_rows > 0 ? CC_LONG_ROWS_SPLIT : CC_LONG_LIST_SPLIT;
    // k_chain_long: one workgroup per table row while k_claims serves the table, else per entry of the
    // round's list.  The large workgroups (SPLIT) while they are few - rows <= 256, or a short list, judged by
    // the previous batch's count -, the small ones (two per CU) when hundreds of chains are long
    p.long_form = p.long_rows > 0 ? (p.long_rows <= 256 ? CC_LONG_ROWS_SPLIT : CC_LONG_ROWS_SMALL)
                  : p.long_listed ? (in.long_few ? CC_LONG_LIST_SPLIT : CC_LONG_LIST_SMALL)
                                  : CC_LONG_NONE;
    return p;
}

// Long chains (k_chain_long over the list k_decide keeps) as the batches of a call saw them: what the next batch's plan
// takes as long_seen / long_few / long_avg
struct LongChains {
    long long prev = 0;         // Ctl::stat_long at the end of the previous batch
    long long rounds_prev = 0;  // Ctl::stat_rounds
    bool seen = false;          // the previous batch added to stat_long
    bool few = true;            // ... by no more than 64 chains per validation round
    long long avg = 1;

    void after_batch(long long stat_long, long long stat_rounds)
    {
        seen = stat_long > prev;
        // (long chains per window and validation round of the batch: up to 64 count as few)
        avg = (stat_long - prev) / std::max<long long>(1, stat_rounds - rounds_prev) + 1;
        few = avg <= 64;
        prev = stat_long;
        rounds_prev = stat_rounds;
    }
};

// Round 0 links the points that decide "create" among themselves (cc_link.h: two more small launches per window)
// while the batch just read back created a microcluster per 256 points or more - a function of device counters
// that are identical on every rank
inline bool link_after_batch(bool allowed, long long rows_created, long long points)
{
    return allowed && rows_created * 256 >= std::max<long long>(1, points);
}

}  // namespace cc
