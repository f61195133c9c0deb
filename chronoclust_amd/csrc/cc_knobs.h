// cc_knobs.h — the experiment knobs of the library: what a handle takes from the environment when it is created, and nowhere
// else.  Each member carries its variable, its values and its default; read_knobs() parses them, one helper per kind of
// predicate (the kinds differ on strings such as "00", "01" or "off", so each knob keeps its own).  INTEGRATION.md lists them
// for users.  (included by cc_handle.h; one translation unit, cc_api.hip)
//
// Read elsewhere, where they are used: CHRONOCLUST_HIP_SCANB_Q and CHRONOCLUST_HIP_SCAN_LDS_KB (the scan dispatcher of
// cc_api.hip), CHRONOCLUST_HIP_POLICY_TRACE (cc_online_run.h), CHRONOCLUST_HIP_COMM_TIMEOUT_S, CHRONOCLUST_HIP_TWO_COMMS and
// CHRONOCLUST_HIP_CALIBRATE (cc_comm_init_rccl, cc_api_comm.inc).
#pragma once
#include <algorithm>
#include <climits>
#include <cstdlib>

struct Knobs {
    bool trace = false;     // CHRONOCLUST_HIP_TRACE=1: one stderr line per batch of windows
    bool light_sync_events = true;  // CHRONOCLUST_HIP_LIGHT_EVENTS=0: hipEventDefault events throughout (get_event, get_sync_event)
    // threads per workgroup of the validation kernels (32-lane groups x 32).  k_chain in workgroups of one wave: beside a
    // lookahead scan a small workgroup finds room on a single SIMD (measured: 4 % per window in steady state)
    // CHRONOCLUST_HIP_CHAIN_THREADS / _DECIDE_THREADS / _COMMIT_THREADS = 64, 128 or 256
    int chain_threads = 64, decide_threads = 256, commit_threads = 256;
    int decide_group = 16;  // CHRONOCLUST_HIP_DECIDE_GROUP=32: k_decide with one 32-lane group per point whatever d (16, the default: 16-lane groups up to 32 dimensions, 32-lane groups beyond)
    bool allow_scan_u = true;  // k_scan_u where it applies (CHRONOCLUST_HIP_SCANU=0: always k_scan)
    // the pruned snapshot scan (k_seed / k_seed_merge / k_scan_p) where k_scan_u applies and d > 8:
    // CHRONOCLUST_HIP_PRUNE = 0 never, 1 (default) while it pays (the device counts the rows it still evaluates in
    // full), 2 always; CHRONOCLUST_HIP_PRUNE_F = threshold factor (default 16)
    int prune_mode = 1;
    double prune_F = 16.0;
    int prune_rounds4 = 0;    // workgroups per CU a pruned scan is split into (CHRONOCLUST_HIP_PRUNE_WGS = 1 .. 64; 0: by width, see scan_plan_dp)
    bool group_guess_always = false;  // CHRONOCLUST_HIP_GROUP_GUESS=1: also in a group of one rank
    bool allow_guess = true;  // CHRONOCLUST_HIP_GUESS=0: seeded thresholds only
    bool allow_lean = true;   // CHRONOCLUST_HIP_LEAN=0: guessed scans always list and rescan the points they missed
    int force_prune_rows = 0;  // CHRONOCLUST_HIP_FORCE_PRUNE_ROWS: pruned scans whatever the phase from this many table rows on (0, the default: never forced - measured: it pays nowhere yet)
    bool allow_seed16 = false;  // CHRONOCLUST_HIP_SEED16=1: the seeds of a seeded pruned chain from the matrix cores (k_seed16) with the tight threshold, not from k_seed (eight-dimension prefix scores, F x the nearest) - measured a wash at C2's shapes, DESIGN section 9
    bool allow_prune_general = true;  // CHRONOCLUST_HIP_PRUNE_GENERAL=0: no pruned scans where the pdim filter is on or k is not a power of two
    bool la_pruned = false;   // CHRONOCLUST_HIP_LA_PRUNED=1: lookahead scans also while the scans are pruned chains on one GPU
    bool allow_probe = true;  // CHRONOCLUST_HIP_PROBE=0: pruned scans are retried blindly after a stretch of points
    // CHRONOCLUST_HIP_SCANA: 0 phase A inside k_scan_p (one point per lane, the round-3 form), 2 always as a kernel of its own
    // (k_scan_a: two points per lane), 1 (default) k_scan_a from 10 000 table rows on: at 5 000 rows the second launch and
    // phase B's own prologue cost what the cheaper phase A saves, at 50 000 the scan launch is 21 % shorter
    // (profiles/r05_tool_scan_a.txt)
    int split_a_mode = 1;
    bool allow_nodirty = true;  // CHRONOCLUST_HIP_NODIRTY=0: always launch the dirty scans
    bool allow_claims = true;   // CHRONOCLUST_HIP_CLAIMS=0: k_decide's atomics whatever the table size
    bool allow_long = true;     // CHRONOCLUST_HIP_LONGCHAINS=0: every chain replayed by k_chain
    bool allow_prep = true;     // CHRONOCLUST_HIP_LONGPREP=0: long chains replayed by one workgroup each, as before round 5
    bool allow_quiet = true;    // CHRONOCLUST_HIP_QUIET=0: k_decide re-derives every decision of a validation round even when k_dseed has shown that all of them repeat their claims
    bool allow_missed_plain = true;  // CHRONOCLUST_HIP_MISSED_PLAIN=0: the points a guessed threshold missed go through the seeded chain, not k_scan_u
    int p3_listed_rows = 10000;  // CHRONOCLUST_HIP_P3_LISTED=<rows>: k_scan_p3 lists the rows phase A keeps from this many table rows on
    bool allow_scan_p3 = true;   // CHRONOCLUST_HIP_SCANP3=0: the prefix test of the window's pruned scan on the VALU (k_scan_p2), not the matrix cores
    bool allow_scan_p2 = true;  // CHRONOCLUST_HIP_SCANP2=0: the pruned scan of a window as k_scan_p (one point per lane) instead of k_scan_p2
    bool allow_link = true;     // CHRONOCLUST_HIP_LINK=0: round 0 does not link the points that decide "create" among themselves (cc_link.h)
    bool allow_heavy = true;    // CHRONOCLUST_HIP_HEAVY=0: k_decide's atomics also for rows that take a large share of a window
    bool allow_seq_r = true;    // CHRONOCLUST_HIP_SEQR=0: the sequential kernel with the table in LDS whatever d
    bool allow_seq_g = true;    // CHRONOCLUST_HIP_SEQG=0: no sequential kernel beyond the LDS image (k_seq_g, the table in HBM)
    int allow_sparse = 128;     // CHRONOCLUST_HIP_SPARSE=0: no sparse dirty scans (the tiles' scans or none); N: while at most one point in N needs them
    int assign_chunk = 0;       // CHRONOCLUST_HIP_ASSIGN_CHUNK=<points>: points per chunk of cc_assign (0, the default: 32 MiB of coordinates, at most 262 144 points)
    int ingest_slab = 0;        // CHRONOCLUST_HIP_INGEST_SLAB=<points>: points per slab of raw float32 on its way through device staging, whole 64-point tiles (0, the default: 32 MiB of it - 16 MiB in a prefetch, a page-locked buffer's worth; the knob only ever shortens a slab)
    int assign_segments = 0;    // CHRONOCLUST_HIP_ASSIGN_SEGMENTS=1 .. 64: row segments per point tile of k_assign_scan (0, the default: by chunk and table size)
};

namespace {

// v = false when the value starts with '0' ("0", "00", "0x1"), true otherwise - unset, empty and "off" included
void knob_off_when_starts_with_0(bool& v, const char* name) { const char* e = getenv(name); v = !(e && e[0] == '0'); }
// v = true when the value starts with '1', false otherwise
void knob_on_when_starts_with_1(bool& v, const char* name) { const char* e = getenv(name); v = e && e[0] == '1'; }
// when set: v = (atoi of the value is not zero) - "00" and "off" switch off, "01" on; unset: v as it is
void knob_atoi_nonzero_when_set(bool& v, const char* name) { if (const char* e = getenv(name)) v = atoi(e) != 0; }
// when set and lo <= atoi <= hi: v = atoi; anything else is ignored
void knob_int_in(int& v, const char* name, int lo, int hi) { const char* e = getenv(name); if (e && atoi(e) >= lo && atoi(e) <= hi) v = atoi(e); }
// ... and a workgroup size: 64, 128 or 256
void knob_threads(int& v, const char* name) { int t = 0; knob_int_in(t, name, 64, 256); if (t == 64 || t == 128 || t == 256) v = t; }

// (once, on the defaults above: "atoi non-zero when set" is also what the knobs do that only ever leave their default -
// MISSED_PLAIN, PRUNE_GENERAL, SCANP3 off at 0, LA_PRUNED on at non-zero)
void read_knobs(Knobs& k)
{
    knob_on_when_starts_with_1(k.trace, "CHRONOCLUST_HIP_TRACE");
    knob_on_when_starts_with_1(k.group_guess_always, "CHRONOCLUST_HIP_GROUP_GUESS");
    knob_off_when_starts_with_0(k.allow_nodirty, "CHRONOCLUST_HIP_NODIRTY");
    knob_off_when_starts_with_0(k.allow_claims, "CHRONOCLUST_HIP_CLAIMS");
    knob_off_when_starts_with_0(k.allow_long, "CHRONOCLUST_HIP_LONGCHAINS");
    knob_off_when_starts_with_0(k.allow_prep, "CHRONOCLUST_HIP_LONGPREP");
    knob_off_when_starts_with_0(k.allow_quiet, "CHRONOCLUST_HIP_QUIET");
    knob_off_when_starts_with_0(k.allow_heavy, "CHRONOCLUST_HIP_HEAVY");
    knob_off_when_starts_with_0(k.allow_seq_r, "CHRONOCLUST_HIP_SEQR");
    knob_off_when_starts_with_0(k.allow_seq_g, "CHRONOCLUST_HIP_SEQG");
    knob_off_when_starts_with_0(k.allow_probe, "CHRONOCLUST_HIP_PROBE");
    knob_off_when_starts_with_0(k.allow_guess, "CHRONOCLUST_HIP_GUESS");
    knob_off_when_starts_with_0(k.allow_lean, "CHRONOCLUST_HIP_LEAN");
    knob_off_when_starts_with_0(k.allow_scan_p2, "CHRONOCLUST_HIP_SCANP2");
    knob_off_when_starts_with_0(k.allow_link, "CHRONOCLUST_HIP_LINK");
    knob_atoi_nonzero_when_set(k.light_sync_events, "CHRONOCLUST_HIP_LIGHT_EVENTS");
    knob_atoi_nonzero_when_set(k.allow_scan_u, "CHRONOCLUST_HIP_SCANU");
    knob_atoi_nonzero_when_set(k.allow_seed16, "CHRONOCLUST_HIP_SEED16");
    knob_atoi_nonzero_when_set(k.allow_missed_plain, "CHRONOCLUST_HIP_MISSED_PLAIN");
    knob_atoi_nonzero_when_set(k.allow_prune_general, "CHRONOCLUST_HIP_PRUNE_GENERAL");
    knob_atoi_nonzero_when_set(k.allow_scan_p3, "CHRONOCLUST_HIP_SCANP3");
    knob_atoi_nonzero_when_set(k.la_pruned, "CHRONOCLUST_HIP_LA_PRUNED");
    knob_threads(k.chain_threads, "CHRONOCLUST_HIP_CHAIN_THREADS");
    knob_threads(k.decide_threads, "CHRONOCLUST_HIP_DECIDE_THREADS");
    knob_threads(k.commit_threads, "CHRONOCLUST_HIP_COMMIT_THREADS");
    { int g = 0; knob_int_in(g, "CHRONOCLUST_HIP_DECIDE_GROUP", 16, 32); if (g == 16 || g == 32) k.decide_group = g; }
    knob_int_in(k.prune_mode, "CHRONOCLUST_HIP_PRUNE", 0, 2);
    knob_int_in(k.prune_rounds4, "CHRONOCLUST_HIP_PRUNE_WGS", 1, 64);
    knob_int_in(k.allow_sparse, "CHRONOCLUST_HIP_SPARSE", 0, INT_MAX);
    knob_int_in(k.assign_chunk, "CHRONOCLUST_HIP_ASSIGN_CHUNK", 1, 1 << 24);
    knob_int_in(k.ingest_slab, "CHRONOCLUST_HIP_INGEST_SLAB", 1, 1 << 26);
    knob_int_in(k.assign_segments, "CHRONOCLUST_HIP_ASSIGN_SEGMENTS", 1, 64);
    knob_int_in(k.force_prune_rows, "CHRONOCLUST_HIP_FORCE_PRUNE_ROWS", INT_MIN, INT_MAX);  // (any integer, as atoi reads it)
    knob_int_in(k.p3_listed_rows, "CHRONOCLUST_HIP_P3_LISTED", INT_MIN, INT_MAX);
    // the two special cases: clamped to 0 .. 2, not ignored outside it; a factor, atof, from 1 on
    if (const char* e = getenv("CHRONOCLUST_HIP_SCANA")) k.split_a_mode = std::max(0, std::min(2, atoi(e)));
    if (const char* e = getenv("CHRONOCLUST_HIP_PRUNE_F")) if (atof(e) >= 1.0) k.prune_F = atof(e);
}

}  // namespace
