#!/usr/bin/env python3
"""Generates tests/golden/surface/ (TEST INFRASTRUCTURE): the Python reference at the places the fuzz tests and the
injected-table referees were designed to hit - k < 1 and k = 1, delta 0 and 1, lambda 0, pi 1 and pi > d, grids and
duplicates, timepoints of one and two points, d = 1 and 2, weights on beta * mu and on omicron, runs of flagged rows at the
decay boundary, distance ties, a radius on eps_sq, stored preference entries outside {1, k}.

Runs ONLY where the upstream Python reference can be imported (oracle/ref_harness/refenv.py); the tests
(tests/test_reference_surface_cpu.py, tests/test_reference_surface.py) read the committed files alone.  The reference is
driven directly - HDDStream(config, logger), tables injected as Microcluster objects - and instrumented like make_golden.py
(Recorder, extended by the path every point took and by the per-pcore results of the offline phase); no reference text
is written anywhere.  The record format is tests/surface_util.py's.

    python tests/golden/make_golden_surface.py            # writes tests/golden/surface/
    python tests/golden/make_golden_surface.py --check    # regenerates into a temporary directory and compares

Sets (the inputs are regenerated from their seeds by the tests; the files keep their SHA-256)
  streams_fuzz_*   test_fuzz_parity._case(seed), seeds 0..191 whose largest timepoint has at most
                   surface_util.FUZZ_MAX_POINTS points - 4 000: all of them, the 4 000-point seeds included (the whole
                   generator takes about seven minutes on eight cores, 40 minutes of the reference in all); seeds a smaller
                   limit leaves out are listed in the files' meta (`left_out`)
  streams_seqr_*   test_sequential._seq_r_case(seed), seeds 0..95 with timepoints of at most 3 000 points
  boundary         test_boundary_tables.SHAPES without (30 000, 20 000, 5), two calls of decay + downgrade each, and the
                   all-flagged cases of test_repeated_calls_empty_the_table until both lists are empty; both lists after
                   every call
  offline          table_util.OFFLINE_TABLES of at most 700 pcores: core, pdim, |N_eps|, |N_w| per pcore and the clusters
                   with their members in merge order
  online           table_util.ONLINE_TABLES with injected rows x points <= 600 000, the victims_by_set_params cases with
                   their first call; the reference's id counters are seeded with what the oracle derives for the same
                   injected lists, last_data_timestamp is the call's daystamp (no decay), the offline phase is not run
"""
import logging
import multiprocessing
import os
import shutil
import sys
import tempfile
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle", "ref_harness"), os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import refenv  # noqa: E402
import surface_util as S  # noqa: E402
import table_util as T  # noqa: E402
from make_golden import Recorder  # noqa: E402

F = 2.0 ** -1.0   # the boundary cases' decay factor: lambda = 1, one day


class SurfaceRecorder(Recorder):
    """Recorder plus the path of every point (0 pcore, 1 outlier, | 4 promoted by the add, 2 new: the oracle's codes, read
    off the three branches of the reference's loop) and the PreDeCon object of the last offline phase."""

    def install(self):
        Recorder.install(self)
        from chronoclust.clustering import hddstream as H
        from chronoclust.clustering import predecon as PD
        rec = self
        self.paths, self.predecon = [], None
        self._orig = (H.HDDStream._add_to_pcore, H.HDDStream._add_to_outlier, H.HDDStream._create_new_outlier_cluster,
                      PD.PreDeCon.run)
        to_pcore, to_outlier, create, run = self._orig

        def add_to_pcore(this, *a):
            done = to_pcore(this, *a)
            if done:
                rec.paths.append(0)
            return done

        def add_to_outlier(this, *a):
            before = len(this.pcore_MC)
            done = to_outlier(this, *a)
            if done:
                rec.paths.append(1 | (4 if len(this.pcore_MC) > before else 0))
            return done

        def create_new(this, *a):
            rec.paths.append(2)
            return create(this, *a)

        def predecon_run(this):
            rec.predecon = this
            return run(this)

        H.HDDStream._add_to_pcore, H.HDDStream._add_to_outlier = add_to_pcore, add_to_outlier
        H.HDDStream._create_new_outlier_cluster = create_new
        PD.PreDeCon.run = predecon_run

    def uninstall(self):
        Recorder.uninstall(self)
        from chronoclust.clustering import hddstream as H
        from chronoclust.clustering import predecon as PD
        (H.HDDStream._add_to_pcore, H.HDDStream._add_to_outlier, H.HDDStream._create_new_outlier_cluster,
         PD.PreDeCon.run) = self._orig

    def dump(self, h, X, daystamp, seconds):
        out = Recorder.dump(self, h, X, daystamp, seconds)
        assert len(self.paths) == len(X)
        out["labels_path"], self.paths = np.array(self.paths, dtype=np.int8), []
        return out

    def lists(self, h, d):
        """The state of an object that saw no points (boundary and offline cases)."""
        self.paths = []
        return self.dump(h, np.zeros((0, d)), 0, 0.0)

    def offline_info(self):
        pts = list(self.predecon.datapoints.values())
        return dict(core=[bool(p.is_core()) for p in pts], pdim=[int(p.get_pdim()) for p in pts],
                    nn=[len(p.neighbour_pts) for p in pts], nw=[len(p.weighted_neighbour_pts) for p in pts])


def record(c, clusters=True, info=None, mid_pref=None):
    """surface_util's record of one of Recorder's dumps."""
    tables = [{col: c["%s_%s" % (kind, col)] for col in S.LIST_COLS} for kind in ("pcore", "outlier")]
    cl = None
    if clusters:
        off = c["cl_offsets"]
        cl = [dict(members=c["cl_members"][off[i]:off[i + 1]], w=c["cl_w"][i], cf1=c["cl_cf1"][i], cf2=c["cl_cf2"][i],
                   cen=c["cl_cen"][i], pref=c["cl_pref"][i]) for i in range(len(off) - 1)]
    return S.make_record(params=c["params"], X=c["X"], uid=c["labels_uid"], path=c["labels_path"], tables=tables,
                         clusters=cl, info=info, mid_pref=mid_pref)


def _logger():
    log = logging.getLogger("make_golden_surface")
    log.propagate = False
    log.setLevel(logging.CRITICAL)
    if not log.handlers:
        log.addHandler(logging.NullHandler())
    return log


def ref_object(par, d, pcores=None, outliers=None, counters=None):
    """The reference's HDDStream with exactly the parameters of `par` (what table_util.make_oracle is to the oracle) and the
    two lists as Microcluster objects."""
    from chronoclust.clustering.hddstream import HDDStream
    from chronoclust.objects.microcluster import Microcluster
    h = HDDStream({"epsilon": 1.0, "upsilon": 1.0, "delta": 0.5, "beta": par.beta, "k": par.k, "lambda": 1.0}, _logger())
    set_params(h, par)
    h.dataset_dimensionality = d
    for mcs, t in ((h.pcore_MC, pcores), (h.outlier_MC, outliers)):
        for r in range(len(t) if t is not None else 0):
            mc = Microcluster(cf1=t.cf1[r].copy(), cf2=t.cf2[r].copy(), id={int(t.id[r])}, cumulative_weight=float(t.w[r]),
                              preferred_dimension_vector=t.pref[r].copy(), cluster_centroids=t.cen[r].copy())
            mc.update_prev_outlier_id(int(t.uid[r]))
            mcs.append(mc)
    if counters is not None:
        h.pcore_MC_last_id, h.outlier_MC_last_id = counters
    return h


def set_params(h, par):
    h.epsilon_squared, h.delta_squared, h.k, h.beta, h.mu, h.omicron = par.eps_sq, par.delta_sq, par.k, par.beta, par.mu, par.omicron
    h.upsilon, h.delta, h.pi = par.ups_eps, par.delta, par.pi


# ---- one case each: [(record name, record)] ----------------------------------------------------------------------------

def gen_stream(case):
    from chronoclust.clustering.hddstream import HDDStream
    cfg, Xs = S.stream_case(case)
    rec = SurfaceRecorder()
    rec.install()
    try:
        h = HDDStream(dict(cfg), _logger())
        for t, X in enumerate(Xs):
            h.online_microcluster_maintenance(X, t)
    finally:
        rec.uninstall()
    return [("%s@%d" % (case, t), record(c)) for t, c in enumerate(rec.calls)]


def gen_boundary(case):
    pcores, outliers, par = S.boundary_case(case)
    flagged = S.boundary_cases()[case][4]
    rec = SurfaceRecorder()
    rec.install()
    try:
        h = ref_object(par, pcores.d, pcores, outliers)
        out = []
        while (len(h.pcore_MC) + len(h.outlier_MC) > 0) if flagged else (len(out) < 2):
            h._decay_clusters_weight(1)      # hddstream.py:199-205 with lambda = 1, one day: the factor is F
            h.downgrade_microclusters()
            out.append(("%s@%d" % (case, len(out)), record(rec.lists(h, pcores.d), clusters=False)))
            assert len(out) < 40
    finally:
        rec.uninstall()
    assert 2 ** (-h.lambbda * 1) == F
    return out


def gen_offline(case):
    t, par, _ = T.build_table(case)
    rec = SurfaceRecorder()
    rec.install()
    try:
        h = ref_object(par, t.d, t)
        rec._merge_log = {}
        h.offline_clustering(0)
        out = record(rec.lists(h, t.d), info=rec.offline_info())
    finally:
        rec.uninstall()
    return [(case + "@0", out)]


def gen_online(case):
    pcores, outliers, par, X, meta = T.build_online(case)
    d = X.shape[1]
    rec = SurfaceRecorder()
    rec.install()
    try:
        if "first" in meta:
            par0, X0 = meta["first"]
            h = ref_object(par0, d)
            h.offline_clustering = lambda daystamp: None
            h.online_microcluster_maintenance(X0, 0, reset_param=False)
            for mc in h.pcore_MC + h.outlier_MC:
                mc.reset_points()            # (bookkeeping of the first call's point numbers: the second call starts at 0)
            set_params(h, par)
        else:
            h = ref_object(par, d, pcores, outliers, counters=T.make_oracle(par, pcores, outliers).counters)
            h.offline_clustering = lambda daystamp: None
        h.online_microcluster_maintenance(X, 0, reset_param=False)
    finally:
        rec.uninstall()
    out = [record(c, clusters=False) for c in rec.calls]
    if "first" in meta:
        out[0] = record(rec.calls[0], clusters=False, mid_pref=rec.calls[0]["pcore_pref"])
    return [("%s@%d" % (case, i), r) for i, r in enumerate(out)]


GENERATORS = {"fuzz": gen_stream, "seqr": gen_stream, "boundary": gen_boundary, "offline": gen_offline, "online": gen_online}


def _work(job):
    kind, case = job
    warnings.simplefilter("ignore", RuntimeWarning)   # (the reference divides 0 by 0 on some of these inputs; so be it)
    t0 = time.time()
    return job, GENERATORS[kind](case), time.time() - t0


def jobs():
    fuzz, left_out, seqr = S.stream_selection()
    return ([("fuzz", "fuzz-%d" % s) for s in fuzz] + [("seqr", "seqr-%d" % s) for s in seqr]
            + [("boundary", n) for n in S.boundary_cases()] + [("offline", n) for n in S.offline_cases()]
            + [("online", n) for n in S.online_cases()]), left_out


def file_of(kind, case):
    """Streams in files of 48 seeds, each table set in one file."""
    if kind in ("fuzz", "seqr"):
        return "streams_%s_%d.npz" % (kind, int(case.split("-")[1]) // 48)
    return kind + ".npz"


def generate(directory, workers):
    from oracle import oracle as O
    O.lib()                                  # (built once, before the workers need it for the id counters)
    todo, left_out = jobs()
    t0 = time.time()
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        done = {job: (recs, sec) for job, recs, sec in pool.imap_unordered(_work, todo, chunksize=1)}
    files = {}
    for job in todo:
        files.setdefault(file_of(*job), []).extend(done[job][0])
    os.makedirs(directory, exist_ok=True)
    limit = os.path.getsize(S.LARGEST_GOLDEN)
    total = 0
    for fn, records in sorted(files.items()):
        meta = {}
        if fn.startswith("streams_"):            # the width of every stream, so that a test knows it before it builds one
            meta["dims"] = {job[1]: int(S.stream_case(job[1])[1][0].shape[1]) for job in todo if file_of(*job) == fn}
        if fn.startswith("streams_fuzz"):
            meta.update(left_out=left_out, fuzz_max_points=S.FUZZ_MAX_POINTS)
        S.save_pack(os.path.join(directory, fn), records, meta)
        size = os.path.getsize(os.path.join(directory, fn))
        total += size
        assert size <= limit, "%s: %d bytes, more than the largest golden (%d)" % (fn, size, limit)
        print("%-22s %4d records %8d bytes" % (fn, len(records), size))
    assert total < S.DIR_LIMIT, "the directory holds %d bytes" % total
    slow = sorted(((sec, job[1]) for job, (_, sec) in done.items()), reverse=True)[:5]
    print("%d cases, %d bytes, %.0f s with %d workers (%.0f s of the reference in all; slowest: %s)" % (
        len(todo), total, time.time() - t0, workers, sum(sec for _, sec in done.values()),
        ", ".join("%s %.0f s" % (n, s) for s, n in slow)))
    print("fuzz seeds left out (largest timepoint above %d points): %s" % (S.FUZZ_MAX_POINTS, left_out))


def check(workers):
    """Regenerates into a temporary directory and compares every array of every file with the committed one."""
    tmp = tempfile.mkdtemp()
    try:
        generate(tmp, workers)
        new, old = sorted(os.listdir(tmp)), sorted(f for f in os.listdir(S.SURFACE) if f.endswith(".npz"))
        assert new == old, "files %r, committed %r" % (new, old)
        for fn in new:
            a, b = np.load(os.path.join(tmp, fn)), np.load(os.path.join(S.SURFACE, fn))
            assert sorted(a.files) == sorted(b.files), fn
            for key in a.files:
                assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), \
                    "%s: %s differs from the committed file" % (fn, key)
        print("check: %d files regenerated, every array equal to the committed one" % len(new))
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    refenv.load()
    n_workers = min(8, os.cpu_count() or 1)
    if "--check" in sys.argv[1:]:
        check(n_workers)
    else:
        generate(S.SURFACE, n_workers)
