"""Checks of the copy-number profile (ambi_batch_profile, csrc/ambi_profile.hpp) shared by the CPU host-simulation tests and
the GPU tests (same assertions, different library).

Expected values never come from the engine's profile: the cells are the ORACLE's path of the unit, counted with plain numpy
(bincount per strand), seg_cn is the oracle's record; target_cn is what Batch.unit_prepare returns (pinned by the parity
tests)."""
import os

import numpy as np

import cases
from ambigram_amd import api, synth

ZERO = dict(cells=0, runs=0, turns=0, max_cn=0, n_uncovered=0, n_off_target=0, n_off_input=0, l1_target=0)


def expected(path_abs, base, n, target_cn, seg_cn, status):
    """(fwd, rev, summary) of a path given as ABSOLUTE signed segment ids; local id = |id| - base.  target_cn / seg_cn: n + 1
    values, slot 0 unused."""
    c = np.asarray(path_abs, np.int64)
    if status < 0 or len(c) == 0:           # a refused unit or one without a path: zero counts, cells = 0
        z = np.zeros(n + 1, np.int32)
        return z, z.copy(), dict(ZERO, status=status)
    c = np.where(c > 0, c - base, c + base)
    assert np.all(c != 0) and np.abs(c).max() <= n
    fwd = np.bincount(c[c > 0], minlength=n + 1)[:n + 1].astype(np.int32)
    rev = np.bincount(-c[c < 0], minlength=n + 1)[:n + 1].astype(np.int32)
    tot = (fwd + rev)[1:].astype(np.int64)
    tgt = np.asarray(target_cn, np.int64)[1:]
    s = dict(status=status, cells=len(c), runs=1 + int(np.count_nonzero(c[1:] != c[:-1] + 1)), turns=int(np.count_nonzero(c[1:] == -c[:-1])),
             max_cn=int(tot.max()), n_uncovered=int(np.count_nonzero(tot == 0)), n_off_target=int(np.count_nonzero(tot != tgt)),
             l1_target=int(np.abs(tot - tgt).sum()), n_off_input=int(np.count_nonzero(np.abs(tot - np.asarray(seg_cn, float)[1:]) >= 0.5)))
    return fwd, rev, s


def unit_expectation(b, u, oc, which, status=None):
    """Expectation of unit u from its oracle record oc (one chromosome of oracle.run_bfb)."""
    s, e = oc["start"], oc["end"]
    n = e - s + 1
    prep = b.unit_prepare(u, n)
    seg_cn = np.concatenate([[0.0], np.asarray(oc["seg_cn"], float)[s - 1:e]]) if len(oc.get("seg_cn") or []) >= e else prep["seg_cn"]
    if status is None:
        status = api.ST_SHORTCUT if oc["shortcut"] else (api.ST_INFEASIBLE if oc["infeasible"] else 0)
    path = oc["path_indel"] if which else oc["path"]
    if (oc["shortcut"] or oc["infeasible"]) and not path:
        path = list(range(s, e + 1))        # the reference path 1+ .. n+ (localhap.cpp:164-170, :213-220)
    return n, expected(path, s - 1, n, prep["target_cn"], seg_cn, status)


def compare_unit(b, u, n, want, tag):
    fwd, rev, summary = want
    got_f, got_r = b.unit_path_cn(u, n)
    assert got_f.tolist() == fwd.tolist(), (tag, "fwd", got_f.tolist(), fwd.tolist())
    assert got_r.tolist() == rev.tolist(), (tag, "rev", got_r.tolist(), rev.tolist())
    assert b.unit_profile(u) == summary, (tag, b.unit_profile(u), summary)


def check_batch(b, records, tag, whichs=(0, 1), statuses=None):
    """Both paths of every unit of a batch that has run and been downloaded."""
    for which in whichs:
        b.profile(which); b.profile_wait()
        for u, oc in enumerate(records):
            n, want = unit_expectation(b, u, oc, which, None if statuses is None else statuses[u])
            compare_unit(b, u, n, want, (tag, which, u))


# ---- case 1: the README example -------------------------------------------------------------------------------------
def check_readme(lib, oracle):
    lh, sol = os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol")
    oc = oracle.run_bfb(lh, [sol])["chr"][0]
    g = api.Graph(lib, lh); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    b.upload(); b.run(0); b.download()
    check_batch(b, [oc], "readme6")
    # README.md:122 by hand: 1+2+3+4+5+6+|6-5-4-3-2-|2+3+4+|4-3-|3+4+|4-3-2-|2+3+4+5+6+|6-5-4-3-2-1-
    #   '+' runs 1-6, 2-4, 3-4, 2-6: segment 1 once, 2 three times, 3 and 4 four times, 5 and 6 twice
    #   '-' runs 6-2, 4-3, 4-2, 6-1: segment 1 once, 2 three times, 3 and 4 four times, 5 and 6 twice
    #   8 runs, every '|' a fold-back turn (7), 32 cells, copy number 8 on segments 3 and 4
    b.profile(1); b.profile_wait()
    fwd, rev = b.unit_path_cn(0, 6)
    assert fwd.tolist() == [0, 1, 3, 4, 4, 2, 2] and rev.tolist() == [0, 1, 3, 4, 4, 2, 2]
    p = b.unit_profile(0)
    assert (p["status"], p["cells"], p["runs"], p["turns"], p["max_cn"], p["n_uncovered"]) == (0, 32, 8, 7, 8, 0), p
    b.close(); g.close()


# ---- case 2: the edge units of engine_checks.check_edge_cases -------------------------------------------------------
NOFBI = ("SAMPLE_NAME nofbi\nAVG_CHR_SEG_DP 30\nAVG_WHOLE_HOST_DP 30\nAVG_JUNC_DP 30\nPURITY 1\nAVG_TUMOR_PLOIDY 2\n"
         "PLOIDY 2m1\nVIRUS_START 5\nSOURCE 1\nSINK 4\n"
         "SEG H:1:chr1:1:10 30.0 1.0\nSEG H:2:chr1:11:20 30.0 1.0\nSEG H:3:chr1:21:30 30.0 1.0\nSEG H:4:chr1:31:40 30.0 1.0\n"
         "JUNC H:1:+ H:2:+ 30.0 1.0 U B\nJUNC H:2:+ H:3:+ 30.0 1.0 U B\nJUNC H:1:+ H:4:+ 30.0 1.0 U B\n")


def check_edge_units(lib, oracle, workdir):
    readme = os.path.join(cases.DATA, "readme6.lh")
    # (1) no fold-back inversion: the shortcut path 1+2+3+4+
    lh = os.path.join(workdir, "prof_nofbi.lh")
    with open(lh, "w") as f:
        f.write(NOFBI)
    g = api.Graph(lib, lh); b = api.Batch(lib)
    b.add_chromosome(g, 0, [], [])
    b.upload(); b.run(0); b.download()
    assert b.unit_result(0)["status"] == api.ST_SHORTCUT
    check_batch(b, [oracle.run_bfb(lh, [])["chr"][0]], "shortcut")
    fwd, rev = b.unit_path_cn(0, 4)
    assert fwd.tolist() == [0, 1, 1, 1, 1] and rev.tolist() == [0, 0, 0, 0, 0]
    p = b.unit_profile(0)
    assert (p["status"], p["cells"], p["runs"], p["turns"], p["max_cn"], p["n_uncovered"]) == (api.ST_SHORTCUT, 4, 1, 0, 1, 0), p
    b.close(); g.close()
    # (2) Infeasible .sol: the reference path over the six segments of the README example
    sol = os.path.join(workdir, "prof_infeasible.sol")
    with open(sol, "w") as f:
        f.write("Infeasible - objective value 0.00000000\n")
    g = api.Graph(lib, readme); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    b.upload(); b.run(0); b.download()
    assert b.unit_result(0)["status"] == api.ST_INFEASIBLE
    check_batch(b, [oracle.run_bfb(readme, [sol])["chr"][0]], "infeasible")
    fwd, rev = b.unit_path_cn(0, 6)
    assert fwd.tolist() == [0] + [1] * 6 and rev.tolist() == [0] * 7 and b.unit_profile(0)["cells"] == 6
    b.close(); g.close()
    # (3) a .sol that selects nothing: status -11, zero counts, cells = 0
    sol0 = os.path.join(workdir, "prof_empty.sol")
    with open(sol0, "w") as f:
        f.write("Optimal - objective value 0.00000000\n")
    g = api.Graph(lib, readme); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol0)
    b.upload(); b.run(0); b.download()
    for which in (0, 1):
        b.profile(which); b.profile_wait()
        fwd, rev = b.unit_path_cn(0, 6)
        assert fwd.tolist() == [0] * 7 and rev.tolist() == [0] * 7
        assert b.unit_profile(0) == dict(ZERO, status=-11)
    b.close(); g.close()


# ---- cases 3, 4: a batch above the express limit --------------------------------------------------------------------
_MANY = {}


def many_units(oracle, workdir, n_samples=40):
    """The units of engine_checks.check_batch_many_units (48 segments, chain / wide / mixed at K = 7, `imperfect` and `n_del`
    alternating) plus one duplication on every third; (lh, sol, oracle record) per unit, computed once."""
    key = (workdir, n_samples)
    if key not in _MANY:
        items = []
        for i in range(n_samples):
            tier, K = [("chain", 7), ("wide", 7), ("mixed", 7)][i % 3]
            s = synth.make_sample(48, 100, tier, K, seed=5000 + i, imperfect=i % 2, n_del=i % 2, n_dup=1 if i % 3 == 0 else 0)
            lh, sols = s.write(workdir, "pm%d" % i)
            items.append((lh, sols[0], oracle.run_bfb(lh, sols)["chr"][0]))
        _MANY[key] = items
    return _MANY[key]


def many_batch(lib, items):
    graphs, b = [], api.Batch(lib)
    for lh, sol, _ in items:
        g = api.Graph(lib, lh); graphs.append(g)
        b.add_chromosome_sol(g, 0, sol)
    return graphs, b


def close_all(graphs, b):
    b.close()
    for g in graphs:
        g.close()


def check_many_units(lib, oracle, workdir, window=None):
    """40 units through the ordinary kernels, both paths; a second run and a second profile give the same again (arrays that are
    not cleared, a stale epoch).  window: AMBI_PROFILE_WINDOW, so that 48 segments take several windows."""
    items = many_units(oracle, workdir)
    records = [oc for _, _, oc in items]
    assert any(oc["path_indel"] != oc["path"] for oc in records)      # indelBFB edits some: which = 0 and 1 differ
    saved = os.environ.pop("AMBI_PROFILE_WINDOW", None)
    if window:
        os.environ["AMBI_PROFILE_WINDOW"] = str(window)
    try:
        graphs, b = many_batch(lib, items)
        b.upload(); b.run(0); b.download()
        for u, oc in enumerate(records):        # precondition: the engine's paths are the oracle's
            assert b.unit_path(u, 0).tolist() == oc["path"] and b.unit_path(u, 1).tolist() == oc["path_indel"], u
        check_batch(b, records, ("many", window))
        b.run(0); b.download()
        check_batch(b, records, ("many, second run", window))
        close_all(graphs, b)
    finally:
        os.environ.pop("AMBI_PROFILE_WINDOW", None)
        if saved is not None:
            os.environ["AMBI_PROFILE_WINDOW"] = saved


# ---- case 5: three chromosomes of one sample (seg_base > 0) ---------------------------------------------------------
def check_three_chromosomes(lib, oracle, workdir):
    s = synth.make_sample(96, 200, "chain", 5, seed=11, n_chr=3, name="prof3chr")
    lh, sols = s.write(workdir)
    o = oracle.run_bfb(lh, sols)
    e = api.reconstruct_sample(lib, lh, sols, profile=True)
    assert o["ok"] and e["ok"] and len(o["chr"]) == 3 and o["chr"][1]["start"] > 1 and o["chr"][2]["start"] > o["chr"][1]["start"]
    for c, (oc, ec) in enumerate(zip(o["chr"], e["chr"])):
        assert ec["path_indel"] == oc["path_indel"], c
        st, en = oc["start"], oc["end"]
        n = en - st + 1
        seg_cn = np.concatenate([[0.0], np.asarray(oc["seg_cn"], float)[st - 1:en]])
        status = api.ST_SHORTCUT if oc["shortcut"] else (api.ST_INFEASIBLE if oc["infeasible"] else 0)
        fwd, rev, summary = expected(oc["path_indel"] or list(range(st, en + 1)), st - 1, n, ec["target_cn"], seg_cn, status)
        assert ec["path_cn_fwd"].tolist() == fwd.tolist() and ec["path_cn_rev"].tolist() == rev.tolist(), c
        assert ec["profile"] == summary, (c, ec["profile"], summary)
    assert "profile" not in api.reconstruct_sample(lib, lh, sols)["chr"][0]      # only when asked for


# ---- case 6: a bench-shaped unit finished at wait() ------------------------------------------------------------------
_BIG = {}


def big_unit(oracle, workdir):
    """256 segments, wide, K = 19, one deletion and one duplication (the bench unit's shape: ~14 000 cells).  Its verdicts are
    injected as engine_checks.check_injected_validity does: no order valid with the forward seed, so the scan (budget 4) ends
    PENDING, the parallel search at wait() flips the orientation and resolves order 0 -- the oracle's --reversed run."""
    if workdir not in _BIG:
        s = synth.make_sample(256, 512, "wide", 19, seed=2100, n_del=1, n_dup=1, name="profbig")
        lh, sols = s.write(workdir)
        plain = oracle.run_bfb(lh, sols)["chr"][0]
        rev = oracle.run_bfb(lh, sols, reversed_=True)["chr"][0]
        assert rev["first_valid"] == 0 and rev["first_forward"] == 0 and len(rev["path"]) > 8 * 256 * 4
        _BIG[workdir] = (lh, sols[0], plain["num_orders"], rev)
    return _BIG[workdir]


def check_big_unit_finished_at_wait(lib, oracle, workdir):
    lh, sol, R, rev = big_unit(oracle, workdir)
    items = many_units(oracle, workdir)[:39]
    graphs, b = [], api.Batch(lib)
    b.configure(first_budget=4)
    g = api.Graph(lib, lh); graphs.append(g)
    b.add_chromosome_sol(g, 0, sol)
    for l2, s2, _ in items:
        g = api.Graph(lib, l2); graphs.append(g)
        b.add_chromosome_sol(g, 0, s2)
    b.debug_inject_validity(0, [0] * R + [1] * R)
    records = [rev] + [oc for _, _, oc in items]
    b.upload()
    for which in (1, 0):
        b.run(0)
        b.profile(which)                 # queued behind a run whose unit 0 is still PENDING
        b.wait()                         # the parallel search finishes it
        b.profile_wait()                 # ... and the profile is that of the final results
        b.download()
        r = b.unit_result(0)
        assert (r["status"], r["first_valid"], r["first_forward"]) == (0, 0, 0), r
        assert b.unit_path(0, 0).tolist() == rev["path"] and b.unit_path(0, 1).tolist() == rev["path_indel"]     # precondition
        for u, oc in enumerate(records):
            n, want = unit_expectation(b, u, oc, which)
            compare_unit(b, u, n, want, ("big", which, u))
    assert b.unit_profile(0)["cells"] == len(rev["path"]) > 2048 * 4      # several tiles of 256 threads x 8 cells
    close_all(graphs, b)


# ---- case 6b: the queueing path's other branches ---------------------------------------------------------------------
def check_request_paths(lib, oracle, workdir, run_stream=None, req_stream=None):
    """A request on another stream than the run's (run_stream / req_stream: raw stream handles; None on the host simulation, where
    the same calls go through the default path), a request nobody waited for followed by another, and a batch closed with a
    request in flight whose lease the next batch takes over."""
    items = many_units(oracle, workdir)
    records = [oc for _, _, oc in items]
    graphs, b = many_batch(lib, items)
    b.upload()

    def compare(which, tag):
        for u, oc in enumerate(records):
            n, want = unit_expectation(b, u, oc, which)
            compare_unit(b, u, n, want, (tag, which, u))
    # (1) run on one stream, request on another, nothing waited for in between
    for which in (0, 1):
        b.run(0, run_stream)
        b.profile(which, req_stream); b.profile_wait()
        b.download()
        compare(which, "other stream")
    # the two paths give different profiles somewhere: (2) can tell which request the getters answer for
    assert any(unit_expectation(b, u, oc, 0)[1][0].tolist() != unit_expectation(b, u, oc, 1)[1][0].tolist() for u, oc in enumerate(records))
    # (2) a request nobody waited for, then another: the second one answers; again after another run; then a single request
    for k in range(2):
        b.run(0, run_stream)
        b.profile(0, req_stream); b.profile(1, req_stream); b.profile_wait()
        b.download()
        compare(1, ("unwaited", k))
    b.run(0, run_stream)
    b.profile(0, req_stream); b.profile_wait()
    b.download()
    compare(0, "single after unwaited")
    # (3) closed with a request in flight; the next batch (other units, other offsets) gets the lease back
    b.run(0, run_stream)
    b.profile(1, req_stream)
    close_all(graphs, b)
    sub = items[3:20]
    graphs, b = many_batch(lib, sub)
    b.upload(); b.run(0, run_stream); b.download()
    check_batch(b, [oc for _, _, oc in sub], "after a close in flight")
    close_all(graphs, b)


# ---- case 7: argument and state errors ------------------------------------------------------------------------------
def check_errors(lib):
    import pytest
    lh, sol = os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol")
    g = api.Graph(lib, lh); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    for call in (lambda: b.profile(1), b.profile_wait):
        with pytest.raises(api.AmbiError) as e:
            call()
        assert e.value.code == -32                         # AMBI_ERR_STATE: nothing uploaded
    b.upload()
    for call in (lambda: b.profile(1), b.profile_wait, lambda: b.unit_profile(0), lambda: b.unit_path_cn(0, 6)):
        with pytest.raises(api.AmbiError) as e:
            call()
        assert e.value.code == -32                         # uploaded, never run
    b.run(0); b.download()
    with pytest.raises(api.AmbiError) as e:
        b.unit_profile(0)
    assert e.value.code == -32                             # run, not profiled
    for which in (2, -1):
        with pytest.raises(api.AmbiError) as e:
            b.profile(which)
        assert e.value.code == -33                         # AMBI_ERR_ARG
    b.profile(1); b.profile_wait()
    import ctypes
    buf = (ctypes.c_int32 * 8)()
    assert lib.ambi_batch_unit_path_cn(b.h, 0, buf, buf, 6) < 0       # cap < n + 1
    assert lib.ambi_batch_unit_path_cn(b.h, 0, buf, None, 7) == 7
    with pytest.raises(api.AmbiError):
        b.unit_profile(1)                                  # no such unit
    b.run(0)
    with pytest.raises(api.AmbiError) as e:
        b.unit_profile(0)
    assert e.value.code == -32                             # a new run: the old profile is gone
    b.wait()
    b.close(); g.close()


# ---- case 9: the CLI ------------------------------------------------------------------------------------------------
def check_cli(lib, exe, cwd, oracle):
    import test_cli_dropin as t
    lh, sol = os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol")
    outs = []
    for k, extra in enumerate(([], ["--cn_profile", "cn.tsv"])):
        sub = os.path.join(cwd, "run%d" % k)
        os.makedirs(sub)
        bindir = os.path.join(sub, "bin")
        t.fake_cbc(bindir, [sol])
        r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", lh, "--lp_prefix", "readme", *extra)
        assert r.returncode == 0, r.stderr
        outs.append((r.stdout, r.stderr, open(os.path.join(sub, "simulation_sv.txt")).read(), sorted(x for x in os.listdir(sub) if x != "bin")))
    assert outs[0][:3] == outs[1][:3]                                      # stdout, stderr, side file: unchanged by the option
    assert outs[1][3] == sorted(outs[0][3] + ["cn.tsv"])
    # expected rows: sample, chromosome, id, start, end, input CN (%g), target CN, forward, reverse, count - target
    segs = [l.split() for l in open(lh) if l.startswith("SEG ")]
    oc = oracle.run_bfb(lh, [sol])["chr"][0]
    g = api.Graph(lib, lh); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    b.upload(); b.run(0); b.download()
    target = b.unit_prepare(0, 6)["target_cn"]
    b.close(); g.close()
    fwd, rev, _ = expected(oc["path_indel"], 0, 6, target, np.zeros(7), 0)
    want = []
    for i, tk in enumerate(segs, 1):
        _, sid, chrom, start, end = tk[1].split(":")
        assert int(sid) == i
        want.append("\t".join([lh, chrom, sid, start, end, "%g" % float(tk[3]), str(target[i]), str(fwd[i]), str(rev[i]), str(fwd[i] + rev[i] - target[i])]))
    got = open(os.path.join(cwd, "run1", "cn.tsv")).read().splitlines()
    assert got == want and len(got) == 6
    # a PROP C2 sample: its printed paths are rebuilt on the host -- refused, exit status 2, no file
    sub = os.path.join(cwd, "c2")
    os.makedirs(sub)
    bindir = os.path.join(sub, "bin")
    t.fake_cbc(bindir, [os.path.join(cases.DATA, "readme_c2_chr0.sol"), os.path.join(cases.DATA, "readme_c2_chr1.sol")])
    r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", os.path.join(cases.DATA, "readme_c2.lh"), "--lp_prefix", "c2", "--cn_profile", "cn.tsv")
    assert r.returncode == 2 and "--cn_profile" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(os.path.join(sub, "cn.tsv"))
    r = t.run_cli(exe, sub, bindir, "--help")
    assert "--cn_profile" in r.stdout
