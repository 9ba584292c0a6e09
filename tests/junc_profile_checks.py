"""Checks of the junction usage profile (ambi_batch_junc_profile, csrc/ambi_junc_profile.hpp) shared by the CPU host-simulation
tests and the GPU tests (same assertions, different library).

Expected values never come from the stage under test: a plain Python walk (a dict over both edges of every junction, lowest
index first) over the ORACLE's path of the unit and the JUNC lines of the .lh.  Hand-built raw units, which no file describes,
use the engine's own unit_path (pinned by the parity tests) and the arrays handed to add_unit."""
import ctypes
import os

import numpy as np

import cases
import profile_checks as pc
from ambigram_amd import api, synth

FIELDS = ("status", "steps", "steps_matched", "steps_unmatched", "first_unmatched", "juncs", "juncs_used", "max_count", "n_over", "n_under")
ZERO = dict.fromkeys(FIELDS, 0)
_SIGN = {"+": 1, "-": -1}


# ---- the plain walk ---------------------------------------------------------------------------------------------------
def walk(path_local, ends, cn, status=0):
    """(count[m], summary, steps matched through edge B only) of a path of LOCAL signed ids over the junctions `ends` = [(s, t)]."""
    m = len(ends)
    if status < 0 or len(path_local) == 0:
        return [0] * m, dict(ZERO, status=status), 0
    edge = {}
    for j, (s, t) in enumerate(ends):                   # lowest index first: setdefault keeps it
        edge.setdefault((s, t), j)
        edge.setdefault((-t, -s), j)
    count, unmatched, first, via_b = [0] * m, 0, -1, 0
    for i in range(len(path_local) - 1):
        step = (path_local[i], path_local[i + 1])
        j = edge.get(step)
        if j is None:
            unmatched += 1
            if first < 0:
                first = i
        else:
            count[j] += 1
            via_b += step != tuple(ends[j])
    steps = len(path_local) - 1
    s = dict(status=status, steps=steps, steps_matched=sum(count), steps_unmatched=unmatched, first_unmatched=first, juncs=m,
             juncs_used=sum(c > 0 for c in count), max_count=max(count, default=0),
             n_over=sum(c - x >= 0.5 for c, x in zip(count, cn)), n_under=sum(x - c >= 0.5 for c, x in zip(count, cn)))
    assert s["steps_matched"] + s["steps_unmatched"] == steps
    return count, s, via_b


def lh_junctions(lh):
    """The JUNC lines of a .lh as (src, sdir, tgt, tdir) in file order; a second copy of an edge (either side) is dropped, as the
    reader drops it (lh_graph.cpp:81)."""
    out, seen = [], set()
    for line in open(lh):
        if not line.startswith("JUNC "):
            continue
        a, b = line.split()[1:3]
        s, sd, t, td = int(a.split(":")[1]), _SIGN[a.split(":")[2]], int(b.split(":")[1]), _SIGN[b.split(":")[2]]
        e = (s * sd, t * td)
        if e in seen or (-e[1], -e[0]) in seen:
            continue
        seen.add(e)
        out.append((s, sd, t, td))
    return out


def unit_junctions(lh, g, start, end):
    """(graph indices, local strand-signed ends, cn) of the junctions with both ends inside [start, end], from the file's JUNC lines;
    the copy numbers are the graph's (the values that are uploaded)."""
    J = lh_junctions(lh)
    gj = g.junctions()
    assert [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(gj["src"], gj["sdir"], gj["tgt"], gj["tdir"])] == J      # file order, nothing added
    idx = [j for j, (s, _, t, _) in enumerate(J) if start <= s <= end and start <= t <= end]
    base = start - 1
    ends = [((J[j][0] - base) * J[j][1], (J[j][2] - base) * J[j][3]) for j in idx]
    return idx, ends, [float(gj["cn"][j]) for j in idx]


def local_path(path_abs, base):
    return [v - base if v > 0 else v + base for v in path_abs]


def oracle_path(oc, which):
    path = oc["path_indel"] if which else oc["path"]
    if (oc["shortcut"] or oc["infeasible"]) and not path:
        path = list(range(oc["start"], oc["end"] + 1))      # the reference path 1+ .. n+ (localhap.cpp:164-170, :213-220)
    return local_path(path, oc["start"] - 1)


def oracle_status(oc):
    return api.ST_SHORTCUT if oc["shortcut"] else (api.ST_INFEASIBLE if oc["infeasible"] else 0)


def unit_expectation(lh, g, oc, which, status=None):
    idx, ends, cn = unit_junctions(lh, g, oc["start"], oc["end"])
    count, summary, via_b = walk(oracle_path(oc, which), ends, cn, oracle_status(oc) if status is None else status)
    return idx, count, summary, via_b


def compare_unit(b, u, idx, count, summary, tag):
    got, gidx = b.unit_junc_usage(u)
    assert gidx.tolist() == list(idx), (tag, "graph_index", gidx.tolist(), idx)
    assert got.tolist() == list(count), (tag, "count", got.tolist(), count)
    s = b.unit_junc_profile(u)
    assert s == summary, (tag, s, summary)
    assert int(got.sum()) == s["steps_matched"] and s["steps_matched"] + s["steps_unmatched"] == s["steps"], (tag, s)


def check_batch(b, items, tag, whichs=(0, 1)):
    """items: (lh, graph, oracle record) per unit of a batch that has run."""
    for which in whichs:
        b.junc_profile(which); b.junc_profile_wait()
        for u, (lh, g, oc) in enumerate(items):
            idx, count, summary, _ = unit_expectation(lh, g, oc, which)
            compare_unit(b, u, idx, count, summary, (tag, which, u))


class _Env:
    """AMBI_JPROFILE_JUNC_WINDOW / AMBI_JPROFILE_SEG_WINDOW for the calls inside."""
    def __init__(self, jwin=None, swin=None):
        self.want = {"AMBI_JPROFILE_JUNC_WINDOW": jwin, "AMBI_JPROFILE_SEG_WINDOW": swin}

    def __enter__(self):
        self.saved = {k: os.environ.pop(k, None) for k in self.want}
        for k, v in self.want.items():
            if v:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---- case 1: the README example -------------------------------------------------------------------------------------
def check_readme(lib, oracle):
    lh, sol = os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol")
    oc = oracle.run_bfb(lh, [sol])["chr"][0]
    g = api.Graph(lib, lh); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    b.upload(); b.run(0); b.download()
    check_batch(b, [(lh, g, oc)], "readme6")
    # By hand.  README.md:122: 1+2+3+4+5+6+|6-5-4-3-2-|2+3+4+|4-3-|3+4+|4-3-2-|2+3+4+5+6+|6-5-4-3-2-1-   (32 cells, 31 steps)
    # The file's junctions, edge A and its complement B:
    #   0  H:2:- H:2:+  (-2, 2), B = (-2, 2)      1  H:3:- H:3:+  (-3, 3), B = (-3, 3)
    #   2  H:4:+ H:4:-  (4, -4), B = (4, -4)      3  H:6:- H:6:+  (-6, 6), B = (-6, 6)
    # The seven '|' are the steps (6,-6) (-2,2) (4,-4) (-3,3) (4,-4) (-2,2) (6,-6): junction 0 twice, 1 once, 2 twice; the turn
    # 6+|6- is the edge (6,-6), which is NOT junction 3's edge (-6,6): 2 steps without a junction.  The file lists no adjacency
    # i+ -> (i+1)+, so the 24 in-run steps match nothing either, the first of them at step 0.
    # cn (2, 1, 2, 2) against (2, 1, 2, 0): one junction under, none over.
    b.junc_profile(1); b.junc_profile_wait()
    count, gidx = b.unit_junc_usage(0)
    assert count.tolist() == [2, 1, 2, 0] and gidx.tolist() == [0, 1, 2, 3]
    assert b.unit_junc_profile(0) == dict(status=0, steps=31, steps_matched=5, steps_unmatched=26, first_unmatched=0, juncs=4, juncs_used=3,
                                          max_count=2, n_over=0, n_under=1)
    b.close(); g.close()


# ---- case 2: edge units ---------------------------------------------------------------------------------------------
ONESEG = ("SAMPLE_NAME oneseg\nAVG_CHR_SEG_DP 30\nAVG_WHOLE_HOST_DP 30\nAVG_JUNC_DP 30\nPURITY 1\nAVG_TUMOR_PLOIDY 2\n"
          "PLOIDY 2m1\nVIRUS_START 5\nSOURCE 1\nSINK 1\nSEG H:1:chr1:1:10 30.0 1.0\n")


def check_edge_units(lib, oracle, workdir):
    readme = os.path.join(cases.DATA, "readme6.lh")
    # (1) no fold-back inversion: the shortcut path 1+2+3+4+, every adjacency once, the junction 1+ -> 4+ unused, nothing unmatched
    lh = os.path.join(workdir, "jp_nofbi.lh")
    with open(lh, "w") as f:
        f.write(pc.NOFBI + "JUNC H:3:+ H:4:+ 30.0 1.0 U B\n")
    g = api.Graph(lib, lh); b = api.Batch(lib)
    b.add_chromosome(g, 0, [], [])
    b.upload(); b.run(0); b.download()
    assert b.unit_result(0)["status"] == api.ST_SHORTCUT
    check_batch(b, [(lh, g, oracle.run_bfb(lh, [])["chr"][0])], "shortcut")
    assert b.unit_junc_usage(0)[0].tolist() == [1, 1, 0, 1]
    p = b.unit_junc_profile(0)
    assert (p["status"], p["steps"], p["steps_matched"], p["steps_unmatched"], p["first_unmatched"], p["juncs_used"]) == (api.ST_SHORTCUT, 3, 3, 0, -1, 3), p
    b.close(); g.close()
    # (2) Infeasible .sol: the reference path over the six segments of the README example (no adjacency in the file: 5 unmatched)
    sol = os.path.join(workdir, "jp_infeasible.sol")
    with open(sol, "w") as f:
        f.write("Infeasible - objective value 0.00000000\n")
    g = api.Graph(lib, readme); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    b.upload(); b.run(0); b.download()
    assert b.unit_result(0)["status"] == api.ST_INFEASIBLE
    check_batch(b, [(readme, g, oracle.run_bfb(readme, [sol])["chr"][0])], "infeasible")
    p = b.unit_junc_profile(0)
    assert (p["steps"], p["steps_matched"], p["steps_unmatched"], p["first_unmatched"], p["juncs"]) == (5, 0, 5, 0, 4), p
    b.close(); g.close()
    # (3) a .sol that selects nothing: status -11, zero counts, a summary that is zero but for the status
    sol0 = os.path.join(workdir, "jp_empty.sol")
    with open(sol0, "w") as f:
        f.write("Optimal - objective value 0.00000000\n")
    g = api.Graph(lib, readme); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol0)
    b.upload(); b.run(0); b.download()
    for which in (0, 1):
        b.junc_profile(which); b.junc_profile_wait()
        assert b.unit_junc_usage(0)[0].tolist() == [0] * 4
        assert b.unit_junc_profile(0) == dict(ZERO, status=-11)
    b.close(); g.close()
    # (4) one segment: a path of one cell, no step
    lh = os.path.join(workdir, "jp_oneseg.lh")
    with open(lh, "w") as f:
        f.write(ONESEG)
    g = api.Graph(lib, lh); b = api.Batch(lib)
    b.add_chromosome(g, 0, [], [])
    b.upload(); b.run(0); b.download()
    assert b.unit_path(0, 1).tolist() == [1]
    b.junc_profile(1); b.junc_profile_wait()
    st = b.unit_result(0)["status"]
    assert b.unit_junc_profile(0) == dict(ZERO, status=st, first_unmatched=-1) and st >= 0
    assert b.unit_junc_usage(0)[0].tolist() == []
    b.close(); g.close()


# ---- cases 3, 4: the 40 units of profile_checks.many_units ----------------------------------------------------------
def many_items(lib, oracle, workdir):
    items = pc.many_units(oracle, workdir)
    graphs, b = pc.many_batch(lib, items)
    return graphs, b, [(lh, g, oc) for (lh, _, oc), g in zip(items, graphs)]


def check_fixture_conditions(items):
    """What the 40 units must offer for the comparison to mean something, from the oracle's paths alone."""
    some_unmatched = via_b = differ = 0
    for lh, g, oc in items:
        _, c1, s1, b1 = unit_expectation(lh, g, oc, 1)
        _, c0, _, b0 = unit_expectation(lh, g, oc, 0)
        some_unmatched += s1["steps_unmatched"] > 0
        via_b += b0 + b1
        differ += c0 != c1
        assert min(c1) == 0 and max(c1) >= 2, (lh, "a junction with count 0 and one with count >= 2 in every unit")
    assert some_unmatched >= 1 and via_b >= 1 and differ >= 1, (some_unmatched, via_b, differ)


def check_many_units(lib, oracle, workdir, jwin=None, swin=None):
    """40 units through the ordinary kernels, both paths; a second run and a second request give the same again (arrays that are not
    cleared, a stale epoch).  jwin / swin: the window switches, so that 100 junctions and 48 segments take several passes -- the
    expectation does not know about windows, so the results equal the one-window results."""
    with _Env(jwin, swin):
        graphs, b, items = many_items(lib, oracle, workdir)
        check_fixture_conditions(items)
        b.upload(); b.run(0); b.download()
        for u, (_, _, oc) in enumerate(items):        # precondition: the engine's paths are the oracle's
            assert b.unit_path(u, 0).tolist() == oc["path"] and b.unit_path(u, 1).tolist() == oc["path_indel"], u
        check_batch(b, items, ("many", jwin, swin))
        b.run(0); b.download()
        check_batch(b, items, ("many, second run", jwin, swin))
        pc.close_all(graphs, b)


# ---- case 5: hand-built raw units ------------------------------------------------------------------------------------
def _raw_source(lib, workdir):
    """A synthetic unit's arrays: segments, junctions (file order) and the planted elements."""
    s = synth.make_sample(48, 100, "chain", 7, seed=5000, name="jpraw")
    lh, _ = s.write(workdir)
    g = api.Graph(lib, lh)
    seg_cn = g.segments()["cn"].tolist()
    gj = g.junctions()
    J = [(int(a), int(b), int(c), int(d), float(e)) for a, b, c, d, e in zip(gj["src"], gj["sdir"], gj["tgt"], gj["tdir"], gj["cn"])]
    g.close()
    assert s.chr_ranges[0] == (1, 48)
    return seg_cn, J, s.elements[0]


def _add_raw(b, seg_cn, J, elements):
    return b.add_unit(len(seg_cn), 0, seg_cn, [j[0] for j in J], [j[2] for j in J], [j[1] for j in J], [j[3] for j in J], [j[4] for j in J],
                      [1 if e.kind == "l" else 0 for e in elements], [e.a for e in elements], [e.b for e in elements], [e.cn for e in elements])


def check_raw_units(lib, workdir):
    seg_cn, J, elements = _raw_source(lib, workdir)
    b = api.Batch(lib)                                                                          # the plain unit first: which junctions its path takes
    _add_raw(b, seg_cn, J, elements)
    b.upload(); b.run(0); b.download()
    plain, _, _ = walk(b.unit_path(0, 1).tolist(), [(x[0] * x[1], x[2] * x[3]) for x in J], [x[4] for x in J])
    b.close()
    fb = next(j for j, x in enumerate(J) if x[0] == x[2] and x[1] != x[3] and plain[j] > 0)    # a fold-back (s, -s) the path turns at
    adj = [j for j, x in enumerate(J) if x[1] == x[3] == 1 and x[2] == x[0] + 1]
    assert len(adj) == 47
    flip = lambda x, cn: (x[2], -x[3], x[0], -x[1], cn)                                         # the same edge from the other side
    lists = {}
    # the same edge twice and once more from the other side, all at higher indices than the original (an adjacency and the fold-back)
    lists["duplicates"] = J + [J[adj[10]][:4] + (9.0,), flip(J[adj[10]], 8.0), J[fb][:4] + (7.0,), flip(J[fb], 6.0)]
    # ... and with the copies in FRONT: the original loses
    lists["duplicates_first"] = [flip(J[adj[10]], 8.0), J[fb][:4] + (7.0,)] + J
    lists["no_adjacency_20"] = [x for j, x in enumerate(J) if j != adj[19]]                      # 20+ -> 21+ removed
    lists["no_junctions"] = []
    units = {}
    b = api.Batch(lib)
    for name, L in lists.items():
        units[name] = _add_raw(b, seg_cn, L, elements)
    b.upload(); b.run(0); b.download()
    checked = 0
    for which in (0, 1):
        b.junc_profile(which); b.junc_profile_wait()
        for name, L in lists.items():
            u = units[name]
            st = b.unit_result(u)["status"]
            if st < 0:
                continue                                                                            # (kept: units that still reconstruct)
            path = b.unit_path(u, which).tolist()
            ends = [(x[0] * x[1], x[2] * x[3]) for x in L]
            count, summary, _ = walk(path, ends, [x[4] for x in L], st)
            compare_unit(b, u, list(range(len(L))), count, summary, (name, which))
            checked += 1
            if name == "duplicates":
                m = len(J)
                assert count[m:] == [0, 0, 0, 0] and count[adj[10]] > 0 and count[fb] > 0, (name, count[m:], count[adj[10]], count[fb])
                turns = sum(1 for i in range(len(path) - 1) if (path[i], path[i + 1]) == ends[fb])
                assert count[fb] == turns >= 1                                                      # once per turn, not twice
            if name == "duplicates_first":
                assert count[0] > 0 and count[1] > 0 and count[2 + adj[10]] == 0 and count[2 + fb] == 0
            if name == "no_adjacency_20":
                lost = [i for i in range(len(path) - 1) if (path[i], path[i + 1]) in ((20, 21), (-21, -20))]
                assert lost and summary["first_unmatched"] == lost[0] and summary["steps_unmatched"] >= len(lost)
            if name == "no_junctions":
                assert summary["juncs"] == 0 and summary["steps_unmatched"] == summary["steps"] and summary["first_unmatched"] == (0 if len(path) > 1 else -1)
    assert checked >= 6, checked
    b.close()


# ---- case 6: one bench-tier unit beside a few small ones -------------------------------------------------------------
def check_bench_unit(lib, oracle, workdir):
    s = synth.make_sample(256, 512, "wide", 19, seed=2100, n_del=1, n_dup=1, name="jpbig")
    lh, sols = s.write(workdir)
    big = oracle.run_bfb(lh, sols)["chr"][0]
    assert len(big["path_indel"]) > 2048 * 4                     # several tiles of 256 threads x 8 cells
    small = pc.many_units(oracle, workdir)[:3]
    graphs, b, items = [], api.Batch(lib), []
    for l2, s2, oc in [(lh, sols[0], big)] + small:
        g = api.Graph(lib, l2); graphs.append(g)
        b.add_chromosome_sol(g, 0, s2)
        items.append((l2, g, oc))
    assert len(unit_junctions(lh, graphs[0], 1, 256)[0]) >= 400   # a table of about a thousand slots
    b.upload(); b.run(0); b.download()
    assert b.unit_path(0, 1).tolist() == big["path_indel"]
    check_batch(b, items, "bench unit")
    pc.close_all(graphs, b)


# ---- case 7: three chromosomes of one sample ------------------------------------------------------------------------
def check_three_chromosomes(lib, oracle, workdir):
    s = synth.make_sample(96, 200, "chain", 5, seed=11, n_chr=3, name="jp3chr")
    lh, sols = s.write(workdir)
    # two junctions between chromosomes: they belong to no unit
    a, c = s.chr_ranges[0][0] + 3, s.chr_ranges[1][0] + 5
    with open(lh, "a") as f:
        f.write("JUNC H:%d:+ H:%d:+ 30.0 1.0 U B\nJUNC H:%d:- H:%d:+ 30.0 1.0 U B\n" % (a, c, s.chr_ranges[2][0] + 1, a))
    o = oracle.run_bfb(lh, sols)
    e = api.reconstruct_sample(lib, lh, sols, junc_profile=True)
    assert o["ok"] and e["ok"] and len(o["chr"]) == 3 and o["chr"][2]["start"] > o["chr"][1]["start"] > 1
    g = api.Graph(lib, lh)
    J = lh_junctions(lh)
    between = [j for j, (x, _, y, _) in enumerate(J) if not any(lo <= x <= hi and lo <= y <= hi for lo, hi in s.chr_ranges)]
    assert len(between) >= 2
    owned = set()
    for ci, (oc, ec) in enumerate(zip(o["chr"], e["chr"])):
        assert ec["path_indel"] == oc["path_indel"], ci
        idx, count, summary, _ = unit_expectation(lh, g, oc, 1)
        assert ec["junc_graph_index"].tolist() == idx and ec["junc_profile"] == summary, (ci, ec["junc_profile"], summary)
        want = np.zeros(len(J), np.int32)
        want[idx] = count
        assert ec["junc_count"].tolist() == want.tolist(), ci
        for j in idx:                                           # graph_index maps back to the graph's junctions, inside the chromosome
            assert oc["start"] <= J[j][0] <= oc["end"] and oc["start"] <= J[j][2] <= oc["end"]
        assert not owned & set(idx)
        owned |= set(idx)
        assert all(ec["junc_count"][j] == 0 for j in between)
    assert not owned & set(between) and len(owned) + len(between) == len(J)
    assert "junc_count" not in api.reconstruct_sample(lib, lh, sols)["chr"][0]      # only when asked for
    g.close()


# ---- case 8: a bench-shaped unit finished at wait() ------------------------------------------------------------------
def check_big_unit_finished_at_wait(lib, oracle, workdir):
    lh, sol, R, rev = pc.big_unit(oracle, workdir)
    small = pc.many_units(oracle, workdir)[:39]
    graphs, b, items = [], api.Batch(lib), []
    b.configure(first_budget=4)
    for l2, s2, oc in [(lh, sol, rev)] + small:
        g = api.Graph(lib, l2); graphs.append(g)
        b.add_chromosome_sol(g, 0, s2)
        items.append((l2, g, oc))
    b.debug_inject_validity(0, [0] * R + [1] * R)
    b.upload()
    for which in (1, 0):
        b.run(0)
        b.junc_profile(which)            # queued behind a run whose unit 0 is still PENDING
        b.wait()                         # the parallel search finishes it
        b.junc_profile_wait()            # ... and the profile is that of the final results
        b.download()
        r = b.unit_result(0)
        assert (r["status"], r["first_valid"], r["first_forward"]) == (0, 0, 0), r
        assert b.unit_path(0, 0).tolist() == rev["path"] and b.unit_path(0, 1).tolist() == rev["path_indel"]     # precondition
        for u, (l2, g, oc) in enumerate(items):
            idx, count, summary, _ = unit_expectation(l2, g, oc, which)
            compare_unit(b, u, idx, count, summary, ("big", which, u))
    assert b.unit_junc_profile(0)["steps"] == len(rev["path"]) - 1 > 2048 * 4
    pc.close_all(graphs, b)


# ---- case 8b: the queueing path's other branches ---------------------------------------------------------------------
def check_request_paths(lib, oracle, workdir, run_stream=None, req_stream=None):
    """As profile_checks.check_request_paths: a request on another stream than the run's (None on the host simulation), a request
    nobody waited for followed by another, and a batch closed with a request in flight whose lease the next batch takes over."""
    graphs, b, items = many_items(lib, oracle, workdir)
    b.upload()

    def compare(which, tag):
        for u, (lh, g, oc) in enumerate(items):
            idx, count, summary, _ = unit_expectation(lh, g, oc, which)
            compare_unit(b, u, idx, count, summary, (tag, which, u))
    # (1) run on one stream, request on another, nothing waited for in between
    for which in (0, 1):
        b.run(0, run_stream)
        b.junc_profile(which, req_stream); b.junc_profile_wait()
        compare(which, "other stream")
    # the two paths give different counts somewhere: (2) can tell which request the getters answer for
    assert any(unit_expectation(lh, g, oc, 0)[1] != unit_expectation(lh, g, oc, 1)[1] for lh, g, oc in items)
    # (2) a request nobody waited for, then another: the second one answers; again after another run; then a single request
    for k in range(2):
        b.run(0, run_stream)
        b.junc_profile(0, req_stream); b.junc_profile(1, req_stream); b.junc_profile_wait()
        compare(1, ("unwaited", k))
    b.run(0, run_stream)
    b.junc_profile(0, req_stream); b.junc_profile_wait()
    compare(0, "single after unwaited")
    # (3) closed with a request in flight; the next batch (other units, other offsets) gets the lease back
    b.run(0, run_stream)
    b.junc_profile(1, req_stream)
    pc.close_all(graphs, b)
    sub = pc.many_units(oracle, workdir)[3:20]
    graphs, b = pc.many_batch(lib, sub)
    b.upload(); b.run(0, run_stream)
    check_batch(b, [(lh, g, oc) for (lh, _, oc), g in zip(sub, graphs)], "after a close in flight")
    pc.close_all(graphs, b)


# ---- case 9: sharded -------------------------------------------------------------------------------------------------
def check_sharded(lib, oracle, workdir, devices):
    import pytest
    graphs, b, items = many_items(lib, oracle, workdir)
    b.run_sharded(0, devices=devices)
    check_batch(b, items, ("sharded", tuple(devices)))
    with pytest.raises(api.AmbiError) as e:
        b.junc_profile_device()          # one block per share: no single device view
    assert e.value.code == -32
    pc.close_all(graphs, b)


# ---- case 10: the CLI ------------------------------------------------------------------------------------------------
def check_cli(lib, exe, cwd, oracle, workdir):
    import test_cli_dropin as t
    readme, rsol = os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol")
    lh2, sol2, _ = pc.many_units(oracle, workdir)[1]
    outs = []
    for k, extra in enumerate(([], ["--junc_profile", "junc.tsv"])):
        sub = os.path.join(cwd, "run%d" % k)
        os.makedirs(sub)
        bindir = os.path.join(sub, "bin")
        t.fake_cbc(bindir, [rsol, sol2])
        r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", readme + "," + lh2, "--lp_prefix", "two", *extra)
        assert r.returncode == 0, r.stderr
        outs.append((r.stdout, r.stderr, open(os.path.join(sub, "simulation_sv.txt"), "rb").read(), sorted(x for x in os.listdir(sub) if x != "bin")))
    assert outs[0][:3] == outs[1][:3]                                      # stdout, stderr, side file: unchanged by the option
    assert outs[1][3] == sorted(outs[0][3] + ["junc.tsv"])
    want = []
    for lh, sol in ((readme, rsol), (lh2, sol2)):
        oc = oracle.run_bfb(lh, [sol])["chr"][0]
        g = api.Graph(lib, lh)
        idx, count, _, _ = unit_expectation(lh, g, oc, 1)
        gj = g.junctions()
        names = {}
        for line in open(lh):
            if line.startswith("SEG "):
                _, sid, chrom = line.split()[1].split(":")[:3]
                names[int(sid)] = chrom
        per = dict(zip(idx, count))
        for j, (s, sd, tt, td) in enumerate(lh_junctions(lh)):
            c = per.get(j, 0)
            cn = float(gj["cn"][j])
            want.append("\t".join([lh, "0" if j in per else "-1", names[s], str(s), "+" if sd > 0 else "-", names[tt], str(tt), "+" if td > 0 else "-",
                                   "%g" % cn, str(c), "%g" % (c - cn)]))
        g.close()
    got = open(os.path.join(cwd, "run1", "junc.tsv")).read().splitlines()
    assert got == want and len(got) > 100
    # a PROP C2 sample: its printed paths are rebuilt on the host -- refused, exit status 2, no file
    sub = os.path.join(cwd, "c2")
    os.makedirs(sub)
    bindir = os.path.join(sub, "bin")
    t.fake_cbc(bindir, [os.path.join(cases.DATA, "readme_c2_chr0.sol"), os.path.join(cases.DATA, "readme_c2_chr1.sol")])
    r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", os.path.join(cases.DATA, "readme_c2.lh"), "--lp_prefix", "c2", "--junc_profile", "junc.tsv")
    assert r.returncode == 2 and "--junc_profile" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(os.path.join(sub, "junc.tsv"))
    r = t.run_cli(exe, sub, bindir, "--help")
    assert "--junc_profile" in r.stdout


# ---- case 11: argument and state errors ------------------------------------------------------------------------------
def check_errors(lib):
    import pytest
    lh, sol = os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol")
    g = api.Graph(lib, lh); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    for call in (lambda: b.junc_profile(1), b.junc_profile_wait):
        with pytest.raises(api.AmbiError) as e:
            call()
        assert e.value.code == -32                         # AMBI_ERR_STATE: nothing uploaded
    b.upload()
    for call in (lambda: b.junc_profile(1), b.junc_profile_wait, lambda: b.unit_junc_profile(0), lambda: b.unit_junc_usage(0)):
        with pytest.raises(api.AmbiError) as e:
            call()
        assert e.value.code == -32                         # uploaded, never run
    b.run(0); b.download()
    with pytest.raises(api.AmbiError) as e:
        b.unit_junc_profile(0)
    assert e.value.code == -32                             # run, not profiled
    with pytest.raises(api.AmbiError) as e:
        b.junc_profile_wait()
    assert e.value.code == -32                             # nothing queued
    for which in (2, -1):
        with pytest.raises(api.AmbiError) as e:
            b.junc_profile(which)
        assert e.value.code == -33                         # AMBI_ERR_ARG
    b.junc_profile(1); b.junc_profile_wait()
    buf = (ctypes.c_int32 * 8)()
    assert lib.ambi_batch_unit_junc_usage(b.h, 0, buf, buf, 3) == -33      # cap < m
    assert lib.ambi_batch_unit_junc_usage(b.h, 0, buf, None, 4) == 4 and list(buf[:4]) == [2, 1, 2, 0]
    assert lib.ambi_batch_unit_junc_usage(b.h, 0, None, buf, 4) == 4 and list(buf[:4]) == [0, 1, 2, 3]
    for u in (1, -1):
        with pytest.raises(api.AmbiError) as e:
            b.unit_junc_profile(u)                         # no such unit
        assert e.value.code == -33
        assert lib.ambi_batch_unit_junc_usage(b.h, u, buf, buf, 8) == -33
    b.run(0)
    with pytest.raises(api.AmbiError) as e:
        b.unit_junc_profile(0)
    assert e.value.code == -32                             # a new run: the old profile is gone
    b.wait()
    b.close(); g.close()
