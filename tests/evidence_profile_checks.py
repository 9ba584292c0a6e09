"""Checks of the evidence depth profile (ambi_batch_evidence_profile, csrc/ambi_evidence_profile.hpp) shared by the CPU host-simulation
tests and the GPU tests (same assertions, different library).

Expected values never come from the stages under test: a plain Python walk written from the definitions -- depth[k] = occurrences,
over all fragments and both directions, whose window covers step k; per junction the credited steps, those of them with depth > 0
and their minimum depth -- over the ORACLE's path of the unit, with the unit's junction list from
junc_profile_checks.unit_expectation's source (the file's JUNC lines).  Hand-built raw units, which no file describes, use the
engine's own unit_path (pinned by the parity tests)."""
import ctypes
import os

import numpy as np

import cases
import frag_profile_checks as fc
import junc_profile_checks as jc
import profile_checks as pc
from ambigram_amd import api, synth

FIELDS = ("status", "steps", "steps_covered", "max_depth", "first_uncovered", "longest_uncovered", "longest_uncovered_at", "juncs",
          "juncs_used", "juncs_covered", "juncs_uncovered", "unmatched_covered", "depth_sum")
ZERO = dict(dict.fromkeys(FIELDS, 0), first_uncovered=-1, longest_uncovered_at=-1)
FLOORS = ("uncovered", "all_covered", "depth3", "partly", "fully_multi", "used_uncovered", "step0_cov", "step0_unc", "last_cov", "last_unc")
_raises = fc._raises


# ---- the plain walk ---------------------------------------------------------------------------------------------------
def walk_depth(path, frags):
    depth = [0] * max(len(path) - 1, 0)
    for f in frags:
        f = list(f)
        pats = [f] if fc.rc(f) == f else [f, fc.rc(f)]
        for p in pats:
            for i in fc.positions(path, p):
                for k in range(i, i + len(p) - 1):
                    depth[k] += 1
    return depth


def walk(path_local, frags, ends, status=0, floors=None):
    """(depth[P-1], count[m], covered[m], min_depth[m], summary) of a path of LOCAL signed ids over the fragments and the junctions."""
    m = len(ends)
    if status < 0 or len(path_local) == 0:
        return [], [0] * m, [0] * m, [-1] * m, dict(ZERO, status=status, juncs=m)
    path = list(path_local)
    depth = walk_depth(path, frags)
    steps = len(path) - 1
    edge = {}
    for j, (s, t) in enumerate(ends):                   # lowest index first: setdefault keeps it
        edge.setdefault((s, t), j)
        edge.setdefault((-t, -s), j)
    count, covered, mind, unmatched_cov = [0] * m, [0] * m, [None] * m, 0
    for k in range(steps):
        j = edge.get((path[k], path[k + 1]))
        if j is None:
            unmatched_cov += depth[k] > 0
        else:
            count[j] += 1; covered[j] += depth[k] > 0
            mind[j] = depth[k] if mind[j] is None else min(mind[j], depth[k])
    mind = [-1 if v is None else v for v in mind]
    best, at, k = 0, -1, 0
    while k < steps:                                    # the longest stretch of zeros, the smallest start on ties
        if depth[k]:
            k += 1
            continue
        q = k
        while q < steps and depth[q] == 0:
            q += 1
        if q - k > best:
            best, at = q - k, k
        k = q
    s = dict(status=status, steps=steps, steps_covered=sum(d > 0 for d in depth), max_depth=max(depth, default=0),
             first_uncovered=next((k for k, d in enumerate(depth) if d == 0), -1), longest_uncovered=best, longest_uncovered_at=at, juncs=m,
             juncs_used=sum(c > 0 for c in count), juncs_covered=sum(c > 0 and v == c for c, v in zip(count, covered)),
             juncs_uncovered=sum(c > 0 and v == 0 for c, v in zip(count, covered)), unmatched_covered=unmatched_cov, depth_sum=sum(depth))
    assert sum(covered) + unmatched_cov == s["steps_covered"]
    if floors is not None and steps > 0:
        floors["uncovered"] += s["steps_covered"] < steps; floors["all_covered"] += s["steps_covered"] == steps
        floors["depth3"] += s["max_depth"] >= 3
        floors["partly"] += any(0 < v < c for c, v in zip(count, covered)); floors["fully_multi"] += any(v == c > 1 for c, v in zip(count, covered))
        floors["used_uncovered"] += s["juncs_uncovered"] > 0
        floors["step0_cov"] += depth[0] > 0; floors["step0_unc"] += depth[0] == 0
        floors["last_cov"] += depth[-1] > 0; floors["last_unc"] += depth[-1] == 0
    return depth, count, covered, mind, s


def compare_unit(b, u, frags, ends, path, status, tag, gidx=None, floors=None):
    depth, count, covered, mind, summary = walk(path, frags, ends, status, floors)
    got = b.unit_evidence_juncs(u)
    assert got[0].tolist() == count, (tag, "count", got[0].tolist(), count)
    assert got[1].tolist() == covered, (tag, "covered", got[1].tolist(), covered)
    assert got[2].tolist() == mind, (tag, "min_depth", got[2].tolist(), mind)
    assert got[3].tolist() == (list(range(len(ends))) if gidx is None else list(gidx)), (tag, "graph_index", got[3].tolist())
    s = b.unit_evidence_profile(u)
    assert list(s) == list(FIELDS) and s == summary, (tag, s, summary)
    n = len(depth)
    half = n // 2                                       # the depth getter, in two halves
    assert b.unit_evidence_depth(u, 0, half).tolist() + b.unit_evidence_depth(u, half, n - half).tolist() == depth, (tag, "depth")
    return summary


def unit_ends(lh, g, oc):
    idx, ends, _ = jc.unit_junctions(lh, g, oc["start"], oc["end"])
    return idx, ends


class _Env:
    """AMBI_FPROFILE_FRAG_WINDOW / AMBI_JPROFILE_JUNC_WINDOW / AMBI_JPROFILE_SEG_WINDOW for the calls inside."""
    def __init__(self, fwin=None, jwin=None, swin=None):
        self.f, self.j = fc._Env(fwin), jc._Env(jwin, swin)

    def __enter__(self):
        self.f.__enter__(); self.j.__enter__()

    def __exit__(self, *exc):
        self.j.__exit__(*exc); self.f.__exit__(*exc)


# ---- case 1: the README example, as literals ---------------------------------------------------------------------------
README_DEPTH = [0, 0, 1, 1, 1, 4, 3, 3, 3, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 3, 3, 3, 4, 1, 1, 1, 0, 0]


def check_readme(lib, oracle):
    lh, sol, juncs = (os.path.join(cases.DATA, "readme6." + x) for x in ("lh", "sol", "juncs"))
    oc = oracle.run_bfb(lh, [sol])["chr"][0]
    path = jc.oracle_path(oc, 1)
    assert len(path) == 32 and walk_depth(path, fc.README_JUNCS) == README_DEPTH        # by the Python walk first ...
    g = api.Graph(lib, lh)
    g.read_fragments(juncs)
    idx, ends = unit_ends(lh, g, oc)
    b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    b.upload(); b.run(0); b.download()               # one unit: the express path
    for which in (0, 1):
        b.evidence_profile(which); b.evidence_profile_wait()
        assert b.unit_evidence_depth(0).tolist() == README_DEPTH                         # ... then as literals
        s = b.unit_evidence_profile(0)
        assert (s["status"], s["steps"], s["steps_covered"], s["max_depth"], s["depth_sum"], s["first_uncovered"], s["longest_uncovered"],
                s["longest_uncovered_at"]) == (0, 31, 18, 4, 40, 0, 9, 11), s
        compare_unit(b, 0, fc.README_JUNCS, ends, jc.oracle_path(oc, which), 0, ("readme", which), idx)
    orev = oracle.run_bfb(lh, [sol], reversed_=True)["chr"][0]
    b.run(api.FLAG_REVERSED); b.download()
    assert b.unit_path(0, 1).tolist() == orev["path_indel"]
    for which in (0, 1):
        b.evidence_profile(which); b.evidence_profile_wait()
        compare_unit(b, 0, fc.README_JUNCS, ends, jc.oracle_path(orev, which), jc.oracle_status(orev), ("readme reversed", which), idx)
    b.close(); g.close()


# ---- cases 2 - 5: the 40 units of profile_checks.many_units with read-like fragments ---------------------------------------
_REV = {}


def many_items(lib, oracle, workdir, n=40, first=0):
    """(graphs, batch, [(fragments, junction indices, junction ends, forward record, reversed record, lh)]): every unit gets the first
    12 fragments of frag_profile_checks.make_fragments -- the read-like ones, without the whole-path lines that cover everything."""
    items = pc.many_units(oracle, workdir)[first:first + n]
    key = (workdir, first, n)
    if key not in _REV:
        _REV[key] = [oracle.run_bfb(lh, [sol], reversed_=True)["chr"][0] for lh, sol, _ in items]
    graphs, b, out = [], api.Batch(lib), []
    for u, ((lh, sol, oc), orev) in enumerate(zip(items, _REV[key])):
        frags = fc.make_fragments(jc.oracle_path(oc, 1), 9000 + first + u)[:12]
        g = api.Graph(lib, lh); graphs.append(g)
        g.set_fragments(frags)
        b.add_chromosome_sol(g, 0, sol)
        idx, ends = unit_ends(lh, g, oc)
        out.append((frags, idx, ends, oc, orev, lh))
    return graphs, b, out


def check_batch(b, items, tag, reversed_=False, whichs=(0, 1), floors=None):
    for which in whichs:
        b.evidence_profile(which); b.evidence_profile_wait()
        for u, (frags, idx, ends, oc, orev, _) in enumerate(items):
            o = orev if reversed_ else oc
            compare_unit(b, u, frags, ends, jc.oracle_path(o, which), jc.oracle_status(o), (tag, which, u), idx, floors if which == 1 else None)


def check_many_units(lib, oracle, workdir, fwin=None, jwin=None, swin=None):
    with _Env(fwin, jwin, swin):
        graphs, b, items = many_items(lib, oracle, workdir)
        b.upload(); b.run(0); b.download()
        for u, it in enumerate(items):                 # precondition: the engine's paths are the oracle's
            assert b.unit_path(u, 0).tolist() == it[3]["path"] and b.unit_path(u, 1).tolist() == it[3]["path_indel"], u
        floors = dict.fromkeys(FLOORS, 0)
        check_batch(b, items, ("many", fwin, jwin, swin), floors=floors)
        assert all(floors[k] >= 1 for k in FLOORS), floors       # what the corpus must offer for the comparison to mean something
        # reversed on the same batch: other and often shorter paths, so stale cells and a stale depth area lie behind P
        b.run(api.FLAG_REVERSED); b.download()
        for u, it in enumerate(items):
            assert b.unit_path(u, 1).tolist() == it[4]["path_indel"], u
        assert sum(it[4]["path_indel"] != it[3]["path_indel"] for it in items) >= 1, "the reversed run must change some path"
        check_batch(b, items, ("many reversed", fwin, jwin, swin), reversed_=True)
        pc.close_all(graphs, b)


def _snapshot(b, U):
    return [(b.unit_evidence_profile(u), [a.tolist() for a in b.unit_evidence_juncs(u)], b.unit_evidence_depth(u).tolist()) for u in range(U)]


def check_repeated_requests(lib, oracle, workdir):
    """Case 4: the same request twice in a row, and which = 0 then 1, on one run: a depth area that is not zeroed doubles the second."""
    graphs, b, items = many_items(lib, oracle, workdir, 10)
    b.upload(); b.run(0); b.download()
    b.evidence_profile(1); b.evidence_profile_wait()
    one = _snapshot(b, len(items))
    b.evidence_profile(1); b.evidence_profile_wait()
    assert _snapshot(b, len(items)) == one
    assert any(s["depth_sum"] > 0 for s, _, _ in one)
    b.evidence_profile(0); b.evidence_profile_wait()
    zero = _snapshot(b, len(items))
    b.evidence_profile(1); b.evidence_profile_wait()
    assert _snapshot(b, len(items)) == one
    for u, (frags, idx, ends, oc, _, _) in enumerate(items):
        compare_unit(b, u, frags, ends, jc.oracle_path(oc, 1), jc.oracle_status(oc), ("again", u), idx)
        assert zero[u][2] == walk_depth(jc.oracle_path(oc, 0), frags), u
    pc.close_all(graphs, b)


def check_identities(lib, oracle, workdir):
    """Case 5: against the junction and the fragment profile of the same run."""
    graphs, b, items = many_items(lib, oracle, workdir, 12)
    b.upload(); b.run(0)
    for which in (0, 1):
        b.evidence_profile(which); b.junc_profile(which); b.frag_profile(which)
        b.frag_profile_wait(); b.junc_profile_wait(); b.evidence_profile_wait()
        b.download()
        for u, (frags, idx, ends, oc, _, _) in enumerate(items):
            count, covered, _, _ = b.unit_evidence_juncs(u)
            s = b.unit_evidence_profile(u)
            assert count.tolist() == b.unit_junc_usage(u)[0].tolist(), u
            fwd, rev, _, _ = b.unit_frag_support(u)
            assert s["depth_sum"] == sum((int(a) + int(r)) * (len(f) - 1) for a, r, f in zip(fwd, rev, frags)), u
            assert int(covered.sum()) + s["unmatched_covered"] == s["steps_covered"], u
            n = s["steps"]
            depth = walk_depth(jc.oracle_path(oc, which), frags)
            assert b.unit_evidence_depth(u, 0, n // 2).tolist() + b.unit_evidence_depth(u, n // 2, n - n // 2).tolist() == depth, u
    pc.close_all(graphs, b)


# ---- case 6: edge units -----------------------------------------------------------------------------------------------
def check_edge_units(lib, oracle, workdir):
    readme, rsol, juncs = (os.path.join(cases.DATA, "readme6." + x) for x in ("lh", "sol", "juncs"))
    # (1) F = 0 beside a unit with fragments, and a unit whose .sol selects nothing (status -11) with fragments
    sol0 = os.path.join(workdir, "ep_empty.sol")
    with open(sol0, "w") as f:
        f.write("Optimal - objective value 0.00000000\n")
    oc = oracle.run_bfb(readme, [rsol])["chr"][0]
    g1 = api.Graph(lib, readme); g1.read_fragments(juncs)
    g0 = api.Graph(lib, readme)
    idx, ends = unit_ends(readme, g0, oc)
    b = api.Batch(lib)
    b.add_chromosome_sol(g0, 0, rsol); b.add_chromosome_sol(g1, 0, rsol); b.add_chromosome_sol(g1, 0, sol0); b.add_chromosome_sol(g0, 0, rsol)
    b.upload(); b.run(0); b.download()
    assert b.unit_result(2)["status"] == -11
    for which in (0, 1):
        b.evidence_profile(which); b.evidence_profile_wait()
        for u in (0, 3):
            s = compare_unit(b, u, [], ends, jc.oracle_path(oc, which), 0, ("F = 0", which, u), idx)
            assert (s["steps"], s["steps_covered"], s["max_depth"], s["first_uncovered"], s["longest_uncovered"], s["longest_uncovered_at"],
                    s["juncs_covered"], s["depth_sum"]) == (31, 0, 0, 0, 31, 0, 0, 0), s
            assert b.unit_evidence_juncs(u)[1].tolist() == [0] * 4
        compare_unit(b, 1, fc.README_JUNCS, ends, jc.oracle_path(oc, which), 0, ("beside F = 0", which), idx)
        got = b.unit_evidence_juncs(2)
        assert [a.tolist() for a in got] == [[0] * 4, [0] * 4, [-1] * 4, list(idx)]
        assert b.unit_evidence_profile(2) == dict(ZERO, status=-11, juncs=4)
        assert b.unit_evidence_depth(2).tolist() == []
        with _raises(-33):
            b.unit_evidence_depth(2, 0, 1)
    b.close(); g0.close(); g1.close()
    # (2) no fold-back inversion: the shortcut path 1+2+3+4+; a fragment with L == P and one that would need a cell behind P
    lh = os.path.join(workdir, "ep_nofbi.lh")
    with open(lh, "w") as f:
        f.write(pc.NOFBI + "JUNC H:3:+ H:4:+ 30.0 1.0 U B\n")
    frags = [[1, 2], [2, 3, 4], [-4, -3], [4, -4], [1, 2, 3, 4, 1], [1, 2, 3, 4], [-4, -3, -2, -1], [2, 4], [3, 4, 1]]
    g = api.Graph(lib, lh); g.set_fragments(frags); b = api.Batch(lib)
    b.add_chromosome(g, 0, [], [])
    b.upload(); b.run(0); b.download()
    assert b.unit_result(0)["status"] == api.ST_SHORTCUT
    o = oracle.run_bfb(lh, [])["chr"][0]
    idx, ends = unit_ends(lh, g, o)
    for which in (0, 1):
        b.evidence_profile(which); b.evidence_profile_wait()
        s = compare_unit(b, 0, frags, ends, jc.oracle_path(o, which), api.ST_SHORTCUT, ("shortcut", which), idx)
    assert b.unit_evidence_depth(0).tolist() == [3, 3, 4] and (s["steps"], s["steps_covered"], s["first_uncovered"], s["depth_sum"]) == (3, 3, -1, 10), s
    b.close(); g.close()
    # (3) Infeasible .sol: the reference path over the six segments of the README example
    sol = os.path.join(workdir, "ep_infeasible.sol")
    with open(sol, "w") as f:
        f.write("Infeasible - objective value 0.00000000\n")
    frags = fc.README_JUNCS + [[1, 2, 3], [-6, -5], [6, -6]]
    g = api.Graph(lib, readme); g.set_fragments(frags); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    b.upload(); b.run(0); b.download()
    assert b.unit_result(0)["status"] == api.ST_INFEASIBLE
    o = oracle.run_bfb(readme, [sol])["chr"][0]
    idx, ends = unit_ends(readme, g, o)
    for which in (0, 1):
        b.evidence_profile(which); b.evidence_profile_wait()
        s = compare_unit(b, 0, frags, ends, jc.oracle_path(o, which), api.ST_INFEASIBLE, ("infeasible", which), idx)
    assert b.unit_evidence_depth(0).tolist() == [1, 1, 0, 0, 1] and (s["longest_uncovered"], s["longest_uncovered_at"]) == (2, 2), s
    b.close(); g.close()
    # (4) raw units without elements: P = 1 (no step) and P = 2 (one step; a fragment with L == P, one longer than the path)
    b = api.Batch(lib)
    u1 = b.add_unit(1, 0, [1.0], [], [], [], [], [], [], [], [], [])
    u2 = b.add_unit(2, 0, [1.0, 1.0], [1], [2], [1], [1], [1.0], [], [], [], [])
    b.upload(); b.run(0); b.download()
    assert b.unit_path(u1, 1).tolist() == [1] and b.unit_path(u2, 1).tolist() == [1, 2]
    b.set_unit_fragments(u1, [[1, 1], [1, -1]])
    b.set_unit_fragments(u2, [[1, 2], [-2, -1], [1, 2, 1], [2, -2]])
    for which in (0, 1):
        b.evidence_profile(which); b.evidence_profile_wait()
        s = compare_unit(b, u1, [[1, 1], [1, -1]], [], [1], b.unit_result(u1)["status"], ("P = 1", which))
        assert s == dict(ZERO, status=b.unit_result(u1)["status"]) and b.unit_evidence_depth(u1).tolist() == [] and b.unit_evidence_juncs(u1)[0].tolist() == []
        s = compare_unit(b, u2, [[1, 2], [-2, -1], [1, 2, 1], [2, -2]], [(1, 2)], [1, 2], b.unit_result(u2)["status"], ("P = 2", which))
        assert b.unit_evidence_depth(u2).tolist() == [2] and [a.tolist() for a in b.unit_evidence_juncs(u2)[:3]] == [[1], [1], [2]]
        assert (s["steps"], s["juncs_covered"], s["first_uncovered"], s["longest_uncovered_at"]) == (1, 1, -1, -1), s
    b.close()


# ---- case 7: one long path ----------------------------------------------------------------------------------------------
def gapped_fragments(path):
    """Two-cell fragments (one per distinct step, so each covers exactly the steps equal to it) over every step but three uncovered
    stretches of equal length: one across the sweep edge at step 2048, a second later, the third ending at the last step.  A step
    inside a stretch stays uncovered only when no kept step equals it or its reverse complement; the stretches' steps are removed
    from the kept set wherever they occur, so further gaps open elsewhere -- the walk decides what the answer is."""
    P = len(path)
    steps = [(path[k], path[k + 1]) for k in range(P - 1)]
    G = 6
    gaps = [range(2048 - G // 2, 2048 + G // 2), range(5000, 5000 + G), range(P - 1 - G, P - 1)]
    drop = set()
    for r in gaps:
        for k in r:
            drop.add(steps[k]); drop.add((-steps[k][1], -steps[k][0]))
    keep, seen = [], set()
    for st in steps:
        canon = min(st, (-st[1], -st[0]))
        if st in drop or canon in seen:
            continue
        seen.add(canon); keep.append(list(st))
    return keep, gaps


def check_bench_unit(lib, oracle, workdir):
    s = synth.make_sample(256, 512, "wide", 19, seed=2100, n_del=1, n_dup=1, name="epbig")
    lh, sols = s.write(workdir)
    big = oracle.run_bfb(lh, sols)["chr"][0]
    path = jc.oracle_path(big, 1)
    assert len(path) > 8192                         # several sweeps of 256 threads x 8 cells
    edge = fc.edge_fragments(path, 3)
    graphs, b, small = many_items(lib, oracle, workdir, 3)
    g = api.Graph(lib, lh); g.set_fragments(edge)
    u = b.add_chromosome_sol(g, 0, sols[0])
    assert u == 3
    idx, ends = unit_ends(lh, g, big)
    b.upload(); b.run(0); b.download()
    assert b.unit_path(3, 1).tolist() == big["path_indel"]
    for which in (0, 1):
        b.evidence_profile(which); b.evidence_profile_wait()
        for k, (fr, i2, e2, oc, _, _) in enumerate(small):
            compare_unit(b, k, fr, e2, jc.oracle_path(oc, which), jc.oracle_status(oc), ("beside bench", which, k), i2)
        s1 = compare_unit(b, 3, edge, ends, jc.oracle_path(big, which), 0, ("bench", which), idx)
    depth = walk_depth(path, edge)
    assert depth[-1] > 0 and depth[2047] > 0 and depth[7] > 0 and s1["steps_covered"] < s1["steps"]      # chunk edge, sweep edge, last step
    pc.close_all(graphs + [g], b)
    # hand-placed gaps: the same unit alone, as a raw request of its final path
    keep, gaps = gapped_fragments(path)
    g = api.Graph(lib, lh); g.set_fragments(keep)
    b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sols[0])
    b.upload(); b.run(0); b.download()
    b.evidence_profile(1); b.evidence_profile_wait()
    s2 = compare_unit(b, 0, keep, ends, path, 0, "bench, gaps", idx)
    depth = walk_depth(path, keep)
    zero = lambda r: all(depth[k] == 0 for k in r)
    assert all(zero(r) for r in gaps)
    runs, k = [], 0
    while k < len(depth):
        q = k
        while q < len(depth) and (depth[q] == 0) == (depth[k] == 0):
            q += 1
        if depth[k] == 0:
            runs.append((k, q - k))
        k = q
    top = max(n for _, n in runs)
    tied = [k for k, n in runs if n == top]
    # a stretch across the sweep edge, the longest one at least twice (the smaller start wins), a longest stretch at the last step
    assert any(k < 2048 < k + n for k, n in runs), runs[:5]
    assert len(tied) >= 2 and tied[-1] + top == len(depth) and s2["longest_uncovered_at"] == tied[0] and s2["longest_uncovered"] == top, (tied, top, s2)
    b.close(); g.close()


# ---- case 8: the big unit finished at wait() ----------------------------------------------------------------------------
def check_big_unit_finished_at_wait(lib, oracle, workdir):
    lh, sol, R, rev = pc.big_unit(oracle, workdir)
    path = jc.oracle_path(rev, 1)
    frags = fc.edge_fragments(path, 5)
    g = api.Graph(lib, lh); g.set_fragments(frags)
    idx, ends = unit_ends(lh, g, rev)
    b = api.Batch(lib)
    b.configure(first_budget=4)
    b.add_chromosome_sol(g, 0, sol)
    graphs, items = [g], []
    for u, (l2, s2, oc) in enumerate(pc.many_units(oracle, workdir)[:7]):
        fr = fc.make_fragments(jc.oracle_path(oc, 1), 9000 + u)[:12]
        g2 = api.Graph(lib, l2); graphs.append(g2)
        g2.set_fragments(fr)
        b.add_chromosome_sol(g2, 0, s2)
        items.append((fr, unit_ends(l2, g2, oc), oc))
    b.debug_inject_validity(0, [0] * R + [1] * R)
    b.upload()
    for which in (1, 0):
        b.run(0)
        b.evidence_profile(which)        # queued behind a run whose unit 0 is still PENDING
        b.wait()                         # the parallel search finishes it
        b.evidence_profile_wait()        # ... and the profile is that of the final results
        b.download()
        r = b.unit_result(0)
        assert (r["status"], r["first_valid"], r["first_forward"]) == (0, 0, 0), r
        assert b.unit_path(0, 0).tolist() == rev["path"] and b.unit_path(0, 1).tolist() == rev["path_indel"]     # precondition
        s = compare_unit(b, 0, frags, ends, jc.oracle_path(rev, which), 0, ("big", which), idx)
        for u, (fr, (i2, e2), oc) in enumerate(items):
            compare_unit(b, u + 1, fr, e2, jc.oracle_path(oc, which), jc.oracle_status(oc), ("beside big", which, u), i2)
    assert s["steps"] + 1 == len(rev["path"]) > 2048 * 4 and s["steps_covered"] > 0
    pc.close_all(graphs, b)


# ---- case 9: the queueing path's branches -----------------------------------------------------------------------------
def check_request_paths(lib, oracle, workdir, run_stream=None, req_stream=None):
    graphs, b, items = many_items(lib, oracle, workdir, 12)
    files = pc.many_units(oracle, workdir)[:12]
    b.upload()

    def compare(which, tag):
        for u, (frags, idx, ends, oc, _, _) in enumerate(items):
            compare_unit(b, u, frags, ends, jc.oracle_path(oc, which), jc.oracle_status(oc), (tag, which, u), idx)
    # (1) run on one stream, request on another, nothing waited for in between
    for which in (0, 1):
        b.run(0, run_stream)
        b.evidence_profile(which, req_stream); b.evidence_profile_wait()
        b.download()
        compare(which, "other stream")
    # (2) a request nobody waited for, then another: the second one answers
    b.run(0, run_stream)
    b.evidence_profile(0, req_stream); b.evidence_profile(1, req_stream); b.evidence_profile_wait()
    b.download()
    compare(1, "unwaited")
    # (3) beside the three other kinds on one run: all four stay correct
    b.run(0, run_stream)
    b.junc_profile(1, req_stream); b.evidence_profile(1, req_stream); b.frag_profile(1, req_stream); b.profile(1, req_stream)
    b.profile_wait(); b.frag_profile_wait(); b.evidence_profile_wait(); b.junc_profile_wait()
    b.download()
    compare(1, "beside three profiles")
    for u, ((lh, _, oc), g) in enumerate(zip(files, graphs)):
        idx, count, summary, _ = jc.unit_expectation(lh, g, oc, 1)
        jc.compare_unit(b, u, idx, count, summary, ("junction beside", u))
        n, want = pc.unit_expectation(b, u, oc, 1)
        pc.compare_unit(b, u, n, want, ("cn beside", u))
        fc.compare_unit(b, u, items[u][0], jc.oracle_path(oc, 1), jc.oracle_status(oc), ("fragment beside", u))
    # (4) closed with a request in flight; the next batch (other units, other offsets) gets the lease back
    b.run(0, run_stream)
    b.evidence_profile(1, req_stream)
    pc.close_all(graphs, b)
    graphs, b, items = many_items(lib, oracle, workdir, 5, first=12)
    b.upload(); b.run(0, run_stream); b.download()
    check_batch(b, items, "after a close in flight")
    pc.close_all(graphs, b)


# ---- case 9b: the fragment and the evidence request on two streams ------------------------------------------------------------
QUIRKS2_UNITS = [(1, 4), (5, 8), (9, 10)]                 # SOURCE / SINK of tests/data/quirks2.lh


def file_fragments(lib, lh, juncs, start, end):
    """The lines of a .juncs file that lie inside [start, end], as chains of LOCAL signed ids."""
    g = api.Graph(lib, lh); g.read_fragments(juncs)
    lines, _ = g.fragments()
    g.close()
    return [jc.local_path(f, start - 1) for f in lines if len(f) >= 2 and all(start <= abs(v) <= end for v in f)]


def check_two_request_streams(lib, oracle, run_stream=None, frag_stream=None, ev_stream=None):
    """Both readers of the fragment image, each on a stream of its own and with nothing between them: the image goes up with the first
    of the two requests, on ITS stream; then a moved version with the requests the other way round.  This checks the request logic --
    who uploads, the layouts redone behind a new version, both kinds' results -- not the ordering behind the upload itself: an image
    this small arrives before the other stream's kernel starts whether or not that stream waits for it.  The batch is the fixtures
    that have a .juncs file: the README example (the oracle's path, the independent reference here) and the three chromosomes of quirks2
    without a .sol (two refused units and a two-cell shortcut: the engine's own status and path, as for hand-built units -- they add
    empty results and F = 0 to the batch, no second reference).  The fragments are attached after the run."""
    readme, rsol, rjuncs = (os.path.join(cases.DATA, "readme6." + x) for x in ("lh", "sol", "juncs"))
    q2, q2juncs = os.path.join(cases.DATA, "quirks2.lh"), os.path.join(cases.DATA, "quirks2.juncs")
    oc = oracle.run_bfb(readme, [rsol])["chr"][0]
    g1, g2 = api.Graph(lib, readme), api.Graph(lib, q2)
    b = api.Batch(lib)
    b.add_chromosome_sol(g1, 0, rsol)
    for c in range(len(QUIRKS2_UNITS)):
        b.add_chromosome(g2, c, [], [])
    ranges = [(oc["start"], oc["end"])] + QUIRKS2_UNITS
    frags = [file_fragments(lib, readme, rjuncs, *ranges[0])] + [file_fragments(lib, q2, q2juncs, s, e) for s, e in QUIRKS2_UNITS]
    assert frags[0] == fc.README_JUNCS and [len(f) for f in frags[1:]] == [2, 2, 0], frags
    juncs = [unit_ends(readme, g1, oc)] + [jc.unit_junctions(q2, g2, s, e)[:2] for s, e in QUIRKS2_UNITS]
    b.upload(); b.run(0, run_stream)

    def requests(order, tag):
        for which in (0, 1):
            for kind in order:
                if kind == "fragment":
                    b.frag_profile(which, frag_stream)
                else:
                    b.evidence_profile(which, ev_stream)
            b.frag_profile_wait(); b.evidence_profile_wait()
            b.download()
            for u, (idx, ends) in enumerate(juncs):
                status = b.unit_result(u)["status"]
                path = jc.oracle_path(oc, which) if u == 0 else b.unit_path(u, which).tolist()
                if u > 0 and path:
                    path = jc.local_path(path, ranges[u][0] - 1)
                assert status == (0 if u == 0 else (-11, -11, api.ST_SHORTCUT)[u - 1]), (tag, u, status)
                fc.compare_unit(b, u, frags[u], path, status, (tag, "fragment", which, u))
                compare_unit(b, u, frags[u], ends, path, status, (tag, "evidence", which, u), idx)

    for u, f in enumerate(frags):
        b.set_unit_fragments(u, f)
    requests(("fragment", "evidence"), "image with the fragment request")
    assert b.unit_evidence_depth(0).tolist() == README_DEPTH and b.unit_evidence_depth(3).tolist() == [0]
    # another set for one unit while both kinds have been queued: the version moves, and the evidence request carries the image up
    frags[0] = fc.README_JUNCS + [[1, 2, 3], [-6, -5], [6, -6]]
    b.set_unit_fragments(0, frags[0])
    requests(("evidence", "fragment"), "image with the evidence request")
    assert b.unit_evidence_depth(0).tolist() != README_DEPTH
    b.close(); g1.close(); g2.close()


# ---- case 10: sharded ---------------------------------------------------------------------------------------------------
def check_sharded(lib, oracle, workdir, devices):
    graphs, b, items = many_items(lib, oracle, workdir, 12)
    b.run_sharded(0, devices=devices)
    check_batch(b, items, ("sharded", tuple(devices)))
    with _raises(-32):
        b.evidence_profile_device()      # one block per share: no single device view
    with _raises(-32):
        b.evidence_depth_device()
    pc.close_all(graphs, b)


# ---- case 12: the CLI -----------------------------------------------------------------------------------------------------
def check_cli(lib, exe, cwd, oracle, workdir):
    import test_cli_dropin as t
    readme, rsol = os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol")
    lh2, sol2, oc2 = pc.many_units(oracle, workdir)[1]
    frags = fc.README_JUNCS + [[3], [3, -3], [2, 3, 4], [-4, -3, -2]] + [list(jc.oracle_path(oc2, 1)[:4])]
    frags = [f for f in frags if all(abs(v) <= 6 for v in f)]
    ffile = os.path.join(cwd, "frags.juncs")
    with open(ffile, "w") as f:
        for line in frags:
            f.write(" ".join("%d%s" % (abs(v), "+" if v > 0 else "-") for v in line) + "\n")
    outs = []
    for k, extra in enumerate(([], ["--evidence_profile", "ev.tsv", "--evidence_depth", "depth.tsv", "--frags", ffile])):
        sub = os.path.join(cwd, "run%d" % k)
        os.makedirs(sub)
        bindir = os.path.join(sub, "bin")
        t.fake_cbc(bindir, [rsol, sol2])
        r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", readme + "," + lh2, "--lp_prefix", "two", *extra)
        assert r.returncode == 0, r.stderr
        outs.append((r.stdout, r.stderr, open(os.path.join(sub, "simulation_sv.txt"), "rb").read(), sorted(x for x in os.listdir(sub) if x != "bin")))
    assert outs[0][:3] == outs[1][:3]                                      # stdout, stderr, side file: unchanged by the options
    assert outs[1][3] == sorted(outs[0][3] + ["ev.tsv", "depth.tsv"])
    want_j, want_d = [], []
    real = [f for f in frags if len(f) >= 2]
    for lh, sol in ((readme, rsol), (lh2, sol2)):
        oc = oracle.run_bfb(lh, [sol])["chr"][0]
        g = api.Graph(lib, lh)
        idx, ends = unit_ends(lh, g, oc)
        m = len(g.junctions()["src"])
        g.close()
        depth, count, covered, mind, _ = walk(jc.oracle_path(oc, 1), real, ends, jc.oracle_status(oc))
        rows = {j: (0, count[k], covered[k], mind[k]) for k, j in enumerate(idx)}
        for j in range(m):
            want_j.append("\t".join([lh] + [str(v) for v in (rows.get(j, (-1, 0, 0, -1))[0], j) + rows.get(j, (-1, 0, 0, -1))[1:]]))
        k = 0
        while k < len(depth):
            q = k
            while q < len(depth) and depth[q] == depth[k]:
                q += 1
            want_d.append("\t".join([lh, "0", str(k), str(q - k), str(depth[k])]))
            k = q
    got_j = open(os.path.join(cwd, "run1", "ev.tsv")).read().splitlines()
    got_d = open(os.path.join(cwd, "run1", "depth.tsv")).read().splitlines()
    assert got_j == want_j and got_d == want_d
    assert any(line.split("\t")[4] != "0" for line in got_j) and any(line.split("\t")[4] not in ("0", "1") for line in got_d)
    # --frags defaults to the file of --juncdb: against a run with --juncdb alone
    outs = []
    for k, extra in enumerate(([], ["--evidence_depth", "depth.tsv"])):
        sub = os.path.join(cwd, "jdb%d" % k)
        os.makedirs(sub)
        bindir = os.path.join(sub, "bin")
        t.fake_cbc(bindir, [rsol])
        r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", readme, "--lp_prefix", "one", "--juncdb", os.path.join(cases.DATA, "readme6.juncs"), *extra)
        assert r.returncode == 0, r.stderr
        outs.append((r.stdout, r.stderr, open(os.path.join(sub, "simulation_sv.txt"), "rb").read()))
    assert outs[0] == outs[1]
    got = [line.split("\t")[2:] for line in open(os.path.join(cwd, "jdb1", "depth.tsv")).read().splitlines()]
    flat = [int(d) for k, n, d in got for _ in range(int(n))]
    assert flat == README_DEPTH and [int(k) for k, _, _ in got] == [0, 2, 5, 6, 9, 11, 20, 22, 25, 26, 29], got
    # a PROP C2 sample: its printed paths are rebuilt on the host -- refused, exit status 2, no file
    for opt, name in (("--evidence_profile", "ev.tsv"), ("--evidence_depth", "depth.tsv")):
        sub = os.path.join(cwd, "c2" + name)
        os.makedirs(sub)
        bindir = os.path.join(sub, "bin")
        t.fake_cbc(bindir, [os.path.join(cases.DATA, "readme_c2_chr0.sol"), os.path.join(cases.DATA, "readme_c2_chr1.sol")])
        r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", os.path.join(cases.DATA, "readme_c2.lh"), "--lp_prefix", "c2", opt, name, "--frags", ffile)
        assert r.returncode == 2 and opt in r.stderr and "PROP I1 / C1 / I2 / C2" in r.stderr, (r.returncode, r.stderr)
        assert not os.path.exists(os.path.join(sub, name))
    r = t.run_cli(exe, sub, bindir, "--help")
    assert "--evidence_profile" in r.stdout and "--evidence_depth" in r.stdout


# ---- case 13: argument and state errors -------------------------------------------------------------------------------
def check_errors(lib):
    lh, sol, juncs = (os.path.join(cases.DATA, "readme6." + x) for x in ("lh", "sol", "juncs"))
    g = api.Graph(lib, lh); g.read_fragments(juncs); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    for call in (lambda: b.evidence_profile(1), b.evidence_profile_wait):
        with _raises(-32):                                 # AMBI_ERR_STATE: nothing uploaded
            call()
    b.upload()
    for call in (lambda: b.evidence_profile(1), b.evidence_profile_wait, lambda: b.unit_evidence_profile(0), lambda: b.unit_evidence_juncs(0),
                 lambda: b.unit_evidence_depth(0, 0, 1), b.evidence_profile_device, b.evidence_depth_device):
        with _raises(-32):                                 # uploaded, never run
            call()
    b.run(0); b.download()
    with _raises(-32):
        b.unit_evidence_profile(0)                         # run, not profiled
    with _raises(-32):
        b.evidence_profile_wait()                          # nothing queued
    for which in (2, -1):
        with _raises(-33):                                 # AMBI_ERR_ARG
            b.evidence_profile(which)
    b.frag_profile(1); b.frag_profile_wait()
    b.junc_profile(1); b.junc_profile_wait()
    with _raises(-32):
        b.unit_evidence_profile(0)                         # another kind's request does not answer for this one
    with _raises(-32):
        b.unit_evidence_depth(0, 0, 1)
    b.evidence_profile(1); b.evidence_profile_wait()
    buf = [(ctypes.c_int32 * 8)() for _ in range(4)]
    assert lib.ambi_batch_unit_evidence_juncs(b.h, 0, *buf, 3) == -33      # cap < m
    assert lib.ambi_batch_unit_evidence_juncs(b.h, 0, buf[0], None, None, None, 4) == 4 and list(buf[0][:4]) == [2, 1, 2, 0]
    assert lib.ambi_batch_unit_evidence_juncs(b.h, 0, None, buf[1], buf[2], buf[3], 4) == 4
    assert (list(buf[1][:4]), list(buf[2][:4]), list(buf[3][:4])) == ([2, 0, 0, 0], [2, 0, 0, -1], [0, 1, 2, 3])
    for u in (1, -1):
        with _raises(-33):
            b.unit_evidence_profile(u)                     # no such unit
        assert lib.ambi_batch_unit_evidence_juncs(b.h, u, *buf, 8) == -33
        with _raises(-33):
            b.unit_evidence_depth(u, 0, 1)
    out = (ctypes.c_int32 * 40)()
    for first, n in ((-1, 1), (0, 32), (31, 1), (32, 0), (0, -1), (30, 2)):        # outside [0, P - 1] = [0, 31]
        assert lib.ambi_batch_unit_evidence_depth(b.h, 0, first, n, out) == -33, (first, n)
    assert lib.ambi_batch_unit_evidence_depth(b.h, 0, 0, 1, None) == -33
    assert lib.ambi_batch_unit_evidence_depth(b.h, 0, 31, 0, None) == 0 and lib.ambi_batch_unit_evidence_depth(b.h, 0, 30, 1, out) == 0 and out[0] == 0
    assert lib.ambi_batch_unit_evidence_depth(b.h, 0, 0, 31, out) == 0 and list(out[:31]) == README_DEPTH
    off = (ctypes.c_int64 * 1)()
    assert lib.ambi_batch_evidence_depth_device(b.h, None, None, off, 0) == -33     # cap < n_units
    b.set_unit_fragments(0, [[1, 2]])
    with _raises(-32):
        b.unit_evidence_profile(0)                         # the fragments changed: the old profile is gone
    b.evidence_profile(1); b.evidence_profile_wait()
    assert b.unit_evidence_profile(0)["depth_sum"] == 2
    b.run(0)
    with _raises(-32):
        b.unit_evidence_profile(0)                         # a new run: the old profile is gone
    b.wait()
    b.close(); g.close()
