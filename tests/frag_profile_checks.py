"""Checks of the fragment support profile (ambi_batch_frag_profile, csrc/ambi_frag_profile.hpp) shared by the CPU host-simulation
tests and the GPU tests (same assertions, different library).

Expected values never come from the stage under test: a plain Python walk -- a naive window compare written from the definitions
(fwd: occurrences of f, rev: occurrences of rc(f) unless rc(f) == f, first: smallest position of either) -- over the ORACLE's path
of the unit.  Hand-built raw units, which no file describes, use the engine's own unit_path (pinned by the parity tests)."""
import ctypes
import os
import random

import numpy as np

import cases
import junc_profile_checks as jc
import profile_checks as pc
from ambigram_amd import api, synth

FIELDS = ("status", "cells", "frags", "frags_supported", "first_unsupported", "max_count", "longest_supported", "reserved", "occurrences")
ZERO = dict.fromkeys(FIELDS, 0)
FLOORS = ("count0", "both", "two", "palindrome", "L==P", "L>P", "at0", "atend")


# ---- the plain walk ---------------------------------------------------------------------------------------------------
def rc(f):
    return [-v for v in reversed(f)]


def positions(path, f):
    L, P = len(f), len(path)
    return [i for i in range(0, P - L + 1) if path[i:i + L] == f]


def walk(path_local, frags, status=0, floors=None):
    """(fwd[F], rev[F], first[F], summary) of a path of LOCAL signed ids over the fragments (lists of local signed ids, L >= 2)."""
    F = len(frags)
    if status < 0 or len(path_local) == 0:
        return [0] * F, [0] * F, [-1] * F, dict(ZERO, status=status, frags=F)
    path = list(path_local)
    P = len(path)
    fwd, rev, first = [], [], []
    for f in frags:
        f = list(f)
        assert len(f) >= 2
        a = positions(path, f)
        b = positions(path, rc(f)) if rc(f) != f else []
        fwd.append(len(a)); rev.append(len(b)); first.append(min(a + b) if a or b else -1)
        if floors is not None:
            L = len(f)
            floors["count0"] += not (a or b); floors["both"] += bool(a and b); floors["two"] += len(a) + len(b) >= 2
            floors["palindrome"] += rc(f) == f; floors["L==P"] += L == P; floors["L>P"] += L > P
            floors["at0"] += 0 in a + b; floors["atend"] += (P - L) in a + b
    tot = [x + y for x, y in zip(fwd, rev)]
    s = dict(status=status, cells=P, frags=F, frags_supported=sum(t > 0 for t in tot),
             first_unsupported=next((i for i, t in enumerate(tot) if t == 0), -1), max_count=max(tot, default=0),
             longest_supported=max((len(f) for f, t in zip(frags, tot) if t > 0), default=0), reserved=0, occurrences=sum(tot))
    return fwd, rev, first, s


def make_fragments(path, seed, n_random=12):
    """The fragments of one unit, cut from its path (local ids): substrings at random positions with L = 2 .. min(40, P), half of them
    reverse-complemented, a quarter mutated in one cell; the whole path and its reverse complement; the path with one more cell;
    the first L and the last L cells; a fold-back pair (x, -x) of the path; two identical lines."""
    rng = random.Random(seed)
    P = len(path)
    out = []
    if P < 2:
        return [[1, 1], [1, -1]]
    top = min(40, P)
    for k in range(n_random):
        L = rng.randint(2, top)
        i = rng.randint(0, P - L)
        f = list(path[i:i + L])
        if k % 4 == 3:
            at = rng.randrange(L)
            f[at] = -f[at] if rng.random() < 0.5 else (abs(f[at]) % max(abs(v) for v in path) + 1) * (1 if f[at] > 0 else -1)
        if k % 2:
            f = rc(f)
        out.append(f)
    out.append(list(path)); out.append(rc(path))
    out.append(list(path) + [path[0]])
    L = rng.randint(2, top)
    out.append(list(path[:L])); out.append(list(path[P - L:]))
    turn = next((i for i in range(P - 1) if path[i + 1] == -path[i]), None)
    if turn is not None:
        out.append([path[turn], path[turn + 1]])
    out.append(list(out[0])); out.append(list(out[0]))
    return out


def to_abs(f, base):
    return [v + base if v > 0 else v - base for v in f]


def compare_unit(b, u, frags, path, status, tag, gidx=None, floors=None):
    fwd, rev, first, summary = walk(path, frags, status, floors)
    got = b.unit_frag_support(u)
    assert got[0].tolist() == fwd, (tag, "fwd", got[0].tolist(), fwd)
    assert got[1].tolist() == rev, (tag, "rev", got[1].tolist(), rev)
    assert got[2].tolist() == first, (tag, "first", got[2].tolist(), first)
    assert got[3].tolist() == (list(range(len(frags))) if gidx is None else list(gidx)), (tag, "graph_index", got[3].tolist())
    s = b.unit_frag_profile(u)
    assert list(s) == list(FIELDS) and s == summary, (tag, s, summary)
    return summary


class _Env:
    """AMBI_FPROFILE_FRAG_WINDOW for the calls inside."""
    def __init__(self, window=None):
        self.window = window

    def __enter__(self):
        self.saved = os.environ.pop("AMBI_FPROFILE_FRAG_WINDOW", None)
        if self.window:
            os.environ["AMBI_FPROFILE_FRAG_WINDOW"] = str(self.window)

    def __exit__(self, *exc):
        os.environ.pop("AMBI_FPROFILE_FRAG_WINDOW", None)
        if self.saved is not None:
            os.environ["AMBI_FPROFILE_FRAG_WINDOW"] = self.saved


# ---- case 1: the README example -------------------------------------------------------------------------------------
README_JUNCS = [[6, -6, -5, -4, -3, -2, 2], [-2, 2, 3, 4, 5, 6, -6], [6, -6, -5, -4, -3]]


def check_readme(lib, oracle):
    import json
    lh, sol, juncs = (os.path.join(cases.DATA, "readme6." + x) for x in ("lh", "sol", "juncs"))
    golden = json.load(open(os.path.join(os.path.dirname(cases.DATA), "golden", "known_answers.json")))
    fwd_path = parse_printed(golden["readme6"]["forward"][0])
    assert len(fwd_path) == 32
    oc = oracle.run_bfb(lh, [sol])["chr"][0]
    assert oc["path_indel"] == fwd_path
    # by the Python walk first ...
    assert walk(fwd_path, README_JUNCS)[:3] == ([1, 1, 2], [1, 1, 2], [5, 5, 2])
    g = api.Graph(lib, lh)
    g.read_fragments(juncs)
    assert g.fragments() == (README_JUNCS, [0, 0, 0])
    b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    b.upload(); b.run(0); b.download()               # one unit: the express path
    for which in (0, 1):
        b.frag_profile(which); b.frag_profile_wait()
        # ... then as literals.  1+2+3+4+5+6+|6-5-4-3-2-|2+3+4+|4-3-|3+4+|4-3-2-|2+3+4+5+6+|6-5-4-3-2-1-:
        #   line 1 (6+ 6- 5- 4- 3- 2- 2+) at 5; its reverse complement IS line 2 (2- 2+ 3+ 4+ 5+ 6+ 6-), at 20: each once in each direction;
        #   line 3 (6+ 6- 5- 4- 3-) at 5 and 25, its reverse complement (3+ 4+ 5+ 6+ 6-) at 2 and 22.
        fwd, rev, first, gidx = b.unit_frag_support(0)
        assert (fwd.tolist(), rev.tolist(), first.tolist(), gidx.tolist()) == ([1, 1, 2], [1, 1, 2], [5, 5, 2], [0, 1, 2])
        assert b.unit_frag_profile(0) == dict(status=0, cells=32, frags=3, frags_supported=3, first_unsupported=-1, max_count=4,
                                              longest_supported=7, reserved=0, occurrences=8)
    orev = oracle.run_bfb(lh, [sol], reversed_=True)["chr"][0]
    b.run(api.FLAG_REVERSED); b.download()
    assert b.unit_path(0, 1).tolist() == orev["path_indel"] == parse_printed(golden["readme6"]["reversed"][0])
    for which in (0, 1):
        b.frag_profile(which); b.frag_profile_wait()
        compare_unit(b, 0, README_JUNCS, jc.oracle_path(orev, which), jc.oracle_status(orev), ("readme reversed", which), [0, 1, 2])
    b.close(); g.close()


def parse_printed(text):
    """printBFB's form "1+2+|2-1-" as signed ids."""
    import re
    return [int(n) if sg == "+" else -int(n) for n, sg in re.findall(r"(\d+)([+-])", text)]


# ---- cases 2, 3: the 40 units of profile_checks.many_units, forward then reversed on the same batch -----------------------------
_REV = {}


def many_items(lib, oracle, workdir, n=40):
    """(graphs, batch, [(fragments, forward record, reversed record)]); every unit's fragments are cut from its forward final path."""
    items = pc.many_units(oracle, workdir)[:n]
    key = (workdir, n)
    if key not in _REV:
        _REV[key] = [oracle.run_bfb(lh, [sol], reversed_=True)["chr"][0] for lh, sol, _ in items]
    graphs, b, out = [], api.Batch(lib), []
    for u, ((lh, sol, oc), orev) in enumerate(zip(items, _REV[key])):
        assert oc["start"] == 1
        frags = make_fragments(jc.oracle_path(oc, 1), 9000 + u)
        g = api.Graph(lib, lh); graphs.append(g)
        g.set_fragments(frags)
        b.add_chromosome_sol(g, 0, sol)
        out.append((frags, oc, orev))
    return graphs, b, out


def check_batch(b, items, tag, reversed_=False, whichs=(0, 1), floors=None):
    for which in whichs:
        b.frag_profile(which); b.frag_profile_wait()
        for u, (frags, oc, orev) in enumerate(items):
            o = orev if reversed_ else oc
            compare_unit(b, u, frags, jc.oracle_path(o, which), jc.oracle_status(o), (tag, which, u), floors=floors)


def check_many_units(lib, oracle, workdir, window=None):
    with _Env(window):
        graphs, b, items = many_items(lib, oracle, workdir)
        b.upload(); b.run(0); b.download()
        for u, (_, oc, _) in enumerate(items):        # precondition: the engine's paths are the oracle's
            assert b.unit_path(u, 0).tolist() == oc["path"] and b.unit_path(u, 1).tolist() == oc["path_indel"], u
        floors = dict.fromkeys(FLOORS, 0)
        check_batch(b, items, ("many", window), floors=floors)
        assert all(floors[k] >= 1 for k in FLOORS), floors       # what the generator must reach for the comparison to mean something
        # reversed on the same batch: other and often shorter paths, so stale cells of the forward run lie behind P
        b.run(api.FLAG_REVERSED); b.download()
        shorter = 0
        for u, (_, oc, orev) in enumerate(items):
            assert b.unit_path(u, 1).tolist() == orev["path_indel"], u
            shorter += len(orev["path_indel"]) < len(oc["path_indel"]) or len(orev["path"]) < len(oc["path"])
        differ = sum(orev["path_indel"] != oc["path_indel"] for _, oc, orev in items)
        assert differ >= 1, "the reversed run must change some path"
        floors = dict.fromkeys(FLOORS, 0)
        check_batch(b, items, ("many reversed", window), reversed_=True, floors=floors)
        assert floors["count0"] >= 1 and floors["L>P"] + shorter >= 1, (floors, shorter)
        pc.close_all(graphs, b)


# ---- case 4: edge units -----------------------------------------------------------------------------------------------
def check_edge_units(lib, oracle, workdir):
    readme, rsol, juncs = (os.path.join(cases.DATA, "readme6." + x) for x in ("lh", "sol", "juncs"))
    # (1) F = 0 beside a unit with fragments, and a unit whose .sol selects nothing (status -11) with fragments
    sol0 = os.path.join(workdir, "fp_empty.sol")
    with open(sol0, "w") as f:
        f.write("Optimal - objective value 0.00000000\n")
    oc = oracle.run_bfb(readme, [rsol])["chr"][0]
    g1 = api.Graph(lib, readme); g1.read_fragments(juncs)
    g0 = api.Graph(lib, readme)
    b = api.Batch(lib)
    b.add_chromosome_sol(g0, 0, rsol); b.add_chromosome_sol(g1, 0, rsol); b.add_chromosome_sol(g1, 0, sol0); b.add_chromosome_sol(g0, 0, rsol)
    b.upload(); b.run(0); b.download()
    assert b.unit_result(2)["status"] == -11
    for which in (0, 1):
        b.frag_profile(which); b.frag_profile_wait()
        for u in (0, 3):
            s = compare_unit(b, u, [], jc.oracle_path(oc, which), 0, ("F = 0", which, u))
            assert s == dict(ZERO, cells=32, first_unsupported=-1)
        compare_unit(b, 1, README_JUNCS, jc.oracle_path(oc, which), 0, ("beside F = 0", which))
        got = b.unit_frag_support(2)
        assert [a.tolist() for a in got] == [[0] * 3, [0] * 3, [-1] * 3, [0, 1, 2]]
        assert b.unit_frag_profile(2) == dict(ZERO, status=-11, frags=3)
    b.close(); g0.close(); g1.close()
    # (2) no fold-back inversion: the shortcut path 1+2+3+4+
    lh = os.path.join(workdir, "fp_nofbi.lh")
    with open(lh, "w") as f:
        f.write(pc.NOFBI)
    frags = [[1, 2], [2, 3, 4], [-4, -3], [4, -4], [1, 2, 3, 4, 1], [1, 2, 3, 4], [-4, -3, -2, -1], [2, 4]]
    g = api.Graph(lib, lh); g.set_fragments(frags); b = api.Batch(lib)
    b.add_chromosome(g, 0, [], [])
    b.upload(); b.run(0); b.download()
    assert b.unit_result(0)["status"] == api.ST_SHORTCUT
    o = oracle.run_bfb(lh, [])["chr"][0]
    for which in (0, 1):
        b.frag_profile(which); b.frag_profile_wait()
        s = compare_unit(b, 0, frags, jc.oracle_path(o, which), api.ST_SHORTCUT, ("shortcut", which))
    assert [a.tolist() for a in b.unit_frag_support(0)[:3]] == [[1, 1, 0, 0, 0, 1, 0, 0], [0, 0, 1, 0, 0, 0, 1, 0], [0, 1, 2, -1, -1, 0, 0, -1]]
    assert s == dict(status=api.ST_SHORTCUT, cells=4, frags=8, frags_supported=5, first_unsupported=3, max_count=1, longest_supported=4, reserved=0, occurrences=5)
    b.close(); g.close()
    # (3) Infeasible .sol: the reference path over the six segments of the README example
    sol = os.path.join(workdir, "fp_infeasible.sol")
    with open(sol, "w") as f:
        f.write("Infeasible - objective value 0.00000000\n")
    frags = README_JUNCS + [[1, 2, 3], [-6, -5], [6, -6]]
    g = api.Graph(lib, readme); g.set_fragments(frags); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    b.upload(); b.run(0); b.download()
    assert b.unit_result(0)["status"] == api.ST_INFEASIBLE
    o = oracle.run_bfb(readme, [sol])["chr"][0]
    for which in (0, 1):
        b.frag_profile(which); b.frag_profile_wait()
        s = compare_unit(b, 0, frags, jc.oracle_path(o, which), api.ST_INFEASIBLE, ("infeasible", which))
    assert (s["cells"], s["frags_supported"], s["first_unsupported"], s["occurrences"]) == (6, 2, 0, 2), s
    b.close(); g.close()


def check_raw_unit(lib, workdir):
    """A raw unit (add_unit + set_unit_fragments) with segment ids above 255: both bytes of a cell matter.  The fragments are
    attached AFTER the run: the image goes to the device with the request."""
    s = synth.make_sample(300, 620, "chain", 7, seed=5100, name="fpraw")
    lh, _ = s.write(workdir)
    g = api.Graph(lib, lh)
    seg_cn = g.segments()["cn"].tolist()
    gj = g.junctions()
    J = [(int(a), int(b), int(c), int(d), float(e)) for a, b, c, d, e in zip(gj["src"], gj["sdir"], gj["tgt"], gj["tdir"], gj["cn"])]
    g.close()
    assert s.chr_ranges[0] == (1, 300)
    b = api.Batch(lib)
    u = jc._add_raw(b, seg_cn, J, s.elements[0])
    b.upload(); b.run(0); b.download()
    st = b.unit_result(u)["status"]
    assert st >= 0
    path = b.unit_path(u, 1).tolist()
    hi = [i for i in range(len(path) - 6) if abs(path[i + 2]) > 256 and abs(path[i + 2]) - 256 != abs(path[i + 3])]
    assert hi, "the path must visit segments above 256"
    frags = make_fragments(path, 77, n_random=16)
    for i in hi[:3] + hi[-3:]:
        f = path[i:i + 6]
        frags.append(list(f))
        low = list(f)
        low[2] = (abs(f[2]) - 256) * (1 if f[2] > 0 else -1)           # the same low byte, another segment
        frags.append(low); frags.append(rc(low))
    b.set_unit_fragments(u, frags)
    floors = dict.fromkeys(FLOORS, 0)
    for which in (0, 1):
        b.frag_profile(which); b.frag_profile_wait()
        compare_unit(b, u, frags, b.unit_path(u, which).tolist(), st, ("raw", which), floors=floors)
    assert floors["count0"] >= 2 and floors["two"] >= 1
    # replaced after a request: the version moves, the image and the layout go up again
    b.set_unit_fragments(u, frags[:5])
    with _raises(-32):
        b.unit_frag_profile(u)
    b.frag_profile(1); b.frag_profile_wait()
    compare_unit(b, u, frags[:5], path, st, "raw, replaced")
    b.close()


# ---- case 5: long paths ------------------------------------------------------------------------------------------------
def edge_fragments(path, seed):
    """Fragments across a thread's chunk edge (i = 8k - 1), across a sweep edge (i = 2048k - 1) and at i = P - L."""
    rng = random.Random(seed)
    P = len(path)
    out = []
    starts = [8 * k - 1 for k in (1, 2, 3, 100, 255, 256, 257)] + [2048 * k - 1 for k in range(1, P // 2048 + 1)] + [2048 * k - 2 for k in range(1, P // 2048 + 1)]
    for n, i in enumerate(starts):
        L = rng.randint(3, 30)
        if i + L > P:
            continue
        f = list(path[i:i + L])
        out.append(rc(f) if n % 3 == 2 else f)
    for L in (2, 9, 33):
        out.append(list(path[P - L:])); out.append(rc(path[P - L - 1:P - 1]))
    out.append(list(path[P - 5:]) + [path[0]])      # would need a cell behind P
    return out


def check_bench_unit(lib, oracle, workdir):
    s = synth.make_sample(256, 512, "wide", 19, seed=2100, n_del=1, n_dup=1, name="fpbig")
    lh, sols = s.write(workdir)
    big = oracle.run_bfb(lh, sols)["chr"][0]
    path = jc.oracle_path(big, 1)
    assert len(path) > 2048 * 4                     # several sweeps of 256 threads x 8 cells
    frags = edge_fragments(path, 3) + make_fragments(path, 4, n_random=8)[:8]
    g = api.Graph(lib, lh); g.set_fragments(frags)
    graphs, b, small = many_items(lib, oracle, workdir, 3)
    u = b.add_chromosome_sol(g, 0, sols[0])
    assert u == 3
    b.upload(); b.run(0); b.download()
    assert b.unit_path(3, 1).tolist() == big["path_indel"]
    floors = dict.fromkeys(FLOORS, 0)
    for which in (0, 1):
        b.frag_profile(which); b.frag_profile_wait()
        for k, (fr, oc, _) in enumerate(small):
            compare_unit(b, k, fr, jc.oracle_path(oc, which), jc.oracle_status(oc), ("beside bench", which, k))
        compare_unit(b, 3, frags, jc.oracle_path(big, which), 0, ("bench", which), floors=floors)
    assert floors["atend"] >= 2 and floors["count0"] >= 1 and floors["two"] >= 1, floors
    pc.close_all(graphs + [g], b)


def check_big_unit_finished_at_wait(lib, oracle, workdir):
    lh, sol, R, rev = pc.big_unit(oracle, workdir)
    path = jc.oracle_path(rev, 1)
    frags = edge_fragments(path, 5)
    g = api.Graph(lib, lh); g.set_fragments(frags)
    b = api.Batch(lib)
    b.configure(first_budget=4)
    b.add_chromosome_sol(g, 0, sol)
    graphs, items = [g], []
    for u, (l2, s2, oc) in enumerate(pc.many_units(oracle, workdir)[:39]):
        fr = make_fragments(jc.oracle_path(oc, 1), 9000 + u)
        g2 = api.Graph(lib, l2); graphs.append(g2)
        g2.set_fragments(fr)
        b.add_chromosome_sol(g2, 0, s2)
        items.append((fr, oc))
    b.debug_inject_validity(0, [0] * R + [1] * R)
    b.upload()
    for which in (1, 0):
        b.run(0)
        b.frag_profile(which)            # queued behind a run whose unit 0 is still PENDING
        b.wait()                         # the parallel search finishes it
        b.frag_profile_wait()            # ... and the profile is that of the final results
        b.download()
        r = b.unit_result(0)
        assert (r["status"], r["first_valid"], r["first_forward"]) == (0, 0, 0), r
        assert b.unit_path(0, 0).tolist() == rev["path"] and b.unit_path(0, 1).tolist() == rev["path_indel"]     # precondition
        s = compare_unit(b, 0, frags, jc.oracle_path(rev, which), 0, ("big", which))
        for u, (fr, oc) in enumerate(items):
            compare_unit(b, u + 1, fr, jc.oracle_path(oc, which), jc.oracle_status(oc), ("beside big", which, u))
    assert s["cells"] == len(rev["path"]) > 2048 * 4 and s["frags_supported"] >= 10
    pc.close_all(graphs, b)


# ---- case 6: three chromosomes of one sample ---------------------------------------------------------------------------
def check_three_chromosomes(lib, oracle, workdir):
    s = synth.make_sample(96, 200, "chain", 5, seed=11, n_chr=3, name="fp3chr")
    lh, sols = s.write(workdir)
    o = oracle.run_bfb(lh, sols)
    assert o["ok"] and len(o["chr"]) == 3 and o["chr"][2]["start"] > o["chr"][1]["start"] > 1
    # fragments of the three chromosomes interleaved, in ABSOLUTE ids as a file holds them; one that spans two chromosomes, a line of
    # one cell and an empty line, which is no fragment at all
    per = [[to_abs(f, oc["start"] - 1) for f in make_fragments(jc.oracle_path(oc, 1), 40 + c, n_random=6)] for c, oc in enumerate(o["chr"])]
    lines, owner = [], []
    for k in range(max(len(p) for p in per)):
        for c in (2, 0, 1):
            if k < len(per[c]):
                lines.append(per[c][k]); owner.append(c)
        if k == 1:
            lines.append([o["chr"][0]["end"], o["chr"][1]["start"]]); owner.append(-1)
            lines.append([o["chr"][1]["start"] + 2]); owner.append(-1)
    path = os.path.join(workdir, "fp3chr.juncs")
    with open(path, "w") as f:
        for k, line in enumerate(lines):
            f.write(" ".join("%d%s" % (abs(v), "+" if v > 0 else "-") for v in line) + "\n")
            if k == 3:
                f.write("\n")
    g = api.Graph(lib, lh)
    before = (g.junctions()["src"].tolist(), g.junctions()["cn"].tolist(), g.components(), g.log())
    g.read_fragments(path)
    assert (g.junctions()["src"].tolist(), g.junctions()["cn"].tolist(), g.components(), g.log()) == before     # the graph stays as it is
    assert g.fragments() == (lines, owner)
    g.set_fragments(lines)                                                                                      # round trip from memory
    assert g.fragments() == (lines, owner)
    b = api.Batch(lib)
    si = 0
    for c, oc in enumerate(o["chr"]):
        if oc["shortcut"]:
            b.add_chromosome(g, c, [], [])
        else:
            b.add_chromosome_sol(g, c, sols[si]); si += 1
    b.upload(); b.run(0); b.download()
    b.frag_profile(1); b.frag_profile_wait()
    owned = set()
    for c, oc in enumerate(o["chr"]):
        assert b.unit_path(c, 1).tolist() == oc["path_indel"], c
        gidx = [k for k, w in enumerate(owner) if w == c]
        base = oc["start"] - 1
        local = [[v - base if v > 0 else v + base for v in lines[k]] for k in gidx]
        compare_unit(b, c, local, jc.oracle_path(oc, 1), jc.oracle_status(oc), ("3chr", c), gidx)
        owned |= set(gidx)
    assert len(owned) + owner.count(-1) == len(lines) and owner.count(-1) == 2
    b.close()
    # unknown segment, a malformed token (read as id 0) and a missing file: the codes of read_juncs
    for text, code in (("1+ 9999+\n", -3), ("1+ x+ 2+\n", -3)):
        bad = os.path.join(workdir, "fp_bad.juncs")
        with open(bad, "w") as f:
            f.write(text)
        with _raises(code):
            g.read_fragments(bad)
        with _raises(code):
            api.Graph(lib, lh).read_juncs(bad)
        assert g.fragments() == (lines, owner)           # kept on an error
    g.read_fragments(os.path.join(workdir, "no_such_file.juncs"))
    api.Graph(lib, lh).read_juncs(os.path.join(workdir, "no_such_file.juncs"))
    assert g.fragments() == ([], [])
    g.close()


# ---- case 7: sharded -------------------------------------------------------------------------------------------------
def check_sharded(lib, oracle, workdir, devices):
    graphs, b, items = many_items(lib, oracle, workdir, 12)
    b.run_sharded(0, devices=devices)
    check_batch(b, items, ("sharded", tuple(devices)))
    with _raises(-32):
        b.frag_profile_device()          # one block per share: no single device view
    with _raises(-32):
        b.set_unit_fragments(0, [[1, 2]])     # the shares hold copies
    pc.close_all(graphs, b)


# ---- case 8: the queueing path's branches ----------------------------------------------------------------------------
def check_request_paths(lib, oracle, workdir, run_stream=None, req_stream=None):
    graphs, b, items = many_items(lib, oracle, workdir, 16)
    files = pc.many_units(oracle, workdir)[:16]
    b.upload()

    def compare(which, tag):
        for u, (frags, oc, _) in enumerate(items):
            compare_unit(b, u, frags, jc.oracle_path(oc, which), jc.oracle_status(oc), (tag, which, u))
    # (1) run on one stream, request on another, nothing waited for in between
    for which in (0, 1):
        b.run(0, run_stream)
        b.frag_profile(which, req_stream); b.frag_profile_wait()
        compare(which, "other stream")
    assert any(walk(jc.oracle_path(oc, 0), fr)[:3] != walk(jc.oracle_path(oc, 1), fr)[:3] for fr, oc, _ in items)    # (2) can tell the requests apart
    # (2) a request nobody waited for, then another: the second one answers
    for k in range(2):
        b.run(0, run_stream)
        b.frag_profile(0, req_stream); b.frag_profile(1, req_stream); b.frag_profile_wait()
        compare(1, ("unwaited", k))
    # (3) a request after download
    b.run(0, run_stream); b.download()
    b.frag_profile(0, req_stream); b.frag_profile_wait()
    compare(0, "after download")
    # (4) beside a junction profile and a copy-number profile of the same run: all three stay correct
    b.run(0, run_stream)
    b.junc_profile(1, req_stream); b.frag_profile(1, req_stream); b.profile(1, req_stream)
    b.profile_wait(); b.frag_profile_wait(); b.junc_profile_wait()
    b.download()
    compare(1, "beside two profiles")
    for u, ((lh, _, oc), g) in enumerate(zip(files, graphs)):
        idx, count, summary, _ = jc.unit_expectation(lh, g, oc, 1)
        jc.compare_unit(b, u, idx, count, summary, ("junction beside", u))
        n, want = pc.unit_expectation(b, u, oc, 1)
        pc.compare_unit(b, u, n, want, ("cn beside", u))
    # (5) closed with a request in flight; the next batch (other units, other offsets) gets the lease back
    b.run(0, run_stream)
    b.frag_profile(1, req_stream)
    pc.close_all(graphs, b)
    graphs, b, items = many_items(lib, oracle, workdir, 7)
    b.upload(); b.run(0, run_stream)
    check_batch(b, items, "after a close in flight")
    pc.close_all(graphs, b)


# ---- case 10: the CLI ------------------------------------------------------------------------------------------------
def check_cli(lib, exe, cwd, oracle, workdir):
    import test_cli_dropin as t
    readme, rsol = os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol")
    lh2, sol2, oc2 = pc.many_units(oracle, workdir)[1]
    # one fragment file for both samples: ids 1..6 exist in both; a line of one cell belongs to no unit
    frags = README_JUNCS + [[3], [3, -3], [2, 3, 4], [-4, -3, -2], [1, 2, 3, 4, 5, 6, 7]] + [list(jc.oracle_path(oc2, 1)[:4])]
    frags = [f for f in frags if all(abs(v) <= 6 for v in f)]
    ffile = os.path.join(cwd, "frags.juncs")
    with open(ffile, "w") as f:
        for line in frags:
            f.write(" ".join("%d%s" % (abs(v), "+" if v > 0 else "-") for v in line) + "\n")
    outs = []
    for k, extra in enumerate(([], ["--frag_profile", "frag.tsv", "--frags", ffile])):
        sub = os.path.join(cwd, "run%d" % k)
        os.makedirs(sub)
        bindir = os.path.join(sub, "bin")
        t.fake_cbc(bindir, [rsol, sol2])
        r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", readme + "," + lh2, "--lp_prefix", "two", *extra)
        assert r.returncode == 0, r.stderr
        outs.append((r.stdout, r.stderr, open(os.path.join(sub, "simulation_sv.txt"), "rb").read(), sorted(x for x in os.listdir(sub) if x != "bin")))
    assert outs[0][:3] == outs[1][:3]                                      # stdout, stderr, side file: unchanged by the option
    assert outs[1][3] == sorted(outs[0][3] + ["frag.tsv"])
    want = []
    for lh, sol in ((readme, rsol), (lh2, sol2)):
        oc = oracle.run_bfb(lh, [sol])["chr"][0]
        real = [f for f in frags if len(f) >= 2]
        fwd, rev, first, _ = walk(jc.oracle_path(oc, 1), real, jc.oracle_status(oc))
        per = iter(zip(fwd, rev, first))
        for k, f in enumerate(frags):
            a, b_, c = next(per) if len(f) >= 2 else (0, 0, -1)
            want.append("\t".join([lh, "0" if len(f) >= 2 else "-1", str(k), str(len(f)), str(a), str(b_), str(c)]))
    got = open(os.path.join(cwd, "run1", "frag.tsv")).read().splitlines()
    assert got == want and len(got) == 2 * len(frags) and any(line.split("\t")[4] != "0" for line in got[len(frags):])
    # --frags defaults to the file of --juncdb: against a run with --juncdb alone
    outs = []
    for k, extra in enumerate(([], ["--frag_profile", "frag.tsv"])):
        sub = os.path.join(cwd, "jdb%d" % k)
        os.makedirs(sub)
        bindir = os.path.join(sub, "bin")
        t.fake_cbc(bindir, [rsol])
        r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", readme, "--lp_prefix", "one", "--juncdb", os.path.join(cases.DATA, "readme6.juncs"), *extra)
        assert r.returncode == 0, r.stderr
        outs.append((r.stdout, r.stderr, open(os.path.join(sub, "simulation_sv.txt"), "rb").read()))
    assert outs[0] == outs[1]
    got = open(os.path.join(cwd, "jdb1", "frag.tsv")).read().splitlines()
    assert [line.split("\t")[1:] for line in got] == [["0", "0", "7", "1", "1", "5"], ["0", "1", "7", "1", "1", "5"], ["0", "2", "5", "2", "2", "2"]], got
    # a PROP C2 sample: its printed paths are rebuilt on the host -- refused, exit status 2, no file
    sub = os.path.join(cwd, "c2")
    os.makedirs(sub)
    bindir = os.path.join(sub, "bin")
    t.fake_cbc(bindir, [os.path.join(cases.DATA, "readme_c2_chr0.sol"), os.path.join(cases.DATA, "readme_c2_chr1.sol")])
    r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", os.path.join(cases.DATA, "readme_c2.lh"), "--lp_prefix", "c2", "--frag_profile", "frag.tsv",
                  "--frags", ffile)
    assert r.returncode == 2 and "--frag_profile" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(os.path.join(sub, "frag.tsv"))
    r = t.run_cli(exe, sub, bindir, "--help")
    assert "--frag_profile" in r.stdout and "--frags" in r.stdout


# ---- case 11: argument and state errors ------------------------------------------------------------------------------
class _raises:
    def __init__(self, code):
        self.code = code

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        assert et is not None and issubclass(et, api.AmbiError), "AmbiError %d expected" % self.code
        assert ev.code == self.code, (ev.code, self.code)
        return True


def check_errors(lib):
    lh, sol, juncs = (os.path.join(cases.DATA, "readme6." + x) for x in ("lh", "sol", "juncs"))
    g = api.Graph(lib, lh); g.read_fragments(juncs); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    for call in (lambda: b.frag_profile(1), b.frag_profile_wait):
        with _raises(-32):                                 # AMBI_ERR_STATE: nothing uploaded
            call()
    b.upload()
    for call in (lambda: b.frag_profile(1), b.frag_profile_wait, lambda: b.unit_frag_profile(0), lambda: b.unit_frag_support(0), b.frag_profile_device):
        with _raises(-32):                                 # uploaded, never run
            call()
    b.run(0); b.download()
    with _raises(-32):
        b.unit_frag_profile(0)                             # run, not profiled
    with _raises(-32):
        b.frag_profile_wait()                              # nothing queued
    for which in (2, -1):
        with _raises(-33):                                 # AMBI_ERR_ARG
            b.frag_profile(which)
    b.junc_profile(1); b.junc_profile_wait()
    with _raises(-32):
        b.unit_frag_profile(0)                             # another kind's request does not answer for this one
    b.frag_profile(1); b.frag_profile_wait()
    buf = [(ctypes.c_int32 * 8)() for _ in range(4)]
    assert lib.ambi_batch_unit_frag_support(b.h, 0, *buf, 2) == -33      # cap < F
    assert lib.ambi_batch_unit_frag_support(b.h, 0, buf[0], None, None, None, 3) == 3 and list(buf[0][:3]) == [1, 1, 2]
    assert lib.ambi_batch_unit_frag_support(b.h, 0, None, None, buf[2], buf[3], 3) == 3 and list(buf[2][:3]) == [5, 5, 2] and list(buf[3][:3]) == [0, 1, 2]
    for u in (1, -1):
        with _raises(-33):
            b.unit_frag_profile(u)                         # no such unit
        assert lib.ambi_batch_unit_frag_support(b.h, u, *buf, 8) == -33
    # the refusals of set_unit_fragments: L < 2, an id outside 1..n_seg, too many fragments, a bad unit
    for bad in ([[1]], [[1, 2], []], [[1, 7]], [[0, 1]], [[1, -7, 2]], [[1, 2]] * 65536):
        with _raises(-33):
            b.set_unit_fragments(0, bad)
    with _raises(-33):
        b.set_unit_fragments(1, [[1, 2]])
    assert b.unit_frag_profile(0)["frags"] == 3            # nothing of the refused calls was kept
    b.run(0)
    with _raises(-32):
        b.unit_frag_profile(0)                             # a new run: the old profile is gone
    b.wait()
    b.close()
    # the refusals of set_fragments: an id outside the graph, offsets that do not ascend from 0
    for bad in ([[1, 7]], [[0, 1]], [[1, 2], [3, -9]]):
        with _raises(-3):
            g.set_fragments(bad)
    cells = (ctypes.c_int32 * 4)(1, 2, 3, 4)
    for off in ((1, 2, 4), (0, 3, 2)):
        assert lib.ambi_graph_set_fragments(g.h, cells, (ctypes.c_int64 * 3)(*off), 2) == -2
    assert lib.ambi_graph_set_fragments(g.h, None, None, 1) == -33 and lib.ambi_graph_set_fragments(g.h, cells, None, -1) == -33
    assert g.fragments() == (README_JUNCS, [0, 0, 0])
    g.close()
    # a graph rebuilt for PROP I1 / C1: refused as .juncs are
    trx = [os.path.join(cases.DATA, x) for x in sorted(os.listdir(cases.DATA)) if x.endswith(".lh") and any(line.startswith("PROP") and ("I1" in line or "C1" in line) for line in open(os.path.join(cases.DATA, x)))]
    assert trx, "a PROP I1 / C1 sample among the test data"
    g = api.Graph(lib, trx[0])
    with _raises(-9):
        g.read_fragments(juncs)
    with _raises(-9):
        g.set_fragments([[1, 2]])
    with _raises(-9):
        g.read_juncs(juncs)
    g.close()
