"""The four on-request profiles (csrc/ambi_profile.hpp, ambi_junc_profile.hpp, ambi_frag_profile.hpp, ambi_evidence_profile.hpp) at
their window caps and under contention: generators, floors and checks shared by the CPU half (host simulation) and the GPU half
(the HIP engine) of tests/test_profile_fuzz.py -- same assertions, different library.

Expected values come only from the plain Python walks of the four *_checks.py modules (profile_checks.expected,
junc_profile_checks.walk, frag_profile_checks.walk, evidence_profile_checks.walk) over the unit's path: the ORACLE's path for units
built from files (precondition: the engine's path is the oracle's), the engine's own unit_path for raw units (pinned by the parity
tests).  A unit's walks are computed once per process and shared by every test that runs the unit, on either library; the
copy-number expectation is cheap and is computed every time (for raw units with far junctions it reads seg_cn after getIndelBias
from the library at hand).

Families
  A  caps      raw shortcut / infeasible units (path 1+ .. n+) whose segments, junctions and fragments sit on both sides of every
               window cap, no window variable set: every unit alone (the windows come from the batch's maxima), then all of them in
               one batch between six small units, which then run inside cap-sized tables
  B  repeats   synthetic units as raw units whose junction list carries 3000 repeats of its own junctions, written from either
               side, shuffled: "the lowest index wins" decided by racing atomic minima, the winner anywhere in the list
  C  dense     periodic paths of eval_checks' `copies` and `lengths` families under 1100 overlapping substrings, 1500 fragments on
               one first step (one chain in the table) and palindromes
  D  overflow  shortcut units of 3000 junction classes behind AMBI_JPROFILE_JUNC_WINDOW=3: partitions of 8 slots that overflow and
               double on the workgroup
"""
import os
import random

import numpy as np

import eval_checks
import evidence_profile_checks as ec
import frag_profile_checks as fc
import junc_profile_checks as jc
import profile_checks as pc
from ambigram_amd import api, synth

KINDS = ("path", "junction", "fragment", "evidence")
# the caps of the headers (kProfileWindowCap, kJuncSegWindowCap, kJuncWindowCap, kEvidenceJuncWindowCap, kFragWindowCap): what a
# window is when the batch's largest unit exceeds it.  Used for the floors only.
CAP_PATH_SEG, CAP_JUNC_SEG, CAP_JUNC, CAP_EVIDENCE_JUNC, CAP_PATTERNS = 4096, 2048, 2048, 1024, 2048


def last_window(total, cap):
    """Entries of the last window when `total` entries are served in windows of min(total, cap)."""
    w = max(1, min(total, cap))
    return total - (total - 1) // w * w if total > 0 else 0


def pattern_window(max_f, asked=0):
    """frag_window of ambi_frag_profile.hpp, for the floors: patterns per window of a batch whose largest unit has max_f fragments."""
    w = CAP_PATTERNS if max_f > CAP_PATTERNS // 2 else max(1, 2 * max_f)
    return asked if 0 < asked < w else w


# ---- units ------------------------------------------------------------------------------------------------------------------
class Unit:
    """One unit of a batch.  raw: the arrays of add_unit (J: (src, sdir, tgt, tdir, cn) per junction); file: .lh, .sol and the
    oracle's record.  frags: chains of LOCAL signed ids."""

    def __init__(self, name, frags, n=0, seg_cn=None, J=None, elements=(), infeasible=False, lh=None, sol=None, oc=None):
        self.name, self.frags, self.n, self.seg_cn, self.J, self.elements, self.infeasible = name, frags, n, seg_cn, J, list(elements), infeasible
        self.lh, self.sol, self.oc = lh, sol, oc
        self.raw = lh is None
        # a junction that is neither an adjacency nor a fold-back over at most two segments (the SVs of getIndelBias)
        self.far = self.raw and any(not ((j[1] == j[3] and j[2] * j[1] - j[0] * j[1] == 1) or (j[1] != j[3] and abs(j[0] - j[2]) <= 2)) for j in J)
        if not self.raw:
            self.n = oc["end"] - oc["start"] + 1


def add_to_batch(lib, b, unit):
    """Unit into the batch; the Graph of a file unit (to be closed by the caller) or None."""
    if unit.raw:
        J, E = unit.J, unit.elements
        b.add_unit(unit.n, 0, unit.seg_cn, [j[0] for j in J], [j[2] for j in J], [j[1] for j in J], [j[3] for j in J], [j[4] for j in J],
                   [1 if e.kind == "l" else 0 for e in E], [e.a for e in E], [e.b for e in E], [e.cn for e in E], infeasible=unit.infeasible)
        return None
    g = api.Graph(lib, unit.lh)
    g.set_fragments(unit.frags)
    b.add_chromosome_sol(g, 0, unit.sol)
    return g


# ---- expectations: the four walks, once per (unit, path) ----------------------------------------------------------------------
_EXPECT = {}


def expectation(unit, kind, which, b, u, g):
    """{kind: expected values} of unit `unit` = unit u of the batch b that has run and been downloaded; the walk of `kind` is run when no
    earlier test has run it for this unit and path."""
    if unit.raw:
        status = b.unit_result(u)["status"]
        path = b.unit_path(u, which).tolist()
        idx, ends, cn = list(range(len(unit.J))), [(x[0] * x[1], x[2] * x[3]) for x in unit.J], [x[4] for x in unit.J]
    else:
        oc = unit.oc
        assert oc["start"] == 1
        assert b.unit_path(u, 0).tolist() == oc["path"] and b.unit_path(u, 1).tolist() == oc["path_indel"], (unit.name, "engine path != oracle path")
        status, path = jc.oracle_status(oc), jc.oracle_path(oc, which)
        idx, ends, cn = jc.unit_junctions(unit.lh, g, oc["start"], oc["end"])
    key = (unit.name, status, tuple(path))
    e = _EXPECT.setdefault(key, dict(path_len=len(path)))
    if kind == "path":                              # cheap (numpy), and not kept: part of it may come from this library's prepare stage
        n = unit.n
        if unit.raw:
            # target_cn from the elements handed to add_unit (a loop counts twice its copies, a pattern once); seg_cn from the input
            # too, unless the unit carries far junctions: getIndelBias (LGM.cpp:3699-3744) then edits the copy numbers in the result
            # blob, which n_off_input is defined on, and they are read from unit_prepare as profile_checks.unit_expectation does
            # (the prepare stage is pinned against the oracle by the prepare fuzz)
            target = np.zeros(n + 1, np.int32)
            for el in unit.elements:
                target[el.a:el.b + 1] += 2 * el.cn if el.kind == "l" else 1
            seg_cn = b.unit_prepare(u, n)["seg_cn"] if unit.far else np.concatenate([[0.0], np.asarray(unit.seg_cn, float)])
        else:
            prep = b.unit_prepare(u, n)
            target, seg_cn = prep["target_cn"], prep["seg_cn"]
            if len(unit.oc.get("seg_cn") or []) >= n:
                seg_cn = np.concatenate([[0.0], np.asarray(unit.oc["seg_cn"], float)[:n]])
        e = dict(e, path=pc.expected(path, 0, n, target, seg_cn, status))
    if kind == "junction" and "junction" not in e:
        e["junction"] = (idx,) + jc.walk(path, ends, cn, status)
    if kind == "fragment" and "fragment" not in e:
        e["fragment"] = fc.walk(path, unit.frags, status)
    if kind == "evidence" and "evidence" not in e:
        floors = dict.fromkeys(ec.FLOORS, 0)
        e["evidence"] = (idx,) + ec.walk(path, unit.frags, ends, status, floors)
        e["evidence_floors"] = floors
    return e


def compare(kind, b, u, unit, e, tag):
    """Every array and every summary field of one kind, exactly."""
    if kind == "path":
        pc.compare_unit(b, u, unit.n, e["path"], tag)
    elif kind == "junction":
        idx, count, summary, _ = e["junction"]
        jc.compare_unit(b, u, idx, count, summary, tag)
    elif kind == "fragment":
        fwd, rev, first, summary = e["fragment"]
        got = b.unit_frag_support(u)
        assert got[0].tolist() == fwd, (tag, "fwd", _first_diff(got[0].tolist(), fwd))
        assert got[1].tolist() == rev, (tag, "rev", _first_diff(got[1].tolist(), rev))
        assert got[2].tolist() == first, (tag, "first", _first_diff(got[2].tolist(), first))
        assert got[3].tolist() == list(range(len(unit.frags))), (tag, "graph_index")
        s = b.unit_frag_profile(u)
        assert list(s) == list(fc.FIELDS) and s == summary, (tag, s, summary)
    else:
        idx, depth, count, covered, mind, summary = e["evidence"]
        got = b.unit_evidence_juncs(u)
        assert got[0].tolist() == count, (tag, "count", _first_diff(got[0].tolist(), count))
        assert got[1].tolist() == covered, (tag, "covered", _first_diff(got[1].tolist(), covered))
        assert got[2].tolist() == mind, (tag, "min_depth", _first_diff(got[2].tolist(), mind))
        assert got[3].tolist() == list(idx), (tag, "graph_index")
        s = b.unit_evidence_profile(u)
        assert list(s) == list(ec.FIELDS) and s == summary, (tag, s, summary)
        n = len(depth)
        half = n // 2                                       # the depth getter, in two halves
        have = b.unit_evidence_depth(u, 0, half).tolist() + b.unit_evidence_depth(u, half, n - half).tolist()
        assert have == depth, (tag, "depth", _first_diff(have, depth))


def _first_diff(got, want):
    if len(got) != len(want):
        return ("length", len(got), len(want))
    k = next(i for i, (x, y) in enumerate(zip(got, want)) if x != y)
    return ("at", k, "got", got[k], "want", want[k], "differing", sum(x != y for x, y in zip(got, want)))


_REQUEST = dict(path=("profile", "profile_wait"), junction=("junc_profile", "junc_profile_wait"), fragment=("frag_profile", "frag_profile_wait"),
                evidence=("evidence_profile", "evidence_profile_wait"))


class _Env:
    """The window variables for the calls inside; every one of them unset unless asked for."""
    NAMES = ("AMBI_PROFILE_WINDOW", "AMBI_JPROFILE_JUNC_WINDOW", "AMBI_JPROFILE_SEG_WINDOW", "AMBI_FPROFILE_FRAG_WINDOW")

    def __init__(self, **want):
        self.want = {k: str(v) for k, v in want.items()}
        assert set(self.want) <= set(self.NAMES)

    def __enter__(self):
        self.saved = {k: os.environ.pop(k, None) for k in self.NAMES}
        os.environ.update(self.want)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def run_batch(lib, units, kinds, tag, run_stream=None, req_stream=None, env=None, same_path_as=None):
    """The units in one batch and one run; then, per kind, both paths requested (on req_stream: a stream of its own on the GPU, None
    on the host simulation) and compared.  same_path_as: {unit index: unit index} -- the first must keep a status >= 0 and both
    paths of the second (family B: a unit and its plain twin)."""
    with _Env(**(env or {})):
        b = api.Batch(lib)
        graphs = [add_to_batch(lib, b, x) for x in units]
        b.upload(); b.run(0, run_stream); b.download()
        for u, x in enumerate(units):
            if x.raw:
                b.set_unit_fragments(u, x.frags)
        for u, v in (same_path_as or {}).items():
            assert b.unit_result(u)["status"] >= 0 and b.unit_result(u)["status"] == b.unit_result(v)["status"], (tag, units[u].name, b.unit_result(u))
            for which in (0, 1):
                assert b.unit_path(u, which).tolist() == b.unit_path(v, which).tolist(), (tag, units[u].name, "the repeats changed the path")
        for kind in kinds:
            request, wait = _REQUEST[kind]
            for which in (0, 1):
                getattr(b, request)(which, req_stream); getattr(b, wait)()
                for u, x in enumerate(units):
                    compare(kind, b, u, x, expectation(x, kind, which, b, u, graphs[u]), (tag, kind, x.name, which))
        b.close()
        for g in graphs:
            if g is not None:
                g.close()


# ---- fragments cut from a path ------------------------------------------------------------------------------------------------
def cut_fragments(path, F, rng, top=40, n_seg=None):
    """F substrings of the path with L = 2 .. top, half of them reverse-complemented, a fifth mutated in one cell."""
    P = len(path)
    n_seg = n_seg or max(abs(v) for v in path)
    out = []
    for k in range(F):
        L = rng.randint(2, min(top, P))
        i = rng.randint(0, P - L)
        f = list(path[i:i + L])
        if k % 5 == 4:
            at = rng.randrange(L)
            f[at] = -f[at] if rng.random() < 0.5 else (abs(f[at]) % n_seg + 1) * (1 if f[at] > 0 else -1)
        out.append(fc.rc(f) if k % 2 else f)
    return out


# ---- family A: the caps from both sides --------------------------------------------------------------------------------------
def cap_unit(name, n, m, F, seed, infeasible, removed=0.01):
    """A raw unit without a fold-back junction: it takes the shortcut (or, infeasible, the reference path), so its path is 1+ .. n+
    whatever junctions it carries.  m junctions: the adjacencies, about 1 % of them removed and half of them written from the other
    side, and distinct same- and opposite-strand far junctions at least three segments apart, shuffled."""
    rng = random.Random(seed)
    drop = set(rng.sample(range(1, n), max(1, int((n - 1) * removed))))
    J, seen = [], set()
    for i in range(1, n):
        if i in drop:
            continue
        seen.add((i, i + 1)); seen.add((-(i + 1), -i))
        J.append((i, 1, i + 1, 1) if rng.random() < 0.5 else (i + 1, -1, i, -1))
    assert len(J) <= m, (name, len(J), m)
    while len(J) < m:
        s, t = rng.randint(1, n), rng.randint(1, n)
        if abs(s - t) < 3:
            continue
        sd, td = rng.choice((1, -1)), rng.choice((1, -1))
        e = (s * sd, t * td)
        if e in seen or (-e[1], -e[0]) in seen:
            continue
        seen.add(e)
        J.append((s, sd, t, td))
    rng.shuffle(J)
    J = [x + (float(rng.randint(0, 2)),) for x in J]
    path = list(range(1, n + 1))
    frags = cut_fragments(path, F, rng, n_seg=n)
    return Unit(name, frags, n=n, seg_cn=[float(rng.randint(1, 3)) for _ in range(n)], J=J, infeasible=infeasible)


# (name, n, m, F, infeasible): every cap with a unit at it and a unit one above it; a last window of one segment (n = 4097 for the
# path profile, 2049 and 4097 for the junction profile), of one junction (m = 2049; 1025 for the evidence scan) and of two patterns
# (F = 1025).  The units with m = 1024 / 1025 have fewer segments than the others: a list with 99 % of the adjacencies has at least
# 0.99 (n - 1) junctions.
# The HIP engine sizes the work areas of its prepare and finish kernels for the largest unit of a batch and refuses the batch at
# upload when one of them exceeds a CU's group memory (about 16 bytes per segment, 10 per junction and 24 more per far junction in
# the finish stage): at 4096 and more segments that leaves room for about 6000 junctions, so the lists of the large units stop
# below that.  The unit with about 10 000 junctions (HOST_ONLY) runs on the host simulation, which has no such limit; on the device
# its refusal is what is asserted.  a5000 stays out of the one-batch run for the same reason: a batch's maxima combine.
CAP_UNITS = (("a2048", 2048, 2048, 1024, False), ("a2049", 2049, 2049, 1025, True), ("a4096", 4096, 5600, 300, False),
             ("a4097", 4097, 5000, 200, True), ("a5000", 5000, 5400, 200, False), ("a700", 700, 1024, 1025, True),
             ("a701", 701, 1025, 1024, False), ("a1500", 1500, 2049, 2500, False), ("a10000", 5000, 9948, 64, True))
HOST_ONLY, ALONE_ONLY = ("a10000",), ("a5000", "a10000")
_CAPS = []


def cap_units():
    if not _CAPS:
        _CAPS.extend(cap_unit(name, n, m, F, 7100 + k, inf) for k, (name, n, m, F, inf) in enumerate(CAP_UNITS))
    return _CAPS


# An even window never splits a fragment's two patterns 2f and 2f + 1, and without a window variable the window is even (twice the
# fragments, or the cap).  The split across two windows is therefore reached with the largest ODD window below the cap: patterns
# 2046 | 2047 of fragment 1023 then lie in different windows of the F = 1025 unit, and the last window has three patterns.
SPLIT_WINDOW = CAP_PATTERNS - 1


def cap_floors():
    """From the inputs alone."""
    units = cap_units()
    ns, ms, Fs = {x.n for x in units}, {len(x.J) for x in units}, {len(x.frags) for x in units}
    assert {CAP_JUNC_SEG, CAP_JUNC_SEG + 1, CAP_PATH_SEG, CAP_PATH_SEG + 1, 5000} <= ns, sorted(ns)
    assert {CAP_EVIDENCE_JUNC, CAP_EVIDENCE_JUNC + 1, CAP_JUNC, CAP_JUNC + 1} <= ms and max(ms) >= 9900, sorted(ms)
    assert {CAP_PATTERNS // 2, CAP_PATTERNS // 2 + 1, 2500} <= Fs, sorted(Fs)
    assert any(last_window(x.n, CAP_PATH_SEG) == 1 for x in units) and any(last_window(x.n, CAP_JUNC_SEG) == 1 for x in units)
    assert any(last_window(len(x.J), CAP_JUNC) == 1 for x in units) and any(last_window(len(x.J), CAP_EVIDENCE_JUNC) == 1 for x in units)
    assert any(last_window(2 * len(x.frags), pattern_window(len(x.frags))) == 2 for x in units)
    assert all(pattern_window(len(x.frags)) % 2 == 0 for x in units)            # (why SPLIT_WINDOW exists)
    split = [x for x in units if len(x.frags) == CAP_PATTERNS // 2 + 1]
    w = pattern_window(len(split[0].frags), SPLIT_WINDOW)
    f = [f for f in range(len(split[0].frags)) if (2 * f) // w != (2 * f + 1) // w]
    assert w == SPLIT_WINDOW and f and all(fc.rc(split[0].frags[k]) != split[0].frags[k] for k in f), (w, f)   # palindrome-free, in two windows
    for x in units:                                                              # the adjacencies removed: something is unmatched
        assert sum(1 for j in x.J if abs(abs(j[0]) - abs(j[2])) == 1 and j[1] == j[3]) < x.n - 1
    return dict(n=sorted(ns), m=sorted(ms), F=sorted(Fs), split_fragments=f)


def small_units(oracle, workdir, k=6):
    out = []
    for u, (lh, sol, oc) in enumerate(pc.many_units(oracle, workdir)[:k]):
        out.append(Unit("small%d" % u, fc.make_fragments(jc.oracle_path(oc, 1), 9000 + u), lh=lh, sol=sol, oc=oc))
    return out


def check_caps(lib, oracle, workdir, kind, run_stream=None, req_stream=None):
    units = cap_units()
    device = lib.ambi_backend_name() == b"hip"
    for x in units:                                                              # alone: the windows are this unit's
        if device and x.name in HOST_ONLY:
            b = api.Batch(lib)
            add_to_batch(lib, b, x)
            with fc._raises(-17):                                                # refused at upload: the finish stage's work area
                b.upload()
            b.close()
            continue
        run_batch(lib, [x], (kind,), "caps, alone", run_stream, req_stream)
    if kind in ("fragment", "evidence"):
        x = next(x for x in units if len(x.frags) == CAP_PATTERNS // 2 + 1)
        run_batch(lib, [x], (kind,), "caps, odd pattern window", run_stream, req_stream, env=dict(AMBI_FPROFILE_FRAG_WINDOW=SPLIT_WINDOW))
    small = small_units(oracle, workdir)
    big = [x for x in units if x.name not in ALONE_ONLY]
    mixed = small[:3] + big[:4] + small[3:4] + big[4:] + small[4:]                # the small units inside cap-sized tables
    run_batch(lib, mixed, (kind,), "caps, one batch", run_stream, req_stream)
    st = {x.name: _cap_status(x) for x in units if not (device and x.name in HOST_ONLY)}
    assert set(st.values()) <= {api.ST_SHORTCUT, api.ST_INFEASIBLE} and {x.infeasible for x in units} == {False, True}, st


def _cap_status(unit):
    keys = [k for k in _EXPECT if k[0] == unit.name]
    assert keys and all(k[2] == tuple(range(1, unit.n + 1)) for k in keys), (unit.name, "the path is not 1+ .. n+")
    return keys[0][1]


# ---- family B: repeats -------------------------------------------------------------------------------------------------------
REPEAT_TIERS = (("chain", 48, 100, 7), ("wide", 96, 200, 7), ("skew", 160, 330, 6), ("mixed", 300, 620, 7))
N_REPEATS = 3000
_REPEATS = {}


def repeat_units(lib, workdir):
    """[(unit with repeats, its plain twin)]: three seeds for each of four synth tiers, read back from the sample's graph as
    junc_profile_checks._raw_source does.  The extras are repeats only -- the same edge or the edge written from the other side, copy
    numbers 0 .. 5 --, and the whole list is shuffled: the winning index of a class sits anywhere."""
    if workdir not in _REPEATS:
        out = []
        for t, (tier, n, m, K) in enumerate(REPEAT_TIERS):
            for k in range(3):
                seed = 5200 + 10 * t + k
                s = synth.make_sample(n, m, tier, K, seed=seed, name="pfz_%s%d" % (tier, k))
                lh, _ = s.write(workdir)
                g = api.Graph(lib, lh)
                seg_cn = g.segments()["cn"].tolist()
                gj = g.junctions()
                J = [(int(a), int(b), int(c), int(d), float(e)) for a, b, c, d, e in zip(gj["src"], gj["sdir"], gj["tgt"], gj["tdir"], gj["cn"])]
                g.close()
                assert s.chr_ranges[0] == (1, n)
                rng = random.Random(seed)
                flip = lambda x, cn: (x[2], -x[3], x[0], -x[1], cn)             # the same edge from the other side
                tagged = [(x, True, False) for x in J]                          # (junction, original, written from the other side)
                for _ in range(N_REPEATS):
                    x = rng.choice(J)
                    cn = float(rng.randint(0, 5))
                    other = rng.random() < 0.5
                    tagged.append((flip(x, cn) if other else x[:4] + (cn,), False, other))
                rng.shuffle(tagged)
                frags = None                                                    # cut from the path once it is known (repeat_fragments)
                twin = Unit("b_%s%d_plain" % (tier, k), frags, n=n, seg_cn=seg_cn, J=J, elements=s.elements[0])
                full = Unit("b_%s%d" % (tier, k), frags, n=n, seg_cn=seg_cn, J=[t[0] for t in tagged], elements=s.elements[0])
                full.original, full.other_side = [t[1] for t in tagged], [t[2] for t in tagged]
                out.append((full, twin))
        b = api.Batch(lib)                                                      # the plain twins' final paths: what the fragments are cut from
        for _, twin in out:
            add_to_batch(lib, b, twin)
        b.upload(); b.run(0); b.download()
        for u, (full, twin) in enumerate(out):
            assert b.unit_result(u)["status"] >= 0, twin.name
            path = b.unit_path(u, 1).tolist()
            full.frags = twin.frags = fc.make_fragments(path, 300 + u) + cut_fragments(path, 40, random.Random(400 + u), n_seg=twin.n)
        b.close()
        _REPEATS[workdir] = out
    return _REPEATS[workdir]


def check_repeats(lib, hostsim_lib, workdir, kind, run_stream=None, req_stream=None):
    pairs = repeat_units(hostsim_lib, workdir)
    units = [x for pair in pairs for x in pair]
    run_batch(lib, units, (kind,), "repeats", run_stream, req_stream, same_path_as={2 * k: 2 * k + 1 for k in range(len(pairs))})


def repeat_floors(hostsim_lib, workdir):
    """From the junction lists and the walks (the expectations of the host simulation's run)."""
    pairs = repeat_units(hostsim_lib, workdir)
    both_sides = 0
    report = []
    for full, _ in pairs:
        classes = {}
        for j, x in enumerate(full.J):
            e = (x[0] * x[1], x[2] * x[3])
            classes.setdefault(min(e, (-e[1], -e[0])), []).append(j)
        assert sum(len(v) >= 3 for v in classes.values()) >= 40, full.name
        keys = [k for k in _EXPECT if k[0] == full.name]
        assert keys, (full.name, "run check_repeats on the host simulation first")
        used = moved = 0
        for key in keys:
            count = _EXPECT[key]["junction"][1]
            for v in classes.values():
                if count[v[0]] > 0:                                             # the walk credits the lowest index
                    used += 1; moved += not full.original[v[0]]
        assert used >= 10 and 3 * moved >= used, (full.name, used, moved)
        # a fold-back class repeated as it stands and "from the other side".  For a fold-back (a, d, a, -d) the other side's writing is the
        # identical tuple, so this adds no input of its own: such a class is repeated, never mirrored.  Kept as the condition it is.
        for v in classes.values():
            x = full.J[v[0]]
            if x[0] == x[2] and x[1] != x[3] and any(full.other_side[j] for j in v) and any(not full.other_side[j] and not full.original[j] for j in v):
                both_sides += 1
        report.append((full.name, len(full.J), len(classes), used, moved))
    assert both_sides >= 1
    return report


# ---- family C: dense evidence and long chains ---------------------------------------------------------------------------------
DENSE_SETS = ("substrings", "one_first_step", "palindromes")
DENSE_MAX_CELLS, DENSE_SMALL_CELLS = 1000, 400
_DENSE = {}


def dense_fragments(path, which_set, seed):
    rng = random.Random(seed)
    P = len(path)
    if which_set == "substrings":                  # (a) 1100 substrings with L = 2 .. 30, half reverse-complemented; the path and its reverse complement
        out = []
        for k in range(1100):
            L = rng.randint(2, min(30, P))
            i = rng.randint(0, P - L)
            f = list(path[i:i + L])
            out.append(fc.rc(f) if k % 2 else f)
        return out + [list(path), fc.rc(path)]
    if which_set == "one_first_step":              # (b) 1500 fragments on the path's most frequent step: one slot, one chain
        steps = {}
        for i in range(P - 1):
            steps.setdefault((path[i], path[i + 1]), []).append(i)
        best = max(sorted(steps), key=lambda s: len(steps[s]))
        top = max(abs(v) for v in path)
        out = []
        for k in range(1500):
            i = rng.choice(steps[best])
            f = list(path[i:i + 2 + min(rng.randint(0, 38), P - i - 2)])        # tails of 0 .. 38 cells, real continuations ...
            if k % 3 == 2 and len(f) > 2:                                       # ... or mutated behind the first step
                at = rng.randrange(2, len(f))
                f[at] = -f[at] if rng.random() < 0.5 else (abs(f[at]) % top + 1) * (1 if f[at] > 0 else -1)
            out.append(f)
        return out
    # (c) palindromes -- fold-back turns of the path grown outwards, and (x, -x) pairs the path does not take -- among ordinary fragments,
    # at odd and even indices
    turns = [i for i in range(P - 1) if path[i + 1] == -path[i]]
    top = max(abs(v) for v in path)
    out = []
    for k in range(60):
        if k % 3 == 0:
            L = rng.randint(2, min(12, P)); i = rng.randint(min(2, P - L), max(min(2, P - L), P - L - 2))   # (not the ends: the first and the last step stay uncovered in some units)
            out.append(list(path[i:i + L]))
            continue
        if turns and k % 3 == 1:
            i = rng.choice(turns)
            arm = rng.randint(1, 6)
            lo = max(0, i - arm + 1)
            left = list(path[lo:i + 1])
            out.append(left + fc.rc(left))         # a palindrome by construction; supported when the path mirrors that far
        else:
            x = rng.randint(1, top) * rng.choice((1, -1))
            arm = [x] if rng.random() < 0.5 else [rng.randint(1, top), x]
            out.append(arm + fc.rc(arm))
        if rng.random() < 0.5:
            out.append([path[P // 2 - 1], path[P // 2]])                        # shifts the parity of the indices behind it
    return out


def dense_candidates(oracle, workdir):
    return [u for fam in ("copies", "lengths") for u in eval_checks.family_units(oracle, workdir, fam)]


def dense_units(oracle, workdir):
    """Twelve units of eval_checks' copies and lengths families, chosen for the floors from the oracle's paths alone: the four with
    at most DENSE_MAX_CELLS cells whose most frequent step occurs most often (counts), and of those with at most DENSE_SMALL_CELLS
    cells the two of that kind, the three longest and the three shortest; {set name: [Unit]}."""
    if workdir not in _DENSE:
        cand = dense_candidates(oracle, workdir)
        score = []
        for u in cand:
            oc = u["o"][False]
            path = jc.oracle_path(oc, 1)
            steps = {}
            for i in range(len(path) - 1):
                steps[(path[i], path[i + 1])] = steps.get((path[i], path[i + 1]), 0) + 1
            score.append((len(path), max(steps.values(), default=0), u))
        # (the walks are quadratic: 1100 fragments x P positions, so only the four units that carry the count floor are long)
        score = [t for t in score if t[0] <= DENSE_MAX_CELLS]
        small = [t for t in score if t[0] <= DENSE_SMALL_CELLS]
        by_rep = sorted(score, key=lambda t: (-t[1], t[2]["name"]))
        small_rep = sorted(small, key=lambda t: (-t[1], t[2]["name"]))
        small_len = sorted(small, key=lambda t: (-t[0], t[2]["name"]))
        chosen = []
        for t in by_rep[:4] + small_rep[:2] + small_len[:3] + small_len[-3:] + small_rep[2:]:
            if t[2]["name"] not in [c["name"] for c in chosen] and len(chosen) < 12:
                chosen.append(t[2])
        assert len(chosen) == 12
        out = {}
        for si, name in enumerate(DENSE_SETS):
            out[name] = []
            for k, u in enumerate(chosen):
                oc = u["o"][False]
                frags = dense_fragments(jc.oracle_path(oc, 1), name, 8000 + 100 * si + k)
                out[name].append(Unit("c_%s_%s" % (name, u["name"]), frags, lh=u["lh"], sol=u["sol"], oc=oc))
                out[name][-1].base = u["name"]
        _DENSE[workdir] = out
    return _DENSE[workdir]


def check_dense(lib, oracle, workdir, kind, run_stream=None, req_stream=None):
    for name, units in dense_units(oracle, workdir).items():                    # three separate runs per unit
        run_batch(lib, units, (kind,), "dense, " + name, run_stream, req_stream)


def dense_floors(oracle, workdir):
    """From the walks (the expectations of the host simulation's run) and the inputs."""
    sets = dense_units(oracle, workdir)
    depth256, count64 = set(), set()                                            # distinct units of the twelve
    chain = pal_yes = pal_no = 0
    floors = dict.fromkeys(ec.FLOORS, 0)
    top = dict(max_depth=0, max_count=0, occurrences=0)
    for name, units in sets.items():
        for x in units:
            keys = [k for k in _EXPECT if k[0] == x.name]
            assert keys, (x.name, "run check_dense on the host simulation first")
            es = [_EXPECT[k] for k in keys]
            base = x.base
            if any(e["evidence"][5]["max_depth"] >= 256 for e in es):
                depth256.add(base)
            if any(e["fragment"][3]["max_count"] >= 64 for e in es):
                count64.add(base)
            for e in es:
                top["max_depth"] = max(top["max_depth"], e["evidence"][5]["max_depth"]); top["max_count"] = max(top["max_count"], e["fragment"][3]["max_count"])
                top["occurrences"] = max(top["occurrences"], e["fragment"][3]["occurrences"])
            for k in ec.FLOORS:
                floors[k] += any(e["evidence_floors"][k] for e in es)
            first = {}
            for f in x.frags:
                first[(f[0], f[1])] = first.get((f[0], f[1]), 0) + 1
                r = fc.rc(f)
                if r != f:
                    first[(r[0], r[1])] = first.get((r[0], r[1]), 0) + 1
            chain += max(first.values()) >= 1500
            if name == "palindromes":
                fwd = es[-1]["fragment"][0]
                for f, c in zip(x.frags, fwd):
                    if fc.rc(f) == f:
                        pal_yes += c > 0; pal_no += c == 0
    depth256, count64 = len(depth256), len(count64)
    assert depth256 >= 3 and count64 >= 3 and chain >= 1 and pal_yes >= 3 and pal_no >= 3, (depth256, count64, chain, pal_yes, pal_no)
    assert all(floors[k] >= 3 for k in ec.FLOORS), floors
    return dict(depth256=depth256, count64=count64, chains_1500=chain, palindromes_supported=pal_yes, palindromes_unsupported=pal_no, floors=floors, top=top)


# ---- family D: overflow and doubling -----------------------------------------------------------------------------------------
# The key functions of ambi_junc_profile.hpp (junc_key, junc_canon, junc_mix, junc_in_part) in a few lines of Python.  This
# transcription is NOT a reference: it only SELECTS inputs -- it says which seeds put more classes into one partition than the table has
# slots -- and the precondition it states is asserted.  Every expected value still comes from the walks.
OVERFLOW_WINDOW, OVERFLOW_SLOTS = 3, 8


def _key(x, y):
    return ((x & 0xFFFF) << 16) | (y & 0xFFFF)


def _canon(x, y):
    return min(_key(x, y), _key(-y, -x))


def _mix(h):
    h ^= h >> 16; h = h * 0x85EBCA6B & 0xFFFFFFFF; h ^= h >> 13; h = h * 0xC2B2AE35 & 0xFFFFFFFF; h ^= h >> 16
    return h


def fullest_partition(unit, nparts):
    load = {}
    for k in {_canon(x[0] * x[1], x[2] * x[3]) for x in unit.J}:
        p = _mix(k ^ 0x9E3779B9) % nparts
        load[p] = load.get(p, 0) + 1
    return max(load.values())


def overflow_rounds(unit):
    """Passes the stage starts with and how often it doubles them before every partition fits the table."""
    nparts = -(-len(unit.J) // OVERFLOW_WINDOW)
    first, doublings = nparts, 0
    while fullest_partition(unit, nparts) > OVERFLOW_SLOTS:
        nparts *= 2; doublings += 1
    return first, doublings


_OVERFLOW = []
OVERFLOW_SEEDS = (7300, 7418)      # the second: the first of 7400 .. with a second-round overflow (seeds 7418, 7422 and 7443 of the first 44 have one)


def overflow_unit(name, seed, infeasible):
    """Half of the adjacencies and as many far junctions (cap_unit): the classes, and with them the partitions' loads, change with the seed."""
    return cap_unit(name, 3000, 3000, 300, seed, infeasible, removed=0.5)


def overflow_units():
    """Two shortcut units of 3000 segments and 3000 distinct junction classes: the first overflows a partition of the first round;
    the second (found by a search over the seeds with the functions above, about a second) overflows one of the second round as
    well and doubles twice.  test_overflow_precondition asserts both."""
    if not _OVERFLOW:
        a = overflow_unit("d_once", OVERFLOW_SEEDS[0], False)
        b = overflow_unit("d_twice", OVERFLOW_SEEDS[1], True)
        _OVERFLOW.extend([a, b])
    return _OVERFLOW


def check_overflow(lib, kind, run_stream=None, req_stream=None):
    for x in overflow_units():
        run_batch(lib, [x], (kind,), "overflow", run_stream, req_stream, env=dict(AMBI_JPROFILE_JUNC_WINDOW=OVERFLOW_WINDOW))
