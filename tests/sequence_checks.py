"""Checks of the path sequences (ambi_batch_sequence, csrc/ambi_sequence.hpp) shared by the CPU host-simulation tests and the GPU
tests (same assertions, different library).

Expected values never come from the engine: the cells are the ORACLE's path of the unit (oracle.run_bfb: path / path_indel), the
bases are what the test attached, and the two are joined by `expected_seq` below: a plain concatenation, a cell on the '-' strand
as the reverse complement through the issue's table."""
import os

import numpy as np
import pytest

import cases
import profile_checks as pc
from ambigram_amd import api

_SRC = b"ACGTUMRWSYKVHDBN"
_DST = b"TGCAAKYWSRMBDHVN"
COMP = bytes.maketrans(_SRC + _SRC.lower(), _DST + _DST.lower())        # every other byte value maps to itself
ALPHABET = b"ACGTNacgtnRYKMSWBDHVryk-*" + bytes([0, 255])
TILE = 4096                                                               # kSeqTile: output bytes per fill work item
ERR_TOO_LARGE, ERR_STATE, ERR_ARG = -34, -32, -33


def revcomp(s):
    return s.translate(COMP)[::-1]


def expected_seq(path_abs, base, segs):
    """path: absolute signed ids; local id = |id| - base; segs[i]: bytes of local segment i + 1."""
    out = bytearray()
    for c in path_abs:
        s = segs[abs(c) - base - 1]
        out += s if c > 0 else revcomp(s)
    return bytes(out)


def oracle_path(oc, which, status=None):
    """The cells ambi_batch_unit_path(unit, which) returns, from the oracle's record; [] for a refused unit."""
    if status is not None and status < 0:
        return []
    path = oc["path_indel"] if which else oc["path"]
    if (oc["shortcut"] or oc["infeasible"]) and not path:
        path = list(range(oc["start"], oc["end"] + 1))        # the reference path 1+ .. n+ (localhap.cpp:164-170, :213-220)
    return path


def draw_segments(rng, lengths):
    return [bytes(rng.choice(np.frombuffer(ALPHABET, np.uint8), size=int(n)).astype(np.uint8)) for n in lengths]


def attach(g, segs):
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    g.set_sequences(b"".join(segs), off)


def want_of(oc, which, segs, status=None):
    return expected_seq(oracle_path(oc, which, status), oc["start"] - 1, segs)


def compare_units(b, wants, tag, first=0):
    for k, w in enumerate(wants):
        u = first + k
        assert b.unit_sequence_len(u) == len(w), (tag, u, b.unit_sequence_len(u), len(w))
        got = b.unit_sequence(u)
        assert got == w, (tag, u, len(w), next(i for i in range(len(w)) if got[i] != w[i]))


# ---- case 1: the README example (express path) ------------------------------------------------------------------------
def check_readme(lib, oracle):
    lh, sol = os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol")
    oc = oracle.run_bfb(lh, [sol])["chr"][0]
    segs = draw_segments(np.random.default_rng(61), [1, 2, 3, 5, 16, 17])
    g = api.Graph(lib, lh); attach(g, segs)
    b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    b.upload(); b.run(0); b.download()
    assert b.unit_path(0, 1).tolist() == oc["path_indel"] and b.unit_path(0, 0).tolist() == oc["path"]       # precondition
    for which in (0, 1):
        b.sequence(which); b.sequence_wait()
        compare_units(b, [want_of(oc, which, segs)], ("readme6", which))
    # README.md:122 by hand, the first two runs: 1+ .. 6+ then 6- .. 2-
    fwd = b"".join(segs)
    assert b.unit_sequence(0, 0, len(fwd)) == fwd
    assert b.unit_sequence(0, len(fwd), len(fwd) - 1) == revcomp(b"".join(segs[1:]))
    b.close(); g.close()


# ---- case 2: edge units -----------------------------------------------------------------------------------------------
def check_edge_units(lib, oracle, workdir):
    """One batch: a long unit, the shortcut path 1+..4+ whose whole output is shorter than 16 bytes, a refused unit (status -11,
    length 0), the reference path of an infeasible .sol, and a long unit again: the neighbours of the short and the empty one intact."""
    readme, rsol = os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol")
    lh = os.path.join(workdir, "seq_nofbi.lh")
    with open(lh, "w") as f:
        f.write(pc.NOFBI)
    inf = os.path.join(workdir, "seq_infeasible.sol")
    with open(inf, "w") as f:
        f.write("Infeasible - objective value 0.00000000\n")
    sol0 = os.path.join(workdir, "seq_empty.sol")
    with open(sol0, "w") as f:
        f.write("Optimal - objective value 0.00000000\n")
    rng = np.random.default_rng(62)
    plan = [(readme, rsol, [7, 9, 33, 4, 21, 18], None), (lh, None, [3, 1, 2, 5], None), (readme, sol0, [5, 5, 5, 5, 5, 5], -11),
            (readme, inf, [2, 30, 1, 1, 16, 9], None), (readme, rsol, [17, 1, 15, 16, 2, 40], None)]
    graphs, wants, b = [], {0: [], 1: []}, api.Batch(lib)
    for path, sol, lens, status in plan:
        segs = draw_segments(rng, lens)
        g = api.Graph(lib, path); attach(g, segs); graphs.append(g)
        if sol is None:
            b.add_chromosome(g, 0, [], [])
        else:
            b.add_chromosome_sol(g, 0, sol)
        oc = oracle.run_bfb(path, [sol] if sol else [])["chr"][0] if status is None else None
        for which in (0, 1):
            wants[which].append(b"" if oc is None else want_of(oc, which, segs))
    b.upload(); b.run(0); b.download()
    assert [b.unit_result(u)["status"] for u in range(5)] == [0, api.ST_SHORTCUT, -11, api.ST_INFEASIBLE, 0]
    for which in (0, 1):
        b.sequence(which); b.sequence_wait()
        compare_units(b, wants[which], ("edge", which))
        assert 0 < len(wants[which][1]) < 16 and len(wants[which][2]) == 0 and len(wants[which][3]) == 59
    pc.close_all(graphs, b)


# ---- case 3: a batch above the express limit, with the coverage the kernel needs -------------------------------------------
def runs_of(path):
    """[(first cell, cells)] of the stretches counting up by one."""
    runs = []
    for c in path:
        if runs and c == runs[-1][0] + runs[-1][1]:
            runs[-1][1] += 1
        else:
            runs.append([c, 1])
    return runs


def coverage(records, seg_lists, long_at):
    """What the oracle's runs, with these segment lengths, exercise; from the oracle alone."""
    cov = dict(starts=set(), one_base=set(), three_in_group=False, ends_on_16=False, long_strands=set())
    lu, ls = long_at
    for u, (oc, segs) in enumerate(zip(records, seg_lists)):
        base = oc["start"] - 1
        for which in (0, 1):
            at, edges = 0, []
            for c, k in runs_of(oracle_path(oc, which)):
                ids = range(abs(c) - base, abs(c) - base + k) if c > 0 else range(abs(c) - base - k + 1, abs(c) - base + 1)
                nbytes = sum(len(segs[i - 1]) for i in ids)
                if nbytes == 0:
                    continue
                strand = c > 0
                cov["starts"].add((at % 16, strand))
                if nbytes == 1:
                    cov["one_base"].add(strand)
                if u == lu and ls in ids:
                    cov["long_strands"].add(strand)
                edges.append(at)
                at += nbytes
                if at % 16 == 0:
                    cov["ends_on_16"] = True
            # runs in a 16-byte group of the output: those that start in it, plus the one that reaches into it from before
            starts = np.asarray(edges, np.int64)
            if len(starts):
                per_group = np.bincount(starts // 16)
                reached = ~np.isin(np.arange(len(per_group)) * 16, starts)
                if np.any(per_group + reached >= 3):
                    cov["three_in_group"] = True
    return cov


def covered(cov):
    return (len(cov["starts"]) == 32 and cov["one_base"] == {True, False} and cov["three_in_group"] and cov["ends_on_16"]
            and cov["long_strands"] == {True, False})


_MANY = {}


def many_sequences(oracle, workdir):
    """pc.many_units plus one hand-made unit, with seeded bases: lengths 1..40, one segment longer than two fill tiles on a segment
    that a path crosses on both strands.  The seed is the first of a short search whose inputs pass `covered`."""
    if workdir not in _MANY:
        items = list(pc.many_units(oracle, workdir))
        # a hand-made unit for what the 40 cannot supply (none of their paths has a '-' run of one cell): readme6 with an empty
        # segment 3 and a one-base segment 4, so that its runs `4-3-` and `3+4+` are one base long
        lh, sol = os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol")
        items.append((lh, sol, oracle.run_bfb(lh, [sol])["chr"][0]))
        hand = {len(items) - 1: [5, 3, 0, 1, 2, 7]}
        records = [oc for _, _, oc in items]
        long_at = None
        for u, oc in enumerate(records):
            for which in (0, 1):
                p = oracle_path(oc, which)
                both = sorted(set(abs(c) for c in p if c > 0) & set(abs(c) for c in p if c < 0))
                if both and long_at is None:
                    long_at = (u, both[len(both) // 2] - (oc["start"] - 1))
        assert long_at is not None

        def lengths(rng):
            lens = [rng.integers(1, 41, size=oc["end"] - oc["start"] + 1) for oc in records]
            lens[long_at[0]][long_at[1] - 1] = 2 * TILE + 37
            for u, l in hand.items():
                lens[u] = np.asarray(l)
            return lens
        chosen = None
        for seed in range(64):
            if covered(coverage(records, [[b"x" * int(n) for n in l] for l in lengths(np.random.default_rng(7000 + seed))], long_at)):
                chosen = seed
                break
        assert chosen is not None, "no seed of the search covers the cases: add hand-made units"
        rng = np.random.default_rng(7000 + chosen)
        seg_lists = [draw_segments(rng, l) for l in lengths(rng)]
        _MANY[workdir] = (items, records, seg_lists, long_at)
    return _MANY[workdir]


def many_batch(lib, items, seg_lists):
    graphs, b = [], api.Batch(lib)
    for (lh, sol, _), segs in zip(items, seg_lists):
        g = api.Graph(lib, lh); attach(g, segs); graphs.append(g)
        b.add_chromosome_sol(g, 0, sol)
    return graphs, b


def check_many_units(lib, oracle, workdir):
    items, records, seg_lists, long_at = many_sequences(oracle, workdir)
    assert any(oc["path_indel"] != oc["path"] for oc in records)
    cov = coverage(records, seg_lists, long_at)
    assert covered(cov), cov                                  # on the oracle's runs alone
    assert len(seg_lists[long_at[0]][long_at[1] - 1]) > 2 * TILE
    graphs, b = many_batch(lib, items, seg_lists)
    b.upload(); b.run(0); b.download()
    for u, oc in enumerate(records):
        assert b.unit_path(u, 0).tolist() == oc["path"] and b.unit_path(u, 1).tolist() == oc["path_indel"], u
    for which in (0, 1):
        b.sequence(which); b.sequence_wait()
        compare_units(b, [want_of(oc, which, segs) for oc, segs in zip(records, seg_lists)], ("many", which))
    pc.close_all(graphs, b)


# ---- case 4: unit ranges, the size limit, byte windows, bad arguments ----------------------------------------------------
def check_ranges_and_limit(lib, oracle, workdir):
    items, records, seg_lists, _ = many_sequences(oracle, workdir)
    U = len(items)
    full = [want_of(oc, 1, segs) for oc, segs in zip(records, seg_lists)]
    graphs, b = many_batch(lib, items, seg_lists)
    b.upload(); b.run(0); b.download()
    for first, n in ((0, U), (3, 1), (U - 1, 1), (5, 17)):
        b.sequence(1, first, n); b.sequence_wait()
        compare_units(b, full[first:first + n], ("range", first, n), first)
        for u in (first - 1, first + n):
            if 0 <= u < U:
                with pytest.raises(api.AmbiError):
                    b.unit_sequence_len(u)                     # outside the request
    # the limit: one byte short is refused with nothing assembled and the lengths readable; the exact total passes
    first, n = 5, 17
    total = sum(len(w) for w in full[first:first + n])
    with pytest.raises(api.AmbiError) as e:
        b.sequence(1, first, n, max_bytes=total - 1)
    assert e.value.code == ERR_TOO_LARGE
    assert [b.unit_sequence_len(u) for u in range(first, first + n)] == [len(w) for w in full[first:first + n]]
    for call in (b.sequence_wait, lambda: b.unit_sequence(first, 0, 1), b.sequence_device):
        with pytest.raises(api.AmbiError) as e:
            call()
        assert e.value.code == ERR_STATE
    b.sequence(1, first, n, max_bytes=total); b.sequence_wait()
    compare_units(b, full[first:first + n], ("limit", first, n), first)
    # byte windows of one unit: at the start, across a 16-byte boundary, the last byte, nothing
    u = first + 2
    w = full[u]
    assert len(w) > 48
    for lo, cnt in ((0, 5), (0, 16), (11, 10), (15, 2), (16, 16), (len(w) - 1, 1), (len(w) - 17, 17), (len(w), 0), (7, 0)):
        assert b.unit_sequence(u, lo, cnt) == w[lo:lo + cnt], (lo, cnt)
    for lo, cnt in ((-1, 2), (0, len(w) + 1), (len(w), 1), (3, -1)):
        with pytest.raises(api.AmbiError):
            b.unit_sequence(u, lo, cnt)
    # bad arguments
    for args in ((2, 0, 1), (-1, 0, 1), (1, -1, 2), (1, 0, 0), (1, 0, U + 1), (1, U, 1), (1, U - 1, 2)):
        with pytest.raises(api.AmbiError) as e:
            b.sequence(*args)
        assert e.value.code == ERR_ARG, args
    with pytest.raises(api.AmbiError):
        b.unit_sequence_len(U)
    pc.close_all(graphs, b)


def check_state_errors(lib):
    lh, sol = os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol")
    segs = draw_segments(np.random.default_rng(63), [4] * 6)
    g0 = api.Graph(lib, lh)                                    # no sequences attached
    g = api.Graph(lib, lh); attach(g, segs)
    for graph, ready in ((g0, False), (g, True)):
        b = api.Batch(lib)
        b.add_chromosome_sol(graph, 0, sol)
        for stage in ("added", "uploaded", "run"):
            if stage == "uploaded":
                b.upload()
            if stage == "run":
                b.run(0); b.download()
            if stage == "run" and ready:
                break
            for call in (lambda: b.sequence(1), b.sequence_wait, lambda: b.unit_sequence_len(0), lambda: b.unit_sequence(0, 0, 1)):
                with pytest.raises(api.AmbiError) as e:
                    call()
                assert e.value.code == ERR_STATE, (ready, stage)
        if ready:
            b.sequence(1); b.sequence_wait()
            assert b.unit_sequence_len(0) == 32 * 4
            b.run(0)
            with pytest.raises(api.AmbiError) as e:
                b.unit_sequence(0, 0, 1)
            assert e.value.code == ERR_STATE                   # a new run: the old sequences are gone
            b.wait()
        b.close()
    # a unit added raw takes its bases from set_unit_sequences: same result as through the graph
    s0, e0 = g.chromosome(0)
    b = api.Batch(lib)
    b.add_chromosome_sol(g0, 0, sol)
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    b.set_unit_sequences(0, b"".join(segs), off)
    b2 = api.Batch(lib)
    b2.add_chromosome_sol(g, 0, sol)
    outs = []
    for x in (b, b2):
        x.upload(); x.run(0); x.download(); x.sequence(1); x.sequence_wait()
        outs.append(x.unit_sequence(0))
        x.close()
    assert outs[0] == outs[1] and len(outs[0]) == 32 * 4
    g.close(); g0.close()


# ---- case 5: two runs of one batch; the unit finished at wait() -----------------------------------------------------------
def check_two_runs(lib, oracle, workdir):
    """Plain, then reversed: the sequences of a run are those of ITS paths (a stale block, a stale epoch)."""
    items, records, seg_lists, _ = many_sequences(oracle, workdir)
    rev = [oracle.run_bfb(lh, [sol], reversed_=True)["chr"][0] for lh, sol, _ in items]
    assert any(a["path_indel"] != r["path_indel"] for a, r in zip(records, rev))
    graphs, b = many_batch(lib, items, seg_lists)
    b.upload()
    for flags, recs in ((0, records), (api.FLAG_REVERSED, rev), (0, records)):
        b.run(flags); b.download()
        for u, oc in enumerate(recs):
            assert b.unit_path(u, 1).tolist() == oc["path_indel"], (flags, u)
        for which in (1, 0):
            b.sequence(which); b.sequence_wait()
            compare_units(b, [want_of(oc, which, segs) for oc, segs in zip(recs, seg_lists)], ("two runs", flags, which))
    pc.close_all(graphs, b)


def check_big_unit_finished_at_wait(lib, oracle, workdir):
    lh, sol, R, rev = pc.big_unit(oracle, workdir)
    items, _, seg_lists, _ = many_sequences(oracle, workdir)
    items, seg_lists = items[:39], seg_lists[:39]
    big_segs = draw_segments(np.random.default_rng(64), np.random.default_rng(65).integers(1, 17, size=256))
    graphs, b = [], api.Batch(lib)
    b.configure(first_budget=4)
    g = api.Graph(lib, lh); attach(g, big_segs); graphs.append(g)
    b.add_chromosome_sol(g, 0, sol)
    for (l2, s2, _), segs in zip(items, seg_lists):
        g = api.Graph(lib, l2); attach(g, segs); graphs.append(g)
        b.add_chromosome_sol(g, 0, s2)
    b.debug_inject_validity(0, [0] * R + [1] * R)
    records = [rev] + [oc for _, _, oc in items]
    all_segs = [big_segs] + list(seg_lists)
    b.upload()
    for which in (1, 0):
        b.run(0)
        b.sequence(which)                # queued behind a run whose unit 0 is still PENDING
        b.wait()                         # the parallel search finishes it
        b.sequence_wait()                # ... and the sequences are those of the final results
        b.download()
        r = b.unit_result(0)
        assert (r["status"], r["first_valid"], r["first_forward"]) == (0, 0, 0), r
        assert b.unit_path(0, 0).tolist() == rev["path"] and b.unit_path(0, 1).tolist() == rev["path_indel"]     # precondition
        compare_units(b, [want_of(oc, which, segs) for oc, segs in zip(records, all_segs)], ("big", which))
    assert b.unit_sequence_len(0) > 8 * TILE
    pc.close_all(graphs, b)


# ---- case 5b: the queueing path's other branches ---------------------------------------------------------------------------
def check_request_paths(lib, oracle, workdir, run_stream=None, req_stream=None):
    """A request on another stream than the run's (run_stream / req_stream: raw stream handles; None on the host simulation), two
    requests over different unit ranges with one wait, and a batch closed with a request in flight whose lease the next batch
    takes over."""
    items, records, seg_lists, _ = many_sequences(oracle, workdir)
    U = len(items)
    full = {which: [want_of(oc, which, segs) for oc, segs in zip(records, seg_lists)] for which in (0, 1)}
    graphs, b = many_batch(lib, items, seg_lists)
    b.upload()
    # (1) run on one stream, request on another, nothing waited for in between
    for which in (0, 1):
        b.run(0, run_stream)
        b.sequence(which, stream=req_stream); b.sequence_wait()
        compare_units(b, full[which], ("other stream", which))
    # (2) a request nobody waited for, then another over other units: the second range answers; the same after another run
    for k in range(2):
        b.run(0, run_stream)
        b.sequence(1, 0, 9, stream=req_stream); b.sequence(1, 5, 17, stream=req_stream); b.sequence_wait()
        compare_units(b, full[1][5:22], ("unwaited", k), 5)
        for u in (0, 4, 22, U - 1):
            with pytest.raises(api.AmbiError) as e:
                b.unit_sequence_len(u)                         # outside the second request (0 and 4 were inside the first)
            assert e.value.code == ERR_ARG, u
    # (3) closed with a request in flight; the next batch (other units, another image) gets the lease back
    b.run(0, run_stream)
    b.sequence(1, stream=req_stream)
    pc.close_all(graphs, b)
    graphs, b = many_batch(lib, items[3:20], seg_lists[3:20])
    b.upload(); b.run(0, run_stream)
    for which in (0, 1):
        b.sequence(which); b.sequence_wait()
        compare_units(b, full[which][3:20], ("after a close in flight", which))
    pc.close_all(graphs, b)


def check_three_requests_in_flight(lib, oracle, workdir, run_stream=None, req_stream=None):
    """Both profiles and a sequence request queued back to back, waited for in the opposite order: each answers for itself."""
    import junc_profile_checks as jc
    items, records, seg_lists, _ = many_sequences(oracle, workdir)
    graphs, b = many_batch(lib, items, seg_lists)
    b.upload()
    for which in (1, 0):
        b.run(0, run_stream)
        b.profile(which, req_stream); b.junc_profile(which, req_stream); b.sequence(which, 5, 17, stream=req_stream)
        b.sequence_wait(); b.junc_profile_wait(); b.profile_wait()
        b.download()
        for u, ((lh, _, oc), g) in enumerate(zip(items, graphs)):
            n, want = pc.unit_expectation(b, u, oc, which)
            pc.compare_unit(b, u, n, want, ("three", which, u))
            idx, count, summary, _ = jc.unit_expectation(lh, g, oc, which)
            jc.compare_unit(b, u, idx, count, summary, ("three", which, u))
        compare_units(b, [want_of(oc, which, segs) for oc, segs in zip(records[5:22], seg_lists[5:22])], ("three", which), 5)
    pc.close_all(graphs, b)


# ---- case 6: sharded ------------------------------------------------------------------------------------------------------
def check_sharded(lib, oracle, workdir, devices):
    items, records, seg_lists, _ = many_sequences(oracle, workdir)
    full = [want_of(oc, 1, segs) for oc, segs in zip(records, seg_lists)]
    graphs, b = many_batch(lib, items, seg_lists)
    b.run_sharded(0, devices=devices)
    for which in (0, 1):
        b.sequence(which); b.sequence_wait()
        compare_units(b, [want_of(oc, which, segs) for oc, segs in zip(records, seg_lists)], ("sharded", which))
    b.sequence(1, 5, 17); b.sequence_wait()
    compare_units(b, full[5:22], ("sharded range",), 5)
    with pytest.raises(api.AmbiError) as e:
        b.sequence(1, 5, 17, max_bytes=sum(len(w) for w in full[5:22]) - 1)
    assert e.value.code == ERR_TOO_LARGE
    assert [b.unit_sequence_len(u) for u in range(5, 22)] == [len(w) for w in full[5:22]]
    with pytest.raises(api.AmbiError):
        b.sequence_device()              # one block per share: no single device view
    pc.close_all(graphs, b)


def check_partial_bases(lib, oracle, devices=None):
    """Bases on only some units (set_unit_sequences on units 1 and 3 of four): the others have length 0, unsharded and, with
    `devices`, when a whole share holds none."""
    lh, sol = os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol")
    oc = oracle.run_bfb(lh, [sol])["chr"][0]
    rng = np.random.default_rng(69)
    g = api.Graph(lib, lh)
    b = api.Batch(lib)
    wants = []
    for u in range(4):
        b.add_chromosome_sol(g, 0, sol)
        if u % 2:
            segs = draw_segments(rng, [3, 17, 1, 8, 16, 5])
            b.set_unit_sequences(u, b"".join(segs), np.concatenate([[0], np.cumsum([len(x) for x in segs])]))
            wants.append(want_of(oc, 1, segs))
        else:
            wants.append(b"")
    if devices is None:
        b.upload(); b.run(0); b.download()
    else:
        b.run_sharded(0, devices=devices)
    b.sequence(1); b.sequence_wait()
    compare_units(b, wants, ("partial", devices))
    assert len(wants[1]) > 0 and len(wants[3]) > 0
    b.close(); g.close()


# ---- case 8: the FASTA reader -----------------------------------------------------------------------------------------------
FASTA_LH = ("SAMPLE_NAME fa\nAVG_CHR_SEG_DP 30\nAVG_WHOLE_HOST_DP 30\nAVG_JUNC_DP 30\nPURITY 1\nAVG_TUMOR_PLOIDY 2\n"
            "PLOIDY 2m1\nVIRUS_START 9\nSOURCE 1,5\nSINK 4,8\n"
            "%s"
            "JUNC H:1:+ H:2:+ 30.0 1.0 U B\nJUNC H:5:+ H:6:+ 30.0 1.0 U B\n")


def fasta_case(workdir, tag, segs=None):
    """A three-record file (line widths 60 / 7 / irregular; CRLF in the second record; lower case; no final newline) and a .lh whose
    segments start or end on line breaks and at a record's end.  Returns (lh, fasta, records: name -> bytes, segments)."""
    rng = np.random.default_rng(66)
    letters = np.frombuffer(b"ACGTNacgtnRYKMryk", np.uint8)
    rec = {"chrA": bytes(rng.choice(letters, 200)), "other": bytes(rng.choice(letters, 33)), "chrB": bytes(rng.choice(letters, 97))}
    def wrap(s, widths, eol):
        out, at, k = [], 0, 0
        while at < len(s):
            w = widths[k % len(widths)]; k += 1
            out.append(s[at:at + w]); at += w
        return eol.join(out)
    text = (b">chrA first record\n" + wrap(rec["chrA"], [60], b"\n") + b"\n"
            + b">other\tignored words\r\n" + wrap(rec["other"], [7], b"\r\n") + b"\r\n"
            + b">chrB\n" + wrap(rec["chrB"], [1, 13, 2, 40, 5], b"\n"))                     # no final newline
    fa = os.path.join(workdir, "seq_%s.fa" % tag)
    with open(fa, "wb") as f:
        f.write(text)
    if segs is None:
        # chrA: a segment ending on a line break (60), one starting on it, one across two breaks, one ending at the record's end
        # chrB: irregular lines; starts at 0, the single-base line, an empty segment, the record's last byte
        segs = [("chrA", 0, 60), ("chrA", 60, 61), ("chrA", 61, 181), ("chrA", 181, 200),
                ("chrB", 0, 1), ("chrB", 1, 14), ("chrB", 14, 14), ("chrB", 14, 97)]
    lines = "".join("SEG H:%d:%s:%d:%d 30.0 1.0\n" % (i + 1, c, s, e) for i, (c, s, e) in enumerate(segs))
    lh = os.path.join(workdir, "seq_%s.lh" % tag)
    with open(lh, "w") as f:
        f.write(FASTA_LH % lines)
    return lh, fa, rec, segs


def check_fasta_reader(lib, workdir):
    lh, fa, rec, segs = fasta_case(workdir, "ok")
    g = api.Graph(lib, lh)
    with pytest.raises(api.AmbiError) as e:
        g.sequences()
    assert e.value.code == ERR_STATE
    g.read_fasta(fa)
    bases, off = g.sequences()
    want = [rec[c][s:e] for c, s, e in segs]
    assert [bases[off[i]:off[i + 1]] for i in range(len(segs))] == want
    assert off[0] == 0 and off[-1] == len(bases) == sum(len(w) for w in want)
    # the same store through set_sequences
    g2 = api.Graph(lib, lh)
    attach(g2, want)
    b2, off2 = g2.sequences()
    assert b2 == bases and off2.tolist() == off.tolist()
    # the errors, each with its own code, the store untouched
    with pytest.raises(api.AmbiError) as e:
        g.read_fasta(os.path.join(workdir, "no_such.fa"))
    assert e.value.code == -40
    for tag, bad, code in (("chrom", ("chrC", 0, 5), -41), ("range", ("chrB", 90, 98), -42), ("order", ("chrA", 20, 19), -43),
                           ("range2", ("other", 0, 34), -42)):
        s2 = list(segs); s2[5] = bad
        lh_bad, fa_bad, _, _ = fasta_case(workdir, tag, s2)
        gb = api.Graph(lib, lh_bad)
        with pytest.raises(api.AmbiError) as e:
            gb.read_fasta(fa_bad)
        assert e.value.code == code, tag
        with pytest.raises(api.AmbiError):
            gb.sequences()
        gb.close()
    assert g.sequences()[0] == bases
    with pytest.raises(api.AmbiError):
        g2.set_sequences(b"ACGT", [0, 2, 1, 4, 4, 4, 4, 4, 4])       # offsets not ascending
    g.close(); g2.close()


# ---- case 9: the CLI ----------------------------------------------------------------------------------------------------------
def readme_fasta(path, rng):
    """A FASTA with the record chr7 of readme6.lh: 'N' up to the segments, seeded bases over them, lines of 60."""
    n = 55287000
    n += -n % 60
    seq = np.full(n, ord("N"), np.uint8)
    seq[55281000:55287000] = rng.choice(np.frombuffer(b"ACGTacgtNRY", np.uint8), 6000)
    lines = np.empty((n // 60, 61), np.uint8)
    lines[:, :60] = seq.reshape(-1, 60)
    lines[:, 60] = 10
    with open(path, "wb") as f:
        f.write(b">chr7 test\n")
        f.write(lines.tobytes())
        f.write(b">chrUn\nACGT\n")
    return seq


def check_cli(lib, exe, cwd, oracle):
    import test_cli_dropin as t
    lh, sol = os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol")
    fa = os.path.join(cwd, "ref.fa")
    seq = readme_fasta(fa, np.random.default_rng(67))
    outs = []
    for k, extra in enumerate(([], ["--ref_fasta", fa, "--out_fasta", "path.fa"], ["--ref_fasta", fa, "--out_fasta", "path.fa", "--fasta_chunk_bytes", "100"])):
        sub = os.path.join(cwd, "run%d" % k)
        os.makedirs(sub)
        bindir = os.path.join(sub, "bin")
        t.fake_cbc(bindir, [sol])
        r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", lh, "--lp_prefix", "readme", *extra)
        assert r.returncode == 0, r.stderr
        outs.append((r.stdout, r.stderr, sorted(x for x in os.listdir(sub) if x != "bin")))
    assert outs[0][:2] == outs[1][:2] == outs[2][:2]                        # stdout, stderr: byte for byte without the switches
    assert outs[1][2] == sorted(outs[0][2] + ["path.fa"])
    segs = []
    for l in open(lh):
        if l.startswith("SEG "):
            _, sid, chrom, start, end = l.split()[1].split(":")
            segs.append(bytes(seq[int(start):int(end)]))                     # 0-based, half-open
    assert [len(s) for s in segs] == [999] * 6
    oc = oracle.run_bfb(lh, [sol])["chr"][0]
    want = b">BFBPATH\n" + expected_seq(oc["path_indel"], 0, segs) + b"\n"
    for k in (1, 2):
        assert open(os.path.join(cwd, "run%d" % k, "path.fa"), "rb").read() == want
    # a PROP I2 sample: its printed paths are rebuilt on the host -- refused, exit status 2, no file
    sub = os.path.join(cwd, "i2")
    os.makedirs(sub)
    bindir = os.path.join(sub, "bin")
    t.fake_cbc(bindir, [os.path.join(cases.DATA, "readme_i2_chr0.sol"), os.path.join(cases.DATA, "readme_i2_chr1.sol")])
    r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", os.path.join(cases.DATA, "readme_i2.lh"), "--lp_prefix", "i2", "--ref_fasta", fa, "--out_fasta", "path.fa")
    assert r.returncode == 2 and "--out_fasta" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(os.path.join(sub, "path.fa"))
    r = t.run_cli(exe, sub, bindir, "--op", "sc_bfb", "--in_lh", lh, "--lp_prefix", "sc", "--ref_fasta", fa, "--out_fasta", "path.fa")
    assert r.returncode != 0 and "--op bfb only" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(os.path.join(sub, "path.fa"))
    r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", lh, "--lp_prefix", "x", "--out_fasta", "path.fa")
    assert r.returncode == 2 and "go together" in r.stderr
    r = t.run_cli(exe, sub, bindir, "--help")
    assert "--out_fasta" in r.stdout and "--ref_fasta" in r.stdout
    # three samples in one batch and a budget that holds two of their sequences: chunks of two units and of one
    sub = os.path.join(cwd, "three")
    os.makedirs(sub)
    bindir = os.path.join(sub, "bin")
    one = len(want) - len(b">BFBPATH\n") - 1
    outs3 = []
    for extra in ([], ["--ref_fasta", fa, "--out_fasta", "path.fa", "--fasta_chunk_bytes", str(2 * one + 5)]):
        t.fake_cbc(bindir, [sol, sol, sol])
        r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", ",".join([lh] * 3), "--lp_prefix", "three", *extra)
        assert r.returncode == 0, r.stderr
        outs3.append((r.stdout, r.stderr))
    assert outs3[0] == outs3[1]
    assert open(os.path.join(sub, "path.fa"), "rb").read() == want * 3
