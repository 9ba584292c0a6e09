"""Checks of the path coordinates (ambi_batch_path_coords, csrc/ambi_path_coords.hpp) shared by the CPU host-simulation tests and the GPU
tests (same assertions, different library).

Expected values never come from the stage under test: the plane is numpy's cumsum of the lengths of the ORACLE's cells, a lift is
searchsorted(plane, pos, side="right") - 1 -- the LAST cell whose offset is <= pos, which of cells with equal offsets is the one that
holds the base -- and everything else is arithmetic on those.  Every compared field is an exact integer: there are no tolerances."""
import os
import random

import numpy as np

import cases
import fold_profile_checks as fp
import junc_profile_checks as jc
import profile_checks as pc
import sequence_checks as sc
from ambigram_amd import api, synth

_raises = fp._raises
ERR_UNSUPPORTED, ERR_BAD_INPUT, ERR_STATE, ERR_ARG = -9, -17, -32, -33
ROUND = 512                                             # cells per round of the scan: 256 threads, two cells each
LENGTHS = (0, 1, 2, 3, 1000, 2 ** 31 - 1)
SUMMARY = ("status", "cells", "runs", "empty_cells", "bp_len", "bp_minus")
RESULT = ("status", "cell", "seg", "reserved", "seg_off", "cell_start")
ROUND_SEED = 0                                          # synth.make_sample(24, 40, "chain", 9, seed=0): a path of exactly 512 cells (check_floors searches again)
_UNITS = {}


# ---- the units ---------------------------------------------------------------------------------------------------------------
def round_sample(seed):
    return synth.make_sample(24, 40, ("chain", "wide", "mixed")[seed % 3], 9 + seed % 5, seed=seed, name="coords%d" % seed)


def units(oracle, workdir):
    """The units of the fold profile's checks (readme6, six synthetic units, three random decompositions, a SHORTCUT unit, a unit
    with status -11 and no path) and the pinned unit whose path is exactly one round long."""
    if workdir not in _UNITS:
        lh, sols = round_sample(ROUND_SEED).write(workdir)
        rec = [oracle.run_bfb(lh, sols, reversed_=r)["chr"][0] for r in (False, True)]
        _UNITS[workdir] = fp.units(oracle, workdir) + [("round", lh, sols[0], rec[0], rec[1])]
    return _UNITS[workdir]


def path_of(item, which, reversed_=False):
    """(path in local ids or [], status) of a unit as the engine must see it."""
    name, _, _, oc, orev = item
    o = orev if reversed_ else oc
    st = fp.unit_status(name, o)
    return (jc.oracle_path(o, which) if st >= 0 else []), st


def n_seg(item):
    return item[3]["end"] - item[3]["start"] + 1


# ---- expected values -----------------------------------------------------------------------------------------------------------
def model(path, lens, status):
    """(plane int64[P + 1], summary dict) of a path in local ids over segments of the lengths `lens`."""
    c = np.asarray(path, np.int64)
    l = np.asarray(lens, np.int64)[np.abs(c) - 1] if len(c) else np.zeros(0, np.int64)
    plane = np.concatenate([np.zeros(1, np.int64), np.cumsum(l, dtype=np.int64)])
    runs = int(1 + np.count_nonzero(c[1:] != c[:-1] + 1)) if len(c) else 0
    st = status if len(c) or status < 0 else ERR_BAD_INPUT
    return plane, dict(status=st, cells=len(c), runs=runs, empty_cells=int(np.count_nonzero(l == 0)), bp_len=int(plane[-1]), bp_minus=int(l[c < 0].sum()))


def lifts(plane, path, lens, status, pos):
    """The expected answers (LIFT_DTYPE) to the positions `pos` of one unit."""
    pos = np.asarray(pos, np.int64)
    out = np.zeros(len(pos), api.LIFT_DTYPE)
    out["status"] = status if status < 0 else 0
    out["cell"], out["seg_off"], out["cell_start"] = -1, -1, -1
    ok = (pos >= 0) & (pos < plane[-1]) if status >= 0 else np.zeros(len(pos), bool)
    k = np.searchsorted(plane, pos[ok], side="right") - 1
    c = np.asarray(path, np.int64)[k]
    j = pos[ok] - plane[k]
    l = np.asarray(lens, np.int64)[np.abs(c) - 1]
    assert np.all((j >= 0) & (j < l))                   # (of the model itself: the cell holds the base)
    out["cell"][ok], out["seg"][ok], out["cell_start"][ok] = k, c, plane[k]
    out["seg_off"][ok] = np.where(c > 0, j, l - 1 - j)
    return out


def positions(plane, rng, cap=4096):
    """plane[k], plane[k] - 1 and a middle position of every cell (of `cap` sampled cells on a longer path), and the ends."""
    P = len(plane) - 1
    ks = np.arange(P) if P <= cap else np.sort(rng.choice(P, cap, replace=False))
    bp = int(plane[-1])
    ends = [-1, 0, bp - 1, bp, 2 ** 62]
    return np.concatenate([plane[ks], plane[ks] - 1, (plane[ks] + plane[ks + 1]) // 2, np.asarray(ends, np.int64)]).astype(np.int64)


def draw_lengths(items, seed):
    """Per unit n_seg lengths from LENGTHS; the segment of the first unit's first cell and of the second unit's last cell are 0, so
    that zero-length cells stand at the front and at the end of a path whatever the seed."""
    rng = np.random.default_rng(seed)
    out = [rng.choice(np.asarray(LENGTHS, np.int64), n_seg(it)) for it in items]
    for u, at in ((1, 0), (2, -1)):
        p, _ = path_of(items[u], 1)
        out[u][abs(p[at]) - 1] = 0
    return out


def check_model_floors(items, lens, which, reversed_=False):
    """What the drawn lengths must offer: an amplicon above 2^32 (a 32-bit carry would wrap), zero-length cells at the front, in the
    middle and at the end of a path that has bases."""
    big = front = mid = end = 0
    for it, l in zip(items, lens):
        p, st = path_of(it, which, reversed_)
        plane, s = model(p, l, st)
        if s["bp_len"] == 0:
            continue
        big += s["bp_len"] > 2 ** 32
        front += plane[1] == 0
        end += plane[-1] == plane[-2]
        inner = plane[1:-1]
        mid += bool(np.any((inner[1:] == inner[:-1]) & (inner[1:] > 0) & (inner[1:] < plane[-1])))
    assert big >= 1 and front >= 1 and mid >= 1 and end >= 1, (big, front, mid, end)


# ---- one request against the model ---------------------------------------------------------------------------------------------
def compare_summaries(b, items, lens, which, tag, reversed_=False):
    got = b.path_coords_summaries()
    assert got.dtype == api.UNIT_COORDS_DTYPE and got.dtype.itemsize == 32 and len(got) == len(items)
    planes = []
    for u, (it, l) in enumerate(zip(items, lens)):
        p, st = path_of(it, which, reversed_)
        plane, want = model(p, l, st)
        have = {k: int(got[u][k]) for k in SUMMARY}
        assert have == want, (tag, it[0], which, have, want)
        planes.append((plane, p, st))
    return planes


def request(b, items, lens, which, queries, tag, stream=None, reversed_=False, planes_too=True):
    """Queues the scan and the queries ([(unit, positions)]), waits, compares every summary, every plane and every answer."""
    q = np.concatenate([api.lift_queries(u, pos) for u, pos in queries]) if queries else None
    b.path_coords(which, q, stream); b.path_coords_wait()
    planes = compare_summaries(b, items, lens, which, tag, reversed_)
    if planes_too:
        for u, (plane, p, st) in enumerate(planes):
            P = len(p)
            assert b.path_coords_copy(u).tolist() == plane.tolist(), (tag, items[u][0], which)      # 0 .. P, plane[P] included
            for first, n in ((P, 1), (0, 0), (P + 1, 0), (P // 3, P - P // 3 - P // 5), (1, min(P, 3)), (max(P - 2, 0), min(P, 2))):   # ranges that start and end mid-slice
                assert b.path_coords_copy(u, first, n).tolist() == plane[first:first + n].tolist(), (tag, items[u][0], first, n)
    got = b.path_coords_results()
    assert got.dtype == api.LIFT_DTYPE and got.dtype.itemsize == 32 and len(got) == (0 if q is None else len(q))
    at = 0
    for u, pos in queries:
        plane, p, st = planes[u]
        want = lifts(plane, p, lens[u], model(p, lens[u], st)[1]["status"], pos)
        have = got[at:at + len(pos)]
        for k in RESULT:
            bad = np.flatnonzero(have[k] != want[k])
            assert len(bad) == 0, (tag, items[u][0], which, k, int(np.asarray(pos)[bad[0]]), have[bad[0]], want[bad[0]])
        at += len(pos)
    return got


class lift_grid:
    """AMBI_LIFT_GRID for the requests inside: the workgroups of the lift kernel (it can only shrink them)."""
    def __init__(self, grid):
        self.grid = grid

    def __enter__(self):
        self.saved = os.environ.pop("AMBI_LIFT_GRID", None)
        if self.grid:
            os.environ["AMBI_LIFT_GRID"] = str(self.grid)

    def __exit__(self, *exc):
        os.environ.pop("AMBI_LIFT_GRID", None)
        if self.saved is not None:
            os.environ["AMBI_LIFT_GRID"] = self.saved


# ---- floors: what the units must offer for the scan to be exercised (CPU half, from the oracle's paths alone) ------------------
def check_floors(oracle, workdir):
    items = units(oracle, workdir)
    lengths, minus, nopath = set(), 0, 0
    for it in items:
        for which in (0, 1):
            p, st = path_of(it, which)
            nopath += not p
            if p:
                lengths.add(len(p)); minus += any(c < 0 for c in p)
    assert nopath >= 1, "a unit without a path"
    assert min(lengths) <= 4, min(lengths)              # the shortest path on offer: the SHORTCUT unit's 1+2+3+4+ (no unit has one cell)
    assert any(P < ROUND for P in lengths) and any(P >= 2 * ROUND + 1 for P in lengths), sorted(lengths)
    assert any(P % 2 for P in lengths) and any(P % 2 == 0 for P in lengths), sorted(lengths)
    assert minus >= 1, "a path with '-' cells"
    assert any(P % ROUND == 0 for P in lengths), sorted(lengths)       # the pinned seed: P an exact multiple of the round
    # the search that pinned it: the first seed of small units whose path is a whole number of rounds
    found = None
    for seed in range(4000):
        lh, sols = round_sample(seed).write(os.path.join(workdir, "coords_search"))
        P = len(oracle.run_bfb(lh, sols)["chr"][0]["path_indel"])
        if P and P % ROUND == 0:
            found = seed
            break
    assert found == ROUND_SEED, found
    lens = draw_lengths(items, 5)
    for which in (0, 1):
        check_model_floors(items, lens, which)


# ---- the small units: every path, lengths from LENGTHS ---------------------------------------------------------------------------
def check_small(lib, oracle, workdir, grid=None, run_stream=None, req_stream=None):
    """All units in one batch, lengths set per unit; both `which`; per unit every cell's first base, the base in front of it and a
    middle base, and the ends; then a failed unit alone, no query, one query.  With `grid`, the lift kernel has that many workgroups:
    more queries than one has threads."""
    items = units(oracle, workdir)
    lens = draw_lengths(items, 5)
    graphs, b, _ = fp.make_batch(lib, items)
    for u, l in enumerate(lens):
        b.set_unit_seg_lengths(u, l)
    b.upload(); b.run(0, run_stream)
    rng = np.random.default_rng(9)
    failed = [u for u, it in enumerate(items) if path_of(it, 1)[1] < 0]
    assert failed
    with lift_grid(grid):
        for which in (0, 1):
            check_model_floors(items, lens, which)
            queries = []
            for u, (it, l) in enumerate(zip(items, lens)):
                p, st = path_of(it, which)
                queries.append((u, positions(model(p, l, st)[0], rng)))
            assert sum(len(pos) for _, pos in queries) > 256
            got = request(b, items, lens, which, queries, ("small", grid), req_stream)
            assert int(got["cell"].max()) >= 2 * ROUND and np.count_nonzero(got["seg"] < 0) > 0
        got = request(b, items, lens, 1, [(failed[0], np.asarray([0, 1, -1], np.int64))], "failed unit", req_stream, planes_too=False)
        assert got["status"].tolist() == [-11] * 3
        request(b, items, lens, 0, [], "no query", req_stream, planes_too=False)
        request(b, items, lens, 1, [(3, np.asarray([7], np.int64))], "one query", req_stream, planes_too=False)
        request(b, items, lens, 1, [(u, np.asarray([0], np.int64)) for u in reversed(range(len(items)))], "units in falling order", req_stream, planes_too=False)
    # a second set of lengths replaces the first; the next request sees it
    lens2 = [np.ones(n_seg(it), np.int64) for it in items]
    b.set_unit_seg_lengths(4, lens2[4]); lens[4] = lens2[4]
    with _raises(ERR_STATE):
        b.path_coords_results()                            # new lengths: the old answers are gone
    request(b, items, lens, 1, [(4, np.arange(-1, len(path_of(items[4], 1)[0]) + 1, dtype=np.int64))], "replaced lengths", req_stream, planes_too=False)
    if run_stream is not None:
        b.wait()
    pc.close_all(graphs, b)


# ---- one convention with the sequence kind -------------------------------------------------------------------------------------
def check_against_sequence(lib, oracle, workdir):
    """Graph-built units with the sequence tests' FASTA fixtures, lengths left to the graph (end - start): byte p of
    ambi_batch_sequence is ref[seg_start + seg_off], complemented on '-'."""
    lh, sol = os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol")
    fa = os.path.join(workdir, "coords_readme.fa")
    ref = sc.readme_fasta(fa, np.random.default_rng(3))
    flh, ffa, rec, segs = sc.fasta_case(workdir, "coords")
    rng = np.random.default_rng(4)
    minus = 0
    for lh_, fa_, sols, refs in ((lh, fa, [sol], {"chr7": ref.tobytes()}), (flh, ffa, [None, None], rec)):
        g = api.Graph(lib, lh_)
        g.read_fasta(fa_)
        b = api.Batch(lib)
        for c, s in enumerate(sols):
            if s:
                b.add_chromosome_sol(g, c, s)
            else:
                b.add_chromosome(g, c, [], [])
        b.upload(); b.run(0)
        seg = g.segments()
        for which in (0, 1):
            b.sequence(which); b.sequence_wait()
            b.path_coords(which); b.path_coords_wait()
            summ = b.path_coords_summaries()
            queries = []
            for u in range(len(sols)):
                n = int(summ[u]["bp_len"])
                assert n == b.unit_sequence_len(u) and n > 0
                queries.append((u, np.unique(np.concatenate([rng.integers(0, n, 300), [0, n - 1]])).astype(np.int64)))
            b.path_coords(which, np.concatenate([api.lift_queries(u, pos) for u, pos in queries])); b.path_coords_wait()
            got = b.path_coords_results()
            where = api.lift_to_genome(g, 0, got[:len(queries[0][1])])
            at = 0
            for u, pos in queries:
                seq = b.unit_sequence(u)
                first, _ = g.chromosome(u)
                for i, p in enumerate(pos.tolist()):
                    r = got[at + i]
                    c = int(r["seg"])
                    sid = first - 1 + abs(c)
                    base = refs[g.chrom_name(sid)][int(seg["start"][sid - 1]) + int(r["seg_off"])]
                    want = bytes([base]) if c > 0 else bytes([base]).translate(sc.COMP)
                    assert seq[p:p + 1] == want, (lh_, which, u, p, r)
                    minus += c < 0
                    if u == 0:
                        assert where[i] == (g.chrom_name(sid), int(seg["start"][sid - 1]) + int(r["seg_off"]), "+" if c > 0 else "-", sid)
                at += len(pos)
        b.close(); g.close()
    assert minus > 100


# ---- two runs, and a run between request and wait ------------------------------------------------------------------------------
def check_two_runs(lib, oracle, workdir, run_stream=None, req_stream=None, before_run=None):
    """Run, request, run again with the other orientation, request with the same queries: the answers are those of the new paths.
    Then a request whose wait follows a run in between: the results' epoch moves, the engine queues the request again at the wait with
    the request's own copy of the queries (the caller's array is overwritten in between), and the answers are the last run's.
    before_run: called in front of the run in between (a request on another stream than the run's reads the results that run writes:
    its kernels are let finish first)."""
    items = units(oracle, workdir)
    lens = draw_lengths(items, 6)
    graphs, b, _ = fp.make_batch(lib, items)
    for u, l in enumerate(lens):
        b.set_unit_seg_lengths(u, l)
    b.upload()
    differ = sum(path_of(it, 1)[0] != path_of(it, 1, True)[0] for it in items)
    assert differ >= 3, differ                          # the two orientations give other paths
    rng = np.random.default_rng(12)
    queries = [(u, positions(model(path_of(it, 1)[0], l, path_of(it, 1)[1])[0], rng, cap=64)) for u, (it, l) in enumerate(zip(items, lens))]
    for reversed_ in (False, True, False):
        b.run(api.FLAG_REVERSED if reversed_ else 0, run_stream)
        request(b, items, lens, 1, queries, ("two runs", reversed_), req_stream, reversed_)
    # the run in between
    q = np.concatenate([api.lift_queries(u, pos) for u, pos in queries])
    b.path_coords(1, q, req_stream)                        # nobody waits for it yet
    q["unit"], q["pos"] = 0, -5                            # the request owns a copy
    if before_run:
        before_run()
    b.run(api.FLAG_REVERSED, run_stream)
    b.path_coords_wait()
    planes = compare_summaries(b, items, lens, 1, "run in between", True)
    got = b.path_coords_results()
    at = 0
    for u, pos in queries:
        plane, p, st = planes[u]
        want = lifts(plane, p, lens[u], model(p, lens[u], st)[1]["status"], pos)
        assert got[at:at + len(pos)].tobytes() == want.tobytes(), ("run in between", items[u][0])
        assert b.path_coords_copy(u).tolist() == plane.tolist()
        at += len(pos)
    b.path_coords(0, None, req_stream)                     # closed with a request in flight
    pc.close_all(graphs, b)


# ---- device view ---------------------------------------------------------------------------------------------------------------
def check_device_view(lib, oracle, workdir):
    """The block and the plane in device memory, read back through torch, are what the host getters return."""
    import torch
    from ambigram_amd.dist import _DevBytes
    items = units(oracle, workdir)
    lens = draw_lengths(items, 7)
    graphs, b, _ = fp.make_batch(lib, items)
    for u, l in enumerate(lens):
        b.set_unit_seg_lengths(u, l)
    stream = torch.cuda.Stream()
    b.upload(); b.run(0, stream.cuda_stream)
    q = np.concatenate([api.lift_queries(u, [0, 5, 2 ** 40]) for u in range(len(items))])
    b.path_coords(1, q, stream.cuda_stream); b.path_coords_wait()
    ptr, nbytes, roff = b.path_coords_device()
    assert ptr and roff == 32 * len(items) and nbytes == roff + 32 * len(q)
    raw = torch.as_tensor(_DevBytes(ptr, nbytes), device="cuda").cpu().numpy().tobytes()
    assert raw[:roff] == b.path_coords_summaries().tobytes() and raw[roff:] == b.path_coords_results().tobytes()
    pptr, pbytes, off = b.path_coords_plane_device()
    assert pptr and np.all(off % 16 == 0) and np.all(np.diff(off) > 0) and pbytes > off[-1]
    area = torch.as_tensor(_DevBytes(pptr, pbytes), device="cuda").cpu().numpy()
    for u, it in enumerate(items):
        plane = b.path_coords_copy(u)
        assert area[off[u]:off[u] + 8 * len(plane)].tobytes() == plane.tobytes(), it[0]
        assert plane.tolist() == model(path_of(it, 1)[0], lens[u], path_of(it, 1)[1])[0].tolist()
    pc.close_all(graphs, b)


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def check_cli(lib, exe, cwd, oracle, workdir):
    import test_cli_dropin as t
    items = fp.units(oracle, workdir)
    (_, readme, rsol, roc, _), (_, lh2, sol2, oc2, _) = items[0], items[1]

    def run(name, lhs, sols, *extra):
        sub = os.path.join(cwd, name)
        os.makedirs(sub)
        bindir = os.path.join(sub, "bin")
        t.fake_cbc(bindir, sols)
        r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", ",".join(lhs), "--lp_prefix", "pc", *extra)
        return sub, bindir, r

    qfile = os.path.join(cwd, "queries.txt")
    outs = []
    for name, lh, sol, oc in (("a", readme, rsol, roc), ("b", lh2, sol2, oc2)):
        g = api.Graph(lib, lh)
        seg = g.segments()
        first, last = g.chromosome(0)
        lens = (seg["end"].astype(np.int64) - seg["start"])[first - 1:last]
        p = jc.oracle_path(oc, 1)
        plane, s = model(p, lens, 0)
        pos = positions(plane, np.random.default_rng(2), cap=50)
        with open(qfile, "w") as f:
            f.write("".join("0 %d\n" % v for v in pos))
        for k, extra in enumerate(([], ["--path_coords", "pc.tsv", "--lift", qfile, "--lift_out", "lift.tsv"])):
            sub, _, r = run("%s%d" % (name, k), [lh], [sol], *extra)
            assert r.returncode == 0, r.stderr
            outs.append((r.stdout, r.stderr, open(os.path.join(sub, "simulation_sv.txt"), "rb").read(), sorted(x for x in os.listdir(sub) if x != "bin")))
        assert outs[-2][:3] == outs[-1][:3]                                 # stdout, stderr, side file: unchanged by the options
        assert outs[-1][3] == sorted(outs[-2][3] + ["pc.tsv", "lift.tsv"])
        assert open(os.path.join(sub, "pc.tsv")).read() == "%d\t%d\t%d\t%d\t%d\n" % tuple(s[k] for k in SUMMARY[1:])
        want = []
        for v, r in zip(pos.tolist(), lifts(plane, p, lens, 0, pos)):
            if r["cell"] < 0:
                want.append("%d\t-1\t0\t.\t.\t-1" % v)
                continue
            sid = first - 1 + abs(int(r["seg"]))
            want.append("%d\t%d\t%d\t%s\t%s\t%d" % (v, r["cell"], sid, "+" if r["seg"] > 0 else "-", g.chrom_name(sid), int(seg["start"][sid - 1]) + int(r["seg_off"])))
        assert open(os.path.join(sub, "lift.tsv")).read().splitlines() == want
        g.close()
    # --path_coords alone; the refusals: exit status 2 in front of anything run or written
    sub, _, r = run("alone", [readme], [rsol], "--path_coords", "pc.tsv")
    assert r.returncode == 0 and len(open(os.path.join(sub, "pc.tsv")).read().splitlines()) == 1
    with open(qfile, "w") as f:
        f.write("0 5\n")
    bad = [("list", [readme, lh2], [rsol, sol2], ["--path_coords", "pc.tsv"], "one sample"),
           ("list2", [readme, lh2], [rsol, sol2], ["--lift", qfile, "--lift_out", "lift.tsv"], "one sample"),
           ("devices", [readme], [rsol], ["--path_coords", "pc.tsv", "--devices", "1"], "--devices"),
           ("half", [readme], [rsol], ["--lift", qfile], "--lift_out"),
           ("half2", [readme], [rsol], ["--lift_out", "lift.tsv"], "--lift_out")]
    for name, lhs, sols, extra, word in bad:
        sub, _, r = run(name, lhs, sols, *extra)
        assert r.returncode == 2 and word in r.stderr, (name, r.returncode, r.stderr)
        assert r.stdout in ("", "bfb\n") and sorted(os.listdir(sub)) == ["bin"], (name, r.stdout, os.listdir(sub))
    for name, text, word in (("noquery", "0\n", "is no query"), ("words", "0 x\n", "is no query"), ("three", "0 1 2\n", "is no query"), ("chrom", "0 1\n1 5\n", "outside the sample"),
                             ("neg", "-1 5\n", "outside the sample")):
        with open(qfile, "w") as f:
            f.write(text)
        sub, _, r = run(name, [readme], [rsol], "--lift", qfile, "--lift_out", "lift.tsv")
        assert r.returncode == 2 and word in r.stderr, (name, r.returncode, r.stderr)
        assert r.stdout in ("", "bfb\n") and sorted(os.listdir(sub)) == ["bin"], (name, r.stdout, os.listdir(sub))
    sub, _, r = run("nofile", [readme], [rsol], "--lift", os.path.join(cwd, "no_such.txt"), "--lift_out", "lift.tsv")
    assert r.returncode != 0 and "Cannot open file" in r.stderr and sorted(os.listdir(sub)) == ["bin"]
    c2 = [os.path.join(cases.DATA, "readme_c2_chr0.sol"), os.path.join(cases.DATA, "readme_c2_chr1.sol")]
    for opt, extra in (("--path_coords", ["--path_coords", "pc.tsv"]), ("--lift", ["--lift", qfile, "--lift_out", "pc.tsv"]), ("--junc_profile", ["--junc_profile", "pc.tsv"])):
        sub, bindir, r = run("c2" + opt, [os.path.join(cases.DATA, "readme_c2.lh")], c2, *extra)
        assert r.returncode == 2 and opt in r.stderr and "PROP I1 / C1 / I2 / C2" in r.stderr, (r.returncode, r.stderr)
        assert not os.path.exists(os.path.join(sub, "pc.tsv"))
    r = t.run_cli(exe, sub, bindir, "--help")
    assert "--path_coords" in r.stdout and "--lift_out" in r.stdout


# ---- argument and state errors -------------------------------------------------------------------------------------------------
def check_errors(lib, sharded_devices):
    lh, sol = (os.path.join(cases.DATA, "readme6." + x) for x in ("lh", "sol"))
    g = api.Graph(lib, lh); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    one = api.lift_queries(0, [5])
    calls = (lambda: b.path_coords(1, one), b.path_coords_wait, b.path_coords_summaries, b.path_coords_results, b.path_coords_copy, b.path_coords_device,
             b.path_coords_plane_device)
    for call in calls:
        with _raises(ERR_STATE):                           # nothing uploaded
            call() if call not in (b.path_coords_copy,) else call(0, 0, 1)
    # the lengths: n must be n_seg, every length 0 .. 2^31 - 1
    for bad in ([1] * 5, [1] * 7, [], [1, 2, 3, 4, 5, -1], [2 ** 31, 1, 1, 1, 1, 1], [1, 1, 1, 2 ** 40, 1, 1]):
        with _raises(ERR_ARG):
            b.set_unit_seg_lengths(0, bad)
    for u in (-1, 1):
        with _raises(ERR_ARG):
            b.set_unit_seg_lengths(u, [1] * 6)
    b.set_unit_seg_lengths(0, [2 ** 31 - 1, 0, 1, 2, 3, 1000])
    b.upload()
    for call in calls:
        with _raises(ERR_STATE):                           # uploaded, never run: a request before a run
            call() if call not in (b.path_coords_copy,) else call(0, 0, 1)
    b.run(0); b.download()
    with _raises(ERR_STATE):
        b.path_coords_wait()                               # nothing queued
    for which in (2, -1):
        with _raises(ERR_ARG):
            b.path_coords(which, one)
    for unit in (1, -1, 2 ** 31 - 1):                      # a unit out of range in a query: refused at the request
        with _raises(ERR_ARG):
            b.path_coords(1, api.lift_queries([0, unit], [5, 5]))
    assert lib.ambi_batch_path_coords(b.h, 1, None, -1, None) == ERR_ARG and lib.ambi_batch_path_coords(b.h, 1, None, 1, None) == ERR_ARG
    with _raises(ERR_STATE):
        b.path_coords_results()                            # a refused request leaves nothing to read
    path = b.unit_path(0, 1).tolist()
    lens = [2 ** 31 - 1, 0, 1, 2, 3, 1000]
    plane, want = model(path, lens, 0)
    b.path_coords(1, api.lift_queries(0, [0, plane[-1] - 1, plane[-1]])); b.path_coords_wait()
    assert {k: int(b.path_coords_summaries()[0][k]) for k in SUMMARY} == want and want["bp_len"] > 2 ** 32
    assert b.path_coords_results().tobytes() == lifts(plane, path, lens, 0, [0, plane[-1] - 1, plane[-1]]).tobytes()
    r, s = api.Lift(), api.UnitCoords()
    for k in (3, -1):
        assert lib.ambi_batch_path_coords_result(b.h, k, r) == ERR_ARG
    assert lib.ambi_batch_path_coords_result(b.h, 0, None) == ERR_ARG
    for u in (1, -1):
        assert lib.ambi_batch_path_coords_summary(b.h, u, s) == ERR_ARG
    P = len(path)
    for first, n in ((-1, 1), (0, -1), (0, P + 2), (P + 1, 1), (P + 2, 0), (1, P + 1)):
        with _raises(ERR_ARG):
            b.path_coords_copy(0, first, n)
    assert lib.ambi_batch_path_coords_copy(b.h, 0, 0, 1, None) == ERR_ARG
    assert lib.ambi_batch_path_coords_plane_device(b.h, None, None, np.zeros(1, np.int64).ctypes.data_as(api._P(api.C.c_int64)), 0) == ERR_ARG
    b.junc_profile(1); b.junc_profile_wait()
    b.path_coords(1); b.path_coords_wait()
    assert len(b.path_coords_results()) == 0               # a request without queries: just the coordinates
    b.run(0)
    with _raises(ERR_STATE):
        b.path_coords_summaries()                          # a new run: the old results are gone
    b.wait()
    b.close()
    # a unit nobody gave lengths: an amplicon of 0 bp, every query out of range
    b = api.Batch(lib)
    b.add_unit(3, 0, [2.0, 2.0, 2.0], [1, 2], [2, 3], [1, 1], [1, 1], [2.0, 2.0], [], [], [], [])
    b.upload(); b.run(0)
    b.path_coords(1, api.lift_queries(0, [0, -1, 1])); b.path_coords_wait()
    s0 = b.path_coords_summaries()[0]
    assert int(s0["status"]) == api.ST_SHORTCUT and int(s0["cells"]) == 3 and int(s0["empty_cells"]) == 3 and int(s0["bp_len"]) == 0
    assert b.path_coords_results()["cell"].tolist() == [-1, -1, -1] and b.path_coords_copy(0).tolist() == [0, 0, 0, 0]
    b.close()
    b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    b.run_sharded(0, devices=sharded_devices)
    for call in (lambda: b.path_coords(1, one), b.path_coords_wait):
        with _raises(ERR_UNSUPPORTED):                     # one plane per share
            call()
    b.close(); g.close()
