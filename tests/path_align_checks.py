"""Checks of the path alignment (ambi_batch_path_align, csrc/ambi_path_align.hpp) shared by the CPU host-simulation tests and the GPU
tests (same assertions, different library).

Expected values never come from the stage under test.  model() is a plain-Python transcription of the rules: the textbook rounds with
one dict per round (ties to the insertion), the traceback from (D, n - m) and the merge into maximal runs; the runs of every entry
are compared with it byte for byte.  Independently of the model every entry is checked by what a script must do: applied to a it
gives Bo, its lengths sum to dist = la + lb - 2 LCS (the bit-vector recurrence of path_compare_checks), the runs are ordered and
maximal, and the slots behind n_runs are zero.  prefix, suffix and dist are also compared with the path comparison's of the same
pairs at the same cap."""
import ctypes
import os
import random

import numpy as np

import cases
import fold_profile_checks as fp
import junc_profile_checks as jc
import path_compare_checks as pcc
import profile_checks as pc
from ambigram_amd import api

U, G, rc, lcs_bits = pcc.U, pcc.G, pcc.rc, pcc.lcs_bits
_raises = fp._raises
ERR_UNSUPPORTED, ERR_STATE, ERR_ARG, ERR_TOO_LARGE = -9, -32, -33, -34
HEAD = ("status", "len_a", "len_b", "orient", "prefix", "suffix", "dist", "n_runs")
DMAXS = pcc.DMAXS


# ---- the model -------------------------------------------------------------------------------------------------------------------
_MODEL = {}


def model(a, B, dmax):
    """(prefix, suffix, dist or -1, [(a_pos, b_pos, len, kind)]) of a against B (already oriented).  The script of a pair does not depend
    on the cap -- the rounds are the same, the cap only decides whether they are run to their end -- so the rounds are walked once per
    pair, with the pair's own distance (the bit-vector recurrence) as the cap, and a smaller dmax gives -1; a pair further apart than
    dmax is never walked."""
    key = (tuple(a), tuple(B))
    if key not in _MODEL:
        p, s, l = pcc.ends_and_lcs(list(a), list(B))
        _MODEL[key] = [p, s, len(a) + len(B) - 2 * l, None]
    p, s, d, full = _MODEL[key]
    if d > dmax:
        return p, s, -1, []
    if full is None:
        full = _MODEL[key][3] = _model(list(a), list(B), d)
        assert full[:3] == (p, s, d), (full[:3], p, s, d)   # the rounds end at the recurrence's distance, not before and not later
    return full


def _model(a, B, dmax):
    la, lb = len(a), len(B)
    p = 0
    while p < min(la, lb) and a[p] == B[p]:
        p += 1
    s = 0
    while s < min(la, lb) - p and a[la - 1 - s] == B[lb - 1 - s]:
        s += 1
    X, Y = a[p:la - s], B[p:lb - s]
    n, m = len(X), len(Y)
    if n == 0 and m == 0:
        return p, s, 0, []
    if n == 0 or m == 0:
        return (p, s, n + m, [(p, p, n + m, 1 if m else 0)]) if n + m <= dmax else (p, s, -1, [])
    if abs(n - m) > dmax:
        return p, s, -1, []

    def starts(prev, k):                                 # the two candidates of diagonal k from the round before
        l, r = prev.get(k - 1), prev.get(k + 1)
        return (l + 1 if l is not None and l + 1 <= n else -1), (r if r is not None and r - k <= m else -1)

    rounds, D = [], -1
    for d in range(dmax + 1):
        new = {}
        for k in range(max(-d, -m), min(d, n) + 1):
            if (k + d) & 1:
                continue
            if d == 0:
                x = 0
            else:
                xl, xr = starts(rounds[d - 1], k)
                x = xl if xl > xr else xr                # a tie goes to the insertion
                if x < 0:
                    continue
            y = x - k
            while x < n and y < m and X[x] == Y[y]:
                x += 1; y += 1
            new[k] = x
        rounds.append(new)
        if new.get(n - m) == n:
            D = d
            break
    if D < 0:
        return p, s, -1, []
    edits, k = [None] * D, n - m
    for d in range(D, 0, -1):
        xl, xr = starts(rounds[d - 1], k)
        if xl > xr:
            edits[d - 1] = (0, p + xl - 1, p + xl - k); k -= 1
        else:
            edits[d - 1] = (1, p + xr, p + xr - k - 1); k += 1
    runs = []
    for kind, ap, bp in edits:
        if runs:
            a0, b0, ln, k0 = runs[-1]
            if k0 == kind and ((kind == 0 and ap == a0 + ln and bp == b0) or (kind == 1 and bp == b0 + ln and ap == a0)):
                runs[-1] = (a0, b0, ln + 1, k0)
                continue
        runs.append((ap, bp, 1, kind))
    return p, s, D, runs


def apply_runs(a, B, runs):
    """What the runs make of a; every run must stand where the text built so far ends in Bo."""
    out, ai = [], 0
    for ap, bp, ln, kind in runs:
        assert ap >= ai and ln >= 1 and kind in (0, 1), (ap, bp, ln, kind)
        out += a[ai:ap]
        assert bp == len(out), ("b_pos", ap, bp, ln, kind, len(out))
        if kind == 0:
            assert ap + ln <= len(a)
            ai = ap + ln
        else:
            assert bp + ln <= len(B)
            out += B[bp:bp + ln]
            ai = ap
    return out + a[ai:]


def check_script(a, B, dmax, head, runs, tag):
    """The checks that do not need the model."""
    d = len(a) + len(B) - 2 * pcc.ends_and_lcs(a, B)[2]     # (lcs_bits, computed once per pair)
    if d > dmax:
        assert head["dist"] == -1 and head["n_runs"] == 0 and len(runs) == 0, (tag, head, d)
        return
    assert head["dist"] == d and sum(r[2] for r in runs) == d and len(runs) == head["n_runs"] <= max(d, 0), (tag, head, d)
    assert apply_runs(a, B, runs) == B, tag
    for (a0, b0, l0, k0), (a1, b1, l1, k1) in zip(runs, runs[1:]):     # ordered, and maximal: a matched cell between two runs of a kind
        ea, eb = (a0 + l0, b0) if k0 == 0 else (a0, b0 + l0)
        assert a1 >= ea and b1 >= eb and a1 - ea == b1 - eb, (tag, (a0, b0, l0, k0), (a1, b1, l1, k1))
        assert k0 != k1 or a1 > ea, (tag, "not maximal", (a0, b0, l0, k0), (a1, b1, l1, k1))


def check_model():
    """The model against the quadratic table and the script checks, on small random pairs."""
    rng = random.Random(13)
    seen = set()
    for it in range(1200):
        alpha = rng.choice((1, 2, 3))
        a = [rng.choice((-1, 1)) * rng.randint(1, alpha) for _ in range(rng.randint(1, 40))]
        if it % 2:
            b = list(a)
            for _ in range(rng.randint(0, 5)):
                at = rng.randrange(len(b) + 1)
                if rng.random() < 0.5 or len(b) < 2:
                    b.insert(at, rng.choice((-1, 1)) * rng.randint(1, alpha))
                else:
                    del b[min(at, len(b) - 1)]
        else:
            b = [rng.choice((-1, 1)) * rng.randint(1, alpha) for _ in range(rng.randint(1, 40))]
        want = len(a) + len(b) - 2 * pcc.lcs_table(a, b)
        for dmax in (0, 1, 4, 16, 64):
            p, s, d, runs = model(a, b, dmax)
            assert d == (want if want <= dmax else -1) and (p, s) == pcc.ends_and_lcs(a, b)[:2], (a, b, dmax, d, want)
            check_script(a, b, dmax, dict(dist=d, n_runs=len(runs)), runs, ("model", it))
            seen |= {(k0, k1, a1 - (a0 + l0 if k0 == 0 else a0)) for (a0, _, l0, k0), (a1, _, _, k1) in zip(runs, runs[1:])}
    assert (0, 1, 0) in seen and {(0, 0), (1, 1), (1, 0)} <= {(x, y) for x, y, _ in seen}    # a D run directly followed by an I run, and every other succession


# ---- a request -------------------------------------------------------------------------------------------------------------------
def expected(a, b, orient, dmax):
    """a, b: (path of local ids or None, status).  (header dict, runs)."""
    (pa, sa), (pb, sb) = a, b
    bad = [st for p, st in (a, b) if p is None]
    if bad:
        return dict(status=bad[0], len_a=len(pa or []), len_b=len(pb or []), orient=orient, prefix=0, suffix=0, dist=-1, n_runs=0), []
    p, s, d, runs = model(pa, rc(pb) if orient else pb, dmax)
    return dict(status=0, len_a=len(pa), len_b=len(pb), orient=orient, prefix=p, suffix=s, dist=d, n_runs=len(runs)), runs


def block_bytes(lib, b):
    """The whole block where the engine left it: host memory of the host simulation, device memory of the HIP engine."""
    ptr, nbytes, runs_off = b.path_align_device()
    if lib.ambi_backend_name() == b"hip":
        import torch
        from ambigram_amd.dist import _DevBytes
        return torch.as_tensor(_DevBytes(ptr, nbytes), device="cuda").cpu().numpy().tobytes(), runs_off
    return ctypes.string_at(ptr, nbytes), runs_off


def request(lib, b, sides, entries, dmax, tag, stream=None, compare=True):
    """Queues the entries (i, j, orient; i and j index `sides`: [(code, path or None, status)]), waits, and checks every entry: against
    the model byte for byte, by the script checks, against the comparison of the same pairs, and the block slot by slot."""
    triples = [(sides[i][0], sides[j][0], o) for i, j, o in entries]
    cmp_ = None
    if compare:
        b.path_compare([t[:2] for t in triples], dmax, stream); b.path_compare_wait()
        cmp_ = b.path_compare_results()
    b.path_align(triples, dmax, stream); b.path_align_wait()
    head, runs = b.path_align_results()
    assert head.dtype == api.PATH_ALIGN_DTYPE and head.dtype.itemsize == 32 and api.ALIGN_RUN_DTYPE.itemsize == 16 and len(head) == len(runs) == len(entries)
    raw, runs_off = block_bytes(lib, b)
    stride = max(dmax, 1)
    assert runs_off == (32 * len(entries) + 15) & ~15 and len(raw) == max(runs_off + 16 * stride * len(entries), 16)
    assert raw[:32 * len(entries)] == head.tobytes()
    for k, (i, j, o) in enumerate(entries):
        want_h, want_r = expected(sides[i][1:], sides[j][1:], o, dmax)
        got_h = {f: int(head[k][f]) for f in HEAD}
        assert got_h == want_h, (tag, dmax, k, triples[k], got_h, want_h)
        assert runs[k].tobytes() == np.array(want_r, np.int32).reshape(-1, 4).tobytes(), (tag, dmax, k, triples[k], runs[k].tolist()[:8], want_r[:8])
        slots = raw[runs_off + 16 * stride * k:runs_off + 16 * stride * (k + 1)]
        assert slots[:16 * len(want_r)] == runs[k].tobytes() and not any(slots[16 * len(want_r):]), (tag, dmax, k, "slots behind n_runs")
        if want_h["status"] == 0:
            pa, pb = sides[i][1], sides[j][1]
            check_script(pa, rc(pb) if o else pb, dmax, got_h, [tuple(r) for r in runs[k].tolist()], (tag, dmax, k))
        if cmp_ is not None:
            c = cmp_[k]
            assert (int(c["status"]), int(c["len_a"]), int(c["len_b"])) == (got_h["status"], got_h["len_a"], got_h["len_b"])
            assert (int(c["prefix"][o]), int(c["suffix"][o]), int(c["dist"][o])) == (got_h["prefix"], got_h["suffix"], got_h["dist"]), (tag, dmax, k, c, got_h)
    return head, runs


class grid_env:
    """AMBI_ALIGN_GRID for the requests inside."""
    def __init__(self, grid):
        self.grid = grid

    def __enter__(self):
        self.saved = os.environ.pop("AMBI_ALIGN_GRID", None)
        if self.grid:
            os.environ["AMBI_ALIGN_GRID"] = str(self.grid)

    def __exit__(self, *exc):
        os.environ.pop("AMBI_ALIGN_GRID", None)
        if self.saved is not None:
            os.environ["AMBI_ALIGN_GRID"] = self.saved


def given_sides(shapes):
    """(sides, given paths, entries): every shape (a, c) as two given paths, aligned both ways round and with itself, in both orientations."""
    sides, given, entries = [], [], []
    for a, c in shapes:
        i = len(sides)
        sides += [(G(len(given)), a, 0), (G(len(given) + 1), c, 0)]
        given += [a, c]
        entries += [(x, y, o) for x, y in ((i, i + 1), (i + 1, i), (i, i)) for o in (0, 1)]
    return sides, given, entries


def one_batch(lib, oracle, workdir):
    it = fp.units(oracle, workdir)[0]
    graphs, b, _ = fp.make_batch(lib, [it])
    b.upload(); b.run(0); b.download()
    return it, graphs, b


# ---- the small shapes of the comparison ------------------------------------------------------------------------------------------
def check_small(lib, oracle, workdir, grid=None):
    """path_compare_checks.small_shapes() in both orientations at every cap: the hand-over and ballot edges, snakes of 7 / 8 / 9 and
    63 / 64 / 65, the 2100-cell pair, a distance of exactly dmax and dmax + 1, the periodic pairs where the tie rule decides; with
    `grid`, more entries than workgroups."""
    it, graphs, b = one_batch(lib, oracle, workdir)
    sides, given, entries = given_sides(pcc.small_shapes())
    u0 = len(sides)
    sides += [(U(0, 0), jc.oracle_path(it[3], 0), 0), (U(0, 1), jc.oracle_path(it[3], 1), 0)]
    entries += [(u0, u0 + 1, 0), (u0, u0 + 1, 1), (u0 + 1, 0, 0), (1, u0, 1)]
    b.set_compare_paths(given)
    dists = set()
    with grid_env(grid):
        for dmax in DMAXS:
            head, _ = request(lib, b, sides, entries, dmax, "small")
            dists |= {(int(d), dmax) for d in head["dist"]}
    assert all((d, d) in dists and (-1, d - 1) in dists for d in (1, 2, 3, 4, 5)), sorted(dists)   # a distance of exactly dmax, and of dmax + 1
    assert len(entries) > 64
    pc.close_all(graphs, b)


# ---- shapes for the traceback and the merge --------------------------------------------------------------------------------------
def traceback_shapes():
    rng = random.Random(7)
    cell = lambda: rng.choice((-1, 1)) * rng.randint(1, 3)
    a = [cell() for _ in range(900)]
    thirds = [c for i, c in enumerate(a) if i % 3 != 1]                              # 300 single deletions, some of them merging
    mixed = []
    for i, c in enumerate(a):                                                        # 150 deletions and 150 insertions of a foreign cell, alternating
        if i % 6 != 1:
            mixed.append(c)
        if i % 6 == 4:
            mixed.append(4)
    long_ = [cell() for _ in range(1500)]
    cut = long_[:200] + long_[500:]                                                  # ONE run of 300 cells (200 .. 499): it crosses the merge tile
    few, many = [cell() for _ in range(3)], [cell() for _ in range(200)]             # history rows clipped by the grid
    mid = [cell() for _ in range(60)]
    ends = ([1] + mid + [2], [3] + mid + [2, -3])                                    # an edit at the first and at the last cell of the middle window
    subst = (mid[:30] + [1] + mid[30:], mid[:30] + [-2] + mid[30:])                  # one cell substituted: a D run directly followed by an I run
    return dict(thirds=(a, thirds), mixed=(a, mixed), cut=(long_, cut), clipped=(few, many), ends=ends, subst=subst)


def check_traceback_floors():
    """What the shapes offer, from the model: more runs than a group has threads, a run longer than a merge tile, both kinds alternating,
    a deletion directly followed by an insertion."""
    T = traceback_shapes()
    for (x, y), kind in ((T["thirds"], 0), (T["thirds"][::-1], 1)):
        _, _, d, runs = model(x, y, 1024)
        assert d == 300 and len(runs) == 293 > 256 and {r[3] for r in runs} == {kind}, (d, len(runs))
    _, _, d, runs = model(*T["mixed"], 1024)
    kinds = [r[3] for r in runs]
    assert d == 300 and len(runs) == 300 and kinds.count(0) == 150 and all(x != y for x, y in zip(kinds, kinds[1:])), (d, len(runs))
    for (x, y), kind in ((T["cut"], 0), (T["cut"][::-1], 1)):
        _, _, d, runs = model(x, y, 1024)
        assert d == 300 and len(runs) == 1 and runs[0][2:] == (300, kind), (d, runs)
    for x, y in (T["clipped"], T["clipped"][::-1]):
        p, s, d, runs = model(x, y, 1024)
        assert d > min(len(x), len(y)) - p - s > 0, (p, s, d)                        # diagonals leave the grid
    p, s, d, runs = model(*T["ends"], 1024)
    assert runs[0][:2] == (p, p) and runs[-1][3] == 1 and runs[-1][1] + runs[-1][2] == len(T["ends"][1]) - s, (p, s, runs)
    _, _, d, runs = model(*T["subst"], 1024)
    assert d == 2 and [r[2:] for r in runs] == [(1, 0), (1, 1)] and runs[1][:2] == (runs[0][0] + 1, runs[0][1]), runs


def check_traceback(lib, oracle, workdir):
    it, graphs, b = one_batch(lib, oracle, workdir)
    sides, given, entries = given_sides(list(traceback_shapes().values()))
    b.set_compare_paths(given)
    for dmax in (1024, 301, 300, 299, 2, 1):
        request(lib, b, sides, entries, dmax, "traceback")
    pc.close_all(graphs, b)


# ---- the real units --------------------------------------------------------------------------------------------------------------
def unit_entries(items, sides, given_of):
    """(entries, given paths, the entries that must end inside the cap of 1024).  path against path_indel of every unit as is, and the
    final path against the other run's final path as a given path in both orientations: none of these is -1 at 1024.  Beside them
    path against the reverse complement of path_indel (some are further apart than 1024: all 1025 rounds, then -1) and the units with
    a negative status against a good one and against a given path."""
    entries, given, inside = [], [], []
    n_unit = len(sides)
    for u in range(len(items)):
        inside.append(len(entries))
        entries += [(2 * u, 2 * u + 1, 0), (2 * u, 2 * u + 1, 1)]
        other = given_of(u)
        if other is not None:
            t = len(sides)
            sides.append((G(len(given)), other, 0)); given.append(other)
            inside += [len(entries) + q for q in range(3)]
            entries += [(2 * u + 1, t, 0), (2 * u + 1, t, 1), (t, 2 * u + 1, 1)]
    bad = [i for i in range(n_unit) if sides[i][1] is None]
    assert bad, "a unit with a negative status"
    for i in bad:
        entries += [(i, 1, 0), (1, i, 1), (i, i, 0), (i, n_unit, 1), (n_unit, i, 0)]
    return entries, given, [k for k in inside if sides[entries[k][0]][1] is not None and sides[entries[k][1]][1] is not None]


def check_units(lib, oracle, workdir, run_stream=None, req_stream=None, runs=(False, True)):
    """One batch of all units at dmax 1024 and 64; then the same batch run reversed against the forward run's final paths."""
    items = fp.units(oracle, workdir)
    graphs, b, _ = fp.make_batch(lib, items)
    b.upload()
    for reversed_ in runs:
        b.run(api.FLAG_REVERSED if reversed_ else 0, run_stream)
        if req_stream is None:
            b.download()
        sides = pcc.unit_sides(items, reversed_)
        entries, given, inside = unit_entries(items, sides, pcc.final_of(items, not reversed_))
        b.set_compare_paths(given)
        head, _ = request(lib, b, sides, entries, 1024, ("units", reversed_), req_stream)
        assert len(inside) > 30 and (head["dist"][inside] >= 0).all()       # the cap of 1024 hides nothing
        head, _ = request(lib, b, sides, entries, 64, ("units", reversed_), req_stream)
        minus = head["status"] == 0
        assert (head["dist"][minus] == -1).any() and not head["n_runs"][head["dist"] == -1].any()
    pc.close_all(graphs, b)


def check_floors(oracle, workdir):
    """What the units must offer, from the model: a pair with at least 40 runs, a run of at least 512 cells, both kinds, equal pairs,
    and NO pair that is -1 at dmax 1024 (the cap must not hide a failure)."""
    items = fp.units(oracle, workdir)
    most, longest, kinds, equal = 0, 0, set(), 0
    for name, _, _, oc, orev in items:
        if fp.unit_status(name, oc) < 0:
            continue
        p0, p1 = jc.oracle_path(oc, 0), jc.oracle_path(oc, 1)
        todo = [(p0, p1)]
        if fp.unit_status(name, orev) >= 0:
            r1 = jc.oracle_path(orev, 1)
            todo += [(p1, r1), (p1, rc(r1))]
        for a, B in todo:
            _, _, d, runs = model(a, B, 1024)
            assert d == len(a) + len(B) - 2 * lcs_bits(a, B) >= 0, (name, d)
            most = max(most, len(runs)); longest = max([longest] + [r[2] for r in runs]); kinds |= {r[3] for r in runs}; equal += d == 0
    assert most >= 40 and longest >= 512 and kinds == {0, 1} and equal >= 5, (most, longest, kinds, equal)


def check_each_alone(lib, oracle, workdir):
    """Every unit in a batch of its own (the one-unit express path)."""
    for it in fp.units(oracle, workdir):
        graphs, b, _ = fp.make_batch(lib, [it])
        b.upload(); b.run(0); b.download()
        sides = pcc.unit_sides([it])
        other = jc.oracle_path(it[4], 1) if fp.unit_status(it[0], it[4]) >= 0 else [1, 2, 3]
        sides.append((G(0), other, 0))
        b.set_compare_paths([other])
        request(lib, b, sides, [(0, 1, 0), (0, 1, 1), (1, 2, 0), (2, 1, 1), (1, 1, 0)], 1024, ("alone", it[0]))
        pc.close_all(graphs, b)


def check_request_paths(lib, oracle, workdir, run_stream=None, req_stream=None):
    """The run on one stream, the request on another, without a download in between; a request nobody waited for, then another with
    other entries and another cap; a batch closed with a request in flight."""
    check_units(lib, oracle, workdir, run_stream, req_stream, runs=(False,))
    items = fp.units(oracle, workdir)[:4]
    graphs, b, _ = fp.make_batch(lib, items)
    b.upload(); b.run(0, run_stream)
    sides = pcc.unit_sides(items)
    given = [pcc.final_of(items, True)(u) for u in range(4)]
    sides += [(G(u), given[u], 0) for u in range(4)]
    entries = [(2 * u, 2 * u + 1, u & 1) for u in range(4)] + [(2 * u + 1, 8 + u, 1 - (u & 1)) for u in range(4)]
    b.set_compare_paths(given)
    b.path_align([(sides[i][0], sides[j][0], o) for i, j, o in entries], 1024, req_stream)     # nobody waits for it
    request(lib, b, sides, entries[::-1], 7, "unwaited", req_stream)
    b.run(0, run_stream)
    b.path_align([(U(0, 0), U(0, 1), 0)], 64, req_stream)
    pc.close_all(graphs, b)
    graphs, b, _ = fp.make_batch(lib, items[::-1])
    b.upload(); b.run(0, run_stream); b.download()
    sides = pcc.unit_sides(items[::-1])
    request(lib, b, sides, [(2 * u, 2 * u + 1, 0) for u in range(4)], 1024, "after a close in flight", req_stream)
    pc.close_all(graphs, b)


def check_set_between_request_and_wait(lib, oracle, workdir, run_stream=None, req_stream=None, before_run=None):
    """A comparison AND an alignment are queued; a run in between moves the results' epoch and the set of given paths is replaced --
    by none, by a smaller one, by one of the same size -- before either is waited for: both are queued again at their wait, each with
    the paths it was made with.  The next request sees the new set."""
    items = fp.units(oracle, workdir)[:3]
    graphs, b, _ = fp.make_batch(lib, items)
    b.upload(); b.run(0, run_stream)
    units = pcc.unit_sides(items)
    base = len(units)
    old = [pcc.final_of(items, True)(u) for u in range(3)] + [[1, 2, 3, -3]]
    sides = units + [(G(t), p, 0) for t, p in enumerate(old)]
    entries = [(2 * u + 1, base + u, u & 1) for u in range(3)] + [(base + 3, 1, 0), (base + 3, base + 3, 1), (0, 1, 0)]
    codes = [(sides[i][0], sides[j][0], o) for i, j, o in entries]
    for new in ([], [[3, 2, 1]], [[2, 2], [1], [-1, -2], [3]]):
        b.set_compare_paths(old)
        b.path_compare([c[:2] for c in codes], 1024, req_stream)                             # nobody waits for either yet
        b.path_align(codes, 1024, req_stream)
        if before_run:
            before_run()
        b.run(0, run_stream)
        b.set_compare_paths(new)
        b.path_align_wait(); b.path_compare_wait()
        head, runs = b.path_align_results()
        got_c = b.path_compare_results()
        for k, (i, j, o) in enumerate(entries):
            want_h, want_r = expected(sides[i][1:], sides[j][1:], o, 1024)
            assert {f: int(head[k][f]) for f in HEAD} == want_h and [tuple(r) for r in runs[k].tolist()] == want_r, ("set between", len(new), k)
            assert pcc.as_dict(got_c[k]) == pcc.expected(sides[i][1:], sides[j][1:], 1024), ("set between, the comparison", len(new), k)
        for t in range(len(new), 4):
            with _raises(ERR_ARG):
                b.path_align([(0, G(t), 0)])                # the new set has fewer paths
        if new:
            now = units + [(G(t), p, 0) for t, p in enumerate(new)]
            request(lib, b, now, [(1, base + t, t & 1) for t in range(len(new))] + [(base, base, 0)], 64, ("after the new set", len(new)), req_stream)
    pc.close_all(graphs, b)


def check_from_compare(lib, oracle, workdir):
    """align_from_compare: the orientation with the smaller dist, ties as is, pairs with both dist -1 dropped; then the request it makes."""
    it, graphs, b = one_batch(lib, oracle, workdir)
    x = [1, 2, -3, 3, 1, -2, 2, 2]
    given = [x, x[:3] + [1] + x[3:], rc(x[:5] + x[6:]), [3] * 40, x + rc(x), x]
    sides = [(G(t), p, 0) for t, p in enumerate(given)]
    pairs = [(0, 1), (0, 2), (0, 3), (4, 4), (0, 5), (3, 0)]
    b.set_compare_paths(given)
    codes = [(sides[i][0], sides[j][0]) for i, j in pairs]
    b.path_compare(codes, 8); b.path_compare_wait()
    triples = api.align_from_compare(codes, b.path_compare_results())
    assert triples.dtype == np.int32 and triples.tolist() == [[G(0), G(1), 0], [G(0), G(2), 1], [G(4), G(4), 0], [G(0), G(5), 0]]
    request(lib, b, sides, [(0, 1, 0), (0, 2, 1), (4, 4, 0), (0, 5, 0)], 8, "from compare")
    assert api.align_from_compare([], b.path_compare_results()[:0]).shape == (0, 3)
    pc.close_all(graphs, b)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------
def printed(path_abs):
    """A path as the CLI prints it: `|` where the direction turns."""
    out = ""
    for i, v in enumerate(path_abs):
        out += ("|" if i and (path_abs[i - 1] > 0) != (v > 0) else "") + "%d%s" % (abs(v), "+" if v > 0 else "-")
    return out


def cli_rows(tag, c, a, b, dmax, shift):
    """The lines of one row: a, b in local ids; shift: global id - local id."""
    d = [model(a, B, dmax)[2] for B in (b, rc(b))]
    if d[0] < 0 and d[1] < 0:
        return ["\t".join(["A", tag, str(c), "-1", "-1", "0"])]
    o = 1 if d[0] < 0 or 0 <= d[1] < d[0] else 0
    B = rc(b) if o else b
    _, _, dist, runs = model(a, B, dmax)
    glob = lambda p: [v + shift if v > 0 else v - shift for v in p]
    out = ["\t".join(["A", tag, str(c), str(o), str(dist), str(len(runs))])]
    for ap, bp, ln, kind in runs:
        out.append("\t".join(["I" if kind else "D", str(ap), str(bp), str(ln), printed(glob(B[bp:bp + ln] if kind else a[ap:ap + ln]))]))
    return out


def check_cli(lib, exe, cwd, oracle, workdir):
    import test_cli_dropin as t
    items = fp.units(oracle, workdir)

    def run(name, lhs, sols, *extra):
        sub = os.path.join(cwd, name)
        os.makedirs(sub)
        bindir = os.path.join(sub, "bin")
        t.fake_cbc(bindir, sols)
        r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", ",".join(lhs), "--lp_prefix", "pa", *extra)
        return sub, bindir, r

    truth = os.path.join(cwd, "truth.txt")
    n_lines = 0
    for k, (dmax, which) in enumerate(((1024, (0, 2, 3, 6)), (64, (2, 6)), (3, (0, 6)))):
        for idx in which:
            name, lh, sol, oc, orev = items[idx]
            with open(truth, "w") as f:
                f.write(pcc.printed(orev["path_indel"], bars=(0, 3)) + "\n")
            sub, _, r = run("a%d_%d" % (k, idx), [lh], [sol], "--path_compare", "pc.tsv", "--truth", truth, "--compare_dmax", str(dmax), "--path_align", "pa.tsv")
            assert r.returncode == 0, r.stderr
            p0, p1, t1 = jc.oracle_path(oc, 0), jc.oracle_path(oc, 1), jc.oracle_path(orev, 1)
            want = cli_rows("P", 0, p0, p1, dmax, oc["start"] - 1) + cli_rows("T", 0, p1, t1, dmax, oc["start"] - 1)
            got = open(os.path.join(sub, "pa.tsv")).read().splitlines()
            assert got == want, (name, dmax, got[:6], want[:6])
            assert open(os.path.join(sub, "pc.tsv")).read().splitlines()[0] == pcc.row("P", lh, 0, pcc.expected((p0, 0), (p1, 0), dmax))
            n_lines += len(got)
    assert n_lines > 40
    (_, lh, sol, _, _) = items[0]
    for name, extra, word in (("alone", ["--path_align", "pa.tsv"], "--path_compare"),
                              ("devices", ["--path_compare", "pc.tsv", "--path_align", "pa.tsv", "--devices", "1"], "--devices")):
        sub, bindir, r = run(name, [lh], [sol], *extra)
        assert r.returncode == 2 and word in r.stderr, (name, r.returncode, r.stderr)
        assert r.stdout in ("", "bfb\n") and sorted(os.listdir(sub)) == ["bin"], (name, r.stdout, os.listdir(sub))
    r = t.run_cli(exe, sub, bindir, "--help")
    assert "--path_align" in r.stdout


# ---- device view -----------------------------------------------------------------------------------------------------------------
def check_device_view(lib, oracle, workdir):
    """ambi_batch_path_align_device: the block in device memory, read back through torch, against the host getters byte for byte (the
    run and the request on a stream of their own)."""
    import torch
    items = fp.units(oracle, workdir)
    graphs, b, _ = fp.make_batch(lib, items)
    stream = torch.cuda.Stream()
    b.upload(); b.run(0, stream.cuda_stream)
    sides = pcc.unit_sides(items)
    request(lib, b, sides, [(2 * u, 2 * u + 1, u & 1) for u in range(len(items))], 1024, "device view", stream.cuda_stream)
    pc.close_all(graphs, b)


# ---- argument and state errors ---------------------------------------------------------------------------------------------------
def check_errors(lib, sharded_devices):
    lh, sol = (os.path.join(cases.DATA, "readme6." + x) for x in ("lh", "sol"))
    g = api.Graph(lib, lh); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    one = [(U(0, 0), U(0, 1), 0)]
    calls = (lambda: b.path_align(one), b.path_align_wait, b.path_align_results, b.path_align_device)
    for call in calls:
        with _raises(ERR_STATE):                           # nothing uploaded
            call()
    b.upload()
    for call in calls:
        with _raises(ERR_STATE):                           # uploaded, never run
            call()
    b.run(0); b.download()
    with _raises(ERR_STATE):
        b.path_align_wait()                                # nothing queued
    for dmax in (-1, 1025):
        with _raises(ERR_ARG):
            b.path_align(one, dmax)
    for o in (2, -1):
        with _raises(ERR_ARG):
            b.path_align([(0, 1, o)])
    for side in (2, 3, -1, -2):                            # one unit, no given path
        for p in ([(side, 0, 0)], [(0, side, 0)], one + [(1, side, 1)]):
            with _raises(ERR_ARG):
                b.path_align(p)
    with _raises(ERR_TOO_LARGE):                           # 65537 entries of 1024 slots of 16 bytes: a run area above 1 GiB
        b.path_align(one * 65537, 1024)
    with _raises(ERR_STATE):
        b.path_align_wait()                                # the refused request queued nothing
    b.set_compare_paths([[32767, -32767], [1]])
    b.path_align([(G(0), G(1), 0), (G(1), G(1), 0), (G(1), G(1), 1)], 0); b.path_align_wait()
    head, runs = b.path_align_results()
    assert head["dist"].tolist() == [-1, 0, -1] and head["n_runs"].tolist() == [0, 0, 0] and head["orient"].tolist() == [0, 0, 1]
    r, n = api.PathAlign(), ctypes.c_int32(-5)
    for k in (3, -1):
        assert lib.ambi_batch_path_align_result(b.h, k, r) == ERR_ARG
        assert lib.ambi_batch_path_align_runs(b.h, k, None, 0, ctypes.byref(n)) == ERR_ARG
    assert lib.ambi_batch_path_align_result(b.h, 0, None) == ERR_ARG and lib.ambi_batch_path_align_runs(b.h, 0, None, 0, None) == ERR_ARG
    assert lib.ambi_batch_path_align_runs(b.h, 0, None, 0, ctypes.byref(n)) == 0 and n.value == 0
    b.path_align([(G(0), G(1), 0)], 3); b.path_align_wait()
    assert lib.ambi_batch_path_align_runs(b.h, 0, None, 0, ctypes.byref(n)) == ERR_ARG and n.value == 2     # too small a cap: the number is still given
    b.set_compare_paths([])
    with _raises(ERR_STATE):
        b.path_align_results()                             # a new set: the old results are gone, as the comparison's
    with _raises(ERR_ARG):
        b.path_align([(0, G(0), 0)])                       # the set was replaced by none
    b.path_compare([(0, 1)]); b.path_compare_wait()
    with _raises(ERR_STATE):
        b.path_align_results()                             # another kind's request does not answer for this one
    b.path_align([], 64); b.path_align_wait()
    assert len(b.path_align_results()[0]) == 0             # a request without entries
    b.path_align(one, 1024); b.path_align_wait()
    assert b.path_align_results()[0]["dist"].tolist() == [0]
    b.run(0)
    with _raises(ERR_STATE):
        b.path_align_results()                             # a new run: the old results are gone
    b.wait()
    b.close()
    b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    b.run_sharded(0, devices=sharded_devices)
    for call in (lambda: b.path_align(one), b.path_align_wait):
        with _raises(ERR_UNSUPPORTED):                     # a pair may span shares
            call()
    b.close(); g.close()
