"""Checks of the path comparison (ambi_batch_path_compare, csrc/ambi_path_compare.hpp) shared by the CPU host-simulation tests and the
GPU tests (same assertions, different library).

Expected values never come from the stage under test: prefix and suffix are plain loops; the LCS is the bit-vector recurrence on
Python integers, V = (V + (V & M)) | (V - (V & M)), which the CPU half checks against the quadratic table on small random pairs;
dist = la + lb - 2 LCS, replaced by -1 above dmax.  Every field of every pair is compared.  walk() is an independent model of the
stage's scheme (trim first, rounds from the previous V only, a diagonal off the grid starts nothing); it yields the floors -- which
distances and snakes the inputs offer -- and is itself checked against the recurrence, never used as an expectation."""
import os
import random

import numpy as np

import cases
import fold_profile_checks as fp
import junc_profile_checks as jc
import profile_checks as pc
from ambigram_amd import api

FIELDS = ("status", "len_a", "len_b", "dmax", "prefix", "suffix", "dist", "lcs")
U, G = api.compare_unit, api.compare_given
_raises = fp._raises
ERR_UNSUPPORTED, ERR_STATE, ERR_ARG = -9, -32, -33


# ---- expected values ---------------------------------------------------------------------------------------------------------
def rc(p):
    return [-v for v in reversed(p)]


def lcs_bits(a, b):
    la = len(a)
    masks = {}
    for i, c in enumerate(a):
        masks[c] = masks.get(c, 0) | (1 << i)
    full = (1 << la) - 1
    V = full
    for c in b:
        M = masks.get(c, 0)
        V = ((V + (V & M)) | (V - (V & M))) & full
    return la - bin(V).count("1")


def lcs_table(a, b):
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[len(b)]


_LCS = {}


def ends_and_lcs(a, B):
    key = (tuple(a), tuple(B))
    if key not in _LCS:
        la, lb = len(a), len(B)
        p = 0
        while p < la and p < lb and a[p] == B[p]:
            p += 1
        s = 0
        while s < min(la, lb) - p and a[la - 1 - s] == B[lb - 1 - s]:
            s += 1
        _LCS[key] = (p, s, lcs_bits(a, B))
    return _LCS[key]


def expected(a, b, dmax):
    """a, b: (path of local ids or None, status).  The dict of every field."""
    (pa, sa), (pb, sb) = a, b
    bad = [st for p, st in (a, b) if p is None]
    if bad:
        return dict(status=bad[0], len_a=len(pa or []), len_b=len(pb or []), dmax=0, prefix=[0, 0], suffix=[0, 0], dist=[-1, -1], lcs=[-1, -1])
    r = dict(status=0, len_a=len(pa), len_b=len(pb), dmax=dmax, prefix=[], suffix=[], dist=[], lcs=[])
    for B in (pb, rc(pb)):
        p, s, l = ends_and_lcs(pa, B)
        d = len(pa) + len(pb) - 2 * l
        r["prefix"].append(p); r["suffix"].append(s); r["dist"].append(d if d <= dmax else -1); r["lcs"].append(l if d <= dmax else -1)
    return r


def as_dict(row):
    return {k: (row[k].tolist() if k in ("prefix", "suffix", "dist", "lcs") else int(row[k])) for k in FIELDS}


def request(b, sides, pairs, dmax, tag, stream=None):
    """Queues the pairs (indices into `sides`: [(code, path or None, status)]), waits, compares every field of every pair."""
    b.path_compare([(sides[i][0], sides[j][0]) for i, j in pairs], dmax, stream); b.path_compare_wait()
    got = b.path_compare_results()
    assert got.dtype == api.PATH_COMPARE_DTYPE and got.dtype.itemsize == 48 and len(got) == len(pairs)
    for k, (i, j) in enumerate(pairs):
        want = expected(sides[i][1:], sides[j][1:], dmax)
        assert as_dict(got[k]) == want, (tag, dmax, k, (sides[i][0], sides[j][0]), as_dict(got[k]), want)
    return got


# ---- the model walk ----------------------------------------------------------------------------------------------------------
def walk(a, B, dmax):
    """(prefix, suffix, dist or -1, longest snake of the rounds) by the stage's scheme, written independently."""
    la, lb = len(a), len(B)
    p = 0
    while p < min(la, lb) and a[p] == B[p]:
        p += 1
    s = 0
    while s < min(la, lb) - p and a[la - 1 - s] == B[lb - 1 - s]:
        s += 1
    X, Y = a[p:la - s], B[p:lb - s]
    n, m = len(X), len(Y)
    if n == 0 or m == 0:
        return p, s, (n + m if n + m <= dmax else -1), 0
    if abs(n - m) > dmax:
        return p, s, -1, 0
    V, longest = {}, 0
    for d in range(dmax + 1):
        new = {}
        for k in range(max(-d, -m), min(d, n) + 1):
            if (k + d) & 1:
                continue
            if d == 0:
                x = 0
            else:
                l, r = V.get(k - 1), V.get(k + 1)
                c = [v for v in (l + 1 if l is not None and l + 1 <= n else None, r if r is not None and r - k <= m else None) if v is not None]
                if not c:
                    continue
                x = max(c)
            y, x0 = x - k, x
            while x < n and y < m and X[x] == Y[y]:
                x += 1; y += 1
            longest = max(longest, x - x0)
            new[k] = x
        V = new                                          # the next round sees this round only
        if V.get(n - m) == n:
            return p, s, d, longest
    return p, s, -1, longest


def check_recurrence():
    """The bit-vector recurrence against the quadratic table, and the model walk against both, on small random pairs."""
    rng = random.Random(11)
    for it in range(1500):
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
        l = lcs_table(a, b)
        assert lcs_bits(a, b) == l and lcs_bits(b, a) == l, (a, b)
        d = len(a) + len(b) - 2 * l
        for dmax in (0, 1, 4, 16, 64):
            p, s, got, _ = walk(a, b, dmax)
            assert got == (d if d <= dmax else -1) and (p, s) == ends_and_lcs(a, b)[:2], (a, b, dmax, got, d)


# ---- the smallest shapes that can still go wrong, as given paths over {+-1 .. +-3} ---------------------------------------------
def small_shapes():
    rng = random.Random(5)
    cell = lambda: rng.choice((-1, 1)) * rng.randint(1, 3)
    path = lambda n: [cell() for _ in range(n)]
    x = [1, 2, -3]
    out = [([1], [1]), ([1], [-1]), ([2], [1]), ([1], [1, 2]), ([1, 2], [2, 1]), ([1, 2], [-2, -1]), ([3, 3], [3])]
    for n in (3, 9, 17, 70):
        a, t = path(n), path(5)
        out += [(a, list(a)), (a, a + t), (a + t, a), (a, t + a), (t + a, a), (a, rc(a)), (a + rc(a), a + rc(a))]
        for at in (0, n // 2, n - 1):
            b = list(a); b[at] = -3 if b[at] == 3 else 3
            out.append((a, b))
    out += [(x * 5, x * 7), (x * 7, x * 5), ([2] * 5, [2] * 7)]                       # periodic: the suffix stops at min - prefix
    for snake in (7, 8, 9, 63, 64, 65):                                              # the hand-over and ballot edges
        s, h, t = path(snake), path(4), path(4)
        out += [(h + [1] + s + [2] + t, h + [-1] + s + [-2] + t), (h + [1, 1] + s + t, h + s + [3] + t), ([1] + s + [2], [-1] + s + [-2])]
    out += [(path(3), path(200)), (path(200), path(3)), ([1, 2, 3], path(90) + [1, 2, 3] + path(107)), (path(40), path(140))]
    big = path(2100)                                                                 # two sweep tiles of the device, a snake above 1024
    edited = big[:500] + [3 if big[500] != 3 else -3] + big[501:1700] + big[1701:]
    out += [(big, edited), (big, rc(edited)), (big[:2048], big[:2049]), (big[1:2049], big[:2048])]
    return out


DMAXS = (0, 1, 2, 3, 4, 5, 64, 1024)


def check_small(lib, oracle, workdir, grid=None):
    """Every shape at every cap (the distances 0 .. 6 of the shapes meet dmax and dmax + 1 among them), both ways round; the pair
    (u, u); one side named in many pairs; with `grid`, more pairs than workgroups."""
    it = fp.units(oracle, workdir)[0]
    graphs, b, _ = fp.make_batch(lib, [it])
    b.upload(); b.run(0); b.download()
    final = jc.oracle_path(it[3], 1)
    shapes = small_shapes()
    sides, pairs = [(U(0, 0), jc.oracle_path(it[3], 0), 0), (U(0, 1), final, 0)], [(0, 0), (1, 1), (0, 1)]
    given = []
    for a, c in shapes:
        i = len(sides)
        sides += [(G(len(given)), a, 0), (G(len(given) + 1), c, 0)]
        given += [a, c]
        pairs += [(i, i + 1), (i + 1, i), (i, i)]
    hub = len(sides)                                    # one side named in many pairs
    sides.append((G(len(given)), final[3:20], 0)); given.append(final[3:20])
    pairs += [(hub, k) for k in range(0, hub, 3)] + [(1, hub), (hub, 1)]
    codes = api.compare_all_pairs([s[0] for s in sides[:7]])          # every side against every other: the single-cell case
    assert codes.shape == (21, 2) and codes.dtype == np.int32 and codes[0].tolist() == [U(0, 0), U(0, 1)] and codes[-1].tolist() == [G(3), G(4)]
    every = [(i, j) for i in range(7) for j in range(i + 1, 7)]
    assert codes.tolist() == [[sides[i][0], sides[j][0]] for i, j in every]     # (request() below sends exactly these codes)
    pairs += every
    b.set_compare_paths(given)
    saved = os.environ.pop("AMBI_COMPARE_GRID", None)
    try:
        if grid:
            os.environ["AMBI_COMPARE_GRID"] = str(grid)
        dists = set()
        for dmax in DMAXS:
            got = request(b, sides, pairs, dmax, "small")
            dists |= {(int(d), dmax) for d in got["dist"].reshape(-1)}
    finally:
        os.environ.pop("AMBI_COMPARE_GRID", None)
        if saved is not None:
            os.environ["AMBI_COMPARE_GRID"] = saved
    assert all((d, d) in dists and (-1, d - 1) in dists for d in (1, 2, 3, 4, 5)), sorted(dists)   # a distance of exactly dmax, and of dmax + 1
    assert len(pairs) > 64
    pc.close_all(graphs, b)


# ---- the real units ------------------------------------------------------------------------------------------------------------
def unit_sides(items, reversed_=False):
    """[(code, path or None, status)] of every unit's two paths, index 2 u + which."""
    sides = []
    for u, (name, _, _, oc, orev) in enumerate(items):
        o = orev if reversed_ else oc
        st = fp.unit_status(name, o)
        for which in (0, 1):
            sides.append((U(u, which), jc.oracle_path(o, which) if st >= 0 else None, st))
    return sides


def unit_pairs(items, sides, given_of):
    """path against path_indel of every unit; the final path against the other run's final path as a given path, as is and
    reverse-complemented, both ways round; (u, u); the units with a negative status against a good one and against a given path."""
    pairs, given = [], []
    n_unit = len(sides)
    for u in range(len(items)):
        pairs += [(2 * u, 2 * u + 1), (2 * u + 1, 2 * u + 1)]
        other = given_of(u)
        if other is not None:
            t = len(sides)
            sides += [(G(len(given)), other, 0), (G(len(given) + 1), rc(other), 0)]
            given += [other, rc(other)]
            pairs += [(2 * u + 1, t), (2 * u + 1, t + 1), (t, 2 * u + 1)]
    bad = [i for i in range(n_unit) if sides[i][1] is None]
    assert bad, "a unit with a negative status"
    for i in bad:
        pairs += [(i, 1), (1, i), (i, i), (i, n_unit), (n_unit, i)]
    return pairs, given


def final_of(items, reversed_):
    def f(u):
        name, _, _, oc, orev = items[u]
        o = orev if reversed_ else oc
        return jc.oracle_path(o, 1) if fp.unit_status(name, o) >= 0 else None
    return f


def check_units(lib, oracle, workdir, run_stream=None, req_stream=None):
    """One batch of all units at dmax 64 and 1024; then the same batch run reversed -- other and often shorter paths, so stale cells
    lie behind P -- against the forward run's final paths as given paths."""
    items = fp.units(oracle, workdir)
    graphs, b, _ = fp.make_batch(lib, items)
    b.upload()
    for reversed_ in (False, True):
        b.run(api.FLAG_REVERSED if reversed_ else 0, run_stream)
        if req_stream is None:
            b.download()
        sides = unit_sides(items, reversed_)
        pairs, given = unit_pairs(items, sides, final_of(items, not reversed_))
        b.set_compare_paths(given)
        minus = 0
        for dmax in (64, 1024):
            got = request(b, sides, pairs, dmax, ("units", reversed_), req_stream)
            minus += int((got["dist"][got["status"] == 0] == -1).sum())
        assert minus > 0                                # the cap of 64 is met
        b.download()
        for u, (name, _, _, oc, orev) in enumerate(items):     # precondition: the engine's paths are the oracle's
            o = orev if reversed_ else oc
            if fp.unit_status(name, o) == 0:
                assert b.unit_path(u, 0).tolist() == o["path"] and b.unit_path(u, 1).tolist() == o["path_indel"], name
    pc.close_all(graphs, b)


def check_each_alone(lib, oracle, workdir):
    """Every unit in a batch of its own (the one-unit express path)."""
    for it in fp.units(oracle, workdir):
        graphs, b, _ = fp.make_batch(lib, [it])
        b.upload(); b.run(0); b.download()
        st = fp.unit_status(it[0], it[3])
        sides = unit_sides([it])
        other = jc.oracle_path(it[4], 1) if fp.unit_status(it[0], it[4]) >= 0 else [1, 2, 3]
        sides.append((G(0), other, 0))
        b.set_compare_paths([other])
        for dmax in (64, 1024):
            request(b, sides, [(0, 1), (1, 2), (2, 0), (1, 1)], dmax, ("alone", it[0], st))
        pc.close_all(graphs, b)


def check_request_paths(lib, oracle, workdir, run_stream=None, req_stream=None):
    """The run on one stream, the request on another, without a download in between; a request nobody waited for, then another with
    other pairs and another cap; a new set of given paths between two requests; a batch closed with a request in flight."""
    check_units(lib, oracle, workdir, run_stream, req_stream)
    items = fp.units(oracle, workdir)[:4]
    graphs, b, _ = fp.make_batch(lib, items)
    b.upload(); b.run(0, run_stream)
    sides = unit_sides(items)
    given = [final_of(items, True)(u) for u in range(4)]
    sides += [(G(u), given[u], 0) for u in range(4)]
    pairs = [(2 * u, 2 * u + 1) for u in range(4)] + [(2 * u + 1, 8 + u) for u in range(4)]
    b.set_compare_paths(given)
    b.path_compare([(sides[i][0], sides[j][0]) for i, j in pairs], 1024, req_stream)      # nobody waits for it
    request(b, sides, pairs[::-1], 7, "unwaited", req_stream)
    b.set_compare_paths([[1, 2, 3], [3, 2, 1, -1]])
    sides2 = sides[:8] + [(G(0), [1, 2, 3], 0), (G(1), [3, 2, 1, -1], 0)]
    request(b, sides2, [(8, 9), (1, 8), (9, 3), (0, 1)], 64, "new given paths", req_stream)
    b.run(0, run_stream)
    b.path_compare([(U(0, 0), U(0, 1))], 64, req_stream)
    pc.close_all(graphs, b)
    graphs, b, _ = fp.make_batch(lib, items[::-1])
    b.upload(); b.run(0, run_stream); b.download()
    sides = unit_sides(items[::-1])
    request(b, sides, [(2 * u, 2 * u + 1) for u in range(4)], 1024, "after a close in flight", req_stream)
    pc.close_all(graphs, b)


def check_set_between_request_and_wait(lib, oracle, workdir, run_stream=None, req_stream=None, before_run=None):
    """A request keeps the given paths it was made with.  The set is replaced -- by none, by a smaller one, by one of the same size --
    between a request and its wait, with a run in between: the results' epoch moves, so the engine queues the request again at the
    wait, with the pairs AND the paths of the request.  The next request sees the new set.  before_run: called in front of the run in
    between (a request on another stream than the run's reads the results that run writes: its kernel is let finish first)."""
    items = fp.units(oracle, workdir)[:3]
    graphs, b, _ = fp.make_batch(lib, items)
    b.upload(); b.run(0, run_stream)
    units = unit_sides(items)
    base = len(units)
    old = [final_of(items, True)(u) for u in range(3)] + [[1, 2, 3, -3]]
    sides = units + [(G(t), p, 0) for t, p in enumerate(old)]
    pairs = [(2 * u + 1, base + u) for u in range(3)] + [(base + 3, 1), (base + 3, base + 3), (0, 1)]
    for new in ([], [[3, 2, 1]], [[2, 2], [1], [-1, -2], [3]]):
        b.set_compare_paths(old)
        b.path_compare([(sides[i][0], sides[j][0]) for i, j in pairs], 1024, req_stream)      # nobody waits for it yet
        if before_run:
            before_run()
        b.run(0, run_stream)
        b.set_compare_paths(new)
        b.path_compare_wait()
        got = b.path_compare_results()
        assert len(got) == len(pairs)
        for k, (i, j) in enumerate(pairs):
            want = expected(sides[i][1:], sides[j][1:], 1024)
            assert as_dict(got[k]) == want, ("set between", len(new), k, as_dict(got[k]), want)
        for t in range(len(new), 4):
            with _raises(ERR_ARG):
                b.path_compare([(0, G(t))])                # the new set has fewer paths
        if new:
            now = units + [(G(t), p, 0) for t, p in enumerate(new)]
            request(b, now, [(1, base + t) for t in range(len(new))] + [(base, base)], 64, ("after the new set", len(new)), req_stream)
    pc.close_all(graphs, b)


# ---- floors: what the units must offer for the comparison to mean something (CPU half, from the walk itself) -------------------
def check_floors(oracle, workdir):
    items = fp.units(oracle, workdir)
    dists, capped, snakes, worst = [], 0, [], 0
    for name, _, _, oc, orev in items:
        if fp.unit_status(name, oc) < 0:
            continue
        p0, p1 = jc.oracle_path(oc, 0), jc.oracle_path(oc, 1)
        todo = [(p0, p1, True)]
        if fp.unit_status(name, orev) >= 0:
            r1 = jc.oracle_path(orev, 1)
            todo += [(p1, r1, False), (p1, rc(r1), False)]
        for a, B, indel in todo:
            p, s, d, snake = walk(a, B, 1024)
            want = len(a) + len(B) - 2 * lcs_bits(a, B)
            assert d == want and (p, s) == ends_and_lcs(a, B)[:2], (name, indel, d, want)   # the walk against the recurrence; and no pair is -1 at dmax 1024
            capped += walk(a, B, 64)[2] == -1
            snakes.append(snake); worst = max(worst, d)
            if indel:
                dists.append(d)
    assert {27, 35, 100, 103, 190} <= set(dists), sorted(set(dists))
    assert 0 in dists, "some pair is equal"
    assert capped >= 1, "some pair is -1 at dmax 64"
    assert worst <= 1024, worst                         # (asserted pair by pair above: d == want means the walk found it under the cap)
    assert max(snakes) >= 1024, max(snakes)


# ---- device view ---------------------------------------------------------------------------------------------------------------
def check_device_view(lib, oracle, workdir):
    """ambi_batch_path_compare_device: the block in device memory, read back through torch, is what the host getter returns, byte for
    byte; `bytes` is the 48-byte results padded to 16."""
    import torch
    from ambigram_amd.dist import _DevBytes
    items = fp.units(oracle, workdir)
    graphs, b, _ = fp.make_batch(lib, items)
    stream = torch.cuda.Stream()
    b.upload(); b.run(0, stream.cuda_stream)
    pairs = [(U(u, 0), U(u, 1)) for u in range(len(items))]
    b.path_compare(pairs, 1024, stream.cuda_stream); b.path_compare_wait()
    ptr, nbytes = b.path_compare_device()
    assert ptr and nbytes == (48 * len(pairs) + 15) & ~15
    raw = torch.as_tensor(_DevBytes(ptr, nbytes), device="cuda").cpu().numpy()
    assert raw[:48 * len(pairs)].tobytes() == b.path_compare_results().tobytes()
    pc.close_all(graphs, b)


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def printed(path_abs, bars=()):
    return "".join(("|" if i in bars else "") + "%d%s" % (abs(v), "+" if v > 0 else "-") for i, v in enumerate(path_abs))


def row(tag, lh, c, e):
    return "\t".join([tag, lh, str(c)] + [str(v) for v in (e["status"], e["len_a"], e["len_b"], e["dmax"], *e["prefix"], *e["suffix"], *e["dist"], *e["lcs"])])


def check_cli(lib, exe, cwd, oracle, workdir):
    import test_cli_dropin as t
    items = fp.units(oracle, workdir)
    (_, readme, rsol, roc, rrev), (_, lh2, sol2, oc2, orev2) = items[0], items[1]

    def run(name, lhs, sols, *extra):
        sub = os.path.join(cwd, name)
        os.makedirs(sub)
        bindir = os.path.join(sub, "bin")
        t.fake_cbc(bindir, sols)
        r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", ",".join(lhs), "--lp_prefix", "pc", *extra)
        return sub, bindir, r

    outs = []
    for k, extra in enumerate(([], ["--path_compare", "pc.tsv"])):
        sub, _, r = run("run%d" % k, [readme, lh2], [rsol, sol2], *extra)
        assert r.returncode == 0, r.stderr
        outs.append((r.stdout, r.stderr, open(os.path.join(sub, "simulation_sv.txt"), "rb").read(), sorted(x for x in os.listdir(sub) if x != "bin")))
    assert outs[0][:3] == outs[1][:3]                                      # stdout, stderr, side file: unchanged by the option
    assert outs[1][3] == sorted(outs[0][3] + ["pc.tsv"])
    want = [row("P", lh, 0, expected((jc.oracle_path(oc, 0), 0), (jc.oracle_path(oc, 1), 0), 64)) for lh, oc in ((readme, roc), (lh2, oc2))]
    assert open(os.path.join(cwd, "run1", "pc.tsv")).read().splitlines() == want
    # --truth: the other run's final path as the truth line, `|` anywhere; dmax from the command line
    truth = os.path.join(cwd, "truth.txt")
    for name, lh, sol, oc, orev, dmax in (("t0", readme, rsol, roc, rrev, 3), ("t1", lh2, sol2, oc2, orev2, 1024)):
        with open(truth, "w") as f:
            f.write(printed(orev["path_indel"], bars=(0, 3, 4)) + "\n")
        sub, _, r = run(name, [lh], [sol], "--path_compare", "pc.tsv", "--truth", truth, "--compare_dmax", str(dmax))
        assert r.returncode == 0, r.stderr
        e = expected((jc.oracle_path(oc, 1), 0), (jc.oracle_path(orev, 1), 0), dmax)
        want = [row("P", lh, 0, expected((jc.oracle_path(oc, 0), 0), (jc.oracle_path(oc, 1), 0), dmax)), row("T", lh, 0, e)]
        assert open(os.path.join(sub, "pc.tsv")).read().splitlines() == want
    with open(truth, "w") as f:
        f.write(".\n")
    sub, _, r = run("dot", [readme], [rsol], "--path_compare", "pc.tsv", "--truth", truth)
    assert r.returncode == 0 and [l[0] for l in open(os.path.join(sub, "pc.tsv")).read().splitlines()] == ["P"]
    # refused, exit status 2, no file: an id outside the chromosome, no line, a sample list with --truth, a cap out of range, a PROP C2 sample
    with open(truth, "w") as f:
        f.write("1+2+7+\n")
    bad = [("outside", [readme], [rsol], ["--path_compare", "pc.tsv", "--truth", truth], "outside chromosome"),
           ("list", [readme, lh2], [rsol, sol2], ["--path_compare", "pc.tsv", "--truth", truth], "one sample"),
           ("cap", [readme], [rsol], ["--path_compare", "pc.tsv", "--compare_dmax", "1025"], "--compare_dmax"),
           ("alone", [readme], [rsol], ["--truth", truth], "--path_compare"),
           ("devices", [readme], [rsol], ["--path_compare", "pc.tsv", "--devices", "1"], "--devices")]   # (any --devices takes the sharded run)
    for name, lhs, sols, extra, word in bad:
        sub, _, r = run(name, lhs, sols, *extra)
        assert r.returncode == 2 and word in r.stderr, (name, r.returncode, r.stderr)
        assert r.stdout in ("", "bfb\n") and sorted(os.listdir(sub)) == ["bin"], (name, r.stdout, os.listdir(sub))   # refused in front of anything run or written (stdout: the echo of --op at most)
    for name, text, word in (("noline", "", "no line"), ("nopath", "1+2\n", "is no path"), ("blank", " \n", "is empty")):
        with open(truth, "w") as f:
            f.write(text)
        sub, _, r = run(name, [readme], [rsol], "--path_compare", "pc.tsv", "--truth", truth)
        assert r.returncode == 2 and word in r.stderr, (name, r.returncode, r.stderr)
        assert r.stdout in ("", "bfb\n") and sorted(os.listdir(sub)) == ["bin"], (name, r.stdout, os.listdir(sub))
    c2 = [os.path.join(cases.DATA, "readme_c2_chr0.sol"), os.path.join(cases.DATA, "readme_c2_chr1.sol")]
    for opt, name in (("--path_compare", "pc.tsv"), ("--junc_profile", "junc.tsv")):
        sub, bindir, r = run("c2" + name, [os.path.join(cases.DATA, "readme_c2.lh")], c2, opt, name)
        assert r.returncode == 2 and opt in r.stderr and "PROP I1 / C1 / I2 / C2" in r.stderr, (r.returncode, r.stderr)
        assert not os.path.exists(os.path.join(sub, name))
    r = t.run_cli(exe, sub, bindir, "--help")
    assert "--path_compare" in r.stdout and "--truth" in r.stdout and "--compare_dmax" in r.stdout


# ---- argument and state errors -------------------------------------------------------------------------------------------------
def check_errors(lib, sharded_devices):
    lh, sol = (os.path.join(cases.DATA, "readme6." + x) for x in ("lh", "sol"))
    g = api.Graph(lib, lh); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    pair = [(U(0, 0), U(0, 1))]
    for call in (lambda: b.path_compare(pair), b.path_compare_wait, b.path_compare_results, b.path_compare_device):
        with _raises(ERR_STATE):                           # nothing uploaded
            call()
    b.upload()
    for call in (lambda: b.path_compare(pair), b.path_compare_wait, b.path_compare_results, b.path_compare_device):
        with _raises(ERR_STATE):                           # uploaded, never run
            call()
    b.run(0); b.download()
    with _raises(ERR_STATE):
        b.path_compare_wait()                              # nothing queued
    for dmax in (-1, 1025):
        with _raises(ERR_ARG):
            b.path_compare(pair, dmax)
    for side in (2, 3, -1, -2):                            # one unit, no given path
        for p in ([(side, 0)], [(0, side)], pair + [(1, side)]):
            with _raises(ERR_ARG):
                b.path_compare(p)
    for paths in ([[1, 0, 2]], [[1], []], [[32768]], [[-32768]], [[1, 2], [3, -40000]]):
        with _raises(ERR_ARG):
            b.set_compare_paths(paths)
    with _raises(ERR_ARG):
        b.path_compare([(0, G(0))])                        # a refused set leaves none behind
    b.set_compare_paths([[32767, -32767], [1]])
    b.path_compare([(G(0), G(1)), (G(1), G(1))], 0); b.path_compare_wait()
    got = b.path_compare_results()
    assert got["dist"].tolist() == [[-1, -1], [0, -1]] and got["len_a"].tolist() == [2, 1]
    r = api.PathCompare()
    for k in (2, -1):
        assert lib.ambi_batch_path_compare_result(b.h, k, r) == ERR_ARG
    assert lib.ambi_batch_path_compare_result(b.h, 0, None) == ERR_ARG
    with _raises(ERR_ARG):
        b.path_compare([(0, G(2))])                        # two given paths
    b.set_compare_paths([])
    with _raises(ERR_ARG):
        b.path_compare([(0, G(0))])                        # the set was replaced by none
    b.junc_profile(1); b.junc_profile_wait()
    with _raises(ERR_STATE):
        b.path_compare_results()                           # another kind's request does not answer for this one
    b.path_compare([], 64); b.path_compare_wait()
    assert len(b.path_compare_results()) == 0              # a request without pairs
    b.path_compare(pair, 1024); b.path_compare_wait()
    assert b.path_compare_results()["dist"].tolist() == [[0, 0]]     # readme6: indelBFB changes nothing, the path is a palindrome
    b.run(0)
    with _raises(ERR_STATE):
        b.path_compare_results()                           # a new run: the old results are gone
    b.wait()
    b.close()
    b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    b.run_sharded(0, devices=sharded_devices)
    for call in (lambda: b.path_compare(pair), b.path_compare_wait):
        with _raises(ERR_UNSUPPORTED):                     # a pair may span shares
            call()
    b.close(); g.close()
