"""Random posets through the order-ideal lattice and the WHOLE order table: generators, a plain-Python reference and the checks
shared by the CPU half (host simulation) and the GPU half of tests/test_order_fuzz.py.  Deterministic by seed.

The reference (class Poset) is independent of the engine and of the oracle: on arbitrary-precision integers it counts the
completions of every order ideal (memoised) and unranks / lists the linear extensions in lexicographic order, lowest node number
first -- the order in which allTopologicalOrders (LGM.cpp:3380-3409) emits them.  The DAG it works on is the oracle's
(oracle.run_bfb(..., dag_only=True, max_orders=64)); the engine's unit_dag must equal it, and where the oracle lists orders (the
first 64) the reference must agree with the oracle, so the reference is pinned too.

Every input is a whole .lh + .sol (prepare_checks.lh_text, synth.rank_ab) with a fold-back at every segment, so no unit takes the
shortcut.  Families (FAMILIES): islands, families, random, tall, counts, lattice; the too-big units have builders of their own.

Sizes: no unit whose table is compared has more than ROW_BUDGET rows; a unit is either that small or so large that no arena
holds its table (count-only units: beyond ARENA_CAP; too-big units: beyond 2^48 bytes) -- never between, where the host
simulation would really allocate and fill the table.
"""
import os
import random
import sys

import numpy as np

from ambigram_amd import api, synth

import engine_checks as ec
import prepare_checks as pc

ROW_BUDGET = 300000                # rows of a unit whose table is compared
RANDOM_ROWS_TOTAL = 250000         # rows of the random family together: its seeds are admitted in order while they fit (51 of the 60
                                   # seeds pass ROW_BUDGET, with 1.6 million rows; the batch has room for about 2 million in all)
WHOLE_TABLE = 20000                # up to here every row is compared, above it windows of WINDOW rows
WINDOW = 128
ARENA_CAP = 128 << 20              # AMBI_ARENA_MAX_BYTES of every run but the one that exercises a failed growth
COUNT_SAT = 1 << 62                # csrc/ambi_orders.hpp: kCountSat
TABLE_MAX_BYTES = 1 << 48          # csrc/ambi_stages.hpp: kOrderTableMaxBytes
DEFAULT_LANES = 524288             # csrc/ambi_backend.hpp: target_lanes
ST_ORDERS_CAPACITY, ST_IDEALS_CAPACITY = -15, -16
FAMILIES = ("islands", "families", "random", "tall", "counts", "lattice")
RANDOM_SEEDS = range(0, 60)


def rows_per_lane(total_rows, lanes):
    """csrc/ambi_stages.hpp: rows_per_lane_for, restated (a multiple of 4 in [4, 1024])."""
    t = (total_rows + lanes - 1) // lanes
    return min(1024, max(4, (t + 3) & ~3))


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------
class Poset:
    def __init__(self, succ):
        self.K = K = len(succ)
        self.pred = [0] * K
        for i, s in enumerate(succ):
            for j in range(K):
                if s >> j & 1:
                    self.pred[j] |= 1 << i
        self.full = (1 << K) - 1
        self._cnt, self._av, self._tail = {self.full: 1}, {}, {}
        sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * K + 1000))

    def avail(self, I):
        a = self._av.get(I)
        if a is None:
            a = self._av[I] = [v for v in range(self.K) if not I >> v & 1 and not self.pred[v] & ~I]
        return a

    def count(self, I=0):
        """Completions of the ideal I: linear extensions of what is left (0 if a cycle blocks the way)."""
        c = self._cnt.get(I)
        if c is None:
            c = self._cnt[I] = sum(self.count(I | 1 << v) for v in self.avail(I))
        return c

    def _forced(self, I):
        """The one completion of an ideal that has exactly one."""
        t = self._tail.get(I)
        if t is None:
            t, J = [], I
            while J != self.full:
                v = self.avail(J)[0] if len(self.avail(J)) == 1 else [v for v in self.avail(J) if self.count(J | 1 << v)][0]
                t.append(v)
                J |= 1 << v
            self._tail[I] = t
        return t

    def unrank(self, r):
        I, row = 0, []
        while I != self.full:
            for v in self.avail(I):
                c = self.count(I | 1 << v)
                if r < c:
                    break
                r -= c
            else:
                raise IndexError(r)
            row.append(v)
            I |= 1 << v
        return row

    def rows(self, first, count):
        """Rows first .. first + count - 1 of the table, as a uint8 array."""
        K = self.K
        out = np.empty((count, K), np.uint8)
        prefix, n = [0] * K, [0]

        def walk(I, d, skip):
            if self.count(I) == 1:                      # one completion left (skip is 0 here): the rest of the row is forced
                out[n[0], :d] = prefix[:d]
                out[n[0], d:] = self._forced(I)
                n[0] += 1
                return
            for v in self.avail(I):
                J = I | 1 << v
                c = self.count(J)
                if skip >= c:
                    skip -= c
                    continue
                prefix[d] = v
                walk(J, d + 1, skip)
                skip = 0
                if n[0] >= count:
                    return
        assert 0 <= first and first + count <= self.count()
        if count:
            walk(0, 0, first)
        assert n[0] == count
        return out

    def shape(self):
        """(order ideals, width): after count() every ideal is in the memo; the free nodes of an ideal are an antichain and every
        maximal antichain is the free set of some ideal."""
        self.count()
        return len(self._cnt), max(len(self.avail(I)) for I in self._cnt if I != self.full)


# ---------------------------------------------------------------------------------------------
# units
# ---------------------------------------------------------------------------------------------
def chain(rng, lo, hi, L):
    """L nested loops inside [lo, hi] (hi - lo >= L - 1), each sharing one end with its parent; which end moves is random."""
    assert hi - lo >= L - 1
    a, b = lo, hi
    out = [(True, a, b)]
    for _ in range(L - 1):
        if rng.random() < 0.5:
            a += 1
        else:
            b -= 1
        out.append((True, a, b))
    return out


def chains_side_by_side(rng, lengths, lo=1, gap=1, slack=0):
    """Disjoint chains in segment ranges of their own (no end in common); returns (elements, last segment used)."""
    els = []
    for L in lengths:
        hi = lo + L - 1 + (rng.randint(0, slack) if slack else 0)
        els += chain(rng, lo, hi, L)
        lo = hi + 1 + gap
    return els, lo - 1 - gap


def make_unit(workdir, name, family, n, els, seed=0, expect="table"):
    """els: (is_loop, a, b) on segments 1..n, all different."""
    assert len(set(els)) == len(els) and all(1 <= a <= b <= n for _, a, b in els), name
    rng = random.Random(0xC2B2AE35 * (seed + 7) & 0xFFFFFFFF)
    seg_cn = {i: float(rng.randint(2, 8)) for i in range(1, n + 1)}
    juncs = [(i, '+', i + 1, '+', 1.0) for i in range(1, n)] + [(i, '+', i, '-', 1.0) for i in range(1, n + 1)]
    num_pat = n * (n + 1) // 2
    rows = sorted((synth.rank_ab(a, b, 1, n) + (num_pat if is_loop else 0), 1 if not is_loop else rng.randint(1, 2)) for (is_loop, a, b) in els)
    lh = pc._write(os.path.join(workdir, name + ".lh"), pc.lh_text(name, [(1, n)], seg_cn, juncs))
    sol = pc._write(os.path.join(workdir, name + ".sol"),
                    "Optimal - objective value 0.00000000\n" + "".join("%7d x%-7d %15d %15d\n" % (c, c, v, 0) for c, v in rows))
    n_loops = sum(1 for e in els if e[0])
    u = pc.file_unit(name, lh, 0, sol, (1, n), [], K=len(els), n_loops=n_loops, n_pats=len(els) - n_loops)
    u.update(family=family, expect=expect)
    return u


def oracle_dag(oracle, u):
    """The oracle's DAG of the unit (u["succ"]) and its row width; returns the oracle's record with its first 64 orders."""
    o = oracle.run_bfb(u["lh"], [u["sol"]], keep_orders=True, max_orders=64, dag_only=True)
    assert o["ok"], (u["name"], o["err"])
    oc = o["chr"][0]
    assert not oc["shortcut"] and not oc["infeasible"], u["name"]
    K = len(oc["adj"])
    assert K == u["K"], (u["name"], K)
    u["succ"] = [sum(1 << j for j in set(a)) for a in oc["adj"]]
    u["stride"] = ec.order_row_bytes(K)
    u["cls"] = ec.row_class(K)
    return oc


def attach_reference(oracle, u):
    """The oracle's DAG, the reference on it, and the pin of the reference against the oracle's first orders."""
    oc = oracle_dag(oracle, u)
    P = u["poset"] = Poset(u["succ"])
    R = u["R"] = P.count()
    u["ideals"], u["width"] = P.shape()
    u["bytes"] = R * u["stride"]
    head = min(R, 64)
    assert oc["num_orders"] == head, (u["name"], oc["num_orders"], R)          # (the oracle stops at 64)
    assert P.rows(0, head).tolist() == oc["orders"][:head], (u["name"], "the reference disagrees with the oracle")
    if head:
        assert P.unrank(head - 1) == oc["orders"][head - 1] and P.unrank(0) == oc["orders"][0], u["name"]
    return u


def islands_units(workdir):
    """2..6 disjoint nested chains: the ideal lattice is a product of m chains; antichains of single-segment loops (R = K!)."""
    specs = [(2, 3), (4, 4, 2), (3, 3, 3), (5, 2, 2, 1), (2, 2, 2, 2), (6, 3, 1, 1), (2, 2, 1, 1, 1), (3, 2, 2, 1, 1), (2, 1, 1, 1, 1, 1),
             (9, 3, 2), (12, 2, 2), (7, 5, 1), (20, 2, 1), (15, 3), (4, 3, 2, 1)]
    units = []
    for i, lengths in enumerate(specs):
        rng = random.Random(4100 + i)
        lengths = list(lengths)
        rng.shuffle(lengths)
        els, n = chains_side_by_side(rng, lengths, lo=rng.randint(1, 3), gap=rng.randint(1, 2), slack=2)
        units.append(make_unit(workdir, "oi%d" % i, "islands", n + rng.randint(0, 2), els, seed=i))
    for K in (2, 3, 5, 7, 8):                                       # antichains: 2^K ideals, K! rows
        units.append(make_unit(workdir, "oa%d" % K, "islands", 2 * K, [(True, 2 * j + 1, 2 * j + 1) for j in range(K)], seed=K))
    for K in (11,):                                                 # ... at the ideal capacity (2048 ideals): the count alone, 11! rows have
                                                                    # no room (9! and 10! rows are past the row budget and would fit the arena)
        units.append(make_unit(workdir, "oa%d" % K, "islands", 2 * K, [(True, 2 * j + 1, 2 * j + 1) for j in range(K)], seed=K, expect="count"))
    return units


def families_units(workdir):
    """A root, two end-sharing families, one or two islands inside or outside the root, loop share 1.0 and 0.7 (an element that
    becomes a pattern brings the l -> p parent rule and the p -> l edges into the DAG)."""
    units = []
    for i in range(16):
        rng = random.Random(4300 + i)
        share = 1.0 if i % 2 == 0 else 0.7
        ka, kb = rng.randint(1, 4), rng.randint(1, 4)
        isl = [rng.randint(1, 3) for _ in range(rng.randint(1, 2))]
        inside = [rng.random() < 0.5 for _ in isl]
        room = sum(L + 2 for L, ins in zip(isl, inside) if ins)
        s, e = 2, 2 + ka + kb + room + 3
        els = [(True, s, e)] + [(True, s + k, e) for k in range(1, ka + 1)] + [(True, s, e - k) for k in range(1, kb + 1)]
        lo_in, lo_out = s + ka + 1, e + 2
        for L, ins in zip(isl, inside):
            if ins:
                els += chain(rng, lo_in + 1, lo_in + L, L)
                lo_in += L + 2
            else:
                els += chain(rng, lo_out, lo_out + L - 1, L)
                lo_out += L + 1
        assert lo_in <= e - kb
        els = [(is_loop and rng.random() < share, a, b) for (is_loop, a, b) in els]
        if share < 1.0 and all(e_[0] for e_ in els):
            els[-1] = (False,) + els[-1][1:]
        units.append(make_unit(workdir, "of%d" % i, "families", lo_out + 1, els, seed=i))
    return units


def random_units(workdir):
    """Element sets with their ends drawn from few shared points (as prepare_checks.element_case), K = 6..16; the caller filters
    them by the reference's count."""
    units = []
    for seed in RANDOM_SEEDS:
        rng = random.Random(0x85EBCA6B * (seed + 1) & 0xFFFFFFFF)
        n = (14, 20, 30)[seed % 3]
        K = 6 + seed % 11
        share = (0.0, 0.3, 0.7, 1.0)[(seed // 3) % 4]
        pts = [1, n] + [rng.randint(2, n - 1) for _ in range(2 + K // 8)]
        els = set()
        while len(els) < K:
            a, b = rng.choice(pts + [rng.randint(1, n)]), rng.choice(pts + [rng.randint(1, n)])
            els.add((rng.random() < share, min(a, b), max(a, b)))
        units.append(make_unit(workdir, "or%d" % seed, "random", n, sorted(els), seed=seed))
    return units


TALL_K = (11, 12, 19, 20, 21, 32, 33, 34, 62, 63, 64, 65, 127, 128, 129)


def tall_units(workdir):
    """A nested chain of K - m loops and m = 1..3 free loops that share no end with it: longer than the chain's root (around it:
    low node numbers), of a middle length (beside it) or a single segment (high node numbers).  R = (K-m+1) ... K."""
    units = []
    for i, K in enumerate(TALL_K):
        for rep in range(2):
            rng = random.Random(4500 + 2 * i + rep)
            m = (i + rep) % 3 + 1
            if K >= 62:
                m = min(m, 2)                                        # (rows: K^3 is past what the batch can take there)
            c = K - m
            places = [("low", "mid", "high")[(i + rep + j) % 3] for j in range(m)]
            n_low = places.count("low")
            lo = 1 + n_low + 1                                       # the chain's range, n_low loops around it
            hi = lo + c - 1
            els = chain(rng, lo, hi, c)
            for j in range(n_low):
                els.append((True, lo - 1 - j, hi + 1 + j))          # nested around the chain, no end in common with anything
            nxt = hi + n_low + 2
            for p in places:
                if p == "mid":
                    L = max(2, c // 2)
                    els.append((True, nxt, nxt + L))
                    nxt += L + 2
                elif p == "high":
                    els.append((True, nxt, nxt))
                    nxt += 2
            units.append(make_unit(workdir, "ot%d_%d" % (K, rep), "tall", nxt, els, seed=100 + 2 * i + rep))
    # width 4 at few rows: the innermost loop of the chain spans four segments and has two children (one at either end), two free
    # single-segment loops beside it: R = 2 (K - 1)(K - 2); ideals with four children in every row class from 12 bytes on
    for K in (20, 40, 66, 130):
        rng = random.Random(4600 + K)
        c = K - 4
        els = chain(rng, 1, c + 3, c)
        a, b = els[-1][1], els[-1][2]
        assert b - a == 3
        els += [(True, a, a + 1), (True, b - 1, b), (True, c + 5, c + 5), (True, c + 7, c + 7)]
        units.append(make_unit(workdir, "ot%d_w4" % K, "tall", c + 8, els, seed=200 + K))
    # the largest unit there is, at width 3: 255 nodes, the two children and ONE free loop: R = 2 * 254
    rng = random.Random(4855)
    els = chain(rng, 1, 255, 252)
    a, b = els[-1][1], els[-1][2]
    els += [(True, a, a + 1), (True, b - 1, b), (True, 257, 257)]
    units.append(make_unit(workdir, "ot255_w3", "tall", 258, els, seed=455))
    return units


def _two_chains(workdir, name, family, a, b, seed, expect="table"):
    rng = random.Random(4700 + seed)
    els, n = chains_side_by_side(rng, [a, b])
    return make_unit(workdir, name, family, n, els, seed=seed, expect=expect)


def _chain_and_free(workdir, name, family, c, m, seed, expect="table"):
    rng = random.Random(4800 + seed)
    els, n = chains_side_by_side(rng, [c] + [1] * m)
    return make_unit(workdir, name, family, n, els, seed=seed, expect=expect)


def counts_units(workdir):
    """R = 1, 2, 63, 64, 65 (first_budget / copy_first_rows); either side of 256 (block_max), of 1024 = 256 * T at T = 4 and of
    262144 = 256 * T at T = 1024 (one work block: the in-LDS image build; two: the build kernel); above 65535 (cnt16)."""
    F = "counts"
    return [_chain_and_free(workdir, "oc_r1", F, 5, 0, 1), _two_chains(workdir, "oc_r2", F, 1, 1, 2),
            _chain_and_free(workdir, "oc_r63", F, 62, 1, 3), _chain_and_free(workdir, "oc_r64", F, 63, 1, 4), _chain_and_free(workdir, "oc_r65", F, 64, 1, 5),
            _two_chains(workdir, "oc_r55", F, 9, 2, 6), _two_chains(workdir, "oc_r66", F, 10, 2, 7), _two_chains(workdir, "oc_r70", F, 4, 4, 8),
            _two_chains(workdir, "oc_r253", F, 21, 2, 9), _two_chains(workdir, "oc_r276", F, 22, 2, 10),
            _chain_and_free(workdir, "oc_r240", F, 14, 2, 11), _chain_and_free(workdir, "oc_r272", F, 15, 2, 12),
            _two_chains(workdir, "oc_r990", F, 43, 2, 13), _two_chains(workdir, "oc_r1035", F, 44, 2, 14),
            _chain_and_free(workdir, "oc_r992", F, 30, 2, 15), _chain_and_free(workdir, "oc_r1056", F, 31, 2, 16),
            _two_chains(workdir, "oc_r249900", F, 47, 4, 17), _two_chains(workdir, "oc_r270725", F, 48, 4, 18),
            _chain_and_free(workdir, "oc_r68880", F, 39, 3, 19), _two_chains(workdir, "oc_r92378", F, 10, 9, 20)]


COUNTS_R = dict(oc_r1=1, oc_r2=2, oc_r63=63, oc_r64=64, oc_r65=65, oc_r55=55, oc_r66=66, oc_r70=70, oc_r253=253, oc_r276=276, oc_r240=240, oc_r272=272,
                oc_r990=990, oc_r1035=1035, oc_r992=992, oc_r1056=1056, oc_r249900=249900, oc_r270725=270725, oc_r68880=68880, oc_r92378=92378)


def lattice_units(workdir):
    """Lattice sizes: up to 256 ideals (group-memory search), 257..2048 (HBM search), and one unit above half the default
    ideal_cap: chain of 57 + 6 free nodes, 58 * 64 = 3712 ideals (ST_ERR_IDEALS_CAPACITY; with ideal_cap = 8192 the lattice is
    built, the count is exact, and the table -- 5e10 rows -- has no room)."""
    F = "lattice"
    units = [_chain_and_free(workdir, "ol_248", F, 30, 3, 1), _chain_and_free(workdir, "ol_256", F, 31, 3, 2),      # 31 * 8, 32 * 8 ideals
             _chain_and_free(workdir, "ol_264", F, 32, 3, 3), _chain_and_free(workdir, "ol_328", F, 40, 3, 4),      # 33 * 8, 41 * 8
             _two_chains(workdir, "ol_510", F, 254, 1, 6),                                                           # 255 * 2
             _chain_and_free(workdir, "ol_512", F, 127, 2, 7)]                                                       # 128 * 4
    rng = random.Random(4900)
    els, n = chains_side_by_side(rng, [15, 15, 6])                                 # 16 * 16 * 7 = 1792 ideals, R = 36!/(15! 15! 6!)
    units.append(make_unit(workdir, "ol_1792", F, n, els, seed=8, expect="count"))
    units.append(_chain_and_free(workdir, "ol_over", F, 57, 6, 9, expect="ideals"))
    els, n = chains_side_by_side(rng, [40, 4, 4, 1])                               # 41 * 5 * 5 * 2 = 2050 ideals: just above ideal_cap / 2
    units.append(make_unit(workdir, "ol_2050", F, n, els, seed=10, expect="ideals"))
    return units


def _chains_unit(workdir, name, lengths, seed, expect="toobig"):
    rng = random.Random(5100 + seed)
    els, n = chains_side_by_side(rng, list(lengths))
    return make_unit(workdir, name, "toobig", n, els, seed=seed, expect=expect)


# kind -> chain lengths of its units (disjoint nested chains; R is the multinomial).  What makes a kind is asserted from the
# reference's byte count (too_big_kind): petabytes: above 2^48 and below 2^62 bytes -- representable, never allocatable;
# wrap_negative: R * row bytes in [2^63, 2^64), a negative int64; wrap_positive: 2^64 or more, wrapped to anything; half: below
# 2^63 alone, two of them (the pairs of RUNNING_SUM_PAIRS) pass it: the running sum; saturated: R itself is 2^62 or more.
# Row bytes 20 / 32 / 40 / 128 / 256, ordinary and wide units.
TOO_BIG = dict(
    petabytes=((11, 11, 11), (12, 11, 10), (25, 25), (12, 12, 11)),
    wrap_negative=((30, 31), (28, 34), (22, 42), (18, 56)),
    wrap_positive=((31, 31), (32, 31), (32, 32)),
    half=((30, 30), (30, 30), (29, 32), (29, 32), (21, 43), (12, 116)),
    saturated=((5, 5, 5, 5, 5, 5), (15, 15, 15), (33, 33)))
RUNNING_SUM_PAIRS = ((0, 1), (2, 3), (4, 5))          # indices into TOO_BIG["half"]
SATURATED_IDEAL_CAP = 131072                          # 6^6 = 46656 and 16^3 = 4096 ideals


def too_big_kind(u):
    b = u["bytes"]
    if u["R"] >= COUNT_SAT:
        return "saturated"
    if b >= 1 << 64:
        return "wrap_positive"
    if b >= 1 << 63:
        return "wrap_negative"
    if 2 * b >= 1 << 63:
        return "half"
    return "petabytes" if b > TABLE_MAX_BYTES else None


def too_big_units(workdir):
    """kind -> list of units."""
    out, seed = {}, 0
    for kind, shapes in TOO_BIG.items():
        out[kind] = []
        for j, lengths in enumerate(shapes):
            seed += 1
            out[kind].append(_chains_unit(workdir, "ob_%s_%d" % (kind, j), lengths, seed))
    return out


def unallocatable_unit(workdir):
    """23 + 23: R = C(46,23) = 8.2e12 rows of 28 bytes = 2.3e14 bytes: below 2^48, so the plan wants it, and above 2^47, the
    whole address space of a process, so the growth of the arena fails whatever memory the machine has."""
    return _two_chains(workdir, "ob_23_23", "toobig", 23, 23, 35, expect="toobig")


_CACHE = {}


def family_units(oracle, workdir):
    """Every unit of the six families with its reference, computed once per session; the count-only units last (a table that
    does not fit the arena refuses every table behind it).  Returns (units, facts about the generation)."""
    key = ("families", workdir)
    if key not in _CACHE:
        units = islands_units(workdir) + families_units(workdir) + tall_units(workdir) + counts_units(workdir) + lattice_units(workdir)
        for u in units:
            attach_reference(oracle, u)
        dropped, random_rows = dict(cycle=0, rows=0, ideals=0, total=0), 0
        for u in random_units(workdir):
            attach_reference(oracle, u)
            why = "cycle" if u["R"] == 0 else "rows" if u["R"] > ROW_BUDGET else "ideals" if u["ideals"] > 2048 else \
                  "total" if random_rows + u["R"] > RANDOM_ROWS_TOTAL else None
            if why:
                dropped[why] += 1
            else:
                random_rows += u["R"]
                units.append(u)
        for u in units:
            if u["name"] in COUNTS_R:
                assert u["R"] == COUNTS_R[u["name"]], (u["name"], u["R"])
            if u["expect"] == "table":
                assert 0 < u["R"] <= ROW_BUDGET and u["ideals"] <= 2048, (u["name"], u["R"], u["ideals"])
            elif u["expect"] == "count":
                assert u["bytes"] > ARENA_CAP and u["ideals"] <= 2048, (u["name"], u["bytes"])
            else:
                assert u["ideals"] > 2048, (u["name"], u["ideals"])
        units.sort(key=lambda u: u["expect"] != "table")          # stable
        _CACHE[key] = (units, dict(random_seeds=len(RANDOM_SEEDS), dropped=dropped))
    return _CACHE[key]


def cached(oracle, workdir, name, make):
    key = (name, workdir)
    if key not in _CACHE:
        made = make(workdir)
        for u in ([made] if "lh" in made else [u for v in made.values() for u in v]):
            attach_reference(oracle, u)
        _CACHE[key] = made
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------
# running and checking
# ---------------------------------------------------------------------------------------------
def _ref_rows(u, first, count):
    key = (first, count)
    memo = u.setdefault("_rows", {})
    if key not in memo:
        memo[key] = u["poset"].rows(first, count)
    return memo[key]


def windows(u, Ts):
    """(first, count) of the rows that are compared with the reference."""
    R = u["R"]
    if R <= WHOLE_TABLE:
        return [(0, R)]
    at = {0, R // 3, R // 2, R - WINDOW, 4096 // u["stride"] - WINDOW // 2}
    for T in Ts:
        at |= {k * 256 * T - WINDOW // 2 for k in (1, 2, 3)}
    return sorted((max(0, f), WINDOW) for f in at if max(0, f) + WINDOW <= R)


def table_invariant(b, i, u):
    """Every row a permutation of 0..K-1, the rows strictly increasing (whole table, in slabs that overlap by a row)."""
    R, K, slab = u["R"], u["K"], 32768
    want = np.arange(K, dtype=np.uint8)
    for first in range(0, R, slab):
        rows = b.unit_orders(i, first, min(slab + 1, R - first), K)
        if not np.array_equal(np.sort(rows, axis=1), np.broadcast_to(want, rows.shape)):
            return "a row at %d.. is no permutation" % first
        if len(rows) > 1:
            x, y = rows[:-1].astype(np.int16), rows[1:].astype(np.int16)
            neq = x != y
            fi = neq.argmax(axis=1)
            ii = np.arange(len(x))
            if not (neq.any(axis=1).all() and (x[ii, fi] < y[ii, fi]).all()):
                return "rows at %d.. are not strictly increasing" % first
    return None


def unit_diffs(b, i, u, Ts):
    d = []
    r = b.unit_result(i)
    st, K = r["status"], u["K"]
    ub = u.get("ub_evaluated")                  # (wide_checks: the oracle's own evaluation is undefined at this order -- refused there, behind the table)
    if ub is not None:
        if st != pc.ST_REF_UB or r["evaluated"] != ub:
            return ["status %d at evaluation %d, the oracle is undefined at evaluation %d" % (st, r["evaluated"], ub)]
    elif st not in pc.HAS_DAG:
        return ["status %d: no DAG" % st]
    if r["n_nodes"] != K:
        return ["n_nodes %d, reference %d" % (r["n_nodes"], K)]
    succ = [int(x) for x in b.unit_dag(i, K)[2]]
    if succ != u["succ"]:
        d.append("DAG adjacency")
    if u["expect"] == "ideals":
        if st != ST_IDEALS_CAPACITY:
            d.append("status %d, expected %d" % (st, ST_IDEALS_CAPACITY))
        return d
    if r["num_orders"] != min(u["R"], COUNT_SAT):
        d.append("num_orders %d, reference %d" % (r["num_orders"], u["R"]))
    if u["expect"] == "cycle":                  # (wide_checks: a cyclic relation, R = 0 by the reference)
        if st != api.ST_NO_VALID_ORDER:
            d.append("status %d, expected %d" % (st, api.ST_NO_VALID_ORDER))
        return d
    if u["expect"] != "table":
        if st != ST_ORDERS_CAPACITY:
            d.append("status %d, expected %d" % (st, ST_ORDERS_CAPACITY))
        return d
    if st not in pc.HAS_TABLE and ub is None:
        return d + ["status %d: no table" % st]
    if d:
        return d
    for first, count in windows(u, Ts):
        got = b.unit_orders(i, first, count, K)
        want = _ref_rows(u, first, count)
        if not np.array_equal(got, want):
            bad = int(np.argwhere((got != want).any(axis=1))[0][0])
            return ["row %d: %s, reference %s" % (first + bad, got[bad].tolist(), want[bad].tolist())]
    inv = table_invariant(b, i, u) if u["R"] > WHOLE_TABLE else None      # (a table compared row by row needs no second look)
    return [inv] if inv else []


def run_and_check(lib, units, variant=("default", {}, 0), ideal_cap=0, arena_cap=ARENA_CAP, arena_bytes=-1, env=None):
    """The units as ONE batch through one table variant of engine_checks.TABLE_VARIANTS; returns {name: differences}."""
    tag, venv, lanes = variant
    e = dict(venv)
    e.update(env or {})
    if arena_cap:
        e["AMBI_ARENA_MAX_BYTES"] = arena_cap
    rows = sum(u["R"] for u in units if u["expect"] == "table")
    Ts = sorted({rows_per_lane(rows, lanes or DEFAULT_LANES), 4, 1024})
    bad = {}
    with pc._Env(**e):
        graphs, b = [], api.Batch(lib)
        if lanes or ideal_cap or arena_bytes >= 0:
            b.configure(order_arena_bytes=arena_bytes, ideal_cap=ideal_cap, target_lanes=lanes)
        for u in units:
            g = api.Graph(lib, u["lh"])
            graphs.append(g)
            b.add_chromosome_sol(g, 0, u["sol"])
        b.upload()
        b.run(0); b.wait()
        b.download()
        for i, u in enumerate(units):
            d = unit_diffs(b, i, u, Ts)
            if d:
                bad[u["name"]] = d
        b.close()
        for g in graphs:
            g.close()
    return bad


def assert_clean(bad, what):
    assert not bad, (what, len(bad), dict(list(bad.items())[:6]))


def coverage(units, lanes=DEFAULT_LANES):
    """Facts of the reference and of the formulas restated here only (no engine value)."""
    tab = [u for u in units if u["expect"] == "table"]
    T = rows_per_lane(sum(u["R"] for u in tab), lanes)
    c = dict(units=len(units), tables=len(tab), rows=sum(u["R"] for u in tab), bytes=sum(u["bytes"] for u in tab), T=T,
             width3=sum(u["width"] >= 3 for u in tab), ideals_over_256=sum(u["ideals"] > 256 for u in tab),
             one_block=sum(u["R"] <= 256 * T for u in tab), several_blocks=sum(u["R"] > 256 * T for u in tab),
             windowed=sum(u["R"] > WHOLE_TABLE for u in tab), over_65535=sum(u["R"] > 65535 for u in tab))
    for f in FAMILIES:
        c["family_" + f] = sum(u["family"] == f for u in tab)
    for k in ec.ROW_CLASSES:
        c["class_" + k] = sum(u["cls"] == k for u in tab)
        c["class_%s_width3" % k] = sum(u["cls"] == k and u["width"] >= 3 for u in tab)
    return c
