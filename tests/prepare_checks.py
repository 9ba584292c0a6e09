"""Random junction sets and random element sets through the prepare stage (getJuncCN, the bias, getIndelBias, the fold-back
shortcut, targetCN, constructDAG): generators and checks shared by the CPU half (host simulation) and the GPU half of
tests/test_prepare_fuzz.py.  Deterministic by seed; files go to `workdir`.

The prepare stage has forms that only a wavefront group takes (`if constexpr (G::kLaneArrays)` in csrc/ambi_prepare.hpp and
csrc/ambi_sort.hpp): the fold-back claim walk over lanes (nfb <= 64), the K x K key ranking, the register replay of the
library sort (LaneWords), the loop-edge pass as one ballot per step, and the junction-order accumulation of shared junction-CN
slots.  The inputs here are shaped to reach every one of them and the sizes at which they change form.

Everything is compared bit for bit (integer work, or f64 in a prescribed order): with the CPU oracle (oracle.run_bfb with
dag_only for files, oracle.prepare_raw for units given as arrays), and the libraries with each other.

Two kinds of unit:
  file  a chromosome of a .lh and a .sol, read by the engine's reader and by the oracle's
  raw   junction arrays handed to ambi_batch_add_unit.  Only this way can a junction-CN slot receive more than two
        contributions: both readers keep one of i+ -> i+1+ and i+1- -> i- (Graph.cpp:489-499 calls them the same junction),
        likewise one of i+1+ -> i+ and i- -> i+1-, and a sum of two f64 values does not depend on their order.
"""
import itertools
import os
import random

import numpy as np

from ambigram_amd import api, synth

HAS_DAG = (0, 3, 4, -15, -16)      # statuses of a unit whose DAG the prepare stage copied out (csrc/ambi_stages.hpp: prep_copy_out)
HAS_TABLE = (0, 3, 4)
ST_REF_UB = -12
ARENA_CAP = 4 << 20                # AMBI_ARENA_MAX_BYTES of the element batches: tables beyond it end with -15, the DAG is still there
ORACLE_ORDERS = 64                 # the oracle stops allTopologicalOrders here

_HEAD = ["AVG_CHR_SEG_DP 30", "AVG_WHOLE_HOST_DP 30", "AVG_JUNC_DP 30", "PURITY 1", "AVG_TUMOR_PLOIDY 2", "PLOIDY 2m1"]


def _f(x):
    return repr(float(x))          # shortest text that reads back as the same f64


def lh_text(name, chr_ranges, seg_cn, juncs):
    """seg_cn: {absolute id: cn}; juncs: (src, sdir, tgt, tdir, cn) with absolute ids and '+' / '-'."""
    n_seg = chr_ranges[-1][1]
    L = ["SAMPLE_NAME %s" % name] + _HEAD + ["VIRUS_START %d" % (n_seg + 1),
                                              "SOURCE " + ",".join(str(s) for s, _ in chr_ranges),
                                              "SINK " + ",".join(str(e) for _, e in chr_ranges)]
    for c, (s, e) in enumerate(chr_ranges):
        for i in range(s, e + 1):
            L.append("SEG H:%d:chr%d:%d:%d 60.0 %s" % (i, c + 1, (i - s) * 1000 + 1, (i - s) * 1000 + 1000, _f(seg_cn[i])))
    for (s, sd, t, td, cn) in juncs:
        L.append("JUNC H:%d:%s H:%d:%s 30.0 %s U B" % (s, sd, t, td, _f(cn)))
    return "\n".join(L) + "\n"


def _write(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    return path


def infeasible_sol(workdir):
    return _write(os.path.join(workdir, "prep_infeasible.sol"), "Infeasible - objective value 0.00000000\n")


# ---------------------------------------------------------------------------------------------
# what a junction list holds, restated here for the coverage counters only (the checks use the oracle)
# ---------------------------------------------------------------------------------------------
def _signed(s, sd, t, td):
    return (s if sd == '+' else -s), (t if td == '+' else -t)


def reader_keeps(juncs):
    """The junctions a reader keeps: the first of every pair that Graph.cpp:489-499 calls the same junction."""
    seen, out = set(), []
    for j in juncs:
        u, v = _signed(*j[:4])
        if (u, v) in seen or (-v, -u) in seen:
            continue
        seen.add((u, v))
        out.append(j)
    return out


def _round(cn):
    return 1.0 if 0.5 < cn < 1 else cn


def order_sensitive(values):
    """Does the sum of the values in the given order differ from their sum in some other order?  (plain f64, numpy)"""
    def total(v):
        s = np.float64(0.0)
        for x in v:
            s = s + np.float64(x)
        return s
    first = total(values)
    return any(total(p) != first for p in itertools.permutations(values))


def junction_stats(juncs):
    """Coverage facts of one chromosome's junction list (local or absolute ids, as long as all lie in the chromosome)."""
    slots, nfb, sv = {}, 0, []
    for pos, (s, sd, t, td, cn) in enumerate(juncs):
        if sd == td:
            if s + 1 == t:
                slots.setdefault(s, []).append(_round(cn))
            elif s - 1 == t:
                slots.setdefault(t, []).append(_round(cn))
            if not ((sd == '+' and t - s == 1) or (sd == '-' and s - t == 1)):
                sv.append(_signed(s, sd, t, td))
        elif abs(s - t) <= 2:
            nfb += 1
    # getIndelBias's grouping (LGM.cpp:3715-3733): one forward pass per group
    chained, far, left = 0, 0, list(enumerate(sv))
    while left:
        group, i, last = [], 0, None
        while i < len(left):
            idx, (s, t) = left[i]
            if not group:
                group = [s, t]
            elif t == group[0]:
                group.insert(0, s)
            elif s == -group[0]:
                group.insert(0, -t)
            elif group[-1] == s:
                group.append(t)
            elif group[-1] == -t:
                group.append(-s)
            else:
                i += 1
                continue
            if last is not None and idx - (last + 1) >= 64:
                far += 1                      # the next link lay beyond the first 64 candidates of the scan
            last = idx
            left.pop(i)
        chained += len(group) > 2
    multi = [v for v in slots.values() if len(v) >= 3 and any(x != int(x) for x in v)]
    return dict(nfb=nfb, nsv=len(sv), chained=chained, far_links=far, slots3=len(multi),
                slots3_sensitive=sum(1 for v in multi if order_sensitive(v)))


# ---------------------------------------------------------------------------------------------
# units
# ---------------------------------------------------------------------------------------------
def file_unit(name, lh, chr_, sol, rng_, juncs_local_kept, K=0, n_loops=0, n_pats=0):
    s, e = rng_
    return dict(kind="file", name=name, lh=lh, chr=chr_, sol=sol, start=s, end=e, n=e - s + 1, K=K, n_loops=n_loops, n_pats=n_pats,
                stats=junction_stats(juncs_local_kept))


def raw_unit(name, n, seg_cn, juncs):
    return dict(kind="raw", name=name, n=n, seg_cn=list(seg_cn), juncs=list(juncs), K=0, n_loops=0, n_pats=0, stats=junction_stats(juncs))


def _one_chr_unit(workdir, name, n, seg_cn, juncs):
    lh = _write(os.path.join(workdir, name + ".lh"), lh_text(name, [(1, n)], seg_cn, juncs))
    return file_unit(name, lh, 0, infeasible_sol(workdir), (1, n), reader_keeps(juncs))


def _adjacencies(n, cn=1.0):
    return [(i, '+', i + 1, '+', cn) for i in range(1, n)]


def junction_case(workdir, seed):
    """A random chromosome: fractional copy numbers, the neighbour junctions in their four strand forms, fold-backs over up to
    two segments in both orientations and written from either side, up to 90 deletions / duplications between a few shared
    points, everything shuffled; the .sol says Infeasible, so the unit ends behind the junction side."""
    rng = random.Random(0x9E3779B1 * (seed + 1) & 0xFFFFFFFF)
    n = rng.choice([3, 5, 17, 63, 64, 65, 130, 200])
    tiny = rng.random() < 0.15               # every fold-back below 1e-6: the serial replay of the sum decides the shortcut

    def cn():
        r = rng.random()
        if r < 0.2:
            return rng.choice([0.5, 1.0, 0.75, 0.5000001, 0.9999999, 2.0, 1.5, 2.5, 3.0, 0.25])
        if r < 0.6:
            return round(rng.uniform(0.05, 4.0), rng.randint(1, 6))
        return rng.uniform(0.01, 6.0)

    seg_cn = {i: rng.uniform(0.5, 8.0) if rng.random() < 0.7 else float(rng.randint(1, 8)) for i in range(1, n + 1)}
    juncs = []
    for i in range(1, n):
        forms = [(i, '+', i + 1, '+'), (i + 1, '+', i, '+'), (i + 1, '-', i, '-'), (i, '-', i + 1, '-')]
        for f in rng.sample(forms, rng.choice([1, 1, 2, 2, 3, 4])):
            juncs.append(f + (cn(),))
    p_fb = rng.choice([0.03, 0.1, 0.2])
    for i in range(1, n + 1):
        for j in range(max(1, i - 2), min(n, i + 2) + 1):
            for sd, td in (('+', '-'), ('-', '+')):
                if rng.random() < p_fb:
                    juncs.append((i, sd, j, td, rng.choice([1e-9, 3e-8, 9.9e-7, 2e-7]) if tiny else cn()))
    pts = [rng.randint(1, n) for _ in range(rng.randint(2, 6))]
    for _ in range(rng.choice([0, 3, 10, 40, 90])):
        a = rng.choice(pts + [rng.randint(1, n)])
        b = rng.choice(pts + [rng.randint(1, n)])
        d = rng.choice("+-")
        juncs.append((a, d, b, d, cn()))
    rng.shuffle(juncs)
    return _one_chr_unit(workdir, "pj%d" % seed, n, seg_cn, juncs)


def shared_slot_units():
    """Raw units: slot 2 of a 6-segment chromosome receives the junctions 2+ -> 3+, 3+ -> 2+, 3- -> 2- and 2- -> 3- (three of
    them in the three-value cases) with values whose f64 sum depends on the order; every other junction of the list is a
    distant strand switch that no prepare scan looks at, apart from two fold-backs and two adjacencies with a slot of their own.
    The list has 255, 256 or 257 junctions, and the contributions sit in lanes of one 64-junction row, in the four rows of one
    256-junction round, across two rounds, and at the very end of the list."""
    forms = [(2, '+', 3, '+'), (3, '+', 2, '+'), (3, '-', 2, '-'), (2, '-', 3, '-')]
    value_sets = [[1e16, 1.0, 1.0, 0.3], [0.3, 1.0, 1e16, 0.7], [0.1, 0.2, 0.3], [0.3, 0.7, 1e16, 2.5], [1.0, 1e16, 0.6, 0.3]]
    units = []
    for m in (255, 256, 257):
        places = {"row": [64 + 3, 64 + 17, 64 + 40, 64 + 63], "rows": [10, 100, 150, 250], "tail": [m - 4, m - 3, m - 2, m - 1],
                  "lane0": [0, 64, 128, 192]}
        if m > 256:
            places["rounds"] = [7, 130, 254, 256]
        for pname, pos in places.items():
            for vi, vals in enumerate(value_sets):
                rng = random.Random(m * 1000 + vi * 10 + len(pname))
                juncs = [None] * m
                for p, f, v in zip(pos, forms, vals):
                    juncs[p] = f + (v,)
                extra = [(4, '+', 5, '+', 0.75), (5, '+', 6, '+', 1.25), (1, '+', 1, '-', 2.5), (6, '-', 5, '+', 1.5)]
                free = [i for i in range(m) if juncs[i] is None]
                for i, j in zip(rng.sample(free, len(extra)), extra):
                    juncs[i] = j
                for i in range(m):
                    if juncs[i] is None:
                        a = rng.randint(1, 3)
                        juncs[i] = (a, '+', a + 3, '-', rng.uniform(0.1, 3.0)) if rng.random() < 0.5 else (a + 3, '-', a, '+', rng.uniform(0.1, 3.0))
                u = raw_unit("slot_m%d_%s_v%d" % (m, pname, vi), 6, [2.0, 3.5, 4.0, 1.0, 2.25, 6.0], juncs)
                u["slot_values"] = [_round(v) for v in vals]
                units.append(u)
    return units


def _foldback_forms(n):
    out = []
    for i in range(1, n + 1):
        for j in range(max(1, i - 2), min(n, i + 2) + 1):
            out += [(i, '+', j, '-'), (i, '-', j, '+')]
    return out


def foldback_count_units(workdir):
    """Exactly 63, 64 and 65 fold-backs on 40 segments (the claim walk changes form behind 64), the claims contested: i+ -> i- and
    i+ -> i+1- in both orders of appearance, then a random fill."""
    units = []
    for count in (63, 64, 65):
        for rep in range(3):
            rng = random.Random(count * 10 + rep)
            n = 40
            juncs = []
            for i in (3, 9, 15, 21):
                pair = [(i, '+', i, '-'), (i, '+', i + 1, '-')]
                juncs += pair if (i // 3) % 2 else pair[::-1]
            forms = _foldback_forms(n)
            rng.shuffle(forms)
            have = reader_keeps([f + (1.0,) for f in juncs + forms])[:count]
            fbs = [f[:4] + (rng.choice([1.0, 2.0, 1.5, 0.7, 2.5, 0.5, 3.25]),) for f in have]
            if rep == 1:
                rng.shuffle(fbs)
            adj = _adjacencies(n, 1.5)
            mixed = fbs + adj if rep == 0 else sorted(fbs + adj, key=lambda _: rng.random())
            seg_cn = {i: 4.0 for i in range(1, n + 1)}
            u = _one_chr_unit(workdir, "pfb%d_%d" % (count, rep), n, seg_cn, mixed)
            assert u["stats"]["nfb"] == count, (count, u["stats"])
            units.append(u)
    return units


def copy_number_unit(workdir):
    """Junction copy numbers around the reference's rounding (0.5 < cn < 1 becomes 1) and fold-back copy numbers with odd and even
    integer parts on fold-backs that join two different segments (the bias counts int(cn) % 2 of those)."""
    n = 16
    vals = [0.5, 0.5000000000000001, 0.75, 0.9999999999999999, 1.0, 1.0000000000000002, 0.49999999999999994, 0.25, 1.5, 2.5, 3.0, 0.7, 2.9999999999999996, 4.2, 5.9]
    juncs = [(i, '+', i + 1, '+', vals[i - 1]) for i in range(1, n)]
    fb = [1.5, 2.5, 3.0, 0.7, 0.5, 2.9999999999999996, 4.2, 5.9, 0.9999999999999999, 1.0000000000000002, 7.5, 0.2]
    for k, v in enumerate(fb):
        i = 1 + k
        juncs.append((i, '+', i + 1, '-', v) if k % 2 else (i + 1, '-', i, '+', v))
    juncs += [(14, '+', 14, '-', 1.5), (15, '-', 15, '+', 0.75)]   # same segment on both sides: not counted by the bias
    return _one_chr_unit(workdir, "pcn", n, {i: 2.0 + 0.125 * i for i in range(1, n + 1)}, juncs)


def tiny_foldback_units(workdir):
    """Every fold-back copy number below 1e-6, so the engine replays the reference's serial sum: a few entries (the sum stays below
    1e-6: shortcut), 200 entries of 9e-9 (1.8e-6: no shortcut), and 99 / 100 / 101 entries of 1e-8 around the threshold itself."""
    units = []
    for name, n, k, v in (("few", 12, 5, 1e-8), ("many", 200, 200, 9e-9), ("at99", 200, 99, 1e-8), ("at100", 200, 100, 1e-8), ("at101", 200, 101, 1e-8)):
        juncs = _adjacencies(n, 1.0) + [(i, '+', i, '-', v) for i in range(1, k + 1)]
        units.append(_one_chr_unit(workdir, "ptiny_" + name, n, {i: 2.0 for i in range(1, n + 1)}, juncs))
    return units


def indel_chain_unit(workdir):
    """getIndelBias with more than 64 SVs: one chain on segments below 40 that grows at the tail and at the head through each of
    the four matching rules, every next link more than 64 list positions behind the previous one; the SVs between them lie on
    segments above 40 and chain among themselves as they fall."""
    n = 130
    rng = random.Random(77)
    links = [(10, '+', 20, '+'), (20, '+', 25, '+'), (5, '+', 10, '+'), (5, '-', 2, '-'), (30, '-', 25, '-')]
    juncs = _adjacencies(n, 2.0) + [(50, '+', 50, '-', 1.0)]
    for link in links:
        juncs.append(link + (1.0,))
        fill = []
        while len(fill) < 70:
            a, b, d = rng.randint(41, n), rng.randint(41, n), rng.choice("+-")
            if (d == '+' and b - a == 1) or (d == '-' and a - b == 1):
                continue
            fill.append((a, d, b, d, rng.choice([1.0, 0.5, 2.25])))
        juncs += fill
    u = _one_chr_unit(workdir, "pindel", n, {i: 9.0 + (i % 4) * 0.25 for i in range(1, n + 1)}, juncs)
    assert u["stats"]["nsv"] > 64 and u["stats"]["far_links"] >= 4 and u["stats"]["chained"] >= 1, u["stats"]
    return u


def hand_built_junction_units(workdir):
    return shared_slot_units() + foldback_count_units(workdir) + [copy_number_unit(workdir)] + tiny_foldback_units(workdir) + [indel_chain_unit(workdir)]


ELEMENT_N = (14, 20, 30, 45)
ELEMENT_K = (1, 2, 15, 16, 17, 18, 31, 32, 33, 47, 62, 63)
ELEMENT_SHARE = (0.0, 0.3, 0.7, 1.0)
ELEMENT_CROSS = (0, 10, 100, 1000)       # the unit's absolute ids straddle this power of ten (0: the chromosome starts at 1)


def element_case(workdir, seed, ns=None, ks=None, prefix="pe"):
    """cases.random_decomposition's .lh (fold-backs everywhere) with a random element set of K in ELEMENT_K elements, a loop share
    in ELEMENT_SHARE, the ends drawn from few shared points (a dense DAG); in multi-chromosome files the unit is the LAST
    chromosome, behind short chromosomes without fold-backs, so that its absolute ids -- the reference's map keys are their
    decimal strings -- straddle 9/10, 99/100 or 999/1000.  Other families give segment counts `ns` (four of them), element
    counts `ks` (twelve) and a name prefix of their own (wide_checks: K = 64..255)."""
    rng = random.Random(0x85EBCA6B * (seed + 1) & 0xFFFFFFFF)
    ns, ks = ns or ELEMENT_N, ks or ELEMENT_K
    assert len(ns) == 4 and len(ks) == 12
    n = ns[seed % 4]
    K = ks[(seed // 4) % 12]
    share = ELEMENT_SHARE[(seed // 48) % 4]
    cross = ELEMENT_CROSS[(seed // 192) % 4] if seed >= 192 else rng.choice(ELEMENT_CROSS)
    start = 1 if cross == 0 else max(1, cross - rng.randint(1, n - 1))
    ranges, lo = [], 1
    while lo < start:                                       # short chromosomes in front: adjacencies only -> shortcut, no .sol
        hi = min(lo + (9 if start <= 100 else 59), start - 1)
        ranges.append((lo, hi))
        lo = hi + 1
    ranges.append((start, start + n - 1))
    base = start - 1
    seg_cn, juncs = {}, []
    for (s, e) in ranges[:-1]:
        for i in range(s, e + 1):
            seg_cn[i] = 2.0
        juncs += [(i, '+', i + 1, '+', 1.0) for i in range(s, e)]
    for i in range(1, n + 1):
        seg_cn[base + i] = float(rng.randint(2, 8))
    local = [(i, '+', i + 1, '+', 1.0) for i in range(1, n)]
    for i in range(1, n + 1):
        r = rng.random()
        if r < 0.4:
            local.append((i, '+', i, '-', float(rng.randint(1, 2))))
        elif r < 0.6 and i < n:
            local.append((i, '+', i + 1, '-', 1.0))
        if rng.random() < 0.4:
            local.append((i, '-', i, '+', 1.0))
    if not any(j[1] != j[3] for j in local):
        local.append((1, '-', 1, '+', 1.0))                 # (never a shortcut: the unit has to reach the DAG)
    juncs += [(a + base, ad, b + base, bd, cn) for (a, ad, b, bd, cn) in local]
    pts = [1, n] + [rng.randint(2, n - 1) for _ in range(2 + K // 8)]
    els = set()
    while len(els) < K:
        a, b = rng.choice(pts + [rng.randint(1, n)]), rng.choice(pts + [rng.randint(1, n)])
        if a > b:
            a, b = b, a
        els.add((rng.random() < share, a, b))
    num_pat = n * (n + 1) // 2
    rows = sorted((synth.rank_ab(a, b, 1, n) + (num_pat if is_loop else 0), 1 if not is_loop else rng.randint(1, 2)) for (is_loop, a, b) in els)
    name = "%s%d" % (prefix, seed)
    lh = _write(os.path.join(workdir, name + ".lh"), lh_text(name, ranges, seg_cn, juncs))
    sol = _write(os.path.join(workdir, name + ".sol"),
                 "Optimal - objective value 0.00000000\n" + "".join("%7d x%-7d %15d %15d\n" % (c, c, v, 0) for c, v in rows))
    n_loops = sum(1 for e in els if e[0])
    u = file_unit(name, lh, len(ranges) - 1, sol, (start, start + n - 1), reader_keeps(local), K=K, n_loops=n_loops, n_pats=K - n_loops)
    u["cross"] = cross
    return u


# ---------------------------------------------------------------------------------------------
# running a list of units as ONE batch
# ---------------------------------------------------------------------------------------------
class _Env:
    def __init__(self, **env):
        self.env, self.saved = {k: str(v) for k, v in env.items()}, {}

    def __enter__(self):
        for k in self.env:
            self.saved[k] = os.environ.get(k)
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


_DIR = {'+': 1, '-': -1}


def run_units(lib, units, first_budget=0, express=False, arena_cap=0):
    """Every unit of the list in one Batch, one upload, one run (express: a second run, which takes the express path when the
    batch is small enough).  Returns one record per unit: the header, unit_prepare's arrays, the DAG and the first rows of the
    order table where the unit has them."""
    env = dict(AMBI_EXPRESS_UNITS=64 if express else 0)
    if arena_cap:
        env["AMBI_ARENA_MAX_BYTES"] = arena_cap
    with _Env(**env):
        graphs, b = {}, api.Batch(lib)
        if first_budget:
            b.configure(first_budget=first_budget)
        for u in units:
            if u["kind"] == "file":
                g = graphs.get(u["lh"])
                if g is None:
                    g = graphs[u["lh"]] = api.Graph(lib, u["lh"])
                assert g.chromosome(u["chr"]) == (u["start"], u["end"]), u["name"]
                b.add_chromosome_sol(g, u["chr"], u["sol"])
            else:
                J = u["juncs"]
                b.add_unit(u["n"], 0, u["seg_cn"], [j[0] for j in J], [j[2] for j in J], [_DIR[j[1]] for j in J], [_DIR[j[3]] for j in J],
                           [j[4] for j in J], [], [], [], [], infeasible=True)
        b.upload()
        b.run(0); b.wait()
        if express:
            b.run(0); b.wait_results(); b.wait()
        b.download()
        out = []
        for i, u in enumerate(units):
            r = dict(b.unit_result(i))
            r.pop("reserved", None)
            rec = dict(header=r, status=r["status"])
            rec.update(b.unit_prepare(i, u["n"]))
            if r["status"] in HAS_DAG:
                pat, loop, succ = b.unit_dag(i, r["n_nodes"])
                rec.update(pat=pat.tolist(), loop=loop.tolist(), succ=[int(x) for x in succ])
            if r["status"] in HAS_TABLE and r["num_orders"] > 0:
                rec["orders"] = b.unit_orders(i, 0, min(r["num_orders"], ORACLE_ORDERS), r["n_nodes"]).tolist()
            out.append(rec)
        b.close()
        for g in graphs.values():
            g.close()
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_record(x, y, arena_independent_only=False):
    """Differences between two libraries' (or two paths') records of one unit; bit patterns for the f64 arrays."""
    d = []
    for k in ("junc_cn", "seg_cn"):
        if not np.array_equal(_bits(x[k]), _bits(y[k])):
            d.append(k)
    for k in ("target_cn", "inv_junc"):
        if not np.array_equal(x[k], y[k]):
            d.append(k)
    for k in ("pat", "loop", "succ"):
        if x.get(k) != y.get(k):
            d.append(k)
    hx, hy = dict(x["header"]), dict(y["header"])
    if arena_independent_only and -15 in (hx["status"], hy["status"]):
        # whether a table fits the arena depends on the units in front of it in the batch: what does not, is compared
        keep = ("bias", "n_nodes", "inv_cn_sum")
        hx, hy = {k: hx[k] for k in keep}, {k: hy[k] for k in keep}
    elif arena_independent_only and hx["status"] < 0 and hx["status"] == hy["status"]:
        # a unit the lattice stage ends with an error behind the express stage keeps the lengths of the path the express stage
        # had written; that path is void (csrc/ambi_stages.hpp: stage_lattice, plan_merge_lattice) and the chain never wrote one
        keep = ("status", "bias", "n_nodes", "num_orders", "inv_cn_sum")
        hx, hy = {k: hx[k] for k in keep}, {k: hy[k] for k in keep}
    elif x.get("orders") != y.get("orders"):
        d.append("orders")
    if hx != hy:
        d.append("header %s" % {k: (hx[k], hy[k]) for k in hx if hx[k] != hy[k]})
    return d


# ---------------------------------------------------------------------------------------------
# the oracle's answer for a unit, and the comparison
# ---------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_reference(oracle, u):
    """Computed once per unit (by name and file) and shared by every test of the session."""
    key = (u["name"], u.get("lh"))
    if key not in _ORACLE:
        if u["kind"] == "raw":
            J = u["juncs"]
            _ORACLE[key] = oracle.prepare_raw(u["seg_cn"], [j[0] for j in J], [_DIR[j[1]] for j in J], [j[2] for j in J],
                                              [_DIR[j[3]] for j in J], [j[4] for j in J])
        else:
            o = oracle.run_bfb(u["lh"], [u["sol"]], keep_orders=True, max_orders=ORACLE_ORDERS, dag_only=True)
            assert o["ok"], (u["name"], o["err"])
            oc = o["chr"][u["chr"]]
            assert (oc["start"], oc["end"]) == (u["start"], u["end"]), u["name"]
            assert all(c["shortcut"] for c in o["chr"][:u["chr"]]), u["name"]   # (the .sol went to this chromosome)
            oc["target_cn"] = o["target_cn"][u["start"] - 1:u["end"]]
            _ORACLE[key] = oc
    return _ORACLE[key]


def junction_side_diffs(u, rec, ref):
    """junc_cn, seg_cn after getIndelBias, the fold-back map, the bias and the status, as parity.compare takes them."""
    d = []
    n = u["n"]
    if u["kind"] == "raw":
        want_jc, want_sc = ref["junc_cn"][1:], ref["seg_cn"][1:]
        want_inv = {i: int(j) for i, j in enumerate(ref["inv_junc"]) if j >= 0}
        got_inv = {i: int(j) for i, j in enumerate(rec["inv_junc"]) if i >= 1 and j >= 0}
        shortcut, infeasible = abs(ref["inv_sum"]) < 0.000001, True
    else:
        s = u["start"]
        want_jc = np.array(ref["junc_cn"], np.float64).reshape(-1, 2)[s:]
        want_sc = np.array(ref["seg_cn"], np.float64)[s - 1:u["end"]]
        want_inv = dict(zip(ref["inv_seg"], ref["inv_junc"]))
        got_inv = {s - 1 + i: int(j) for i, j in enumerate(rec["inv_junc"]) if i >= 1 and j >= 0}
        shortcut, infeasible = ref["shortcut"], ref["infeasible"]
    if not np.array_equal(_bits(want_jc), _bits(rec["junc_cn"][1:])):
        bad = np.argwhere(_bits(want_jc) != _bits(rec["junc_cn"][1:]))[0]
        d.append("junc_cn[%d][%d] %r, oracle %r" % (bad[0] + 1, bad[1], rec["junc_cn"][1:][tuple(bad)], want_jc[tuple(bad)]))
    if not np.array_equal(_bits(want_sc), _bits(rec["seg_cn"][1:])):
        d.append("seg_cn after getIndelBias")
    if want_inv != got_inv:
        d.append("fold-back map: %s" % sorted(set(want_inv.items()) ^ set(got_inv.items()))[:6])
    fb = np.array(want_jc)[:, 1]
    if fb.max() < 0.000001:      # every entry tiny: the engine replays the reference's serial sum (no_foldback_g) and reports it
        total = 0.0
        for v in fb:
            total += float(v)
        if _bits([total])[0] != _bits([rec["header"]["inv_cn_sum"]])[0]:
            d.append("fold-back sum %r, in the reference's order %r" % (rec["header"]["inv_cn_sum"], total))
    if ref["bias"] != rec["header"]["bias"]:
        d.append("bias %d, oracle %d" % (rec["header"]["bias"], ref["bias"]))
    if shortcut:
        if rec["status"] != api.ST_SHORTCUT:
            d.append("status %d, oracle: shortcut" % rec["status"])
    elif infeasible:
        if rec["status"] != api.ST_INFEASIBLE:
            d.append("status %d, oracle: infeasible" % rec["status"])
    elif rec["status"] in (api.ST_SHORTCUT, api.ST_INFEASIBLE):
        d.append("status %d, oracle: neither shortcut nor infeasible" % rec["status"])
    return d


def element_side_diffs(u, rec, ref, counters):
    d = []
    if rec["status"] not in HAS_DAG:
        return ["status %d: no DAG" % rec["status"]]
    if ref["node2pat"] != [[] if r[0] == 0 else r for r in rec["pat"]]:
        d.append("node2pat")
    if ref["node2loop"] != [[] if r[0] == 0 else r for r in rec["loop"]]:
        d.append("node2loop")
    if [sum(1 << j for j in set(a)) for a in ref["adj"]] != rec["succ"]:
        d.append("DAG adjacency")
    if not np.array_equal(np.array(ref["target_cn"], np.int64), rec["target_cn"][1:]):
        d.append("target_cn")
    R = rec["header"]["num_orders"]
    if rec["status"] != -16:                                    # (-16: the lattice outgrew its table and the count was never finished -- also the end of a graph with a cycle, whose count is 0)
        if ref["num_orders"] < ORACLE_ORDERS:
            counters["counts_compared"] += 1
            if R != ref["num_orders"]:
                d.append("num_orders %d, oracle %d" % (R, ref["num_orders"]))
        elif R < ORACLE_ORDERS:
            d.append("num_orders %d, oracle at least %d" % (R, ORACLE_ORDERS))
    if rec["status"] in HAS_TABLE:
        rows = min(R, len(ref["orders"]))
        counters["tables_compared"] += 1
        if rec.get("orders", [])[:rows] != ref["orders"][:rows]:
            d.append("first %d rows of the order table" % rows)
    return d


# ---------------------------------------------------------------------------------------------
# the two families
# ---------------------------------------------------------------------------------------------
JUNCTION_SEEDS = range(0, 80)
ELEMENT_SEEDS = range(0, 200)
REFUSED_CAP = 0.02       # share of element units the engine may refuse as ST_ERR_REF_UB (they are not sent to the oracle: its
                         # real std::sort would be off its contract)

_UNITS = {}


def junction_units(workdir):
    if ("j", workdir) not in _UNITS:
        _UNITS[("j", workdir)] = [junction_case(workdir, s) for s in JUNCTION_SEEDS] + hand_built_junction_units(workdir)
    return _UNITS[("j", workdir)]


def element_units(workdir):
    """Sorted by K: the arena limit refuses every table behind the first one that does not fit, so the small units go first."""
    if ("e", workdir) not in _UNITS:
        _UNITS[("e", workdir)] = sorted((element_case(workdir, s) for s in ELEMENT_SEEDS), key=lambda u: u["K"])
    return _UNITS[("e", workdir)]


def run_junction_family(lib, workdir, express=False, units=None):
    return run_units(lib, junction_units(workdir) if units is None else units, express=express)


def run_element_family(lib, workdir, express=False, units=None):
    return run_units(lib, element_units(workdir) if units is None else units, first_budget=1, express=express, arena_cap=ARENA_CAP)


def check_junction_family(oracle, units, recs):
    """Every unit against the oracle; returns the coverage counters."""
    bad = {}
    c = dict(units=len(units), slots3=0, slots3_sensitive=0, nfb_over_64=0, nfb_63_64_65=set(), chained=0, far_links=0, nsv_over_64=0,
             shortcut_replay=0, tiny_no_shortcut=0, fractional_sums=0, bias_over_1=0)
    for u, rec in zip(units, recs):
        ref = oracle_reference(oracle, u)
        d = junction_side_diffs(u, rec, ref)
        if d:
            bad[u["name"]] = d
        st = u["stats"]
        if "slot_values" in u:
            # the case discriminates only if the order of the additions matters for its values
            assert order_sensitive(u["slot_values"]), u["name"]
            want = np.float64(0.0)
            for v in u["slot_values"]:
                want = want + np.float64(v)
            assert _bits([ref["junc_cn"][2][0]])[0] == _bits([want])[0], (u["name"], ref["junc_cn"][2][0], want)   # the oracle adds in junction order
        c["slots3"] += st["slots3"] > 0
        c["slots3_sensitive"] += st["slots3_sensitive"] > 0
        c["nfb_over_64"] += st["nfb"] > 64
        if st["nfb"] in (63, 64, 65):
            c["nfb_63_64_65"].add(st["nfb"])
        c["chained"] += st["chained"] > 0
        c["far_links"] += st["far_links"] > 0
        c["nsv_over_64"] += st["nsv"] > 64
        fb = rec["junc_cn"][1:, 1]
        tiny = st["nfb"] > 0 and fb.max() > 0 and fb.max() < 0.000001
        c["shortcut_replay"] += bool(tiny and rec["status"] == api.ST_SHORTCUT)
        c["tiny_no_shortcut"] += bool(tiny and rec["status"] != api.ST_SHORTCUT)
        c["fractional_sums"] += bool(np.any(rec["junc_cn"][1:, 0] != np.floor(rec["junc_cn"][1:, 0])))
        c["bias_over_1"] += rec["header"]["bias"] > 1
    c["nfb_63_64_65"] = sorted(c["nfb_63_64_65"])
    assert not bad, (len(bad), dict(list(bad.items())[:8]))
    return c


def check_element_family(oracle, units, recs):
    """Every unit the engine did not refuse against the oracle's DAG; returns the coverage counters."""
    bad = {}
    c = dict(units=len(units), refused=0, loops_over_16=0, mixed_over_16=0, K_over_16=0, counts_compared=0, tables_compared=0,
             cross=set(), statuses={})
    for u, rec in zip(units, recs):
        c["statuses"][rec["status"]] = c["statuses"].get(rec["status"], 0) + 1
        if rec["status"] == ST_REF_UB:
            c["refused"] += 1
            continue
        ref = oracle_reference(oracle, u)
        d = junction_side_diffs(u, rec, ref) + element_side_diffs(u, rec, ref, c)
        if d:
            bad[u["name"]] = d
        c["loops_over_16"] += u["n_loops"] > 16
        c["K_over_16"] += u["K"] > 16
        c["mixed_over_16"] += u["K"] > 16 and u["n_loops"] > 0 and u["n_pats"] > 0
        c["cross"].add(u["cross"])
    c["cross"] = sorted(c["cross"])
    assert not bad, (len(bad), dict(list(bad.items())[:8]))
    assert c["refused"] <= REFUSED_CAP * len(units), c
    return c
