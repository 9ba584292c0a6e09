"""Random element sets, lattices that are no products of chains, and the capacities of the wide front (units with 64..255 DAG
nodes: csrc/ambi_wide.hpp, stage_prepare_wide and write_wide_row in csrc/ambi_stages.hpp): generators and checks shared by the
CPU half (host simulation) and the GPU half of tests/test_wide_fuzz.py.  Deterministic by seed.

Three families:
  dag      prepare_checks.element_case's generator at K = 64..255: dense random element sets through construct_dag_wide, every
           array bit for bit against the oracle (dag_only); status and count wherever the reference can say them
  lattice  a nested chain of 60..250 elements with 2..6 extras that share an end with a chain member or are free, loop share 1.0
           or 0.7 (order_checks.make_unit): classified BY THE REFERENCE ALONE into table / count / ideals / cycle
  caps     hand-built units on both sides of kWideIdealCap (4096 order ideals) and of kWideMaxOrders (2^20 rows)

The reference for the lattice side is order_checks.Poset on the oracle's DAG, pinned against the oracle's first 64 orders; a
breadth-first walk with a limit (lattice_facts) says "more than 4096 ideals" without counting them all.
"""
import random

import numpy as np

from ambigram_amd import api

import order_checks as oc
import prepare_checks as pc

WIDE_IDEAL_CAP = 4096              # csrc/ambi_wide.hpp: kWideIdealCap
WIDE_LINK_CAP = 16384              #                     kWideLinkCap
WIDE_MAX_ORDERS = 1 << 20          #                     kWideMaxOrders
ROW_BUDGET = 12000                 # rows of a lattice-family unit whose table is compared (the CPU half's time)
SMALL_R = 4096                     # up to here a table unit also goes through the whole run (parity.compare)
CAP_ARENA = 320 << 20              # AMBI_ARENA_MAX_BYTES of the runs that write a table at the row cap (2^20 rows of 256 bytes: 256 MiB)


# ---------------------------------------------------------------------------------------------
# the reference's side of the capacities
# ---------------------------------------------------------------------------------------------
def _preds(succ):
    pred = [0] * len(succ)
    for i, s in enumerate(succ):
        j = 0
        while s:
            if s & 1:
                pred[j] |= 1 << i
            s >>= 1
            j += 1
    return pred


def lattice_facts(succ, limit=WIDE_IDEAL_CAP):
    """(order ideals reachable from the empty one, child links) or None when there are more than `limit` ideals.  An ideal with
    w free nodes has 2^w ideals above it, so a wide antichain ends the walk at once."""
    K = len(succ)
    pred = _preds(succ)
    first = sum(1 << v for v in range(K) if not pred[v])
    seen, frontier, links = {0: first}, [0], 0
    wide = limit.bit_length()                      # 2^wide > limit
    while frontier:
        nxt = []
        for I in frontier:
            free = seen[I]
            if bin(free).count("1") >= wide:
                return None
            m = free
            while m:
                low = m & -m
                m ^= low
                links += 1
                J = I | low
                if J in seen:
                    continue
                if len(seen) >= limit:
                    return None
                f, s = free ^ low, succ[low.bit_length() - 1] & ~J
                while s:
                    w = s & -s
                    s ^= w
                    if not pred[w.bit_length() - 1] & ~J:
                        f |= w
                seen[J] = f
                nxt.append(J)
        frontier = nxt
    return len(seen), links


def reference_lattice(u, succ, orders, num_orders):
    """Fills u with what the reference says about the lattice: over (more ideals or links than a wide unit holds), else poset, R,
    ideals, links, width -- the reference pinned against the oracle's first orders as order_checks.attach_reference does."""
    facts = lattice_facts(succ)
    u["succ"] = succ
    u["over"] = facts is None or facts[1] > WIDE_LINK_CAP
    if facts is None:
        u.update(poset=None, R=None, ideals=None, links=None, width=None)
        return u
    P = u["poset"] = oc.Poset(succ)
    R = u["R"] = P.count()
    ideals, u["width"] = P.shape()
    u["ideals"], u["links"] = facts
    assert ideals == facts[0] + (R == 0), (u["name"], ideals, facts)      # (Poset's memo starts with the full set, which a cycle never reaches)
    head = min(R, 64)
    assert num_orders == head, (u["name"], num_orders, R)
    assert P.rows(0, head).tolist() == orders[:head], (u["name"], "the reference disagrees with the oracle")
    return u


def classify(u, row_budget=ROW_BUDGET):
    if u["over"]:
        return "ideals"
    if u["R"] == 0:
        return "cycle"
    if u["R"] > WIDE_MAX_ORDERS:
        return "count"
    return "table" if u["R"] <= row_budget else "rows"


def attach(oracle, u):
    """order_checks.attach_reference for a unit that may have more ideals than anybody should count."""
    ocr = oc.oracle_dag(oracle, u)
    reference_lattice(u, u["succ"], ocr["orders"], ocr["num_orders"])
    u["cls_lattice"] = classify(u)
    if not u["over"]:
        u["bytes"] = u["R"] * u["stride"]
    return u


# ---------------------------------------------------------------------------------------------
# family 1: random element sets through construct_dag_wide
# ---------------------------------------------------------------------------------------------
DAG_N = (30, 45, 60, 90)
DAG_K = (64, 65, 96, 100, 127, 128, 129, 160, 192, 200, 254, 255)
DAG_SEEDS = range(0, 200)          # 192 = every (n, K, share) once (the crossing drawn), then 8 with the crossing counted up

_CACHE = {}


def dag_units(workdir):
    if ("dag", workdir) not in _CACHE:
        _CACHE[("dag", workdir)] = sorted((pc.element_case(workdir, s, ns=DAG_N, ks=DAG_K, prefix="wd") for s in DAG_SEEDS), key=lambda u: u["K"])
    return _CACHE[("dag", workdir)]


def run_dag_family(lib, workdir, units=None):
    return pc.run_units(lib, dag_units(workdir) if units is None else units, first_budget=1, arena_cap=pc.ARENA_CAP)


def lattice_side_diffs(u, rec, counters):
    """Status and num_orders by the reference's rule; a table that is there need not have fitted the arena of this batch."""
    st, R = rec["status"], rec["header"]["num_orders"]
    cls = classify(u)
    counters["class_" + cls] = counters.get("class_" + cls, 0) + 1
    if cls == "ideals":
        return [] if st == oc.ST_IDEALS_CAPACITY else ["status %d, the reference has more than %d ideals" % (st, WIDE_IDEAL_CAP)]
    d = []
    if R != min(u["R"], oc.COUNT_SAT):
        d.append("num_orders %d, reference %d" % (R, u["R"]))
    if cls == "cycle":
        if st != api.ST_NO_VALID_ORDER:
            d.append("status %d, the reference has no order" % st)
    elif cls == "count":
        if st != oc.ST_ORDERS_CAPACITY:
            d.append("status %d, expected %d" % (st, oc.ST_ORDERS_CAPACITY))
    elif st not in pc.HAS_TABLE + (oc.ST_ORDERS_CAPACITY,):
        d.append("status %d for a unit with %d orders" % (st, u["R"]))
    elif st in pc.HAS_TABLE:
        rows = min(u["R"], pc.ORACLE_ORDERS)
        counters["tables_compared"] += 1
        if rec.get("orders", [])[:rows] != u["poset"].rows(0, rows).tolist():
            d.append("first %d rows of the order table" % rows)
    return d


def dag_diffs(rec, ref):
    d = []
    if rec["status"] not in pc.HAS_DAG:           # (3, ST_NO_VALID_ORDER, is among them: a cyclic relation ends there)
        return ["status %d: no DAG" % rec["status"]]
    if ref["node2pat"] != [[] if r[0] == 0 else r for r in rec["pat"]]:
        d.append("node2pat")
    if ref["node2loop"] != [[] if r[0] == 0 else r for r in rec["loop"]]:
        d.append("node2loop")
    if [sum(1 << j for j in set(a)) for a in ref["adj"]] != rec["succ"]:            # all four words of every successor set
        d.append("DAG adjacency")
    if not np.array_equal(np.array(ref["target_cn"], np.int64), rec["target_cn"][1:]):
        d.append("target_cn")
    return d


def check_dag_family(oracle, units, recs):
    """Every unit the engine did not refuse against the oracle's DAG and junction side and the reference's lattice; returns the
    coverage counters (facts of the generator and of the reference only)."""
    bad = {}
    c = dict(units=len(units), refused=0, refused_by_share={}, per_K={}, loops_over_16=0, loops_over_64=0, mixed=0, tables_compared=0,
             cross=set(), statuses={})
    for u, rec in zip(units, recs):
        c["statuses"][rec["status"]] = c["statuses"].get(rec["status"], 0) + 1
        c["per_K"][u["K"]] = c["per_K"].get(u["K"], 0) + 1
        c["loops_over_16"] += u["n_loops"] > 16
        c["loops_over_64"] += u["n_loops"] > 64
        c["mixed"] += u["n_loops"] > 0 and u["n_pats"] > 0
        c["cross"].add(u["cross"])
        if rec["status"] == pc.ST_REF_UB:
            c["refused"] += 1
            share = round(u["n_loops"] / u["K"], 1)
            c["refused_by_share"][share] = c["refused_by_share"].get(share, 0) + 1
            continue
        ref = pc.oracle_reference(oracle, u)
        if "over" not in u:
            reference_lattice(u, [sum(1 << j for j in set(a)) for a in ref["adj"]], ref["orders"], ref["num_orders"])
        d = pc.junction_side_diffs(u, rec, ref) + dag_diffs(rec, ref) + lattice_side_diffs(u, rec, c)
        if d:
            bad[u["name"]] = d
    c["cross"] = sorted(c["cross"])
    assert not bad, (len(bad), dict(list(bad.items())[:8]))
    assert c["refused"] <= pc.REFUSED_CAP * len(units), c
    return c


# ---------------------------------------------------------------------------------------------
# family 2 (a): a backbone and a few extras
# ---------------------------------------------------------------------------------------------
BACKBONE_SEEDS = range(0, 96)
FEW_PATTERNS = "few"               # one to three elements become patterns (see backbone_unit)


def backbone_unit(workdir, seed):
    """A nested chain of L = 60..250 elements in [lo, hi] and 2..6 extras: an extra keeps the left or the right end of a random
    chain member and gets a random other end, or lies outside the chain's range with no end in common with anything.  Loop share
    1.0 (even seeds) or 0.7: the elements that become patterns bring the l -> p parent rule and the p -> l edges."""
    rng = random.Random(0x27D4EB2F * (seed + 3) & 0xFFFFFFFF)
    share = (1.0, 0.7, 1.0, FEW_PATTERNS, 1.0, FEW_PATTERNS, 1.0, FEW_PATTERNS)[seed % 8]
    L = rng.choice([60, 62, 63, 64, 70, 90, 120, 125, 126, 127, 128, 140, 180, 200, 249, 250])
    m = rng.choice([2, 2, 2, 3, 3, 4, 5, 6] if share != FEW_PATTERNS else [2, 2, 3, 4])
    m = max(min(m, 255 - L), 64 - L)
    lo = 2 + 2 * m
    hi = lo + L - 1 + rng.randint(0, 3)
    els = oc.chain(rng, lo, hi, L)
    have = set((a, b) for _, a, b in els)
    n = hi + 2 * m + 2
    left, right = lo - 2, hi + 2                      # free extras: single segments outward from the chain's range
    kinds = []
    while len(kinds) < m:
        kind = rng.choice(["left", "right", "free", "free"])
        if kind == "free":
            if rng.random() < 0.5:
                a = b = left
                left -= 2
            else:
                a = b = right
                right += 2
        else:
            _, ma, mb = els[rng.randrange(L)]
            if kind == "left":
                a, b = ma, rng.randint(ma, hi)
            else:
                a, b = rng.randint(lo, mb), mb
        if (a, b) in have:
            continue
        have.add((a, b))
        els.append((True, a, b))
        kinds.append(kind)
    if share == FEW_PATTERNS:
        where = range(L, len(els)) if rng.random() < 0.6 else range(len(els))      # among the extras alone, or anywhere
        for i in rng.sample(where, min(len(where), rng.choice([1, 1, 2, 2, 3]))):
            els[i] = (False,) + els[i][1:]
    else:
        els = [(is_loop and rng.random() < share, a, b) for (is_loop, a, b) in els]
        if share < 1.0 and all(e[0] for e in els):
            els[-1] = (False,) + els[-1][1:]
    u = oc.make_unit(workdir, "wb%d" % seed, "backbone", n, els, seed=seed)
    u["extras"], u["share"] = kinds, share
    return u


def backbone_units(oracle, workdir):
    """(units kept, facts): every seed classified by the reference; a unit between the row budget and the row cap is dropped
    ("rows": the host simulation would spend its time writing it), nothing else is."""
    key = ("backbone", workdir)
    if key not in _CACHE:
        units, dropped, classes = [], dict(rows=0), {}
        for s in BACKBONE_SEEDS:
            u = attach(oracle, backbone_unit(workdir, s))
            u["expect"] = u["cls_lattice"]
            if u["expect"] == "table":
                # a node without a record (a pattern leaves one behind) makes the reference's own evaluation undefined: such a unit is
                # refused behind its table, at the evaluation the oracle names
                o = oracle.run_bfb(u["lh"], [u["sol"]], keep_orders=False)["chr"][0]
                if o["ub_valid"]:
                    u["ub_evaluated"] = o["evaluated"]
            classes[u["cls_lattice"]] = classes.get(u["cls_lattice"], 0) + 1
            if u["cls_lattice"] == "rows":
                dropped["rows"] += 1
            else:
                units.append(u)
        units.sort(key=lambda u: u["expect"] != "table")          # stable: the tables first
        _CACHE[key] = (units, dict(seeds=len(BACKBONE_SEEDS), classes=classes, dropped=dropped))
    return _CACHE[key]


def backbone_coverage(units):
    tab = [u for u in units if u["expect"] == "table"]
    has_pat = lambda u: u["n_pats"] > 0
    return dict(units=len(units), table=len(tab), table_K128=sum(u["K"] >= 128 for u in tab), table_width3=sum(u["width"] >= 3 for u in tab),
                table_pattern=sum(has_pat(u) for u in tab), table_small=sum(u["R"] <= SMALL_R for u in tab),
                table_windowed=sum(u["R"] > oc.WHOLE_TABLE for u in tab), table_rows=sum(u["R"] for u in tab), table_bytes=sum(u["bytes"] for u in tab),
                count=sum(u["expect"] == "count" for u in units), ideals=sum(u["expect"] == "ideals" for u in units),
                cycle=sum(u["expect"] == "cycle" for u in units),
                not_a_product=sum(any(k != "free" for k in u["extras"]) for u in tab),
                max_links=max(u["links"] for u in units if not u["over"]))


# ---------------------------------------------------------------------------------------------
# family 2 (b), (c): the capacities, both sides
# ---------------------------------------------------------------------------------------------
def _chains(workdir, name, lengths, seed):
    rng = random.Random(5300 + seed)
    els, n = oc.chains_side_by_side(rng, list(lengths))
    return oc.make_unit(workdir, name, "caps", n, els, seed=seed)


def vee_unit(workdir, name, a, b, seed):
    """One loop around two nested chains of a and b loops, one keeping its left end and one its right end: the two chains have no
    end in common, so the ideals are the empty one and (a + 1)(b + 1) more -- counts that no product of chains gives."""
    N = a + b + 2
    els = [(True, 1, N)] + [(True, 1, N - k) for k in range(1, a + 1)] + [(True, 1 + k, N) for k in range(1, b + 1)]
    return oc.make_unit(workdir, name, "caps", N, els, seed=seed)


def diamonds_unit(workdir, name, d, c, seed):
    """d nested diamonds (i, N+1-i) -> {(i, N-i), (i+1, N+1-i)} -> (i+1, N-i) and a chain of c below the last: R = 2^d exactly."""
    N = 2 * d + 2 + c
    els = set()
    for i in range(1, d + 1):
        els |= {(True, i, N + 1 - i), (True, i, N - i), (True, i + 1, N + 1 - i), (True, i + 1, N - i)}
    els |= {(True, d + 1, N - d - k) for k in range(1, c + 1)}
    return oc.make_unit(workdir, name, "caps", N, sorted(els), seed=seed)


def tree_unit(workdir, name, leaves, c, m, seed):
    """A binary tree of loops over `leaves` segments (a loop, its left part with the same left end, its right part with the same
    right end, down to single segments), a chain of c loops around its root that keep the root's right end, and m free loops.  An
    ideal of the tree has up to `leaves` free nodes: more child links per ideal than a chain with free loops gives."""
    lo = c + 2
    hi = lo + leaves - 1

    def tree(a, b):
        return [(True, a, b)] + (tree(a, (a + b) // 2) + tree((a + b) // 2 + 1, b) if b > a else [])
    els = sorted(set(tree(lo, hi))) + [(True, lo - k, hi) for k in range(1, c + 1)] + [(True, hi + 2 + 2 * k, hi + 2 + 2 * k) for k in range(m)]
    return oc.make_unit(workdir, name, "caps", hi + 2 + 2 * m, els, seed=seed)


# name -> (builder, ideals, class)
IDEAL_CAP_UNITS = dict(
    wc_3050=(lambda w: _chains(w, "wc_3050", (60, 4, 4, 1), 1), 61 * 5 * 5 * 2, "count"),          # between 2049 and 4095: built (ol_2050: the ordinary cap refuses)
    wc_4095a=(lambda w: _chains(w, "wc_4095a", (62, 64), 2), 4095, "count"),
    wc_4095b=(lambda w: _chains(w, "wc_4095b", (64, 8, 6), 3), 4095, "count"),
    wc_4096a=(lambda w: _chains(w, "wc_4096a", (63, 1, 1, 1, 1, 1, 1), 4), 4096, "count"),        # chain of 63 + 6 free, K = 69
    wc_4096b=(lambda w: _chains(w, "wc_4096b", (127, 1, 1, 1, 1, 1), 5), 4096, "count"),          # chain of 127 + 5 free, K = 132
    wc_4096v=(lambda w: vee_unit(w, "wc_4096v", 62, 64, 6), 4096, "count"),                       # 1 + 63 * 65, K = 127
    wc_4096w=(lambda w: vee_unit(w, "wc_4096w", 34, 116, 7), 4096, "count"),                      # 1 + 35 * 117, K = 151
    wc_4097v=(lambda w: vee_unit(w, "wc_4097v", 63, 63, 8), 4097, "ideals"),                      # 1 + 64 * 64: ONE ideal too many, K = 127
    wc_4097w=(lambda w: vee_unit(w, "wc_4097w", 31, 127, 9), 4097, "ideals"),                     # 1 + 32 * 128, K = 159
    wc_4100=(lambda w: _chains(w, "wc_4100", (81, 4, 4, 1), 10), 4100, "ideals"),
    wc_4160=(lambda w: _chains(w, "wc_4160", (64, 1, 1, 1, 1, 1, 1), 11), 4160, "ideals"),        # chain of 64 + 6 free
    # the link cap (kWideLinkCap = 16384) below the ideal cap: 4096 ideals either time
    wl_16384=(lambda w: tree_unit(w, "wl_16384", 2, 59, 6, 12), 4096, "count"),                   # exactly 16384 links: built, K = 68
    wl_16704=(lambda w: tree_unit(w, "wl_16704", 3, 53, 6, 13), 4096, "ideals"))                  # 16704 links: refused, K = 64
LINKS = dict(wc_4096a=16320, wl_16384=16384, wl_16704=16704)
ROW_CAP_REFUSED = dict(
    wr_100_3=(lambda w: _chains(w, "wr_100_3", (100, 1, 1, 1), 21), 101 * 102 * 103),             # 1 061 106
    wr_69_4=(lambda w: _chains(w, "wr_69_4", (69, 4), 22), 1088430))                               # C(73, 4)
ROW_CAP_WRITTEN = dict(
    wr_99_3=(lambda w: _chains(w, "wr_99_3", (99, 1, 1, 1), 31), 100 * 101 * 102),                # 1 030 200 rows of 128 bytes
    wr_68_4=(lambda w: _chains(w, "wr_68_4", (68, 4), 32), 1028790))                               # C(72, 4)
ROW_CAP_EXACT = dict(
    wr_2p20=(lambda w: diamonds_unit(w, "wr_2p20", 20, 10, 33), 1 << 20))                          # exactly kWideMaxOrders, K = 71
ROW_CAP_MID = dict(
    wr_1e5=(lambda w: _chains(w, "wr_1e5", (90, 3), 42), 129766))                                  # C(93, 3): a written table of about 10^5 rows


def cap_units(oracle, workdir, which):
    """The units of one of the tables above with their reference; the stated ideal counts, classes and row counts are asserted."""
    key = ("caps", which, workdir)
    if key not in _CACHE:
        table = dict(ideals=IDEAL_CAP_UNITS, refused=ROW_CAP_REFUSED, written=ROW_CAP_WRITTEN, exact=ROW_CAP_EXACT, mid=ROW_CAP_MID)[which]
        units = []
        for name, spec in table.items():
            u = attach(oracle, spec[0](workdir))
            assert u["name"] == name and u["K"] >= 64, (name, u["K"])
            if which == "ideals":
                if spec[2] == "ideals":
                    assert u["over"] and lattice_facts(u["succ"], limit=1 << 14)[0] == spec[1], name
                else:
                    assert not u["over"] and u["ideals"] == spec[1] and u["R"] > WIDE_MAX_ORDERS, (name, u["ideals"], u["R"])
                assert name not in LINKS or u["links"] == LINKS[name], (name, u["links"])
            else:
                assert not u["over"] and (spec[1] is None or u["R"] == spec[1]), (name, u["R"])
                assert (u["R"] > WIDE_MAX_ORDERS) == (which == "refused"), (name, u["R"])
            u["expect"] = "table" if u["cls_lattice"] == "rows" else u["cls_lattice"]      # (here the tables beyond the row budget are written)
            units.append(u)
        _CACHE[key] = units
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------
# running
# ---------------------------------------------------------------------------------------------
def mixed_batch(oracle, workdir, wide_tables):
    """The wide table units between ordinary units of other row widths (4, 24 and 8 bytes) from the order fuzz."""
    key = ("ordinary", workdir)
    if key not in _CACHE:
        pick = (("oi0", oc.islands_units), ("ot34_0", oc.tall_units), ("oc_r253", oc.counts_units), ("of3", oc.families_units))
        _CACHE[key] = [oc.attach_reference(oracle, next(u for u in make(workdir) if u["name"] == name)) for name, make in pick]
    small = list(_CACHE[key])
    out = []
    for i, u in enumerate(wide_tables):
        out.append(u)
        if i % 4 == 1 and small:
            out.append(small.pop(0))
    return out + small


def whole_run_without_path(lib, u, rev, o):
    """A unit of which the oracle says that no order assembles (record `o` of a full run): the engine evaluates every order too and
    ends with ST_NO_VALID_ORDER; the DAG and the whole table against the reference."""
    d = []
    g = api.Graph(lib, u["lh"])
    b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, u["sol"])
    b.upload(); b.run(api.FLAG_REVERSED if rev else 0); b.download()
    r = b.unit_result(0)
    if (r["status"], r["num_orders"], r["evaluated"], r["bias"]) != (api.ST_NO_VALID_ORDER, o["num_orders"], o["evaluated"], o["bias"]):
        d.append("header %s, oracle: no order of %d after %d evaluations" % (r, o["num_orders"], o["evaluated"]))
    elif [int(x) for x in b.unit_dag(0, u["K"])[2]] != u["succ"]:
        d.append("DAG adjacency")
    elif not np.array_equal(b.unit_orders(0, 0, u["R"], u["K"]), u["poset"].rows(0, u["R"])):
        d.append("order table")
    b.close(); g.close()
    return d


def records(lib, units, arena_cap=oc.ARENA_CAP):
    """prepare_checks.run_units' records of the units as one batch (for the comparison of the two libraries)."""
    return pc.run_units(lib, units, arena_cap=arena_cap)


def same_records(units, hip, host):
    bad = {}
    for u, x, y in zip(units, hip, host):
        d = pc.same_record(x, y)
        if d:
            bad[u["name"]] = d
    assert not bad, ("HIP differs from the host simulation", len(bad), dict(list(bad.items())[:8]))
