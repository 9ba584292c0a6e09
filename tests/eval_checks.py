"""High copy numbers and random fold-back maps through the per-order evaluation (getBFB's placement, LGM.cpp:3519-3646, and
imperfectFBI, :3431-3512): generators, a plain walk of both with a counter on every branch, and the runners shared by the CPU half
(host simulation) and the GPU half of tests/test_eval_fuzz.py.  Deterministic by seed; files go to `workdir`.

The evaluation exists in three device forms -- the wavefront form in group memory (eval_place / imperfect_fbi), one thread per
order (eval_order_lane / imperfect_fbi_lane; --all, bkp_cap <= 192) and the register form of the express kernel
(eval_place_regs_n<1|2|4> by bkp_cap <= 64 / 128 / 256, imperfect_fbi_regs_n<1|2> by L <= 64 / 128).  The register form is device
code only: the host simulation never runs it.  The units here are shaped for what decides between the forms and inside them: the
final length of the breakpoint path, inserts of 64 cells and more, slots at the last lane of a register, palindromes across a
register boundary, and fold-back maps under which imperfectFBI really rewrites cells.

Placement reads only the DAG, imperfectFBI only the breakpoint cells and the fold-back map; a junction enters that map when its
strands are opposite and |src - tgt| <= 2 (LGM.cpp:3996-4049).  So every unit is a planted decomposition whose fold-back junctions
are either the perfect ones or a random set, and stays valid.  Everything is compared bit for bit with oracle.run_bfb.
"""
import os
import random

from ambigram_amd import api, synth
from ambigram_amd.synth import Element

BIG = (3, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
ALL_MAX_R = 70


# ---------------------------------------------------------------------------------------------
# the plain walk: placement (LGM.cpp:3519-3646) and imperfectFBI (:3431-3512) on Python lists, statement by statement
# ---------------------------------------------------------------------------------------------
def bkp_capacity(elements):
    """The engine's capacity of a unit's breakpoint path: four cells per loop copy, two per pattern, rounded up to eight."""
    return max(4, (sum(4 * e.cn if e.kind == 'l' else 2 for e in elements) + 7) & ~7)


def _nr(cap):
    return "nr1" if cap <= 64 else "nr2" if cap <= 128 else "nr4" if cap <= 256 else "lds"


def _rfind(bkp, v, hi):
    """std::find on reverse iterators from index hi downwards: the index, or -1 (rend)."""
    for q in range(hi, -1, -1):
        if bkp[q] == v:
            return q
    return -1


def place_walk(node2pat, node2loop, order, forward, cap, c, own_register=False):
    """Returns (bkp, placed).  c: dict of facts of this run, raised in place.  own_register: NOT the reference -- the nesting test
    of a candidate at lane 63 reads the cell 64 places lower, as a register form that forgot the next register would; make_unit
    uses it to tell whether a unit would notice."""
    def bump(k, by=1):
        c[k] = c.get(k, 0) + by

    regs = cap <= 256
    bkp = []
    x = order[0]
    if node2pat[x]:
        start, end = node2pat[x][0], node2pat[x][1]
        bkp += [start, end] if forward else [-end, -start]
    else:
        start, end, cn = node2loop[x][0], node2loop[x][1], node2loop[x][2]
        for _ in range(cn):                                            # :3533-3540 / :3559-3566
            bkp += [start, end, -end, -start] if forward else [-end, -start, start, end]
        if regs and len(bkp) >= 64:
            bump("seed_ge_64")
        if regs and len(bkp) >= 128:
            bump("seed_ge_128")
    i = 1
    while i < len(order):
        x = order[i]
        if node2pat[x]:                                                # :3572-3585
            start, end = node2pat[x][0], node2pat[x][1]
            if len(bkp) in (64, 128, 256):
                bump("pat_at_%d" % len(bkp))
            if bkp[-1] == -start:
                bkp += [start, end]; bump("pat_arm_start")
            elif bkp[-1] == end:
                bkp += [-end, -start]; bump("pat_arm_end")
            else:
                break
        elif node2loop[x]:                                             # :3586-3644
            start, end, cn = node2loop[x][0], node2loop[x][1], node2loop[x][2]
            L = len(bkp)

            def search(v, less, tag):
                pos = _rfind(bkp, v, L - 1)
                while pos >= 0:
                    even = pos % 2 == 0           # (rend - pos) % 2 == 1
                    nest = False
                    if not even and pos < L - 2:  # pos - rbegin > 1
                        a, b = abs(bkp[pos - 1]), abs(bkp[pos + 2])
                        nest = a < b if less else a > b
                        if regs and pos % 64 == 63:
                            bump("lane63_%s_%s" % (tag, "skipped" if nest else "passed"))
                            # ... and the cell 64 places lower (the same lane of the candidate's OWN register) would decide otherwise
                            other = abs(bkp[pos + 2 - 64])
                            if (a < other if less else a > other) != nest:
                                bump("lane63_%s_decisive" % tag)
                                if own_register:
                                    nest = not nest
                        if nest:
                            bump("nest_skip_" + tag)
                    if not even and not nest:
                        return pos
                    pos = _rfind(bkp, v, pos - 1)
                return -1

            f = search(-start, True, "s")
            via_s = f >= 0
            if not via_s:
                f = search(end, False, "e")
            if f < 0:
                break
            cnt = 4 * cn
            bump("via_s_" + _nr(cap) if via_s else "via_e_" + _nr(cap))
            if regs:
                if cnt >= 64:
                    bump("insert_ge_64")
                if cnt >= 128:
                    bump("insert_ge_128")
                if cnt % 64 == 0:
                    bump("insert_mod_64")
                if L > f + 1 and (L - 1) // 64 - (f + 1) // 64 >= 2:
                    bump("moved_three_regs")
                if f % 64 == 63:
                    bump("behind_lane_63")
                if cnt >= 12:
                    for lane in (1, 61, 63):
                        if f % 64 == lane:
                            bump("big_behind_lane_%d" % lane)
            if f + 1 == L:
                bump("insert_at_end")
                if cnt >= 12:
                    bump("big_at_end")
            if L - (f + 1) > 512:
                bump("shift_two_rounds")          # shift_up moves 8 x 64 cells per round on a wavefront
            if L - (f + 1) > 1024:
                bump("shift_three_rounds")
            if via_s:                                                  # :3617-3629
                loop = [start, end, -end, -start] * cn
                bkp[f] = -start
                if f + 1 != L:
                    bkp[f + 1] = start
            else:                                                      # :3630-3642
                loop = [-end, -start, start, end] * cn
                bkp[f] = end
                if f + 1 != L:
                    bkp[f + 1] = -end
            bkp[f + 1:f + 1] = loop
        i += 1
    return bkp, i


def fbi_walk(bkp, inv, c):
    """imperfectFBI.  inv: {segment: (source id, target id)}.  Returns the rewritten cells, or None where the reference reads
    behind the end.  c: facts of this run."""
    def bump(k, by=1):
        c[k] = c.get(k, 0) + by

    b = list(bkp)
    L = len(b)
    pos = 0
    last_changed = {}           # cells that the p1 = pos - 1 iteration of the palindrome just before changed, with what they held

    def rewrite(v):
        if abs(v) not in inv:
            return None
        s, t = inv[abs(v)]
        return ((s, -t) if s < t else (t, -s)) if v > 0 else ((-t, s) if s < t else (-s, t))

    prev_changed = set()        # cells that any of its iterations changed
    while pos < L:
        if pos + 1 >= L:
            return None
        r = L
        for q in range(pos + 3, L):
            if b[q] == -b[pos]:
                r = q
                break
        l = r - 1
        if r == L or b[l] != -b[pos + 1]:
            bump("plain_steps")
            before = (b[pos], b[pos + 1])
            idn = abs(b[pos + 1])
            if idn in inv:                                             # :3444-3457
                s, t = inv[idn]
                b[pos + 1] = (s if s < t else t) if b[pos + 1] > 0 else (-t if s < t else -s)
            if pos > 0:                                                # :3458-3468
                idn = abs(b[pos])
                if idn in inv and abs(b[pos - 1]) == idn:
                    s, t = inv[idn]
                    other = t if s == idn else s
                    bump("n0_taken")
                    if other != idn:
                        bump("n0_changes")
                    b[pos] = other if b[pos] > 0 else -other
            if b[pos] > 0 and abs(b[pos]) > abs(b[pos + 1]):           # :3469
                b[pos + 1] = b[pos]; bump("adjustments")
            if b[pos] < 0 and abs(b[pos]) < abs(b[pos + 1]):           # :3470
                b[pos + 1] = b[pos]; bump("adjustments")
            if (b[pos], b[pos + 1]) != before:
                bump("plain_changes")
            last_changed, prev_changed = {}, set()
            pos += 2
        else:
            bump("palindromes")
            single = b[pos + 2] == -b[pos]       # a loop on ONE segment (a a -a -a): the cell two behind pos already holds -cell[pos]
            if pos <= 63 and r >= 64:
                bump("straddle_63_64")
            if pos <= 127 and r >= 128:
                bump("straddle_127_128")
            p1 = pos + (l - pos) // 2
            p2 = p1 + 1
            iters, any_change, mirrored, mine, every = 0, False, False, {}, set()
            while p1 >= pos - 1 and p1 > 0:
                iters += 1
                if p1 == pos - 1 and p1 in prev_changed:
                    bump("last_reads_changed")             # ... a cell that some iteration of the palindrome before changed
                if p1 == pos - 1 and p1 in last_changed:
                    bump("last_reads_last_write")          # ... that its LAST iteration changed (what the register form calls a conflict)
                    if rewrite(last_changed[p1]) != rewrite(b[p1]):
                        bump("last_reads_last_write_decisive")     # ... and the cell as it stood before would be rewritten differently
                idn = abs(b[p1])
                if idn in inv:
                    s, t = inv[idn]
                    if p1 + 1 >= L:
                        return None
                    if b[p1] > 0:
                        w0, w1 = (s, -t) if s < t else (t, -s)
                    else:
                        w0, w1 = (-t, s) if s < t else (-s, t)
                    writes = [(p1, w0), (p1 + 1, w1)]
                    if p2 != p1 + 1:
                        if p1 > pos - 1:
                            if p2 >= L:
                                return None
                            writes.append((p2, -w0))
                        writes.append((p2 - 1, -w1))
                    for k, (q, v) in enumerate(writes):
                        if b[q] != v:
                            any_change = True
                            every.add(q)
                            if k >= 2:
                                mirrored = True
                            if p1 == pos - 1:
                                mine.setdefault(q, b[q])
                        b[q] = v
                    if p1 == pos - 1 and mine:
                        bump("last_changes")
                p1 -= 2
                p2 += 2
            if any_change:
                bump("pal_changes")
                if single:
                    bump("single_segment_pal_changes")
            if mirrored:
                bump("pal_mirrored_changes")
            if iters > 64:
                bump("pal_over_64_iterations")
            last_changed, prev_changed = mine, every
            pos = r + 1
    if not c.get("plain_steps"):
        bump("no_plain_step")
        if c.get("last_reads_last_write_decisive"):
            bump("conflict_without_plain_step")      # the one case in which the register form has to leave its all-at-once pass 3
    return b


def expand_walk(bkp):
    """LGM.cpp:3661-3670: the breakpoint pairs as runs of segments."""
    path = []
    for j in range(1, len(bkp), 2):
        a, z = bkp[j - 1], bkp[j]
        if a > 0:
            path += list(range(a, abs(z) + 1))
        else:
            path += [-k for k in range(-a, abs(z) - 1, -1)]
    return path


# ---------------------------------------------------------------------------------------------
# units
# ---------------------------------------------------------------------------------------------
def _write(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    return path


def perfect_folds(elements):
    """A fold-back junction at every loop end, as synth.make_sample writes them."""
    ends, starts = {}, {}
    for el in elements:
        if el.kind == 'l':
            ends[el.b] = ends.get(el.b, 0) + el.cn
            starts[el.a] = starts.get(el.a, 0) + el.cn
    return [(b, '+', b, '-', cn) for b, cn in sorted(ends.items())] + [(a, '-', a, '+', cn) for a, cn in sorted(starts.items())]


def random_folds(rng, n, density, keep=(), avoid=()):
    """A random fold-back map: per segment with probability `density` a junction of opposite strands to a segment 0, 1 or 2 away,
    on either strand, written from either side; `keep`: junctions placed by hand (first), `avoid`: segments left to them."""
    seen, out = set(), []

    def add(src, sd, tgt, td, cn):
        u, v = (src if sd == '+' else -src), (tgt if td == '+' else -tgt)
        if (u, v) in seen or (-v, -u) in seen:
            return
        seen.add((u, v))
        out.append((src, sd, tgt, td, cn))

    for j in keep:
        add(*j)
    for i in range(1, n + 1):
        if i in avoid or rng.random() >= density:
            continue
        d = rng.choice((0, 0, 1, 1, 2, 2)) * rng.choice((1, -1))
        j = i + d
        if j < 1 or j > n or j in avoid:
            j = i
        sd = rng.choice("+-")
        td = '-' if sd == '+' else '+'
        if rng.random() < 0.5:
            add(i, sd, j, td, rng.randint(1, 3))
        else:
            add(j, sd, i, td, rng.randint(1, 3))
    if not out:
        add(1, '-', 1, '+', 1)      # (a unit without any fold-back junction takes the reference's shortcut)
    return out


def lh_text(name, n, elements, folds, rng=None):
    """The .lh of one chromosome of n segments: segment copy numbers from the elements (localhap.cpp:222-232), the normal
    adjacencies, the fold-back junctions; rng: the JUNC lines shuffled."""
    seg_cn = [0] * (n + 2)
    for el in elements:
        for i in range(el.a, el.b + 1):
            seg_cn[i] += el.cn if el.kind == 'p' else 2 * el.cn
    juncs = [(i, '+', i + 1, '+', max(1, min(seg_cn[i], seg_cn[i + 1]))) for i in range(1, n)] + list(folds)
    if rng is not None:
        rng.shuffle(juncs)
    L = ["SAMPLE_NAME %s" % name, "AVG_CHR_SEG_DP 30", "AVG_WHOLE_HOST_DP 30", "AVG_JUNC_DP 30", "PURITY 1", "AVG_TUMOR_PLOIDY 2", "PLOIDY 2m1",
         "VIRUS_START %d" % (n + 1), "SOURCE 1", "SINK %d" % n]
    for i in range(1, n + 1):
        st = (i - 1) * 1000 + 1
        L.append("SEG H:%d:chr1:%d:%d %.1f %.1f" % (i, st, st + 999, 15.0 * seg_cn[i], float(seg_cn[i])))
    for (src, sd, tgt, td, cn) in juncs:
        L.append("JUNC H:%d:%s H:%d:%s %.1f %.1f U B" % (src, sd, tgt, td, 15.0 * cn, float(cn)))
    return "\n".join(L) + "\n"


def _inv_map(oc, rows):
    return {seg: (rows[j][0], rows[j][2]) for seg, j in zip(oc["inv_seg"], oc["inv_junc"])}


def make_unit(oracle, workdir, name, family, seed, n, elements, folds=None, shuffle=False, tier=""):
    """Writes the unit, asks the oracle for both orientations (and for --all where the unit has few orders), and runs the plain walk.
    The oracle calls the unit valid through its first order without reading behind the end of anything, or this raises."""
    rng = random.Random(seed * 2654435761 + 11)
    lh = _write(os.path.join(workdir, name + ".lh"), lh_text(name, n, elements, perfect_folds(elements) if folds is None else folds, rng if shuffle else None))
    sol = _write(os.path.join(workdir, name + ".sol"), synth.sol_text(elements, 1, n))
    rows = oracle.graph_dump(lh)["juncs"]
    cap = bkp_capacity(elements)
    u = dict(name=name, family=family, seed=seed, tier=tier, lh=lh, sol=sol, n=n, cap=cap, K=len(elements), o={}, out_juncs={}, facts={}, all={})
    for rev in (False, True):
        o = oracle.run_bfb(lh, [sol], reversed_=rev, keep_orders=True)
        assert o["ok"], (name, o["err"])
        oc = o["chr"][0]
        assert not oc["shortcut"] and not oc["infeasible"] and not oc["ub_valid"] and oc["first_valid"] == 0, \
            (name, family, seed, rev, oc["shortcut"], oc["ub_valid"], oc["first_valid"])
        u["o"][rev], u["out_juncs"][rev] = oc, [tuple(x) for x in o["out_juncs"]]
        facts = {}
        bkp, placed = place_walk(oc["node2pat"], oc["node2loop"], oc["orders"][0], bool(oc["first_forward"]), cap, facts)
        assert placed == len(oc["orders"][0]), ("the plain walk does not place every element of the oracle's valid order", name, rev)
        facts["placed_len"] = len(bkp)
        got = fbi_walk(bkp, _inv_map(oc, rows), facts)
        facts["walk_bkp"] = got
        for tag in "se":
            # a decisive candidate counts as visible when the cells AFTER imperfectFBI differ (the mirror half of a palindrome
            # rewrite can wipe out a loop that went into the wrong copy of its parent, and with it the difference)
            if facts.get("lane63_%s_decisive" % tag):
                other, _ = place_walk(oc["node2pat"], oc["node2loop"], oc["orders"][0], bool(oc["first_forward"]), cap, {}, own_register=True)
                if fbi_walk(other, _inv_map(oc, rows), {}) != got:
                    facts["lane63_%s_visible" % tag] = 1
        u["facts"][rev] = facts
    u["L"] = len(u["o"][False]["bkp"])
    u["R"] = u["o"][False]["num_orders"]
    if u["R"] <= ALL_MAX_R:
        for rev in (False, True):
            oa = oracle.run_bfb(lh, [sol], reversed_=rev, all_=True)["chr"][0]
            u["all"][rev] = dict(idx=list(oa["all_eval_idx"]), paths=oa["all_paths"], evaluated=oa["evaluated"])
    return u


# ---- element sets ------------------------------------------------------------------------------
def tier_elements(rng, tier, n, K, cn_choices=(1, 2)):
    if tier == "chain":
        return synth.planted_chain(rng, 1, n, K, cn_choices)
    if tier == "wide":
        return synth.planted_wide(rng, 1, n, (K - 1) // 2, cn_choices)
    if tier == "mixed":
        return synth.planted_mixed(rng, 1, n, K, cn_choices)
    return synth.planted_skew(rng, 1, n, K, cn_choices, k2=int(tier[4:] or 3))


TIERS = (("chain", 4), ("wide", 5), ("mixed", 5), ("skew", 6), ("skew2", 6))


def two_children(n, cn_root, cn_a, cn_b):
    """root l(1, n), A = l(a, n) and B = l(1, b) with b < a: two loops that hang on the root alone, one at each of its ends."""
    b = max(2, n // 3)
    a = min(n - 1, 2 * n // 3 + 1)
    return [Element('l', 1, n, cn_root), Element('l', a, n, cn_a), Element('l', 1, b, cn_b)]


def chain_of(n, cns, first_moves_start=True):
    """Nested loops with the given copy numbers, each sharing one end with its parent (the end that moves alternates)."""
    els, a, b, move_start = [Element('l', 1, n, cns[0])], 1, n, first_moves_start
    for cn in cns[1:]:
        if move_start:
            a += 1
        else:
            b -= 1
        assert a < b
        els.append(Element('l', a, b, cn))
        move_start = not move_start
    return els


def chain_moves(n, cns, moves):
    """Nested loops; moves[i]: loop i + 1 shares its END with its parent (its start moves), else its start."""
    els, a, b = [Element('l', 1, n, cns[0])], 1, n
    for cn, move_start in zip(cns[1:], moves):
        if move_start:
            a += 1
        else:
            b -= 1
        els.append(Element('l', a, b, cn))
    return els


def _split(rng, total, parts):
    """`parts` positive integers that sum to `total`."""
    cuts = sorted(rng.sample(range(1, total), parts - 1))
    return [y - x for x, y in zip([0] + cuts, cuts + [total])]


# ---- families ----------------------------------------------------------------------------------
COPIES_SEEDS = range(0, 130)
SLOT_ROOTS = (1, 15, 16, 17, 31, 32)


def _family_copies(oracle, workdir):
    """Loop copy numbers from BIG among 1 and 2, over the five tiers: the large loop as the root (the seed of the path) and as a
    later element; then hand-built nests in which a large loop goes in behind a slot at a chosen lane or at the end of the path."""
    out = []
    for s in COPIES_SEEDS:
        tier, K = TIERS[s % len(TIERS)]
        big = BIG[(s // len(TIERS)) % len(BIG)]
        rng = random.Random(91000 + s)
        n = rng.choice((16, 20, 24, 31, 32, 33, 40, 48, 63, 64))
        els = tier_elements(rng, tier, n, K)
        loops = [i for i, e in enumerate(els) if e.kind == 'l']
        at = 0 if s >= 65 else rng.choice(loops[1:])
        els[at].cn = big
        out.append(make_unit(oracle, workdir, "ec%d" % s, "copies", 91000 + s, n, els, tier=tier))
    k = 0
    for root in SLOT_ROOTS:
        for big in (3, 16, 33):
            for shape in ("share_end", "share_start", "two_a", "two_b", "three"):
                if shape == "share_end":
                    els = chain_of(24, (root, big), True)
                elif shape == "share_start":
                    els = chain_of(24, (root, big), False)
                elif shape == "two_a":
                    els = two_children(24, root, big, 1)
                elif shape == "two_b":
                    els = two_children(24, root, 1, big)
                else:
                    els = chain_of(24, (root, 1, big), k % 2 == 0)
                if sum(e.cn for e in els) * 4 > 256 and shape not in ("share_end", "share_start"):
                    continue
                out.append(make_unit(oracle, workdir, "es%d" % k, "copies", 92000 + k, 24, els, tier="slots"))
                k += 1
    # a candidate slot at lane 63 that FAILS its nesting test, whose other operand sits in the next register: the closing cell of
    # the last copy of a loop nested two deep, met by the search for the loop nested inside it (found by a search over the copy
    # numbers of four-loop chains with the plain walk; via -s in the forward orientation, via e in the reversed one)
    for k, cns in enumerate(((1, 11, 5, 1), (1, 12, 4, 2), (1, 13, 3, 1), (2, 10, 5, 1))):
        out.append(make_unit(oracle, workdir, "ek%d_s" % k, "copies", 92500 + k, 24, chain_moves(24, cns, (True, False, False)), tier="skip63"))
        out.append(make_unit(oracle, workdir, "ek%d_e" % k, "copies", 92600 + k, 24, chain_moves(24, cns, (False, True, True)), tier="skip63"))
    # ... and where the cell 64 places lower -- what a lane-63 test that stayed in its own register would read -- decides otherwise
    for k, (cs, ce) in enumerate((((1, 10, 7, 1), (1, 9, 7, 1)), ((1, 12, 5, 2), (1, 10, 6, 2)), ((1, 13, 4, 1), (1, 12, 4, 1)), ((1, 14, 3, 2), (1, 13, 3, 2)))):
        out.append(make_unit(oracle, workdir, "ej%d_s" % k, "copies", 92700 + k, 24, chain_moves(24, cs, (True, False, False)), tier="decide63"))
        out.append(make_unit(oracle, workdir, "ej%d_e" % k, "copies", 92800 + k, 24, chain_moves(24, ce, (True, False, True)), tier="decide63"))
    # ... and where that still shows after imperfectFBI (in the eight units above but one, the mirror half of a palindrome rewrite
    # wipes out the loop that went into the wrong copy of its parent, and the difference with it)
    for k, (cs, ce) in enumerate((((14, 2, 1, 1), (15, 1, 1, 2)), ((12, 2, 3, 2), (14, 1, 2, 2)), ((11, 5, 1, 1), (3, 12, 2, 2)), ((1, 13, 3, 2), (6, 9, 2, 2)),
                                  ((4, 10, 3, 2), (10, 5, 2, 1)))):
        out.append(make_unit(oracle, workdir, "ev%d_s" % k, "copies", 92900 + k, 24, chain_moves(24, cs, (False, True, False)), tier="visible63"))
        out.append(make_unit(oracle, workdir, "ev%d_e" % k, "copies", 92950 + k, 24, chain_moves(24, ce, (True, False, True)), tier="visible63"))
    return out


LENGTH_RANGES = ((52, 76), (116, 140), (180, 204), (244, 268), (508, 524), (1020, 1036))


def _family_lengths(oracle, workdir):
    """Chains whose copy numbers sum so that the final length takes every multiple of 4 around 64, 128, 192, 256, 512 and 1024; the
    two-children shape with one huge loop, where the other loop goes in near the front of a path of more than 512 / 1024 cells; and
    mixed units whose pattern is appended at exactly 64, 128 and 256 cells."""
    out = []
    k = 0
    for lo, hi in LENGTH_RANGES:
        for L in range(lo, hi + 1, 4):
            rng = random.Random(93000 + L)
            K = 3 + L % 3
            cns = _split(rng, L // 4, K)
            n = rng.choice((16, 24, 33, 48, 64))
            out.append(make_unit(oracle, workdir, "el%d" % L, "lengths", 93000 + L, n, chain_of(n, cns, L % 8 == 0), tier="chain"))
            if L >= 500:
                for big_on_a in (True, False):
                    rest = L // 4 - 2
                    els = two_children(20, 1, rest if big_on_a else 1, 1 if big_on_a else rest)
                    out.append(make_unit(oracle, workdir, "ef%d_%d" % (L, big_on_a), "lengths", 93500 + k, 20, els, tier="front"))
                    k += 1
    for total in (16, 32, 64):
        for rep in range(3):
            rng = random.Random(94000 + total + rep)
            els = chain_of(20, _split(rng, total, 2 + rep), rep % 2 == 0)
            els.append(Element('p', 1, rng.randint(2, 12), 1))
            out.append(make_unit(oracle, workdir, "ep%d_%d" % (total, rep), "lengths", 94000 + total + rep, 20, els, tier="mixed"))
    return out


FOLD_SEEDS = range(0, 150)
DENSITIES = (0.2, 0.5, 0.9)


def _fold_base(rng, s):
    """The element set under a random fold-back map: a third of the seeds end at 64 cells or less, a third in 65..128, the rest
    above (up to a palindrome of more than 256 cells)."""
    cls = s % 3
    tier, K = TIERS[(s // 3) % len(TIERS)]
    n = rng.choice((16, 20, 24, 31, 32, 33, 40, 48, 63, 64))
    if tier == "chain" or s % 7 == 0:
        total = (rng.randint(8, 16), rng.randint(17, 32), rng.choice((33, 40, 48, 49, 64, 70, 130)))[cls]
        K = rng.randint(2, 5)
        return n, "chain", chain_of(n, _split(rng, total, K), rng.random() < 0.5)
    els = tier_elements(rng, tier, n, K)
    loops = [e for e in els if e.kind == 'l']
    have = sum(e.cn for e in loops)
    want = (rng.randint(max(have, 10), 15), rng.randint(max(have, 18), 31), rng.randint(max(have, 34), 80))[cls]
    rng.choice(loops).cn += max(0, want - have)
    return n, tier, els


def _family_foldbacks(oracle, workdir):
    """Random fold-back maps over element sets of the first two families' kinds; and, by hand, the adjustment of LGM.cpp:3469: a
    pattern p(1, x), x <= 3, behind the root's last cell with a fold-back junction from segment 1 to segment 2 or 3."""
    out = []
    for s in FOLD_SEEDS:
        rng = random.Random(95000 + s)
        n, tier, els = _fold_base(rng, s)
        folds = random_folds(rng, n, DENSITIES[(s // 15) % 3])
        out.append(make_unit(oracle, workdir, "ed%d" % s, "foldbacks", 95000 + s, n, els, folds=folds, shuffle=True, tier=tier))
    k = 0
    for cls_total in (6, 12, 14, 20, 26, 28, 31, 40, 52):
        for x, far in ((2, 3), (3, 3), (2, 2)):
            rng = random.Random(96000 + k)
            els = chain_of(24, _split(rng, cls_total, 2 + k % 3), k % 2 == 0)
            els.append(Element('p', 1, x, 1))
            hand = (1, '+', far, '-', 1) if k % 2 else (far, '+', 1, '-', 1)
            folds = random_folds(rng, 24, DENSITIES[k % 3], keep=[hand], avoid=(1, 2, 3))
            out.append(make_unit(oracle, workdir, "ea%d" % k, "foldbacks", 96000 + k, 24, els, folds=folds, shuffle=True, tier="adjust"))
            k += 1
    # A row of top-level palindromes whose outer cells are NOT the ends of the chromosome (there every rewrite puts back what stood
    # there): the copies of a loop l(a, x) behind the pattern p(1, x) that closes the path.  With a fold-back junction from x to a
    # neighbour, the last iteration (p1 = pos - 1) of one palindrome changes the cell that the last iteration of the next one reads.
    k = 0
    for root, cn in ((1, 4), (2, 6), (3, 9), (4, 8), (6, 14), (9, 17), (12, 12), (12, 30), (20, 33), (8, 60)):
        for x, far in ((9, 10), (12, 11), (7, 9)):
            rng = random.Random(97000 + k)
            els = [Element('l', 1, 24, root), Element('p', 1, x, 1), Element('l', 2 + k % 3, x, cn)]
            # x < far: written from x, so that segment `far` keeps a junction of its own (far -> far + 1), whatever the order of the
            # lines: the cell rewritten to `far` is then rewritten differently from the cell `x` that stood there
            hand = (x, '+', far, '-', 1) if k % 2 or x < far else (far, '+', x, '-', 1)
            folds = random_folds(rng, 24, DENSITIES[k % 3], keep=[hand, (far, '+', far + 1, '-', 1)], avoid=(x, far, far + 1))
            out.append(make_unit(oracle, workdir, "et%d" % k, "foldbacks", 97000 + k, 24, els, folds=folds, shuffle=True, tier="tail"))
            k += 1
    # The same without any pattern, so that the walk has no plain step at all: the root on segments 2 .. 23 of 24 (its outer cells
    # are no longer the ends of the chromosome), a fold-back junction written from segment 2 to segment 1 and one of segment 1's own.
    k = 0
    for root, rest in ((3, ()), (4, (2,)), (6, (3, 2)), (9, (5,)), (12, (8, 4)), (16, (6, 6)), (20, (10,)), (24, (12, 9)), (33, (20, 10)), (40, (30,))):
        for variant in range(2):
            rng = random.Random(99000 + k)
            els, a, b = [Element('l', 2, 23, root)], 2, 23
            for i, cn in enumerate(rest):
                if (i + variant) % 2:
                    a += 1
                else:
                    b -= 1
                els.append(Element('l', a, b, cn))
            hand = [(2, '-', 1, '+', 1), (1, '-', 1, '+', 1)] if variant else [(23, '+', 24, '-', 1), (24, '+', 24, '-', 1)]
            folds = random_folds(rng, 24, DENSITIES[k % 3], keep=hand, avoid=(1, 2, 23, 24))
            out.append(make_unit(oracle, workdir, "ei%d" % k, "foldbacks", 99000 + k, 24, els, folds=folds, shuffle=True, tier="inner"))
            k += 1
    # A loop on ONE segment, l(x, x), behind the pattern p(1, x) that closes the path: its copies -x -x x x are top-level palindromes
    # that hold -cell[pos] already two cells behind pos, one cell in front of where imperfectFBI's search starts; under a fold-back
    # junction from x to a neighbour the palindrome rewrites them.
    k = 0
    for root, mid_cn, cn in ((1, 2, 3), (2, 1, 9), (3, 4, 6), (5, 9, 12), (2, 20, 7), (8, 8, 14), (16, 20, 9), (4, 30, 33), (30, 2, 40)):
        for x, far in ((9, 10), (12, 11)):
            rng = random.Random(98000 + k)
            els = [Element('l', 1, 24, root), Element('l', 2, 24, mid_cn), Element('p', 1, x, 1), Element('l', x, x, cn)]
            hand = (x, '+', far, '-', 1) if k % 2 else (far, '+', x, '-', 1)
            folds = random_folds(rng, 24, DENSITIES[k % 3], keep=[hand], avoid=(x, far))
            out.append(make_unit(oracle, workdir, "eo%d" % k, "foldbacks", 98000 + k, 24, els, folds=folds, shuffle=True, tier="single"))
            k += 1
    return out


FAMILIES = dict(copies=_family_copies, lengths=_family_lengths, foldbacks=_family_foldbacks)
_UNITS = {}


def family_units(oracle, workdir, family):
    """Built once per session and shared (the oracle's answers ride on the units and are never changed)."""
    if (family, workdir) not in _UNITS:
        _UNITS[(family, workdir)] = FAMILIES[family](oracle, workdir)
    return _UNITS[(family, workdir)]


# ---------------------------------------------------------------------------------------------
# coverage: distinct units per branch (either orientation), counted by the walk on the reference side
# ---------------------------------------------------------------------------------------------
def length_class(L):
    return "le64" if L <= 64 else "le128" if L <= 128 else "gt128"


FBI_BRANCHES = ("plain_changes", "n0_changes", "adjustments", "pal_mirrored_changes", "straddle_63_64", "straddle_127_128", "last_changes",
                "last_reads_changed", "last_reads_last_write", "last_reads_last_write_decisive", "no_plain_step", "conflict_without_plain_step", "single_segment_pal_changes")


def coverage(units):
    """{counter: number of distinct units that reach it}; the imperfectFBI branches also per length class ("adjustments/le64");
    "cap_<n>": units whose final bkp_cap is n.  Asserts that the walk gives the oracle's cells on every unit."""
    c = {}

    def bump(k):
        c[k] = c.get(k, 0) + 1

    for u in units:
        hit = set()
        for rev in (False, True):
            f, oc = u["facts"][rev], u["o"][rev]
            assert f["walk_bkp"] == oc["bkp"], ("the plain walk and the oracle disagree on bkp", u["name"], u["family"], u["seed"], rev)
            assert expand_walk(oc["bkp"]) == oc["path"], ("the expansion of the breakpoint pairs and the oracle's path disagree", u["name"], rev)
            assert f["placed_len"] == len(oc["bkp"])
            for k, v in f.items():
                if k not in ("walk_bkp", "placed_len") and v:
                    hit.add(k)
                    if k in FBI_BRANCHES or k in ("palindromes", "pal_changes", "pal_over_64_iterations"):
                        hit.add(k + "/" + length_class(len(oc["bkp"])))
        for k in hit:
            bump(k)
        bump("units")
        bump("cap_%d" % u["cap"])
        bump("units/" + length_class(u["L"]))
        if u["all"]:
            bump("units_all")
            bump("units_all_lane" if u["cap"] <= 192 else "units_all_wave_only")
    return c


def counters_of(u):
    return {rev: {k: v for k, v in u["facts"][rev].items() if k != "walk_bkp"} for rev in (False, True)}


# ---------------------------------------------------------------------------------------------
# runners and comparisons
# ---------------------------------------------------------------------------------------------
class _Env:
    NAMES = ("AMBI_EXPRESS_UNITS", "AMBI_ALL_LANES", "AMBI_ALL_AUTO_LDS")

    def __init__(self, env):
        self.env, self.saved = {k: str(v) for k, v in env.items()}, {}

    def __enter__(self):
        for k in self.NAMES:
            self.saved[k] = os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def run_units(lib, units, reversed_=False, express=False):
    """Every unit of the list in one Batch and one run (express: a second run, which takes the express kernel when the batch is
    small enough).  One record per unit: header, cells, both paths, the output junctions."""
    flags = api.FLAG_REVERSED if reversed_ else 0
    with _Env({"AMBI_EXPRESS_UNITS": 64 if express else 0}):
        graphs, b = [], api.Batch(lib)
        for u in units:
            g = api.Graph(lib, u["lh"])
            graphs.append(g)
            b.add_chromosome_sol(g, 0, u["sol"])
        b.upload()
        b.run(flags); b.wait()
        if express:
            b.run(flags); b.wait_results(); b.wait()
        b.download()
        out = []
        for i in range(len(units)):
            r = dict(b.unit_result(i))
            r.pop("reserved", None)
            rec = dict(header=r, status=r["status"])
            if r["status"] == 0:
                rec.update(bkp=b.unit_bkp(i).tolist(), path=b.unit_path(i, 0).tolist(), path_indel=b.unit_path(i, 1).tolist(), out_juncs=b.unit_out_juncs(i))
            out.append(rec)
        b.close()
        for g in graphs:
            g.close()
    return out


_HEADER = ("num_orders", "first_valid", "first_forward", "evaluated")


def unit_diffs(u, rec, rev):
    oc, d = u["o"][rev], []
    if rec["status"] != 0:
        return ["status %d" % rec["status"]]
    h = rec["header"]
    for k in _HEADER:
        if h[k] != oc[k]:
            d.append("%s %s, oracle %s" % (k, h[k], oc[k]))
    for k in ("bkp", "path", "path_indel"):
        if rec[k] != oc[k]:
            first = next((i for i, (a, b) in enumerate(zip(rec[k], oc[k])) if a != b), min(len(rec[k]), len(oc[k])))
            d.append("%s differs from cell %d on (%d cells, oracle %d)" % (k, first, len(rec[k]), len(oc[k])))
    if rec["out_juncs"] != u["out_juncs"][rev]:
        d.append("output junctions (%d, oracle %d)" % (len(rec["out_juncs"]), len(u["out_juncs"][rev])))
    return d


def _describe(u, rev):
    return dict(family=u["family"], seed=u["seed"], tier=u["tier"], cap=u["cap"], L=u["L"], reversed=rev, counters=counters_of(u)[rev])


def check_against_oracle(units, recs, rev, tag=""):
    bad = {}
    for u, rec in zip(units, recs):
        d = unit_diffs(u, rec, rev)
        if d:
            bad[u["name"]] = (d, _describe(u, rev))
    assert not bad, (tag, "reversed" if rev else "forward", len(bad), dict(list(bad.items())[:4]))


def same_records(units, xs, ys, rev, tag=""):
    bad = {}
    for u, x, y in zip(units, xs, ys):
        if x != y:
            bad[u["name"]] = (sorted(k for k in set(x) | set(y) if x.get(k) != y.get(k)), _describe(u, rev))
    assert not bad, (tag, len(bad), dict(list(bad.items())[:4]))


def run_all(lib, units, reversed_=False, lanes=True):
    """--all over the units (those with few orders): per unit the status, the evaluation count, the valid orders of both passes and
    the path of every one of them."""
    flags = api.FLAG_ALL | (api.FLAG_REVERSED if reversed_ else 0)
    with _Env({"AMBI_EXPRESS_UNITS": 0, "AMBI_ALL_LANES": 1 if lanes else 0}):
        graphs, b = [], api.Batch(lib)
        for u in units:
            g = api.Graph(lib, u["lh"])
            graphs.append(g)
            b.add_chromosome_sol(g, 0, u["sol"])
        b.upload(); b.run(flags); b.download()
        out = []
        for i, u in enumerate(units):
            r = b.unit_result(i)
            rec = dict(status=r["status"], evaluated=r["evaluated"], idx=[], paths=[])
            if r["status"] == 0:
                stride = (len(u["o"][reversed_]["path"]) * 2 + 64 + 7) & ~7
                for ps in (0, 1):
                    idx = b.all_orders(i, ps).tolist()
                    rec["idx"] += [ps * u["R"] + j for j in idx]
                    if idx:
                        rec["paths"] += [p.tolist() for p in b.all_paths(i, ps, 0, len(idx), stride)]
            out.append(rec)
        b.close()
        for g in graphs:
            g.close()
    return out


def check_all_against_oracle(units, recs, rev, tag=""):
    bad = {}
    for u, rec in zip(units, recs):
        want, d = u["all"][rev], []
        if rec["status"] != 0:
            d.append("status %d" % rec["status"])
        else:
            if rec["evaluated"] != want["evaluated"]:
                d.append("evaluated %d, oracle %d" % (rec["evaluated"], want["evaluated"]))
            if rec["idx"] != want["idx"]:
                d.append("valid orders %s, oracle %s" % (rec["idx"][:8], want["idx"][:8]))
            elif rec["paths"] != want["paths"]:
                first = next(i for i, (a, b) in enumerate(zip(rec["paths"], want["paths"])) if a != b)
                d.append("path of valid order %d (evaluation %d) differs" % (first, want["idx"][first]))
        if d:
            bad[u["name"]] = (d, _describe(u, rev))
    assert not bad, (tag, "reversed" if rev else "forward", len(bad), dict(list(bad.items())[:4]))
