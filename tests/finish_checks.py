"""Planted and random SV sets through the finish stages (indelBFB, LGM.cpp:3746-3837, and the output junctions of localhap.cpp:267-289):
generators, a plain walk of indelBFB with a counter on every branch, and the checks shared by the CPU half (host simulation) and
the GPU half of tests/test_finish_fuzz.py.  Deterministic by seed; files go to `workdir`.

indelBFB exists in three forms -- on the cells (indel_bfb: stage_finish, stage_finish<true>), on the runs (indel_bfb_runs:
stage_finish_edit) and as look-ups only (stage_finish_lean) -- and a unit reaches them through five kernels and the express kernel.
The host simulation runs all of them with ONE thread: every `i += g.size()` sweep, every minimum over the group and every barrier is
trivially right there, tables_from_runs_pass<1..3> and the wave-specialised branches never run.  The units here are shaped for the
thread counts of the kernels (256 in the edit kernel, 512 / 1024 in the full stage, g.size() - 64 look-up threads in the lean stage).

Every unit is a whole unit (.lh + .sol) read by the engine's reader and by the oracle's.  Two phases: the unit without SVs gives the
oracle's `path`; the SVs are planted relative to that path and the final unit is written.  Everything is compared bit for bit with
oracle.run_bfb; nothing has a tolerance.
"""
import os
import random

from ambigram_amd import api, synth

ST_ERR_PATH_CAPACITY = -14
ST_ERR_OUTJUNC_CAPACITY = -18


# ---------------------------------------------------------------------------------------------
# indelBFB as lists, list.index and slices: LGM.cpp:3746-3837 statement by statement, a counter on every branch.
# It is the third hand: it has to give the oracle's path_indel on every unit.
# ---------------------------------------------------------------------------------------------
COUNTERS = (
    "applied_deletion", "applied_duplication", "applied_inversion", "applied_insertion",
    "second_deletion", "second_duplication", "second_inversion", "second_insertion",          # applied through the complemented attempt
    "noop_deletion", "noop_duplication", "noop_inversion", "noop_insertion",                    # the four `continue` exits
    "deletion_at_3", "deletion_exit_at_4", "inversion_at_5", "inversion_exit_at_6",            # the limits met exactly
    "erase_empty_two", "erase_empty_insertion",                                                 # path->erase of an empty range
    "arm_front_a_tgt", "arm_front_b_tgt", "arm_back_a_src", "arm_back_b_src",                    # the four chaining arms
    "group_3", "group_4", "group_5_up",
    "find_after_with_earlier",             # find(pos1 + 1, end, v) where v also occurs at or before pos1: a real scan in the engine
    "noop_end_absent", "dup_target_only_behind",
    "units", "units_over_capacity", "units_over_steps", "units_edited", "units_two_edits", "units_sv_over_256", "units_sv_over_512", "units_sv_over_1024",
    "link_256_ahead", "link_1024_ahead",
)


def qualifies(u, v, n):
    """LGM.cpp:3750-3759 on signed local vertices: inside the chromosome, no fold-back inversion, no normal junction."""
    s, t = abs(u), abs(v)
    if s < 1 or s > n or t < 1 or t > n:
        return False
    same = (u > 0) == (v > 0)
    if not same and abs(s - t) <= 2:
        return False
    if same and ((u > 0 and t - s == 1) or (u < 0 and s - t == 1)):
        return False
    return True


def _find(path, val, lo, hi):
    """std::find(path + lo, path + hi, val): the index, or hi."""
    try:
        return path.index(val, lo, hi)
    except ValueError:
        return hi


def indel_walk(path, svs, c):
    """path: signed vertices; svs: (u, v) per qualifying junction in junction order (edge A is u -> v, edge B -v -> -u).
    Returns the edited path; c: dict of counters (COUNTERS), raised in place.  Facts of the unit come back in c["_unit"]."""
    path = list(path)
    left = list(enumerate(svs))
    applied, peak = 0, len(path)          # peak: the longest the path ever is (the reference has no limit; the engine's is path_capacity)
    first_applied = None                  # list position of the first SV of the first group that changes the path

    def bump(k):
        c[k] = c.get(k, 0) + 1

    def find_after(pos1, val):
        if pos1 >= len(path):
            return len(path)                      # (the reference's pos1 + 1 behind end(): every later test sees pos1 == end first)
        q = _find(path, val, pos1 + 1, len(path))
        if q < len(path) and _find(path, val, 0, pos1 + 1) <= pos1:
            bump("find_after_with_earlier")
        return q

    while left:
        group, i, last = [], 0, None
        group_first = left[0][0]
        while i < len(left):
            idx, (u, v) = left[i]
            arm = None
            if not group:
                group = [u, v]
            elif v == group[0]:
                group.insert(0, u); arm = "arm_front_a_tgt"
            elif -u == group[0]:
                group.insert(0, -v); arm = "arm_front_b_tgt"
            elif group[-1] == u:
                group.append(v); arm = "arm_back_a_src"
            elif group[-1] == -v:
                group.append(-u); arm = "arm_back_b_src"
            else:
                i += 1
                continue
            if arm:
                bump(arm)
                if idx - last >= 256:
                    bump("link_256_ahead")
                if idx - last >= 1024:
                    bump("link_1024_ahead")
            last = idx
            left.pop(i)
        P = len(path)

        def complement():
            group.reverse()
            for k in range(len(group)):
                group[k] = -group[k]

        if len(group) == 2:
            same = (group[0] > 0) == (group[1] > 0)
            if same and ((group[0] > 0 and abs(group[0]) < abs(group[1])) or (group[0] < 0 and abs(group[0]) > abs(group[1]))):
                kind, limit = "deletion", 3
            elif same:
                kind, limit = "duplication", 0
            else:
                kind, limit = "inversion", 5
            if kind == "duplication":
                second = False
                pos1 = _find(path, group[0], 0, P)
                pos2 = _find(path, group[1], 0, pos1)
                if pos1 == P or pos2 == pos1:
                    complement(); second = True
                    pos1 = _find(path, group[0], 0, P)
                    pos2 = _find(path, group[1], 0, pos1)
                if pos1 == P or pos2 == pos1:
                    bump("noop_duplication")
                    if pos1 != P and group[1] in path:
                        bump("dup_target_only_behind")
                    elif pos1 == P:
                        bump("noop_end_absent")
                    continue
                path[pos1 + 1:pos1 + 1] = path[pos2:pos1 + 1]
                peak = max(peak, len(path))
                bump("applied_duplication"); applied += 1
                if first_applied is None:
                    first_applied = group_first
                if second:
                    bump("second_duplication")
                continue
            second = False
            pos1 = _find(path, group[0], 0, P)
            pos2 = find_after(pos1, group[1])
            if pos1 == P or pos2 == P:
                complement(); second = True
                pos1 = _find(path, group[0], 0, P)
                pos2 = find_after(pos1, group[1])
            if pos1 == P or pos2 == P or pos2 - pos1 > limit:
                bump("noop_" + kind)
                if pos1 == P or pos2 == P:
                    bump("noop_end_absent")
                elif pos2 - pos1 == limit + 1:
                    bump("deletion_exit_at_4" if kind == "deletion" else "inversion_exit_at_6")
                continue
            if pos2 - pos1 == limit:
                bump("deletion_at_3" if kind == "deletion" else "inversion_at_5")
            if pos2 == pos1 + 1:
                bump("erase_empty_two")
            del path[pos1 + 1:pos2]
            bump("applied_" + kind); applied += 1
            if first_applied is None:
                first_applied = group_first
            if second:
                bump("second_" + kind)
        else:
            bump("group_3" if len(group) == 3 else "group_4" if len(group) == 4 else "group_5_up")
            second = False
            pos1 = _find(path, group[0], 0, P)
            pos2 = find_after(pos1, group[-1])
            if pos1 == P or pos2 == P:
                complement(); second = True
                pos1 = _find(path, group[0], 0, P)
                pos2 = find_after(pos1, group[-1])
            if pos1 == P or pos2 == P:
                bump("noop_insertion"); bump("noop_end_absent")
                continue
            if pos2 == pos1 + 1:
                bump("erase_empty_insertion")
            path[pos1 + 1:pos2] = group[1:-1]
            peak = max(peak, len(path))
            bump("applied_insertion"); applied += 1
            if first_applied is None:
                first_applied = group_first
            if second:
                bump("second_insertion")
    c["_unit"] = dict(applied=applied, nsv=len(svs), peak=peak, first_applied=first_applied)
    return path


def out_juncs_walk(path):
    """localhap.cpp:267-289: consecutive vertices that are not a reference adjacency, the first of an edge or its complement keeps the count."""
    acc = []
    for a, b in zip(path, path[1:]):
        if abs(abs(a) - abs(b)) == 1 and (a > 0) == (b > 0):
            continue
        for j in acc:
            if (j[0] == a and j[1] == b) or (j[0] == -b and j[1] == -a):
                j[2] += 1
                break
        else:
            acc.append([a, b, 1])
    return [tuple(j) for j in acc]


def path_capacity(n, elements, svs):
    """The engine's limit on a unit's path (HostBatch::add_unit): the breakpoint path has at most 4 cells per loop
    copy and 2 per pattern, every pair of them expands to at most n cells; twice that where a same-strand SV may duplicate a stretch, a
    cell per SV for the insertions, 64 more, rounded up to eight."""
    bkp_len = sum(4 * e.cn if e.kind == 'l' else 2 for e in elements)
    bound = max(64, n, ((bkp_len + 1) // 2) * n)
    may_dup = any((u > 0) == (v > 0) for u, v in svs)
    return (bound * (2 if may_dup else 1) + len(svs) + 64 + 7) & ~7


def step_capacity(elements, svs):
    """The engine's limit on the junction steps of the final path, repeats included, and on its output-junction records (DESIGN.md
    section 8; HostBatch::add_unit): the capacity of the breakpoint path (rounded up to eight, at least four), 64, and one per SV."""
    bkp_len = sum(4 * e.cn if e.kind == 'l' else 2 for e in elements)
    return max(4, (bkp_len + 7) & ~7) + 64 + len(svs)


def n_steps(path):
    return sum(1 for a, b in zip(path, path[1:]) if not (abs(abs(a) - abs(b)) == 1 and (a > 0) == (b > 0)))


def n_runs(path):
    return sum(1 for i in range(len(path)) if i == 0 or path[i] != path[i - 1] + 1)


# ---------------------------------------------------------------------------------------------
# units: phase 1 (the path), phase 2 (the SVs planted relative to it)
# ---------------------------------------------------------------------------------------------
def _write(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    return path


def _parse_juncs(lh_text):
    out = []
    for line in lh_text.splitlines():
        if line.startswith("JUNC "):
            t = line.split()
            a, b = t[1].split(":"), t[2].split(":")
            u = int(a[1]) if a[2] == '+' else -int(a[1])
            v = int(b[1]) if b[2] == '+' else -int(b[1])
            out.append((u, v))
    return out


class Planter:
    """The SV list of one unit: what a reader would keep (Graph.cpp:489-499 calls u -> v and -v -> -u the same junction), every pair
    written from either side at random."""

    def __init__(self, rng, n, path, base_juncs):
        self.rng, self.n, self.path = rng, n, path
        self.seen = set(base_juncs)
        self.svs = []            # (u, v) as written
        self.where = {}
        for i, v in enumerate(path):
            self.where.setdefault(v, []).append(i)

    def add(self, u, v, side=None):
        """False: not an SV, or the readers would drop it as a repeat."""
        if not qualifies(u, v, self.n) or (u, v) in self.seen or (-v, -u) in self.seen:
            return False
        if (self.rng.random() < 0.5) if side is None else side:
            u, v = -v, -u
        self.seen.add((u, v))
        self.svs.append((u, v))
        return True

    def pad(self, count, avoid=()):
        """far head-to-head inversions i+ -> j- (j - i >= 6) until the list has `count` SVs: looked up, never applied on their own.  They
        cannot chain with each other (a target is a '-' vertex, a group's front a '+' one); `avoid`: segments they stay away from, so
        that they do not chain with the SVs planted there either."""
        n, guard = self.n, 0
        while len(self.svs) < count:
            guard += 1
            assert guard < 200 * count + 1000, "no room for %d padding SVs on %d segments" % (count, n)
            i = self.rng.randint(1, n - 6)
            j = self.rng.randint(i + 6, n)
            if i not in avoid and j not in avoid:
                self.add(i, -j, side=False)

    def vertex(self):
        return self.rng.choice((1, -1)) * self.rng.randint(1, self.n)

    def absent(self):
        miss = [v for s in range(1, self.n + 1) for v in (s, -s) if v not in self.where]
        return self.rng.choice(miss) if miss else None


def make_unit(oracle, workdir, name, n, tier, K, seed, plant, shuffle=True, cn_choices=(1, 2), imperfect=0, family=""):
    """plant(p: Planter) fills p.svs; returns the unit (dict) with the oracle's answer for the final files."""
    base = synth.make_sample(n, 0, tier, K, seed, name=name, cn_choices=cn_choices, imperfect=imperfect)
    sol = _write(os.path.join(workdir, name + ".sol"), base.sol_texts[0])
    lh0 = _write(os.path.join(workdir, name + ".base.lh"), base.lh_text)
    o0 = oracle.run_bfb(lh0, [sol])
    assert o0["ok"] and not o0["chr"][0]["shortcut"] and o0["chr"][0]["first_valid"] >= 0, (name, o0["err"])
    path0 = o0["chr"][0]["path"]
    rng = random.Random((seed * 2654435761 + 97) & 0xFFFFFFFF)
    p = Planter(rng, n, path0, _parse_juncs(base.lh_text))
    plant(p)
    if shuffle:
        rng.shuffle(p.svs)
    lines = ["JUNC H:%d:%s H:%d:%s 15.0 1.0 U B" % (abs(u), '+' if u > 0 else '-', abs(v), '+' if v > 0 else '-') for (u, v) in p.svs]
    lh = _write(os.path.join(workdir, name + ".lh"), base.lh_text + "\n".join(lines) + ("\n" if lines else ""))
    o = oracle.run_bfb(lh, [sol])
    assert o["ok"], (name, o["err"])
    oc = o["chr"][0]
    # the oracle neither refuses the unit nor takes a shortcut (no share of the cases is left out)
    assert not oc["shortcut"] and not oc["infeasible"] and not oc["ub_valid"] and oc["first_valid"] >= 0, name
    u = dict(name=name, family=family, lh=lh, sol=sol, n=n, svs=list(p.svs), oc=oc, out_juncs=[tuple(x) for x in o["out_juncs"]],
             np=len(oc["bkp"]) // 2, same_strand=any((u > 0) == (v > 0) for u, v in p.svs))
    # the reference has no limit on the path; a unit whose edits take it beyond the engine's documented one has to end with
    # ST_ERR_PATH_CAPACITY there (decided here, on the reference side: the plain walk over the oracle's path)
    facts = {}
    indel_walk(oc["path"], u["svs"], facts)
    cap = path_capacity(n, base.elements[0], u["svs"])
    if facts["_unit"]["peak"] > cap:
        u["over_capacity"] = cap
    elif n_steps(oc["path_indel"]) > step_capacity(base.elements[0], u["svs"]):
        u["over_steps"] = step_capacity(base.elements[0], u["svs"])     # duplications repeated more junction steps than the unit has room for
    u["first_applied"] = facts["_unit"]["first_applied"]
    return u


# ---- the planting rules ------------------------------------------------------------------------
def plant_near(p, count=8):
    """path[q] -> path[q + d], d = 1..7, as it stands or complemented (-path[q + d] -> -path[q]: the second attempt decides)"""
    P = len(p.path)
    for _ in range(count):
        for _try in range(20):
            d = p.rng.randint(1, 7)
            q = p.rng.randrange(0, P - d)
            u, v = p.path[q], p.path[q + d]
            if p.rng.random() < 0.4:
                u, v = -v, -u
            if p.add(u, v):
                break


def plant_first_near(p, count=6):
    """the same from the FIRST occurrence of a vertex, so that the distance the reference measures is the planted one"""
    firsts = sorted(w[0] for w in p.where.values())
    for _ in range(count):
        for _try in range(20):
            q = p.rng.choice(firsts)
            d = p.rng.choice((2, 3, 3, 4, 4, 5, 5, 6, 6, 7))
            if q + d >= len(p.path):
                continue
            v = p.path[q + d]
            if p.where[v][0] < q and p.rng.random() < 0.7:     # (mostly a target that is first met behind q)
                continue
            if p.add(p.path[q], v):
                break


def plant_backward(p, count=4):
    """path[q + d] -> path[q] on one strand: duplication; some whose target occurs only behind pos1 (no-op)"""
    P = len(p.path)
    for k in range(count):
        for _try in range(40):
            d = p.rng.randint(1, 6)
            q = p.rng.randrange(0, P - d)
            u, v = p.path[q + d], p.path[q]
            if (u > 0) != (v > 0):
                continue
            if k % 3 == 2:                      # a target that lies only behind the first occurrence of the source
                u, v = v, u
                if p.where[v][0] < p.where[u][0]:
                    continue
            if p.add(u, v):
                break


def plant_chain(p, links=None, ends="path", mid=None):
    """path[a] -> m1 -> .. -> path[b]: `links` junctions, middle vertices random (or `mid`), each link complemented at random by add().
    ends: "path" (both in the path, b behind a), "absent" (an end the path does not hold), "both_sides" (the back vertex occurs in
    front of the first occurrence of the front vertex and behind it)."""
    rng = p.rng
    L = links or rng.randint(2, 6)
    for _try in range(60):
        P = len(p.path)
        a = rng.randrange(0, P - 1)
        front = p.path[a]
        a = p.where[front][0]
        b = rng.randrange(a + 1, min(P, a + 12))
        back = p.path[b]
        if ends == "absent":
            miss = p.absent()
            if miss is None:
                return False
            if rng.random() < 0.5:
                front = miss
            else:
                back = miss
        elif ends == "both_sides":
            cands = [v for v, w in p.where.items() if w[0] < a and w[-1] > a and v != front]
            if not cands:
                continue
            back = rng.choice(cands)
        mids = list(mid) if mid is not None else [p.vertex() for _ in range(L - 1)]
        chain = [front] + mids + [back]
        if len(set(chain)) < len(chain) or any(-x in chain for x in chain):
            continue
        pairs = list(zip(chain, chain[1:]))
        if any(not qualifies(u, v, p.n) or (u, v) in p.seen or (-v, -u) in p.seen for u, v in pairs):
            continue
        rng.shuffle(pairs)
        for u, v in pairs:
            p.add(u, v)
        return True
    return False


def plant_chain_exact(p, chain):
    pairs = list(zip(chain, chain[1:]))
    p.rng.shuffle(pairs)
    return all([p.add(u, v) for u, v in pairs])


def plant_insertions(p, groups, mids, pool_lo):
    """`groups` insertion groups front -> m1 (-> m2 ..) -> back between the neighbouring cells 2k, 2k + 1 of the path's first stretch, the
    links in chain order; a middle vertex lies on a segment from pool_lo up that no other group uses on either strand, so that the
    groups neither chain with each other nor erase each other's cells.  Every group adds `mids` cells and mids + 1 junction steps."""
    segs = list(range(pool_lo, p.n + 1))
    p.rng.shuffle(segs)
    done = 0
    for q in range(0, len(p.path) - 1, 2):
        if done == groups or len(segs) < mids or p.path[q + 1] != p.path[q] + 1 or p.path[q + 1] >= pool_lo - 2:
            break
        for _try in range(50):
            take = p.rng.sample(segs, mids)
            chain = [p.path[q]] + [x * p.rng.choice((1, -1)) for x in take] + [p.path[q + 1]]
            if all(qualifies(u, v, p.n) and (u, v) not in p.seen and (-v, -u) not in p.seen for u, v in zip(chain, chain[1:])):
                break
        else:
            continue
        for x in take:
            segs.remove(x)
        for u, v in zip(chain, chain[1:]):
            p.add(u, v)
        done += 1
    return done


def plant_random(p, count=6):
    for _ in range(count):
        for _try in range(20):
            if p.add(p.vertex(), p.vertex()):
                break


def plant_short_inversions(p, count):
    """path[q] -> path[q + d] across a turn of the path (the two cells on opposite strands, d = 2..5), q the first occurrence of its
    vertex and the target not met in between: the reference finds exactly these two cells and erases what lies between them"""
    P, done = len(p.path), 0
    spots = [(w[0], d) for w in p.where.values() for d in range(2, 6) if w[0] + d < P]
    p.rng.shuffle(spots)
    for q, d in spots:
        u, v = p.path[q], p.path[q + d]
        if done == count:
            break
        if (u > 0) == (v > 0) or v in p.path[q + 1:q + d]:
            continue
        done += p.add(u, v)
    return done


def plant_short_deletions(p, count):
    """path[q] -> path[q + d] inside one stretch of the path (d = 2, 3), q the first occurrence of its vertex: the reference finds
    exactly these two cells and erases what lies between them"""
    P, done = len(p.path), 0
    spots = [(w[0], d) for w in p.where.values() for d in (2, 3) if w[0] + d < P]
    p.rng.shuffle(spots)
    for q, d in spots:
        if done == count:
            break
        if p.path[q + d] == p.path[q] + d:           # (one stretch: the cells count up by one)
            done += p.add(p.path[q], p.path[q + d])
    return done


def plant_opposite_only(p):
    """opposite-strand SVs only (the unit does not go straight to the edit kernel): a short inversion that edits, an insertion chain
    made of inversions, far padding"""
    rng, P = p.rng, len(p.path)
    plant_short_inversions(p, 2)
    for _try in range(60):                       # front+ -> m- , m- -> back+ : both links switch the strand
        a = rng.randrange(0, P - 8)
        front = p.path[a]
        a = p.where[front][0]
        back = p.path[rng.randrange(a + 1, min(P, a + 8))]
        if (front > 0) != (back > 0):
            continue
        m = rng.randint(1, p.n) * (-1 if front > 0 else 1)
        if qualifies(front, m, p.n) and qualifies(m, back, p.n) and abs(m) not in (abs(front), abs(back)):
            if p.add(front, m) and p.add(m, back):
                break
    p.pad(len(p.svs) + rng.randint(0, 6))


# ---- families ----------------------------------------------------------------------------------
_TIERS = (("chain", 3), ("chain", 5), ("mixed", 5), ("wide", 5), ("chain", 9), ("mixed", 8), ("wide", 7), ("chain", 2))


def _shape(seed):
    rng = random.Random(seed * 7919 + 13)
    tier, K = _TIERS[seed % len(_TIERS)]
    return rng.choice((16, 20, 24, 31, 32, 33, 40, 48, 63, 64)), tier, K


RANDOM_SEEDS = {"near": range(0, 70), "backward": range(100, 150), "chains": range(200, 290), "random": range(300, 360), "lean": range(400, 430), "inversions": range(0, 60)}


def _family_near(oracle, workdir):
    out = []
    for s in RANDOM_SEEDS["near"]:
        n, tier, K = _shape(s)
        out.append(make_unit(oracle, workdir, "fn%d" % s, n, tier, K, 61000 + s, lambda p: (plant_near(p, 6), plant_first_near(p, 6)),
                             imperfect=s % 2, family="near"))
    return out


def _family_backward(oracle, workdir):
    out = []
    for s in RANDOM_SEEDS["backward"]:
        n, tier, K = _shape(s)
        out.append(make_unit(oracle, workdir, "fb%d" % s, n, tier, K, 62000 + s, lambda p: (plant_backward(p, 2 + s % 4), plant_near(p, s % 3)),
                             family="backward"))
    return out


def _family_chains(oracle, workdir):
    out = []
    for s in RANDOM_SEEDS["chains"]:
        n, tier, K = _shape(s)

        def plant(p, s=s):
            kinds = ("path", "path", "both_sides", "absent", "path", "both_sides")
            for k in range(1 + s % 3):
                plant_chain(p, links=2 + (s + k) % 5, ends=kinds[(s + k) % len(kinds)])
            plant_near(p, s % 3)
        out.append(make_unit(oracle, workdir, "fc%d" % s, n, tier, K, 63000 + s, plant, family="chains"))
    return out


def _family_random(oracle, workdir):
    out = []
    for s in RANDOM_SEEDS["random"]:
        n, tier, K = _shape(s)
        out.append(make_unit(oracle, workdir, "fr%d" % s, n, tier, K, 64000 + s, lambda p: plant_random(p, 4 + s % 9), family="random"))
    return out


def _family_inversions(oracle, workdir):
    """short inversions among random pairs: the edits of the one remove what the other would have found, so that a group is applied
    through its second (complemented) attempt although a BFB path holds nearly every vertex on both strands"""
    out = []
    for s in RANDOM_SEEDS["inversions"]:
        n, tier, K = _shape(s)
        out.append(make_unit(oracle, workdir, "fi%d" % s, n, tier, K, 80000 + s,
                             lambda p: (plant_short_inversions(p, 3), plant_random(p, 8), plant_short_inversions(p, 3)), family="inversions"))
    return out


def _family_lean(oracle, workdir):
    out = []
    for s in RANDOM_SEEDS["lean"]:
        n, tier, K = _shape(s)
        u = make_unit(oracle, workdir, "fl%d" % s, n, tier, K, 65000 + s, plant_opposite_only, family="lean")
        assert not u["same_strand"], u["name"]
        out.append(u)
    return out


SV_COUNTS = (255, 256, 257, 511, 513, 1025)
SV_WHERE = ("first", "255", "256", "257", "last", "chain", "opp_191", "opp_192", "opp_193", "opp_447", "opp_448", "opp_449", "opp_last", "opp_none")


def _family_sv_counts(oracle, workdir):
    """Thread-count edges: exact SV counts; the first editing SV at list positions 0, 255, 256, 257 and last; a chain whose next link
    lies at least 256 / 1024 list positions behind the previous one; units of opposite-strand SVs only (the lean stage's) whose one
    editing SV sits at 191, 192, 193 (the lean kernel looks SVs up with 192 of its 256 threads), 447, 448, 449 (the express kernel
    with 448 of its 512; clamped to the last position in the shorter lists) or last, or that have none.  The lists are NOT shuffled: the positions are the point."""
    out = []
    for count in SV_COUNTS:
        for where in SV_WHERE:
            planted = []

            def plant(p, count=count, where=where, planted=planted):
                editing = Planter(p.rng, p.n, p.path, [])
                editing.seen = p.seen
                if where.startswith("opp_") and where != "opp_none":
                    # opposite strands only: the unit is the lean stage's, which looks the SVs up with 192 of its 256 threads and has to
                    # hand the unit over for the ONE SV that edits
                    assert plant_short_inversions(editing, 1) == 1
                elif where != "opp_none":                # (opp_none: look-ups only, the lean stage finishes the unit itself)
                    assert plant_short_deletions(editing, 2) == 2
                if where == "chain":
                    # three links, far apart in the list; their middle vertices come from add()'s own complementing
                    nl = 2 if count > 1024 else 3
                    assert plant_chain(editing, links=nl, ends="path")
                    links = editing.svs[-nl:]
                    at = {0: links[0], 1024: links[1]} if count > 1024 else {0: links[0], min(256, count - 2): links[1], count - 1: links[2]}
                    rest = editing.svs[:-nl]
                else:
                    pos = dict(first=0, last=count - 1, opp_last=count - 1, opp_none=0).get(where)
                    pos = min(int(where.replace("opp_", "")), count - 1) if pos is None else pos
                    at = {pos + k: sv for k, sv in enumerate(editing.svs) if pos + k < count}
                    if len(at) < len(editing.svs):
                        at = {count - len(editing.svs) + k: sv for k, sv in enumerate(editing.svs)}
                    rest = []
                p.pad(count - len(at) - len(rest), avoid={abs(x) for sv in editing.svs for x in sv})
                fill = p.svs + rest
                p.svs = [at[i] if i in at else fill.pop() for i in range(count)]
                assert not fill and len(p.svs) == count
                planted.extend(editing.svs)
            name = "fs%d_%s" % (count, where)
            out.append(make_unit(oracle, workdir, name, 64 if count < 1000 else 72, "chain", 4, 66000 + count + len(where) * 7 + ord(where[0]),
                                 plant, shuffle=False, family="sv_counts"))
            assert len(out[-1]["svs"]) == count
            # no padding SV edits the path: the first SV that does is one of the planted ones, at the list position this unit is about
            at = sorted(i for i, sv in enumerate(out[-1]["svs"]) if sv in planted)
            first = out[-1]["first_applied"]
            assert (first is None) if where == "opp_none" else (first in at if where != "chain" else first is None or first in at), (name, first, at)
            if where.startswith("opp_") and where != "opp_none":
                assert len(at) == 1 and first == at[0] == min(int(where[4:]) if where[4:].isdigit() else count - 1, count - 1), (name, first, at)
            if where.startswith("opp_"):
                assert not out[-1]["same_strand"] and (out[-1]["oc"]["path_indel"] != out[-1]["oc"]["path"]) == (where != "opp_none"), name
    return out


N_CLASSES = (128, 129, 256, 257, 384, 385, 512, 513)


def _family_segments(oracle, workdir):
    """Segment counts around the vertex tiling of tables_from_runs (256 threads x up to 4 vertices per pass: 2n = 256, 258, 512, 514,
    768, 770, 1024 and 1026 -- the last with a second trip), on units that go through the edit stage and are edited there, the edits
    near the top segments so that the last vertices of the tables decide."""
    out = []
    for n in N_CLASSES:
        for rep in range(2):
            def plant(p, rep=rep):
                plant_first_near(p, 4)
                plant_backward(p, 2)
                hi = [q for q, v in enumerate(p.path[:-4]) if abs(v) >= p.n - 2]
                for q in hi[:3]:
                    p.add(p.path[q], p.path[q + 3 + rep])
                    p.add(p.path[q + 2], p.path[q])
                plant_chain(p, links=2 + rep, ends="both_sides")
            u = make_unit(oracle, workdir, "fg%d_%d" % (n, rep), n, "chain", 3, 67000 + n + rep, plant, cn_choices=(1,), family="segments")
            assert u["same_strand"], u["name"]
            out.append(u)
    return out


RUN_CLASSES = (7, 8, 9, 16, 17)


def _family_runs(oracle, workdir):
    """Final paths of 7, 8, 9, 16 and 17 runs (the rounds of eight in tables_from_runs_pass) and of more than 256 runs (the stride of
    runs_build and runs_find_first), searched among small seeds."""
    out, have = [], {}
    for s in range(0, 400):
        if len(have) == len(RUN_CLASSES):
            break
        K = 1 + s % 7
        u = make_unit(oracle, workdir, "fu%d" % s, 24 + s % 9, "chain", K, 68000 + s, lambda p: (plant_first_near(p, 1 + s % 2), plant_backward(p, 1)),
                      cn_choices=(1,), family="runs")
        r = n_runs(u["oc"]["path_indel"])
        if r in RUN_CLASSES and r not in have and u["oc"]["path_indel"] != u["oc"]["path"] and u["same_strand"]:
            have[r] = u
    assert sorted(have) == list(RUN_CLASSES), sorted(have)
    out = [have[r] for r in RUN_CLASSES]

    # more than 256 runs INSIDE the edit stage (its lists hold twice the breakpoint pairs and 32 runs): a unit of 256 pairs and 30 insertions
    seed, tier, n, K, cns = PAIR_UNITS[256]
    u = make_unit(oracle, workdir, "fu_many", n, tier, K, seed, lambda p: (plant_insertions(p, 30, 1, 40), plant_backward(p, 1)), shuffle=False, cn_choices=cns, family="runs")
    assert n_runs(u["oc"]["path_indel"]) > 256 and u["same_strand"], n_runs(u["oc"]["path_indel"])
    out.append(u)
    return out


NP_CLASSES = (255, 256, 257)
# A loop copy gives two breakpoint pairs, so the chain tier only has even counts; the mixed tier's patterns make the count odd in a few
# per cent of its samples.  Found by a search over seeds (profiles/r14_notes.md); make_unit's oracle run asserts the count.
PAIR_UNITS = {255: (69758, "mixed", 90, 62, (2, 2, 2, 2, 3)), 256: (69076, "mixed", 100, 63, (2, 2, 2, 3)), 257: (69008, "mixed", 90, 61, (2, 2, 2, 3))}


def _family_pairs(oracle, workdir):
    """Breakpoint pairs around the np <= 256 split of the lean and the edit stage (one wavefront for the output junctions, one for the
    runs, the others for look-ups or cells -- or the whole workgroup phase by phase), with and without SVs."""
    out = []
    for np_, (seed, tier, n, K, cns) in sorted(PAIR_UNITS.items()):
        plants = (("none", lambda p: None), ("lookups", lambda p: p.pad(20)), ("edits", lambda p: (plant_first_near(p, 4), plant_backward(p, 2), p.pad(12))),
                  ("opposite", plant_opposite_only))
        for tag, plant in plants:
            u = make_unit(oracle, workdir, "fp%d_%s" % (np_, tag), n, tier, K, seed, plant, cn_choices=cns, family="pairs")
            assert u["np"] == np_, (u["name"], u["np"])
            out.append(u)
    return out


def _family_out_juncs(oracle, workdir):
    """Few elements (a short breakpoint path, so few output-junction records by the old rule) and many applied insertion groups, each of
    which adds junction steps to the path: the units that ended with ST_ERR_OUTJUNC_CAPACITY while the reference prints a path."""
    out = []
    for rep, (n, mids) in enumerate(((160, 2), (160, 1), (220, 3))):
        def plant(p, mids=mids):
            assert plant_insertions(p, 50, mids, 103) >= 28
        u = make_unit(oracle, workdir, "fo%d" % rep, n, "chain", 1, 70000 + rep, plant, shuffle=False, cn_choices=(1,), family="out_juncs")
        old_cap = max(4, (len(u["oc"]["bkp"]) + 7) & ~7) + 64
        assert len(u["out_juncs"]) > old_cap, (u["name"], len(u["out_juncs"]), old_cap)          # more records than bkp_cap + 64 held
        out.append(u)
    return out


def _family_capacity(oracle, workdir):
    """Duplications that really exceed the unit's path capacity (csrc/ambi_pack.cpp: twice the bound of the breakpoint path, the SV
    count and 64): the reference has no limit, the engine ends the unit with ST_ERR_PATH_CAPACITY.  Neighbours: ordinary edited units."""
    n = 100

    def plant(p):
        for seg in range(n, n - 6, -1):        # seg+ -> 1+: a copy of everything up to the first seg+, six times
            p.add(seg, 1, side=False)
    u = make_unit(oracle, workdir, "fcap", n, "chain", 1, 71000, plant, shuffle=False, cn_choices=(1,), family="capacity")
    assert u.get("over_capacity") and len(u["oc"]["path_indel"]) > u["over_capacity"], (len(u["oc"]["path_indel"]), u.get("over_capacity"))

    # the other limit: 50 insertion groups of three steps each and ONE duplication over all of them (101+ -> 2+; it chains with none of
    # them): the path stays far inside its capacity, its junction steps, repeats included, do not
    def steps(p):
        assert plant_insertions(p, 50, 2, 103) == 50
        assert p.add(101, 2, side=False)
    v = make_unit(oracle, workdir, "fsteps", 220, "chain", 1, 71003, steps, shuffle=False, cn_choices=(1,), family="capacity")
    assert v.get("over_steps") and "over_capacity" not in v and len(v["out_juncs"]) <= v["over_steps"], (v.get("over_steps"), len(v["out_juncs"]))
    return [make_unit(oracle, workdir, "fcap_a", 48, "chain", 3, 71001, lambda p: plant_first_near(p, 4), family="capacity"), u,
            make_unit(oracle, workdir, "fcap_b", 48, "mixed", 5, 71002, lambda p: plant_backward(p, 3), family="capacity"), v,
            make_unit(oracle, workdir, "fcap_c", 40, "chain", 3, 71004, lambda p: plant_first_near(p, 4), family="capacity")]


FAMILIES = dict(near=_family_near, backward=_family_backward, chains=_family_chains, random=_family_random, inversions=_family_inversions, lean=_family_lean,
                sv_counts=_family_sv_counts, segments=_family_segments, runs=_family_runs, pairs=_family_pairs, out_juncs=_family_out_juncs,
                capacity=_family_capacity)
_UNITS = {}


def family_units(oracle, workdir, family):
    """Built once per session and shared (the oracle's answers ride on the units and are never changed)."""
    if (family, workdir) not in _UNITS:
        _UNITS[(family, workdir)] = FAMILIES[family](oracle, workdir)
    return _UNITS[(family, workdir)]


# ---------------------------------------------------------------------------------------------
# coverage (on the reference side: the oracle's path and the unit's junction list, never the engine)
# ---------------------------------------------------------------------------------------------
def coverage(units):
    c = {k: 0 for k in COUNTERS}
    c["n_classes"], c["np_classes"], c["run_classes"], c["runs_over_256"] = set(), set(), set(), 0
    for u in units:
        oc = u["oc"]
        got = indel_walk(oc["path"], u["svs"], c)
        assert got == oc["path_indel"], ("the plain walk of indelBFB and the oracle disagree", u["name"])
        assert out_juncs_walk(got) == u["out_juncs"], ("output junctions: the plain walk and the oracle disagree", u["name"])
        assert oc["indel_printed"] == (len(u["svs"]) > 0), u["name"]
        f = c.pop("_unit")
        c["units"] += 1
        c["units_over_capacity"] += "over_capacity" in u
        c["units_over_steps"] += "over_steps" in u
        c["units_edited"] += oc["path_indel"] != oc["path"]
        c["units_two_edits"] += f["applied"] >= 2
        c["units_sv_over_256"] += f["nsv"] > 256
        c["units_sv_over_512"] += f["nsv"] > 512
        c["units_sv_over_1024"] += f["nsv"] > 1024
        if u["family"] == "segments":
            c["n_classes"].add(u["n"])
        if u["family"] == "pairs":
            c["np_classes"].add(u["np"])
        if u["family"] == "runs":
            r = n_runs(oc["path_indel"])
            c["run_classes"].add(r if r <= 256 else 257)
            c["runs_over_256"] += r > 256
    for k in ("n_classes", "np_classes", "run_classes"):
        c[k] = sorted(c[k])
    return c


# ---------------------------------------------------------------------------------------------
# running a list of units as ONE batch, and the comparison
# ---------------------------------------------------------------------------------------------
class _Env:
    NAMES = ("AMBI_EXPRESS_UNITS", "AMBI_HOSTSIM_EDIT", "AMBI_DIRECT_EDIT", "AMBI_DIRECT_FULL", "AMBI_DIRECT_EXT", "AMBI_FULL_THREADS",
             "AMBI_EDIT_RUN_CAP", "AMBI_RUN_SLOTS")

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


def run_units(lib, units, env=None, express=False):
    """Every unit of the list in one Batch, one upload, one run (express: a second run, which takes the express kernel when the batch
    is small enough).  One record per unit: header, both paths, the output junctions, the path expanded from the run-length form."""
    e = dict(env or {})
    e.setdefault("AMBI_EXPRESS_UNITS", 64 if express else 0)
    with _Env(e):
        graphs, b = [], api.Batch(lib)
        for u in units:
            g = api.Graph(lib, u["lh"])
            graphs.append(g)
            b.add_chromosome_sol(g, 0, u["sol"])
        b.upload()
        b.run(0); b.wait()
        if express:
            b.run(0); b.wait_results(); b.wait()
        b.runs_to_host(1, 0); b.runs_wait(0)
        runs = [b.runs_unit_path(0, i).tolist() for i in range(len(units))]
        b.download()
        out = []
        for i in range(len(units)):
            r = dict(b.unit_result(i))
            r.pop("reserved", None)
            rec = dict(header=r, status=r["status"], runs=runs[i], path=b.unit_path(i, 0).tolist())
            if r["status"] == 0:
                rec.update(bkp=b.unit_bkp(i).tolist(), path_indel=b.unit_path(i, 1).tolist(), out_juncs=b.unit_out_juncs(i))
            out.append(rec)
        b.close()
        for g in graphs:
            g.close()
    return out


_HEADER = ("num_orders", "first_valid", "first_forward", "evaluated", "bias")


def unit_diffs(u, rec):
    """One engine record against the oracle's answer for the unit."""
    oc, d = u["oc"], []
    if "over_capacity" in u:
        # the one unit whose duplications exceed its path capacity: the status, getBFB's path untouched, nothing published behind it
        if rec["status"] != ST_ERR_PATH_CAPACITY:
            d.append("status %d, expected ST_ERR_PATH_CAPACITY" % rec["status"])
        if rec["path"] != oc["path"]:
            d.append("getBFB's path of the unit over its capacity")
        if rec["header"]["path_indel_len"] > u["over_capacity"] or len(rec["runs"]) > u["over_capacity"]:
            d.append("lengths beyond the capacity: %d cells, %d from the runs" % (rec["header"]["path_indel_len"], len(rec["runs"])))
        return d
    if "over_steps" in u:
        # duplications repeated more junction steps than the unit has room for: the status in every stage, getBFB's path untouched
        if rec["status"] != ST_ERR_OUTJUNC_CAPACITY:
            d.append("status %d, expected ST_ERR_OUTJUNC_CAPACITY" % rec["status"])
        if rec["path"] != oc["path"]:
            d.append("getBFB's path of the unit over its step capacity")
        return d
    if rec["status"] != 0:
        return ["status %d" % rec["status"]]
    h = rec["header"]
    for k in _HEADER:
        if h[k] != oc[k]:
            d.append("%s %s, oracle %s" % (k, h[k], oc[k]))
    if bool(h["indel_printed"]) != oc["indel_printed"]:
        d.append("indel_printed %s, oracle %s" % (h["indel_printed"], oc["indel_printed"]))
    if (h["bkp_len"], h["path_len"], h["path_indel_len"], h["n_out_junc"]) != (len(oc["bkp"]), len(oc["path"]), len(oc["path_indel"]), len(u["out_juncs"])):
        d.append("lengths (bkp, path, path_indel, out_juncs) %s, oracle %s" % ((h["bkp_len"], h["path_len"], h["path_indel_len"], h["n_out_junc"]),
                                                                               (len(oc["bkp"]), len(oc["path"]), len(oc["path_indel"]), len(u["out_juncs"]))))
    for k in ("bkp", "path", "path_indel"):
        if rec[k] != oc[k]:
            first = next((i for i, (a, b) in enumerate(zip(rec[k], oc[k])) if a != b), min(len(rec[k]), len(oc[k])))
            d.append("%s differs from cell %d on (%d cells, oracle %d)" % (k, first, len(rec[k]), len(oc[k])))
    if rec["out_juncs"] != u["out_juncs"]:
        d.append("output junctions (%d, oracle %d)" % (len(rec["out_juncs"]), len(u["out_juncs"])))
    if rec["runs"] != oc["path_indel"]:
        d.append("the run-length form expands to %d cells, path_indel has %d" % (len(rec["runs"]), len(oc["path_indel"])))
    return d


def check_against_oracle(units, recs, tag=""):
    bad = {}
    for u, rec in zip(units, recs):
        d = unit_diffs(u, rec)
        if d:
            bad[u["name"]] = d
    assert not bad, (tag, len(bad), dict(list(bad.items())[:6]))


def same_records(units, xs, ys, tag=""):
    bad = {}
    for u, x, y in zip(units, xs, ys):
        if x != y:
            bad[u["name"]] = sorted(k for k in set(x) | set(y) if x.get(k) != y.get(k))
    assert not bad, (tag, len(bad), dict(list(bad.items())[:6]))
