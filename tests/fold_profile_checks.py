"""Checks of the fold-back arm profile (ambi_batch_fold_profile, csrc/ambi_fold_profile.hpp) shared by the CPU host-simulation tests
and the GPU tests (same assertions, different library).

Expected values never come from the stages under test: a plain Python walk written from the definitions -- a fold is a step whose
cells have opposite sign; its alignment is the first of (0,1) (-1,1) (0,2) (-2,1) (0,3) whose first pair is reverse-complementary and
its arm is how far that palindrome extends; cover[s] counts the folds whose span i-r+1 .. j+r-2 holds step s, added step by step;
per junction the folds credited to it and their longest arm -- over the ORACLE's path of the unit, with the unit's junction list
from the file's JUNC lines (junc_profile_checks.unit_junctions).  Every summary field, both per-junction arrays and both planes
in full are compared."""
import ctypes
import os

import numpy as np

import cases
import frag_profile_checks as fc
import junc_profile_checks as jc
import profile_checks as pc
from ambigram_amd import api, synth

FIELDS = ("status", "steps", "folds", "folds_perfect", "folds_gapped", "folds_open", "folds_unmatched", "max_arm", "max_arm_at", "max_cover",
          "max_cover_at", "steps_covered", "arm_sum")
ZERO = dict(dict.fromkeys(FIELDS, 0), max_arm_at=-1, max_cover_at=-1)
ALIGNMENTS = ((0, 1), (-1, 1), (0, 2), (-2, 1), (0, 3))
_raises = fc._raises


# ---- the plain walk ---------------------------------------------------------------------------------------------------
def walk(path_local, ends, status=0):
    """(fold[P-1], cover[P-1], folds[m], max_arm[m], summary) of a path of LOCAL signed ids over the junctions."""
    m = len(ends)
    if status < 0 or len(path_local) == 0:
        return [], [], [0] * m, [0] * m, dict(ZERO, status=status)
    c = list(path_local)
    P = len(c)
    steps = P - 1
    edge = {}
    for j, (s, t) in enumerate(ends):                   # lowest index first: setdefault keeps it
        edge.setdefault((s, t), j)
        edge.setdefault((-t, -s), j)
    fold, cover, folds, max_arm = [0] * steps, [0] * steps, [0] * m, [0] * m
    n = dict(perfect=0, gapped=0, open=0, unmatched=0)
    arms = []                                           # (k, alignment, arm)
    for k in range(steps):
        if (c[k] > 0) == (c[k + 1] > 0):
            continue
        al, arm = -1, 0
        for a, (dl, dr) in enumerate(ALIGNMENTS):
            i, j = k + dl, k + dr
            r = 0
            while i - r >= 0 and j + r < P and c[i - r] == -c[j + r]:
                r += 1
            if r > 0:
                al, arm = a, r
                for s in range(i - r + 1, j + r - 1):   # the span, step by step
                    cover[s] += 1
                assert i - r + 1 <= k <= j + r - 2
                break
        fold[k] = ((al + 2) << 24) | arm
        arms.append((k, al, arm))
        n["perfect" if al == 0 else "gapped" if al > 0 else "open"] += 1
        jn = edge.get((c[k], c[k + 1]))
        if jn is None:
            n["unmatched"] += 1
        else:
            folds[jn] += 1
            max_arm[jn] = max(max_arm[jn], arm)
    top_arm = max((r for _, _, r in arms), default=0)
    top_cover = max(cover, default=0)
    s = dict(status=status, steps=steps, folds=len(arms), folds_perfect=n["perfect"], folds_gapped=n["gapped"], folds_open=n["open"],
             folds_unmatched=n["unmatched"], max_arm=top_arm, max_arm_at=next((k for k, _, r in arms if r == top_arm), -1) if top_arm else -1,
             max_cover=top_cover, max_cover_at=cover.index(top_cover) if top_cover else -1, steps_covered=sum(v > 0 for v in cover),
             arm_sum=sum(r for _, _, r in arms))
    return fold, cover, folds, max_arm, s


def compare_unit(b, u, ends, path, status, tag, gidx=None):
    fold, cover, folds, max_arm, summary = walk(path, ends, status)
    got = b.unit_fold_juncs(u)
    assert got[0].tolist() == folds, (tag, "folds", got[0].tolist(), folds)
    assert got[1].tolist() == max_arm, (tag, "max_arm", got[1].tolist(), max_arm)
    assert got[2].tolist() == (list(range(len(ends))) if gidx is None else list(gidx)), (tag, "graph_index", got[2].tolist())
    s = b.unit_fold_profile(u)
    assert list(s) == list(FIELDS) and s == summary, (tag, s, summary)
    n = len(fold)
    half = n // 2                                       # the plane getter, in two halves
    for plane, want in ((0, fold), (1, cover)):
        have = b.unit_fold_plane(u, plane, 0, half).tolist() + b.unit_fold_plane(u, plane, half, n - half).tolist()
        assert have == want, (tag, "plane", plane, [(k, a, w) for k, (a, w) in enumerate(zip(have, want)) if a != w][:8])
    assert api.fold_arm(b.unit_fold_plane(u, 0)).tolist() == [v & 0xffffff for v in fold]
    return summary


class _Env:
    """AMBI_FOLD_WINDOW / AMBI_JPROFILE_JUNC_WINDOW for the calls inside."""
    def __init__(self, fwin=None, jwin=None):
        self.fwin, self.j = fwin, jc._Env(jwin, None)

    def __enter__(self):
        self.saved = os.environ.pop("AMBI_FOLD_WINDOW", None)
        if self.fwin:
            os.environ["AMBI_FOLD_WINDOW"] = str(self.fwin)
        self.j.__enter__()

    def __exit__(self, *exc):
        self.j.__exit__(*exc)
        os.environ.pop("AMBI_FOLD_WINDOW", None)
        if self.saved is not None:
            os.environ["AMBI_FOLD_WINDOW"] = self.saved


# ---- the units -------------------------------------------------------------------------------------------------------------
SPECS = (("chain", 9, 48, 100), ("wide", 11, 48, 100), ("mixed", 12, 48, 100), ("skew", 23, 64, 128), ("chain", 25, 128, 256), ("wide", 13, 64, 128))
RANDOM_SEEDS = (35, 42, 43)
_UNITS = {}


def units(oracle, workdir):
    """[(name, lh, sol or None, forward record, reversed record)]: readme6, the six synthetic units, the three random decompositions, a
    SHORTCUT unit without any fold and a unit whose .sol selects nothing (status -11); computed once."""
    if workdir not in _UNITS:
        src = [("readme6", os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol"))]
        for i, (tier, K, n, m) in enumerate(SPECS):
            s = synth.make_sample(n, m, tier, K, seed=7600 + i, imperfect=i % 2, n_del=i % 3, n_dup=(i + 1) % 2, name="fold%d" % i)
            lh, sols = s.write(workdir)
            src.append((s.name, lh, sols[0]))
        for seed in RANDOM_SEEDS:
            lh, sols = cases.random_decomposition(os.path.join(workdir, "foldrnd"), seed)
            src.append(("rnd%d" % seed, lh, sols[0]))
        nofbi = os.path.join(workdir, "fold_nofbi.lh")
        with open(nofbi, "w") as f:
            f.write(pc.NOFBI)
        src.append(("shortcut", nofbi, None))
        sol0 = os.path.join(workdir, "fold_empty.sol")
        with open(sol0, "w") as f:
            f.write("Optimal - objective value 0.00000000\n")
        src.append(("empty", os.path.join(cases.DATA, "readme6.lh"), sol0))
        out = []
        for name, lh, sol in src:
            sols = [sol] if sol else []
            out.append((name, lh, sol, oracle.run_bfb(lh, sols)["chr"][0], oracle.run_bfb(lh, sols, reversed_=True)["chr"][0]))
        _UNITS[workdir] = out
    return _UNITS[workdir]


def unit_status(name, oc):
    return -11 if name == "empty" else jc.oracle_status(oc)


def make_batch(lib, items):
    """(graphs, batch, [(junction indices, junction ends)]) of the given units, in order."""
    graphs, b, js = [], api.Batch(lib), []
    for name, lh, sol, oc, _ in items:
        g = api.Graph(lib, lh); graphs.append(g)
        if sol:
            b.add_chromosome_sol(g, 0, sol)
        else:
            b.add_chromosome(g, 0, [], [])
        idx, ends, _ = jc.unit_junctions(lh, g, oc["start"], oc["end"])
        js.append((idx, ends))
    return graphs, b, js


def check_profiled(b, items, js, tag, reversed_=False, whichs=(0, 1), stream=None):
    for which in whichs:
        b.fold_profile(which, stream); b.fold_profile_wait()
        for u, ((name, _, _, oc, orev), (idx, ends)) in enumerate(zip(items, js)):
            o = orev if reversed_ else oc
            st = unit_status(name, o)
            compare_unit(b, u, ends, jc.oracle_path(o, which) if st >= 0 else [], st, (tag, name, which), idx)


# ---- floors: what the units must offer for the comparison to mean something (CPU half, from the walk itself) ----------------
def check_floors(oracle, workdir):
    items = units(oracle, workdir)
    aligns, arms, covers, differs = set(), [], [], 0
    by_name = {}
    for name, lh, sol, oc, _ in items:
        st = unit_status(name, oc)
        if st < 0:
            continue
        per = []
        for which in (0, 1):
            path = jc.oracle_path(oc, which)
            fold, cover, _, _, s = walk(path, [], st)
            per.append((fold, cover))
            for v in fold:
                if v:
                    aligns.add((v >> 24) - 2); arms.append(v & 0xffffff)
            covers.append(s["max_cover"])
            by_name[(name, which)] = s
        differs += per[0] != per[1]
    assert {-1, 0, 1, 2} <= aligns, aligns
    assert any(1 <= r <= 7 for r in arms) and any(8 <= r <= 63 for r in arms), sorted(set(arms))
    assert 63 in arms and 64 in arms, sorted(set(arms))
    assert max(arms) >= 1024, max(arms)
    assert max(covers) >= 5, covers
    assert differs >= 1, "which = 1 must differ from which = 0 for some unit"
    r = by_name[("readme6", 1)]
    assert (r["steps"], r["folds"]) == (31, 7), r                          # P = 32, 7 folds
    big = by_name[("fold4", 0)]
    assert big["steps"] + 1 == 6392 and big["folds"] == 67 and big["max_arm"] == 3196 and big["max_cover"] == 5, big   # the largest path of the tests
    assert by_name[("shortcut", 1)]["folds"] == 0


def check_floors_served(lib, oracle, workdir):
    """The floors once more, from the planes the engine returns for the final paths of one batch of all units."""
    items = units(oracle, workdir)
    graphs, b, _ = make_batch(lib, items)
    b.upload(); b.run(0); b.download()
    b.fold_profile(1); b.fold_profile_wait()
    aligns, arms, covers = set(), [], []
    for u in range(len(items)):
        fold = b.unit_fold_plane(u, 0)
        fold = fold[fold != 0]
        aligns |= set(api.fold_align(fold).tolist()); arms += api.fold_arm(fold).tolist()
        covers.append(b.unit_fold_profile(u)["max_cover"])
    assert {-1, 0, 1, 2} <= aligns and any(1 <= r <= 7 for r in arms) and any(8 <= r <= 63 for r in arms) and 63 in arms and max(arms) >= 1024 and max(covers) >= 5
    pc.close_all(graphs, b)


# ---- one batch holding all units, and each unit alone ---------------------------------------------------------------------
def check_all_units(lib, oracle, workdir, fwin=None, jwin=None):
    """One batch of all units, which 0 and 1; then the same batch run reversed: other and often shorter paths, so stale cells and stale
    planes lie behind P."""
    with _Env(fwin, jwin):
        items = units(oracle, workdir)
        graphs, b, js = make_batch(lib, items)
        b.upload(); b.run(0); b.download()
        for u, (name, _, _, oc, _) in enumerate(items):     # precondition: the engine's paths and statuses are the oracle's
            assert b.unit_result(u)["status"] == unit_status(name, oc), (name, b.unit_result(u)["status"])
            if unit_status(name, oc) == 0:
                assert b.unit_path(u, 0).tolist() == oc["path"] and b.unit_path(u, 1).tolist() == oc["path_indel"], name
        check_profiled(b, items, js, ("all", fwin, jwin))
        b.run(api.FLAG_REVERSED); b.download()
        changed = 0
        for u, (name, _, _, oc, orev) in enumerate(items):
            if unit_status(name, orev) == 0:
                assert b.unit_path(u, 1).tolist() == orev["path_indel"], name
                changed += orev["path_indel"] != oc["path_indel"]
        assert changed >= 1, "the reversed run must change some path"
        check_profiled(b, items, js, ("all reversed", fwin, jwin), reversed_=True)
        pc.close_all(graphs, b)


def check_each_alone(lib, oracle, workdir):
    """Every unit in a batch of its own (the one-unit express path)."""
    for it in units(oracle, workdir):
        graphs, b, js = make_batch(lib, [it])
        b.upload(); b.run(0); b.download()
        check_profiled(b, [it], js, "alone")
        pc.close_all(graphs, b)


README_COVER = [1, 2, 2, 2, 2, 2, 2, 2, 3, 3, 2, 2, 3, 2, 2, 1, 2, 2, 3, 2, 2, 3, 3, 2, 2, 2, 2, 2, 2, 2, 1]


def check_readme(lib, oracle, workdir):
    """The README example as literals: 1+2+3+4+5+6+|6-5-4-3-2-|2+3+4+|4-3-|3+4+|4-3-2-|2+3+4+5+6+|6-5-4-3-2-1-."""
    it = units(oracle, workdir)[0]
    path = jc.oracle_path(it[3], 1)
    assert path == [1, 2, 3, 4, 5, 6, -6, -5, -4, -3, -2, 2, 3, 4, -4, -3, 3, 4, -4, -3, -2, 2, 3, 4, 5, 6, -6, -5, -4, -3, -2, -1]
    graphs, b, js = make_batch(lib, [it])
    b.upload(); b.run(0); b.download()
    b.fold_profile(1); b.fold_profile_wait()
    fold = b.unit_fold_plane(0, 0)
    ks = np.nonzero(fold)[0].tolist()
    assert ks == [5, 10, 13, 15, 17, 20, 25]
    assert api.fold_align(fold[ks]).tolist() == [0] * 7 and api.fold_arm(fold[ks]).tolist() == [5, 3, 2, 16, 2, 3, 5]
    s = b.unit_fold_profile(0)
    assert (s["folds"], s["folds_perfect"], s["max_arm"], s["max_arm_at"], s["arm_sum"], s["steps_covered"], s["max_cover"], s["max_cover_at"]) == (7, 7, 16, 15, 36, 31, 3, 8), s
    assert b.unit_fold_plane(0, 1).tolist() == README_COVER
    compare_unit(b, 0, js[0][1], path, 0, "readme", js[0][0])
    pc.close_all(graphs, b)


# ---- sharded, streams, device views ------------------------------------------------------------------------------------
def check_sharded(lib, oracle, workdir, devices):
    items = units(oracle, workdir)
    graphs, b, js = make_batch(lib, items)
    b.run_sharded(0, devices=devices)
    check_profiled(b, items, js, ("sharded", tuple(devices)))
    with _raises(-32):
        b.fold_profile_device()          # one block per share: no single device view
    with _raises(-32):
        b.fold_planes_device()
    pc.close_all(graphs, b)


def check_request_paths(lib, oracle, workdir, run_stream=None, req_stream=None):
    """The run on one stream, every request on another; a request nobody waited for; beside the junction profile; a batch closed with a
    request in flight and the next batch on its lease."""
    items = units(oracle, workdir)
    graphs, b, js = make_batch(lib, items)
    b.upload()
    for which in (0, 1):
        b.run(0, run_stream)
        b.fold_profile(which, req_stream); b.fold_profile_wait()
        b.download()
        check_profiled(b, items, js, "other stream", whichs=(which,), stream=req_stream)
    b.run(0, run_stream)
    b.fold_profile(0, req_stream); b.fold_profile(1, req_stream); b.junc_profile(1, req_stream)
    b.junc_profile_wait(); b.fold_profile_wait()
    b.download()
    for u, ((name, lh, _, oc, _), (idx, ends)) in enumerate(zip(items, js)):
        st = unit_status(name, oc)
        compare_unit(b, u, ends, jc.oracle_path(oc, 1) if st >= 0 else [], st, ("unwaited", name), idx)
        if st >= 0:                                     # the fold counts against the junction profile of the same run
            count = b.unit_junc_usage(u)[0]
            assert all(f <= c for f, c in zip(b.unit_fold_juncs(u)[0].tolist(), count.tolist())), name
    b.run(0, run_stream)
    b.fold_profile(1, req_stream)
    pc.close_all(graphs, b)
    graphs, b, js = make_batch(lib, items[:4][::-1])
    b.upload(); b.run(0, run_stream); b.download()
    check_profiled(b, items[:4][::-1], js, "after a close in flight", stream=req_stream)
    pc.close_all(graphs, b)


def check_device_views(lib, oracle, workdir):
    """ambi_batch_fold_profile_device / ambi_batch_fold_planes_device: block and planes in device memory, read back through torch, are
    what the host getters return, byte for byte; the block ends exactly at `bytes`; every unit_off is a multiple of 16."""
    import torch
    from ambigram_amd.dist import _DevBytes
    items = units(oracle, workdir)
    graphs, b, js = make_batch(lib, items)
    stream = torch.cuda.Stream()
    b.upload(); b.run(0, stream.cuda_stream)
    b.fold_profile(1, stream.cuda_stream); b.fold_profile_wait()
    ptr, nbytes = b.fold_profile_device()
    U = len(items)
    assert ptr and nbytes >= 56 * U
    raw = torch.as_tensor(_DevBytes(ptr, nbytes), device="cuda").cpu().numpy()
    dptr, dbytes, doff = b.fold_planes_device()
    half = dbytes // 2
    assert dptr and dbytes > 0 and dbytes % 32 == 0 and all(int(o) % 16 == 0 and 0 <= int(o) < half for o in doff) and sorted(doff.tolist()) == doff.tolist()
    draw = torch.as_tensor(_DevBytes(dptr, dbytes), device="cuda").cpu().numpy()
    off = (56 * U + 15) & ~15
    for u in range(U):
        p = b.unit_fold_profile(u)
        s = raw[56 * u:56 * u + 56]
        assert s[:48].view(np.int32).tolist() + s[48:].view(np.int64).tolist() == [p[k] for k in FIELDS], u
        folds, max_arm, _ = b.unit_fold_juncs(u)
        m = len(folds)
        for arr in (folds, max_arm):
            assert raw[off:off + 4 * m].tobytes() == arr.tobytes(), u
            off += (4 * m + 15) & ~15
        for plane in (0, 1):
            vals = b.unit_fold_plane(u, plane)
            at = plane * half + int(doff[u])
            assert len(vals) == p["steps"] and draw[at:at + 4 * len(vals)].tobytes() == vals.tobytes(), (u, plane)
            assert int(doff[u]) + 4 * len(vals) <= (int(doff[u + 1]) if u + 1 < U else half), u
    assert off == nbytes
    pc.close_all(graphs, b)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------
def check_cli(lib, exe, cwd, oracle, workdir):
    import test_cli_dropin as t
    items = units(oracle, workdir)
    (_, readme, rsol, _, _), (_, lh2, sol2, _, _) = items[0], items[1]
    outs = []
    for k, extra in enumerate(([], ["--fold_profile", "fold.tsv", "--fold_arms", "arms.tsv"])):
        sub = os.path.join(cwd, "run%d" % k)
        os.makedirs(sub)
        bindir = os.path.join(sub, "bin")
        t.fake_cbc(bindir, [rsol, sol2])
        r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", readme + "," + lh2, "--lp_prefix", "two", *extra)
        assert r.returncode == 0, r.stderr
        outs.append((r.stdout, r.stderr, open(os.path.join(sub, "simulation_sv.txt"), "rb").read(), sorted(x for x in os.listdir(sub) if x != "bin")))
    assert outs[0][:3] == outs[1][:3]                                      # stdout, stderr, side file: unchanged by the options
    assert outs[1][3] == sorted(outs[0][3] + ["fold.tsv", "arms.tsv"])
    want_p, want_a = [], []
    for lh, sol in ((readme, rsol), (lh2, sol2)):
        oc = oracle.run_bfb(lh, [sol])["chr"][0]
        g = api.Graph(lib, lh)
        idx, ends, _ = jc.unit_junctions(lh, g, oc["start"], oc["end"])
        m = len(g.junctions()["src"])
        g.close()
        fold, cover, folds, max_arm, s = walk(jc.oracle_path(oc, 1), ends, jc.oracle_status(oc))
        want_p.append("\t".join(["U", lh, "0"] + [str(s[k]) for k in FIELDS]))
        rows = {j: (0, folds[k], max_arm[k]) for k, j in enumerate(idx)}
        for j in range(m):
            c, f, a = rows.get(j, (-1, 0, 0))
            want_p.append("\t".join(["J", lh, str(c), str(j), str(f), str(a)]))
        for k, v in enumerate(fold):
            if v:
                want_a.append("\t".join([lh, "0", str(k), str((v >> 24) - 2), str(v & 0xffffff), str(cover[k] - 1)]))
    got_p = open(os.path.join(cwd, "run1", "fold.tsv")).read().splitlines()
    got_a = open(os.path.join(cwd, "run1", "arms.tsv")).read().splitlines()
    assert got_p == want_p and got_a == want_a
    assert len(got_a) > 7 and any(line.split("\t")[5] not in ("0", "-1") for line in got_a)
    # a PROP C2 sample: its printed paths are rebuilt on the host -- refused where --junc_profile is, exit status 2, no file
    for opt, name in (("--fold_profile", "fold.tsv"), ("--fold_arms", "arms.tsv"), ("--junc_profile", "junc.tsv")):
        sub = os.path.join(cwd, "c2" + name)
        os.makedirs(sub)
        bindir = os.path.join(sub, "bin")
        t.fake_cbc(bindir, [os.path.join(cases.DATA, "readme_c2_chr0.sol"), os.path.join(cases.DATA, "readme_c2_chr1.sol")])
        r = t.run_cli(exe, sub, bindir, "--op", "bfb", "--in_lh", os.path.join(cases.DATA, "readme_c2.lh"), "--lp_prefix", "c2", opt, name)
        assert r.returncode == 2 and opt in r.stderr and "PROP I1 / C1 / I2 / C2" in r.stderr, (r.returncode, r.stderr)
        assert not os.path.exists(os.path.join(sub, name))
    r = t.run_cli(exe, sub, bindir, "--help")
    assert "--fold_profile" in r.stdout and "--fold_arms" in r.stdout


# ---- argument and state errors ------------------------------------------------------------------------------------------
def check_errors(lib):
    lh, sol = (os.path.join(cases.DATA, "readme6." + x) for x in ("lh", "sol"))
    g = api.Graph(lib, lh); b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol)
    for call in (lambda: b.fold_profile(1), b.fold_profile_wait):
        with _raises(-32):                                 # AMBI_ERR_STATE: nothing uploaded
            call()
    b.upload()
    for call in (lambda: b.fold_profile(1), b.fold_profile_wait, lambda: b.unit_fold_profile(0), lambda: b.unit_fold_juncs(0),
                 lambda: b.unit_fold_plane(0, 0, 0, 1), b.fold_profile_device, b.fold_planes_device):
        with _raises(-32):                                 # uploaded, never run
            call()
    b.run(0); b.download()
    with _raises(-32):
        b.unit_fold_profile(0)                             # run, not profiled
    with _raises(-32):
        b.fold_profile_wait()                              # nothing queued
    for which in (2, -1):
        with _raises(-33):                                 # AMBI_ERR_ARG
            b.fold_profile(which)
    b.junc_profile(1); b.junc_profile_wait()
    with _raises(-32):
        b.unit_fold_profile(0)                             # another kind's request does not answer for this one
    with _raises(-32):
        b.unit_fold_plane(0, 1, 0, 1)
    b.fold_profile(1); b.fold_profile_wait()
    buf = [(ctypes.c_int32 * 8)() for _ in range(3)]
    assert lib.ambi_batch_unit_fold_juncs(b.h, 0, *buf, 3) == -33          # cap < m
    assert lib.ambi_batch_unit_fold_juncs(b.h, 0, buf[0], None, None, 4) == 4
    assert lib.ambi_batch_unit_fold_juncs(b.h, 0, None, buf[1], buf[2], 4) == 4 and list(buf[2][:4]) == [0, 1, 2, 3]
    assert sum(buf[0][:4]) + b.unit_fold_profile(0)["folds_unmatched"] == 7 and max(buf[1][:4]) == 16
    for u in (1, -1):
        with _raises(-33):
            b.unit_fold_profile(u)                         # no such unit
        assert lib.ambi_batch_unit_fold_juncs(b.h, u, *buf, 8) == -33
        with _raises(-33):
            b.unit_fold_plane(u, 0, 0, 1)
    out = (ctypes.c_int32 * 40)()
    for first, n in ((-1, 1), (0, 32), (31, 1), (32, 0), (0, -1), (30, 2)):        # outside [0, P - 1] = [0, 31]
        for plane in (0, 1):
            assert lib.ambi_batch_unit_fold_plane(b.h, 0, plane, first, n, out) == -33, (plane, first, n)
    for plane in (2, -1):
        assert lib.ambi_batch_unit_fold_plane(b.h, 0, plane, 0, 1, out) == -33
    assert lib.ambi_batch_unit_fold_plane(b.h, 0, 0, 0, 1, None) == -33
    assert lib.ambi_batch_unit_fold_plane(b.h, 0, 1, 31, 0, None) == 0
    assert lib.ambi_batch_unit_fold_plane(b.h, 0, 0, 5, 1, out) == 0 and out[0] == (2 << 24) | 5
    assert lib.ambi_batch_unit_fold_plane(b.h, 0, 1, 0, 31, out) == 0 and list(out[:31]) == README_COVER
    off = (ctypes.c_int64 * 1)()
    assert lib.ambi_batch_fold_planes_device(b.h, None, None, off, 0) == -33     # cap < n_units
    b.run(0)
    with _raises(-32):
        b.unit_fold_profile(0)                             # a new run: the old profile is gone
    b.wait()
    b.close(); g.close()
