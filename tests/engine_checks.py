"""Parity checks shared by the CPU host-simulation tests and the GPU tests (same assertions, different library)."""
import os
import numpy as np

import cases
import parity
from ambigram_amd import api


def check_fixed_and_synthetic(lib, oracle, workdir, small_only):
    bad = {}
    for name, lh, sols in cases.fixed_cases() + cases.synthetic_cases(workdir, small_only=small_only):
        d = parity.compare(lib, oracle, lh, sols)
        if d:
            bad[name] = d
        d = parity.compare(lib, oracle, lh, sols, reversed_=True, keep_orders=False)
        if d:
            bad[name + "/reversed"] = d
    assert not bad, bad


def check_search_budget(lib, oracle, workdir):
    """first_budget=1 forces the parallel search path whenever the first order is not the valid one."""
    bad = {}
    for name, lh, sols in cases.synthetic_cases(workdir, small_only=True)[:6]:
        d = parity.compare(lib, oracle, lh, sols, first_budget=1, keep_orders=False)
        if d:
            bad[name] = d
    assert not bad, bad


def check_random_decompositions(lib, oracle, workdir, seeds, budget=0):
    stats = dict(valid=0, none=0, deep=0, reversed_pass=0, refused=0)
    for seed in seeds:
        lh, sols = cases.random_decomposition(workdir, seed)
        for rev in (False, True):
            o = oracle.run_bfb(lh, sols, reversed_=rev, keep_orders=True)
            assert o["ok"], o["err"]
            oc = o["chr"][0]
            if oc["shortcut"]:
                continue
            g = api.Graph(lib, lh)
            b = api.Batch(lib)
            if budget:
                b.configure(first_budget=budget)
            b.add_chromosome_sol(g, 0, sols[0])
            b.upload(); b.run(api.FLAG_REVERSED if rev else 0); b.download()
            r = b.unit_result(0)
            if oc["ub_valid"]:
                # the reference reads out of bounds while rewriting a VALID order: its printed path is not defined by its
                # source; the engine refuses.  (The same read on an order that is invalid anyway changes nothing.)
                assert r["status"] == -12, (seed, r)
                stats["refused"] += 1
                continue
            assert r["num_orders"] == oc["num_orders"], (seed, rev)
            K = r["n_nodes"]
            if oc["num_orders"] and oc["num_orders"] <= 20000:
                assert b.unit_orders(0, 0, r["num_orders"], K).tolist() == oc["orders"], (seed, rev)
            if oc["first_valid"] < 0:
                assert r["status"] == api.ST_NO_VALID_ORDER, (seed, rev, r)
                assert r["evaluated"] == oc["evaluated"], (seed, rev, r["evaluated"], oc["evaluated"])
                stats["none"] += 1
            else:
                assert r["status"] == 0, (seed, rev, r)
                assert (r["first_valid"], r["first_forward"], r["evaluated"]) == (oc["first_valid"], oc["first_forward"], oc["evaluated"]), (seed, rev)
                assert b.unit_bkp(0).tolist() == oc["bkp"], (seed, rev)
                assert b.unit_path(0, 0).tolist() == oc["path"], (seed, rev)
                assert b.unit_path(0, 1).tolist() == oc["path_indel"], (seed, rev)
                stats["valid"] += 1
                if oc["first_valid"] > 0:
                    stats["deep"] += 1
                if oc["first_forward"] == (1 if rev else 0):
                    stats["reversed_pass"] += 1
            b.close(); g.close()
        for f in [lh] + list(sols):    # long runs (tests/soak.py) must not fill the temporary directory
            try:
                os.remove(f)
            except OSError:
                pass
    return stats


def check_edge_cases(lib, oracle, workdir):
    import os
    # (1) chromosome without any fold-back inversion -> shortcut path 1+..n+ (localhap.cpp:164-170)
    lh = os.path.join(workdir, "nofbi.lh")
    with open(lh, "w") as f:
        f.write("SAMPLE_NAME nofbi\nAVG_CHR_SEG_DP 30\nAVG_WHOLE_HOST_DP 30\nAVG_JUNC_DP 30\nPURITY 1\nAVG_TUMOR_PLOIDY 2\n"
                "PLOIDY 2m1\nVIRUS_START 5\nSOURCE 1\nSINK 4\n"
                "SEG H:1:chr1:1:10 30.0 1.0\nSEG H:2:chr1:11:20 30.0 1.0\nSEG H:3:chr1:21:30 30.0 1.0\nSEG H:4:chr1:31:40 30.0 1.0\n"
                "JUNC H:1:+ H:2:+ 30.0 1.0 U B\nJUNC H:2:+ H:3:+ 30.0 1.0 U B\nJUNC H:1:+ H:4:+ 30.0 1.0 U B\n")
    assert parity.compare(lib, oracle, lh, []) == []
    # (2) infeasible ILP -> reference path + "ILP is unsolvable." (localhap.cpp:213-220)
    sol = os.path.join(workdir, "infeasible.sol")
    with open(sol, "w") as f:
        f.write("Infeasible - objective value 0.00000000\n")
    assert parity.compare(lib, oracle, os.path.join(cases.DATA, "readme6.lh"), [sol]) == []
    # (3) a .sol that selects nothing -> the reference indexes an empty order; the engine refuses
    sol0 = os.path.join(workdir, "empty.sol")
    with open(sol0, "w") as f:
        f.write("Optimal - objective value 0.00000000\n")
    g = api.Graph(lib, os.path.join(cases.DATA, "readme6.lh"))
    b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sol0)
    b.upload(); b.run(0); b.download()
    assert b.unit_result(0)["status"] == -11
    # (4) missing .sol / missing .lh error codes (localhap.cpp:187-190, Graph.cpp:111-114)
    import pytest
    with pytest.raises(api.AmbiError) as e:
        b2 = api.Batch(lib); b2.add_chromosome_sol(g, 0, os.path.join(workdir, "nope.sol"))
    assert e.value.code == -7
    with pytest.raises(api.AmbiError) as e:
        api.Graph(lib, os.path.join(workdir, "nope.lh"))
    assert e.value.code == -1


def check_juncs_file(lib, oracle, workdir):
    """.juncs components (readComponents, LGM.cpp:5096-5156): adds junctions / bumps CN before getJuncCN."""
    import os
    j = os.path.join(workdir, "readme6.juncs")
    with open(j, "w") as f:
        f.write("6+ 6- 5- 4- 3- 2- 2+\n2- 2+ 3+ 4+ 5+ 6+ 6-\n6+ 6- 5- 4- 3-\n")   # README.md:173-177
    lh = os.path.join(cases.DATA, "readme6.lh")
    assert parity.compare(lib, oracle, lh, [os.path.join(cases.DATA, "readme6.sol")], juncs=j) == []


def check_batch_many_units(lib, oracle, workdir, n_samples):
    """Many independent samples in ONE batch == each sample alone (units do not interact)."""
    from ambigram_amd import synth
    graphs, b = [], api.Batch(lib)
    expect = []
    for i in range(n_samples):
        tier, K = [("chain", 7), ("wide", 7), ("mixed", 7)][i % 3]
        s = synth.make_sample(48, 100, tier, K, seed=5000 + i, imperfect=i % 2, n_del=i % 2)
        lh, sols = s.write(workdir, "b%d" % i)
        g = api.Graph(lib, lh)
        graphs.append(g)
        b.add_chromosome_sol(g, 0, sols[0])
        expect.append(oracle.run_bfb(lh, sols)["chr"][0])
    b.upload(); b.run(0); b.download()
    for i, oc in enumerate(expect):
        r = b.unit_result(i)
        assert r["status"] == 0 and r["num_orders"] == oc["num_orders"], i
        assert b.unit_path(i, 0).tolist() == oc["path"], i
        assert b.unit_path(i, 1).tolist() == oc["path_indel"], i
    # a second run over the resident batch gives the same answer (idempotence)
    b.run(0); b.download()
    for i, oc in enumerate(expect):
        assert b.unit_path(i, 1).tolist() == oc["path_indel"], i
    return b, graphs, expect


def check_enumerate_variants(lib, oracle, workdir, big=False):
    """The order table (allTopologicalOrders, LGM.cpp:3380-3409) through every enumeration path of the engine:
    block emission with several block sizes (AMBI_BLOCK_MAX: 1 = one row per block ... 1024), with an LDS budget that
    forces the general per-lane DFS (AMBI_BLOCK_LDS=64), and with few / many rows per lane -- all byte-identical to the
    oracle's orders."""
    import os
    from ambigram_amd import synth
    specs = [("wide", 11, 40, 90), ("mixed", 12, 48, 100), ("chain", 9, 40, 80), ("wide", 13, 64, 128)]
    if big:
        specs += [("wide", 15, 96, 200), ("mixed", 22, 128, 256), ("chain", 35, 256, 512)]
    specs += [("skew", 23, 64, 128), ("skew", 27, 64, 128), ("skew", 34, 96, 200), ("skew", 45, 128, 256), ("skew", 50, 128, 256)]
    samples = []
    for i, (tier, K, nseg, njunc) in enumerate(specs):
        s = synth.make_sample(nseg, njunc, tier, K, seed=7100 + i)
        lh, sols = s.write(workdir, "ev%d" % i)
        oc = oracle.run_bfb(lh, sols, keep_orders=True)["chr"][0]
        samples.append((lh, sols, oc))
    variants = [({}, 0), ({"AMBI_BLOCK_MAX": "1"}, 0), ({"AMBI_BLOCK_MAX": "6"}, 64), ({"AMBI_BLOCK_MAX": "1024", "AMBI_BLOCK_LDS": "150000"}, 0),
                ({"AMBI_BLOCK_LDS": "64"}, 0), ({"AMBI_BLOCK_LDS": "64"}, 100000), ({"AMBI_BLOCK_MAX": "37"}, 1 << 20),
                # budgets in which the directory of most units does not fit but tables + suffix rows do: the
                # directory-free block walk, started at the top of the table and (few rows per lane) in the middle of it
                ({"AMBI_BLOCK_LDS": "12288"}, 0), ({"AMBI_BLOCK_LDS": "8192", "AMBI_BLOCK_MAX": "24"}, 256), ({"AMBI_BLOCK_LDS": "6144"}, 64)]
    saved = {k: os.environ.get(k) for k in ("AMBI_BLOCK_MAX", "AMBI_BLOCK_LDS")}
    try:
        for env, lanes in variants:
            for k in saved:
                os.environ.pop(k, None)
            os.environ.update(env)
            graphs, b = [], api.Batch(lib)
            if lanes:
                b.configure(target_lanes=lanes)
            for lh, sols, oc in samples:
                g = api.Graph(lib, lh)
                graphs.append(g)
                b.add_chromosome_sol(g, 0, sols[0])
            b.upload(); b.run(0); b.download()
            for u, (lh, sols, oc) in enumerate(samples):
                r = b.unit_result(u)
                assert r["status"] == 0 and r["num_orders"] == oc["num_orders"], (env, lanes, u, r)
                got = b.unit_orders(u, 0, r["num_orders"], r["n_nodes"])
                if oc["orders"]:
                    assert got.tolist() == oc["orders"], (env, lanes, u)
                assert b.unit_path(u, 1).tolist() == oc["path_indel"], (env, lanes, u)
            b.close()
            for g in graphs:
                g.close()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def check_large_lattice(lib, oracle, workdir, K=50, k2=5):
    """A lattice with more ideals than the group-local search holds (256): (K-k2)(k2+1)+1 ideals take the HBM path of
    the lattice search.  R = C(K-1,k2) rows; the table is checked against the oracle's order count, by sampling rows
    (permutation, DAG-respecting, lexicographically increasing) and through the reconstructed path."""
    from ambigram_amd import synth
    s = synth.make_sample(128, 256, "skew%d" % k2, K, seed=7300 + K)
    lh, sols = s.write(workdir, "ll%d" % K)
    oc = oracle.run_bfb(lh, sols)["chr"][0]
    g = api.Graph(lib, lh)
    b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sols[0])
    b.upload(); b.run(0); b.download()
    r = b.unit_result(0)
    assert r["status"] == 0 and r["num_orders"] == oc["num_orders"], (r, oc["num_orders"])
    assert (K - k2) * (k2 + 1) + 1 > 256
    R = r["num_orders"]
    for first in (0, R // 3, R - 5000):
        rows = b.unit_orders(0, first, 5000, K)
        assert np.array_equal(np.sort(rows, axis=1), np.tile(np.arange(K, dtype=np.uint8), (len(rows), 1)))
        a, bb = rows[:-1].astype(np.int16), rows[1:].astype(np.int16)
        neq = a != bb
        fi = neq.argmax(axis=1)
        ii = np.arange(len(a))
        assert neq.any(axis=1).all() and (a[ii, fi] < bb[ii, fi]).all()
    assert b.unit_path(0, 0).tolist() == oc["path"] and b.unit_path(0, 1).tolist() == oc["path_indel"]
    b.close(); g.close()


def check_all_mode(lib, oracle, workdir, seeds=range(40)):
    """--all (LGM.cpp:3672-3695): every valid order is reported, in the reference's print order, with the orientation
    flip only when the last order of the first pass is invalid; `evaluated` counts every order of the executed passes."""
    bad = {}
    for name, lh, sols in cases.fixed_cases() + cases.synthetic_cases(workdir, small_only=True)[:8]:
        for rev in (False, True):
            d = parity.compare(lib, oracle, lh, sols, reversed_=rev, all_=True, keep_orders=False)
            if d:
                bad[name + ("/reversed" if rev else "")] = d
    stats = dict(flipped=0, multi=0, none=0)
    for seed in seeds:
        lh, sols = cases.random_decomposition(workdir, seed)
        for rev in (False, True):
            o = oracle.run_bfb(lh, sols, reversed_=rev, all_=True)
            assert o["ok"], o["err"]
            oc = o["chr"][0]
            if oc["shortcut"] or oc["ub_valid"]:
                continue
            d = parity.compare(lib, oracle, lh, sols, reversed_=rev, all_=True, keep_orders=False)
            if oc["first_valid"] < 0:
                # no valid order: the engine reports the status, the oracle an empty path
                stats["none"] += 1
                continue
            if d:
                bad["random%d%s" % (seed, "/reversed" if rev else "")] = d
            stats["multi"] += len(oc["all_paths"]) > 1
            stats["flipped"] += oc["evaluated"] > oc["num_orders"]
    assert not bad, bad
    return stats


def check_mixed_batch(lib, oracle, workdir, big=False):
    """ONE batch with every kind of unit side by side: all three row-width classes of the enumerate kernels (K <= 20,
    <= 32, <= 63), units whose block image does not fit next to units whose image does (small AMBI_BLOCK_LDS budget),
    a chromosome without fold-backs (shortcut), an infeasible .sol, units without any valid order and units whose first
    valid order lies behind the scan budget.  Every unit equals its own oracle run."""
    import os
    from ambigram_amd import synth
    specs = [("chain", 9, 48, 100), ("wide", 11, 48, 100), ("mixed", 12, 48, 100), ("skew", 23, 64, 128), ("skew", 27, 64, 128),
             ("skew", 34, 96, 200), ("skew", 45, 128, 256), ("wide", 13, 64, 128), ("chain", 25, 128, 256)]
    if big:
        specs += [("wide", 15, 96, 200), ("skew", 50, 128, 256), ("wide", 19, 256, 512)]
    items = []
    for i, (tier, K, nseg, njunc) in enumerate(specs):
        s = synth.make_sample(nseg, njunc, tier, K, seed=7600 + i, imperfect=i % 2, n_del=i % 3)
        lh, sols = s.write(workdir, "mb%d" % i)
        items.append((lh, sols[0]))
    for seed in (3, 5, 8, 13, 21, 34):
        lh, sols = cases.random_decomposition(workdir, 900 + seed)
        items.append((lh, sols[0]))
    # shortcut (no fold-back) and infeasible
    nofbi = os.path.join(workdir, "mb_nofbi.lh")
    with open(nofbi, "w") as f:
        f.write("SAMPLE_NAME nofbi\nAVG_CHR_SEG_DP 30\nAVG_WHOLE_HOST_DP 30\nAVG_JUNC_DP 30\nPURITY 1\nAVG_TUMOR_PLOIDY 2\n"
                "PLOIDY 2m1\nVIRUS_START 5\nSOURCE 1\nSINK 4\n"
                "SEG H:1:chr1:1:10 30.0 1.0\nSEG H:2:chr1:11:20 30.0 1.0\nSEG H:3:chr1:21:30 30.0 1.0\nSEG H:4:chr1:31:40 30.0 1.0\n"
                "JUNC H:1:+ H:2:+ 30.0 1.0 U B\nJUNC H:2:+ H:3:+ 30.0 1.0 U B\nJUNC H:1:+ H:4:+ 30.0 1.0 U B\n")
    infeasible = os.path.join(workdir, "mb_infeasible.sol")
    with open(infeasible, "w") as f:
        f.write("Infeasible - objective value 0.00000000\n")
    items.append((nofbi, None))
    items.append((os.path.join(cases.DATA, "readme6.lh"), infeasible))
    expect = []
    for lh, sol in items:
        o = oracle.run_bfb(lh, [sol] if sol else [], keep_orders=True)
        assert o["ok"], o["err"]
        expect.append(o["chr"][0])
    saved = {k: os.environ.get(k) for k in ("AMBI_BLOCK_LDS",)}
    try:
        for lds in (None, "6000"):          # 6000 bytes: only the smallest images fit, the rest take the general path
            os.environ.pop("AMBI_BLOCK_LDS", None)
            if lds:
                os.environ["AMBI_BLOCK_LDS"] = lds
            graphs, b = [], api.Batch(lib)
            b.configure(first_budget=3)
            for lh, sol in items:
                g = api.Graph(lib, lh)
                graphs.append(g)
                if sol:
                    b.add_chromosome_sol(g, 0, sol)
                else:
                    b.add_chromosome(g, 0, [], [])
            b.upload(); b.run(0); b.download()
            for u, oc in enumerate(expect):
                r = b.unit_result(u)
                tag = (lds, u, items[u][0])
                if oc["shortcut"] or oc["infeasible"]:
                    assert r["status"] == (api.ST_SHORTCUT if oc["shortcut"] else api.ST_INFEASIBLE), tag
                    want = oc["path_indel"] or oc["path"]      # the reference path 1+ .. n+ (no indelBFB on this branch)
                    assert b.unit_path(u, 1).tolist() == want or not want, tag
                    continue
                if oc["ub_valid"]:
                    assert r["status"] == -12, tag
                    continue
                assert r["num_orders"] == oc["num_orders"], tag
                if oc["orders"]:
                    assert b.unit_orders(u, 0, r["num_orders"], r["n_nodes"]).tolist() == oc["orders"], tag
                if oc["first_valid"] < 0:
                    assert r["status"] == api.ST_NO_VALID_ORDER and r["evaluated"] == oc["evaluated"], tag
                    continue
                assert r["status"] == 0, (tag, r)
                assert (r["first_valid"], r["first_forward"], r["evaluated"]) == (oc["first_valid"], oc["first_forward"], oc["evaluated"]), tag
                assert b.unit_bkp(u).tolist() == oc["bkp"], tag
                assert b.unit_path(u, 0).tolist() == oc["path"] and b.unit_path(u, 1).tolist() == oc["path_indel"], tag
            b.close()
            for g in graphs:
                g.close()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def check_max_sizes(lib, oracle, workdir):
    """The engine's documented limits: 63 DAG nodes per unit on the fast path, 64..255 on the wide path
    (tests/test_wide_units.py), 256 are refused when the unit is added;
    a path longer than the 65 536 cells the full finish stage can hold in group memory is served by the lean stage (runs
    only); if its SVs edit the path, by the direct full-stage launch with the cells in device memory -- ST_ERR_PATH_CAPACITY
    only where the group-memory form runs."""
    import pytest
    from ambigram_amd import synth
    for tier, K in (("chain", 63), ("skew", 63)):
        s = synth.make_sample(512, 1024, tier, K, seed=4242)
        lh, sols = s.write(workdir, "max_%s%d" % (tier, K))
        o = oracle.run_bfb(lh, sols)["chr"][0]
        assert len(o["path"]) > 65536                       # really beyond the group-memory limit
        g = api.Graph(lib, lh)
        b = api.Batch(lib)
        b.add_chromosome_sol(g, 0, sols[0])
        b.upload(); b.run(0); b.download()
        r = b.unit_result(0)
        assert r["status"] == 0 and r["n_nodes"] == K and r["num_orders"] == o["num_orders"], r
        assert b.unit_path(0, 0).tolist() == o["path"] and b.unit_path(0, 1).tolist() == o["path_indel"]
        b.close(); g.close()
    s = synth.make_sample(620, 1300, "chain", 256, seed=4242)
    lh, sols = s.write(workdir, "max_chain256")
    g = api.Graph(lib, lh)
    with pytest.raises(api.AmbiError) as e:
        api.Batch(lib).add_chromosome_sol(g, 0, sols[0])
    assert e.value.code == -10
    g.close()
    s = synth.make_sample(512, 1024, "chain", 64, seed=4242)            # one node more than the fast path takes: the wide path, same long path
    lh, sols = s.write(workdir, "max_chain64")
    o = oracle.run_bfb(lh, sols)["chr"][0]
    g = api.Graph(lib, lh)
    b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sols[0])
    b.upload(); b.run(0); b.download()
    r = b.unit_result(0)
    assert r["status"] == 0 and r["n_nodes"] == 64 and r["num_orders"] == o["num_orders"], r
    assert b.unit_path(0, 0).tolist() == o["path"] and b.unit_path(0, 1).tolist() == o["path_indel"]
    b.close(); g.close()
    s = synth.make_sample(512, 1024, "chain", 63, seed=4242, n_del=2)      # long path AND an SV that edits it
    lh, sols = s.write(workdir, "max_chain63_del")
    o = oracle.run_bfb(lh, sols)["chr"][0]
    assert len(o["path"]) > 65536 and o["path_indel"] != o["path"]
    g = api.Graph(lib, lh)
    b = api.Batch(lib)
    b.add_chromosome_sol(g, 0, sols[0])
    b.upload(); b.run(0); b.download()
    r = b.unit_result(0)
    if r["status"] == 0:    # the direct full-stage launch keeps the path cells in device memory: no limit but the unit's own capacity
        assert b.unit_path(0, 0).tolist() == o["path"] and b.unit_path(0, 1).tolist() == o["path_indel"]
    else:                   # the form with the cells in group memory (AMBI_DIRECT_EXT=0, or a unit the lean stage handed over)
        assert r["status"] == -14
    b.close(); g.close()


def check_injected_validity(lib, oracle, workdir):
    """Control flow around the per-order evaluation of getBFB (LGM.cpp:3519-3696) at places no known input reaches.

    An exhaustive search (tests/tools/search_mixed_validity.py: every element set of up to 5 patterns/loops over 4 and 5
    segments, both orientations, 360 000+ runs of the oracle) found NO unit whose orders differ in validity, so on real
    inputs the first valid order is always order 0 of one of the two passes.  The scan budget, the parallel search for
    the minimum index, the error-before-valid rule, the orientation flip and --all are therefore driven here through the
    diagnostics hook ambi_batch_debug_inject_validity: verdicts are injected, everything else (orders, breakpoints,
    paths) is the real thing and is compared with the oracle's --all output for the same order."""
    from ambigram_amd import synth
    s = synth.make_sample(48, 100, "wide", 9, seed=9100)
    lh, sols = s.write(workdir, "inj")
    of = oracle.run_bfb(lh, sols, all_=True, keep_orders=True)["chr"][0]
    orv = oracle.run_bfb(lh, sols, all_=True, reversed_=True)["chr"][0]
    R = of["num_orders"]
    orders = of["orders"]
    assert R == 70 and len(of["all_paths"]) == R and len(orv["all_paths"]) == R      # every order valid in both orientations
    E = -12    # AMBI_ERR_REF_UB

    def run(fwd, rev, flags=0, budget=4):
        g = api.Graph(lib, lh)
        b = api.Batch(lib)
        b.configure(first_budget=budget)
        b.add_chromosome_sol(g, 0, sols[0])
        b.debug_inject_validity(0, list(fwd) + list(rev))
        b.upload(); b.run(flags); b.download()
        return g, b, b.unit_result(0)

    zeros = [0] * R
    mid = R // 2
    cases = [
        # (forward verdicts, reversed verdicts, expected (status, first_valid, first_forward, evaluated))
        ("hit at 1 (inside the scan budget)", [0, 1] + [127] * (R - 2), zeros, (0, 1, 1, 2)),
        ("hit mid-table, later orders valid too", [0] * mid + [1] * (R - mid), zeros, (0, mid, 1, mid + 1)),
        ("hit at the last order", [0] * (R - 1) + [1], zeros, (0, R - 1, 1, R)),
        ("flip, hit at 3", zeros, [0, 0, 0, 1] + [1] * (R - 4), (0, 3, 0, R + 4)),
        ("flip, hit at the last order", zeros, [0] * (R - 1) + [1], (0, R - 1, 0, 2 * R)),
        ("no valid order", zeros, zeros, (api.ST_NO_VALID_ORDER, -1, -1, 2 * R)),
        ("valid at 5 before undefined at 10", [0] * 5 + [1] + [0] * 4 + [E] + [1] * (R - 11), zeros, (0, 5, 1, 6)),
        ("undefined at 5 before valid at 10", [0] * 5 + [E] + [0] * 4 + [1] * (R - 10), zeros, (E, -1, -1, 6)),
        ("undefined in the flipped pass before its first valid order", zeros, [0] * 20 + [E] + [0] * 9 + [1] * (R - 30), (E, -1, -1, R + 21)),
        ("valid and undefined in the same chunk, valid first", [0] * 33 + [1, E] + [0] * (R - 35), zeros, (0, 33, 1, 34)),
    ]
    for name, fwd, rev, want in cases:
        for budget in (4, 64, 1):
            g, b, r = run(fwd, rev, budget=budget)
            got = (r["status"], r["first_valid"], r["first_forward"], r["evaluated"])
            if want[0] < 0:
                assert got[0] == want[0] and got[3] == want[3], (name, budget, got, want)
            else:
                assert got == want, (name, budget, got, want)
            if want[0] == 0:      # the winner's path is the oracle's path of that very order and orientation
                ref = (of if want[2] == 1 else orv)["all_paths"][want[1]]
                assert b.unit_path(0, 0).tolist() == ref, (name, budget)
                # ... and, since every valid order of this unit gives that same path, the order it was made from: the row the
                # engine decoded is the oracle's order of that index (check_injected_validity_matrix: every row width)
                assert b.debug_unit_order(0).tolist() == orders[want[1]], (name, budget, b.debug_unit_order(0).tolist(), orders[want[1]])
            b.close(); g.close()
    # --all: bitmaps, counts, flip rule and `evaluated` with mixed verdicts
    import random
    rng = random.Random(5)
    for last_valid in (True, False):
        fwd = [rng.randint(0, 1) for _ in range(R)]
        rev = [rng.randint(0, 1) for _ in range(R)]
        fwd[0] = 1                       # the default-mode scan finds order 0 (the unit's ordinary results)
        fwd[-1] = 1 if last_valid else 0
        g, b, r = run(fwd, rev, flags=api.FLAG_ALL, budget=64)
        assert r["status"] == 0 and r["evaluated"] == (R if last_valid else 2 * R), (last_valid, r)
        i0 = b.all_orders(0, 0).tolist()
        i1 = b.all_orders(0, 1).tolist()
        assert i0 == [i for i in range(R) if fwd[i]], last_valid
        assert i1 == ([] if last_valid else [i for i in range(R) if rev[i]]), last_valid
        got = b.all_paths(0, 0, 0, len(i0), 4096)
        assert [p.tolist() for p in got] == [of["all_paths"][i] for i in i0]
        if i1:
            got = b.all_paths(0, 1, 0, len(i1), 4096)
            assert [p.tolist() for p in got] == [orv["all_paths"][i] for i in i1]
        b.close(); g.close()
    # --all with an undefined order: the unit is refused
    fwd = [1] * R
    fwd[40] = E
    g, b, r = run(fwd, [1] * R, flags=api.FLAG_ALL, budget=64)
    assert r["status"] == E, r
    b.close(); g.close()


def check_all_two_forms(lib, workdir, seeds=range(300, 420)):
    """--all evaluates an order with one THREAD (ambi_eval_lane.hpp, units with a short breakpoint path) or with one
    WAVEFRONT (ambi_eval.hpp): the same valid-order lists, counts, flip decisions and statuses from both, on random
    decompositions (most orders invalid, both orientations) and on wide synthetic samples (every order valid).  The lane
    form also with the unit's automaton staged in group memory (AMBI_ALL_AUTO_LDS bytes; a unit needs 16 nI + 4 (nI + 1) +
    2 nC + 16): 16384 holds every unit of this batch, 1024 the small ones only, the others are read through."""
    import os
    from ambigram_amd import synth
    items = []
    for seed in seeds:
        lh, sols = cases.random_decomposition(workdir, seed)
        items.append((lh, sols[0]))
    for i, (tier, K) in enumerate([("wide", 9), ("mixed", 9), ("wide", 13), ("chain", 7), ("mixed", 17), ("mixed", 19)]):
        s = synth.make_sample(64, 128, tier, K, seed=8800 + i, imperfect=i % 2)
        lh, sols = s.write(workdir, "tf%d" % i)
        items.append((lh, sols[0]))
    names = ("AMBI_ALL_LANES", "AMBI_ALL_AUTO_LDS")
    saved = {n: os.environ.get(n) for n in names}
    forms = {"1": ("1", None), "0": ("0", None), "staged all": ("1", "16384"), "staged small": ("1", "1024")}
    got = {}
    try:
        for form, values in forms.items():
            for n, v in zip(names, values):
                os.environ.pop(n, None)
                if v is not None:
                    os.environ[n] = v
            for rev in (0, api.FLAG_REVERSED):
                graphs, b = [], api.Batch(lib)
                for lh, sol in items:
                    g = api.Graph(lib, lh); graphs.append(g)
                    b.add_chromosome_sol(g, 0, sol)
                b.upload(); b.run(api.FLAG_ALL | rev); b.download()
                rec = []
                for u in range(len(items)):
                    r = b.unit_result(u)
                    rec.append((r["status"], r["evaluated"], b.all_orders(u, 0).tolist(), b.all_orders(u, 1).tolist()))
                got[(form, rev)] = rec
                b.close()
                for g in graphs:
                    g.close()
    finally:
        for n in names:
            os.environ.pop(n, None)
            if saved[n] is not None:
                os.environ[n] = saved[n]
    for rev in (0, api.FLAG_REVERSED):
        for form in forms:
            for u, (x, y) in enumerate(zip(got[("1", rev)], got[(form, rev)])):
                assert x == y, (form, rev, u, items[u][0], x[:2], y[:2])
    assert sum(1 for x in got[("1", 0)] if x[0] == 0 and len(x[2]) > 1) >= 2


def check_arena_limit(lib, workdir, n_units=40, budget=3, seeds=range(9300, 9340)):
    """The order-table arena has an upper limit (AMBI_ARENA_MAX_BYTES): the plan stage gives rows to the units that fit, in
    unit order, and the others end with ORDERS_CAPACITY (-15) -- whatever the scan for the first valid order, which may run
    BESIDE the plan stage, made of them.  Units that got their rows are exactly what they are without the limit; runs are
    repeatable; the same batch without the limit reconstructs every unit."""
    import os
    from ambigram_amd import synth
    items = []
    for i, seed in zip(range(n_units), seeds):
        s = synth.make_sample(48, 100, ("chain", "wide", "mixed")[i % 3], 9 + 2 * (i % 3), seed=seed, imperfect=i % 2, n_del=(i % 5 == 4) * 2, n_dup=(i % 7 == 6) * 1)
        lh, sols = s.write(workdir, "al%d_%d" % (n_units, i))
        items.append((lh, sols[0]))

    def run(cap):
        os.environ.pop("AMBI_ARENA_MAX_BYTES", None)
        if cap:
            os.environ["AMBI_ARENA_MAX_BYTES"] = str(cap)
        try:
            graphs, b = [], api.Batch(lib)
            b.configure(order_arena_bytes=4096, first_budget=budget)
            for lh, sol in items:
                g = api.Graph(lib, lh); graphs.append(g)
                b.add_chromosome_sol(g, 0, sol)
            b.upload()
            outs = []
            for flags in (0, 0, api.FLAG_REVERSED):
                b.run(flags); b.wait(); b.download()
                out = []
                for u in range(len(items)):
                    r = dict(b.unit_result(u))
                    if r["status"] == 0:
                        r["path"] = b.unit_path(u, 0).tolist(); r["path_indel"] = b.unit_path(u, 1).tolist(); r["out"] = b.unit_out_juncs(u)
                        r["orders"] = b.unit_orders(u, 0, min(r["num_orders"], 200), r["n_nodes"]).tolist()
                    out.append(r)
                outs.append(out)
            b.close()
            for g in graphs:
                g.close()
            return outs
        finally:
            os.environ.pop("AMBI_ARENA_MAX_BYTES", None)

    free = run(None)
    assert all(r["status"] != -15 for out in free for r in out)
    with_rows = [u for u, r in enumerate(free[0]) if r["status"] == 0 and r["num_orders"] > 0]
    assert len(with_rows) >= n_units // 2
    cap = 4096 * (len(with_rows) // 2)                      # every table of these small units is one 4 KB granule
    lim = run(cap)
    for u, (x, y) in enumerate(zip(lim[0], lim[1])):
        assert x == y, ("two runs of the limited batch differ", u, {k: (x.get(k), y.get(k)) for k in set(x) | set(y) if x.get(k) != y.get(k)})
    n_refused = 0
    for flags_i in (0, 2):
        refused = [u for u, r in enumerate(lim[flags_i]) if r["status"] == -15]
        wanted = [u for u, r in enumerate(free[flags_i]) if r["num_orders"] > 0 and free[flags_i][u]["status"] not in (1, 2)]
        assert refused and len(refused) < len(wanted), (cap, refused)
        assert refused == [u for u in wanted if u >= refused[0]], (refused, wanted)   # unit order: the tail of the units with rows
        for u, (x, y) in enumerate(zip(lim[flags_i], free[flags_i])):
            if u in refused:
                continue
            assert x == y, (flags_i, u, items[u][0])
        n_refused = len(refused)
    return n_refused


def check_large_batch_of_pending_units(lib, oracle, workdir, seeds=range(20000, 20600), budget=1, runs=2):
    """ONE batch of many random decompositions with a scan budget of one order: most of them have no valid order at all and
    more orders than the budget, so their scan ends PENDING and the parallel search resolves them -- while, in the same
    launch, the plan stage hands out rows beside the scan (they run on two streams and must not share a word: round 1 let
    the plan stage read the status the scan rewrites).  Every unit equals its own oracle run: status, counts, the order
    table, paths.  The batch is run twice (first run: arena sizing; second: the resident path)."""
    units = []
    for seed in seeds:
        lh, sols = cases.random_decomposition(workdir, seed)
        o = oracle.run_bfb(lh, sols, keep_orders=True)
        assert o["ok"], o["err"]
        oc = o["chr"][0]
        if oc["shortcut"]:
            continue
        units.append((seed, lh, sols[0], oc))
    graphs, b = [], api.Batch(lib)
    b.configure(first_budget=budget)
    for _, lh, sol, _ in units:
        g = api.Graph(lib, lh); graphs.append(g)
        b.add_chromosome_sol(g, 0, sol)
    b.upload()
    stats = dict(units=len(units), none_pending=0, valid=0, refused=0)
    for run in range(runs):
        b.run(0); b.wait(); b.download()
        for u, (seed, lh, sol, oc) in enumerate(units):
            r = b.unit_result(u)
            if oc["ub_valid"]:
                assert r["status"] == -12, (run, seed, r)
                stats["refused"] += run == 0
                continue
            assert r["num_orders"] == oc["num_orders"], (run, seed)
            if 0 < oc["num_orders"] <= 5000:
                assert b.unit_orders(u, 0, r["num_orders"], r["n_nodes"]).tolist() == oc["orders"], (run, seed)
            if oc["first_valid"] < 0:
                assert r["status"] == api.ST_NO_VALID_ORDER, (run, seed, r)
                assert r["evaluated"] == oc["evaluated"], (run, seed, r["evaluated"], oc["evaluated"])
                stats["none_pending"] += run == 0 and oc["num_orders"] > budget
            else:
                assert r["status"] == 0, (run, seed, r)
                assert (r["first_valid"], r["first_forward"], r["evaluated"]) == (oc["first_valid"], oc["first_forward"], oc["evaluated"]), (run, seed)
                assert b.unit_bkp(u).tolist() == oc["bkp"] and b.unit_path(u, 0).tolist() == oc["path"] and b.unit_path(u, 1).tolist() == oc["path_indel"], (run, seed)
                stats["valid"] += run == 0
    b.close()
    for g in graphs:
        g.close()
    assert stats["none_pending"] >= len(units) // 3, stats
    return stats


# ---------------------------------------------------------------------------------------------
# Which row of the order table the search, resolve and --all stages read (tests/test_search_rows.py)
# ---------------------------------------------------------------------------------------------
def order_row_bytes(K):
    """Bytes between two rows of a unit's order table, written out here and not taken from the engine: a unit of up to 63
    nodes stores an order as its Lehmer code, digit m - 1 (m nodes still free) in ceil(log2 m) bits, the code padded to whole
    dwords and never shorter than one; a wide unit (64..255 nodes) keeps a byte per node in rows of 128 or 256 bytes."""
    if K > 63:
        return 128 if K <= 127 else 256
    bits = sum((m - 1).bit_length() for m in range(1, K + 1))      # (m - 1).bit_length() == ceil(log2 m)
    return 4 * max(1, -(-bits // 32))


ROW_CLASSES = ("4", "8", "12-16", "20-40", "128", "256")
# the enumeration paths that write a fast-path unit's table (the switches of check_enumerate_variants), the reader of a
# table that is a copy of the first rows, and the table readers that are not the search: --all on a wide unit, the scan of a
# backend without pre-unranked first rows (host simulation only: the HIP backend always has them)
TABLE_VARIANTS = (("default", {}, 0), ("block_max_1", {"AMBI_BLOCK_MAX": "1"}, 0), ("block_lds_64", {"AMBI_BLOCK_LDS": "64"}, 0),
                  ("block_lds_12288", {"AMBI_BLOCK_LDS": "12288"}, 0), ("lanes_64", {}, 64), ("lanes_1M", {}, 1 << 20))


def row_class(K):
    w = order_row_bytes(K)
    return str(w) if w <= 8 or w >= 128 else ("12-16" if w <= 16 else "20-40")


# (tier, K, segments, junctions, seed, copy numbers of the planted loops, R, orientations whose --all paths the oracle is asked for)
# R as a plain oracle run reports it (asserted before --all is asked for): wide: C(K-1, (K-1)/2), skewN: C(K-1, N), skew = skew3.
# K <= 11 (one-dword rows): no tier reaches R > 256 there (wide 11 is the largest with 252); every other class has a unit above
# 256.  K = 19 is the bench unit (synth.config_sample(2)); its reversed --all is not asked for (cost), so it gets forward hits only.
# skew2 128 with copy number 1 throughout: the shortest paths the tier gives (the oracle's --all is R x path length).
SEARCH_ROW_UNITS = (
    ("wide", 9, 48, 100, 9100, (1, 2), 70, (1, 0)),
    ("wide", 11, 48, 100, 9111, (1, 2), 252, (1, 0)),
    ("skew", 12, 48, 100, 9112, (1, 2), 165, (1, 0)),
    ("wide", 19, 256, 512, 2000, (1, 2), 48620, (1,)),
    ("skew", 23, 64, 128, 9123, (1, 2), 1540, (1, 0)),
    ("skew", 25, 64, 128, 9125, (1, 2), 2024, (1, 0)),
    ("skew", 27, 64, 128, 9127, (1, 2), 2600, (1, 0)),
    ("skew", 34, 96, 200, 9134, (1, 2), 5456, (1, 0)),
    ("skew2", 45, 128, 256, 9145, (1, 2), 946, (1, 0)),
    ("skew2", 63, 70, 150, 9163, (1, 2), 1891, (1, 0)),
    ("skew2", 64, 70, 150, 9164, (1, 2), 1953, (1, 0)),
    ("skew1", 100, 110, 230, 9200, (1, 2), 99, (1, 0)),
    ("skew1", 127, 136, 280, 9227, (1, 2), 126, (1, 0)),
    ("skew2", 128, 132, 280, 9228, (1,), 8001, (1, 0)),
    ("skew1", 255, 264, 540, 9255, (1, 2), 254, (1, 0)),
)
FIRST_ROWS_UNIT = ("mixed", 12, 48, 100, 9112, (1, 2), 55, (1,))     # R <= 64: its table is a copy of the first rows (copy_first_rows)
E_REF_UB = -12
_ROW_UNIT_CACHE = {}


class RowUnit:
    """One unit of the matrix with what the oracle says about it: orders[f] (allTopologicalOrders) and, per orientation
    (1 forward, 0 reversed), the --all path of every order."""

    def __init__(self, oracle, workdir, spec):
        from ambigram_amd import synth
        tier, K, nseg, njunc, seed, cns, R, orients = spec
        self.spec, self.K, self.R, self.orients = spec, K, R, orients
        self.stride, self.cls, self.wide = order_row_bytes(K), row_class(K), K > 63
        s = synth.make_sample(nseg, njunc, tier, K, seed=seed, cn_choices=cns, name="sr_%s%d_%d" % (tier, K, seed))
        self.lh, sols = s.write(workdir)
        self.sol = sols[0]
        oc = oracle.run_bfb(self.lh, sols)["chr"][0]
        assert oc["num_orders"] == R and len(oc["node2pat"]) == K and not oc["ub_valid"], (spec, oc["num_orders"])      # before --all is asked for
        self.paths, self.orders = {}, None

    def all_calls(self):
        """the oracle's --all runs this unit needs: (orientation, arguments of run_bfb)"""
        return [(o, (self.lh, [self.sol]), dict(all_=True, reversed_=(o == 0), keep_orders=(o == self.orients[0]), dedup_all=True)) for o in self.orients]

    def take(self, o, out):
        oc = out["chr"][0]
        # precondition: every order is valid in this orientation, so any index can take a hit and has a reference path
        assert len(oc["all_paths"]) == self.R and oc["evaluated"] == self.R and not oc["ub_valid"], (self.spec, o, len(oc["all_paths"]))
        self.paths[o] = oc["all_paths"]
        if o == self.orients[0]:
            self.orders = oc["orders"]
            assert len(self.orders) == self.R and all(len(x) == self.K for x in self.orders[:3])

    def distinct_row(self, f):
        """precondition of the row comparison: row f is not row 0 and not a neighbour's (true of any table of distinct orders)"""
        for g in (0, f - 1, f + 1):
            if g != f and 0 <= g < self.R:
                assert self.orders[f] != self.orders[g], (self.spec, f, g)


def row_units(oracle, workdir, specs):
    """The oracle's records of the units.  Its --all runs are made side by side in freshly started worker processes (the oracle is
    one-threaded and not re-entrant; two units -- K = 19 with its 48 620 orders, skew2 128 -- cost as much as all the others
    together).  Returns (units, seconds of wall time this took)."""
    import multiprocessing
    import time
    from concurrent.futures import ProcessPoolExecutor
    t0 = time.time()
    todo = [RowUnit(oracle, workdir, s) for s in specs if s not in _ROW_UNIT_CACHE]
    calls = sorted(((U, o, a, kw) for U in todo for o, a, kw in U.all_calls()), key=lambda c: -c[0].R * c[0].spec[2])      # the costly ones first
    if calls:
        with ProcessPoolExecutor(max_workers=min(8, len(calls)), mp_context=multiprocessing.get_context("spawn")) as pool:
            futures = [(U, o, pool.submit(oracle.run_bfb, *a, **kw)) for U, o, a, kw in calls]
            for U, o, fut in futures:
                U.take(o, fut.result())
    for U in todo:
        _ROW_UNIT_CACHE[U.spec] = U
    return [_ROW_UNIT_CACHE[s] for s in specs], time.time() - t0


def search_row_cases(U):
    """The cases of one unit: (name, scan budget, run flags, {index: verdict} forward seed, the same reversed seed, want);
    anything not named has verdict 0.  want: ("hit", f, orientation) or ("err", status, evaluated)."""
    R, stride = U.R, U.stride
    out, seen = [], set()
    last_chunk = 16 * ((R - 1) // 16)                  # the search deals the orders out in chunks of 16
    kb = 4096 // stride                                # rows kb - 1 / kb (/ kb + 1 when a row straddles) around the first 4 KB of the table

    def hit(f, o, budget=4, flags=0, name=""):
        if not (0 <= f < R) or o not in U.orients or (f, o, budget, flags) in seen:
            return
        seen.add((f, o, budget, flags))
        U.distinct_row(f)
        mine = {f: 1}
        fwd, rev = (mine, {}) if o == 1 else ({}, mine)
        out.append(("%s f=%d o=%d" % (name, f, o), budget, flags, fwd, rev, ("hit", f, o)))

    for b in (1, 4, 64):                               # the seam between the first rows in group memory and the table
        for f in (b - 1, b, b + 1):
            hit(f, 1, b, name="seam of budget %d" % b)
    for f in (15, 16, 17, last_chunk, kb - 1, kb, kb + 1, R // 2, R - 1):
        hit(f, 1, name="table")
    for f in (3, 4, 5, 15, 16, 17, last_chunk, kb - 1, kb, kb + 1, R // 2, R - 1):       # the same in the flipped pass: evaluated == R + f + 1
        hit(f, 0, name="flipped pass")
    hit(R // 2, 0, flags=api.FLAG_REVERSED, name="--reversed, first pass")
    hit(min(5, R - 1), 1, flags=api.FLAG_REVERSED, name="--reversed, flipped pass")
    f = R // 2
    lo, hi = min(5, R - 2), R - 1
    if f // 16 != hi // 16:
        out.append(("two hits in different chunks", 4, 0, {f: 1, hi: 1}, {}, ("hit", f, 1)))
    if lo // 16 != last_chunk // 16 and lo != f:
        U.distinct_row(lo)
        out.append(("two hits, first and last chunk", 4, 0, {lo: 1, last_chunk: 1}, {}, ("hit", lo, 1)))
    if 4 < f - 1 and f + 1 < R:
        out.append(("undefined just before the hit", 4, 0, {f - 1: E_REF_UB, f: 1}, {}, ("err", E_REF_UB, f)))
        out.append(("undefined just after the hit", 4, 0, {f: 1, f + 1: E_REF_UB}, {}, ("hit", f, 1)))
    return out


def _row_verdicts(R, fwd, rev):
    v = [0] * (2 * R)
    for i, x in fwd.items():
        v[i] = x
    for i, x in rev.items():
        v[R + i] = x
    return v


def _row_check(b, u, U, case, tag, table_off, covered, variant):
    """One armed unit of a finished run against the oracle.  covered: (row class, variant) of every hit behind the scan budget
    whose decoded row was compared."""
    name, budget, flags, fwd, rev, want = case
    r = b.unit_result(u)
    got = (r["status"], r["first_valid"], r["first_forward"], r["evaluated"])
    where = "%s: unit %d K=%d R=%d row stride %d, table expected at byte %d of the arena (4 KB granules, unit order), case '%s', budget %d, flags %d, variant %s" % (
        tag, u, U.K, U.R, U.stride, table_off, name, budget, flags, variant)
    if want[0] == "err":
        assert (got[0], got[3]) == (want[1], want[2]), (where, got, want)
        return
    _, f, o = want
    first_o = 0 if flags & api.FLAG_REVERSED else 1
    expect = (0, f, o, (0 if o == first_o else U.R) + f + 1)
    row = b.debug_unit_order(u).tolist()
    if got != expect or row != U.orders[f]:
        is_row = U.orders.index(row) if row in U.orders else None
        raise AssertionError("%s\n  header (status, first_valid, first_forward, evaluated) got %s want %s\n  row got    %s (order %s of the table)\n  row wanted %s (order %d)"
                             % (where, got, expect, row, is_row, U.orders[f], f))
    assert b.unit_path(u, 0).tolist() == U.paths[o][f], where
    if f >= budget:
        covered.add((U.cls, variant))


def _row_batch(lib, units, cases, budget=4, flags=0, lanes=0):
    """ONE batch of `units`, unit i armed with cases[i] (None: not armed); returns (graphs, batch, byte offset of every table)."""
    graphs, b = [], api.Batch(lib)
    if lanes:
        b.configure(first_budget=budget, target_lanes=lanes)
    else:
        b.configure(first_budget=budget)
    offs, off = [], 0
    for i, (U, case) in enumerate(zip(units, cases)):
        g = api.Graph(lib, U.lh)
        graphs.append(g)
        b.add_chromosome_sol(g, 0, U.sol)
        if case is not None:
            b.debug_inject_validity(i, _row_verdicts(U.R, case[3], case[4]))
        offs.append(off)
        off += -(-(U.R * U.stride) // 4096) * 4096
    b.upload(); b.run(flags); b.download()
    return graphs, b, offs


def _row_close(graphs, b):
    b.close()
    for g in graphs:
        g.close()


class _Env:
    def __init__(self, env):
        self.env, self.saved = env, {}

    def __enter__(self):
        for k in ("AMBI_BLOCK_MAX", "AMBI_BLOCK_LDS", "AMBI_HOSTSIM_SEARCH_ORDER", "AMBI_HOSTSIM_TABLE_SCAN"):
            self.saved[k] = os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def check_injected_validity_matrix(lib, oracle, workdir, search_orders=(None,), table_scan=False):
    """WHICH row of the order table the device-side readers fetch, at every row width (see tests/test_search_rows.py).

    For a hit injected at index f the engine must publish status 0, first_valid f, the orientation, evaluated = pass * R + f + 1,
    the oracle's path of order f AND -- the observable that depends on the row, since every valid order of these units gives the
    same path -- the order it evaluated, byte for byte the oracle's orders[f] (ambi_batch_debug_unit_order).
    search_orders: values of AMBI_HOSTSIM_SEARCH_ORDER for the cases in which the order of the chunks matters (host simulation);
    table_scan: also the scan of a backend without first rows (AMBI_HOSTSIM_TABLE_SCAN, host simulation only).
    Returns (batches run, seconds of wall time spent in the oracle, covered (row class, variant) pairs)."""
    import random
    units, oracle_seconds = row_units(oracle, workdir, SEARCH_ROW_UNITS + (FIRST_ROWS_UNIT,))
    small = units.pop()
    assert [U.stride for U in units] == [4, 4, 8, 8, 12, 12, 16, 20, 28, 40, 128, 128, 128, 256, 256]     # the table of the issue, from order_row_bytes
    assert {U.cls for U in units} == set(ROW_CLASSES)
    for cls in ROW_CLASSES[1:]:
        assert any(U.R > 256 for U in units if U.cls == cls), cls
    assert all(U.R > 64 for U in units) and small.R <= 64
    covered, batches = set(), 0
    all_cases = [search_row_cases(U) for U in units]
    # (1) every unit alone
    for U, cases in zip(units, all_cases):
        for case in cases:
            orders = search_orders if (len(case[3]) + len(case[4]) > 1) else search_orders[:1]
            for so in orders:
                with _Env({"AMBI_HOSTSIM_SEARCH_ORDER": so} if so else {}):
                    graphs, b, offs = _row_batch(lib, [U], [case], budget=case[1], flags=case[2])
                    _row_check(b, 0, U, case, "alone (search order %s)" % so, offs[0], covered, "default")
                    _row_close(graphs, b)
                    batches += 1
    # (2) all of them in ONE batch, so that the tables start far from byte 0 of the arena and the neighbours have rows of
    # other widths; every unit with another case, through every enumeration path that writes the tables
    shared = [[c for c in cases if c[1] == 4 and c[2] == 0] for cases in all_cases]
    fast = [i for i, U in enumerate(units) if not U.wide]
    for vi, (variant, env, lanes) in enumerate(TABLE_VARIANTS):
        for rot in range(3):
            with _Env(env):
                picked = [sh[(7 * i + 5 * rot + 3 * vi) % len(sh)] for i, sh in enumerate(shared)]
                if rot == 2:        # a hit behind the budget for every unit: what the (class, variant) cover counts
                    picked = [next(c for c in sh if c[5][0] == "hit" and c[5][1] == U.R // 2) for U, sh in zip(units, shared)]
                graphs, b, offs = _row_batch(lib, units, picked, budget=4, lanes=lanes)
                assert offs[-1] > (1 << 20)
                for i, (U, case) in enumerate(zip(units, picked)):
                    _row_check(b, i, U, case, "one batch", offs[i], covered, variant)
                if rot == 2 and variant == "default":      # the resident batch once more: the same rows
                    b.run(0); b.download()
                    for i, (U, case) in enumerate(zip(units, picked)):
                        _row_check(b, i, U, case, "one batch, second run", offs[i], covered, variant)
                _row_close(graphs, b)
                batches += 1
    for i in fast:
        for variant, _, _ in TABLE_VARIANTS:
            assert (units[i].cls, variant) in covered, (units[i].cls, variant)
    # (3) --all on the wide units (the only --all form that reads the table): bitmaps and counts with seeded random verdicts as
    # in check_injected_validity, the decoded row of one requested order per run, and the row behind a request for ONE path
    rng = random.Random(11)
    for U in [U for U in units if U.wide]:
        R = U.R
        for last_valid, q in ((True, 1), (False, R // 2), (True, R - 1)):
            U.distinct_row(q)
            fwd = [rng.randint(0, 1) for _ in range(R)]
            rev = [rng.randint(0, 1) for _ in range(R)]
            fwd[0] = 1
            fwd[-1] = 1 if last_valid else 0
            marked = list(fwd)
            marked[q] += 64                                 # kInjectRecord: the same verdict, and "leave the row you decoded for this order"
            graphs, b = [api.Graph(lib, U.lh)], api.Batch(lib)
            b.configure(first_budget=64)
            b.add_chromosome_sol(graphs[0], 0, U.sol)
            b.debug_inject_validity(0, marked + rev)
            b.upload(); b.run(api.FLAG_ALL); b.download()
            batches += 1
            r = b.unit_result(0)
            tag = (U.spec, last_valid, q)
            assert r["status"] == 0 and r["evaluated"] == (R if last_valid else 2 * R), (tag, r)
            i0, i1 = b.all_orders(0, 0).tolist(), b.all_orders(0, 1).tolist()
            assert i0 == [i for i in range(R) if fwd[i]] and i1 == ([] if last_valid else [i for i in range(R) if rev[i]]), tag
            assert b.debug_unit_order(0).tolist() == U.orders[q], (tag, "row of the requested order", b.debug_unit_order(0).tolist(), U.orders[q])
            cap = max(len(U.paths[1][0]), len(U.paths[0][0])) + 8
            for ps, idx, o in ((0, i0, 1), (1, i1, 0)):
                for j in sorted({0, len(idx) // 2, len(idx) - 1} if idx else ()):
                    got = b.all_paths(0, ps, j, 1, cap)
                    assert [p.tolist() for p in got] == [U.paths[o][idx[j]]], (tag, ps, j)
                    U.distinct_row(idx[j])
                    assert b.debug_unit_order(0).tolist() == U.orders[idx[j]], (tag, "row behind the single path", ps, j, idx[j])
            covered.add((U.cls, "all_wide"))
            _row_close(graphs, b)
    # (4) a table that is a copy of the first rows (R <= budget): the scan never leaves the first rows, the reader of this table is
    # the path of a listed order (--all); and the same reader on an ordinary table
    for U, budget, variant in ((small, 64, "copy_first_rows"), (units[7], 64, "default")):
        R = U.R
        fwd = [rng.randint(0, 1) for _ in range(R)]
        fwd[0] = fwd[-1] = 1
        graphs, b = [api.Graph(lib, U.lh)], api.Batch(lib)
        b.configure(first_budget=budget)
        b.add_chromosome_sol(graphs[0], 0, U.sol)
        b.debug_inject_validity(0, fwd + [0] * R)
        b.upload(); b.run(api.FLAG_ALL); b.download()
        batches += 1
        i0 = b.all_orders(0, 0).tolist()
        assert i0 == [i for i in range(R) if fwd[i]] and b.unit_result(0)["evaluated"] == R, U.spec
        cap = len(U.paths[1][0]) + 8
        for j in sorted({1, len(i0) // 2, len(i0) - 1}):
            got = b.all_paths(0, 0, j, 1, cap)
            assert [p.tolist() for p in got] == [U.paths[1][i0[j]]], (U.spec, j)
            U.distinct_row(i0[j])
            assert b.debug_unit_order(0).tolist() == U.orders[i0[j]], (U.spec, "row behind the single path", j, i0[j], b.debug_unit_order(0).tolist())
        covered.add((U.cls, variant + "/single_path"))
        _row_close(graphs, b)
    # (5) the scan of a backend that has no pre-unranked first rows reads the table itself (stage_first's other source)
    if table_scan:
        for U in (units[3], units[7]):          # K = 19 and K = 34
            for f in (1, 37, 63):
                case = ("scan without first rows f=%d" % f, 64, 0, {f: 1}, {}, ("hit", f, 1))
                U.distinct_row(f)
                with _Env({"AMBI_HOSTSIM_TABLE_SCAN": "1"}):
                    graphs, b, offs = _row_batch(lib, [U], [case], budget=64)
                    _row_check(b, 0, U, case, "table scan", offs[0], set(), "table_scan")
                    covered.add((U.cls, "table_scan"))
                    _row_close(graphs, b)
                    batches += 1
    # what was compared with orders[f] behind the scan budget: every row class, through every table path
    assert {c for c, _ in covered} >= set(ROW_CLASSES), covered
    want_variants = {v for v, _, _ in TABLE_VARIANTS} | {"all_wide", "copy_first_rows/single_path", "default/single_path"} | ({"table_scan"} if table_scan else set())
    assert {v for _, v in covered} >= want_variants, covered
    return batches, oracle_seconds, covered
