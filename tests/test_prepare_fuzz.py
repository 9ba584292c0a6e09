"""Random junction sets and random element sets through the prepare stage, bit for bit against the CPU oracle
(tests/prepare_checks.py has the generators, the hand-built units and the checks).

The CPU half runs the host simulation (one thread: none of the wavefront forms).  The GPU half runs the same units through
libambigram_hip.so -- the only place where the `G::kLaneArrays` branches of csrc/ambi_prepare.hpp and csrc/ambi_sort.hpp run
-- as one batch per family through the ordinary kernel chain, in slices of 32 through the express kernel (the prepare on two
wavefronts, the lattice kernel's own second DAG beside it), and unit by unit against the host simulation's arrays.

The floors of the coverage counters are what the seeds of prepare_checks give (measured on the host simulation, where the
generators and the counters are the same code; profiles/r12_notes.md has the figures): a change of a generator that empties
a class of inputs fails here and not silently.
"""
import pytest

import prepare_checks as pc

# measured on the host simulation with JUNCTION_SEEDS / ELEMENT_SEEDS as they stand; every floor is at least 1
JUNCTION_FLOORS = dict(slots3=65, slots3_sensitive=65, nfb_over_64=35, chained=80, far_links=28, nsv_over_64=32, shortcut_replay=4,
                       tiny_no_shortcut=11, fractional_sums=155, bias_over_1=137)
ELEMENT_FLOORS = dict(loops_over_16=64, mixed_over_16=64, K_over_16=128, counts_compared=57, tables_compared=42)


def _floors(c, floors):
    assert all(v >= 1 for v in floors.values())
    short = {k: (c[k], v) for k, v in floors.items() if c[k] < v}
    assert not short, ("coverage below its floor (have, floor)", short, c)


def check_junctions(oracle, units, recs):
    c = pc.check_junction_family(oracle, units, recs)
    print("junction family:", c)
    _floors(c, JUNCTION_FLOORS)
    assert c["nfb_63_64_65"] == [63, 64, 65], c
    return c


def check_elements(oracle, units, recs):
    c = pc.check_element_family(oracle, units, recs)
    print("element family:", c)
    _floors(c, ELEMENT_FLOORS)
    assert c["cross"] == [0, 10, 100, 1000], c
    return c


# ---------------------------------------------------------------------------------------------
# CPU half
# ---------------------------------------------------------------------------------------------
def test_junction_family_on_the_host_simulation(hostsim_lib, oracle, workdir):
    units = pc.junction_units(workdir)
    check_junctions(oracle, units, pc.run_junction_family(hostsim_lib, workdir))


def test_element_family_on_the_host_simulation(hostsim_lib, oracle, workdir):
    units = pc.element_units(workdir)
    check_elements(oracle, units, pc.run_element_family(hostsim_lib, workdir))


def test_generators_are_deterministic(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for make, seeds in ((pc.junction_case, (0, 7, 33)), (pc.element_case, (0, 5, 199))):
        for s in seeds:
            x, y = make(a, s), make(b, s)
            assert open(x["lh"]).read() == open(y["lh"]).read() and open(x["sol"]).read() == open(y["sol"]).read(), (make.__name__, s)
    assert [u["juncs"] for u in pc.shared_slot_units()] == [u["juncs"] for u in pc.shared_slot_units()]


def test_oracle_dag_only_is_the_front_of_a_full_run(oracle, workdir):
    """dag_only stops behind allTopologicalOrders: the DAG, the count, the orders and targetCN of a full run, and no path."""
    import cases
    for seed in (3, 11, 40):
        lh, sols = cases.random_decomposition(workdir, 31000 + seed)
        full = oracle.run_bfb(lh, sols, keep_orders=True)
        front = oracle.run_bfb(lh, sols, keep_orders=True, dag_only=True)
        assert full["ok"] and front["ok"]
        assert front["target_cn"] == full["target_cn"]
        for f, g in zip(front["chr"], full["chr"]):
            for k in ("start", "end", "bias", "shortcut", "infeasible", "junc_cn", "inv_seg", "inv_junc", "seg_cn", "node2pat", "node2loop", "adj",
                      "num_orders", "orders"):
                assert f[k] == g[k], (seed, k)
            if not f["shortcut"]:
                assert f["path"] == [] and f["evaluated"] == 0, seed
        capped = oracle.run_bfb(lh, sols, keep_orders=True, dag_only=True, max_orders=2)
        for f, g in zip(capped["chr"], full["chr"]):
            assert f["orders"] == g["orders"][:2], seed


# ---------------------------------------------------------------------------------------------
# GPU half
# ---------------------------------------------------------------------------------------------
def _three_way(units, hip, host):
    bad = {}
    for u, x, y in zip(units, hip, host):
        d = pc.same_record(x, y)
        if d:
            bad[u["name"]] = d
    assert not bad, ("HIP differs from the host simulation", len(bad), dict(list(bad.items())[:8]))


def _express_slices(lib, units, chain, run):
    """Slices of at most 32 units through the express path (second run of a small batch); the same answers as the ordinary chain
    gave for the whole batch."""
    bad = {}
    for lo in range(0, len(units), 32):
        part = units[lo:lo + 32]
        recs = run(lib, None, express=True, units=part)
        for u, x, y in zip(part, recs, chain[lo:lo + 32]):
            d = pc.same_record(x, y, arena_independent_only=True)
            if d:
                bad[u["name"]] = d
    assert not bad, ("express path differs from the kernel chain", len(bad), dict(list(bad.items())[:8]))


@pytest.mark.gpu
def test_junction_family_on_the_gpu(hip_lib, hostsim_lib, oracle, workdir):
    units = pc.junction_units(workdir)
    chain = pc.run_junction_family(hip_lib, workdir)
    check_junctions(oracle, units, chain)
    _three_way(units, chain, pc.run_junction_family(hostsim_lib, workdir))
    _express_slices(hip_lib, units, chain, pc.run_junction_family)


@pytest.mark.gpu
def test_element_family_on_the_gpu(hip_lib, hostsim_lib, oracle, workdir):
    units = pc.element_units(workdir)
    chain = pc.run_element_family(hip_lib, workdir)
    host = pc.run_element_family(hostsim_lib, workdir)
    _three_way(units, chain, host)          # first: it names the diverging form even for the units the oracle is not asked about
    check_elements(oracle, units, chain)
    _express_slices(hip_lib, units, chain, pc.run_element_family)
