"""Random element sets, lattices that are no products of chains, and the capacities of the wide front (units with 64..255 DAG
nodes, csrc/ambi_wide.hpp), against the CPU oracle and the plain-Python reference of order_checks (tests/wide_checks.py has the
generators, the classification by the reference and the checks).

The CPU half runs the host simulation, where construct_dag_wide, lattice_wide and write_wide_row run with one thread.  The GPU
half runs the same units through libambigram_hip.so -- the only place where the key ranking, the atomic ORs on pred / succ and
the sync pairs of the sequential loop phase run on 64 lanes --, against the oracle / the reference and unit by unit against the
host simulation's records.  profiles/r18_notes.md has the figures.

The floors are facts of the generators and of the reference (measured once, with the seeds as they stand): a change that empties
a class of inputs fails here and not silently.
"""
import os
import subprocess
import time

import pytest

import engine_checks as ec
import order_checks as oc
import parity
import prepare_checks as pc
import wide_checks as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# family 1, as the seeds of wide_checks give them (every floor is at least 1)
DAG_FLOORS = dict(loops_over_16=144, loops_over_64=95, mixed=96)
DAG_PER_K = 16
# family 2 (a): the least the family has to hold (the seeds give more: profiles/r18_notes.md)
BACKBONE_FLOORS = dict(table=12, table_K128=4, table_width3=6, table_pattern=6, count=3, ideals=3, cycle=3, table_small=12, not_a_product=12)
ASSEMBLED_FLOOR = 3
# the table variants that change anything for a wide unit: its own table kernel takes no switch, and a row is one thread's
# whatever the rows per lane are; target_lanes changes the plan's work blocks of the batch the wide units lie in
WIDE_VARIANTS = tuple(v for v in ec.TABLE_VARIANTS if v[0] in ("default", "lanes_64", "lanes_1M"))


def _floors(c, floors):
    assert all(v >= 1 for v in floors.values())
    short = {k: (c[k], v) for k, v in floors.items() if c[k] < v}
    assert not short, ("coverage below its floor (have, floor)", short, c)


def check_dag(oracle, units, recs):
    c = wc.check_dag_family(oracle, units, recs)
    print("wide DAG family:", c)
    _floors(c, DAG_FLOORS)
    assert set(c["per_K"]) == set(wc.DAG_K) and min(c["per_K"].values()) >= DAG_PER_K, c
    assert c["cross"] == [0, 10, 100, 1000], c
    return c


def _tables(oracle, workdir):
    return [u for u in wc.backbone_units(oracle, workdir)[0] if u["expect"] == "table"]


def _check_alone(lib, units):
    bad = {}
    for u in units:
        bad.update(oc.run_and_check(lib, [u]))
    oc.assert_clean(bad, "units alone")


def _check_behind_the_table(lib, oracle, workdir):
    """Whole runs of the small table units in both orientations: the parallel search over 128- and 256-byte rows and eval_order on
    WideDag.  Either verdict is a comparison; a unit on which the reference's own behaviour is undefined is refused at the same
    evaluation (test_wide_units._check_unit)."""
    from test_wide_units import _check_unit
    small = [u for u in _tables(oracle, workdir) if u["R"] <= wc.SMALL_R]
    assembled, seen = set(), {}
    for u in small:
        for rev in (False, True):
            o = oracle.run_bfb(u["lh"], [u["sol"]], reversed_=rev, keep_orders=False)["chr"][0]
            if o["ub_valid"]:
                what = _check_unit(lib, oracle, u["lh"], [u["sol"]], rev, orders=False)
                assert what == "refused", u["name"]
            elif o["first_valid"] < 0:          # every order evaluated, none assembles: the verdicts of all R rows, as check_mixed_batch takes them
                what = "none"
                d = wc.whole_run_without_path(lib, u, rev, o)
                assert d == [], (u["name"], rev, d)
            else:
                what = "path"
                assert parity.compare(lib, oracle, u["lh"], [u["sol"]], reversed_=rev, keep_orders=True) == [], (u["name"], rev)
                assembled.add(u["name"])
            seen[what] = seen.get(what, 0) + 1
    print("behind the table: %d units, runs %s, units that assemble a path: %d" % (len(small), seen, len(assembled)))
    assert len(assembled) >= ASSEMBLED_FLOOR, (seen, sorted(assembled))


def _check_ideal_caps(lib, oracle, workdir):
    units = wc.cap_units(oracle, workdir, "ideals")
    by = {u["name"]: u for u in units}
    assert 2049 <= by["wc_3050"]["ideals"] <= 4095 and by["wc_4096a"]["links"] == 16320      # (the most links of a chain with free loops)
    oc.assert_clean(oc.run_and_check(lib, units), "ideal cap, one batch")
    _check_alone(lib, units)


def _check_row_cap(lib, oracle, workdir, which):
    for u in wc.cap_units(oracle, workdir, which):
        t = time.time()
        oc.assert_clean(oc.run_and_check(lib, [u], arena_cap=wc.CAP_ARENA), "row cap: " + u["name"])
        print("row cap: %s, %d rows, %.1f s" % (u["name"], u["R"], time.time() - t))


# ---------------------------------------------------------------------------------------------
# CPU half
# ---------------------------------------------------------------------------------------------
def test_lattice_facts_on_known_posets():
    """The walk with a limit against closed forms and against Poset: a product of chains, an antichain past the limit, a cycle
    (the full set is never reached), the vee and the diamonds of the capacity units."""
    chain_and_free = [1 << (i + 1) if i < 4 else 0 for i in range(5)] + [0, 0]               # 0 -> 1 -> 2 -> 3 -> 4, 5, 6
    assert wc.lattice_facts(chain_and_free) == (6 * 4, 5 * 4 + 6 * 4) and oc.Poset(chain_and_free).shape() == (24, 3)
    assert wc.lattice_facts([0] * 12) == (4096, 12 * 2048) and wc.lattice_facts([0] * 13) is None and wc.lattice_facts([0] * 5, limit=31) is None
    assert wc.lattice_facts([0b10, 0b01, 0]) == (2, 1)                                       # 0 <-> 1: only node 2 is ever free
    vee = [0b110, 0, 0]
    assert wc.lattice_facts(vee) == (1 + 2 * 2, 1 + 2 + 1 + 1) and oc.Poset(vee).count() == 2


def test_backbone_coverage(oracle, workdir):
    units, facts = wc.backbone_units(oracle, workdir)
    c = wc.backbone_coverage(units)
    print("wide lattice family:", c, facts)
    _floors(c, BACKBONE_FLOORS)
    assert all(u["K"] >= 64 for u in units) and len({u["name"] for u in units}) == len(units)
    assert c["table_bytes"] <= oc.ARENA_CAP // 2 and c["max_links"] < wc.WIDE_LINK_CAP, c
    assert facts["dropped"]["rows"] < facts["seeds"] // 4, facts
    # share 0.7 of 60..250 elements: every pattern leaves a node without a record, each of them free -- more ideals than a wide unit holds
    assert all(u["expect"] == "ideals" for u in units if u["share"] == 0.7)


def test_dag_family_on_the_host_simulation(hostsim_lib, oracle, workdir):
    units = wc.dag_units(workdir)
    check_dag(oracle, units, wc.run_dag_family(hostsim_lib, workdir))


def test_backbone_units_alone_on_the_host_simulation(hostsim_lib, oracle, workdir):
    _check_alone(hostsim_lib, wc.backbone_units(oracle, workdir)[0])


def test_backbone_units_in_one_batch_on_the_host_simulation(hostsim_lib, oracle, workdir):
    units = wc.backbone_units(oracle, workdir)[0]
    oc.assert_clean(oc.run_and_check(hostsim_lib, units), "one batch")


def test_wide_and_ordinary_tables_in_one_batch_on_the_host_simulation(hostsim_lib, oracle, workdir):
    mixed = wc.mixed_batch(oracle, workdir, _tables(oracle, workdir))
    assert len({u["stride"] for u in mixed}) >= 5
    oc.assert_clean(oc.run_and_check(hostsim_lib, mixed), "wide and ordinary tables in one batch")


def test_behind_the_table_on_the_host_simulation(hostsim_lib, oracle, workdir):
    _check_behind_the_table(hostsim_lib, oracle, workdir)


def test_ideal_cap_on_the_host_simulation(hostsim_lib, oracle, workdir):
    _check_ideal_caps(hostsim_lib, oracle, workdir)


def test_row_cap_on_the_host_simulation(hostsim_lib, oracle, workdir):
    """Refused with the exact count one step past 2^20 rows; written at exactly 2^20 rows (diamonds) and at 1.3e5 rows.  The two
    tables just below the cap (1 030 200 and 1 028 790 rows) are the GPU half's."""
    _check_row_cap(hostsim_lib, oracle, workdir, "refused")
    _check_row_cap(hostsim_lib, oracle, workdir, "exact")
    _check_row_cap(hostsim_lib, oracle, workdir, "mid")


def test_generators_are_deterministic(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for make in (lambda w, s: pc.element_case(w, s, ns=wc.DAG_N, ks=wc.DAG_K, prefix="wd"), wc.backbone_unit):
        for s in (0, 7, 33, 95):
            x, y = make(a, s), make(b, s)
            assert open(x["lh"]).read() == open(y["lh"]).read() and open(x["sol"]).read() == open(y["sol"]).read(), s


def test_stage_check_under_asan_ubsan(tmp_path):
    """tests/tools/wide_stage_check.cpp: construct_dag_wide, lattice_wide, unrank_wide and write_wide_row on the host group over
    random element sets and the capacity units, WideUnit and the rows in heap blocks of exactly their size, as a stand-alone
    program under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "wide_stage_check")
    src = os.path.join(ROOT, "tests", "tools", "wide_stage_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-Wall", "-Wno-sign-compare", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "ambigram_amd", "csrc"),
                        "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and "wide_stage_check: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------
# GPU half
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dag_family_on_the_gpu(hip_lib, hostsim_lib, oracle, workdir):
    units = wc.dag_units(workdir)
    hip = wc.run_dag_family(hip_lib, workdir)
    wc.same_records(units, hip, wc.run_dag_family(hostsim_lib, workdir))       # first: it names the diverging unit even where the oracle is not asked
    check_dag(oracle, units, hip)


@pytest.mark.gpu
def test_backbone_units_alone_on_the_gpu(hip_lib, oracle, workdir):
    _check_alone(hip_lib, wc.backbone_units(oracle, workdir)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", WIDE_VARIANTS, ids=[v[0] for v in WIDE_VARIANTS])
def test_backbone_units_in_one_batch_on_the_gpu(hip_lib, hostsim_lib, oracle, workdir, variant):
    units = wc.backbone_units(oracle, workdir)[0]
    oc.assert_clean(oc.run_and_check(hip_lib, units, variant), variant[0])
    oc.assert_clean(oc.run_and_check(hip_lib, wc.mixed_batch(oracle, workdir, _tables(oracle, workdir)), variant), "mixed batch, " + variant[0])
    if variant[0] == "default":
        wc.same_records(units, wc.records(hip_lib, units), wc.records(hostsim_lib, units))


@pytest.mark.gpu
def test_behind_the_table_on_the_gpu(hip_lib, oracle, workdir):
    _check_behind_the_table(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_ideal_cap_on_the_gpu(hip_lib, hostsim_lib, oracle, workdir):
    _check_ideal_caps(hip_lib, oracle, workdir)
    units = wc.cap_units(oracle, workdir, "ideals")
    wc.same_records(units, wc.records(hip_lib, units), wc.records(hostsim_lib, units))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("refused", "exact", "mid", "written"))
def test_row_cap_on_the_gpu(hip_lib, oracle, workdir, which):
    """written: 1 030 200 and 1 028 790 rows of 128 bytes, every window of order_checks.windows and the permutation / strictly
    increasing invariant over the whole table."""
    _check_row_cap(hip_lib, oracle, workdir, which)
