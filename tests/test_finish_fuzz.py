"""Planted and random SV sets through the finish stages, bit for bit against the CPU oracle (tests/finish_checks.py has the
generators, the plain walk of indelBFB that counts the coverage, and the checks).

The CPU half runs every family on the host simulation, indelBFB on the cells (AMBI_HOSTSIM_EDIT=0) and on the runs (=1).  The GPU
half runs the same units through libambigram_hip.so -- the only place where a sweep takes a second stride, a chain link lies a
block width ahead, tables_from_runs_pass<1..3> and the wave-specialised branches of the lean and the edit stage run -- as one
batch per family against the oracle and unit by unit against the host simulation, over every route a unit can take to a finish
stage (ROUTES), and in slices of 32 through the express kernel.

The floors of the coverage counters are what the plain walk gives on the committed seeds (measured on the CPU, on the reference
side: the oracle's path and the unit's junction list; profiles/r14_notes.md has them beside the seeds): a change of a generator
that empties a class of inputs fails here and not silently.
"""
import os
import subprocess

import pytest

import finish_checks as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# measured with the seeds of finish_checks as they stand; no floor is zero
FLOORS = dict(applied_deletion=290, applied_duplication=362, applied_inversion=255, applied_insertion=828,
              second_deletion=4, second_duplication=13, second_inversion=2, second_insertion=13,
              noop_deletion=548, noop_duplication=11, noop_inversion=39849, noop_insertion=23,
              deletion_at_3=134, deletion_exit_at_4=110, inversion_at_5=106, inversion_exit_at_6=23,
              erase_empty_insertion=198,
              arm_front_a_tgt=346, arm_front_b_tgt=325, arm_back_a_src=322, arm_back_b_src=306,
              group_3=530, group_4=216, group_5_up=105,
              find_after_with_earlier=815, noop_end_absent=112, dup_target_only_behind=7,
              units=486, units_over_capacity=2, units_over_steps=1, units_edited=458, units_two_edits=393, units_sv_over_256=56, units_sv_over_512=28, units_sv_over_1024=14,
              link_256_ahead=5, link_1024_ahead=1, runs_over_256=1)
# erase_empty_two (a two-vertex group whose ends are neighbours in the path) has no floor: the cells u, v can only be neighbours
# through an edit that applied the junction u -> v itself, and both readers drop a second copy of a junction -- it cannot be reached
# through a .lh (tests/tools/finish_stage_check.cpp reaches it: its junction lists are not read from a file).

FAMILY_NAMES = tuple(fc.FAMILIES)


def all_units(oracle, workdir):
    return [(f, fc.family_units(oracle, workdir, f)) for f in FAMILY_NAMES]


# ---------------------------------------------------------------------------------------------
# CPU half
# ---------------------------------------------------------------------------------------------
def test_coverage_of_the_families(oracle, workdir):
    """The plain walk gives the oracle's path_indel and output junctions on every unit, and every branch it counts is reached at
    least as often as on the committed seeds."""
    c = fc.coverage([u for _, units in all_units(oracle, workdir) for u in units])
    print("finish families:", c)
    assert all(v >= 1 for v in FLOORS.values())
    short = {k: (c[k], v) for k, v in FLOORS.items() if c[k] < v}
    assert not short, ("coverage below its floor (have, floor)", short)
    assert c["n_classes"] == list(fc.N_CLASSES) and c["np_classes"] == list(fc.NP_CLASSES), c
    assert c["run_classes"] == list(fc.RUN_CLASSES) + [257], c        # (257: more than 256 runs)
    over = sorted(u["name"] for _, units in all_units(oracle, workdir) for u in units if "over_capacity" in u)
    assert over == ["fcap", "fi16"], over      # the units whose edits outgrow the documented path capacity (the reference has none)
    over = sorted(u["name"] for _, units in all_units(oracle, workdir) for u in units if "over_steps" in u)
    assert over == ["fsteps"], over            # ... and the one whose duplication repeats more junction steps than a unit has room for
    svs = sorted(len(u["svs"]) for u in fc.family_units(oracle, workdir, "sv_counts"))
    assert svs == sorted(n for n in fc.SV_COUNTS for _ in fc.SV_WHERE), svs
    lean = fc.family_units(oracle, workdir, "lean")
    assert all(not u["same_strand"] and u["oc"]["path_indel"] != u["oc"]["path"] for u in lean)      # opposite-strand SVs only, and they edit


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_family_on_the_host_simulation(hostsim_lib, oracle, workdir, family):
    units = fc.family_units(oracle, workdir, family)
    cells = fc.run_units(hostsim_lib, units, env={"AMBI_HOSTSIM_EDIT": 0})
    fc.check_against_oracle(units, cells, "indelBFB on the cells")
    runs = fc.run_units(hostsim_lib, units, env={"AMBI_HOSTSIM_EDIT": 1})
    fc.check_against_oracle(units, runs, "indelBFB on the runs")


def test_host_simulation_serves_runs_that_outgrow_their_slots(hostsim_lib, oracle, workdir):
    """Run slots of 8 runs per unit (AMBI_RUN_SLOTS): the batch comes through the backend's pack_runs, as on the GPU."""
    for family in ("chains", "out_juncs"):
        units = fc.family_units(oracle, workdir, family)
        assert any(fc.n_runs(u["oc"]["path_indel"]) > 8 for u in units)
        fc.check_against_oracle(units, fc.run_units(hostsim_lib, units, env={"AMBI_RUN_SLOTS": 8}), "run slots of 8")


def test_generators_are_deterministic(oracle, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for make in (fc._family_lean, fc._family_capacity, fc._family_out_juncs):
        for x, y in zip(make(oracle, a), make(oracle, b)):
            assert open(x["lh"]).read() == open(y["lh"]).read() and open(x["sol"]).read() == open(y["sol"]).read(), x["name"]


def test_stage_check_under_asan_ubsan(tmp_path):
    """tests/tools/finish_stage_check.cpp: the finish-stage functions on the host group over random paths and junction lists, every
    buffer of exactly its stated size, as a stand-alone program under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "finish_stage_check")
    src = os.path.join(ROOT, "tests", "tools", "finish_stage_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-Wall", "-Wno-sign-compare", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "ambigram_amd", "csrc"),
                        "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and "finish_stage_check: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------
# GPU half
# ---------------------------------------------------------------------------------------------
ROUTES = (("default", {}),
          ("direct_edit_0", {"AMBI_DIRECT_EDIT": 0}),              # the direct launch as the full stage with the cells in device memory
          ("direct_full_0", {"AMBI_DIRECT_FULL": 0}),              # every unit through the lean stage first: ST_REFINISH and the list kernel
          ("direct_ext_0", {"AMBI_DIRECT_EXT": 0}),                # the full stage with the cells in group memory
          ("full_threads_256", {"AMBI_FULL_THREADS": 256}),
          ("full_threads_1024", {"AMBI_FULL_THREADS": 1024}),
          ("edit_run_cap_24", {"AMBI_EDIT_RUN_CAP": 24}),          # the edit kernel hands most units to ambi_finish_ext_kernel
          ("run_slots_8", {"AMBI_RUN_SLOTS": 8}))                  # runs that outgrow their slots: the pack kernels
_HOST = {}


def _host_records(hostsim_lib, family, units):
    """The host simulation's records of a family, computed once for all routes (the routes differ in how the GPU gets to a stage, not
    in what the stage computes)."""
    if family not in _HOST:
        _HOST[family] = fc.run_units(hostsim_lib, units)
    return _HOST[family]


def _against_host(units, hip, host, tag):
    """Unit by unit: everything the two libraries publish about a reconstructed unit.  (The unit over its path capacity ends with the
    same status in both; how far its edits got before the capacity stopped them is not a result.)"""
    keep = [i for i, u in enumerate(units) if "over_capacity" not in u and "over_steps" not in u]
    fc.same_records([units[i] for i in keep], [hip[i] for i in keep], [host[i] for i in keep], tag)
    for i, u in enumerate(units):
        if "over_capacity" in u or "over_steps" in u:
            want = fc.ST_ERR_PATH_CAPACITY if "over_capacity" in u else fc.ST_ERR_OUTJUNC_CAPACITY
            assert hip[i]["status"] == host[i]["status"] == want, (tag, u["name"], hip[i]["status"], host[i]["status"])


@pytest.mark.gpu
@pytest.mark.parametrize("route", [r[0] for r in ROUTES])
def test_families_on_the_gpu(hip_lib, hostsim_lib, oracle, workdir, route):
    env = dict(ROUTES)[route]
    for family, units in all_units(oracle, workdir):
        recs = fc.run_units(hip_lib, units, env=env)
        fc.check_against_oracle(units, recs, "%s, route %s" % (family, route))
        _against_host(units, recs, _host_records(hostsim_lib, family, units), "%s, route %s: HIP differs from the host simulation" % (family, route))


@pytest.mark.gpu
def test_families_through_the_express_kernel(hip_lib, oracle, workdir):
    """Slices of at most 32 units, run twice: the second run of a small batch takes the express kernel."""
    for family, units in all_units(oracle, workdir):
        for lo in range(0, len(units), 32):
            part = units[lo:lo + 32]
            fc.check_against_oracle(part, fc.run_units(hip_lib, part, express=True), "%s, express slice at %d" % (family, lo))
