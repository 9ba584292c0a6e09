"""High copy numbers and random fold-back maps through the per-order evaluation (placement + imperfectFBI), bit for bit against the
CPU oracle (tests/eval_checks.py has the generators, the plain walk that counts the coverage, and the runners).

The CPU half checks the walk against the oracle on every unit, the coverage floors, and every family on the host simulation (the
wavefront form with one thread, and both --all forms).  The GPU half runs the same units through libambigram_hip.so: as one batch
per family through the ordinary kernel chain, in slices of 32 through the express kernel -- the ONLY place where the register form
(eval_place_regs_n, imperfect_fbi_regs_n) runs at all --, both with and without FLAG_REVERSED, through --all in the lane form and
in the wave form with every order's verdict and path compared, and unit by unit against the host simulation.

The floors are conditions on the corpus (distinct units that reach a branch, in either orientation), counted by the plain walk on
the reference side; profiles/r16_notes.md has the measured values beside the seeds.
"""
import os
import subprocess

import pytest

import eval_checks as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY_NAMES = tuple(ec.FAMILIES)

# placement: at least 3 units each
PLACEMENT_FLOORS = dict(insert_ge_64=3, insert_ge_128=3, insert_mod_64=3, seed_ge_64=3, seed_ge_128=3, moved_three_regs=3,
                        lane63_s_passed=3, lane63_s_skipped=3, lane63_e_passed=3, lane63_e_skipped=3, lane63_s_decisive=3, lane63_e_decisive=3, lane63_s_visible=3, lane63_e_visible=3,
                        behind_lane_63=3, insert_at_end=3,
                        via_s_nr1=3, via_e_nr1=3, via_s_nr2=3, via_e_nr2=3, via_s_nr4=3, via_e_nr4=3, via_s_lds=3, via_e_lds=3,
                        # what the generators are built for, beyond the list above
                        big_behind_lane_1=3, big_behind_lane_61=3, big_behind_lane_63=3, big_at_end=3, pat_at_64=3, pat_at_128=3, pat_at_256=3,
                        pat_arm_start=3, pat_arm_end=3, shift_two_rounds=3, shift_three_rounds=2, pal_over_64_iterations=3)
CAP_FLOORS = {"cap_%d" % c: 2 for c in (64, 72, 128, 136, 192, 200, 256, 264)}
# imperfectFBI: at least 3 units per branch and length class (a palindrome cannot straddle a cell the path does not reach)
FBI_FLOORS = {"%s/%s" % (b, k): 3 for b in ec.FBI_BRANCHES for k in ("le64", "le128", "gt128")
              if not (b == "straddle_63_64" and k == "le64") and not (b == "straddle_127_128" and k != "gt128")}


def all_units(oracle, workdir):
    return [(f, ec.family_units(oracle, workdir, f)) for f in FAMILY_NAMES]


# ---------------------------------------------------------------------------------------------
# CPU half
# ---------------------------------------------------------------------------------------------
def test_walk_equals_the_oracle_and_reaches_the_floors(oracle, workdir):
    """Every generated unit is valid for the oracle through its first order (asserted where it is made); the plain walk of the
    placement and of imperfectFBI gives the oracle's cells on every unit and in both orientations (asserted in coverage()), which is
    what entitles its counters to carry the floors."""
    units = [u for _, us in all_units(oracle, workdir) for u in us]
    c = ec.coverage(units)
    print("eval families:", {k: c[k] for k in sorted(c)})
    floors = dict(PLACEMENT_FLOORS, **CAP_FLOORS, **FBI_FLOORS)
    short = {k: (c.get(k, 0), v) for k, v in floors.items() if c.get(k, 0) < v}
    assert not short, ("coverage below its floor (have, floor)", short)
    fold = ec.family_units(oracle, workdir, "foldbacks")
    assert 3 * sum(u["L"] <= 64 for u in fold) >= len(fold) and 3 * sum(64 < u["L"] <= 128 for u in fold) >= len(fold), c
    assert all(u["K"] <= 12 and 16 <= u["n"] <= 64 and u["R"] <= ec.ALL_MAX_R for u in units)
    # every length the lengths family is built for
    have = {u["L"] for u in ec.family_units(oracle, workdir, "lengths")}
    want = {L for lo, hi in ec.LENGTH_RANGES for L in range(lo, hi + 1, 4)}
    assert want <= have, sorted(want - have)
    # every large copy number, as the seed of the path and as a later insert
    seeds = {u["o"][False]["node2loop"][u["o"][False]["orders"][0][0]][2] for u in ec.family_units(oracle, workdir, "copies")}
    later = {cn for u in ec.family_units(oracle, workdir, "copies") for x in u["o"][False]["orders"][0][1:] for cn in u["o"][False]["node2loop"][x][2:3]}
    assert set(ec.BIG) <= seeds and set(ec.BIG) <= later, (sorted(seeds), sorted(later))


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_family_on_the_host_simulation(hostsim_lib, oracle, workdir, family):
    units = ec.family_units(oracle, workdir, family)
    for rev in (False, True):
        ec.check_against_oracle(units, ec.run_units(hostsim_lib, units, reversed_=rev), rev, "%s on the host simulation" % family)


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_all_orders_on_the_host_simulation(hostsim_lib, oracle, workdir, family):
    """--all: every order's verdict and path (the host simulation hands every chunk to the lane form and to the wave form)."""
    units = [u for u in ec.family_units(oracle, workdir, family) if u["all"]]
    assert len(units) >= 60
    for rev in (False, True):
        ec.check_all_against_oracle(units, ec.run_all(hostsim_lib, units, reversed_=rev), rev, "%s, --all on the host simulation" % family)


def test_generators_are_deterministic(oracle, workdir, tmp_path):
    """The family with the random maps and the shuffled lines, made a second time: the same files."""
    xs, ys = ec.family_units(oracle, workdir, "foldbacks"), ec.FAMILIES["foldbacks"](oracle, str(tmp_path))
    assert len(xs) == len(ys)
    for x, y in zip(xs, ys):
        assert open(x["lh"]).read() == open(y["lh"]).read() and open(x["sol"]).read() == open(y["sol"]).read(), x["name"]
        assert x["o"] == y["o"] and x["facts"] == y["facts"], x["name"]


def test_stage_check_under_asan_ubsan(tmp_path):
    """tests/tools/eval_stage_check.cpp: eval_place, imperfect_fbi, eval_order_lane (strides 1 and 64), shift_up, shift_down and
    expand_bkp on the host group over random DAG records and fold-back maps, the cells in heap blocks of exactly their capacity, as
    a stand-alone program under AddressSanitizer + UBSan.  (The register form is device code: it cannot be built for the host.)"""
    exe = str(tmp_path / "eval_stage_check")
    src = os.path.join(ROOT, "tests", "tools", "eval_stage_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-Wall", "-Wno-sign-compare", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "ambigram_amd", "csrc"),
                        "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and "eval_stage_check: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------
# GPU half
# ---------------------------------------------------------------------------------------------
_HOST = {}


def _host_records(hostsim_lib, family, units, rev):
    if (family, rev) not in _HOST:
        _HOST[(family, rev)] = ec.run_units(hostsim_lib, units, reversed_=rev)
    return _HOST[(family, rev)]


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_family_through_the_kernel_chain(hip_lib, hostsim_lib, oracle, workdir, family):
    """One batch per family through the ordinary chain (AMBI_EXPRESS_UNITS=0): the wavefront form in group memory."""
    units = ec.family_units(oracle, workdir, family)
    for rev in (False, True):
        recs = ec.run_units(hip_lib, units, reversed_=rev)
        ec.check_against_oracle(units, recs, rev, "%s through the kernel chain" % family)
        ec.same_records(units, recs, _host_records(hostsim_lib, family, units, rev), rev, "%s: HIP differs from the host simulation" % family)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_family_through_the_express_kernel(hip_lib, hostsim_lib, oracle, workdir, family):
    """Slices of at most 32 units, run twice: the second run of a small batch takes the express kernel, and with it the register
    form of the placement (bkp_cap <= 256) and of imperfectFBI (L <= 128)."""
    units = ec.family_units(oracle, workdir, family)
    for rev in (False, True):
        host = _host_records(hostsim_lib, family, units, rev)
        for lo in range(0, len(units), 32):
            part = units[lo:lo + 32]
            recs = ec.run_units(hip_lib, part, reversed_=rev, express=True)
            ec.check_against_oracle(part, recs, rev, "%s, express slice at %d" % (family, lo))
            ec.same_records(part, recs, host[lo:lo + 32], rev, "%s, express slice at %d: HIP differs from the host simulation" % (family, lo))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("lanes", "wave"))
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_all_orders_on_the_gpu(hip_lib, oracle, workdir, family, form):
    """--all: one thread per order (units with bkp_cap <= 192; the others take the wave form there too) and AMBI_ALL_LANES=0, a
    wavefront per order for every unit.  Every order's verdict and the path of every valid one."""
    units = [u for u in ec.family_units(oracle, workdir, family) if u["all"]]
    for rev in (False, True):
        recs = ec.run_all(hip_lib, units, reversed_=rev, lanes=form == "lanes")
        ec.check_all_against_oracle(units, recs, rev, "%s, --all in the %s form" % (family, form))
