"""Random posets through the order-ideal lattice and the whole order table, against a plain-Python reference on
arbitrary-precision integers (tests/order_checks.py has the generators, the reference and the checks).

The CPU half runs the host simulation; the GPU half runs the same units through libambigram_hip.so, where alone the
one-work-block image build of stage_unit_image runs (the host simulation never takes it).  Every unit alone and
all of them as one batch under every member of engine_checks.TABLE_VARIANTS; the too-big units (tables that no arena holds:
five kinds, among them the two directions in which the byte count leaves int64) each between two ordinary units.
profiles/r17_notes.md has the figures.

The coverage floors are facts of the reference and of formulas restated in order_checks (rows per lane, row bytes): at least
three units per family, per row class, of width three or more, with more than 256 ideals, with one and with several work blocks,
and per too-big kind (order_checks.too_big_kind: from the reference's byte count alone).
"""
import pytest

import engine_checks as ec
import order_checks as oc

FLOOR = 3


def _floors(c):
    keys = ["width3", "ideals_over_256", "one_block", "several_blocks", "windowed", "over_65535"] + ["family_" + f for f in oc.FAMILIES] + \
           ["class_" + k for k in ec.ROW_CLASSES]
    short = {k: c[k] for k in keys if c[k] < FLOOR}
    assert not short, ("coverage below its floor of %d" % FLOOR, short, c)
    assert all(c["class_%s_width3" % k] >= 1 for k in ec.ROW_CLASSES), c
    assert c["rows"] <= 2500000 and c["bytes"] <= oc.ARENA_CAP, c


def _neighbours(oracle, workdir):
    units, _ = oc.family_units(oracle, workdir)
    by = {u["name"]: u for u in units}
    assert by["oi0"]["R"] <= 256 * 4 < by["ot34_0"]["R"]
    return by["oi0"], by["ot34_0"]          # rows of 4 and of 24 bytes, one work block and two


def _too_big_batches(oracle, workdir):
    """(what, units, ideal_cap): every too-big unit between two ordinary ones, the pairs of the running sum in one batch, and all of
    the ordinary kinds mixed in one batch.  The floor of three per kind is asserted here, from the reference's byte counts."""
    big = oc.cached(oracle, workdir, "toobig", oc.too_big_units)
    a, b = _neighbours(oracle, workdir)
    kinds = {}
    for kind, units in big.items():
        for u in units:
            assert oc.too_big_kind(u) == kind and u["bytes"] > oc.TABLE_MAX_BYTES and u["R"] > 10 ** 14, (u["name"], kind, u["R"], u["bytes"])
            kinds[kind] = kinds.get(kind, 0) + 1
    pairs = [(big["half"][i], big["half"][j]) for i, j in oc.RUNNING_SUM_PAIRS]
    for x, y in pairs:
        assert x["bytes"] < 1 << 63 and y["bytes"] < 1 << 63 and x["bytes"] + y["bytes"] >= 1 << 63, (x["name"], y["name"])
    kinds["running_sum"] = len(pairs)
    del kinds["half"]
    short = {k: n for k, n in kinds.items() if n < FLOOR}
    assert not short and set(kinds) == {"petabytes", "wrap_negative", "wrap_positive", "running_sum", "saturated"}, ("too-big kinds below the floor", kinds)
    strides = {k: {u["stride"] for u in v} for k, v in big.items()}
    assert all(len(v) >= 2 for v in strides.values()), strides                      # no kind at one row width only
    out = [("%s %s" % (kind, u["name"]), [a, u, b], 0) for kind in ("petabytes", "wrap_negative", "wrap_positive") for u in big[kind]]
    out += [("running_sum %s %s" % (x["name"], y["name"]), [a, x, y, b], 0) for x, y in pairs]
    out += [("saturated %s" % u["name"], [a, u, b], oc.SATURATED_IDEAL_CAP) for u in big["saturated"]]
    mixed = [u for kind in ("half", "wrap_negative", "petabytes", "wrap_positive") for u in big[kind]]
    out.append(("all", mixed[:5] + [a] + mixed[5:] + [b], 0))
    return out


def _check_too_big(lib, oracle, workdir):
    for what, units, ideal_cap in _too_big_batches(oracle, workdir):
        oc.assert_clean(oc.run_and_check(lib, units, ideal_cap=ideal_cap), "too big: " + what)


def _check_ideal_caps(lib, oracle, workdir):
    """ol_2050 (2050 ideals, just above half the default ideal_cap of 4096) and ol_over (3712) end with IDEALS_CAPACITY in the
    family batch; with ideal_cap = 8192 their lattices are built: exact counts, no room for 10^12 / 5e10 rows.  ol_264 (264
    ideals, a table in the family batch) ends with IDEALS_CAPACITY when ideal_cap is 512, and ol_256 (256 ideals) keeps its table."""
    units, _ = oc.family_units(oracle, workdir)
    by = {u["name"]: u for u in units}
    just, over = dict(by["ol_2050"], expect="count"), dict(by["ol_over"], expect="count")
    assert just["ideals"] == 2050 and over["ideals"] == 58 * 64 and min(just["bytes"], over["bytes"]) > oc.ARENA_CAP
    oc.assert_clean(oc.run_and_check(lib, [by["oi0"], just, over], ideal_cap=8192), "ideal_cap raised")
    small = dict(by["ol_264"], expect="ideals")
    assert small["ideals"] == 264 and by["ol_256"]["ideals"] == 256
    oc.assert_clean(oc.run_and_check(lib, [by["oi0"], by["ol_256"], small], ideal_cap=512), "ideal_cap lowered")


def _check_alone(lib, units):
    bad = {}
    for u in units:
        bad.update(oc.run_and_check(lib, [u]))
    oc.assert_clean(bad, "units alone")


# ---------------------------------------------------------------------------------------------
# CPU half
# ---------------------------------------------------------------------------------------------
def test_reference_on_known_posets():
    """The reference against closed forms: a product of chains has multinomial many extensions, an antichain K!; unrank agrees with
    the listing; a cycle has none."""
    import math
    P = oc.Poset([0b10, 0b100, 0, 0b10000, 0])              # 0 -> 1 -> 2 and 3 -> 4
    assert P.count() == math.comb(5, 2) and P.shape() == (4 * 3, 2)
    rows = P.rows(0, 10).tolist()
    assert rows == sorted(rows) and len({tuple(r) for r in rows}) == 10 and rows[0] == [0, 1, 2, 3, 4] and rows[-1] == [3, 4, 0, 1, 2]
    assert [P.unrank(r) for r in range(10)] == rows and P.rows(3, 4).tolist() == rows[3:7]
    A = oc.Poset([0] * 6)
    assert A.count() == 720 and A.shape() == (64, 6) and A.unrank(719) == [5, 4, 3, 2, 1, 0]
    big = oc.Poset([1 << (i + 1) if i % 31 != 30 else 0 for i in range(62)])          # 31 + 31
    assert big.count() == math.comb(62, 31) and big.count() * 40 > 1 << 64
    assert oc.Poset([0b10, 0b1]).count() == 0


def test_family_coverage(oracle, workdir):
    units, facts = oc.family_units(oracle, workdir)
    c = oc.coverage(units)
    print("order fuzz:", c, facts)
    _floors(c)
    assert c["T"] == 4 and oc.coverage(units, lanes=64)["T"] == 1024          # the counts family straddles 256 * T for both
    assert sum(facts["dropped"].values()) < facts["random_seeds"] // 2, facts
    assert len({u["name"] for u in units}) == len(units)


def test_units_alone_on_the_host_simulation(hostsim_lib, oracle, workdir):
    _check_alone(hostsim_lib, oc.family_units(oracle, workdir)[0])


@pytest.mark.parametrize("variant", ec.TABLE_VARIANTS, ids=[v[0] for v in ec.TABLE_VARIANTS])
def test_one_batch_on_the_host_simulation(hostsim_lib, oracle, workdir, variant):
    oc.assert_clean(oc.run_and_check(hostsim_lib, oc.family_units(oracle, workdir)[0], variant), variant[0])


def test_ideal_capacity_on_the_host_simulation(hostsim_lib, oracle, workdir):
    _check_ideal_caps(hostsim_lib, oracle, workdir)


def test_too_big_units_on_the_host_simulation(hostsim_lib, oracle, workdir):
    """Without the rule of order_table_too_big (csrc/ambi_stages.hpp) the 30 + 31 unit gets a negative byte count, "fits" at the
    offset of the unit in front, is given 10^12 work blocks and the host simulation writes outside its arena."""
    _check_too_big(hostsim_lib, oracle, workdir)


def test_failed_arena_growth_on_the_host_simulation(hostsim_lib, oracle, workdir):
    """No AMBI_ARENA_MAX_BYTES: the plan asks for 2.3e14 bytes (below 2^48: a table it wants; above 2^47: more than a process can
    address), the growth fails, the arena of 1 MiB stays: the unit in front keeps its table, the unit itself and the one behind
    it (whose offset lies beyond the arena: the plan's prefix sum) end with ORDERS_CAPACITY, all counts exact."""
    big = oc.cached(oracle, workdir, "unallocatable", oc.unallocatable_unit)
    assert 1 << 47 < big["bytes"] < oc.TABLE_MAX_BYTES
    a, b = _neighbours(oracle, workdir)
    assert a["bytes"] + 16 <= 1 << 20
    oc.assert_clean(oc.run_and_check(hostsim_lib, [a, big, dict(b, expect="count")], arena_cap=0, arena_bytes=1 << 20), "failed growth")


# ---------------------------------------------------------------------------------------------
# GPU half
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_too_big_units_on_the_gpu(hip_lib, oracle, workdir):
    _check_too_big(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_units_alone_on_the_gpu(hip_lib, oracle, workdir):
    _check_alone(hip_lib, oc.family_units(oracle, workdir)[0])


GPU_VARIANTS = ec.TABLE_VARIANTS + (("block_dfs_0", {"AMBI_BLOCK_DFS": "0"}, 0), ("build_in_emit_0", {"AMBI_BUILD_IN_EMIT": "0"}, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", GPU_VARIANTS, ids=[v[0] for v in GPU_VARIANTS])
def test_one_batch_on_the_gpu(hip_lib, oracle, workdir, variant):
    oc.assert_clean(oc.run_and_check(hip_lib, oc.family_units(oracle, workdir)[0], variant), variant[0])


@pytest.mark.gpu
def test_ideal_capacity_on_the_gpu(hip_lib, oracle, workdir):
    _check_ideal_caps(hip_lib, oracle, workdir)
