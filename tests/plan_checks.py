"""Checks of the plan stage past one chunk, shared by the CPU host-simulation tests and the GPU tests (same assertions, different
library; tests/test_plan_chunks.py).  ambi_plan_kernel (csrc/ambi_engine.hip) takes 4096 units per chunk and carries the table
offsets (`off_carry`) and the work blocks (`blk_carry`) from chunk to chunk, so those carries are met only by a launch of more
units than that.  The host simulation runs the serial form, plan_serial (csrc/ambi_stages.hpp): its runs prove the test logic and
the arithmetic, the GPU runs test the kernel's chunk loop.

The batch has 4096 + 107 units, so that the kernel enters a second chunk and that chunk is partial.  Unit u is sample u % 7 of
seven small synthetic samples whose order tables are one 4096-byte granule of the arena each (asserted first, on the unlimited
run).  With the arena limited to k granules (AMBI_ARENA_MAX_BYTES = 4096 * k) the tables of the units 0 .. k - 1 fill it exactly,
so the units refused with ORDERS_CAPACITY must be k .. 4202: that expectation is arithmetic on the granule, not engine output."""
import os

import numpy as np

from ambigram_amd import api, synth

N_UNITS, N_SAMPLES, CHUNK, GRANULE = 4203, 7, 4096, 4096
ORDERS_CAPACITY = -15
_items, _free = {}, {}


def samples(workdir):
    """the seven .lh files and their solutions, written once per work directory"""
    if workdir not in _items:
        items = []
        for i in range(N_SAMPLES):
            s = synth.make_sample(48, 100, ("chain", "wide", "mixed")[i % 3], 9 + 2 * (i % 3), seed=9300 + i, imperfect=i % 2)
            lh, sols = s.write(workdir, "pc%d" % i)
            items.append((lh, sols[0]))
        _items[workdir] = items
    return _items[workdir]


def run_batch(lib, workdir, granules):
    """The batch run twice, plainly (first run: the arena grows from one granule) and with FLAG_REVERSED (resident path: plan
    reset, then plan), under an arena limit of `granules` granules (None: no limit).  Per run and unit: (status, num_orders,
    n_nodes, path, the whole order table); path and table only for the units that end with status 0."""
    items = samples(workdir)
    saved = os.environ.pop("AMBI_ARENA_MAX_BYTES", None)
    if granules:
        os.environ["AMBI_ARENA_MAX_BYTES"] = str(GRANULE * granules)
    graphs, b = [], api.Batch(lib)
    try:
        graphs = [api.Graph(lib, lh) for lh, _ in items]
        b.configure(order_arena_bytes=GRANULE, first_budget=3)
        for u in range(N_UNITS):
            b.add_chromosome_sol(graphs[u % N_SAMPLES], 0, items[u % N_SAMPLES][1])
        b.upload()
        outs = []
        for flags in (0, api.FLAG_REVERSED):
            b.run(flags); b.wait(); b.download()
            out = []
            for u in range(N_UNITS):
                r = b.unit_result(u)
                rec = (r["status"], r["num_orders"], r["n_nodes"])
                if r["status"] == 0:
                    rec += (b.unit_path(u, 1).tobytes(), b.unit_orders(u, 0, r["num_orders"], r["n_nodes"]).tobytes())
                out.append(rec)
            outs.append(out)
        return outs
    finally:
        b.close()
        for g in graphs:
            g.close()
        os.environ.pop("AMBI_ARENA_MAX_BYTES", None)
        if saved is not None:
            os.environ["AMBI_ARENA_MAX_BYTES"] = saved


def free_run(lib, workdir):
    """The unlimited run (once per library) and the preconditions of the arithmetic: every unit has rows, every table is one granule."""
    key = (id(lib), workdir)
    if key not in _free:
        free = run_batch(lib, workdir, None)
        for out in free:
            assert all(r[0] == 0 and r[1] > 0 for r in out), [(u, r[:3]) for u, r in enumerate(out) if r[0] != 0 or r[1] <= 0][:8]
            assert max(r[1] * r[2] for r in out) <= GRANULE, max(r[1] * r[2] for r in out)
            assert {r[1] for r in out} == {1, 252, 66}, sorted({r[1] for r in out})   # the three tiers' counts (K = 9, 11, 13)
        _free[key] = free
    return _free[key]


def check_arena_of(lib, workdir, granules):
    """Arena of `granules` granules: exactly the units granules .. 4202 are refused, in both runs; every other unit is what it is in
    the unlimited run (status, counts, path, order table); the order table of a unit of the second chunk equals that of the unit
    u % 7 of the same run (a wrong work-block offset behind the first chunk sends rows to another unit's table or to none)."""
    free = free_run(lib, workdir)
    print("unlimited run: num_orders of the samples", [r[1] for r in free[0][:N_SAMPLES]], "max R * K", max(r[1] * r[2] for r in free[0]))
    lim = run_batch(lib, workdir, granules)
    want = list(range(granules, N_UNITS))
    for i, (out, ref) in enumerate(zip(lim, free)):
        refused = [u for u, r in enumerate(out) if r[0] == ORDERS_CAPACITY]
        print("arena of %d granules, run %d: %d units refused, first %s" % (granules, i, len(refused), refused[0] if refused else None))
        assert refused == want, (granules, i, len(refused), refused[:4], refused[-4:])
        for u in range(granules):
            assert out[u] == ref[u], (granules, i, u, out[u][:3], ref[u][:3])
    for i, out in enumerate(free + lim):
        beyond = [u for u in range(CHUNK, N_UNITS) if out[u][0] == 0]
        assert i >= 2 or len(beyond) == N_UNITS - CHUNK
        for u in beyond:
            assert out[u][4] == out[u % N_SAMPLES][4], (granules, i, u)
            assert np.frombuffer(out[u][4], np.uint8).size == out[u][1] * out[u][2]
    return len(want)
