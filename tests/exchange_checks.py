"""Checks of the end-of-batch payload (ambi_batch_pack_paths, ambi_batch_pack_runs, ambi_expand_runs, ambi_batch_runs_to_host) shared
by the CPU host-simulation tests and the GPU tests (same assertions, different library; tests/test_exchange_payload.py).  On the GPU
these are the kernels ambi_pack_scan / _copy, ambi_pack_runs_count / _scan / _write and ambi_expand_runs of csrc/ambi_engine.hip: set-up
around the functions of csrc/ambi_exchange.hpp, which tests/hostsim/host_backend.cpp calls in the same order with one thread.  The CPU
runs check those functions (and the test logic), the GPU runs check them on workgroups and wavefronts and with the kernels' set-up.

Expected values never come from the engine: the cells are the ORACLE's paths (`path` for which = 0, `path_indel` for which = 1), cut
into runs and laid out with plain numpy (runs_of, Reference); the synthetic runs of check 4 are expanded with numpy.arange.  Every
output buffer is torch memory on `device` ("cpu" or "cuda"), allocated at the size the whole payload needs plus PAD words and filled
with SENT, so a write that should not happen lands in memory the test owns and is seen."""
import ctypes as C

import numpy as np
import torch

import cases
from ambigram_amd import api, synth
from ambigram_amd.dist import RunExchange

SENT = -0x5a5a5a5a      # no segment id, run length or count takes this value
PAD = 8
EMPTY = np.zeros(0, np.int64)


# ---- the reference: plain numpy on the oracle's paths ---------------------------------------------------------------------------
def runs_of(path):
    """(start values, lengths) of the runs of a path: a run starts where a cell is not its predecessor + 1."""
    a = np.asarray(path, np.int64)
    if len(a) == 0:
        return EMPTY, EMPTY
    pos = np.concatenate([[0], np.flatnonzero(a[1:] != a[:-1] + 1) + 1])
    return a[pos], np.diff(np.concatenate([pos, [len(a)]]))


class Reference:
    """Both pack forms of a batch whose unit u has the oracle record records[u]."""

    def __init__(self, records, which):
        memo = {}
        for oc in records:                                  # (a big batch repeats a dozen records)
            if id(oc) not in memo:
                p = np.asarray(oc["path_indel"] if which else oc["path"], np.int64)
                memo[id(oc)] = (p,) + runs_of(p)
        per = [memo[id(oc)] for oc in records]
        self.paths = [p for p, _, _ in per]
        self.lengths = np.array([len(p) for p, _, _ in per], np.int64)
        self.counts = np.array([len(s) for _, s, _ in per], np.int64)
        self.cell_off = np.concatenate([[0], np.cumsum(self.lengths, dtype=np.int64)])
        self.run_off = np.concatenate([[0], np.cumsum(self.counts, dtype=np.int64)])
        self.cells = np.concatenate([p for p, _, _ in per] + [EMPTY])
        self.run_start = np.concatenate([s for _, s, _ in per] + [EMPTY])
        self.run_len = np.concatenate([l for _, _, l in per] + [EMPTY])
        self.n_cells, self.n_runs = int(self.cell_off[-1]), int(self.run_off[-1])
        assert self.n_cells == len(self.cells) and self.n_runs == len(self.run_start) == len(self.run_len)
        assert int(self.run_len.sum()) == self.n_cells


def expected_status(oc):
    return 0 if oc["first_valid"] >= 0 else api.ST_NO_VALID_ORDER


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
SMALL = [((24, 48, "chain", 5), dict()), ((40, 80, "wide", 7), dict(n_del=2)), ((32, 64, "mixed", 6), dict(imperfect=1)),
         ((48, 96, "chain", 9), dict(n_dup=1, n_del=1)), ((40, 80, "wide", 9), dict())]
N_BIG = 2103            # three blocks of 1024 units for the one-workgroup scans, the last one partial
AT_512, AT_PARTIAL = 1023, 1024     # the last slot of the first block, the first slot of the second
_INPUTS = {}


def _one(oracle, workdir, stem, sample):
    lh, sols = sample.write(workdir, stem)
    o = oracle.run_bfb(lh, sols)
    assert o["ok"], o["err"]
    return [(lh, sols[c], c, oc) for c, oc in enumerate(o["chr"])]


def inputs(oracle, workdir):
    """The distinct samples of every check, (lh, sol, chromosome, oracle record) each, computed once per work directory:
    small: the five small units; empty: three random decompositions without a valid order; u512 / u376: the wide units whose path
    has two full groups of 256 runs / a partial second group; chr3: the three chromosomes of one sample (seg_base 0, 32, 64)."""
    if workdir in _INPUTS:
        return _INPUTS[workdir]
    d = {"small": [], "empty": []}
    for i, (spec, kw) in enumerate(SMALL):
        d["small"] += _one(oracle, workdir, "xs%d" % i, synth.make_sample(*spec, seed=8100 + i, **kw))
    seed = 20000
    while len(d["empty"]) < 3:
        lh, sols = cases.random_decomposition(workdir, seed)
        o = oracle.run_bfb(lh, sols)
        oc = o["chr"][0]
        if o["ok"] and oc["first_valid"] < 0 and not oc["shortcut"] and not oc["infeasible"] and not oc["ub_valid"]:
            d["empty"].append((lh, sols[0], 0, oc))
        seed += 1
        assert seed < 20200, "no random decomposition without a valid order"
    d["u512"] = _one(oracle, workdir, "x512", synth.make_sample(420, 840, "chain", 180, seed=778))[0]
    d["u376"] = _one(oracle, workdir, "x376", synth.make_sample(300, 600, "chain", 130, seed=778, n_del=3, n_dup=3))[0]
    d["chr3"] = _one(oracle, workdir, "x3chr", synth.make_sample(96, 192, "chain", 7, seed=5, n_chr=3))
    assert len(d["chr3"]) == 3 and [x[3]["start"] - 1 for x in d["chr3"]] == [0, 32, 64]
    for x in d["small"] + [d["u512"], d["u376"]] + d["chr3"]:
        oc = x[3]
        assert oc["first_valid"] >= 0 and not oc["shortcut"] and not oc["infeasible"] and not oc["ub_valid"] and len(oc["path"]) > 0, x[0]
    for x in d["empty"]:
        assert x[3]["path"] == [] and x[3]["path_indel"] == []
    _INPUTS[workdir] = d
    return d


def big_items(oracle, workdir):
    """Check 1's batch, with its conditions asserted from the oracle alone."""
    d = inputs(oracle, workdir)
    cycle = d["small"] + d["empty"]
    items = [d["u512"] if u == AT_512 else d["u376"] if u == AT_PARTIAL else cycle[u % len(cycle)] for u in range(N_BIG - 3)] + d["chr3"]
    assert len(items) == N_BIG and 2 * 1024 < N_BIG < 3 * 1024 and N_BIG % 1024 != 0
    records = [x[3] for x in items]
    shortest = []
    for which in (0, 1):
        ref = Reference(records, which)
        empty = ref.lengths == 0
        assert empty.sum() >= 500 and (~empty).sum() >= 500
        assert all(empty[k:k + 1024].any() and (~empty[k:k + 1024]).any() for k in (0, 1024, 2048))
        assert ref.counts[AT_512] >= 512 and ref.counts.max() == ref.counts[AT_512]        # two full groups of 256 runs (or more)
        assert 257 <= ref.counts[AT_PARTIAL] <= 511                                          # a partial second group
        assert (ref.run_start < 0).any() and (ref.run_start > 0).any()
        shortest.append(int(ref.run_len.min()))
        assert ref.run_start[ref.run_off[N_BIG - 1]:].max() > 64 and ref.run_start[ref.run_off[N_BIG - 1]:].min() < -64    # absolute ids of the third chromosome, both strands
        assert ref.lengths[AT_512] > 70000 + 256 and ref.counts[AT_512] > 300                # check 2's capacities fall inside this unit
    assert min(shortest) == 1                                                                # a run of one cell (in the edited paths)
    assert any(oc["path"] != oc["path_indel"] for oc in records)                             # which = 0 and 1 differ
    return items


def small_items(oracle, workdir):
    """Checks 5 and 6: the five small units, then the 512-run and the 376-run unit."""
    d = inputs(oracle, workdir)
    return d["small"] + [d["u512"], d["u376"]]


def make_batch(lib, items):
    """One Graph per distinct file, one unit per item."""
    graphs, b = {}, api.Batch(lib)
    for lh, sol, c, _ in items:
        if lh not in graphs:
            graphs[lh] = api.Graph(lib, lh)
        b.add_chromosome_sol(graphs[lh], c, sol)
    return graphs, b


def close_all(graphs, b):
    b.close()
    for g in graphs.values():
        g.close()


def check_statuses(b, records, tag):
    """After a download: a unit without a path is one the oracle finds no valid order for, every other ended with status 0."""
    for u, oc in enumerate(records):
        assert b.unit_result(u)["status"] == expected_status(oc), (tag, u, b.unit_result(u), oc["first_valid"])


# ---- device buffers ---------------------------------------------------------------------------------------------------------------
def _full(n, device, dtype=torch.int32):
    return torch.full((int(n) + PAD,), SENT, dtype=dtype, device=device)


def _stream(device):
    return torch.cuda.current_stream().cuda_stream if device == "cuda" else 0


def _sync(device):
    if device == "cuda":
        torch.cuda.synchronize()


def _same(got, want, tag):
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (tag, "%d words differ, the first at %d: %d, expected %d" % (len(bad), bad[0], got[bad[0]], want[bad[0]]))


def _sent(n):
    return np.full(int(n), SENT, np.int64)


def packed_paths(b, which, U, alloc, cap, device):
    """ambi_batch_pack_paths into sentinel-filled buffers of `alloc` (+ PAD) cells with the capacity `cap`: (lengths, cells, total)"""
    lengths, cells, total = _full(U, device), _full(alloc, device), _full(1, device, torch.int64)
    b.pack_paths(which, lengths.data_ptr(), cells.data_ptr(), int(cap), total.data_ptr(), _stream(device))
    _sync(device)
    return lengths.cpu().numpy(), cells.cpu().numpy(), total.cpu().numpy()


def packed_runs(b, which, U, alloc, cap, device):
    """ambi_batch_pack_runs likewise: (lengths, run_counts, run_start, run_len, totals)"""
    lengths, counts, start, rlen, totals = _full(U, device), _full(U, device), _full(alloc, device), _full(alloc, device), _full(2, device, torch.int64)
    b.pack_runs(which, lengths.data_ptr(), counts.data_ptr(), start.data_ptr(), rlen.data_ptr(), int(cap), totals.data_ptr(), _stream(device))
    _sync(device)
    return lengths.cpu().numpy(), counts.cpu().numpy(), start.cpu().numpy(), rlen.cpu().numpy(), totals.cpu().numpy()


def compare_paths(b, ref, which, cap, device, tag):
    """The cell form with capacity `cap` <= the cells the paths have: lengths and total complete, the cells before `cap` exact,
    nothing written from `cap` on."""
    U = len(ref.lengths)
    lengths, cells, total = packed_paths(b, which, U, ref.n_cells, cap, device)
    _same(lengths, np.concatenate([ref.lengths, _sent(PAD)]), (tag, "lengths"))
    _same(total, np.concatenate([[ref.n_cells], _sent(PAD)]), (tag, "total"))
    _same(cells, np.concatenate([ref.cells[:cap], _sent(ref.n_cells - cap + PAD)]), (tag, "cells"))


def compare_runs(b, ref, which, cap, device, tag):
    """The run-length form with capacity `cap` <= the runs the paths have: counts and totals complete; a unit whose runs all lie
    before `cap` exact; not one word of any other unit, nor any at or past `cap`, written."""
    U = len(ref.lengths)
    lengths, counts, start, rlen, totals = packed_runs(b, which, U, ref.n_runs, cap, device)
    _same(lengths, np.concatenate([ref.lengths, _sent(PAD)]), (tag, "lengths"))
    _same(counts, np.concatenate([ref.counts, _sent(PAD)]), (tag, "run_counts"))
    _same(totals, np.concatenate([[ref.n_runs, ref.n_cells], _sent(PAD)]), (tag, "totals"))
    fits = np.repeat(ref.run_off[:-1] + ref.counts <= cap, ref.counts)       # per run: does its whole unit fit?
    assert not fits[cap:].any()
    _same(start, np.concatenate([np.where(fits, ref.run_start, SENT), _sent(PAD)]), (tag, "run_start"))
    _same(rlen, np.concatenate([np.where(fits, ref.run_len, SENT), _sent(PAD)]), (tag, "run_len"))
    return int(fits.sum())


# ---- check 1: a big mixed batch, exact capacities --------------------------------------------------------------------------------
def check_big_batch(lib, oracle, workdir, device):
    """2103 units (the unit scans carry over two block edges), empty paths in every block, a 512-run unit at the end of the first
    block and a 376-run unit at the start of the second (the run positions carry over groups of 256), three chromosomes with
    seg_base 0 / 32 / 64 at the end.  Two runs (the first sizes the order arena, the second is resident), both forms and both
    paths after each."""
    items = big_items(oracle, workdir)
    records = [x[3] for x in items]
    refs = [Reference(records, which) for which in (0, 1)]
    graphs, b = make_batch(lib, items)
    b.upload()
    for rep in range(2):
        b.run(0, _stream(device)); b.wait(); b.download()
        check_statuses(b, records, ("big", rep))
        for which in (0, 1):
            compare_paths(b, refs[which], which, refs[which].n_cells, device, ("big", rep, which))
            assert compare_runs(b, refs[which], which, refs[which].n_runs, device, ("big", rep, which)) == refs[which].n_runs
    close_all(graphs, b)
    return dict(units=len(items), empty=int((refs[0].lengths == 0).sum()), runs=[r.n_runs for r in refs], cells=[r.n_cells for r in refs],
                max_runs=int(refs[0].counts.max()))


# ---- check 2: capacities that are too small --------------------------------------------------------------------------------------
def check_short_capacities(lib, oracle, workdir, device):
    """The same batch after its second run.  pack_paths clamps per cell; pack_runs writes a unit whole or not at all."""
    items = big_items(oracle, workdir)
    records = [x[3] for x in items]
    graphs, b = make_batch(lib, items)
    b.upload()
    for rep in range(2):
        b.run(0, _stream(device)); b.wait()
    b.download()
    check_statuses(b, records, "short")
    for which in (0, 1):
        ref = Reference(records, which)
        caps = [0, 1, int(ref.cell_off[AT_512]) + 70000, int(ref.cell_off[AT_PARTIAL]), ref.n_cells - 1]
        assert ref.cell_off[AT_512] < caps[2] < ref.cell_off[AT_512 + 1] == caps[3] and sorted(set(caps)) == caps
        for cap in caps:
            compare_paths(b, ref, which, cap, device, ("short cells", which, cap))
        caps = [0, 1, int(ref.run_off[AT_512]) + 300, int(ref.run_off[AT_PARTIAL]), ref.n_runs - 1]
        assert ref.run_off[AT_512] < caps[2] < ref.run_off[AT_512 + 1] == caps[3] and sorted(set(caps)) == caps
        written = [compare_runs(b, ref, which, cap, device, ("short runs", which, cap)) for cap in caps]
        # capacity 1: no unit has fewer than two runs; inside the 512-run unit: everything before it; at the unit edge: it too;
        # one short of everything: all but the last unit (the last chromosome has a path)
        assert written == [0, 0, int(ref.run_off[AT_512]), int(ref.run_off[AT_PARTIAL]), int(ref.run_off[-2])], written
        assert ref.counts[ref.counts > 0].min() >= 2 and ref.counts[-1] > 0
    close_all(graphs, b)


# ---- check 3: a batch whose every unit is empty ----------------------------------------------------------------------------------
def check_all_empty(lib, oracle, workdir, device):
    items = inputs(oracle, workdir)["empty"]
    records = [x[3] for x in items]
    graphs, b = make_batch(lib, items)
    b.upload(); b.run(0, _stream(device)); b.wait(); b.download()
    check_statuses(b, records, "empty")
    U = len(items)
    for which in (0, 1):
        ref = Reference(records, which)
        assert ref.n_cells == 0 and ref.n_runs == 0
        for cap in (0, 64):             # (the buffers are 64 + PAD words either way)
            lengths, cells, total = packed_paths(b, which, U, 64, cap, device)
            _same(lengths, [0] * U + [SENT] * PAD, ("empty", which, "lengths"))
            _same(total, [0] + [SENT] * PAD, ("empty", which, "total"))
            _same(cells, _sent(64 + PAD), ("empty", which, "cells"))
            lengths, counts, start, rlen, totals = packed_runs(b, which, U, 64, cap, device)
            _same(lengths, [0] * U + [SENT] * PAD, ("empty", which, "lengths of runs"))
            _same(counts, [0] * U + [SENT] * PAD, ("empty", which, "run_counts"))
            _same(totals, [0, 0] + [SENT] * PAD, ("empty", which, "totals"))
            _same(start, _sent(64 + PAD), ("empty", which, "run_start"))
            _same(rlen, _sent(64 + PAD), ("empty", which, "run_len"))
    close_all(graphs, b)


# ---- check 4: expand_runs alone ----------------------------------------------------------------------------------------------------
def expand(lib, start, lens, cap, device, alloc=None):
    """ambi_expand_runs of the given runs at the numpy.cumsum offsets into a sentinel-filled buffer: (return code, cells + PAD)"""
    lens = np.asarray(lens, np.int64)
    off = np.cumsum(lens, dtype=np.int64) - lens
    t_start = torch.from_numpy(np.asarray(start, np.int32)).to(device)
    t_len = torch.from_numpy(lens.astype(np.int32)).to(device)
    t_off = torch.from_numpy(off).to(device)
    cells = _full(int(lens.sum()) if alloc is None else alloc, device)
    rc = lib.ambi_expand_runs(C.c_void_p(t_start.data_ptr()), C.c_void_p(t_len.data_ptr()), C.c_void_p(t_off.data_ptr()), len(lens),
                              C.c_void_p(cells.data_ptr()), int(cap), C.c_void_p(_stream(device)))
    _sync(device)
    return rc, cells.cpu().numpy()


def expanded(start, lens):
    return np.concatenate([np.arange(s, s + l, dtype=np.int64) for s, l in zip(start, lens)] + [EMPTY])


EDGE_LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 420, 70000]      # around one and two strides of the 64 lanes of a wavefront, and many strides


def check_expand_edge_lengths(lib, device):
    """(a) 700 runs whose lengths cycle through EDGE_LENGTHS, half of the starts negative; exact capacity, then one that cuts a
    70 000-cell run in the middle."""
    rng = np.random.default_rng(4101)
    n = 700
    lens = np.array([EDGE_LENGTHS[i % len(EDGE_LENGTHS)] for i in range(n)], np.int64)
    start = rng.integers(1, 30001, n) * np.where(np.arange(n) % 2, -1, 1)
    assert (start < 0).sum() == n // 2 and np.abs(start).max() <= 30000
    assert all(((lens == l) & (start < 0)).any() and ((lens == l) & (start > 0)).any() for l in EDGE_LENGTHS)
    want = expanded(start, lens)
    total = int(lens.sum())
    assert len(want) == total
    rc, cells = expand(lib, start, lens, total, device)
    assert rc == 0
    _same(cells, np.concatenate([want, _sent(PAD)]), "expand, exact capacity")
    r = int(np.flatnonzero(lens == 70000)[3])
    cap = int(lens[:r].sum()) + 35000
    assert 0 < cap < total - 70000
    rc, cells = expand(lib, start, lens, cap, device)
    assert rc == 0
    _same(cells, np.concatenate([want[:cap], _sent(total - cap + PAD)]), "expand, capacity inside a run")


GRID_WAVES = 65536 * 4      # the most wavefronts the launch starts; more runs than that take a second trip of the run loop


def check_expand_many_runs(lib, device):
    """(b) 262 144 + 5 runs of 0 .. 3 cells: five runs more than wavefronts, each of the five with cells."""
    rng = np.random.default_rng(4102)
    n = GRID_WAVES + 5
    lens = rng.integers(0, 4, n)
    lens[GRID_WAVES:] = [3, 1, 2, 3, 1]           # a run that only a second trip reaches must have cells to be seen
    start = rng.integers(1, 30001, n) * np.where(rng.integers(0, 2, n) == 1, -1, 1)
    assert all((lens == l).sum() > 1000 for l in range(4))
    pos = np.cumsum(lens) - lens
    want = np.repeat(start, lens) + (np.arange(int(lens.sum())) - np.repeat(pos, lens))      # (= expanded(), vectorised) ...
    k = GRID_WAVES - 40
    assert want[pos[k]:].tolist() == expanded(start[k:], lens[k:]).tolist()                  # ... as the tail shows
    rc, cells = expand(lib, start, lens, len(want), device)
    assert rc == 0
    _same(cells, np.concatenate([want, _sent(PAD)]), "expand, more runs than wavefronts")


def check_expand_no_runs(lib, device):
    """(c) n_runs = 0: return code 0, nothing written."""
    rc, cells = expand(lib, np.zeros(0, np.int32), np.zeros(0, np.int64), 64, device, alloc=64)
    assert rc == 0
    _same(cells, _sent(64 + PAD), "expand, no runs")


# ---- check 5: runs_to_host with which = 0 (the engine only) -------------------------------------------------------------------------
def check_runs_to_host(lib, oracle, workdir, device):
    """which = 0 always goes through the pack kernels, into a slot sized from the breakpoint capacities (and by runs_wait once
    more, should the totals name more runs than that); which = 1 is the copy of the finish kernels' run slots.  Both slots, both
    paths, every unit expanded on the host."""
    items = small_items(oracle, workdir)
    records = [x[3] for x in items]
    U = len(items)
    graphs, b = make_batch(lib, items)
    b.upload(); b.run(0, _stream(device)); b.wait()
    caps = []
    for which in (0, 1):
        ref = Reference(records, which)
        b.runs_to_host(which, 0, _stream(device)); views = [b.runs_wait(0)]
        b.runs_to_host(which, 1, _stream(device)); views.append(b.runs_wait(1))
        if which == 0:      # through the pack kernels: the block that travelled is 4 + 2 U + 2 * capacity words
            caps = [(v["copied_bytes"] // 4 - 4 - 2 * U) // 2 for v in views]
            assert min(caps) >= ref.n_runs, (caps, ref.n_runs)
        for slot, v in enumerate(views):
            assert (v["n_runs"], v["n_cells"]) == (ref.n_runs, ref.n_cells), (which, slot, v["n_runs"], v["n_cells"])
            _same(v["lengths"], ref.lengths, (which, slot, "lengths"))
            _same(v["run_counts"], ref.counts, (which, slot, "run_counts"))
            for u in range(U):
                _same(b.runs_unit_path(slot, u), ref.paths[u], (which, slot, u))
    b.download()
    check_statuses(b, records, "runs_to_host")
    close_all(graphs, b)
    return dict(capacities=caps, runs=Reference(records, 0).n_runs)


# ---- check 6: RunExchange with slack ------------------------------------------------------------------------------------------------
def check_exchange_with_slack(lib, oracle, workdir, device):
    """One rank whose buffers are larger than its payload: 100 spare runs and cells, 5 spare unit slots."""
    items = small_items(oracle, workdir)
    records = [x[3] for x in items]
    U = len(items)
    graphs, b = make_batch(lib, items)
    b.upload(); b.run(0, _stream(device)); b.wait(); b.download()
    check_statuses(b, records, "slack")
    for which in (0, 1):
        ref = Reference(records, which)
        rx = RunExchange(lib, U + 5, ref.n_runs + 100, ref.n_cells + 100, device, world=1, rank=0)
        assert (rx.unit_cap, rx.run_cap, rx.cell_cap) == (U + 5, ref.n_runs + 100, ref.n_cells + 100)
        rx.pack(b, which)
        _sync(device)
        # the packed runs are checked BEFORE they are expanded: expand_runs trusts its offsets, wrong lengths must end the check here
        runs, counts = rx.runs.cpu().numpy(), rx.counts.cpu().numpy()
        _same(counts, np.concatenate([ref.lengths, [0] * 5, ref.counts, [0] * 5]), ("slack", which, "counts"))
        _same(runs[:rx.run_cap], np.concatenate([ref.run_start, [0] * 100]), ("slack", which, "run_start"))
        _same(runs[rx.run_cap:], np.concatenate([ref.run_len, [0] * 100]), ("slack", which, "run_len"))
        rx.exchange()
        rx.expand()
        _sync(device)
        got = rx.collect()
        assert len(got) == 1 and len(got[0]) == U + 5
        for u in range(U):
            _same(got[0][u], ref.paths[u], ("slack", which, u))
        assert got[0][U:] == [[]] * 5
        assert rx.totals.cpu().tolist() == [ref.n_runs, ref.n_cells]
    close_all(graphs, b)
