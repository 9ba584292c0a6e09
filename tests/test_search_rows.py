"""Which row of the order table the device-side readers fetch.

The writers of the table are pinned against the oracle's orders for every node count (tests/test_row_packing.py) and the row
format on the host (tests/test_lehmer_rows.py).  The readers -- eval_indexed under the parallel search, the resolve stage and
the path of a listed order, the wide branch of the --all stage, the scan of a backend without first rows -- were pinned at one
shape only (check_injected_validity: K = 9, one-dword rows, a 280-byte table) and through an observable that does not depend
on the row: every valid order of a unit gives the same path (measured with the oracle for every unit below: one distinct
path among the R of each orientation), so a reader that fetched row f + 1, row 0 or a neighbour's row passed.

Here a hit is injected at a chosen index f (diagnostics hook ambi_batch_debug_inject_validity) and the engine must publish,
beside status / first_valid / first_forward / evaluated and the oracle's path of order f, THE ORDER IT EVALUATED
(ambi_batch_debug_unit_order), equal to the oracle's allTopologicalOrders()[f] -- at every row width of the table:

    row bytes  K               row bytes  K
    4          9, 11           20 - 40    34, 45, 63
    8          12, 19          128        64, 100, 127
    12 - 16    23, 25, 27      256        128, 255

every unit alone and all of them in one batch, through every enumeration path that writes the table; the cases are listed in
engine_checks.search_row_cases.  Integer work, plain equality."""
import time

import pytest

import engine_checks as ec


def _report(kind, t0, batches, oracle_seconds, covered):
    print("\n%s: %d batches, %.1f s in all, %.1f s of them in the oracle; compared with orders[f] behind the scan budget: %s"
          % (kind, batches, time.time() - t0, oracle_seconds, sorted(covered)))


def test_search_and_resolve_read_the_injected_row_on_the_host_simulation(hostsim_lib, oracle, workdir):
    """The stage code on the host simulation, the chunks of the search ascending / descending / shuffled where their order
    matters, and the scan without pre-unranked first rows (a source only the host simulation still has: the HIP backend
    always allocates the first rows).  Measured on 8 cores: 654 batches, 174 s in all, 119 s of them waiting for the oracle, whose
    --all runs are made side by side in worker processes (one after the other they add up to about 175 s: the forward --all of
    K = 19 alone takes 93 s, skew2 128 38 s); the longest test of the suite before this one took 164 s (the sanitizer build)."""
    t0 = time.time()
    batches, oracle_seconds, covered = ec.check_injected_validity_matrix(hostsim_lib, oracle, workdir, search_orders=("asc", "desc", "shuffle"),
                                                                         table_scan=True)
    _report("host simulation", t0, batches, oracle_seconds, covered)
    assert oracle_seconds < 200      # the oracle's share stays affordable (about three minutes at most)


@pytest.mark.gpu
def test_search_and_resolve_read_the_injected_row_on_the_gpu(hip_lib, oracle, workdir):
    t0 = time.time()
    batches, oracle_seconds, covered = ec.check_injected_validity_matrix(hip_lib, oracle, workdir)
    _report("gpu", t0, batches, oracle_seconds, covered)
    assert batches <= 600
