"""The end-of-batch payload at its edges (tests/exchange_checks.py): ambi_batch_pack_paths, ambi_batch_pack_runs, ambi_expand_runs,
ambi_batch_runs_to_host and dist.RunExchange against plain numpy on the ORACLE's paths.  Every check runs on the CPU through the
host simulation with CPU tensors -- the functions of csrc/ambi_exchange.hpp that the kernels call, on one thread, so a thread's
every trip through their loops -- and, marked gpu, through the HIP engine with device tensors: there the kernels ambi_pack_scan /
_copy, ambi_pack_runs_count / _scan / _write and ambi_expand_runs run the same functions with more than one block of 1024 units,
more than one group of 256 runs per unit, empty paths, capacities that are too small and more runs than the expansion starts
wavefronts."""
import pytest

import exchange_checks as xc

# what the oracle and numpy give for check 1's batch ([which = 0, which = 1]); the engine has no part in these figures
BIG = dict(units=2103, empty=785, runs=[29300, 30091], cells=[1176769, 1148383], max_runs=512)


# ---- CPU: host simulation -------------------------------------------------------------------------------------------
def test_big_batch(hostsim_lib, oracle, workdir):
    st = xc.check_big_batch(hostsim_lib, oracle, workdir, "cpu")
    assert st == BIG, st


def test_short_capacities(hostsim_lib, oracle, workdir):
    xc.check_short_capacities(hostsim_lib, oracle, workdir, "cpu")


def test_all_units_empty(hostsim_lib, oracle, workdir):
    xc.check_all_empty(hostsim_lib, oracle, workdir, "cpu")


def test_expand_edge_lengths(hostsim_lib):
    xc.check_expand_edge_lengths(hostsim_lib, "cpu")


def test_expand_many_runs(hostsim_lib):
    xc.check_expand_many_runs(hostsim_lib, "cpu")


def test_expand_no_runs(hostsim_lib):
    xc.check_expand_no_runs(hostsim_lib, "cpu")


def test_exchange_with_slack(hostsim_lib, oracle, workdir):
    xc.check_exchange_with_slack(hostsim_lib, oracle, workdir, "cpu")


# ---- GPU: the HIP engine --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_big_batch(hip_lib, oracle, workdir):
    st = xc.check_big_batch(hip_lib, oracle, workdir, "cuda")
    assert st == BIG, st


@pytest.mark.gpu
def test_gpu_short_capacities(hip_lib, oracle, workdir):
    xc.check_short_capacities(hip_lib, oracle, workdir, "cuda")


@pytest.mark.gpu
def test_gpu_all_units_empty(hip_lib, oracle, workdir):
    xc.check_all_empty(hip_lib, oracle, workdir, "cuda")


@pytest.mark.gpu
def test_gpu_expand_edge_lengths(hip_lib):
    xc.check_expand_edge_lengths(hip_lib, "cuda")


@pytest.mark.gpu
def test_gpu_expand_many_runs(hip_lib):
    xc.check_expand_many_runs(hip_lib, "cuda")


@pytest.mark.gpu
def test_gpu_expand_no_runs(hip_lib):
    xc.check_expand_no_runs(hip_lib, "cuda")


@pytest.mark.gpu
def test_gpu_runs_to_host_both_paths(hip_lib, oracle, workdir):
    """The host simulation refuses which = 0 (it has the runs where the stages wrote them): the engine only."""
    xc.check_runs_to_host(hip_lib, oracle, workdir, "cuda")


@pytest.mark.gpu
def test_gpu_exchange_with_slack(hip_lib, oracle, workdir):
    xc.check_exchange_with_slack(hip_lib, oracle, workdir, "cuda")
