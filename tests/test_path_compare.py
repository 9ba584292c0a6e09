"""Path comparison (ambi_batch_path_compare: csrc/ambi_path_compare.hpp, ambi_path_compare_kernel): common prefix and suffix, indel
distance and LCS of pairs of paths in both orientations -- against plain loops and the bit-vector LCS recurrence on Python integers
over the ORACLE's paths (tests/path_compare_checks.py).  Every check runs on the CPU through the host simulation (the same stage
code on the 1-thread group) and, marked gpu, through the HIP engine."""
import os
import subprocess

import pytest

import path_compare_checks as pcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU: host simulation -------------------------------------------------------------------------------------------
def test_recurrence_against_table():
    """The source of the expected values, the bit-vector recurrence, against the quadratic table; the model walk against both."""
    pcc.check_recurrence()


def test_floors(oracle, workdir):
    """What the units must offer, from the walk itself: the distances 27, 35, 100, 103 and 190 between path and path_indel, an equal
    pair, a pair above the cap of 64, NO pair above the cap of 1024 (the cap must not hide a failure), a snake of 1024 cells or more."""
    pcc.check_floors(oracle, workdir)


def test_small_shapes(hostsim_lib, oracle, workdir):
    pcc.check_small(hostsim_lib, oracle, workdir)


def test_small_shapes_more_pairs_than_workgroups(hostsim_lib, oracle, workdir):
    pcc.check_small(hostsim_lib, oracle, workdir, grid=3)


def test_all_units_two_runs(hostsim_lib, oracle, workdir):
    pcc.check_units(hostsim_lib, oracle, workdir)


def test_each_unit_alone(hostsim_lib, oracle, workdir):
    pcc.check_each_alone(hostsim_lib, oracle, workdir)


def test_request_paths(hostsim_lib, oracle, workdir):
    pcc.check_request_paths(hostsim_lib, oracle, workdir)


def test_set_between_request_and_wait(hostsim_lib, oracle, workdir):
    pcc.check_set_between_request_and_wait(hostsim_lib, oracle, workdir)


def test_cli_path_compare(hostsim_lib, oracle, workdir, tmp_path):
    exe = os.path.join(ROOT, "tests", "hostsim", "Ambigram_hostsim")
    assert os.path.exists(exe)
    pcc.check_cli(hostsim_lib, exe, str(tmp_path), oracle, workdir)


def test_errors(hostsim_lib):
    pcc.check_errors(hostsim_lib, [0, 0, 0])


def test_stage_check_under_asan_ubsan(tmp_path):
    """tests/tools/path_compare_stage_check.cpp: compare_pair on the host group against a naive transcription (plain loops, the
    quadratic LCS table) over hand-built and random pairs of {+-1 .. +-3}, every buffer a heap block of exactly its stated size, as
    a stand-alone program under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "path_compare_stage_check")
    src = os.path.join(ROOT, "tests", "tools", "path_compare_stage_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-Wall", "-Wno-sign-compare", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "ambigram_amd", "csrc"),
                        "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and "path_compare_stage_check: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---- GPU: the HIP engine --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_small_shapes(hip_lib, oracle, workdir):
    pcc.check_small(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_small_shapes_more_pairs_than_workgroups(hip_lib, oracle, workdir):
    pcc.check_small(hip_lib, oracle, workdir, grid=3)


@pytest.mark.gpu
def test_gpu_all_units_two_runs(hip_lib, oracle, workdir):
    pcc.check_units(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_each_unit_alone(hip_lib, oracle, workdir):
    pcc.check_each_alone(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_request_paths(hip_lib, oracle, workdir):
    """The run on one stream, every request on another."""
    import torch
    run_s, req_s = torch.cuda.Stream(), torch.cuda.Stream()
    pcc.check_request_paths(hip_lib, oracle, workdir, run_s.cuda_stream, req_s.cuda_stream)


@pytest.mark.gpu
def test_gpu_set_between_request_and_wait(hip_lib, oracle, workdir):
    """The engine queues the request again at the wait (a run in between moved the results' epoch): with the request's own paths.
    Once on the run's stream, once with the request on another."""
    import torch
    pcc.check_set_between_request_and_wait(hip_lib, oracle, workdir)
    run_s, req_s = torch.cuda.Stream(), torch.cuda.Stream()
    pcc.check_set_between_request_and_wait(hip_lib, oracle, workdir, run_s.cuda_stream, req_s.cuda_stream, req_s.synchronize)


@pytest.mark.gpu
def test_gpu_device_view(hip_lib, oracle, workdir):
    pcc.check_device_view(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_cli_path_compare(hip_lib, oracle, workdir, tmp_path):
    exe = os.path.join(ROOT, "ambigram_amd", "bin", "Ambigram")
    assert os.path.exists(exe), "build the CLI first (__graft_entry__.build)"
    pcc.check_cli(hip_lib, exe, str(tmp_path), oracle, workdir)


@pytest.mark.gpu
def test_gpu_errors(hip_lib):
    pcc.check_errors(hip_lib, [0, 0])
