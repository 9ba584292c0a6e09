"""Path coordinates (ambi_batch_path_coords: csrc/ambi_path_coords.hpp, ambi_path_coords_kernel, ambi_path_lift_kernel): the base-pair
offset of every cell of every path and the lift-over of amplicon positions to cell, segment and offset in the segment -- against
numpy's cumsum and searchsorted over the ORACLE's paths (tests/path_coords_checks.py).  Every check runs on the CPU through the host
simulation (the same stage code on the 1-thread group) and, marked gpu, through the HIP engine."""
import os
import subprocess

import pytest

import path_coords_checks as pcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU: host simulation -------------------------------------------------------------------------------------------
def test_floors(oracle, workdir):
    """What the units must offer, from the oracle's paths alone: a unit without a path, the shortest path (4 cells), a path below one
    round of the scan (512 cells), one of at least two rounds plus one, both parities, '-' cells, a path of exactly one round (the
    pinned seed, found again by the bounded search); and from the drawn lengths an amplicon above 2^32 and zero-length cells at the
    front, in the middle and at the end."""
    pcc.check_floors(oracle, workdir)


def test_small_shapes(hostsim_lib, oracle, workdir):
    pcc.check_small(hostsim_lib, oracle, workdir)


def test_small_shapes_one_lift_workgroup(hostsim_lib, oracle, workdir):
    pcc.check_small(hostsim_lib, oracle, workdir, grid=1)


def test_against_sequence(hostsim_lib, oracle, workdir):
    pcc.check_against_sequence(hostsim_lib, oracle, workdir)


def test_two_runs(hostsim_lib, oracle, workdir):
    pcc.check_two_runs(hostsim_lib, oracle, workdir)


def test_cli_path_coords(hostsim_lib, oracle, workdir, tmp_path):
    exe = os.path.join(ROOT, "tests", "hostsim", "Ambigram_hostsim")
    assert os.path.exists(exe)
    pcc.check_cli(hostsim_lib, exe, str(tmp_path), oracle, workdir)


def test_errors(hostsim_lib):
    pcc.check_errors(hostsim_lib, [0, 0, 0])


def test_stage_check_under_asan_ubsan(tmp_path):
    """tests/tools/path_coords_stage_check.cpp: coords_unit and lift_query on the host group against a naive transcription (a running
    sum, a linear search) over hand-built and random paths of {+-1 .. +-3} with lengths including 0 and 2^31 - 1, every buffer a heap
    block of exactly its stated size, as a stand-alone program under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "path_coords_stage_check")
    src = os.path.join(ROOT, "tests", "tools", "path_coords_stage_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-Wall", "-Wno-sign-compare", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "ambigram_amd", "csrc"),
                        "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and "path_coords_stage_check: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---- GPU: the HIP engine --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_small_shapes(hip_lib, oracle, workdir):
    pcc.check_small(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_small_shapes_one_lift_workgroup(hip_lib, oracle, workdir):
    """AMBI_LIFT_GRID=1: one workgroup of 256 threads strides over tens of thousands of queries; run and requests on two streams."""
    import torch
    run_s, req_s = torch.cuda.Stream(), torch.cuda.Stream()
    pcc.check_small(hip_lib, oracle, workdir, grid=1, run_stream=run_s.cuda_stream, req_stream=req_s.cuda_stream)


@pytest.mark.gpu
def test_gpu_against_sequence(hip_lib, oracle, workdir):
    pcc.check_against_sequence(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_two_runs(hip_lib, oracle, workdir):
    """Once on the run's stream, once with the requests on a second stream."""
    import torch
    pcc.check_two_runs(hip_lib, oracle, workdir)
    run_s, req_s = torch.cuda.Stream(), torch.cuda.Stream()
    pcc.check_two_runs(hip_lib, oracle, workdir, run_s.cuda_stream, req_s.cuda_stream, req_s.synchronize)


@pytest.mark.gpu
def test_gpu_device_view(hip_lib, oracle, workdir):
    pcc.check_device_view(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_cli_path_coords(hip_lib, oracle, workdir, tmp_path):
    exe = os.path.join(ROOT, "ambigram_amd", "bin", "Ambigram")
    assert os.path.exists(exe), "build the CLI first (__graft_entry__.build)"
    pcc.check_cli(hip_lib, exe, str(tmp_path), oracle, workdir)


@pytest.mark.gpu
def test_gpu_errors(hip_lib):
    pcc.check_errors(hip_lib, [0, 0])
