"""Path alignment (ambi_batch_path_align: csrc/ambi_path_align.hpp, ambi_path_align_kernel): a canonical shortest insert / delete
script of pairs of paths in one orientation as maximal runs -- against a plain-Python model of the rules and against what any script
must do (tests/path_align_checks.py).  Every check runs on the CPU through the host simulation (the same stage code on the 1-thread
group) and, marked gpu, through the HIP engine."""
import os
import subprocess

import pytest

import path_align_checks as pac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU: host simulation -------------------------------------------------------------------------------------------
def test_model_against_table():
    """The source of the expected runs, the model, against the quadratic LCS table and the script checks."""
    pac.check_model()


def test_traceback_floors():
    """What the traceback shapes offer, from the model: 300 edits in more runs than a group has threads (all deletions, and all
    insertions the other way round), 300 alternating runs, ONE run of 300 cells, clipped history rows, edits at both ends of the
    middle window, a deletion directly followed by an insertion."""
    pac.check_traceback_floors()


def test_floors(oracle, workdir):
    """What the units offer, from the model: a pair with at least 40 runs, a run of at least 512 cells, both kinds, five equal pairs,
    and NO pair above the cap of 1024 (the cap must not hide a failure)."""
    pac.check_floors(oracle, workdir)


def test_small_shapes(hostsim_lib, oracle, workdir):
    pac.check_small(hostsim_lib, oracle, workdir)


def test_small_shapes_more_pairs_than_workgroups(hostsim_lib, oracle, workdir):
    pac.check_small(hostsim_lib, oracle, workdir, grid=3)


def test_traceback_shapes(hostsim_lib, oracle, workdir):
    pac.check_traceback(hostsim_lib, oracle, workdir)


def test_all_units_two_runs(hostsim_lib, oracle, workdir):
    pac.check_units(hostsim_lib, oracle, workdir)


def test_each_unit_alone(hostsim_lib, oracle, workdir):
    pac.check_each_alone(hostsim_lib, oracle, workdir)


def test_request_paths(hostsim_lib, oracle, workdir):
    pac.check_request_paths(hostsim_lib, oracle, workdir)


def test_set_between_request_and_wait(hostsim_lib, oracle, workdir):
    pac.check_set_between_request_and_wait(hostsim_lib, oracle, workdir)


def test_align_from_compare(hostsim_lib, oracle, workdir):
    pac.check_from_compare(hostsim_lib, oracle, workdir)


def test_cli_path_align(hostsim_lib, oracle, workdir, tmp_path):
    exe = os.path.join(ROOT, "tests", "hostsim", "Ambigram_hostsim")
    assert os.path.exists(exe)
    pac.check_cli(hostsim_lib, exe, str(tmp_path), oracle, workdir)


def test_errors(hostsim_lib):
    pac.check_errors(hostsim_lib, [0, 0, 0])


def test_stage_check_under_asan_ubsan(tmp_path):
    """tests/tools/path_align_stage_check.cpp: align_pair on the host group against a naive transcription (the quadratic LCS table for
    the distance, apply-the-script for validity) over hand-built and random pairs of {+-1 .. +-3}, every buffer -- the history
    included -- a heap block of exactly its stated size, as a stand-alone program under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "path_align_stage_check")
    src = os.path.join(ROOT, "tests", "tools", "path_align_stage_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-Wall", "-Wno-sign-compare", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "ambigram_amd", "csrc"),
                        "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and "path_align_stage_check: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---- GPU: the HIP engine --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_small_shapes(hip_lib, oracle, workdir):
    pac.check_small(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_small_shapes_more_pairs_than_workgroups(hip_lib, oracle, workdir):
    pac.check_small(hip_lib, oracle, workdir, grid=3)


@pytest.mark.gpu
def test_gpu_traceback_shapes(hip_lib, oracle, workdir):
    pac.check_traceback(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_all_units_two_runs(hip_lib, oracle, workdir):
    pac.check_units(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_each_unit_alone(hip_lib, oracle, workdir):
    pac.check_each_alone(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_request_paths(hip_lib, oracle, workdir):
    """The run on one stream, every request on another."""
    import torch
    run_s, req_s = torch.cuda.Stream(), torch.cuda.Stream()
    pac.check_request_paths(hip_lib, oracle, workdir, run_s.cuda_stream, req_s.cuda_stream)


@pytest.mark.gpu
def test_gpu_set_between_request_and_wait(hip_lib, oracle, workdir):
    """The engine queues both requests again at their waits (a run in between moved the results' epoch): each with its own paths.
    Once on the run's stream, once with the requests on another."""
    import torch
    pac.check_set_between_request_and_wait(hip_lib, oracle, workdir)
    run_s, req_s = torch.cuda.Stream(), torch.cuda.Stream()
    pac.check_set_between_request_and_wait(hip_lib, oracle, workdir, run_s.cuda_stream, req_s.cuda_stream, req_s.synchronize)


@pytest.mark.gpu
def test_gpu_align_from_compare(hip_lib, oracle, workdir):
    pac.check_from_compare(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_device_view(hip_lib, oracle, workdir):
    pac.check_device_view(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_cli_path_align(hip_lib, oracle, workdir, tmp_path):
    exe = os.path.join(ROOT, "ambigram_amd", "bin", "Ambigram")
    assert os.path.exists(exe), "build the CLI first (__graft_entry__.build)"
    pac.check_cli(hip_lib, exe, str(tmp_path), oracle, workdir)


@pytest.mark.gpu
def test_gpu_errors(hip_lib):
    pac.check_errors(hip_lib, [0, 0])
