"""Fold-back arm profile of the paths (ambi_batch_fold_profile: csrc/ambi_fold_profile.hpp, ambi_fold_arm_kernel and
ambi_fold_scan_kernel): the folds of a unit's path, the palindrome arm around each, how the arms nest, and per junction its folds --
against a plain Python walk of the definitions over the ORACLE's paths (tests/fold_profile_checks.py).  Every check runs on the CPU
through the host simulation (the same stage code on the 1-thread group) and, marked gpu, through the HIP engine."""
import os
import subprocess

import pytest

import fold_profile_checks as fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (AMBI_FOLD_WINDOW, AMBI_JPROFILE_JUNC_WINDOW): one and three folds per round -- 67 and 23 rounds on the largest paths --, one and
# three junctions per pass of the scan stage
WINDOWS = [(1, None), (3, None), (None, 1), (None, 3), (3, 3)]


# ---- CPU: host simulation -------------------------------------------------------------------------------------------
def test_floors(hostsim_lib, oracle, workdir):
    """What the units must offer -- alignments -1, 0, 1, 2; arms in 1..7, in 8..63, of 63, of 64 and of 1024 or more; max_cover >= 5;
    a unit whose two paths differ -- asserted from the walk itself; then the same floors read from the engine's own planes."""
    fp.check_floors(oracle, workdir)
    fp.check_floors_served(hostsim_lib, oracle, workdir)


def test_readme_fold_profile(hostsim_lib, oracle, workdir):
    fp.check_readme(hostsim_lib, oracle, workdir)


def test_all_units_two_runs(hostsim_lib, oracle, workdir):
    fp.check_all_units(hostsim_lib, oracle, workdir)


@pytest.mark.parametrize("fwin,jwin", WINDOWS)
def test_all_units_windows(hostsim_lib, oracle, workdir, fwin, jwin):
    fp.check_all_units(hostsim_lib, oracle, workdir, fwin, jwin)


def test_each_unit_alone(hostsim_lib, oracle, workdir):
    fp.check_each_alone(hostsim_lib, oracle, workdir)


def test_request_paths(hostsim_lib, oracle, workdir):
    fp.check_request_paths(hostsim_lib, oracle, workdir)


def test_sharded_fold_profile(hostsim_lib, oracle, workdir):
    """After run_sharded the request goes to every share and the getters answer from the share that holds the unit."""
    fp.check_sharded(hostsim_lib, oracle, workdir, [0, 0, 0])


def test_cli_fold_profile(hostsim_lib, oracle, workdir, tmp_path):
    exe = os.path.join(ROOT, "tests", "hostsim", "Ambigram_hostsim")
    assert os.path.exists(exe)
    fp.check_cli(hostsim_lib, exe, str(tmp_path), oracle, workdir)


def test_errors(hostsim_lib):
    fp.check_errors(hostsim_lib)


def test_stage_check_under_asan_ubsan(tmp_path):
    """tests/tools/fold_profile_stage_check.cpp: both stages on the host group against a naive transcription over hand-built and
    random paths of {+-1 .. +-3} (P = 1 and 2, folds at step 0 and P - 2, arms that end at the first and the last cell, arms of
    7 / 8 / 9 and 63 / 64 / 65, every alignment alone, arm-less folds, alternating paths, fold windows of 1), every buffer a heap
    block of exactly its stated size, as a stand-alone program under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "fold_profile_stage_check")
    src = os.path.join(ROOT, "tests", "tools", "fold_profile_stage_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-Wall", "-Wno-sign-compare", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "ambigram_amd", "csrc"),
                        "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and "fold_profile_stage_check: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---- GPU: the HIP engine --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_readme_fold_profile(hip_lib, oracle, workdir):
    fp.check_readme(hip_lib, oracle, workdir)          # one unit: the express path


@pytest.mark.gpu
def test_gpu_all_units_two_runs(hip_lib, oracle, workdir):
    fp.check_all_units(hip_lib, oracle, workdir)


@pytest.mark.gpu
@pytest.mark.parametrize("fwin,jwin", WINDOWS)
def test_gpu_all_units_windows(hip_lib, oracle, workdir, fwin, jwin):
    fp.check_all_units(hip_lib, oracle, workdir, fwin, jwin)


@pytest.mark.gpu
def test_gpu_each_unit_alone(hip_lib, oracle, workdir):
    fp.check_each_alone(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_request_paths(hip_lib, oracle, workdir):
    """The run on one stream, every request on another."""
    import torch
    run_s, req_s = torch.cuda.Stream(), torch.cuda.Stream()
    fp.check_request_paths(hip_lib, oracle, workdir, run_s.cuda_stream, req_s.cuda_stream)


@pytest.mark.gpu
def test_gpu_sharded_fold_profile(hip_lib, oracle, workdir):
    fp.check_sharded(hip_lib, oracle, workdir, [0, 0])


@pytest.mark.gpu
def test_gpu_fold_device_views(hip_lib, oracle, workdir):
    fp.check_device_views(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_cli_fold_profile(hip_lib, oracle, workdir, tmp_path):
    exe = os.path.join(ROOT, "ambigram_amd", "bin", "Ambigram")
    assert os.path.exists(exe), "build the CLI first (__graft_entry__.build)"
    fp.check_cli(hip_lib, exe, str(tmp_path), oracle, workdir)


@pytest.mark.gpu
def test_gpu_errors(hip_lib):
    fp.check_errors(hip_lib)
