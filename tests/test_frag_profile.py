"""Fragment support profile of the paths (ambi_batch_frag_profile: csrc/ambi_frag_profile.hpp, ambi_frag_profile_kernel): how often
a unit's path contains every fragment of its .juncs evidence, forward and reverse-complemented, and where first -- against a plain
Python walk over the ORACLE's paths (tests/frag_profile_checks.py).  Every check runs on the CPU through the host simulation (the
same stage code on the 1-thread group) and, marked gpu, through the HIP engine."""
import os
import subprocess

import numpy as np
import pytest

import frag_profile_checks as fc
import profile_checks as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = [1, 3, 64]      # AMBI_FPROFILE_FRAG_WINDOW: one pattern per window; f split from rc(f); a partial last window


# ---- CPU: host simulation -------------------------------------------------------------------------------------------
def test_readme_frag_profile(hostsim_lib, oracle):
    fc.check_readme(hostsim_lib, oracle)


def test_many_units_two_runs(hostsim_lib, oracle, workdir):
    fc.check_many_units(hostsim_lib, oracle, workdir)


@pytest.mark.parametrize("window", WINDOWS)
def test_many_units_windows(hostsim_lib, oracle, workdir, window):
    """About 20 fragments = 40 patterns per unit in 40 / 14 / 1 windows: equal to the one-window profile, which the expectation is."""
    fc.check_many_units(hostsim_lib, oracle, workdir, window=window)


def test_edge_units(hostsim_lib, oracle, workdir):
    fc.check_edge_units(hostsim_lib, oracle, workdir)


def test_raw_unit_wide_ids(hostsim_lib, workdir):
    fc.check_raw_unit(hostsim_lib, workdir)


def test_bench_unit(hostsim_lib, oracle, workdir):
    fc.check_bench_unit(hostsim_lib, oracle, workdir)


def test_big_unit_finished_at_wait(hostsim_lib, oracle, workdir):
    fc.check_big_unit_finished_at_wait(hostsim_lib, oracle, workdir)


def test_three_chromosomes(hostsim_lib, oracle, workdir):
    fc.check_three_chromosomes(hostsim_lib, oracle, workdir)


def test_sharded_frag_profile(hostsim_lib, oracle, workdir):
    """After run_sharded the request goes to every share and the getters answer from the share that holds the unit."""
    fc.check_sharded(hostsim_lib, oracle, workdir, [0, 0, 0])


def test_request_paths(hostsim_lib, oracle, workdir):
    fc.check_request_paths(hostsim_lib, oracle, workdir)


def test_cli_frag_profile(hostsim_lib, oracle, workdir, tmp_path):
    exe = os.path.join(ROOT, "tests", "hostsim", "Ambigram_hostsim")
    assert os.path.exists(exe)
    fc.check_cli(hostsim_lib, exe, str(tmp_path), oracle, workdir)


def test_errors(hostsim_lib):
    fc.check_errors(hostsim_lib)


def test_stage_check_under_asan_ubsan(tmp_path):
    """tests/tools/frag_profile_stage_check.cpp: the stage on the host group against a naive transcription over random paths of
    {+-1, +-2} (overlapping occurrences, periodic paths, long chains on one first step; P = 1, P = 2, F = 0, windows of 1, a table
    filled to its load limit), every buffer of exactly its stated size, as a stand-alone program under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "frag_profile_stage_check")
    src = os.path.join(ROOT, "tests", "tools", "frag_profile_stage_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-Wall", "-Wno-sign-compare", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "ambigram_amd", "csrc"),
                        "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and "frag_profile_stage_check: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---- GPU: the HIP engine --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_readme_frag_profile(hip_lib, oracle):
    fc.check_readme(hip_lib, oracle)          # one unit: the express path


@pytest.mark.gpu
def test_gpu_many_units_two_runs(hip_lib, oracle, workdir):
    fc.check_many_units(hip_lib, oracle, workdir)


@pytest.mark.gpu
@pytest.mark.parametrize("window", WINDOWS)
def test_gpu_many_units_windows(hip_lib, oracle, workdir, window):
    fc.check_many_units(hip_lib, oracle, workdir, window=window)


@pytest.mark.gpu
def test_gpu_edge_units(hip_lib, oracle, workdir):
    fc.check_edge_units(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_raw_unit_wide_ids(hip_lib, workdir):
    fc.check_raw_unit(hip_lib, workdir)


@pytest.mark.gpu
def test_gpu_bench_unit(hip_lib, oracle, workdir):
    fc.check_bench_unit(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_big_unit_finished_at_wait(hip_lib, oracle, workdir):
    fc.check_big_unit_finished_at_wait(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_three_chromosomes(hip_lib, oracle, workdir):
    fc.check_three_chromosomes(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_sharded_frag_profile(hip_lib, oracle, workdir):
    fc.check_sharded(hip_lib, oracle, workdir, [0, 0])


@pytest.mark.gpu
def test_gpu_request_paths(hip_lib, oracle, workdir):
    """The run on one stream, every request on another."""
    import torch
    run_s, req_s = torch.cuda.Stream(), torch.cuda.Stream()
    fc.check_request_paths(hip_lib, oracle, workdir, run_s.cuda_stream, req_s.cuda_stream)


@pytest.mark.gpu
def test_gpu_frag_profile_device_view(hip_lib, oracle, workdir):
    """ambi_batch_frag_profile_device: the block in device memory, read back through torch, is what the host getters return, byte
    for byte, and ends exactly at `bytes`."""
    import torch
    from ambigram_amd.dist import _DevBytes
    graphs, b, items = fc.many_items(hip_lib, oracle, workdir, 12)
    stream = torch.cuda.Stream()
    b.upload(); b.run(0, stream.cuda_stream)
    b.frag_profile(1, stream.cuda_stream); b.frag_profile_wait()
    ptr, nbytes = b.frag_profile_device()
    U = len(items)
    assert ptr and nbytes >= 40 * U
    raw = torch.as_tensor(_DevBytes(ptr, nbytes), device="cuda").cpu().numpy()
    off = (40 * U + 15) & ~15
    for u in range(U):
        p = b.unit_frag_profile(u)
        s = raw[40 * u:40 * u + 40]
        assert s[:32].view(np.int32).tolist() + s[32:].view(np.int64).tolist() == [p[k] for k in fc.FIELDS], u
        fwd, rev, first, _ = b.unit_frag_support(u)
        F = len(fwd)
        assert F == p["frags"] == len(items[u][0])
        for arr in (fwd, rev, first):
            assert raw[off:off + 4 * F].tobytes() == arr.tobytes(), u
            off += (4 * F + 15) & ~15
    assert off == nbytes
    pc.close_all(graphs, b)


@pytest.mark.gpu
def test_gpu_cli_frag_profile(hip_lib, oracle, workdir, tmp_path):
    exe = os.path.join(ROOT, "ambigram_amd", "bin", "Ambigram")
    assert os.path.exists(exe), "build the CLI first (__graft_entry__.build)"
    fc.check_cli(hip_lib, exe, str(tmp_path), oracle, workdir)


@pytest.mark.gpu
def test_gpu_errors(hip_lib):
    fc.check_errors(hip_lib)
