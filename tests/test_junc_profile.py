"""Junction usage profile of the paths (ambi_batch_junc_profile: csrc/ambi_junc_profile.hpp, ambi_junc_profile_kernel): per-junction
traversal counts and the per-unit summary, against a plain Python walk over the ORACLE's paths and the .lh's JUNC lines
(tests/junc_profile_checks.py).  Every check runs on the CPU through the host simulation (the same stage code on the 1-thread
group) and, marked gpu, through the HIP engine."""
import os
import subprocess

import numpy as np
import pytest

import junc_profile_checks as jc
import profile_checks as pc
from ambigram_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = [(32, None), (7, None), (None, 16), (None, 5), (32, 16), (7, 5)]      # (AMBI_JPROFILE_JUNC_WINDOW, AMBI_JPROFILE_SEG_WINDOW)


# ---- CPU: host simulation -------------------------------------------------------------------------------------------
def test_readme_junc_profile(hostsim_lib, oracle):
    jc.check_readme(hostsim_lib, oracle)


def test_edge_units(hostsim_lib, oracle, workdir):
    jc.check_edge_units(hostsim_lib, oracle, workdir)


def test_many_units_two_runs(hostsim_lib, oracle, workdir):
    jc.check_many_units(hostsim_lib, oracle, workdir)


@pytest.mark.parametrize("jwin,swin", WINDOWS)
def test_many_units_windows(hostsim_lib, oracle, workdir, jwin, swin):
    """100 junctions in 4 / 15 passes over the key space, 48 segments in three / ten windows, the last one partial, runs straddling
    window edges: equal to the one-window profile."""
    jc.check_many_units(hostsim_lib, oracle, workdir, jwin=jwin, swin=swin)


def test_raw_units(hostsim_lib, workdir):
    jc.check_raw_units(hostsim_lib, workdir)


@pytest.mark.parametrize("jwin,swin", [(7, 5)])
def test_raw_units_windows(hostsim_lib, workdir, jwin, swin):
    """Duplicates and a missing adjacency with several passes: the winner of a class and its losers meet in one partition."""
    with jc._Env(jwin, swin):
        jc.check_raw_units(hostsim_lib, workdir)


def test_bench_unit(hostsim_lib, oracle, workdir):
    jc.check_bench_unit(hostsim_lib, oracle, workdir)


def test_three_chromosomes(hostsim_lib, oracle, workdir):
    jc.check_three_chromosomes(hostsim_lib, oracle, workdir)


def test_big_unit_finished_at_wait(hostsim_lib, oracle, workdir):
    jc.check_big_unit_finished_at_wait(hostsim_lib, oracle, workdir)


def test_sharded_junc_profile(hostsim_lib, oracle, workdir):
    """After run_sharded the request goes to every share and the getters answer from the share that holds the unit."""
    jc.check_sharded(hostsim_lib, oracle, workdir, [0, 0, 0])


def test_cli_junc_profile(hostsim_lib, oracle, workdir, tmp_path):
    exe = os.path.join(ROOT, "tests", "hostsim", "Ambigram_hostsim")
    assert os.path.exists(exe)
    jc.check_cli(hostsim_lib, exe, str(tmp_path), oracle, workdir)


def test_request_paths(hostsim_lib, oracle, workdir):
    jc.check_request_paths(hostsim_lib, oracle, workdir)


def test_errors(hostsim_lib):
    jc.check_errors(hostsim_lib)


def test_stage_check_under_asan_ubsan(tmp_path):
    """tests/tools/junc_profile_stage_check.cpp: the stage on the host group against a std::map transcription over random paths and
    junction lists (m = 0, P = 1, duplicate edges, windows of size 1, tables filled to their capacity), every buffer of exactly its
    stated size, as a stand-alone program under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "junc_profile_stage_check")
    src = os.path.join(ROOT, "tests", "tools", "junc_profile_stage_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-Wall", "-Wno-sign-compare", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "ambigram_amd", "csrc"),
                        "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and "junc_profile_stage_check: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---- GPU: the HIP engine --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_readme_junc_profile(hip_lib, oracle):
    jc.check_readme(hip_lib, oracle)          # one unit: the express path


@pytest.mark.gpu
def test_gpu_edge_units(hip_lib, oracle, workdir):
    jc.check_edge_units(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_many_units_two_runs(hip_lib, oracle, workdir):
    jc.check_many_units(hip_lib, oracle, workdir)


@pytest.mark.gpu
@pytest.mark.parametrize("jwin,swin", WINDOWS)
def test_gpu_many_units_windows(hip_lib, oracle, workdir, jwin, swin):
    jc.check_many_units(hip_lib, oracle, workdir, jwin=jwin, swin=swin)


@pytest.mark.gpu
def test_gpu_raw_units(hip_lib, workdir):
    jc.check_raw_units(hip_lib, workdir)


@pytest.mark.gpu
@pytest.mark.parametrize("jwin,swin", [(7, 5)])
def test_gpu_raw_units_windows(hip_lib, workdir, jwin, swin):
    with jc._Env(jwin, swin):
        jc.check_raw_units(hip_lib, workdir)


@pytest.mark.gpu
def test_gpu_bench_unit(hip_lib, oracle, workdir):
    jc.check_bench_unit(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_three_chromosomes(hip_lib, oracle, workdir):
    jc.check_three_chromosomes(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_big_unit_finished_at_wait(hip_lib, oracle, workdir):
    jc.check_big_unit_finished_at_wait(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_sharded_junc_profile(hip_lib, oracle, workdir):
    jc.check_sharded(hip_lib, oracle, workdir, [0, 0])


@pytest.mark.gpu
def test_gpu_junc_profile_device_view(hip_lib, oracle, workdir):
    """ambi_batch_junc_profile_device: the block in device memory, read back through torch, is what the host getters return, byte
    for byte, and ends exactly at `bytes`."""
    import torch
    from ambigram_amd.dist import _DevBytes
    graphs, b, items = jc.many_items(hip_lib, oracle, workdir)
    stream = torch.cuda.Stream()
    b.upload(); b.run(0, stream.cuda_stream)
    b.junc_profile(1, stream.cuda_stream); b.junc_profile_wait()
    ptr, nbytes = b.junc_profile_device()
    U = len(items)
    assert ptr and nbytes >= 40 * U
    raw = torch.as_tensor(_DevBytes(ptr, nbytes), device="cuda").cpu().numpy()
    summ = raw[:40 * U].view(np.int32).reshape(U, 10)
    off = (40 * U + 15) & ~15
    for u in range(U):
        p = b.unit_junc_profile(u)
        assert summ[u].tolist() == [p[k] for k in jc.FIELDS], u
        count, _ = b.unit_junc_usage(u)
        m = len(count)
        assert m == p["juncs"] and raw[off:off + 4 * m].tobytes() == count.tobytes(), u
        off += (4 * m + 15) & ~15
    assert off == nbytes
    pc.close_all(graphs, b)


@pytest.mark.gpu
def test_gpu_cli_junc_profile(hip_lib, oracle, workdir, tmp_path):
    exe = os.path.join(ROOT, "ambigram_amd", "bin", "Ambigram")
    assert os.path.exists(exe), "build the CLI first (__graft_entry__.build)"
    jc.check_cli(hip_lib, exe, str(tmp_path), oracle, workdir)


@pytest.mark.gpu
def test_gpu_request_paths(hip_lib, oracle, workdir):
    """The run on one stream, every request on another."""
    import torch
    run_s, req_s = torch.cuda.Stream(), torch.cuda.Stream()
    jc.check_request_paths(hip_lib, oracle, workdir, run_s.cuda_stream, req_s.cuda_stream)


@pytest.mark.gpu
def test_gpu_errors(hip_lib):
    jc.check_errors(hip_lib)
