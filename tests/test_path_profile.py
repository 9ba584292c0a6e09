"""Copy-number profile of the paths (ambi_batch_profile: csrc/ambi_profile.hpp, ambi_path_profile_kernel): per-segment traversal
counts per strand and the per-unit summary, against plain numpy on the ORACLE's paths (tests/profile_checks.py).  Every check
runs on the CPU through the host simulation (the same stage code on the 1-thread group) and, marked gpu, through the HIP engine."""
import os
import subprocess
import sys

import numpy as np
import pytest

import profile_checks as pc
from ambigram_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU: host simulation -------------------------------------------------------------------------------------------
def test_readme_profile(hostsim_lib, oracle):
    pc.check_readme(hostsim_lib, oracle)


def test_edge_units(hostsim_lib, oracle, workdir):
    pc.check_edge_units(hostsim_lib, oracle, workdir)


def test_many_units_two_runs(hostsim_lib, oracle, workdir):
    pc.check_many_units(hostsim_lib, oracle, workdir)


@pytest.mark.parametrize("window", [16, 5])
def test_many_units_segment_windows(hostsim_lib, oracle, workdir, window):
    """48 segments in three / ten windows, the last one partial, runs straddling window edges: equal to the one-window profile."""
    pc.check_many_units(hostsim_lib, oracle, workdir, window=window)


def test_three_chromosomes(hostsim_lib, oracle, workdir):
    pc.check_three_chromosomes(hostsim_lib, oracle, workdir)


def test_big_unit_finished_at_wait(hostsim_lib, oracle, workdir):
    pc.check_big_unit_finished_at_wait(hostsim_lib, oracle, workdir)


def test_request_paths(hostsim_lib, oracle, workdir):
    pc.check_request_paths(hostsim_lib, oracle, workdir)


def test_errors(hostsim_lib):
    pc.check_errors(hostsim_lib)


def test_sharded_profile(hostsim_lib, oracle, workdir):
    """After run_sharded the profile goes to every share and the getters answer from the share that holds the unit."""
    _sharded(hostsim_lib, oracle, workdir, [0, 0, 0])


def test_cli_cn_profile(hostsim_lib, oracle, tmp_path):
    exe = os.path.join(ROOT, "tests", "hostsim", "Ambigram_hostsim")
    assert os.path.exists(exe)
    pc.check_cli(hostsim_lib, exe, str(tmp_path), oracle)


ASAN_CHILD = r"""
import sys, tempfile
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import profile_checks as pc
from ambigram_amd import api
from oracle import oracle_py
oracle_py.build(ref=False)
lib = api.load(%(lib)r)
with tempfile.TemporaryDirectory() as d:
    pc.check_many_units(lib, oracle_py, d)
    pc.check_many_units(lib, oracle_py, d, window=5)
print("SANITIZED RUN CLEAN")
"""


def test_profile_stage_under_asan_ubsan():
    """The profile stage under AddressSanitizer + UBSan through the host simulation, loaded the way tests/test_hostsim_asan.py does."""
    def runtime(name):
        p = subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
        return p if os.path.isabs(p) and os.path.exists(p) else None
    asan, ubsan = runtime("libasan.so"), runtime("libubsan.so")
    if not asan or not ubsan:
        pytest.skip("sanitizer runtimes not installed")
    hs = os.path.join(ROOT, "tests", "hostsim")
    r = subprocess.run(["make", "-s", "-C", hs, "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, LD_PRELOAD=asan + " " + ubsan, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    code = ASAN_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), lib=os.path.join(hs, "libambigram_hostsim_asan.so"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=os.path.join(ROOT, "tests"), timeout=900)
    assert r.returncode == 0 and "SANITIZED RUN CLEAN" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_stage_check_under_asan_ubsan(tmp_path):
    """tests/tools/path_profile_stage_check.cpp: the stage on the host group against a cell-by-cell transcription, and the chunked
    cell read the three profile stages share on its own (path lengths around the tile edges, the cells at every offset from an
    8-byte boundary, windows of 1 .. n + 1, single runs, single-cell runs, -n .. -1, a last run that ends at n, fold-back turns),
    every buffer of exactly its stated size, as a stand-alone program under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "path_profile_stage_check")
    src = os.path.join(ROOT, "tests", "tools", "path_profile_stage_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-Wall", "-Wno-sign-compare", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "ambigram_amd", "csrc"),
                        "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and "path_profile_stage_check: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def _sharded(lib, oracle, workdir, devices):
    items = pc.many_units(oracle, workdir)
    records = [oc for _, _, oc in items]
    graphs, b = pc.many_batch(lib, items)
    b.run_sharded(0, devices=devices)
    pc.check_batch(b, records, ("sharded", tuple(devices)))
    with pytest.raises(api.AmbiError):
        b.profile_device()               # one block per share: no single device view
    pc.close_all(graphs, b)


# ---- GPU: the HIP engine --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_readme_profile(hip_lib, oracle):
    pc.check_readme(hip_lib, oracle)          # one unit: the express path


@pytest.mark.gpu
def test_gpu_edge_units(hip_lib, oracle, workdir):
    pc.check_edge_units(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_many_units_two_runs(hip_lib, oracle, workdir):
    pc.check_many_units(hip_lib, oracle, workdir)


@pytest.mark.gpu
@pytest.mark.parametrize("window", [16, 5])
def test_gpu_many_units_segment_windows(hip_lib, oracle, workdir, window):
    pc.check_many_units(hip_lib, oracle, workdir, window=window)


@pytest.mark.gpu
def test_gpu_three_chromosomes(hip_lib, oracle, workdir):
    pc.check_three_chromosomes(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_big_unit_finished_at_wait(hip_lib, oracle, workdir):
    pc.check_big_unit_finished_at_wait(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_request_paths(hip_lib, oracle, workdir):
    """The run on one stream, every request on another."""
    import torch
    run_s, req_s = torch.cuda.Stream(), torch.cuda.Stream()
    pc.check_request_paths(hip_lib, oracle, workdir, run_s.cuda_stream, req_s.cuda_stream)


@pytest.mark.gpu
def test_gpu_errors(hip_lib):
    pc.check_errors(hip_lib)


@pytest.mark.gpu
def test_gpu_sharded_profile(hip_lib, oracle, workdir):
    _sharded(hip_lib, oracle, workdir, [0, 0])


@pytest.mark.gpu
def test_gpu_profile_device_view(hip_lib, oracle, workdir):
    """ambi_batch_profile_device: the block in device memory, read back through torch, is what the host getters return."""
    import torch
    from ambigram_amd.dist import _DevBytes
    items = pc.many_units(oracle, workdir)
    graphs, b = pc.many_batch(hip_lib, items)
    stream = torch.cuda.Stream()
    b.upload(); b.run(0, stream.cuda_stream)
    b.profile(1, stream.cuda_stream); b.profile_wait()
    ptr, nbytes = b.profile_device()
    U = len(items)
    assert ptr and nbytes >= 40 * U
    raw = torch.as_tensor(_DevBytes(ptr, nbytes), device="cuda").cpu().numpy()
    summ = raw[:40 * U].view(np.int32).reshape(U, 10)
    off = (40 * U + 15) & ~15
    for u, (_, _, oc) in enumerate(items):
        n = oc["end"] - oc["start"] + 1
        p = b.unit_profile(u)
        assert summ[u, :8].tolist() == [p[k] for k in ("status", "cells", "runs", "turns", "max_cn", "n_uncovered", "n_off_target", "n_off_input")], u
        assert int(summ[u, 8:10].view(np.int64)[0]) == p["l1_target"], u
        stride = (4 * (n + 1) + 15) & ~15
        fwd, rev = b.unit_path_cn(u, n)
        assert raw[off:off + 4 * (n + 1)].view(np.int32).tolist() == fwd.tolist(), u
        assert raw[off + stride:off + stride + 4 * (n + 1)].view(np.int32).tolist() == rev.tolist(), u
        assert p["cells"] == len(oc["path_indel"]), u
        off += 2 * stride
    assert off == nbytes
    pc.close_all(graphs, b)


@pytest.mark.gpu
def test_gpu_cli_cn_profile(hip_lib, oracle, tmp_path):
    exe = os.path.join(ROOT, "ambigram_amd", "bin", "Ambigram")
    assert os.path.exists(exe), "build the CLI first (__graft_entry__.build)"
    pc.check_cli(hip_lib, exe, str(tmp_path), oracle)
