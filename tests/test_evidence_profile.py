"""Evidence depth profile of the paths (ambi_batch_evidence_profile: csrc/ambi_evidence_profile.hpp, ambi_evidence_mark_kernel and
ambi_evidence_scan_kernel): how many fragment occurrences lie over every step of a unit's path, and per junction how many of its
traversals are covered -- against a plain Python walk over the ORACLE's paths (tests/evidence_profile_checks.py).  Every check runs
on the CPU through the host simulation (the same stage code on the 1-thread group) and, marked gpu, through the HIP engine."""
import os
import subprocess

import numpy as np
import pytest

import evidence_profile_checks as ec
import profile_checks as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (AMBI_FPROFILE_FRAG_WINDOW, AMBI_JPROFILE_JUNC_WINDOW, AMBI_JPROFILE_SEG_WINDOW): one pattern per window, f split from rc(f); the
# junction profile test's small windows.  The junction window sends the scan stage through several key partitions.  The segment
# window is set beside it as in that test, but the scan stage probes every step and has no segment array, so it has nothing to
# shrink here: these cases exercise the junction window alone.
WINDOWS = [(1, None, None), (3, None, None), (None, 32, 16), (None, 7, 5), (3, 7, 5)]


# ---- CPU: host simulation -------------------------------------------------------------------------------------------
def test_readme_evidence_profile(hostsim_lib, oracle):
    ec.check_readme(hostsim_lib, oracle)


def test_many_units_two_runs(hostsim_lib, oracle, workdir):
    ec.check_many_units(hostsim_lib, oracle, workdir)


@pytest.mark.parametrize("fwin,jwin,swin", WINDOWS)
def test_many_units_windows(hostsim_lib, oracle, workdir, fwin, jwin, swin):
    """24 patterns and about 100 junctions per unit in several windows and partitions: equal to the one-window profile, which the
    expectation is."""
    ec.check_many_units(hostsim_lib, oracle, workdir, fwin, jwin, swin)


def test_repeated_requests(hostsim_lib, oracle, workdir):
    ec.check_repeated_requests(hostsim_lib, oracle, workdir)


def test_identities(hostsim_lib, oracle, workdir):
    ec.check_identities(hostsim_lib, oracle, workdir)


def test_edge_units(hostsim_lib, oracle, workdir):
    ec.check_edge_units(hostsim_lib, oracle, workdir)


def test_bench_unit(hostsim_lib, oracle, workdir):
    ec.check_bench_unit(hostsim_lib, oracle, workdir)


def test_big_unit_finished_at_wait(hostsim_lib, oracle, workdir):
    ec.check_big_unit_finished_at_wait(hostsim_lib, oracle, workdir)


def test_request_paths(hostsim_lib, oracle, workdir):
    ec.check_request_paths(hostsim_lib, oracle, workdir)


def test_two_request_streams(hostsim_lib, oracle):
    """The request logic of the fragment and the evidence request side by side (the host simulation has no streams)."""
    ec.check_two_request_streams(hostsim_lib, oracle)


def test_sharded_evidence_profile(hostsim_lib, oracle, workdir):
    """After run_sharded the request goes to every share and the getters answer from the share that holds the unit."""
    ec.check_sharded(hostsim_lib, oracle, workdir, [0, 0, 0])


def test_cli_evidence_profile(hostsim_lib, oracle, workdir, tmp_path):
    exe = os.path.join(ROOT, "tests", "hostsim", "Ambigram_hostsim")
    assert os.path.exists(exe)
    ec.check_cli(hostsim_lib, exe, str(tmp_path), oracle, workdir)


def test_errors(hostsim_lib):
    ec.check_errors(hostsim_lib)


def test_stage_check_under_asan_ubsan(tmp_path):
    """tests/tools/evidence_profile_stage_check.cpp: both stages on the host group against a naive transcription over random periodic
    paths of {+-1, +-2} full of overlapping occurrences (P = 1, 2, 3, 8, 9, 2048, 2049; F = 0; windows of 1), every buffer a heap
    block of exactly its stated size, and the predicate of the 2^31 depth bound, as a stand-alone program under AddressSanitizer +
    UBSan."""
    exe = str(tmp_path / "evidence_profile_stage_check")
    src = os.path.join(ROOT, "tests", "tools", "evidence_profile_stage_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-Wall", "-Wno-sign-compare", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "ambigram_amd", "csrc"),
                        "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and "evidence_profile_stage_check: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---- GPU: the HIP engine --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_readme_evidence_profile(hip_lib, oracle):
    ec.check_readme(hip_lib, oracle)          # one unit: the express path


@pytest.mark.gpu
def test_gpu_many_units_two_runs(hip_lib, oracle, workdir):
    ec.check_many_units(hip_lib, oracle, workdir)


@pytest.mark.gpu
@pytest.mark.parametrize("fwin,jwin,swin", WINDOWS)
def test_gpu_many_units_windows(hip_lib, oracle, workdir, fwin, jwin, swin):
    ec.check_many_units(hip_lib, oracle, workdir, fwin, jwin, swin)


@pytest.mark.gpu
def test_gpu_repeated_requests(hip_lib, oracle, workdir):
    ec.check_repeated_requests(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_identities(hip_lib, oracle, workdir):
    ec.check_identities(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_edge_units(hip_lib, oracle, workdir):
    ec.check_edge_units(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_bench_unit(hip_lib, oracle, workdir):
    ec.check_bench_unit(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_big_unit_finished_at_wait(hip_lib, oracle, workdir):
    ec.check_big_unit_finished_at_wait(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_request_paths(hip_lib, oracle, workdir):
    """The run on one stream, every request on another."""
    import torch
    run_s, req_s = torch.cuda.Stream(), torch.cuda.Stream()
    ec.check_request_paths(hip_lib, oracle, workdir, run_s.cuda_stream, req_s.cuda_stream)


@pytest.mark.gpu
def test_gpu_two_request_streams(hip_lib, oracle):
    """The run, the fragment request and the evidence request on three streams, the image going up with either request: the request
    logic and the new layout behind a moved version.  The image is a few hundred bytes and arrives long before the other stream's
    kernel starts, so a missing wait for its upload would not show here; that ordering is read in DeviceImage::upload."""
    import torch
    run_s, frag_s, ev_s = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    ec.check_two_request_streams(hip_lib, oracle, run_s.cuda_stream, frag_s.cuda_stream, ev_s.cuda_stream)


@pytest.mark.gpu
def test_gpu_sharded_evidence_profile(hip_lib, oracle, workdir):
    ec.check_sharded(hip_lib, oracle, workdir, [0, 0])


@pytest.mark.gpu
def test_gpu_evidence_device_views(hip_lib, oracle, workdir):
    """ambi_batch_evidence_profile_device / ambi_batch_evidence_depth_device: both blocks in device memory, read back through torch,
    are what the host getters return, byte for byte; the profile block ends exactly at `bytes`; every unit_off is a multiple of 16."""
    import torch
    from ambigram_amd.dist import _DevBytes
    graphs, b, items = ec.many_items(hip_lib, oracle, workdir, 12)
    stream = torch.cuda.Stream()
    b.upload(); b.run(0, stream.cuda_stream)
    b.evidence_profile(1, stream.cuda_stream); b.evidence_profile_wait()
    ptr, nbytes = b.evidence_profile_device()
    U = len(items)
    assert ptr and nbytes >= 56 * U
    raw = torch.as_tensor(_DevBytes(ptr, nbytes), device="cuda").cpu().numpy()
    dptr, dbytes, doff = b.evidence_depth_device()
    assert dptr and dbytes > 0 and all(int(o) % 16 == 0 and 0 <= int(o) < dbytes for o in doff) and sorted(doff.tolist()) == doff.tolist()
    draw = torch.as_tensor(_DevBytes(dptr, dbytes), device="cuda").cpu().numpy()
    off = (56 * U + 15) & ~15
    for u in range(U):
        p = b.unit_evidence_profile(u)
        s = raw[56 * u:56 * u + 56]
        assert s[:48].view(np.int32).tolist() + s[48:].view(np.int64).tolist() == [p[k] for k in ec.FIELDS], u
        count, covered, mind, _ = b.unit_evidence_juncs(u)
        m = len(count)
        assert m == p["juncs"]
        for arr in (count, covered, mind):
            assert raw[off:off + 4 * m].tobytes() == arr.tobytes(), u
            off += (4 * m + 15) & ~15
        depth = b.unit_evidence_depth(u)
        assert len(depth) == p["steps"] and draw[int(doff[u]):int(doff[u]) + 4 * len(depth)].tobytes() == depth.tobytes(), u
        assert int(doff[u]) + 4 * len(depth) <= (int(doff[u + 1]) if u + 1 < U else dbytes), u
    assert off == nbytes
    pc.close_all(graphs, b)


@pytest.mark.gpu
def test_gpu_cli_evidence_profile(hip_lib, oracle, workdir, tmp_path):
    exe = os.path.join(ROOT, "ambigram_amd", "bin", "Ambigram")
    assert os.path.exists(exe), "build the CLI first (__graft_entry__.build)"
    ec.check_cli(hip_lib, exe, str(tmp_path), oracle, workdir)


@pytest.mark.gpu
def test_gpu_errors(hip_lib):
    ec.check_errors(hip_lib)
