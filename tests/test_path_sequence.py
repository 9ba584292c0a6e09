"""Path sequences (ambi_batch_sequence: csrc/ambi_sequence.hpp, ambi_seq_extents_kernel, ambi_seq_fill_kernel): every unit's path as
nucleotides, against a plain concat / reverse complement of the ORACLE's paths (tests/sequence_checks.py).  Every check runs on the
CPU through the host simulation (the same stage code on the 1-thread group) and, marked gpu, through the HIP engine."""
import os
import subprocess

import numpy as np
import pytest

import sequence_checks as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM_EXE = os.path.join(ROOT, "tests", "hostsim", "Ambigram_hostsim")
HIP_EXE = os.path.join(ROOT, "ambigram_amd", "bin", "Ambigram")


# ---- CPU: host simulation -------------------------------------------------------------------------------------------
def test_readme_sequence(hostsim_lib, oracle):
    sc.check_readme(hostsim_lib, oracle)


def test_edge_units(hostsim_lib, oracle, workdir):
    sc.check_edge_units(hostsim_lib, oracle, workdir)


def test_many_units(hostsim_lib, oracle, workdir):
    sc.check_many_units(hostsim_lib, oracle, workdir)


def test_ranges_and_limit(hostsim_lib, oracle, workdir):
    sc.check_ranges_and_limit(hostsim_lib, oracle, workdir)


def test_state_errors(hostsim_lib):
    sc.check_state_errors(hostsim_lib)


def test_two_runs(hostsim_lib, oracle, workdir):
    sc.check_two_runs(hostsim_lib, oracle, workdir)


def test_big_unit_finished_at_wait(hostsim_lib, oracle, workdir):
    sc.check_big_unit_finished_at_wait(hostsim_lib, oracle, workdir)


def test_request_paths(hostsim_lib, oracle, workdir):
    sc.check_request_paths(hostsim_lib, oracle, workdir)


def test_three_requests_in_flight(hostsim_lib, oracle, workdir):
    sc.check_three_requests_in_flight(hostsim_lib, oracle, workdir)


def test_sharded_sequence(hostsim_lib, oracle, workdir):
    sc.check_sharded(hostsim_lib, oracle, workdir, [0, 0, 0])


def test_partial_bases(hostsim_lib, oracle):
    sc.check_partial_bases(hostsim_lib, oracle)
    sc.check_partial_bases(hostsim_lib, oracle, [0, 0])      # share 0 holds the units without bases


def test_fasta_reader(hostsim_lib, workdir):
    sc.check_fasta_reader(hostsim_lib, workdir)


def test_reconstruct_sample_sequence(hostsim_lib, oracle, workdir):
    """api.reconstruct_sample(ref_fasta=...) adds `sequence` per chromosome, only when asked for."""
    from ambigram_amd import api
    lh, fa, rec, segs = sc.fasta_case(workdir, "sample")
    e = api.reconstruct_sample(hostsim_lib, lh, [], ref_fasta=fa)
    o = oracle.run_bfb(lh, [])
    assert e["ok"] and len(e["chr"]) == 2
    bases = [rec[c][s:t] for c, s, t in segs]
    for oc, ec in zip(o["chr"], e["chr"]):
        n = oc["end"] - oc["start"] + 1
        assert ec["sequence"] == sc.want_of(oc, 1, bases[oc["start"] - 1:oc["start"] - 1 + n]) and len(ec["sequence"]) > 0
    assert "sequence" not in api.reconstruct_sample(hostsim_lib, lh, [])["chr"][0]


def test_cli_out_fasta(hostsim_lib, oracle, tmp_path):
    assert os.path.exists(HOSTSIM_EXE)
    sc.check_cli(hostsim_lib, HOSTSIM_EXE, str(tmp_path), oracle)


def test_stage_check_under_asan_ubsan(tmp_path):
    """tests/tools/sequence_stage_check.cpp: the extents and fill functions on the host group over hand-made blobs, every buffer of
    exactly its stated size, as a stand-alone program under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "sequence_stage_check")
    src = os.path.join(ROOT, "tests", "tools", "sequence_stage_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-Wall", "-Wno-sign-compare", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and "sequence_stage_check: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---- GPU: the HIP engine --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_readme_sequence(hip_lib, oracle):
    sc.check_readme(hip_lib, oracle)          # one unit: the express path


@pytest.mark.gpu
def test_gpu_edge_units(hip_lib, oracle, workdir):
    sc.check_edge_units(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_many_units(hip_lib, oracle, workdir):
    sc.check_many_units(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_ranges_and_limit(hip_lib, oracle, workdir):
    sc.check_ranges_and_limit(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_state_errors(hip_lib):
    sc.check_state_errors(hip_lib)


@pytest.mark.gpu
def test_gpu_two_runs(hip_lib, oracle, workdir):
    sc.check_two_runs(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_big_unit_finished_at_wait(hip_lib, oracle, workdir):
    sc.check_big_unit_finished_at_wait(hip_lib, oracle, workdir)


@pytest.mark.gpu
def test_gpu_request_paths(hip_lib, oracle, workdir):
    """The run on one stream, every request on another."""
    import torch
    run_s, req_s = torch.cuda.Stream(), torch.cuda.Stream()
    sc.check_request_paths(hip_lib, oracle, workdir, run_s.cuda_stream, req_s.cuda_stream)


@pytest.mark.gpu
def test_gpu_three_requests_in_flight(hip_lib, oracle, workdir):
    import torch
    run_s, req_s = torch.cuda.Stream(), torch.cuda.Stream()
    sc.check_three_requests_in_flight(hip_lib, oracle, workdir, run_s.cuda_stream, req_s.cuda_stream)


@pytest.mark.gpu
def test_gpu_sharded_sequence(hip_lib, oracle, workdir):
    sc.check_sharded(hip_lib, oracle, workdir, [0, 0])


@pytest.mark.gpu
def test_gpu_megabyte_unit(hip_lib, oracle):
    """readme6 with segments of 30-40 kB: about a megabyte of output from one unit, 270 tiles, long runs on both strands."""
    from ambigram_amd import api
    import cases
    lh, sol = os.path.join(cases.DATA, "readme6.lh"), os.path.join(cases.DATA, "readme6.sol")
    oc = oracle.run_bfb(lh, [sol])["chr"][0]
    segs = sc.draw_segments(np.random.default_rng(68), [30011, 33000, 35003, 40001, 31999, 32768])
    g = api.Graph(hip_lib, lh); sc.attach(g, segs)
    b = api.Batch(hip_lib)
    b.add_chromosome_sol(g, 0, sol)
    b.upload(); b.run(0)
    b.sequence(1); b.sequence_wait()
    want = sc.want_of(oc, 1, segs)
    assert len(want) > 1000000
    sc.compare_units(b, [want], "megabyte")
    b.close(); g.close()


@pytest.mark.gpu
def test_gpu_sequence_device_view(hip_lib, oracle, workdir):
    """ambi_batch_sequence_device: the block in device memory, read back through torch, holds every unit's sequence at the reported
    offset, zero bytes up to the next multiple of 16 and nothing else."""
    import torch
    from ambigram_amd.dist import _DevBytes
    items, records, seg_lists, _ = sc.many_sequences(oracle, workdir)
    graphs, b = sc.many_batch(hip_lib, items, seg_lists)
    stream = torch.cuda.Stream()
    b.upload(); b.run(0, stream.cuda_stream)
    b.sequence(1, 0, len(items), 0, stream.cuda_stream); b.sequence_wait()
    ptr, nbytes, off = b.sequence_device()
    assert ptr and nbytes > 0 and nbytes % 16 == 0
    raw = torch.as_tensor(_DevBytes(ptr, nbytes), device="cuda").cpu().numpy()
    at = 0
    for u, (oc, segs) in enumerate(zip(records, seg_lists)):
        n = b.unit_sequence_len(u)
        assert off[u] == at and off[u] % 16 == 0, u
        got = raw[at:at + n].tobytes()
        assert got == b.unit_sequence(u) == sc.want_of(oc, 1, segs), u
        pad = -n % 16
        assert not raw[at + n:at + n + pad].any(), u
        at += n + pad
    assert at == nbytes
    b.sequence(1, 5, 17); b.sequence_wait()
    _, _, off = b.sequence_device()
    assert off[4] == -1 and off[5] == 0 and off[22] == -1
    sc.pc.close_all(graphs, b)


@pytest.mark.gpu
def test_gpu_partial_bases(hip_lib, oracle):
    sc.check_partial_bases(hip_lib, oracle)
    sc.check_partial_bases(hip_lib, oracle, [0, 0])


@pytest.mark.gpu
def test_gpu_fasta_reader(hip_lib, workdir):
    sc.check_fasta_reader(hip_lib, workdir)


@pytest.mark.gpu
def test_gpu_cli_out_fasta(hip_lib, oracle, tmp_path):
    assert os.path.exists(HIP_EXE), "build the CLI first (__graft_entry__.build)"
    sc.check_cli(hip_lib, HIP_EXE, str(tmp_path), oracle)
