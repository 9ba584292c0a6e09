"""The four on-request profiles at their window caps and under contention (tests/profile_fuzz_checks.py has the generators, the
floors and the checks): the copy-number profile, junction usage, fragment support and evidence depth against the plain Python walks
of their own *_checks.py modules, every array and every summary field exactly, both paths.

The CPU half runs every family on the host simulation (the same stage code on the 1-thread group) and asserts the floors -- what the
inputs must reach for the comparison to mean something, from the walks and the inputs alone.  The GPU half runs the same families
through libambigram_hip.so, the requests on a stream of their own, one test per family and profile kind so that a failure names its
kernel: there the capped windows (the largest group memory of each kernel), the racing atomic minima, the compare-and-swap chains,
the device-memory atomics of the depth area and the overflow found by racing claims run for the first time.
profiles/r23_notes.md has the floors as measured and the device-code mutations these tests were run against.
"""
import pytest

import profile_fuzz_checks as fz

OVERFLOW_KINDS = ("junction", "evidence")


# ---------------------------------------------------------------------------------------------
# CPU half: the host simulation
# ---------------------------------------------------------------------------------------------
def test_cap_floors():
    print("family A:", fz.cap_floors())


@pytest.mark.parametrize("kind", fz.KINDS)
def test_caps(hostsim_lib, oracle, workdir, kind):
    """Family A: every cap from both sides, no window variable set; alone and in one batch between six small units."""
    fz.check_caps(hostsim_lib, oracle, workdir, kind)


@pytest.mark.parametrize("kind", fz.KINDS)
def test_repeats(hostsim_lib, workdir, kind):
    """Family B: 3000 shuffled repeats of the unit's own junctions; the unit keeps its plain twin's status and paths (asserted)."""
    fz.check_repeats(hostsim_lib, hostsim_lib, workdir, kind)


def test_repeat_floors(hostsim_lib, workdir):
    fz.check_repeats(hostsim_lib, hostsim_lib, workdir, "junction")
    print("family B (unit, junctions, classes, used classes, of them won by a repeat):", fz.repeat_floors(hostsim_lib, workdir))


@pytest.mark.parametrize("kind", fz.KINDS)
def test_dense(hostsim_lib, oracle, workdir, kind):
    """Family C: dense substrings, 1500 fragments on one first step, palindromes."""
    fz.check_dense(hostsim_lib, oracle, workdir, kind)


def test_dense_floors(hostsim_lib, oracle, workdir):
    for kind in ("fragment", "evidence"):               # the two walks the floors read (shared with test_dense when it ran first)
        fz.check_dense(hostsim_lib, oracle, workdir, kind)
    print("family C:", fz.dense_floors(oracle, workdir))


def test_overflow_precondition():
    """Family D: more classes in one partition than the table has slots, in the first round and, for the second unit, in the second."""
    once, twice = fz.overflow_units()
    assert fz.overflow_rounds(once)[0] == fz.overflow_rounds(twice)[0] == 1000
    assert fz.fullest_partition(once, 1000) > fz.OVERFLOW_SLOTS and fz.fullest_partition(twice, 1000) > fz.OVERFLOW_SLOTS
    assert fz.fullest_partition(twice, 2000) > fz.OVERFLOW_SLOTS and fz.overflow_rounds(twice)[1] >= 2
    print("family D:", fz.overflow_rounds(once), fz.overflow_rounds(twice))


@pytest.mark.parametrize("kind", OVERFLOW_KINDS)
def test_overflow(hostsim_lib, kind):
    fz.check_overflow(hostsim_lib, kind)


# ---------------------------------------------------------------------------------------------
# GPU half: the HIP engine, the run on one stream and every request on another
# ---------------------------------------------------------------------------------------------
def _streams():
    import torch
    run_s, req_s = torch.cuda.Stream(), torch.cuda.Stream()
    return run_s, req_s


@pytest.mark.gpu
@pytest.mark.parametrize("kind", fz.KINDS)
def test_gpu_caps(hip_lib, oracle, workdir, kind):
    run_s, req_s = _streams()
    fz.check_caps(hip_lib, oracle, workdir, kind, run_s.cuda_stream, req_s.cuda_stream)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", fz.KINDS)
def test_gpu_repeats(hip_lib, hostsim_lib, workdir, kind):
    run_s, req_s = _streams()
    fz.check_repeats(hip_lib, hostsim_lib, workdir, kind, run_s.cuda_stream, req_s.cuda_stream)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", fz.KINDS)
def test_gpu_dense(hip_lib, oracle, workdir, kind):
    run_s, req_s = _streams()
    fz.check_dense(hip_lib, oracle, workdir, kind, run_s.cuda_stream, req_s.cuda_stream)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", OVERFLOW_KINDS)
def test_gpu_overflow(hip_lib, kind):
    run_s, req_s = _streams()
    fz.check_overflow(hip_lib, kind, run_s.cuda_stream, req_s.cuda_stream)
