"""The plan stage past one chunk (tests/plan_checks.py): a batch of 4096 + 107 units under an arena limit of k granules must refuse
exactly the units k .. 4202, on the first run and on the resident one, and leave every other unit as it is without the limit.
  k = 1401: the boundary lies in the kernel's first chunk, the refusals run on through the second, `off_carry` continues past the arena;
  k = 4100: the boundary lies in the second chunk, where `off_carry` decides it and `blk_carry` places the rows of 4096 .. 4099.
Every check runs on the CPU through the host simulation (plan_serial, the serial form of the kernel) and, marked gpu, through the
HIP engine, where ambi_plan_kernel walks its two chunks."""
import pytest

import plan_checks as pc


# ---- CPU: host simulation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("granules", [1401, 4100])
def test_arena_boundary(hostsim_lib, workdir, granules):
    assert pc.check_arena_of(hostsim_lib, workdir, granules) == pc.N_UNITS - granules


# ---- GPU: the HIP engine --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("granules", [1401, 4100])
def test_gpu_arena_boundary(hip_lib, workdir, granules):
    assert pc.check_arena_of(hip_lib, workdir, granules) == pc.N_UNITS - granules
