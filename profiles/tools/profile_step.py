#!/usr/bin/env python3
"""Cost of the copy-number profile (ambi_batch_profile) on the bench batch: 4096 synthetic 256-segment units, wide tier, K = 19,
every 8th with deletions / a duplication -- the batch of bench.py, built the same way.

    python3 profiles/tools/profile_step.py [batch] [steps]

Prints one JSON line:
  kernel_ms            ambi_path_profile_kernel alone: HIP events on the stream around ambi_batch_profile with the batch idle
                       (the device-to-host copy of the block runs on the engine's copy stream, outside the events); median of `steps`
  plain_ms_per_step    `steps` runs back to back, one wait at the end (the headline loop of bench.py)
  profiled_ms_per_step the same with profile(1) queued behind every run; profile_wait after the last one
  bytes_read / bytes_written per profile: 2 P cells + 12 (n + 1) of target_cn and seg_cn per unit; 8 (n + 1) + 40 per unit
"""
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    import torch
    from ambigram_amd import api, synth
    torch.cuda.set_device(0)
    lib = api.load()
    lib.ambi_set_device(0)
    tmp = tempfile.mkdtemp(prefix="ambi_prof_")
    graphs, batch = [], api.Batch(lib)
    for i in range(B):
        edits = i % 8 == 7
        s = synth.make_sample(256, 512, "wide", 19, seed=2000 + i, n_del=2 if edits else 0, n_dup=1 if edits else 0)
        lh, sols = s.write(tmp, "s%d" % i)
        g = api.Graph(lib, lh); graphs.append(g)
        batch.add_chromosome_sol(g, 0, sols[0])
    shutil.rmtree(tmp, True)
    batch.upload()
    stream = torch.cuda.current_stream().cuda_stream
    batch.run(0, stream); batch.wait(); batch.download()
    res = [batch.unit_result(u) for u in range(B)]
    assert all(r["status"] == 0 for r in res)
    cells = sum(r["path_indel_len"] for r in res)
    for _ in range(3):
        batch.run(0, stream)
    batch.profile(1, stream); batch.profile_wait(); torch.cuda.synchronize()
    assert sum(batch.unit_profile(u)["cells"] for u in range(B)) == cells

    def loop(with_profile):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            batch.run(0, stream)
            if with_profile:
                batch.profile(1, stream)
        batch.wait()
        if with_profile:
            batch.profile_wait()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    plain, profiled = [], []
    for _ in range(3):                       # interleaved: the two loops see the same box at the same time
        plain.append(loop(False)); profiled.append(loop(True))
    kernel = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); batch.profile(1, stream); b.record()
        batch.profile_wait(); torch.cuda.synchronize()
        kernel.append(a.elapsed_time(b))
    kernel.sort()
    n = 256
    print(json.dumps({"batch": B, "steps": steps, "cells": cells, "kernel_ms": kernel[len(kernel) // 2], "kernel_ms_min": kernel[0],
                      "plain_ms_per_step": plain, "profiled_ms_per_step": profiled,
                      "bytes_read": 2 * cells + 12 * (n + 1) * B, "bytes_written": (8 * (n + 1) + 40) * B,
                      "read_GBps_at_kernel_ms": (2 * cells + 12 * (n + 1) * B) / (kernel[len(kernel) // 2] * 1e-3) / 1e9}))
    batch.close()


if __name__ == "__main__":
    main()
