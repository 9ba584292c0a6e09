#!/usr/bin/env python3
"""Junction usage profile against the copy-number profile: python3 profiles/tools/junc_profile_bench.py [units=4096] [pairs=8]

The bench batch (synth: 256 segments, 512 junctions, wide K = 19, every 8th unit with two deletions and a duplication: bench.py's
seeds), after one run.  Per pair, in ONE process and interleaved: ambi_batch_junc_profile and ambi_batch_profile, which = 1, each
between two HIP events on the caller's stream (the kernel and the waits in front of it; the device-to-host copy of the block runs
on the engine's copy stream and is outside the events), each waited for before the next is queued.  The copy-number profile is
the yardstick: ambi_junc_profile_kernel reads the same cells and adds, per unit, the build of a table of m classes and n probes.
Prints one JSON line with the pairs, both medians, the ratio and the sizes."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ambigram_amd import api, synth

n_units = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 8
assert pairs >= 5
lib = api.load(); lib.ambi_set_device(0); torch.cuda.set_device(0)

tmp = tempfile.mkdtemp(); b = api.Batch(lib); keep = []
for i in range(n_units):
    edits = i % 8 == 7
    s = synth.make_sample(256, 512, "wide", 19, seed=2000 + i, n_del=2 if edits else 0, n_dup=1 if edits else 0)
    lh, sols = s.write(tmp, "j%d" % i)
    g = api.Graph(lib, lh); keep.append(g)
    b.add_chromosome_sol(g, 0, sols[0])
stream = torch.cuda.Stream(); st = stream.cuda_stream
b.upload(); b.run(0, st); b.wait(); b.download()
res = [b.unit_result(u) for u in range(n_units)]
assert all(r["status"] == 0 for r in res)
cells = sum(r["path_indel_len"] for r in res)

e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(queue, wait):
    with torch.cuda.stream(stream):
        e0.record(stream)
        queue(1, st)
        e1.record(stream)
    wait()
    e1.synchronize()
    return e0.elapsed_time(e1)


jp, cp = [], []
for r in range(pairs + 2):
    a = timed(b.junc_profile, b.junc_profile_wait)
    c = timed(b.profile, b.profile_wait)
    if r >= 2:   # (two warm-up pairs: the offsets travel with the first request)
        jp.append(a); cp.append(c)
summ = [b.unit_junc_profile(u) for u in range(n_units)]
_, jbytes = b.junc_profile_device()
_, pbytes = b.profile_device()
med = lambda v: float(np.median(v))
print(json.dumps(dict(device=torch.cuda.get_device_name(0), units=n_units, pairs=pairs, cells=int(cells), juncs=int(sum(s["juncs"] for s in summ)),
                      steps_unmatched=int(sum(s["steps_unmatched"] for s in summ)), junc_block_bytes=int(jbytes), profile_block_bytes=int(pbytes),
                      junc_profile_ms=[round(x, 4) for x in jp], profile_ms=[round(x, 4) for x in cp], junc_profile_med_ms=med(jp), profile_med_ms=med(cp),
                      ratio=med(jp) / med(cp), junc_profile_GBps=2 * cells / med(jp) / 1e6)))
