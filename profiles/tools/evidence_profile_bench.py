#!/usr/bin/env python3
"""Evidence depth profile against the fragment profile plus the junction profile: python3 profiles/tools/evidence_profile_bench.py [units=4096] [pairs=8] [frags=32] [max_len=40]

The bench batch and the fragments of profiles/tools/frag_profile_bench.py (synth: 256 segments, 512 junctions, wide K = 19, every 8th
unit with two deletions and a duplication; `frags` fragments per unit cut from the unit's own final path, every second one
reverse-complemented, every fourth one mutated in one cell).  Per round, in ONE process and interleaved: ambi_batch_evidence_profile,
ambi_batch_frag_profile and ambi_batch_junc_profile, which = 1, each between two HIP events on the caller's stream (the kernels and
the waits in front of them; the device-to-host copy of the block runs on the engine's copy stream and is outside the events), each
waited for before the next is queued.  The yardstick is the SUM of the other two: the evidence request does the matching of the
first and the probe of the second, plus a zero, a scan and one read per junction pass of a 4-byte array.
Prints one JSON line with the rounds, the three medians, the ratio against the sum, and the sizes."""
import json
import os
import random
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ambigram_amd import api, synth

n_units = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 8
n_frags = int(sys.argv[3]) if len(sys.argv) > 3 else 32
max_len = int(sys.argv[4]) if len(sys.argv) > 4 else 40
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

rng = random.Random(1)
frag_cells = 0
for u in range(n_units):
    path = b.unit_path(u, 1).tolist()
    P = len(path)
    frags = []
    for k in range(n_frags):
        L = rng.randint(2, min(max_len, P)); i = rng.randint(0, P - L)
        f = path[i:i + L]
        if k % 4 == 3:
            f[rng.randrange(L)] *= -1
        if k % 2:
            f = [-v for v in reversed(f)]
        frags.append(f); frag_cells += L
    b.set_unit_fragments(u, frags)

e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(queue, wait):
    with torch.cuda.stream(stream):
        e0.record(stream)
        queue(1, st)
        e1.record(stream)
    wait()
    e1.synchronize()
    return e0.elapsed_time(e1)


ep, fp, jp = [], [], []
for r in range(pairs + 2):
    x = timed(b.evidence_profile, b.evidence_profile_wait)
    a = timed(b.frag_profile, b.frag_profile_wait)
    c = timed(b.junc_profile, b.junc_profile_wait)
    if r >= 2:   # (two warm-up rounds: the fragment image and the offsets travel with the first request)
        ep.append(x); fp.append(a); jp.append(c)
summ = [b.unit_evidence_profile(u) for u in range(n_units)]
fsum = [b.unit_frag_profile(u) for u in range(n_units)]
_, ebytes = b.evidence_profile_device()
_, dbytes, _ = b.evidence_depth_device()
med = lambda v: float(np.median(v))
print(json.dumps(dict(device=torch.cuda.get_device_name(0), units=n_units, pairs=pairs, cells=int(cells), frags_per_unit=n_frags, max_len=max_len, frag_cells=int(frag_cells),
                      occurrences=int(sum(s["occurrences"] for s in fsum)), steps=int(sum(s["steps"] for s in summ)), steps_covered=int(sum(s["steps_covered"] for s in summ)),
                      depth_sum=int(sum(s["depth_sum"] for s in summ)), max_depth=int(max(s["max_depth"] for s in summ)),
                      juncs_used=int(sum(s["juncs_used"] for s in summ)), juncs_covered=int(sum(s["juncs_covered"] for s in summ)),
                      evidence_block_bytes=int(ebytes), depth_area_bytes=int(dbytes),
                      evidence_profile_ms=[round(v, 4) for v in ep], frag_profile_ms=[round(v, 4) for v in fp], junc_profile_ms=[round(v, 4) for v in jp],
                      evidence_profile_med_ms=med(ep), frag_profile_med_ms=med(fp), junc_profile_med_ms=med(jp),
                      ratio_to_sum=med(ep) / (med(fp) + med(jp)))))
