#!/usr/bin/env python3
"""Fold-back arm profile against the evidence profile and the junction profile: python3 profiles/tools/fold_profile_bench.py [units=4096] [pairs=8] [frags=32] [max_len=40]

The bench batch and the fragments of profiles/tools/evidence_profile_bench.py (synth: 256 segments, 512 junctions, wide K = 19, every
8th unit with two deletions and a duplication; `frags` fragments per unit cut from the unit's own final path, for the evidence
request).  Per round, in ONE process and interleaved: ambi_batch_fold_profile, ambi_batch_evidence_profile and
ambi_batch_junc_profile, which = 1, each between two HIP events on the caller's stream (the kernels and the waits in front of them;
the device-to-host copy of the block runs on the engine's copy stream and is outside the events), each waited for before the next
is queued.  The yardstick is the evidence request: the fold request reads every cell once and about 2 x sum-of-arms cells more,
issues two atomics per fold where the evidence mark issues two per occurrence, and probes the folds where the evidence scan
probes every step.
Prints one JSON line with the rounds, the three medians, the ratio against the evidence request, and the sizes."""
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
        frags.append(f)
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


fo, ep, jp = [], [], []
for r in range(pairs + 2):
    x = timed(b.fold_profile, b.fold_profile_wait)
    a = timed(b.evidence_profile, b.evidence_profile_wait)
    c = timed(b.junc_profile, b.junc_profile_wait)
    if r >= 2:   # (two warm-up rounds: the planes, the fragment image and the offsets travel with the first request)
        fo.append(x); ep.append(a); jp.append(c)
summ = [b.unit_fold_profile(u) for u in range(n_units)]
_, fbytes = b.fold_profile_device()
_, pbytes, _ = b.fold_planes_device()
med = lambda v: float(np.median(v))
print(json.dumps(dict(device=torch.cuda.get_device_name(0), units=n_units, pairs=pairs, cells=int(cells), frags_per_unit=n_frags, max_len=max_len,
                      steps=int(sum(s["steps"] for s in summ)), folds=int(sum(s["folds"] for s in summ)), folds_perfect=int(sum(s["folds_perfect"] for s in summ)),
                      folds_gapped=int(sum(s["folds_gapped"] for s in summ)), folds_open=int(sum(s["folds_open"] for s in summ)),
                      arm_sum=int(sum(s["arm_sum"] for s in summ)), max_arm=int(max(s["max_arm"] for s in summ)), max_cover=int(max(s["max_cover"] for s in summ)),
                      fold_block_bytes=int(fbytes), plane_area_bytes=int(pbytes),
                      fold_profile_ms=[round(v, 4) for v in fo], evidence_profile_ms=[round(v, 4) for v in ep], junc_profile_ms=[round(v, 4) for v in jp],
                      fold_profile_med_ms=med(fo), evidence_profile_med_ms=med(ep), junc_profile_med_ms=med(jp),
                      ratio_to_evidence=med(fo) / med(ep), ratio_to_junction=med(fo) / med(jp))))
