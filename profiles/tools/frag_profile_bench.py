#!/usr/bin/env python3
"""Fragment support profile against the junction usage profile: python3 profiles/tools/frag_profile_bench.py [units=4096] [pairs=8] [frags=32] [max_len=40]

The bench batch (synth: 256 segments, 512 junctions, wide K = 19, every 8th unit with two deletions and a duplication: bench.py's
seeds), after one run, with `frags` fragments per unit cut from the unit's own final path (L = 2 .. max_len at random positions, every
second one reverse-complemented, every fourth one mutated in one cell) and attached with ambi_batch_set_unit_fragments.  Per pair,
in ONE process and interleaved: ambi_batch_frag_profile and ambi_batch_junc_profile, which = 1, each between two HIP events on the
caller's stream (the kernel and the waits in front of it; the device-to-host copy of the block runs on the engine's copy stream
and is outside the events), each waited for before the next is queued.  The junction profile is the yardstick: it reads the same
cells once and probes a table per boundary step; ambi_frag_profile_kernel probes at EVERY step and walks a chain on a hit.
Prints one JSON line with the pairs, both medians, the ratio, the bytes read and the passes taken."""
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
max_len = int(sys.argv[4]) if len(sys.argv) > 4 else 40      # 2: no cell is compared behind the first step -- the probes and the chain walks alone
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


fp, jp = [], []
for r in range(pairs + 2):
    a = timed(b.frag_profile, b.frag_profile_wait)
    c = timed(b.junc_profile, b.junc_profile_wait)
    if r >= 2:   # (two warm-up pairs: the fragment image and the offsets travel with the first request)
        fp.append(a); jp.append(c)
summ = [b.unit_frag_profile(u) for u in range(n_units)]
_, fbytes = b.frag_profile_device()
_, jbytes = b.junc_profile_device()
window = min(2048, 2 * n_frags)
env = os.environ.get("AMBI_FPROFILE_FRAG_WINDOW")
if env and 0 < int(env) < window:
    window = int(env)
passes = -(-2 * n_frags // window)
med = lambda v: float(np.median(v))
print(json.dumps(dict(device=torch.cuda.get_device_name(0), units=n_units, pairs=pairs, cells=int(cells), frags_per_unit=n_frags, max_len=max_len, frag_cells=int(frag_cells),
                      passes_per_unit=passes, path_bytes_read=int(2 * cells * passes), frag_image_bytes=int(2 * frag_cells),
                      frags_supported=int(sum(s["frags_supported"] for s in summ)), occurrences=int(sum(s["occurrences"] for s in summ)),
                      frag_block_bytes=int(fbytes), junc_block_bytes=int(jbytes),
                      frag_profile_ms=[round(x, 4) for x in fp], junc_profile_ms=[round(x, 4) for x in jp], frag_profile_med_ms=med(fp), junc_profile_med_ms=med(jp),
                      ratio=med(fp) / med(jp), frag_profile_GBps=2 * cells * passes / med(fp) / 1e6)))
