#!/usr/bin/env python3
"""Path sequences against a plain copy: python3 profiles/tools/seq_bench.py [units=16] [rounds=12]

16 bench-tier units (synth: 256 segments, 512 junctions, wide K = 19) with seeded segment lengths of 2-20 kb, which = 1.  Per
round, in ONE process and interleaved: ambi_batch_sequence (its extents kernel -- both launches, pass 0 + pass 1 -- and its fill kernel timed by HIP events,
read through the engine's kernel-time getters) and a hipMemcpyAsync device-to-device copy of exactly the output block's byte count, timed by
events on the same stream.  The copy is the yardstick: the fill writes every output byte once from a store that mostly sits in L2,
so it should approach a copy's write half.  Prints one JSON line with both medians, the ratio and the bytes."""
import ctypes as C
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ambigram_amd import api, synth

n_units = int(sys.argv[1]) if len(sys.argv) > 1 else 16
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 12
lib = api.load(); lib.ambi_set_device(0); torch.cuda.set_device(0)
hip = api._RUNTIME[0] or C.CDLL("libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
hip.hipMemcpyAsync.restype = C.c_int
D2D = 3   # hipMemcpyDeviceToDevice

tmp = tempfile.mkdtemp(); b = api.Batch(lib); keep = []
rng = np.random.default_rng(13)
letters = np.frombuffer(b"ACGTacgtN", np.uint8)
for i in range(n_units):
    s = synth.make_sample(256, 512, "wide", 19, seed=2000 + 8 * i + 7, n_del=2, n_dup=1)
    lh, sols = s.write(tmp, "q%d" % i)
    g = api.Graph(lib, lh); keep.append(g)
    lens = rng.integers(2000, 20001, size=g.n_seg)
    g.set_sequences(rng.choice(letters, int(lens.sum())), np.concatenate([[0], np.cumsum(lens)]))
    b.add_chromosome_sol(g, 0, sols[0])
stream = torch.cuda.Stream(); st = stream.cuda_stream
b.upload(); b.run(0, st); b.wait()
b.set_timing(True)
b.run(0, st); b.wait()
b.sequence(1, 0, n_units, 0, st); b.sequence_wait()
ptr, nbytes, off = b.sequence_device()
seq_bytes = sum(b.unit_sequence_len(u) for u in range(n_units))
b.download()
cells = sum(b.unit_result(u)["path_indel_len"] for u in range(n_units))
src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").random_(0, 255)
dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
fill, ext, copy = [], [], []
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for r in range(rounds + 2):
    b.sequence(1, 0, n_units, 0, st); b.sequence_wait()
    kt = dict(b.kernel_times())
    with torch.cuda.stream(stream):
        e0.record(stream)
        rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, D2D, st)
        e1.record(stream)
    assert rc == 0
    e1.synchronize()
    if r >= 2:   # (two warm-up rounds)
        fill.append(kt["ambi_seq_fill_kernel"]); ext.append(kt["ambi_seq_extents_kernel"]); copy.append(e0.elapsed_time(e1))
assert torch.equal(dst, src)
med = lambda v: float(np.median(v))
out = dict(units=n_units, rounds=rounds, cells=int(cells), seq_bytes=int(seq_bytes), block_bytes=int(nbytes), fill_ms=med(fill), fill_min_ms=min(fill),
           extents_ms=med(ext), copy_ms=med(copy), copy_min_ms=min(copy), fill_GBps=nbytes / med(fill) / 1e6, copy_GBps=nbytes / med(copy) / 1e6,
           fill_over_copy_time=med(fill) / med(copy))
print(json.dumps(out))
