#!/usr/bin/env python3
"""The ILP fill kernel on the single-graph and on the joint (`--op sc_bfb`) model of one 256-segment chromosome, in ONE process on one
device, so that the single-graph rate is the yardstick of the joint one:  python3 profiles/tools/ilp_sc_fill.py [cells] [reps] [--host]

  single graph   56.5 M non-zeros, 0.68 GB     ambi_ilp_fill_kernel<false>
  joint, 3 cells about 170 M non-zeros, 2 GB     ambi_ilp_fill_kernel<true>
Per model: kernel_ms (mean of the last 4 of 5 launches) and 12 * nnz / time; for the joint model also the wall time of
ambi_ilp_build_sc_device end to end (rows on the host, kernel, the device-to-host copy of the entries) and, with --host, of the host
generator ambi_ilp_build_sc for the same model plus an entry-for-entry comparison of the two; with --copy the time of a plain
hipMemcpy of the joint model's entries (4 + 8 bytes per non-zero) from the device into pageable host memory that has been written before --
the copy at the end of ambi_ilp_build_sc_device, which dominates its end-to-end time."""
import os, sys, tempfile, time
os.environ.setdefault("AMBI_EXPERIMENTS", "1")   # the engine honours its AMBI_* switches only with this (ambi_common.hpp: ambi_env)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from ambigram_amd import api, synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
G = int(args[0]) if len(args) > 0 else 3
reps = int(args[1]) if len(args) > 1 else 3
n = 256
lib = api.load(os.environ.get("AMBI_BENCH_LIB") or None); lib.ambi_set_device(0)
tmp = tempfile.mkdtemp()
samples = [synth.make_sample(n, 2 * n, ("wide", "chain", "mixed")[k % 3], 19 if k % 3 == 0 else 9, seed=2000 + k, name="cell%d" % k) for k in range(G)]
graphs = [api.Graph(lib, s.write(tmp)[0]) for s in samples]
lib.ambi_graph_recalculate(graphs[0].h)
seg = np.zeros((G, n)); fold = np.zeros((G, n))
for k, g in enumerate(graphs):
    b = api.Batch(lib); b.add_chromosome(g, 0, [], []); b.upload(); b.run(0); b.download()
    prep = b.unit_prepare(0, n); r = b.unit_result(0)
    fold[k] = np.asarray(prep["junc_cn"])[1:, 1]
    seg[k] = np.asarray(prep["seg_cn"])[1:] if k == 0 else g.segments()["cn"]
    if k == 0:
        prep0, bias0 = prep, r["bias"]
    b.close()


def line(what, m, wall=None):
    rate = 12 * m.nnz / (m.kernel_ms * 1e-3) / 1e9 if m.kernel_ms > 0 else float("nan")   # (nan: host simulation, no device time)
    print("%-12s fill %.4f ms = %.0f GB/s of 12-byte entries (%d rows, %d non-zeros)%s"
          % (what, m.kernel_ms, rate, m.n_rows, m.nnz, "" if wall is None else "; build end to end %.3f s" % wall), flush=True)


for _ in range(reps):   # interleaved: single, joint, single, joint ...
    m = api.IlpModel(lib, graphs[0], 0, prep0["seg_cn"], prep0["junc_cn"], bias0, float(sum(prep0["seg_cn"][1:])), device=True)
    line("single graph", m); m.close()
    t0 = time.perf_counter()
    m = api.IlpModel.joint(lib, graphs[0], 0, seg, fold, device=True)
    line("joint G=%d" % G, m, time.perf_counter() - t0)
    if not ({"--host", "--copy"} & set(sys.argv)) or _ < reps - 1:
        m.close()
if "--copy" in sys.argv:
    import ctypes as C
    # the HIP runtime the engine is already bound to (a process must hold one): its path from the process's own map
    hip = C.CDLL(next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l))
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    nnz = m.nnz
    for _ in range(2):
        total = 0.0
        for width in (4, 8):
            host = np.ones(nnz * width, np.uint8)   # written: the pages exist, as those of the model's zeroed vectors do
            dev = C.c_void_p()
            assert hip.hipMalloc(C.byref(dev), nnz * width) == 0 and hip.hipMemset(dev, 0, nnz * width) == 0 and hip.hipDeviceSynchronize() == 0
            t0 = time.perf_counter()
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), dev, nnz * width, 2) == 0   # hipMemcpyDeviceToHost
            total += time.perf_counter() - t0
            hip.hipFree(dev)
        print("device-to-host copy of %d x (4 + 8) bytes = %.2f GB into pageable memory: %.3f s = %.1f GB/s" % (nnz, 12e-9 * nnz, total, 12e-9 * nnz / total), flush=True)
if "--host" in sys.argv:
    t0 = time.perf_counter()
    h = api.IlpModel.joint(lib, graphs[0], 0, seg, fold)
    print("host generator ambi_ilp_build_sc: %.3f s" % (time.perf_counter() - t0), flush=True)
    x, y = m.arrays(), h.arrays()
    same = (m.n_cols, m.n_int, m.n_rows, m.nnz) == (h.n_cols, h.n_int, h.n_rows, h.nnz) and all(np.array_equal(x[k], y[k]) for k in x)
    print("device form == host generator:", same)
    sys.exit(0 if same else 1)
