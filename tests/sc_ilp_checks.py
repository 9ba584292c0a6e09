"""Shared pieces of test_sc_ilp_device.py: synthetic cells over one segmentation, the inputs BFB_ILP_SC takes from the prepare
stage, and the comparisons of the joint model's device form (row descriptors + entry function, ambi_ilp_rows.hpp) with the host
loop generator and the oracle's literal restatement."""
import os

import numpy as np

from ambigram_amd import api, synth

_cells = {}


def cells(workdir, G, n, n_chr=1):
    """G samples over the same segmentation, n segments on every chromosome, different planted decompositions + the joint .sol
    per chromosome (made once per shape: the files are read, never changed)."""
    key = (workdir, G, n, n_chr)
    if key not in _cells:
        tiers = ("chain", "wide", "mixed") if n >= 8 else ("chain",)
        samples = [synth.make_sample(n * n_chr, (2 * n + 4) * n_chr, tiers[k % len(tiers)], min(3, n), seed=9500 + 10 * k + n, n_chr=n_chr,
                                     name="scd_g%d_n%d_c%d_cell%d" % (G, n, n_chr, k)) for k in range(G)]
        lhs = [s.write(workdir)[0] for s in samples]
        sols = []
        for c, text in enumerate(synth.joint_sol_texts(samples)):
            p = os.path.join(workdir, "scd_g%d_n%d_c%d.joint.chr%d.sol" % (G, n, n_chr, c))
            with open(p, "w") as f:
                f.write(text)
            sols.append(p)
        _cells[key] = (lhs, sols)
    return _cells[key]


def joint_inputs(lib, lhs, c):
    """What run_sc_bfb hands to the joint model for chromosome c: graph 0 after its second calculateCopyNum, the segment CNs
    (first graph after its getIndelBias, the others as read) and every graph's own fold-back CNs, from the prepare stage."""
    graphs = [api.Graph(lib, p) for p in lhs]
    lib.ambi_graph_recalculate(graphs[0].h)
    s, e = graphs[0].chromosome(c)
    n = e - s + 1
    seg = np.zeros((len(lhs), n)); fold = np.zeros((len(lhs), n))
    for k, g in enumerate(graphs):
        b = api.Batch(lib)
        b.add_chromosome(g, c, [], [])
        b.upload(); b.run(0); b.download()
        prep = b.unit_prepare(0, n)
        fold[k] = np.asarray(prep["junc_cn"])[1:, 1]
        seg[k] = np.asarray(prep["seg_cn"])[1:] if k == 0 else g.segments()["cn"][s - 1:e]
        b.close()
    return graphs, seg, fold


def same_models(a, b):
    x, y = a.arrays(), b.arrays()
    assert (a.n_cols, a.n_int, a.n_rows, a.nnz) == (b.n_cols, b.n_int, b.n_rows, b.nnz)
    for k in x:
        assert np.array_equal(x[k], y[k]), k


def same_as_oracle(m, o):
    a = m.arrays()
    assert o["ok"] and m.n_cols == o["n_cols"] and m.n_int == o["n_int"] and m.n_rows == len(o["row_lo"])
    assert a["row_ptr"].tolist() == o["row_ptr"]
    assert a["col"].tolist() == o["col"]
    assert np.array_equal(a["val"], np.array(o["val"]))
    for k in ("row_lo", "row_up", "col_lo", "col_up", "obj"):
        assert np.array_equal(a[k], np.array(o[k])), k


def check_case(lib, oracle, workdir, G, n, second_chr, with_oracle):
    """device form == host generator (array for array, plus sizes) and, where asked, == the oracle's literal restatement"""
    lhs, _ = cells(workdir, G, n, 2 if second_chr else 1)
    c = 1 if second_chr else 0
    graphs, seg, fold = joint_inputs(lib, lhs, c)
    assert graphs[0].chromosome(c) == ((n + 1, 2 * n) if second_chr else (1, n))
    d = api.IlpModel.joint(lib, graphs[0], c, seg, fold, device=True)
    h = api.IlpModel.joint(lib, graphs[0], c, seg, fold)
    same_models(d, h)
    if with_oracle:
        same_as_oracle(d, oracle.ilp_sc(lhs, c))
    ms = d.kernel_ms
    d.close(); h.close()
    for g in graphs:
        g.close()
    return ms


def check_cli(exe, lib, oracle, cwd):
    """`--op sc_bfb` on two cells of one 40-segment chromosome (>= 32 segments: the CLI takes the device form): stdout is the
    oracle's log, <prefix>.lp / <prefix>.mps are byte for byte what the HOST form of the model writes for the same inputs."""
    import test_cli_dropin as t
    lhs, sols = cells(cwd, 2, 40)
    bindir = os.path.join(cwd, "bin")
    t.fake_cbc(bindir, sols)
    r = t.run_cli(exe, cwd, bindir, "--op", "sc_bfb", "--in_lh", ",".join(lhs), "--lp_prefix", "cells40")
    assert r.returncode == 0, r.stderr
    got = [l for l in r.stdout.splitlines() if not l.startswith("fake cbc")]
    assert got == oracle.run_sc_bfb(lhs, sols)["log"]
    graphs, seg, fold = joint_inputs(lib, lhs, 0)
    h = api.IlpModel.joint(lib, graphs[0], 0, seg, fold)
    h.write_lp(os.path.join(cwd, "host40.lp"))
    h.write_mps(os.path.join(cwd, "host40.mps"))
    for ext in ("lp", "mps"):
        assert open(os.path.join(cwd, "cells40." + ext), "rb").read() == open(os.path.join(cwd, "host40." + ext), "rb").read(), ext
    h.close()
    for g in graphs:
        g.close()
