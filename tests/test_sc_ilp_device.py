"""The joint model of `--op sc_bfb` (BFB_ILP_SC, LGM.cpp:4754-5093) with its entries written through the row descriptors
(ambi_ilp_build_sc_device): bit-identical to the host loop generator (ambi_ilp_build_sc) and to the oracle's literal
restatement.  CPU tests run the shared entry function on the host simulation, `-m gpu` tests run ambi_ilp_fill_kernel."""
import ctypes as C
import os

import numpy as np
import pytest

import sc_ilp_checks as sc
from ambigram_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMBI_ERR_ARG = -33

# (G, n) on a chromosome that starts at segment 1 ...
CASES = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 2), (4, 6), (3, 7), (2, 9), (1, 12), (2, 20), (3, 33), (2, 64)]
# ... and on the SECOND chromosome of a two-chromosome sample (start id n + 1: the only place a forgotten `- s` shows)
CASES_CHR1 = [(2, 9), (3, 7)]


@pytest.mark.parametrize("G,n", CASES)
def test_row_form_equals_loop_generator(hostsim_lib, workdir, G, n):
    sc.check_case(hostsim_lib, None, workdir, G, n, False, False)


@pytest.mark.parametrize("G,n", CASES_CHR1)
def test_row_form_equals_loop_generator_second_chromosome(hostsim_lib, workdir, G, n):
    sc.check_case(hostsim_lib, None, workdir, G, n, True, False)


@pytest.mark.parametrize("G,n", [c for c in CASES if c[1] <= 33])
def test_row_form_equals_oracle(hostsim_lib, oracle, workdir, G, n):
    sc.check_case(hostsim_lib, oracle, workdir, G, n, False, True)


@pytest.mark.parametrize("G,n", CASES_CHR1)
def test_row_form_equals_oracle_second_chromosome(hostsim_lib, oracle, workdir, G, n):
    sc.check_case(hostsim_lib, oracle, workdir, G, n, True, True)


_LH = ("SAMPLE %s\nAVG_CHR_SEG_DP 30\nAVG_WHOLE_HOST_DP 30\nAVG_JUNC_DP 30\nPURITY 1\nAVG_TUMOR_PLOIDY 2\nPLOIDY 2m1\nVIRUS_START 3\n"
       "SOURCE 1\nSINK 2\nSEG H:1:chr1:1:1000 %.1f %.1f\nSEG H:2:chr1:1001:2000 %.1f %.1f\n"
       "JUNC H:1:+ H:2:+ %.1f %.1f U B\nJUNC H:2:+ H:2:- %.1f %.1f U B\nJUNC H:1:- H:1:+ %.1f %.1f U B\n")


def _two_cells(workdir):
    """two cells of one two-segment chromosome: segment CNs (3, 5) and (4, 6), fold-back CNs (1, 2) and (1, 3)"""
    lhs = []
    for name, (c1, c2, adj, f2, f1) in (("cellA", (3, 5, 3, 2, 1)), ("cellB", (4, 6, 4, 3, 1))):
        p = os.path.join(workdir, "sc2_%s.lh" % name)
        with open(p, "w") as f:
            f.write(_LH % ((name,) + tuple(v for cn in (c1, c2, adj, f2, f1) for v in (30.0 * cn, float(cn)))))
        lhs.append(p)
    return lhs


def _check_two_cells_two_segments(lib, oracle, workdir, device):
    """BFB_ILP_SC (LGM.cpp:4754-5093) written out BY HAND for G = 2 graphs of one chromosome of two segments.

    start = 1, end = 2.  combinations: (1,1) (1,2) (2,2); numComp = 6, in a graph's block p11 = 0, p12 = 1, p22 = 2, l11 = 3,
    l12 = 4, l22 = 5; graph 1's block is shifted by numComp: p11' = 6 .. l22' = 11.  numElements = numComp * G = 12; then
    2 n G = 8 columns set aside for the fit epsilons (12..19) and G (G - 1) numComp = 12 linking epsilons (20..31): 32 columns.
    The epsilon of a fit row is numElements + idx / 2 with idx the RUNNING ROW COUNTER (:4815, :4821, :4858, :4864).
    c_i / f_i = segment CN / fold-back CN of graph 0, c_i' / f_i' of graph 1, entries in the order the reference inserts them:

      graph 0 (idx 0..16, the rows of BFB_ILP without its bias row):
        segment 1   r0  p11 + p12 + 2 l11 + 2 l12 + e12 >= c1       r1  ... - e12 <= c1          (12 + 0/2, 12 + 1/2)
                    r2  .5 p11 + .5 p12 + l11 + l12 + e13 >= f1     r3  ... - e13 <= f1          (12 + 2/2, 12 + 3/2)
        segment 2   r4  p12 + p22 + 2 l12 + 2 l22 + e14 >= c2       r5  ... - e14 <= c2
                    r6  .5 p12 + .5 p22 + l12 + l22 + e15 >= f2     r7  ... - e15 <= f2
        patterns    (:4867-4911)  r8  p12 - p11 >= 0    r9  0 <= p11 + p22 + p12 <= 2    r10  p12 - p22 >= 0
        loops       (:4914-4940)  r11  p12 + l12 - l11 >= 0         r12  p12 + l12 - l22 >= 0
                    (:4943-4974)  r13  0 <= l11 + l22 + l12 <= 2    r14  0 <= l11 + l22 + p12 <= 2
        patterns    (:4977-5008)  r15  0 <= l11 + p22 + p12 <= 2    r16  0 <= p11 + l22 + p12 <= 2
      graph 1 (idx 17..33): the same 17 rows on the columns + 6.  SEVENTEEN rows per graph is odd, so the counter enters
      graph 1 at an odd idx and the two rows of one pair get DIFFERENT epsilons, all of them among the linking epsilons:
        segment 1   r17 ... + e20 >= c1'   (12 + 17/2)      r18 ... - e21 <= c1'   (12 + 18/2)
                    r19 ... + e21 >= f1'   (12 + 19/2)      r20 ... - e22 <= f1'   (12 + 20/2)
        segment 2   r21 ... + e22 >= c2'                    r22 ... - e23 <= c2'
                    r23 ... + e23 >= f2'                    r24 ... - e24 <= f2'
        r25 .. r33  the nesting rows of r8 .. r16, columns + 6
      linking rows (:5032-5072), the one pair (0, 1), cnt from 2 * (numElements + 2 n G) = 40, epsilon cnt / 2:
        element c = 0..5:   r(34 + 2c)  x_c - x_(c+6) + e(20 + c) >= 0      r(35 + 2c)  x_c - x_(c+6) - e(20 + c) <= 0
    46 rows.  Columns (:5012-5027, :5074-5086): p in [0,1], l in [0, CN sum of THAT graph's segments 1..2], epsilons in [0, inf);
    objective 1 on every column from numElements up; the 12 elements are integer."""
    lhs = _two_cells(workdir)
    graphs, seg, fold = sc.joint_inputs(lib, lhs, 0)
    # what the prepare stage hands over for these files: no SV edits the CNs, fold-back CN = CN of the segment's fold-back junction
    assert seg.tolist() == [[3.0, 5.0], [4.0, 6.0]] and fold.tolist() == [[1.0, 2.0], [1.0, 3.0]]
    inf = float("inf")

    def graph_rows(o, eps, c1, c2, f1, f2):
        p11, p12, p22, l11, l12, l22 = range(o, o + 6)
        return [
            ([(p11, 1), (p12, 1), (l11, 2), (l12, 2), (eps[0], 1)], c1, inf), ([(p11, 1), (p12, 1), (l11, 2), (l12, 2), (eps[1], -1)], -inf, c1),
            ([(p11, .5), (p12, .5), (l11, 1), (l12, 1), (eps[2], 1)], f1, inf), ([(p11, .5), (p12, .5), (l11, 1), (l12, 1), (eps[3], -1)], -inf, f1),
            ([(p12, 1), (p22, 1), (l12, 2), (l22, 2), (eps[4], 1)], c2, inf), ([(p12, 1), (p22, 1), (l12, 2), (l22, 2), (eps[5], -1)], -inf, c2),
            ([(p12, .5), (p22, .5), (l12, 1), (l22, 1), (eps[6], 1)], f2, inf), ([(p12, .5), (p22, .5), (l12, 1), (l22, 1), (eps[7], -1)], -inf, f2),
            ([(p12, 1), (p11, -1)], 0, inf), ([(p11, 1), (p22, 1), (p12, 1)], 0, 2), ([(p12, 1), (p22, -1)], 0, inf),
            ([(p12, 1), (l12, 1), (l11, -1)], 0, inf), ([(p12, 1), (l12, 1), (l22, -1)], 0, inf),
            ([(l11, 1), (l22, 1), (l12, 1)], 0, 2), ([(l11, 1), (l22, 1), (p12, 1)], 0, 2),
            ([(l11, 1), (p22, 1), (p12, 1)], 0, 2), ([(p11, 1), (l22, 1), (p12, 1)], 0, 2),
        ]

    rows = graph_rows(0, [12, 12, 13, 13, 14, 14, 15, 15], 3.0, 5.0, 1.0, 2.0)
    rows += graph_rows(6, [20, 21, 21, 22, 22, 23, 23, 24], 4.0, 6.0, 1.0, 3.0)
    for c in range(6):
        rows += [([(c, 1), (c + 6, -1), (20 + c, 1)], 0, inf), ([(c, 1), (c + 6, -1), (20 + c, -1)], -inf, 0)]
    col_lo = [0] * 32
    col_up = [1, 1, 1, 8, 8, 8, 1, 1, 1, 10, 10, 10] + [inf] * 20
    obj = [0] * 12 + [1] * 20

    def clip(v):     # (the arrays carry the solver's "infinity", 1e30 or larger, for unbounded sides)
        return inf if v >= 1e29 else (-inf if v <= -1e29 else v)

    def check(n_cols, n_int, row_ptr, col, val, row_lo, row_up, clo, cup, ob):
        assert (n_cols, n_int, len(row_ptr) - 1) == (32, 12, 46)
        for r, (ent, lo, up) in enumerate(rows):
            got = list(zip(col[row_ptr[r]:row_ptr[r + 1]], val[row_ptr[r]:row_ptr[r + 1]]))
            assert got == [(c, float(v)) for c, v in ent], (r, got)          # the entries in the reference's insertion order
            assert (clip(row_lo[r]), clip(row_up[r])) == (lo, up), r
        assert [clip(v) for v in clo] == col_lo and [clip(v) for v in cup] == col_up and list(ob) == obj
        eps_of = lambda r: col[row_ptr[r + 1] - 1]
        graph1_first_cn_pair = (eps_of(17), eps_of(18))
        first_linking_row = eps_of(34)
        assert graph1_first_cn_pair == (20, 21)      # rows 17 and 18: 12 + 17/2 and 12 + 18/2 -- one pair, two epsilons
        assert first_linking_row == 20               # ... the first of which is also the first linking epsilon

    m = api.IlpModel.joint(lib, graphs[0], 0, seg, fold, device=device)
    a = m.arrays()
    check(m.n_cols, m.n_int, a["row_ptr"].tolist(), a["col"].tolist(), a["val"].tolist(), a["row_lo"].tolist(), a["row_up"].tolist(),
          a["col_lo"].tolist(), a["col_up"].tolist(), a["obj"].tolist())
    o = oracle.ilp_sc(lhs, 0)
    assert o["ok"]
    check(o["n_cols"], o["n_int"], o["row_ptr"], o["col"], o["val"], o["row_lo"], o["row_up"], o["col_lo"], o["col_up"], o["obj"])
    m.close()
    for g in graphs:
        g.close()


def test_two_cells_two_segments_hand_derived(hostsim_lib, oracle, workdir):
    _check_two_cells_two_segments(hostsim_lib, oracle, workdir, True)      # row descriptors + entry function
    _check_two_cells_two_segments(hostsim_lib, oracle, workdir, False)     # the loop generator against the same rows


def test_limits_are_refused(hostsim_lib, workdir):
    """Each limit of the row descriptor (ambi_ilp_rows.hpp) is AMBI_ERR_ARG with *out left null -- on a one-segment chromosome,
    where rows = columns = 2 G^2 + 2 G, so every limit is reached by the graph count alone and nothing large is built."""
    lhs, _ = sc.cells(workdir, 1, 1)
    g = api.Graph(hostsim_lib, lhs[0])
    assert g.chromosome(0) == (1, 1)
    pd = C.POINTER(C.c_double)

    def build(G):
        cn = np.ones(max(G, 1))
        out = C.c_void_p()
        rc = hostsim_lib.ambi_ilp_build_sc_device(g.h, 0, G, cn.ctypes.data_as(pd), cn.ctypes.data_as(pd), None, C.byref(out))
        return rc, out.value

    assert build(0) == (AMBI_ERR_ARG, None) and build(-3) == (AMBI_ERR_ARG, None)       # n_graphs < 1
    assert build(1 << 23) == (AMBI_ERR_ARG, None)        # g + 1 no longer fits the 23 bits of `family` (the limit is 2^23 - 1)
    assert 2 * 40000 ** 2 + 2 * 40000 > 2 ** 31 - 1
    assert build(40000) == (AMBI_ERR_ARG, None)          # 3.2e9 rows > INT32_MAX
    rows = 2 * 23171 ** 2 + 2 * 23171
    assert rows <= 2 ** 31 - 1 and 2 * rows >= 2 ** 31   # rows still fit, 2 * n_cols does not: the `rep` packing
    assert build(23171) == (AMBI_ERR_ARG, None)
    rc, h = build(3)                                     # (the same call within the limits builds)
    assert rc == 0 and h
    hostsim_lib.ambi_ilp_destroy(C.c_void_p(h))
    g.close()


def test_cli_takes_the_device_form(hostsim_lib, oracle, tmp_path):
    sc.check_cli(os.path.join(ROOT, "tests", "hostsim", "Ambigram_hostsim"), hostsim_lib, oracle, str(tmp_path))


# ---- on the GPU: the smallest shapes at which ambi_ilp_fill_kernel<joint> can still go wrong
#   (2,1)  36 non-zeros: one partial chunk, the scalar tail (want < 4), both pieces of the +- epsilon fix-up
#   (2,2), (3,7)  linking rows straddled by every 4-entry span; (3,7) crosses chunk boundaries in per-graph and linking rows
#   (2,20), (3,33) on a chromosome with start id > 1: CN rows that span several chunks, many short rows inside one chunk
@pytest.mark.gpu
@pytest.mark.parametrize("G,n,second_chr", [(2, 1, False), (2, 2, False), (3, 7, False), (2, 20, True), (3, 33, True)])
def test_joint_entries_written_on_the_device(hip_lib, oracle, workdir, G, n, second_chr):
    sc.check_case(hip_lib, oracle, workdir, G, n, second_chr, True)


@pytest.mark.gpu
def test_joint_entries_written_on_the_device_full_chunks(hip_lib, workdir):
    """(2,64): about 1.8 M non-zeros, almost every thread on the four-entries-of-one-row path; host generator only"""
    ms = sc.check_case(hip_lib, None, workdir, 2, 64, False, False)
    assert ms > 0


@pytest.mark.gpu
def test_two_cells_two_segments_hand_derived_on_the_gpu(hip_lib, oracle, workdir):
    _check_two_cells_two_segments(hip_lib, oracle, workdir, True)


@pytest.mark.gpu
def test_cli_takes_the_device_form_on_the_gpu(hip_lib, oracle, tmp_path):
    sc.check_cli(os.path.join(ROOT, "ambigram_amd", "bin", "Ambigram"), hip_lib, oracle, str(tmp_path))
