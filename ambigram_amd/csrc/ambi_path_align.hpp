// ambi_path_align.hpp -- path alignment: the edit script of pairs of paths as maximal runs.
//
// Where do two paths differ, and by which cells?  The path comparison (ambi_path_compare.hpp) says how far apart they are; this stage
// returns a canonical shortest insert / delete script for ONE orientation per pair.  An entry is a triple (A, B, orient): the sides of
// the comparison (2 * unit + which, or ~t for a given path) and 0 (as is) or 1 (against the reverse complement Bo[i] = -b[lb-1-i]).
// With p / s the common prefix and suffix the middle windows are X = a[p .. la-s) and Y = Bo[p .. lb-s) of n and m cells:
//   both empty      distance 0, no runs
//   one empty       distance n + m if that is <= dmax (one run: all of X deleted, or all of Y inserted), else -1
//   |n - m| > dmax  -1
//   otherwise       Myers' forward rounds exactly as the comparison runs them (compare_rounds; ties go to the insertion), the V of every
//                   round kept, and the traceback from (D, n - m): at (d, k) the round's two candidates are recomputed from round d - 1,
//                   xl = V[k-1] + 1 and xr = V[k+1] where they are on the grid; if xl > xr edit d - 1 deletes X[xl-1] and the walk goes
//                   to k - 1, else it inserts Y[xr-k-1] and goes to k + 1.
// A unit edit is (kind, a_pos, b_pos) in the coordinates of the whole a and the whole Bo: kind 0 deletes a[a_pos] (b_pos: the cell of
// Bo in front of which it would stand), kind 1 inserts Bo[b_pos] in front of a[a_pos].  Consecutive unit edits of one kind with no
// matched cell between them merge into one maximal run {a_pos, b_pos, len, kind}: a_pos advances through a deletion run and b_pos
// stays, the other way round for insertions; a deletion directly followed by an insertion stays two runs.  A pair has at most dist
// runs.  dist == -1 (above dmax, or a failed side) has no runs.
//
// One group per pair:
//   trim, shortcuts  as compare_pair, for the one orientation
//   rounds           compare_rounds with AlignHistory: behind the second barrier of round d the round's V goes to row d of the
//                    group's history area in device memory -- row d at d (d + 1) / 2, d + 1 slots, diagonal k at (k + d) / 2, a
//                    diagonal clipped off the grid holds kCompareNone.  The round that ends the pair and round dmax are not kept: a
//                    traceback from D reads rows below D only, so at dmax 0 nothing is written.  The area belongs to the group and
//                    is written and read by it alone, the group barrier between.
//   traceback        thread 0 walks D steps, two reads of the history each, and writes unit edit d - 1 at its place in group memory
//                    (8 bytes an edit: a_pos, and b_pos with the kind in bit 30)
//   merge            the whole group flags the run heads, ranks them tile by tile (flag_exscan, the count carried), leaves every
//                    run's first edit in V (free behind the rounds), then writes the runs -- 16 bytes each -- zeroes the pair's other
//                    slots, and thread 0 writes the header.
// Every loop has a bound known before it starts (rounds <= dmax + 1, traceback D, merge D / size + 1 tiles, slots dmax / size + 1);
// nothing is read at or behind a window's end.  Group memory: V (2 * dmax + 3 ints) + the edit list (2 * dmax ints): 16396 bytes at
// the cap of 1024.  History: (dmax + 1)(dmax + 2) / 2 ints per group, 8.6 KB at dmax 64 and 2.1 MB at 1024.
//
// SPMD over the group policies of ambi_group.hpp: BlockGroup in ambi_path_align_kernel, HostGroup in Backend::profile's default (the
// host simulation) and in tests/tools/path_align_stage_check.cpp.
#pragma once
#include "ambi_path_compare.hpp"

namespace ambi {

// one pair's header; the layout of ambi_path_align_t (include/ambigram_hip.h)
struct PathAlign {
    int32_t status;   // 0, or the first failing side's status
    int32_t len_a;    // la (0 for a side that failed)
    int32_t len_b;    // lb
    int32_t orient;   // the request's: 0 as is, 1 against the reverse complement
    int32_t prefix;   // 0 for a failed pair
    int32_t suffix;
    int32_t dist;     // -1 above dmax and for a failed pair
    int32_t n_runs;   // 0 where dist is -1
};
static_assert(sizeof(PathAlign) == 32, "PathAlign is ambi_path_align_t");
// one maximal run of unit edits; the layout of ambi_align_run_t
struct AlignRun {
    int32_t a_pos;    // the first cell of a it deletes / the cell of a in front of which it inserts
    int32_t b_pos;    // the cell of Bo in front of which the deleted cells would stand / the first cell of Bo it inserts
    int32_t len;
    int32_t kind;     // 0 deletion, 1 insertion
};
static_assert(sizeof(AlignRun) == 16, "AlignRun is ambi_align_run_t");

constexpr int kAlignGridCap = 2048;                         // workgroups of a request (AMBI_ALIGN_GRID shrinks it) ...
constexpr int64_t kAlignHistoryCap = int64_t(256) << 20;    // ... and fewer where their history areas would exceed this
constexpr int64_t kAlignRunAreaCap = int64_t(1) << 30;      // a request whose run area is larger is refused
constexpr int kAlignKindBit = 1 << 30;                      // the edit list: b_pos | kind << 30 (positions stay below 2^22)

AMBI_HD int align_stride(int dmax) { return dmax > 0 ? dmax : 1; }   // run slots per pair
AMBI_HD int64_t align_lds_bytes(int dmax) { return compare_lds_bytes(dmax) + int64_t(8) * dmax; }
AMBI_HD int64_t align_history_ints(int dmax) { return int64_t(dmax + 1) * (dmax + 2) / 2; }
AMBI_HD int64_t align_history_bytes(int dmax) { return pad16(int64_t(4) * align_history_ints(dmax)); }
// Align block: [PathAlign[n_pairs]] padded to 16 bytes, then AlignRun[n_pairs * align_stride(dmax)] (16 bytes for a request without pairs)
AMBI_HD int64_t align_runs_off(int64_t n_pairs) { return pad16(int64_t(sizeof(PathAlign)) * n_pairs); }
AMBI_HD int64_t align_run_area_bytes(int64_t n_pairs, int dmax) { return int64_t(sizeof(AlignRun)) * n_pairs * align_stride(dmax); }
AMBI_HD int64_t align_block_bytes(int64_t n_pairs, int dmax) { const int64_t b = align_runs_off(n_pairs) + align_run_area_bytes(n_pairs, dmax); return b > 0 ? b : 16; }
AMBI_HD int align_grid(int64_t n_pairs, int dmax, int asked) {
    const int64_t fit = kAlignHistoryCap / align_history_bytes(dmax);
    return capped_window((int)(n_pairs < kAlignGridCap ? n_pairs : kAlignGridCap), (int)(fit < kAlignGridCap ? fit : kAlignGridCap), asked);
}

// compare_rounds' hook: the V of round d to row d of the group's history (see above)
struct AlignHistory {
    int32_t* H; int dmax;
    template <class G> AMBI_HD void row(const G& g, int d, int klo, int khi, const int32_t* Vk) const {
        if (d >= dmax) return;   // (uniform; a traceback never reads row dmax)
        int32_t* R = H + d * (d + 1) / 2;
        for (int j = g.tid(); j <= d; j += g.size()) { const int k = 2 * j - d; R[j] = k >= klo && k <= khi ? Vk[k] : kCompareNone; }
    }
};
AMBI_HD int align_history_at(const int32_t* H, int d, int k) { return k < -d || k > d ? kCompareNone : H[d * (d + 1) / 2 + (k + d) / 2]; }

// One entry of a request: triples[3 i .. 3 i + 3) = (A, B, orient); head[i] and runs[i * align_stride(dmax) ..] are its results.  V:
// 2 * dmax + 3 ints and E: 2 * dmax ints of group memory; H: align_history_ints(dmax) ints of device memory of this group.  Whole group.
template <class G>
AMBI_HD void align_pair(const G& g, const UnitIn* units, const uint8_t* results, const CompareGiven& given, const int32_t* triples, int i, int dmax,
                        int32_t* V, int32_t* E, int32_t* H, PathAlign* head, AlignRun* runs) {
    const int tid = g.tid(), sz = g.size(), stride = align_stride(dmax);
    const CompareSide A = compare_side(units, results, given, triples[3 * i]), B = compare_side(units, results, given, triples[3 * i + 1]);
    const int o = triples[3 * i + 2];
    const bool ok = A.ok && B.ok;
    AlignRun* out = runs + (int64_t)i * stride;
    int p = 0, s = 0, D = -1, n_runs = 0;
    if (ok) {
        const int la = A.len, lb = B.len, L = la < lb ? la : lb, sb = o ? -1 : 1;   // Bo[t] = sb * b[o ? lb-1-t : t]
        p = compare_first_mismatch(g, A.cells, la, 0, 1, B.cells, lb, o ? lb - 1 : 0, sb, sb, L);
        s = compare_first_mismatch(g, A.cells, la, la - 1, -1, B.cells, lb, o ? 0 : lb - 1, -sb, sb, L - p);
        const int n = la - p - s, m = lb - p - s;
        if (n == 0 || m == 0) {
            D = n + m <= dmax ? n + m : -1;
            if (D > 0) { n_runs = 1; if (tid == 0) out[0] = AlignRun{p, p, D, m > 0 ? 1 : 0}; }
        } else if ((n > m ? n - m : m - n) <= dmax) {
            D = compare_rounds(g, CompareSeq{A.cells, p, 1, 1}, n, CompareSeq{B.cells, o ? lb - 1 - p : p, sb, sb}, m, dmax, V, AlignHistory{H, dmax});
            g.sync();   // (the history rows and the last reads of V)
            if (D > 0) {
                if (tid == 0) {   // the traceback: edit d - 1 from round d - 1's neighbours of diagonal k
                    int k = n - m;
                    for (int d = D; d > 0; d--) {
                        const int l = align_history_at(H, d - 1, k - 1), r = align_history_at(H, d - 1, k + 1);
                        const int xl = l >= 0 && l + 1 <= n ? l + 1 : kCompareNone, xr = r >= 0 && r - k <= m ? r : kCompareNone;
                        const bool del = xl > xr;
                        E[2 * (d - 1)] = p + (del ? xl - 1 : xr);
                        E[2 * (d - 1) + 1] = del ? p + xl - k : (p + xr - k - 1) | kAlignKindBit;
                        k += del ? -1 : 1;
                    }
                }
                g.sync();
                // the run heads, ranked tile by tile; V[r] = the first edit of run r
                int carry = 0;
                for (int base = 0; base < D; base += sz) {
                    const int e = base + tid;
                    bool head_e = false;
                    if (e < D) {
                        head_e = e == 0;
                        if (e > 0) {
                            const int a0 = E[2 * e - 2], b0 = E[2 * e - 1], a1 = E[2 * e], b1 = E[2 * e + 1];
                            const bool ins = (b1 & kAlignKindBit) != 0;
                            head_e = ((b0 ^ b1) & kAlignKindBit) != 0 || (ins ? a1 != a0 || b1 != b0 + 1 : a1 != a0 + 1 || b1 != b0);
                        }
                    }
                    int count;
                    const int rank = g.flag_exscan(head_e, &count);
                    if (head_e) V[carry + rank] = e;
                    carry += count;
                }
                n_runs = carry;
                if (tid == 0) V[n_runs] = D;
                g.sync();
                for (int r = tid; r < n_runs; r += sz) {
                    const int e = V[r], b = E[2 * e + 1];
                    out[r] = AlignRun{E[2 * e], b & ~kAlignKindBit, V[r + 1] - e, (b & kAlignKindBit) != 0 ? 1 : 0};
                }
            }
        }
    }
    for (int r = n_runs + tid; r < stride; r += sz) out[r] = AlignRun{0, 0, 0, 0};
    if (tid == 0) {   // (thread 0 writes the fields where they go)
        PathAlign* R = head + i;
        R->status = ok ? 0 : !A.ok ? A.status : B.status;
        R->len_a = A.ok ? A.len : 0; R->len_b = B.ok ? B.len : 0; R->orient = o;
        R->prefix = p; R->suffix = s; R->dist = D; R->n_runs = n_runs;
    }
}

}  // namespace ambi
