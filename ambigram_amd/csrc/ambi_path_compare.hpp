// ambi_path_compare.hpp -- path comparison: common ends and indel distance of pairs of paths.
//
// How close are two paths?  A reconstructed path against the simulated truth, a unit's path before indelBFB against the path after
// it, one cell's path against another cell's under --op sc_bfb (shared segmentation, the same local ids).  The paths people compare
// are nearly equal -- a prefix relation between BFB cycles, a handful of SV edits -- so a quadratic table over up to 4 M cells a
// side is the wrong shape: the common ends are trimmed first and the rest goes through Myers' O(ND) greedy diff with insertions and
// deletions only, capped at `dmax` rounds.  Everything is an exact integer; nothing depends on the order of a reduction.
//
// A pair is two sides (A, B).  A side is a unit's path ambi_batch_unit_path(unit, which), encoded 2 * unit + which, or a GIVEN path
// uploaded by the caller in the local signed ids of whatever it is compared with, encoded ~t.  With the cells a[0..la) and
// b[0..lb) there are two orientations o: B0 = b, and the reverse complement B1[i] = -b[lb-1-i].  Per orientation:
//   prefix[o]   the largest p with a[t] == Bo[t] for all t < p
//   suffix[o]   the largest s <= min(la, lb) - prefix[o] with a[la-1-t] == Bo[lb-1-t] for all t < s
//   dist[o]     the fewest single-cell insertions plus deletions that turn a into Bo if that is <= dmax, otherwise -1
//   lcs[o]      (la + lb - dist[o]) / 2, or -1 when dist[o] is -1
// status is 0, or the first failing side's status when a unit side has a negative status or no path (ST_ERR_BAD_INPUT for a unit
// without a path whose own status is not negative, so a failure is never 0): every other field but the lengths is then 0, dist and
// lcs are -1.
//
// One group per pair, both orientations one after the other:
//   trim      whole-group first-mismatch sweeps from both ends: eight cells of either side per thread and tile (two 8-byte loads
//             where the alignment allows, as path_load_chunk; the reverse orientation is read descending), a group minimum finds the
//             first mismatch, and the sweep stops at the tile that holds it.  The middle windows have n and m cells.
//   shortcuts no rounds: both windows empty -> 0; one empty -> the other's length; |n - m| > dmax -> -1.
//   rounds    d = 0 .. dmax on the middle windows.  V[k] is the furthest x on diagonal k = x - y (x cells of the first window and y
//             of the second consumed).  Diagonal k of round d starts from the previous round's V[k-1] (one deletion) and V[k+1]
//             (one insertion) only, so all diagonals of a round are independent and V is updated in place by parity.  A per-thread
//             pre-pass, one thread per diagonal, computes the start of the snake and compares its first kCompareHandover pairs with
//             loads that do not depend on one another; a snake still open behind them is handed to a whole sub-group (a wavefront):
//             64 pairs per ballot round, as the fold arms of ambi_fold_profile.hpp.  The round ends when diagonal n - m reaches n.
//   bounds    a diagonal that leaves the grid (x > n or y > m) holds kCompareNone and starts nothing; nothing is read at or behind
//             a window's end (cells behind P are stale); every loop has a bound known before it starts: rounds <= dmax + 1, a sweep
//             L / tile + 1 tiles, a snake window / sub_size() + 1 ballot rounds.
// Group memory: V, 2 * dmax + 3 ints (2051 ints = 8204 bytes at the cap of 1024).
//
// SPMD over the group policies of ambi_group.hpp: BlockGroup in ambi_path_compare_kernel, HostGroup (sub_size() == 1) in
// Backend::profile's default (the host simulation) and in tests/tools/path_compare_stage_check.cpp.
#pragma once
#include <cstring>
#include <vector>

#include "ambi_batch.hpp"
#include "ambi_group.hpp"
#include "ambi_profile.hpp"

namespace ambi {

// one pair's result; the layout of ambi_path_compare_t (include/ambigram_hip.h)
struct PathCompare {
    int32_t status;      // 0, or the first failing side's status
    int32_t len_a;       // la (0 for a side that failed)
    int32_t len_b;       // lb
    int32_t dmax;        // the request's cap
    int32_t prefix[2];   // [orientation]
    int32_t suffix[2];
    int32_t dist[2];     // -1 above dmax
    int32_t lcs[2];      // -1 where dist is
};
static_assert(sizeof(PathCompare) == 48, "PathCompare is ambi_path_compare_t");

constexpr int kCompareDmaxCap = 1024, kCompareDmaxDefault = 64;
constexpr int kCompareCellCap = 32767, kComparePathCap = 1 << 22;   // a given path: |c| <= 32767 (rcell_t), 1 .. 4 M cells
// The hand-over length: the pre-pass compares this many pairs of a snake per thread; a snake still open behind them goes to a whole
// sub-group (the fold arms' rule, kFoldHandover).
constexpr int kCompareHandover = 8;
constexpr int kCompareNone = -1;            // V[k]: no point of the grid on this diagonal
constexpr int kCompareOpenBit = 1 << 30;    // V[k] between pre-pass and hand-over: the snake is still open (x stays below 2^22)
constexpr int kCompareGridCap = 2048;       // workgroups of a request; a request with more pairs strides (AMBI_COMPARE_GRID shrinks it)

AMBI_HD int64_t compare_lds_bytes(int dmax) { return int64_t(4) * (2 * dmax + 3); }
// Compare block: [PathCompare[n_pairs]] padded to 16 bytes (16 bytes for a request without pairs)
AMBI_HD int64_t compare_block_bytes(int64_t n_pairs) { const int64_t b = pad16(int64_t(sizeof(PathCompare)) * n_pairs); return b > 0 ? b : 16; }

// The given paths of a batch on the host (ambi_batch_set_compare_paths): cells back to back, every path on a multiple of four cells
// (8 bytes); off[t] in cells.  The device image is [off i64 (T)] [len i32 (T), padded to 16 bytes] [cells]: compare_image_bytes.
struct ComparePaths {
    std::vector<rcell_t> cells;
    std::vector<int64_t> off;
    std::vector<int32_t> len;
    int64_t version = 0;   // bumped by every set: the device re-uploads when it holds another
    int n() const { return (int)len.size(); }
    int64_t off_bytes() const { return pad16(int64_t(8) * n()); }
    int64_t len_bytes() const { return pad16(int64_t(4) * n()); }
    int64_t image_bytes() const { const int64_t b = off_bytes() + len_bytes() + pad16(int64_t(2) * (int64_t)cells.size()); return b > 0 ? b : 16; }
    void image(uint8_t* dst) const {
        if (n() > 0) { memcpy(dst, off.data(), sizeof(int64_t) * (size_t)n()); memcpy(dst + off_bytes(), len.data(), sizeof(int32_t) * (size_t)n()); }
        if (!cells.empty()) memcpy(dst + off_bytes() + len_bytes(), cells.data(), sizeof(rcell_t) * cells.size());
    }
};
// the same where the stage reads it
struct CompareGiven {
    const rcell_t* cells; const int64_t* off; const int32_t* len; int n;
};
inline CompareGiven compare_given(const uint8_t* image, const ComparePaths& H) {
    return CompareGiven{reinterpret_cast<const rcell_t*>(image + H.off_bytes() + H.len_bytes()), reinterpret_cast<const int64_t*>(image),
                        reinterpret_cast<const int32_t*>(image + H.off_bytes()), H.n()};
}

// a side of a pair: its cells, or ok == false with the unit's status
struct CompareSide { const rcell_t* cells; int len, status; bool ok; };
AMBI_HD CompareSide compare_side(const UnitIn* units, const uint8_t* results, const CompareGiven& G, int side) {
    if (side < 0) { const int t = ~side; return CompareSide{G.cells + G.off[t], G.len[t], 0, true}; }
    const ProfilePath Q = profile_path(units, results, side >> 1, side & 1);
    // (a failing side always reports a negative status: ST_ERR_BAD_INPUT for a unit whose own status is not negative but that has no path)
    return CompareSide{Q.cells, Q.P, Q.P > 0 || Q.status < 0 ? Q.status : (int)ST_ERR_BAD_INPUT, Q.P > 0};
}

// a window of a path read in one direction: element t is sign * c[base + step * t]
struct CompareSeq { const rcell_t* c; int base, step, sign; };
AMBI_HD int compare_at(const CompareSeq& S, int t) { return S.sign * (int)S.c[S.base + S.step * t]; }

// cells[at .. at + 8) of a path of `len` cells, 0 outside the path: two 8-byte loads when the path and `at` are 8-byte aligned and
// the eight cells lie inside it, else cell by cell; no load depends on another
AMBI_HD void compare_load8(const rcell_t* cells, int len, bool vec, int at, rcell_t (&c)[kProfileChunk]) {
    if (vec && (at & 3) == 0 && at >= 0 && at + kProfileChunk <= len) {
        for (int q = 0; q < kProfileChunk / 4; q++) {
            const ProfileCell4 w = *reinterpret_cast<const ProfileCell4*>(cells + at + 4 * q);
            for (int k = 0; k < 4; k++) c[4 * q + k] = w.v[k];
        }
    } else {
        for (int k = 0; k < kProfileChunk; k++) { const int p = at + k; c[k] = p >= 0 && p < len ? cells[p] : (rcell_t)0; }
    }
}

// The first t in [0, L) with a[a0 + sa * t] != sgn * b[b0 + sb * t], L if there is none (sa, sb: +1 ascending, -1 descending; every
// position named lies inside its path).  Whole group; stops at the tile that holds the mismatch.
template <class G>
AMBI_HD int compare_first_mismatch(const G& g, const rcell_t* a, int la, int a0, int sa, const rcell_t* b, int lb, int b0, int sb, int sgn, int L) {
    const int tid = g.tid(), sz = g.size();
    const bool va = (reinterpret_cast<uintptr_t>(a) & 7) == 0, vb = (reinterpret_cast<uintptr_t>(b) & 7) == 0;
    const int kNone = 0x7fffffff;
    for (int base = 0; base < L; base += sz * kProfileChunk) {
        const int s = base + tid * kProfileChunk;
        int first = kNone;
        if (s < L) {
            rcell_t ca[kProfileChunk], cb[kProfileChunk];
            compare_load8(a, la, va, sa > 0 ? a0 + s : a0 - s - (kProfileChunk - 1), ca);
            compare_load8(b, lb, vb, sb > 0 ? b0 + s : b0 - s - (kProfileChunk - 1), cb);
            for (int k = kProfileChunk - 1; k >= 0; k--) {
                const int x = sa > 0 ? ca[k] : ca[kProfileChunk - 1 - k], y = sgn * (int)(sb > 0 ? cb[k] : cb[kProfileChunk - 1 - k]);
                if (s + k < L && x != y) first = s + k;
            }
        }
        const int m = g.min_i32(first);
        if (m != kNone) return m;   // (uniform)
    }
    return L;
}

// What compare_rounds does with the V of a round that did not end the pair: nothing here; the alignment keeps it for its traceback
// (AlignHistory, ambi_path_align.hpp).  row(g, d, klo, khi, Vk): whole group, behind the round's second barrier; Vk[k] is diagonal k.
struct CompareNoHistory {
    template <class G> AMBI_HD void row(const G&, int, int, int, const int32_t*) const {}
};

// The indel distance of the windows X[0..n) and Y[0..m), n > 0 and m > 0, if it is <= dmax, else -1.  V: 2 * dmax + 3 ints of group
// memory.  Whole group.
template <class G, class H = CompareNoHistory>
AMBI_HD int compare_rounds(const G& g, const CompareSeq& X, int n, const CompareSeq& Y, int m, int dmax, int32_t* V, const H& hist = H()) {
    const int tid = g.tid(), sz = g.size(), W = g.sub_size(), lane = g.sub_lane();
    const int off = dmax + 1, delta = n - m;
    g.sync();   // (V is read by the round that ended the pair or orientation before)
    for (int i = tid; i < 2 * dmax + 3; i += sz) V[i] = kCompareNone;
    g.sync();
    for (int d = 0; d <= dmax; d++) {
        // the diagonals of the round: k = klo, klo + 2 .. khi inside [-m, n], k = d (mod 2)
        int klo = -d < -m ? -m : -d, khi = d > n ? n : d;
        if ((klo + d) & 1) klo++;
        if ((khi + d) & 1) khi--;
        const int cnt = khi >= klo ? (khi - klo) / 2 + 1 : 0;
        // the pre-pass: the start of the snake and its first kCompareHandover pairs, a thread per diagonal
        for (int idx = tid; idx < cnt; idx += sz) {
            const int k = klo + 2 * idx;
            int x = 0;
            if (d > 0) {
                const int l = V[off + k - 1], r = V[off + k + 1];
                const int xl = l >= 0 && l + 1 <= n ? l + 1 : kCompareNone;   // a deletion: x + 1, y stays
                const int xr = r >= 0 && r - k <= m ? r : kCompareNone;       // an insertion: x stays, y + 1 = r - k
                x = xl > xr ? xl : xr;
            }
            int v = kCompareNone;
            if (x >= 0) {
                const int y = x - k;
                int xa[kCompareHandover], yb[kCompareHandover];
                for (int t = 0; t < kCompareHandover; t++) {
                    const bool in = x + t < n && y + t < m;
                    xa[t] = in ? compare_at(X, x + t) : 0; yb[t] = in ? compare_at(Y, y + t) : 1;   // (a cell is never 0)
                }
                int r = 0;
                bool open = true;
                for (int t = 0; t < kCompareHandover; t++) { open = open && xa[t] == yb[t]; r += open; }
                v = (x + r) | (open ? kCompareOpenBit : 0);
            }
            V[off + k] = v;
        }
        g.sync();
        // the open snakes: a sub-group each, sub_size() pairs per round
        for (int idx = g.sub_id(); idx < cnt; idx += g.n_subs()) {
            const int k = klo + 2 * idx, v = V[off + k];
            if (v < 0 || !(v & kCompareOpenBit)) continue;   // (uniform over the sub-group)
            int x = v & ~kCompareOpenBit;
            const int y0 = x - k, room = n - x < m - y0 ? n - x : m - y0, x0 = x;
            for (int it = 0; it <= room / W; it++) {
                const int t = x - x0 + lane;
                const bool in = t < room;
                const int ca = in ? compare_at(X, x + lane) : 0, cb = in ? compare_at(Y, y0 + t) : 1;
                const uint64_t stop = g.sub_ballot_u64(ca != cb);
                if (stop) { x += (int)__builtin_ctzll(stop); break; }
                x += W;
            }
            if (lane == 0) V[off + k] = x;
        }
        g.sync();
        if ((delta < 0 ? -delta : delta) <= d && ((delta + d) & 1) == 0 && V[off + delta] == n) return d;   // (uniform: read behind the barrier)
        hist.row(g, d, klo, khi, V + off);
    }
    return -1;
}

// One pair of a request: pairs[2 i] and pairs[2 i + 1] are the sides; out[i] the result.  Whole group.
template <class G>
AMBI_HD void compare_pair(const G& g, const UnitIn* units, const uint8_t* results, const CompareGiven& given, const int32_t* pairs, int i, int dmax,
                          int32_t* V, PathCompare* out) {
    const CompareSide A = compare_side(units, results, given, pairs[2 * i]), B = compare_side(units, results, given, pairs[2 * i + 1]);
    PathCompare* R = out + i;   // (thread 0 writes the fields where they go: no array of the result is indexed in registers)
    const bool ok = A.ok && B.ok;
    if (g.tid() == 0) {
        R->status = ok ? 0 : !A.ok ? A.status : B.status;
        R->len_a = A.ok ? A.len : 0; R->len_b = B.ok ? B.len : 0; R->dmax = ok ? dmax : 0;
        for (int o = 0; o < 2; o++) { R->prefix[o] = 0; R->suffix[o] = 0; R->dist[o] = -1; R->lcs[o] = -1; }
    }
    if (!ok) return;
    const int la = A.len, lb = B.len, L = la < lb ? la : lb;
    for (int o = 0; o < 2; o++) {
        const int sb = o ? -1 : 1;   // Bo[t] = sb * b[o ? lb-1-t : t]
        const int p = compare_first_mismatch(g, A.cells, la, 0, 1, B.cells, lb, o ? lb - 1 : 0, sb, sb, L);
        const int s = compare_first_mismatch(g, A.cells, la, la - 1, -1, B.cells, lb, o ? 0 : lb - 1, -sb, sb, L - p);
        const int n = la - p - s, m = lb - p - s;
        int d;
        if (n == 0 || m == 0) d = n + m <= dmax ? n + m : -1;
        else if ((n > m ? n - m : m - n) > dmax) d = -1;
        else d = compare_rounds(g, CompareSeq{A.cells, p, 1, 1}, n, CompareSeq{B.cells, o ? lb - 1 - p : p, sb, sb}, m, dmax, V);
        if (g.tid() == 0) { R->prefix[o] = p; R->suffix[o] = s; R->dist[o] = d; R->lcs[o] = d < 0 ? -1 : (la + lb - d) / 2; }
    }
}

}  // namespace ambi
