// ambi_path_coords.hpp -- path coordinates: the base-pair offset of every cell of a unit's path, and the lift-over of positions of
// the reconstructed amplicon to the cell, the segment and the offset in the segment they come from.
//
// Every other on-request kind reports a path in cells.  A user of a reconstruction works in base pairs: how long is the amplicon,
// where in it does a junction or a fold sit, where in the genome does position p of the amplicon FASTA come from -- the last asked
// once per read when reads are aligned to the amplicon.  With the cells c[0..P) and len(c) the length of segment |c| from the
// batch's length image (LenImage, ambi_pack.hpp: end - start of the .lh, the sequence kind's convention, so that position p here is
// byte p of ambi_batch_sequence's output for the same unit):
//   plane[k]     base pairs in front of cell k, k = 0 .. P; plane[P] is the amplicon's length.  int64: a length is below 2^31 and a
//                path has at most 2^22 cells, so every offset is below 2^53
//   UnitCoords   status, cells, runs (counted as the sequence kind counts them), cells of length 0, bp_len = plane[P], and the base
//                pairs crossed on the '-' strand
//   a query      (unit, pos) -> the LAST k in [0, P) with plane[k] <= pos (of equal offsets the one that holds the base, as
//                seq_prefix_find), its signed local id, plane[k], and the offset from the segment's start in GENOME orientation:
//                j = pos - plane[k] on a '+' cell, len - 1 - j on a '-' cell.  seg_start + seg_off is the genomic coordinate; the
//                base there, complemented on '-', is byte pos of the sequence kind
// Everything is an exact integer; nothing depends on the order of a reduction.
//
// Two stages, two launches:
//   coords_unit   one group per unit.  Rounds of two consecutive cells per thread: the threads' sums go through exscan_i64 with a
//       64-bit carry between the rounds, and a thread writes its two offsets as ONE 16-byte store (a unit's slice starts on a
//       16-byte boundary and a thread's first entry is even).  The entries 0 .. P are written, nothing behind them: P is clamped
//       to the unit's path capacity, so a path that changes under the kernel cannot send a store outside the slice.  A cell whose id
//       is outside 1..n has length 0 (no finish stage writes such a cell).
//   lift_query    one thread per query, behind the scan: a bisection over the unit's slice, bounded by its range (at most 23 steps
//       for 2^22 cells), then one cell and one length.  It reads the summaries and the plane the first launch wrote.
// A unit with a negative status or without a path has P = 0, plane[0] = 0, bp_len = 0 and the comparison's status of a failed
// side (the unit's negative status, or ST_ERR_BAD_INPUT when its status is not negative): every query into it answers that status.
//
// SPMD over the group policies of ambi_group.hpp: BlockGroup in ambi_path_coords_kernel, plain threads in ambi_path_lift_kernel,
// HostGroup in Backend::profile's default (the host simulation) and in tests/tools/path_coords_stage_check.cpp.
#pragma once
#include <vector>

#include "ambi_batch.hpp"
#include "ambi_group.hpp"
#include "ambi_profile.hpp"

namespace ambi {

// per-unit summary; the layout of ambi_unit_coords_t (include/ambigram_hip.h)
struct UnitCoords {
    int32_t status;        // the unit's status, or that of a failed side (above)
    int32_t cells;         // P of the scanned path
    int32_t runs;          // i == 0 || c[i] != c[i-1] + 1
    int32_t empty_cells;   // cells of length 0
    int64_t bp_len;        // plane[P]
    int64_t bp_minus;      // base pairs of the cells with c < 0
};
static_assert(sizeof(UnitCoords) == 32, "UnitCoords is ambi_unit_coords_t");
// a query and its answer; the layouts of ambi_lift_query_t and ambi_lift_t
struct LiftQuery { int32_t unit, reserved; int64_t pos; };
struct PathLift {
    int32_t status;        // 0, or the failed unit's UnitCoords::status
    int32_t cell;          // k, -1 when pos is outside [0, bp_len) or the unit failed
    int32_t seg;           // the signed local id of cell k, 0 where cell is -1
    int32_t reserved;      // 0
    int64_t seg_off;       // offset from the segment's start in genome orientation, -1 where cell is -1
    int64_t cell_start;    // plane[k], -1 where cell is -1
};
static_assert(sizeof(LiftQuery) == 16 && sizeof(PathLift) == 32, "LiftQuery / PathLift are ambi_lift_query_t / ambi_lift_t");

// the length image where the stages read it: unit u's segment i + 1 has len[len_off[u] + i]
struct LenArgs { const int32_t* len; const int64_t* len_off; };
AMBI_HD int64_t coords_cell_len(const LenArgs& I, int u, int n, int c) {
    const int id = c < 0 ? -c : c;
    return id >= 1 && id <= n ? (int64_t)I.len[I.len_off[u] + id - 1] : 0;
}

// Coords block: [UnitCoords[U]] [PathLift[n]] (both multiples of 16 bytes; 16 bytes for an empty batch without queries)
AMBI_HD int64_t coords_results_off(int64_t U) { return int64_t(sizeof(UnitCoords)) * U; }
AMBI_HD int64_t coords_block_bytes(int64_t U, int64_t n) { const int64_t b = coords_results_off(U) + int64_t(sizeof(PathLift)) * n; return b > 0 ? b : 16; }
// Plane area: 8 bytes per cell of every unit's path capacity plus one, a unit's slice padded to 16 bytes.  off[u] = byte offset of
// unit u's slice; returns the bytes of the area.  The area stays on the device.
inline int64_t coords_plane_layout(const std::vector<UnitIn>& units, std::vector<int64_t>& off) {
    int64_t o = 0;
    off.resize(units.size());
    for (size_t u = 0; u < units.size(); u++) { off[u] = o; o += pad16(int64_t(8) * ((int64_t)units[u].path_cap + 1)); }
    return o;
}
// Workgroups of the lift kernel: one thread per query and round, capped; a request with more queries strides (AMBI_LIFT_GRID
// (tests) can only shrink it)
constexpr int kLiftGridCap = 4096;
AMBI_HD int lift_grid(int64_t n, int threads, int asked) { const int64_t g = (n + threads - 1) / threads; return capped_window((int)(g < kLiftGridCap ? g : kLiftGridCap), kLiftGridCap, asked); }

struct CoordPair { int64_t v[2]; } __attribute__((aligned(16)));

// ---- stage 1: the scan ----
// The path of unit u to scan: P = 0 for a negative status or no path, else the length clamped to the capacity.
AMBI_HD ProfilePath coords_path(const UnitIn* units, const uint8_t* results, int u, int which) {
    const UnitPath Q = unit_path(units, results, u, which);
    const int P = (Q.status < 0 || Q.len <= 0) ? 0 : Q.len < Q.path_cap ? Q.len : Q.path_cap;
    return ProfilePath{Q.cells, P < 0 ? 0 : P, Q.status};
}
// planes: the area; plane_off: every unit's byte offset in it; block: the coords block (this stage writes UnitCoords[u]).  Whole group.
template <class G>
AMBI_HD void coords_unit(const G& g, const UnitIn* units, const uint8_t* results, const LenArgs& I, int u, int which, uint8_t* planes,
                         const int64_t* plane_off, uint8_t* block) {
    const int tid = g.tid(), sz = g.size();
    const int n = units[u].n_seg;
    const ProfilePath Q = coords_path(units, results, u, which);
    const int P = Q.P;
    int64_t* plane = reinterpret_cast<int64_t*>(planes + plane_off[u]);
    const bool vec = (reinterpret_cast<uintptr_t>(plane) & 15) == 0;
    int runs = 0, empty = 0;
    int64_t minus = 0, carry = 0;
    // the entries 0 .. P: entry k is the sum of the lengths of the cells in front of k, cells at and behind P count 0
    for (int base = 0; base <= P; base += 2 * sz) {
        const int k = base + 2 * tid;
        int64_t l0 = 0, l1 = 0;
        if (k < P) {
            const int c0 = Q.cells[k];
            l0 = coords_cell_len(I, u, n, c0);
            runs += k == 0 || c0 != (int)Q.cells[k - 1] + 1;
            empty += l0 == 0;
            if (c0 < 0) minus += l0;
            if (k + 1 < P) {
                const int c1 = Q.cells[k + 1];
                l1 = coords_cell_len(I, u, n, c1);
                runs += c1 != c0 + 1;
                empty += l1 == 0;
                if (c1 < 0) minus += l1;
            }
        }
        int64_t tot;
        const int64_t at = carry + g.exscan_i64(l0 + l1, &tot);
        if (k + 1 <= P) {
            if (vec) { CoordPair w; w.v[0] = at; w.v[1] = at + l0; *reinterpret_cast<CoordPair*>(plane + k) = w; }
            else { plane[k] = at; plane[k + 1] = at + l0; }
        } else if (k == P) plane[k] = at;
        carry += tot;
    }
    runs = g.sum_i32(runs); empty = g.sum_i32(empty);
    int64_t minus_all;
    (void)g.exscan_i64(minus, &minus_all);
    if (tid == 0) {
        UnitCoords S;
        S.status = P > 0 || Q.status < 0 ? Q.status : (int)ST_ERR_BAD_INPUT;
        S.cells = P; S.runs = runs; S.empty_cells = empty; S.bp_len = carry; S.bp_minus = minus_all;
        reinterpret_cast<UnitCoords*>(block)[u] = S;
    }
}

// ---- stage 2: the lift ----
// Query i of the request: block holds the summaries of every unit as coords_unit left them, planes their offsets; out[i] is written.
// One thread; the unit index was checked on the host.
AMBI_HD void lift_query(const UnitIn* units, const uint8_t* results, const LenArgs& I, int which, const uint8_t* planes, const int64_t* plane_off,
                        const uint8_t* block, const LiftQuery* queries, int64_t i, PathLift* out) {
    const LiftQuery q = queries[i];
    const int u = q.unit;
    const UnitCoords S = reinterpret_cast<const UnitCoords*>(block)[u];
    PathLift R;
    R.status = S.status < 0 ? S.status : 0; R.cell = -1; R.seg = 0; R.reserved = 0; R.seg_off = -1; R.cell_start = -1;
    if (S.status >= 0 && q.pos >= 0 && q.pos < S.bp_len) {
        const int64_t* plane = reinterpret_cast<const int64_t*>(planes + plane_off[u]);
        int lo = 0, hi = S.cells;   // plane[0] = 0 <= pos < plane[P]: the last k with plane[k] <= pos is in [0, P)
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (plane[mid] <= q.pos) lo = mid; else hi = mid; }
        const int c = unit_path(units, results, u, which).cells[lo];
        const int64_t start = plane[lo], j = q.pos - start;
        R.cell = lo; R.seg = c; R.cell_start = start;
        R.seg_off = c > 0 ? j : coords_cell_len(I, u, units[u].n_seg, c) - 1 - j;
    }
    out[i] = R;
}

}  // namespace ambi
