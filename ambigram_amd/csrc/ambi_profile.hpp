// ambi_profile.hpp -- copy-number profile of a unit's path: how often the path crosses every segment, per strand, and a
// summary of how that compares with the decomposition's target copy numbers and with the input copy numbers.
//
// The reference meant to report this (localhap.cpp:318-324 computes an `isResolved` verdict from the sum of |CN - targetCN|,
// localhap.cpp:340-351 is a commented-out CN.txt writer whose fallback for a segment counts the segment's occurrences in the
// path).  The reference's `isResolved` sum is NOT reproduced: it truncates a running `int` after every add and only
// commented-out code reads it.  What is computed here are exact integers (no floating-point sums: nothing depends on the
// order of a reduction):
//   fwd[i], rev[i]   traversals of segment i on the '+' / '-' strand
//   UnitProfile      status, cells, runs, fold-back turns taken, max / uncovered / off-target / off-input counts, L1 distance
//
// A path is a concatenation of runs counting up by one (`3 4 5`, `-5 -4 -3`), so the stage works on run boundaries and not on
// cells: every boundary cell posts ONE event into a per-strand difference array in group memory, and an inclusive prefix sum
// over the segments gives the counts.  Start and end of a run are never paired.
//   cell i begins a run  <=>  i == 0      ||  c[i] != c[i-1] + 1
//   cell i ends a run    <=>  i == P - 1  ||  c[i+1] != c[i] + 1          (so: i ends a run exactly when i + 1 begins one)
//   '+' strand:  d_f[c] += 1 at a beginning,      d_f[c+1] -= 1 at an end
//   '-' strand:  d_r[|c|+1] -= 1 at a beginning,  d_r[|c|] += 1 at an end    (the run -5 -4 -3 covers the segments 5, 4, 3)
// The difference arrays hold `window` segments; a unit with more segments is served by passes over segment windows: a pass
// posts only the events whose index falls into its window, and the running counts at the end of a window carry into the next.
// Only group-memory atomics are used (one per event), no atomic on device memory.
//
// SPMD over the group policies of ambi_group.hpp like the stages of ambi_stages.hpp: BlockGroup in ambi_path_profile_kernel,
// HostGroup in Backend::profile's default (the host simulation).
#pragma once
#include <vector>

#include "ambi_batch.hpp"
#include "ambi_group.hpp"

namespace ambi {

// per-unit summary; the layout of ambi_unit_profile_t (include/ambigram_hip.h)
struct UnitProfile {
    int32_t status;        // the unit's status, copied
    int32_t cells;         // P of the profiled path
    int32_t runs;          // number of runs
    int32_t turns;         // steps with c[i+1] == -c[i]: fold-back turns actually taken
    int32_t max_cn;        // max over i of fwd[i] + rev[i]
    int32_t n_uncovered;   // segments with fwd + rev == 0
    int32_t n_off_target;  // segments with fwd + rev != target_cn[i]
    int32_t n_off_input;   // segments with |fwd + rev - seg_cn[i]| >= 0.5 (seg_cn after getIndelBias, as in the result blob)
    int64_t l1_target;     // sum over i of |fwd + rev - target_cn[i]|
};
static_assert(sizeof(UnitProfile) == 40, "UnitProfile is ambi_unit_profile_t");

// ---- what the on-request profiles (this one, ambi_junc_profile.hpp, ambi_frag_profile.hpp, ambi_evidence_profile.hpp) share ----
// The window rule: the largest unit of the batch, capped, and what a test asks for can only shrink it.
AMBI_HD int capped_window(int max, int cap, int asked) {
    int w = max < 1 ? 1 : max;
    if (w > cap) w = cap;
    if (asked > 0 && asked < w) w = asked;
    return w;
}

// The unit prologue: the path of unit u to profile (unit_path, ambi_batch.hpp), or P = 0 -- the unit gets its kind's empty result --
// for a negative status, no path, or a length above the capacity (never: the finish stages refuse such a path).
struct ProfilePath { const rcell_t* cells; int P, status; };
AMBI_HD ProfilePath profile_path(const UnitIn* units, const uint8_t* results, int u, int which) {
    const UnitPath Q = unit_path(units, results, u, which);
    return ProfilePath{Q.cells, (Q.status < 0 || Q.len <= 0 || Q.len > Q.path_cap) ? 0 : Q.len, Q.status};
}

// The chunked cell read: a thread's chunk [s, s + kProfileChunk) of the path as two 8-byte loads (vec: the path is 8-byte
// aligned; per-unit arrays of the blob are 8-byte padded) or cell by cell, zero behind P (but for the padding of the 8-byte word
// that holds cell P - 1).  Returns e, the cells of the chunk inside the path -- the caller's loop is `k < e` --; prev = the cell
// in front of the chunk (0 in front of the path): the steps (i - 1, i) of the chunk need it.
constexpr int kProfileChunk = 8;   // cells per thread and tile
struct ProfileCell4 { rcell_t v[4]; } __attribute__((aligned(8)));
AMBI_HD int path_load_chunk(const rcell_t* cells, int P, bool vec, int s, rcell_t (&c)[kProfileChunk], int& prev) {
    for (int q = 0; q < kProfileChunk / 4; q++) {
        const int at = s + 4 * q;
        if (at >= P) { for (int k = 0; k < 4; k++) c[4 * q + k] = 0; continue; }
        if (vec) { const ProfileCell4 w = *reinterpret_cast<const ProfileCell4*>(cells + at); for (int k = 0; k < 4; k++) c[4 * q + k] = w.v[k]; }
        else for (int k = 0; k < 4; k++) c[4 * q + k] = at + k < P ? cells[at + k] : (rcell_t)0;
    }
    prev = s > 0 ? (int)cells[s - 1] : 0;
    return s + kProfileChunk < P ? kProfileChunk : P - s;
}

// Segments per window: the largest unit of the batch, capped so that the two difference arrays take 32 KB of group memory
// (four workgroups of the profile kernel still fit a CU's 160 KB); AMBI_PROFILE_WINDOW (tests) can only shrink it.
constexpr int kProfileWindowCap = 4096;
AMBI_HD int profile_window(int max_n, int asked) { return capped_window(max_n, kProfileWindowCap, asked); }
AMBI_HD int64_t profile_bins_bytes(int window) { return int64_t(2) * 4 * window; }

// Profile block: [UnitProfile[U]] [per unit: fwd i32 (n+1), rev i32 (n+1)], every per-unit array on a 16-byte boundary, slot 0
// unused (zero) as in the other per-segment arrays.  off[u] = byte offset of unit u's fwd array; rev follows at profile_rev_off.
AMBI_HD int64_t profile_rev_off(int n) { return pad16(int64_t(4) * (n + 1)); }
inline int64_t profile_block_layout(const std::vector<UnitIn>& units, std::vector<int64_t>& off) {
    int64_t o = pad16(int64_t(sizeof(UnitProfile)) * (int64_t)units.size());
    off.resize(units.size());
    for (size_t u = 0; u < units.size(); u++) { off[u] = o; o += 2 * profile_rev_off(units[u].n_seg); }
    return o;
}

// one event of a run boundary into the window [w0, w0 + wn) of the difference arrays (begin: the cell begins a run, else it ends one)
AMBI_HD void profile_post(int32_t* df, int32_t* dr, int w0, int wn, int c, bool begin) {
    if (c == 0) return;
    int32_t* d = c > 0 ? df : dr;
    const int idx = c > 0 ? (begin ? c : c + 1) : (begin ? -c + 1 : -c);
    const int j = idx - w0;
    if (j < 0 || j >= wn) return;   // another window's event, or index n + 1 (never read)
    atomic_add_i32(d + j, (c > 0) == begin ? 1 : -1);
}

// cells: the unit's path as the result blob holds it (local signed ids), P > 0 cells, readable up to the next multiple of four
// cells; target_cn / seg_cn: the unit's arrays of the blob (slot 0 unused); bins: group memory, profile_bins_bytes(window);
// out_fwd / out_rev: n + 1 counts each; out: every field but `status`.  Whole group.
template <class G>
AMBI_HD void stage_path_profile(const G& g, const rcell_t* cells, int P, int n, const int32_t* target_cn, const double* seg_cn, int window,
                                int32_t* bins, int32_t* out_fwd, int32_t* out_rev, UnitProfile* out) {
    int32_t* df = bins;
    int32_t* dr = bins + window;
    const int tid = g.tid(), sz = g.size();
    const bool vec = (reinterpret_cast<uintptr_t>(cells) & 7) == 0;
    int runs = 0, turns = 0, max_cn = 0, n_unc = 0, n_off_t = 0, n_off_in = 0;
    int64_t l1 = 0;
    int carry_f = 0, carry_r = 0;
    if (tid == 0) { out_fwd[0] = 0; out_rev[0] = 0; }
    for (int w0 = 1; w0 <= n; w0 += window) {
        const int wn = n - w0 + 1 < window ? n - w0 + 1 : window;
        const bool first = w0 == 1;   // runs and turns are counted once
        for (int j = tid; j < wn; j += sz) { df[j] = 0; dr[j] = 0; }
        g.sync();
        // the boundaries (i - 1, i) of a thread's chunk [s, s + kProfileChunk) need c[s - 1] besides the chunk: one extra cell
        for (int base = 0; base < P; base += sz * kProfileChunk) {
            const int s = base + tid * kProfileChunk;
            if (s >= P) continue;
            rcell_t c[kProfileChunk];
            int prev;
            const int e = path_load_chunk(cells, P, vec, s, c, prev);
            for (int k = 0; k < e; k++) {
                const int cur = c[k];
                if (s + k == 0) { profile_post(df, dr, w0, wn, cur, true); runs += first; }
                else if (cur != prev + 1) {
                    profile_post(df, dr, w0, wn, prev, false);
                    profile_post(df, dr, w0, wn, cur, true);
                    if (first) { runs++; turns += cur == -prev; }
                }
                prev = cur;
            }
            if (s + e == P) profile_post(df, dr, w0, wn, prev, false);   // the last cell of the path ends its run
        }
        g.sync();
        // counts of the window: inclusive prefix sums, tile by tile, on top of what the windows before left
        for (int base = 0; base < wn; base += sz) {
            const int j = base + tid;
            const int vf = j < wn ? df[j] : 0, vr = j < wn ? dr[j] : 0;
            int tf, tr;
            const int ef = g.exscan_i32(vf, &tf), er = g.exscan_i32(vr, &tr);
            if (j < wn) {
                const int seg = w0 + j, f = carry_f + ef + vf, r = carry_r + er + vr, t = f + r;
                out_fwd[seg] = f; out_rev[seg] = r;
                if (t > max_cn) max_cn = t;
                n_unc += t == 0;
                const int dt = t - target_cn[seg];
                n_off_t += dt != 0;
                l1 += dt < 0 ? -(int64_t)dt : (int64_t)dt;
                const double di = (double)t - seg_cn[seg];
                n_off_in += (di < 0 ? -di : di) >= 0.5;
            }
            carry_f += tf; carry_r += tr;
        }
        g.sync();   // the arrays are cleared for the next window
    }
    runs = g.sum_i32(runs); turns = g.sum_i32(turns); max_cn = g.max_i32(max_cn);
    n_unc = g.sum_i32(n_unc); n_off_t = g.sum_i32(n_off_t); n_off_in = g.sum_i32(n_off_in);
    // 64-bit sum out of two 32-bit ones: the low 20 bits of up to 1024 threads stay below 2^30
    const int lo = g.sum_i32((int)(l1 & 0xFFFFF)), hi = g.sum_i32((int)(l1 >> 20));
    if (tid == 0) {
        out->cells = P; out->runs = runs; out->turns = turns; out->max_cn = max_cn;
        out->n_uncovered = n_unc; out->n_off_target = n_off_t; out->n_off_input = n_off_in;
        out->l1_target = ((int64_t)hi << 20) + lo;
    }
}

// One unit of a batch: profiles the path ambi_batch_unit_path(unit, which) returns (profile_path) into the profile block.  SHORTCUT
// and INFEASIBLE units, whose path is 1+..n+, like any other; a unit with a negative status or without a path gets zero counts
// and a summary that is zero but for the status.  Whole group.
template <class G>
AMBI_HD void profile_unit(const G& g, const UnitIn* units, const uint8_t* results, int u, int which, int window, int32_t* bins,
                          uint8_t* block, const int64_t* off) {
    const UnitIn& U = units[u];
    const UnitLayout L = unit_layout(U.n_seg, U.bkp_cap, U.path_cap, U.out_cap);
    const uint8_t* r = results + U.res_off;
    const int n = U.n_seg;
    const ProfilePath Q = profile_path(units, results, u, which);
    int32_t* fwd = reinterpret_cast<int32_t*>(block + off[u]);
    int32_t* rev = reinterpret_cast<int32_t*>(block + off[u] + profile_rev_off(n));
    UnitProfile* out = reinterpret_cast<UnitProfile*>(block) + u;
    if (Q.P == 0) {
        for (int i = g.tid(); i <= n; i += g.size()) { fwd[i] = 0; rev[i] = 0; }
        if (g.tid() == 0) { UnitProfile z{}; z.status = Q.status; *out = z; }
        return;
    }
    stage_path_profile(g, Q.cells, Q.P, n, reinterpret_cast<const int32_t*>(r + L.target_cn), reinterpret_cast<const double*>(r + L.seg_cn), window,
                       bins, fwd, rev, out);
    if (g.tid() == 0) out->status = Q.status;
}

}  // namespace ambi
