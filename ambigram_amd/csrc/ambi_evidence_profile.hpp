// ambi_evidence_profile.hpp -- evidence depth profile of a unit's path: how many occurrences of the unit's .juncs fragments lie over
// every step of the path, and which junction traversals no fragment spans.
//
// The fragment profile (ambi_frag_profile.hpp) answers per fragment ("this read occurs twice"), the junction profile
// (ambi_junc_profile.hpp) per junction ("taken three times").  The question in between -- which parts of the printed path are backed
// by evidence, and which traversal of a junction is not -- needs the two joined per STEP.  The reference never checks a path against
// the chains (readComponents, LocalGenomicMap.cpp:5096-5156, cuts them into unordered id sets).  Everything is an exact integer;
// nothing depends on the order of a reduction:
//   step k            (c[k], c[k+1]), k = 0 .. P-2; an occurrence at i of a pattern of L cells covers the steps i .. i+L-2
//   depth[k]          occurrences, over all fragments and both directions (ambi_frag_profile.hpp: f and rc(f), a palindrome once),
//                     that cover step k
//   count[j]          steps credited to junction j, by the rule of ambi_junc_profile.hpp (edge A or B, lowest index wins)
//   covered[j]        credited steps with depth > 0;   min_depth[j]: the minimum of depth over the credited steps, -1 if none
//   UnitEvidenceProfile   status, steps, covered steps, max depth, first uncovered step, longest uncovered stretch and its start,
//                     junctions, used / fully covered / never covered junctions, covered steps of no junction, sum of depth
//
// Two stages, two launches:
//   stage_evidence_mark   zeroes the unit's depth area over P entries (the area is reused: it holds the last request's values), runs
//       the fragment profile's windowed match (frag_window_build / frag_window_sweep: the same table of first steps with chains, the
//       same cell-by-cell verification, the same i + L > P rejection) and, on every verified occurrence, adds +1 at depth[i] and -1
//       at depth[i + L - 1] with DEVICE-memory integer atomics whose value is not used.  Integer adds commute: the difference array
//       does not depend on arrival order.  The plain zero stores are in front of the atomics by the group's barrier.  The atomics
//       are what this stage costs over the fragment profile's (profiles/r22_notes.md).
//   stage_evidence_scan   in a SEPARATE launch behind the first -- the kernel boundary makes the atomics' results visible to plain
//       loads; the two are not fused, because a CU's vector L1 is not refreshed by atomics that went to L2 --: an inclusive scan of
//       the difference array in place, in sweeps of size() x kProfileChunk steps with a carry between sweeps (depth[k] holds the
//       depth for k < P - 1 behind it; entry P - 1 ends at 0); covered steps, max, sum and first uncovered step in the same sweep; the
//       longest zero stretch as an associative combine of (start, steps, leading zeros, trailing zeros, best length, best start) over
//       the threads' chunks (a tree in thread order through group memory), carried across sweeps, the smallest start winning ties.
//       Then the junction table of ambi_junc_profile.hpp in group memory (one slot per edge class: lds_claim / lds_find, junc_canon,
//       partitions of the key space, doubled when one does not fit) with three values per slot -- steps, covered steps, minimum
//       depth: group-memory add, add and min -- and EVERY step probed with depth[k] beside its cells.  (The junction profile counts
//       the in-run steps through a difference array over the segments; a depth per step leaves no such shortcut, so this stage has no
//       segment window.)  A step is unmatched when no slot holds its class; the partition that owns the class decides that.
//
// Limits.  depth is int32.  A pattern of L cells has at most L - 1 occurrences over one step, so depth[k] <= 2 * (fragment cells - F)
// of the unit; a request is refused when that bound reaches 2^31 (evidence_depth_overflows; AMBI_ERR_TOO_LARGE).
//
// SPMD over the group policies of ambi_group.hpp: BlockGroup in ambi_evidence_mark_kernel / ambi_evidence_scan_kernel, HostGroup in
// Backend::profile's default (the host simulation) and in tests/tools/evidence_profile_stage_check.cpp.
#pragma once
#include <vector>

#include "ambi_batch.hpp"
#include "ambi_frag_profile.hpp"
#include "ambi_group.hpp"
#include "ambi_junc_profile.hpp"
#include "ambi_profile.hpp"

namespace ambi {

// per-unit summary; the layout of ambi_unit_evidence_profile_t (include/ambigram_hip.h)
struct UnitEvidenceProfile {
    int32_t status;                // the unit's status, copied
    int32_t steps;                 // P - 1 of the profiled path
    int32_t steps_covered;         // steps with depth > 0
    int32_t max_depth;             // max over k of depth[k]
    int32_t first_uncovered;       // smallest k with depth[k] == 0, -1 if none
    int32_t longest_uncovered;     // steps of the longest stretch of consecutive steps with depth 0
    int32_t longest_uncovered_at;  // the smallest start of such a stretch, -1 if none
    int32_t juncs;                 // m
    int32_t juncs_used;            // junctions with count > 0
    int32_t juncs_covered;         // ... with count > 0 and covered == count
    int32_t juncs_uncovered;       // ... with count > 0 and covered == 0
    int32_t unmatched_covered;     // steps credited to no junction that have depth > 0
    int64_t depth_sum;             // sum over k of depth[k]
};
static_assert(sizeof(UnitEvidenceProfile) == 56, "UnitEvidenceProfile is ambi_unit_evidence_profile_t");

// the depth bound of a unit with `frag_cells` fragment cells in F fragments reaches 2^31: the request is refused
AMBI_HD bool evidence_depth_overflows(int64_t frag_cells, int64_t F) { return 2 * (frag_cells - F) >= (int64_t(1) << 31); }

// Junctions per pass: the junction profile's rule (AMBI_JPROFILE_JUNC_WINDOW shrinks it here too), capped at half its cap: a slot
// holds 20 bytes here (key, lowest index, steps, covered steps, minimum depth), two slots per junction, so the table takes at most
// 40 KB and, with the stretch descriptors of the group (24 bytes per thread), stays below the 64 KB a launch gets without raising
// the function's ceiling.
constexpr int kEvidenceJuncWindowCap = 1024;
AMBI_HD int evidence_junc_window(int max_m, int asked) { return capped_window(max_m, kEvidenceJuncWindowCap, asked); }
AMBI_HD int64_t evidence_scan_lds_bytes(int slots, int threads) { return int64_t(20) * slots + int64_t(24) * threads; }

// Evidence profile block: [UnitEvidenceProfile[U]] [per unit: count i32 (m), covered i32 (m), min_depth i32 (m)], every array on a
// 16-byte boundary and padded to 16 bytes.  off[u] = byte offset of unit u's count; covered and min_depth follow at
// evidence_arr_bytes(m) each.
AMBI_HD int64_t evidence_arr_bytes(int m) { return pad16(int64_t(4) * m); }
inline int64_t evidence_block_layout(const std::vector<UnitIn>& units, std::vector<int64_t>& off) {
    int64_t o = pad16(int64_t(sizeof(UnitEvidenceProfile)) * (int64_t)units.size());
    off.resize(units.size());
    for (size_t u = 0; u < units.size(); u++) { off[u] = o; o += 3 * evidence_arr_bytes(units[u].n_junc); }
    return o;
}
// Depth area: 4 bytes per cell of every unit's path capacity, each unit's slice padded to 16 bytes (about as large as the two path
// areas of the result blob together).  off[u] = byte offset of unit u's slice.  It stays on the device.
inline int64_t evidence_depth_layout(const std::vector<UnitIn>& units, std::vector<int64_t>& off) {
    int64_t o = 0;
    off.resize(units.size());
    for (size_t u = 0; u < units.size(); u++) { off[u] = o; o += pad16(int64_t(4) * units[u].path_cap); }
    return o;
}


// ---- stage 1: the difference array ----
// cells: the unit's path (local signed ids), P > 0 cells, readable up to the next multiple of four cells; fc / foff: the unit's F
// fragments; T: group memory (frag_profile_lds_bytes); depth: P entries.  Whole group.
template <class G>
AMBI_HD void stage_evidence_mark(const G& g, const rcell_t* cells, int P, const rcell_t* fc, const int32_t* foff, int F, const FragTable& T,
                                 int32_t* depth) {
    const int tid = g.tid(), sz = g.size();
    const bool vec = (reinterpret_cast<uintptr_t>(cells) & 7) == 0;
    for (int i = tid; i < P; i += sz) depth[i] = 0;
    g.sync();
    const int NP = 2 * F;
    for (int w0 = 0; w0 < NP; w0 += T.pwin) {
        const int wn = NP - w0 < T.pwin ? NP - w0 : T.pwin;
        // a match covers the steps i .. i + L - 2 (i + L - 1 <= P - 1: the sweep rejects i + L > P)
        if (frag_window_build(g, P, fc, foff, w0, wn, T))
            frag_window_sweep(g, cells, P, vec, fc, foff, w0, T, [depth](int, int i, int L) { (void)atomic_add_i32(depth + i, 1); (void)atomic_add_i32(depth + i + L - 1, -1); });
        g.sync();   // the table is cleared for the next window
    }
}

// ---- stage 2: depth, summary, junctions ----
// a stretch of consecutive steps [start, start + len): its leading and trailing zeros and the longest zero stretch inside (best
// steps at `at`, the smallest start; 0 at -1: none)
struct ZeroRuns { int32_t start, len, lead, trail, best, at; };
AMBI_HD ZeroRuns zero_runs_empty(int start) { return ZeroRuns{start, 0, 0, 0, 0, -1}; }
// A in front of B (B.start == A.start + A.len); associative
AMBI_HD ZeroRuns zero_runs_combine(const ZeroRuns& A, const ZeroRuns& B) {
    ZeroRuns R;
    R.start = A.start; R.len = A.len + B.len;
    R.lead = A.lead == A.len ? A.len + B.lead : A.lead;
    R.trail = B.trail == B.len ? B.len + A.trail : B.trail;
    R.best = A.best; R.at = A.at;
    const int mid = A.trail + B.lead;                        // the stretch across the seam starts inside A or at the seam
    if (mid > R.best) { R.best = mid; R.at = A.start + A.len - A.trail; }
    if (B.best > R.best) { R.best = B.best; R.at = B.at; }   // (ties stay with the earlier start)
    return R;
}
AMBI_HD ZeroRuns zero_runs_push(const ZeroRuns& A, bool zero) {   // one more step behind A
    const int k = A.start + A.len;
    return zero_runs_combine(A, zero ? ZeroRuns{k, 1, 1, 1, 1, k} : ZeroRuns{k, 1, 0, 0, 0, -1});
}

// the junction table and the group's stretch descriptors in group memory (evidence_scan_lds_bytes)
struct EvidenceTable {
    uint32_t* key;   // [slots] canonical key, 0 = empty
    int32_t* val;    // [slots] lowest junction index of the class
    int32_t* cnt;    // [slots] steps of the class
    int32_t* cov;    // [slots] ... with depth > 0
    int32_t* mind;   // [slots] minimum depth over them
    ZeroRuns* runs;  // [threads]
    int slots;
};
AMBI_HD EvidenceTable evidence_table(void* lds, int slots) {
    EvidenceTable T;
    int32_t* w = reinterpret_cast<int32_t*>(lds);
    T.key = reinterpret_cast<uint32_t*>(w); T.val = w + slots; T.cnt = w + 2 * slots; T.cov = w + 3 * slots; T.mind = w + 4 * slots;
    T.runs = reinterpret_cast<ZeroRuns*>(w + 5 * slots);
    T.slots = slots;
    return T;
}

struct EvidenceInt4 { int32_t v[4]; } __attribute__((aligned(16)));
// a thread's chunk [s, s + kProfileChunk) of the depth array, zero behind P; two 16-byte words when the chunk lies inside the array
// (s is a multiple of the chunk and the unit's slice lies on a 16-byte boundary)
AMBI_HD void evidence_load_chunk(const int32_t* depth, int P, bool vec, int s, int32_t (&d)[kProfileChunk]) {
    if (vec && s + kProfileChunk <= P) {
        for (int q = 0; q < kProfileChunk / 4; q++) {
            const EvidenceInt4 w = *reinterpret_cast<const EvidenceInt4*>(depth + s + 4 * q);
            for (int k = 0; k < 4; k++) d[4 * q + k] = w.v[k];
        }
    } else for (int k = 0; k < kProfileChunk; k++) d[k] = s + k < P ? depth[s + k] : 0;
}
AMBI_HD void evidence_store_chunk(int32_t* depth, int P, bool vec, int s, const int32_t (&d)[kProfileChunk]) {
    if (vec && s + kProfileChunk <= P) {
        for (int q = 0; q < kProfileChunk / 4; q++) {
            EvidenceInt4 w;
            for (int k = 0; k < 4; k++) w.v[k] = d[4 * q + k];
            *reinterpret_cast<EvidenceInt4*>(depth + s + 4 * q) = w;
        }
    } else for (int k = 0; k < kProfileChunk; k++) if (s + k < P) depth[s + k] = d[k];
}

// cells: the unit's path, P > 0 cells (as above); ends: the unit's m junctions; jwin: junctions a pass is sized for; T: group
// memory; depth: P entries, the difference array of stage_evidence_mark on entry, the depths behind it; out_count / out_covered /
// out_min: m values each; out: every field but `status`.  Whole group.
template <class G>
AMBI_HD void stage_evidence_scan(const G& g, const rcell_t* cells, int P, const JuncEnds* ends, int m, int jwin, const EvidenceTable& T,
                                 int32_t* depth, int32_t* out_count, int32_t* out_covered, int32_t* out_min, UnitEvidenceProfile* out) {
    const int tid = g.tid(), sz = g.size();
    const bool vec = (reinterpret_cast<uintptr_t>(cells) & 7) == 0;
    const bool dvec = (reinterpret_cast<uintptr_t>(depth) & 15) == 0;
    const int kNone = 0x7fffffff;
    const int steps = P - 1;
    // the scan: depth in place, the step statistics and the zero stretches
    int covered = 0, max_depth = 0, first_unc = kNone, carry = 0;
    int64_t sum = 0;
    ZeroRuns all = zero_runs_empty(0);
    for (int base = 0; base < P; base += sz * kProfileChunk) {
        const int s = base + tid * kProfileChunk;
        int32_t d[kProfileChunk];
        int mine = 0;
        if (s < P) {
            evidence_load_chunk(depth, P, dvec, s, d);
            for (int k = 0; k < kProfileChunk; k++) { mine += d[k]; d[k] = mine; }   // inclusive inside the chunk
        }
        int tot;
        const int before = carry + g.exscan_i32(mine, &tot);
        ZeroRuns R = zero_runs_empty(s < steps ? s : (steps > 0 ? steps : 0));
        if (s < P) {
            for (int k = 0; k < kProfileChunk; k++) {
                d[k] += before;
                if (s + k < steps) {
                    const int x = d[k];
                    covered += x > 0;
                    if (x > max_depth) max_depth = x;
                    sum += x;
                    if (x == 0 && s + k < first_unc) first_unc = s + k;
                    R = zero_runs_push(R, x == 0);
                }
            }
            evidence_store_chunk(depth, P, dvec, s, d);
        }
        carry += tot;
        // the sweep's stretches: a tree in thread order
        T.runs[tid] = R;
        g.sync();
        for (int st = 1; st < sz; st <<= 1) {
            if ((tid & (2 * st - 1)) == 0 && tid + st < sz) T.runs[tid] = zero_runs_combine(T.runs[tid], T.runs[tid + st]);
            g.sync();
        }
        all = zero_runs_combine(all, T.runs[0]);
        g.sync();   // (the descriptors are written again in the next sweep; the depths are read by other threads below)
    }
    covered = g.sum_i32(covered); max_depth = g.max_i32(max_depth); first_unc = g.min_i32(first_unc);
    int64_t sum_all;
    (void)g.exscan_i64(sum, &sum_all);

    // the junctions: every step against the classes of its partition
    int nparts = jwin > 0 ? (m + jwin - 1) / jwin : 1;
    if (nparts < 1) nparts = 1;
    int used, full_cov, none_cov, unmatched_cov;
    for (;;) {
        used = 0; full_cov = 0; none_cov = 0; unmatched_cov = 0;
        bool full = false;
        for (int part = 0; part < nparts && !full; part++) {
            for (int s = tid; s < T.slots; s += sz) { T.key[s] = 0; T.val[s] = kNone; T.cnt[s] = 0; T.cov[s] = 0; T.mind[s] = kNone; }
            g.sync();
            bool mine_full = false;
            for (int j = tid; j < m; j += sz) {
                const JuncEnds E = ends[j];
                const uint32_t canon = junc_canon(E.s, E.t);
                if (!junc_in_part(canon, nparts, part)) continue;
                const int slot = lds_claim(T.key, T.slots, canon);
                if (slot >= 0) atomic_min_i32(T.val + slot, j); else mine_full = true;
            }
            if (g.any(mine_full)) { full = true; break; }   // (any: a barrier; the table is complete behind it)
            for (int base = 0; base < P; base += sz * kProfileChunk) {
                const int s = base + tid * kProfileChunk;
                if (s >= P) continue;
                rcell_t c[kProfileChunk];
                int32_t d[kProfileChunk];
                int prev;
                const int e = path_load_chunk(cells, P, vec, s, c, prev);
                evidence_load_chunk(depth, P, dvec, s, d);
                int dprev = s > 0 ? depth[s - 1] : 0;       // the depth of the step in front of the chunk
                for (int k = 0; k < e; k++) {
                    const int cur = c[k];
                    if (s + k > 0) {                        // the step (c[i], c[i + 1]), i = s + k - 1, with depth dprev
                        const uint32_t canon = junc_canon(prev, cur);
                        if (junc_in_part(canon, nparts, part)) {
                            const int slot = lds_find(T.key, T.slots, canon);
                            if (slot >= 0) {
                                (void)atomic_add_i32(T.cnt + slot, 1);
                                if (dprev > 0) (void)atomic_add_i32(T.cov + slot, 1);
                                atomic_min_i32(T.mind + slot, dprev);
                            } else unmatched_cov += dprev > 0;
                        }
                    }
                    prev = cur; dprev = d[k];
                }
            }
            g.sync();
            // this partition's junctions: the winner of a class takes the slot's values
            for (int j = tid; j < m; j += sz) {
                const JuncEnds E = ends[j];
                const uint32_t canon = junc_canon(E.s, E.t);
                if (!junc_in_part(canon, nparts, part)) continue;
                const int slot = lds_find(T.key, T.slots, canon);
                const bool won = slot >= 0 && T.val[slot] == j;
                const int c = won ? T.cnt[slot] : 0, v = won ? T.cov[slot] : 0;
                out_count[j] = c; out_covered[j] = v; out_min[j] = c > 0 ? T.mind[slot] : -1;
                used += c > 0; full_cov += c > 0 && v == c; none_cov += c > 0 && v == 0;
            }
            g.sync();   // the table is cleared for the next partition
        }
        if (!full) break;
        nparts *= 2;   // (ends as in stage_junc_profile)
    }
    used = g.sum_i32(used); full_cov = g.sum_i32(full_cov); none_cov = g.sum_i32(none_cov); unmatched_cov = g.sum_i32(unmatched_cov);
    if (tid == 0) {
        out->steps = steps; out->steps_covered = covered; out->max_depth = max_depth; out->first_uncovered = first_unc == kNone ? -1 : first_unc;
        out->longest_uncovered = all.best; out->longest_uncovered_at = all.at;
        out->juncs = m; out->juncs_used = used; out->juncs_covered = full_cov; out->juncs_uncovered = none_cov;
        out->unmatched_covered = unmatched_cov; out->depth_sum = sum_all;
    }
}

// ---- one unit of a batch ----
// Both profile the path ambi_batch_unit_path(unit, which) returns (profile_path).  SHORTCUT and INFEASIBLE units like any other; a
// unit with a negative status or without a path gets zero counts, min_depth = -1 and a summary that is zero but for the status, the
// number of junctions and first_uncovered = longest_uncovered_at = -1; its depth area is not touched.  Whole group.
template <class G>
AMBI_HD void evidence_mark_unit(const G& g, const UnitIn* units, const FragArgs& I, const uint8_t* results, int u, int which, const FragTable& T,
                                uint8_t* depth_area, const int64_t* depth_off) {
    const ProfilePath Q = profile_path(units, results, u, which);
    if (Q.P == 0) return;
    stage_evidence_mark(g, Q.cells, Q.P, I.cells + I.cell_off[u], I.frag_off + I.pref_off[u], I.n_frag[u], T,
                        reinterpret_cast<int32_t*>(depth_area + depth_off[u]));
}
template <class G>
AMBI_HD void evidence_scan_unit(const G& g, const UnitIn* units, const JuncEnds* junc_ends, const uint8_t* results, int u, int which, int jwin,
                                const EvidenceTable& T, uint8_t* depth_area, const int64_t* depth_off, uint8_t* block, const int64_t* off) {
    const UnitIn& U = units[u];
    const int m = U.n_junc;
    const ProfilePath Q = profile_path(units, results, u, which);
    const int64_t arr = evidence_arr_bytes(m);
    int32_t* count = reinterpret_cast<int32_t*>(block + off[u]);
    int32_t* covered = reinterpret_cast<int32_t*>(block + off[u] + arr);
    int32_t* min_depth = reinterpret_cast<int32_t*>(block + off[u] + 2 * arr);
    UnitEvidenceProfile* out = reinterpret_cast<UnitEvidenceProfile*>(block) + u;
    if (Q.P == 0) {
        for (int j = g.tid(); j < m; j += g.size()) { count[j] = 0; covered[j] = 0; min_depth[j] = -1; }
        if (g.tid() == 0) { UnitEvidenceProfile z{}; z.status = Q.status; z.juncs = m; z.first_uncovered = -1; z.longest_uncovered_at = -1; *out = z; }
        return;
    }
    stage_evidence_scan(g, Q.cells, Q.P, junc_ends + U.junc_off, m, jwin, T, reinterpret_cast<int32_t*>(depth_area + depth_off[u]), count, covered,
                        min_depth, out);
    if (g.tid() == 0) out->status = Q.status;
}

}  // namespace ambi
