// ambi_fold_profile.hpp -- fold-back arm profile of a unit's path: where the path folds back, how long the reverse-complement
// palindrome around every fold is, and how deeply the palindromes nest.
//
// What makes a path a breakage-fusion-bridge path is its nested palindromes: every cycle folds the chromosome back at a fold-back
// inversion and duplicates an arm (printBFB prints `|` at every such step).  UnitProfile::turns (ambi_profile.hpp) counts the steps
// with c[i+1] == -c[i] and says nothing about arm lengths, imperfect fold-backs or nesting.  Everything here is an exact integer;
// nothing depends on the order of a reduction.  With the cells c[0..P) and the steps k = 0 .. P-2:
//   fold              a step whose two cells have opposite sign
//   alignment a       0..4 with (dl, dr) = (0,1) (-1,1) (0,2) (-2,1) (0,3): the perfect fold-back, then one or two unpaired cells on
//                     the left or on the right (the reference's fold-back test allows |i - j| <= 2, LocalGenomicMap.cpp:4012).
//                     With i = k + dl and j = k + dr, arm_a is the largest r >= 0 with i-t >= 0, j+t < P and c[i-t] == -c[j+t] for
//                     all t < r; 0 when i < 0 or j >= P
//   a fold's alignment and arm   the smallest a with arm_a > 0 and that arm; alignment -1 and arm 0 when there is none
//   span              a fold with arm r > 0 covers the steps i-r+1 .. j+r-2 (k is always among them)
//   cover[s]          folds whose span covers step s; the nesting of a fold at k is cover[k] - 1
//   folds[j]          folds credited to junction j by the rule of ambi_junc_profile.hpp (edge A or B, lowest index wins)
//   max_arm[j]        the longest arm among them, 0 when there are none
// Two int32 planes of P entries stay where they were computed: fold[k] = 0 for a step that is no fold, else
// (alignment + 2) << 24 | arm (fold_arm / fold_align below); cover[k].
//
// Two stages, two launches:
//   stage_fold_arms   zeroes both planes over P entries (the planes are reused: they hold the last request's values).  Then, in
//       rounds of `fwin` folds (a unit with more folds takes further rounds; nothing is dropped): the cells are swept with
//       path_load_chunk, a scan of the threads' fold counts numbers the folds in path order and those of the round go into the list
//       in group memory.  A per-lane pre-pass, one thread per fold, picks the alignment from the six cells around the fold and
//       compares the first kFoldHandover pairs of its arm -- every load of it is independent of the others, out-of-range cells read
//       as 0, which no cell is.  The short arms end there.  An arm that is still open after kFoldHandover pairs is handed to a whole
//       sub-group (a wavefront): 64 pairs per round, the left side read descending, the right ascending, and a ballot finds the
//       first mismatch; the loads of a round do not depend on one another (profiles/r20_notes.md: what a chain of dependent cell
//       loads cost the fragment profile).  A thread per fold would leave a wavefront waiting on one lane for thousands of
//       dependent 2-byte loads: folds are few (about 1 % of the steps) and the outermost arm is about P / 2.  Then fold[k] is
//       written and the span's ends go into `cover` as +1 / -1 with DEVICE-memory integer atomics whose value is not used.  The
//       plain zero stores are in front of the atomics by the group's barrier.  Nothing is read at or behind P: cells there are stale.
//   stage_fold_scan   in a SEPARATE launch behind the first, for the reason ambi_evidence_profile.hpp gives (a CU's vector L1 is not
//       refreshed by atomics that went to L2; the kernel boundary makes them visible to plain loads): an inclusive scan of `cover`
//       in place (entry P - 1 ends at 0), the summary in the same sweep (maxima with the smallest index: a thread keeps its first
//       maximum, the group takes the maximum and then the smallest index that has it), and the folds -- not every step -- probed
//       against the junction table of ambi_junc_profile.hpp (lds_claim / lds_find, partitions of the key space) with a count and a
//       maximum per slot.
//
// Limits.  An arm is below P / 2 + 1 <= 2^22 (a path has at most 4 M cells), so it fits the low 24 bits of fold[k].
//
// SPMD over the group policies of ambi_group.hpp: BlockGroup in ambi_fold_arm_kernel / ambi_fold_scan_kernel, HostGroup in
// Backend::profile's default (the host simulation) and in tests/tools/fold_profile_stage_check.cpp.
#pragma once
#include <vector>

#include "ambi_batch.hpp"
#include "ambi_evidence_profile.hpp"
#include "ambi_group.hpp"
#include "ambi_junc_profile.hpp"
#include "ambi_profile.hpp"

namespace ambi {

// per-unit summary; the layout of ambi_unit_fold_profile_t (include/ambigram_hip.h)
struct UnitFoldProfile {
    int32_t status;           // the unit's status, copied
    int32_t steps;            // P - 1 of the profiled path
    int32_t folds;            // steps whose two cells have opposite sign
    int32_t folds_perfect;    // folds with alignment 0
    int32_t folds_gapped;     // ... 1..4
    int32_t folds_open;       // ... -1 (no arm)
    int32_t folds_unmatched;  // folds credited to no junction
    int32_t max_arm;          // the longest arm
    int32_t max_arm_at;       // the smallest k of a fold with that arm, -1 if max_arm == 0
    int32_t max_cover;        // max over the steps of cover
    int32_t max_cover_at;     // the smallest step with that cover, -1 if max_cover == 0
    int32_t steps_covered;    // steps with cover > 0
    int64_t arm_sum;          // sum of the arms of all folds
};
static_assert(sizeof(UnitFoldProfile) == 56, "UnitFoldProfile is ambi_unit_fold_profile_t");

// fold[k]: (alignment + 2) << 24 | arm; AMBI_FOLD_ARM / AMBI_FOLD_ALIGN of the C header
constexpr int kFoldArmMask = 0xffffff;
AMBI_HD int fold_pack(int align, int arm) { return ((align + 2) << 24) | arm; }
AMBI_HD int fold_arm(int v) { return v & kFoldArmMask; }
AMBI_HD int fold_align(int v) { return (v >> 24) - 2; }
constexpr int kFoldAligns = 5;
AMBI_HD int fold_dl(int a) { return a == 1 ? -1 : a == 3 ? -2 : 0; }
AMBI_HD int fold_dr(int a) { return a == 2 ? 2 : a == 4 ? 3 : 1; }

// The hand-over length: the per-lane pre-pass compares this many pairs of an arm (pair 0 is among the six cells that pick the
// alignment, so 2 x 7 independent 2-byte loads beside those six); an arm that is still open behind them goes to a whole sub-group.  It ends about half the arms
// of random decompositions and few of the synthetic tiers', whose arms are tens of cells and longer (profiles/r24_notes.md).
constexpr int kFoldHandover = 8;
constexpr int kFoldOpenBit = 1 << 30;   // list entry: the arm is still open after the pre-pass

// Folds per round: 8 bytes of group memory each (step, packed value); AMBI_FOLD_WINDOW (tests) can only shrink it.  Junctions per
// pass of the scan stage: the junction profile's rule (AMBI_JPROFILE_JUNC_WINDOW shrinks it here too), capped at half its cap: a
// slot holds 16 bytes here (key, lowest index, folds, longest arm), two slots per junction, 32 KB at most.
constexpr int kFoldWindowCap = 2048, kFoldJuncWindowCap = 1024;
AMBI_HD int fold_window(int asked) { return capped_window(kFoldWindowCap, kFoldWindowCap, asked); }
AMBI_HD int fold_junc_window(int max_m, int asked) { return capped_window(max_m, kFoldJuncWindowCap, asked); }
AMBI_HD int64_t fold_arm_lds_bytes(int fwin) { return int64_t(8) * fwin; }
AMBI_HD int64_t fold_scan_lds_bytes(int slots) { return int64_t(16) * slots; }

// Fold profile block: [UnitFoldProfile[U]] [per unit: folds i32 (m), max_arm i32 (m)], every array on a 16-byte boundary and padded
// to 16 bytes.  off[u] = byte offset of unit u's folds; max_arm follows at fold_arr_bytes(m).
AMBI_HD int64_t fold_arr_bytes(int m) { return pad16(int64_t(4) * m); }
inline int64_t fold_block_layout(const std::vector<UnitIn>& units, std::vector<int64_t>& off) {
    int64_t o = pad16(int64_t(sizeof(UnitFoldProfile)) * (int64_t)units.size());
    off.resize(units.size());
    for (size_t u = 0; u < units.size(); u++) { off[u] = o; o += 2 * fold_arr_bytes(units[u].n_junc); }
    return o;
}
// Plane area: two planes, the fold plane of every unit and behind them the cover plane of every unit, each laid out as the evidence
// kind's depth area (4 bytes per cell of every unit's path capacity, a unit's slice padded to 16 bytes).  off[u] = byte offset of
// unit u's slice in a plane; returns the bytes of ONE plane.  The area stays on the device.
inline int64_t fold_plane_layout(const std::vector<UnitIn>& units, std::vector<int64_t>& off) { return evidence_depth_layout(units, off); }

// the round's folds in group memory (fold_arm_lds_bytes)
struct FoldList {
    int32_t* k;     // [fwin] the fold's step
    int32_t* val;   // [fwin] fold_pack(alignment, arm so far) | kFoldOpenBit
    int fwin;
};
AMBI_HD FoldList fold_list(void* lds, int fwin) {
    FoldList L;
    L.k = reinterpret_cast<int32_t*>(lds); L.val = L.k + fwin; L.fwin = fwin;
    return L;
}

// ---- stage 1: the arms ----
// cells: the unit's path (local signed ids), P > 0 cells, readable up to the next multiple of four cells; L: group memory;
// fold / cover: P entries each.  Whole group.
template <class G>
AMBI_HD void stage_fold_arms(const G& g, const rcell_t* cells, int P, const FoldList& L, int32_t* fold, int32_t* cover) {
    const int tid = g.tid(), sz = g.size();
    const bool vec = (reinterpret_cast<uintptr_t>(cells) & 7) == 0;
    const int fwin = L.fwin;
    // cell `at`, 0 outside the path (a cell is never 0: 0 equals no cell's complement)
    auto cell = [cells, P](int at) -> int { return at >= 0 && at < P ? (int)cells[at] : 0; };
    for (int i = tid; i < P; i += sz) { fold[i] = 0; cover[i] = 0; }
    g.sync();
    for (int w0 = 0;; w0 += fwin) {
        // the folds number w0 .. w0 + fwin - 1 in path order into the list
        int carry = 0;
        bool more = false;
        for (int base = 0; base < P; base += sz * kProfileChunk) {
            const int s = base + tid * kProfileChunk;
            rcell_t c[kProfileChunk];
            int prev = 0, e = 0, mine = 0;
            if (s < P) {
                e = path_load_chunk(cells, P, vec, s, c, prev);
                int p = prev;
                for (int q = 0; q < e; q++) { const int cur = c[q]; mine += s + q > 0 && (p ^ cur) < 0; p = cur; }
            }
            int tot;
            int ord = carry + g.exscan_i32(mine, &tot);
            if (mine > 0 && ord < w0 + fwin && ord + mine > w0) {
                int p = prev;
                for (int q = 0; q < e; q++) {
                    const int cur = c[q];
                    if (s + q > 0 && (p ^ cur) < 0) { if (ord >= w0 && ord < w0 + fwin) L.k[ord - w0] = s + q - 1; ord++; }
                    p = cur;
                }
            }
            carry += tot;
            if (carry >= w0 + fwin) { more = carry > w0 + fwin || base + sz * kProfileChunk < P; break; }   // (uniform: carry is)
        }
        g.sync();
        const int nf = (carry < w0 + fwin ? carry : w0 + fwin) - w0;
        // the pre-pass: alignment and the first kFoldHandover pairs, a thread per fold
        for (int f = tid; f < nf; f += sz) {
            const int k = L.k[f];
            int x[6];
            for (int q = 0; q < 6; q++) x[q] = cell(k - 2 + q);   // c[k-2 .. k+3]
            int a = -1;
            for (int q = kFoldAligns - 1; q >= 0; q--) { const int ci = x[2 + fold_dl(q)], cj = x[2 + fold_dr(q)]; if (ci != 0 && ci == -cj) a = q; }
            int v = fold_pack(-1, 0);
            if (a >= 0) {
                const int i = k + fold_dl(a), j = k + fold_dr(a);
                int lo[kFoldHandover], hi[kFoldHandover];
                for (int t = 1; t < kFoldHandover; t++) { lo[t] = cell(i - t); hi[t] = cell(j + t); }
                int r = 1;
                bool open = true;
                for (int t = 1; t < kFoldHandover; t++) { open = open && lo[t] != 0 && lo[t] == -hi[t]; r += open; }
                v = fold_pack(a, r) | (open ? kFoldOpenBit : 0);
            }
            L.val[f] = v;
        }
        g.sync();
        // the open arms: a sub-group each, sub_size() pairs per round
        {
            const int W = g.sub_size(), lane = g.sub_lane();
            for (int f = g.sub_id(); f < nf; f += g.n_subs()) {
                const int v = L.val[f];
                if (!(v & kFoldOpenBit)) continue;   // (uniform over the sub-group)
                const int k = L.k[f], a = fold_align(v & ~kFoldOpenBit), i = k + fold_dl(a), j = k + fold_dr(a);
                int r = fold_arm(v);
                for (;;) {
                    const int t = r + lane;
                    const int lo = cell(i - t), hi = cell(j + t);
                    const uint64_t stop = g.sub_ballot_u64(lo == 0 || lo != -hi);   // (ends: i - t < 0 at the latest)
                    if (stop) { r += (int)__builtin_ctzll(stop); break; }
                    r += W;
                }
                if (lane == 0) L.val[f] = fold_pack(a, r);
            }
        }
        g.sync();
        // fold[k], and the span's ends into the difference array
        for (int f = tid; f < nf; f += sz) {
            const int k = L.k[f], v = L.val[f], a = fold_align(v), r = fold_arm(v);
            fold[k] = v;
            if (r > 0) {   // the steps i-r+1 .. j+r-2: 0 <= i-r+1 and j+r-1 <= P-1 by the arm's definition
                (void)atomic_add_i32(cover + k + fold_dl(a) - r + 1, 1);
                (void)atomic_add_i32(cover + k + fold_dr(a) + r - 1, -1);
            }
        }
        g.sync();   // the list is written again in the next round
        if (!more) break;
    }
}

// ---- stage 2: cover, summary, junctions ----
// the junction table in group memory (fold_scan_lds_bytes)
struct FoldTable {
    uint32_t* key;   // [slots] canonical key, 0 = empty
    int32_t* val;    // [slots] lowest junction index of the class
    int32_t* cnt;    // [slots] folds of the class
    int32_t* arm;    // [slots] the longest arm among them
    int slots;
};
AMBI_HD FoldTable fold_table(void* lds, int slots) {
    FoldTable T;
    int32_t* w = reinterpret_cast<int32_t*>(lds);
    T.key = reinterpret_cast<uint32_t*>(w); T.val = w + slots; T.cnt = w + 2 * slots; T.arm = w + 3 * slots; T.slots = slots;
    return T;
}

// cells: the unit's path, P > 0 cells (as above); ends: the unit's m junctions; jwin: junctions a pass is sized for; T: group
// memory; fold: P entries as stage_fold_arms left them; cover: P entries, the difference array on entry, the covers behind it;
// out_folds / out_max: m values each; out: every field but `status`.  Whole group.
template <class G>
AMBI_HD void stage_fold_scan(const G& g, const rcell_t* cells, int P, const JuncEnds* ends, int m, int jwin, const FoldTable& T, const int32_t* fold,
                             int32_t* cover, int32_t* out_folds, int32_t* out_max, UnitFoldProfile* out) {
    const int tid = g.tid(), sz = g.size();
    const bool fvec = (reinterpret_cast<uintptr_t>(fold) & 15) == 0, cvec = (reinterpret_cast<uintptr_t>(cover) & 15) == 0;
    const int kNone = 0x7fffffff;
    const int steps = P - 1;
    // the scan: cover in place, and the statistics of steps and folds
    int covered = 0, max_cover = 0, max_cover_at = kNone, max_arm = 0, max_arm_at = kNone, folds = 0, perfect = 0, gapped = 0, carry = 0;
    int64_t sum = 0;
    for (int base = 0; base < P; base += sz * kProfileChunk) {
        const int s = base + tid * kProfileChunk;
        int32_t d[kProfileChunk], f[kProfileChunk];
        int mine = 0;
        if (s < P) {
            evidence_load_chunk(cover, P, cvec, s, d);
            evidence_load_chunk(fold, P, fvec, s, f);
            for (int k = 0; k < kProfileChunk; k++) { mine += d[k]; d[k] = mine; }   // inclusive inside the chunk
        }
        int tot;
        const int before = carry + g.exscan_i32(mine, &tot);
        if (s < P) {
            for (int k = 0; k < kProfileChunk; k++) {
                d[k] += before;
                if (s + k < steps) {
                    const int x = d[k], v = f[k];
                    covered += x > 0;
                    if (x > max_cover) { max_cover = x; max_cover_at = s + k; }
                    if (v != 0) {
                        const int a = fold_align(v), r = fold_arm(v);
                        folds++; perfect += a == 0; gapped += a > 0;
                        sum += r;
                        if (r > max_arm) { max_arm = r; max_arm_at = s + k; }
                    }
                }
            }
            evidence_store_chunk(cover, P, cvec, s, d);
        }
        carry += tot;
    }
    covered = g.sum_i32(covered); folds = g.sum_i32(folds); perfect = g.sum_i32(perfect); gapped = g.sum_i32(gapped);
    const int top_cover = g.max_i32(max_cover), top_arm = g.max_i32(max_arm);
    max_cover_at = g.min_i32(top_cover > 0 && max_cover == top_cover ? max_cover_at : kNone);
    max_arm_at = g.min_i32(top_arm > 0 && max_arm == top_arm ? max_arm_at : kNone);
    int64_t sum_all;
    (void)g.exscan_i64(sum, &sum_all);

    // the junctions: every fold against the classes of its partition
    int nparts = jwin > 0 ? (m + jwin - 1) / jwin : 1;
    if (nparts < 1) nparts = 1;
    int unmatched;
    for (;;) {
        unmatched = 0;
        bool full = false;
        for (int part = 0; part < nparts && !full; part++) {
            for (int s = tid; s < T.slots; s += sz) { T.key[s] = 0; T.val[s] = kNone; T.cnt[s] = 0; T.arm[s] = 0; }
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
                int32_t f[kProfileChunk];
                evidence_load_chunk(fold, P, fvec, s, f);
                for (int k = 0; k < kProfileChunk; k++) {
                    if (f[k] == 0 || s + k >= steps) continue;
                    const uint32_t canon = junc_canon(cells[s + k], cells[s + k + 1]);
                    if (!junc_in_part(canon, nparts, part)) continue;
                    const int slot = lds_find(T.key, T.slots, canon);
                    if (slot >= 0) { (void)atomic_add_i32(T.cnt + slot, 1); atomic_max_i32(T.arm + slot, fold_arm(f[k])); }
                    else unmatched++;
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
                out_folds[j] = won ? T.cnt[slot] : 0; out_max[j] = won ? T.arm[slot] : 0;
            }
            g.sync();   // the table is cleared for the next partition
        }
        if (!full) break;
        nparts *= 2;   // (ends as in stage_junc_profile)
    }
    unmatched = g.sum_i32(unmatched);
    if (tid == 0) {
        out->steps = steps; out->folds = folds; out->folds_perfect = perfect; out->folds_gapped = gapped; out->folds_open = folds - perfect - gapped;
        out->folds_unmatched = unmatched; out->max_arm = top_arm; out->max_arm_at = max_arm_at == kNone ? -1 : max_arm_at;
        out->max_cover = top_cover; out->max_cover_at = max_cover_at == kNone ? -1 : max_cover_at; out->steps_covered = covered;
        out->arm_sum = sum_all;
    }
}

// ---- one unit of a batch ----
// Both profile the path ambi_batch_unit_path(unit, which) returns (profile_path).  SHORTCUT and INFEASIBLE units like any other; a
// unit with a negative status or without a path gets zero counts and a summary that is zero but for the status and
// max_arm_at = max_cover_at = -1; its planes are not touched.  planes: the area, `plane_bytes` per plane.  Whole group.
template <class G>
AMBI_HD void fold_arms_unit(const G& g, const UnitIn* units, const uint8_t* results, int u, int which, const FoldList& L, uint8_t* planes,
                            int64_t plane_bytes, const int64_t* plane_off) {
    const ProfilePath Q = profile_path(units, results, u, which);
    if (Q.P == 0) return;
    stage_fold_arms(g, Q.cells, Q.P, L, reinterpret_cast<int32_t*>(planes + plane_off[u]), reinterpret_cast<int32_t*>(planes + plane_bytes + plane_off[u]));
}
template <class G>
AMBI_HD void fold_scan_unit(const G& g, const UnitIn* units, const JuncEnds* junc_ends, const uint8_t* results, int u, int which, int jwin,
                            const FoldTable& T, uint8_t* planes, int64_t plane_bytes, const int64_t* plane_off, uint8_t* block, const int64_t* off) {
    const UnitIn& U = units[u];
    const int m = U.n_junc;
    const ProfilePath Q = profile_path(units, results, u, which);
    int32_t* folds = reinterpret_cast<int32_t*>(block + off[u]);
    int32_t* max_arm = reinterpret_cast<int32_t*>(block + off[u] + fold_arr_bytes(m));
    UnitFoldProfile* out = reinterpret_cast<UnitFoldProfile*>(block) + u;
    if (Q.P == 0) {
        for (int j = g.tid(); j < m; j += g.size()) { folds[j] = 0; max_arm[j] = 0; }
        if (g.tid() == 0) { UnitFoldProfile z{}; z.status = Q.status; z.max_arm_at = -1; z.max_cover_at = -1; *out = z; }
        return;
    }
    stage_fold_scan(g, Q.cells, Q.P, junc_ends + U.junc_off, m, jwin, T, reinterpret_cast<const int32_t*>(planes + plane_off[u]),
                    reinterpret_cast<int32_t*>(planes + plane_bytes + plane_off[u]), folds, max_arm, out);
    if (g.tid() == 0) out->status = Q.status;
}

}  // namespace ambi
