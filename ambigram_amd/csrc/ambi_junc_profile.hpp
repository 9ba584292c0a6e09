// ambi_junc_profile.hpp -- junction usage profile of a unit's path: how often the path takes every input junction (SV, fold-back,
// adjacency) of the unit, and a summary of how that compares with the junctions' input copy numbers.
//
// The reference leaves the raw material in simulation_sv.txt (localhap.cpp:326-337: every input junction with its copy number as
// an `input` row, every non-adjacent step of the paths with its count as an `output` row) and applies the join test itself at
// localhap.cpp:277-278: a step u -> v belongs to a junction when it equals the junction's edge A or its complement edge B
// (Junction.cpp:27-39).  Here the join is done on the device.  Everything is an exact integer; nothing depends on the order of a
// reduction:
//   step i            (c[i], c[i+1]), i = 0 .. P-2
//   junction (s, t)   matches step (x, y) when (x, y) == (s, t) or (x, y) == (-t, -s); a fold-back (s, -s) has equal edges
//   count[j]          steps credited to junction j; when several junctions match a step the LOWEST index is credited
//   UnitJuncProfile   status, steps, matched / unmatched steps, first unmatched step, junctions, used, max count, over / under CN
//
// Edge classes.  (x, y) -> (-y, -x) is an involution, so two junctions share an edge exactly when their edge SETS {A, B} are
// equal: the junctions fall into classes named by the smaller of the two 32-bit edge keys (the canonical key), and a step belongs
// to the class of ITS canonical key.  The hash table in group memory therefore holds ONE slot per class -- canonical key, lowest
// junction index (atomic min), count -- instead of both edges of every junction with a count array beside them: half the slots, no
// second array, and a fold-back is one key like every other junction.  The count of a class lives in its slot and is handed to
// the winning junction when the junctions are walked a second time; every other junction of the class gets 0.
//
// Steps.  A path is a few hundred runs counting up by one, not P independent steps:
//   run-boundary steps (c[i+1] != c[i] + 1) are looked up one by one;
//   in-run steps (x, x + 1) are exactly the steps of the adjacency classes (i, i + 1) ~ (-(i+1), -i): a run over the segments
//   a..b on either strand crosses the adjacencies a..b-1, so ONE difference array over the segments (d[a] += 1, d[b] -= 1, fed by
//   the run-boundary cells as in ambi_profile.hpp) and a prefix sum give the crossings of every adjacency, and one probe per
//   segment credits them or books them as unmatched.  Only when a crossed adjacency has no junction (hand-built units) the cells
//   are read once more to find the first such step.
//
// Limits.  The table has `slots` slots (a power of two), the difference array `swin` segments.  A unit with more junctions than
// `jwin` is served in passes over PARTITIONS OF THE KEY SPACE (a second hash of the canonical key, modulo the number of passes;
// a pass inserts the junctions and looks at the steps of its partition only), a unit with more segments than `swin` in passes
// over segment windows inside every partition.  Partitions, not windows of junction indices: a step's class lies in exactly one
// partition with all its junctions, so "lowest index" and "matches nothing" are decided inside one pass and no per-step state
// crosses passes.  A partition that does not fit the table (more classes than slots) doubles the number of passes and starts
// the unit again; with the key hash a bijection this ends.  No unit is refused.
//
// Only group-memory atomics are used (compare-and-swap + min at insertion, add at a hit), no atomic on device memory.
// SPMD over the group policies of ambi_group.hpp: BlockGroup in ambi_junc_profile_kernel, HostGroup in Backend::profile's
// default (the host simulation) and in tests/tools/junc_profile_stage_check.cpp.
#pragma once
#include <vector>

#include "ambi_batch.hpp"
#include "ambi_group.hpp"
#include "ambi_profile.hpp"

namespace ambi {

// per-unit summary; the layout of ambi_unit_junc_profile_t (include/ambigram_hip.h)
struct UnitJuncProfile {
    int32_t status;           // the unit's status, copied
    int32_t steps;            // P - 1 of the profiled path
    int32_t steps_matched;    // steps credited to a junction (= sum of count[])
    int32_t steps_unmatched;  // steps that match no junction of the unit
    int32_t first_unmatched;  // smallest i whose step matches nothing, -1 if none
    int32_t juncs;            // m
    int32_t juncs_used;       // junctions with count > 0
    int32_t max_count;        // max over j of count[j]
    int32_t n_over;           // junctions with count - cn >= 0.5
    int32_t n_under;          // junctions with cn - count >= 0.5
};
static_assert(sizeof(UnitJuncProfile) == 40, "UnitJuncProfile is ambi_unit_junc_profile_t");

// Junctions per pass and segments per window: the largest unit of the batch, capped so that table (12 bytes per slot, two slots
// per junction) and difference array take 48 + 8 KB of group memory (two workgroups fit a CU's 160 KB, and the kernel stays below
// the 64 KB a launch gets without raising the function's ceiling); AMBI_JPROFILE_JUNC_WINDOW and AMBI_JPROFILE_SEG_WINDOW (tests)
// can only shrink them.
constexpr int kJuncWindowCap = 2048, kJuncSegWindowCap = 2048, kJuncMinSlots = 8;
AMBI_HD int junc_window(int max_m, int asked) { return capped_window(max_m, kJuncWindowCap, asked); }
AMBI_HD int junc_seg_window(int max_n, int asked) { return capped_window(max_n, kJuncSegWindowCap, asked); }
AMBI_HD int junc_slots(int jwin) {   // load factor <= 1/2
    int t = kJuncMinSlots;
    while (t < 2 * jwin) t <<= 1;
    return t;
}
AMBI_HD int64_t junc_profile_lds_bytes(int slots, int swin) { return int64_t(12) * slots + int64_t(4) * swin; }

// Junction profile block: [UnitJuncProfile[U]] [per unit: count i32 (m)], every per-unit array on a 16-byte boundary and padded to
// 16 bytes.  off[u] = byte offset of unit u's counts.
inline int64_t junc_profile_block_layout(const std::vector<UnitIn>& units, std::vector<int64_t>& off) {
    int64_t o = pad16(int64_t(sizeof(UnitJuncProfile)) * (int64_t)units.size());
    off.resize(units.size());
    for (size_t u = 0; u < units.size(); u++) { off[u] = o; o += pad16(int64_t(4) * units[u].n_junc); }
    return o;
}

// the table and the difference array in group memory (junc_profile_lds_bytes)
struct JuncTable {
    uint32_t* key;   // [slots] canonical key, 0 = empty (a cell is never 0)
    int32_t* val;    // [slots] lowest junction index of the class
    int32_t* cnt;    // [slots] steps of the class
    int32_t* diff;   // [swin]  difference array / crossings / flags of the adjacencies of a segment window
    int slots, swin;
};
AMBI_HD JuncTable junc_table(void* lds, int slots, int swin) {
    JuncTable T;
    T.key = reinterpret_cast<uint32_t*>(lds);
    T.val = reinterpret_cast<int32_t*>(lds) + slots;
    T.cnt = reinterpret_cast<int32_t*>(lds) + 2 * slots;
    T.diff = reinterpret_cast<int32_t*>(lds) + 3 * slots;
    T.slots = slots; T.swin = swin;
    return T;
}

AMBI_HD uint32_t junc_key(int x, int y) { return ((uint32_t)(uint16_t)(int16_t)x << 16) | (uint32_t)(uint16_t)(int16_t)y; }
AMBI_HD uint32_t junc_canon(int x, int y) {
    const uint32_t a = junc_key(x, y), b = junc_key(-y, -x);
    return a < b ? a : b;
}
// a bijection of the 32-bit keys (the finalizer of MurmurHash3): distinct keys keep distinct hashes
AMBI_HD uint32_t junc_mix(uint32_t h) {
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}
AMBI_HD bool junc_in_part(uint32_t canon, int nparts, int part) {
    return nparts == 1 || (int)(junc_mix(canon ^ 0x9e3779b9u) % (uint32_t)nparts) == part;
}
// An open-addressing table in group memory: key[slots] (a power of two), 0 = empty, linear probing from junc_mix(k), at most
// `slots` probes (a full table ends the walk as an empty slot does).  lds_find: the slot of key k or -1.  lds_claim: the slot
// that holds k from now on (compare-and-swap of 0 to k), or -1 when the table is full of other keys.
AMBI_HD int lds_find(const uint32_t* key, int slots, uint32_t k) {
    const int mask = slots - 1;
    int s = (int)(junc_mix(k) & (uint32_t)mask);
    for (int i = 0; i < slots; i++, s = (s + 1) & mask) {
        const uint32_t have = key[s];
        if (have == k) return s;
        if (have == 0) return -1;
    }
    return -1;
}
AMBI_HD int lds_claim(uint32_t* key, int slots, uint32_t k) {
    const int mask = slots - 1;
    int s = (int)(junc_mix(k) & (uint32_t)mask);
    for (int i = 0; i < slots; i++, s = (s + 1) & mask) {
        const uint32_t have = (uint32_t)atomic_cas_i32(reinterpret_cast<int*>(key + s), 0, (int)k);
        if (have == 0 || have == k) return s;
    }
    return -1;
}
// junction j into its class: the lowest index stays; false: the table is full of other keys
AMBI_HD bool junc_insert(const JuncTable& T, uint32_t canon, int j) {
    const int s = lds_claim(T.key, T.slots, canon);
    if (s >= 0) atomic_min_i32(T.val + s, j);
    return s >= 0;
}

// one event of a run boundary into the window [w0, w0 + wn) of the difference array: a run over the segments a..b crosses the
// adjacencies a..b-1 on either strand (d[a] += 1, d[b] -= 1; a '+' run begins at a, a '-' run at b)
AMBI_HD void junc_post(int32_t* d, int w0, int wn, int c, bool begin) {
    if (c == 0) return;
    const int j = (c > 0 ? c : -c) - w0;
    if (j < 0 || j >= wn) return;
    atomic_add_i32(d + j, (c > 0) == begin ? 1 : -1);
}

// cells: the unit's path (local signed ids), P > 0 cells, readable up to the next multiple of four cells; ends / cn: the unit's m
// junctions; T: group memory; jwin: junctions a pass is sized for (the number of passes starts at ceil(m / jwin));
// out_count: m counts; out: every field but `status`.  Whole group.
template <class G>
AMBI_HD void stage_junc_profile(const G& g, const rcell_t* cells, int P, int n, const JuncEnds* ends, const double* cn, int m, int jwin,
                                const JuncTable& T, int32_t* out_count, UnitJuncProfile* out) {
    const int tid = g.tid(), sz = g.size();
    const bool vec = (reinterpret_cast<uintptr_t>(cells) & 7) == 0;
    const int kNone = 0x7fffffff;
    int nparts = jwin > 0 ? (m + jwin - 1) / jwin : 1;
    if (nparts < 1) nparts = 1;
    int matched, unmatched, first, used, max_count, n_over, n_under;
    for (;;) {
        matched = 0; unmatched = 0; first = kNone; used = 0; max_count = 0; n_over = 0; n_under = 0;
        bool full = false;
        for (int part = 0; part < nparts && !full; part++) {
            // the classes of this partition
            for (int s = tid; s < T.slots; s += sz) { T.key[s] = 0; T.val[s] = kNone; T.cnt[s] = 0; }
            g.sync();
            bool mine_full = false;
            for (int j = tid; j < m; j += sz) {
                const JuncEnds E = ends[j];
                const uint32_t canon = junc_canon(E.s, E.t);
                if (junc_in_part(canon, nparts, part) && !junc_insert(T, canon, j)) mine_full = true;
            }
            if (g.any(mine_full)) { full = true; break; }   // (any: a barrier; the table is complete behind it)
            // the steps of this partition: boundary steps in the first cell pass, adjacency crossings window by window
            int carry = 0;
            for (int w0 = 1; w0 <= n; w0 += T.swin) {
                const int wn = n - w0 + 1 < T.swin ? n - w0 + 1 : T.swin;
                const bool boundary = w0 == 1;   // the boundary steps are looked up once per partition
                for (int j = tid; j < wn; j += sz) T.diff[j] = 0;
                g.sync();
                for (int base = 0; base < P; base += sz * kProfileChunk) {
                    const int s = base + tid * kProfileChunk;
                    if (s >= P) continue;
                    rcell_t c[kProfileChunk];
                    int prev;
                    const int e = path_load_chunk(cells, P, vec, s, c, prev);
                    for (int k = 0; k < e; k++) {
                        const int cur = c[k];
                        if (s + k == 0) junc_post(T.diff, w0, wn, cur, true);
                        else if (cur != prev + 1) {
                            junc_post(T.diff, w0, wn, prev, false);
                            junc_post(T.diff, w0, wn, cur, true);
                            const uint32_t canon = junc_canon(prev, cur);
                            if (boundary && junc_in_part(canon, nparts, part)) {
                                const int slot = lds_find(T.key, T.slots, canon);
                                if (slot >= 0) { atomic_add_i32(T.cnt + slot, 1); matched++; }
                                else { unmatched++; if (s + k - 1 < first) first = s + k - 1; }
                            }
                        }
                        prev = cur;
                    }
                    if (s + e == P) junc_post(T.diff, w0, wn, prev, false);   // the last cell of the path ends its run
                }
                g.sync();
                // crossings of the adjacencies seg | seg + 1 of the window: inclusive prefix sums on top of the windows before
                bool lost = false;
                for (int base = 0; base < wn; base += sz) {
                    const int j = base + tid;
                    const int v = j < wn ? T.diff[j] : 0;
                    int tot;
                    const int ex = g.exscan_i32(v, &tot);
                    if (j < wn) {
                        const int seg = w0 + j, x = carry + ex + v;
                        int flag = 0;
                        if (x > 0 && seg < n) {
                            const uint32_t canon = junc_canon(seg, seg + 1);
                            if (junc_in_part(canon, nparts, part)) {
                                const int slot = lds_find(T.key, T.slots, canon);
                                if (slot >= 0) { atomic_add_i32(T.cnt + slot, x); matched += x; }
                                else { unmatched += x; flag = 1; lost = true; }
                            }
                        }
                        T.diff[j] = flag;   // (read by nobody else before the barrier below)
                    }
                    carry += tot;
                }
                // a crossed adjacency without a junction: the cells once more, for the first in-run step over a flagged adjacency
                if (g.any(lost)) {
                    for (int base = 0; base < P; base += sz * kProfileChunk) {
                        const int s = base + tid * kProfileChunk;
                        if (s >= P) continue;
                        rcell_t c[kProfileChunk];
                        int prev;
                        const int e = path_load_chunk(cells, P, vec, s, c, prev);
                        for (int k = 0; k < e; k++) {
                            const int cur = c[k];
                            if (s + k > 0 && cur == prev + 1) {
                                const int j = (prev > 0 ? prev : -prev - 1) - w0;   // (x, x + 1) crosses x | x + 1, (-(x+1), -x) too
                                if (j >= 0 && j < wn && T.diff[j] && s + k - 1 < first) first = s + k - 1;
                            }
                            prev = cur;
                        }
                    }
                }
                g.sync();   // the array is cleared for the next window
            }
            // the counts of this partition's junctions: the winner of a class takes the slot's count
            for (int j = tid; j < m; j += sz) {
                const JuncEnds E = ends[j];
                const uint32_t canon = junc_canon(E.s, E.t);
                if (!junc_in_part(canon, nparts, part)) continue;
                const int slot = lds_find(T.key, T.slots, canon);
                const int c = (slot >= 0 && T.val[slot] == j) ? T.cnt[slot] : 0;
                out_count[j] = c;
                used += c > 0;
                if (c > max_count) max_count = c;
                const double d = (double)c - cn[j];
                n_over += d >= 0.5; n_under += -d >= 0.5;
            }
            g.sync();   // the table is cleared for the next partition
        }
        if (!full) break;
        nparts *= 2;   // (ends: from 2^29 passes on a partition has at most kJuncMinSlots of the 2^32 hash values, and m < 2^16)
    }
    matched = g.sum_i32(matched); unmatched = g.sum_i32(unmatched); first = g.min_i32(first);
    used = g.sum_i32(used); max_count = g.max_i32(max_count); n_over = g.sum_i32(n_over); n_under = g.sum_i32(n_under);
    if (tid == 0) {
        out->steps = P - 1; out->steps_matched = matched; out->steps_unmatched = unmatched; out->first_unmatched = first == kNone ? -1 : first;
        out->juncs = m; out->juncs_used = used; out->max_count = max_count; out->n_over = n_over; out->n_under = n_under;
    }
}

// One unit of a batch: profiles the path ambi_batch_unit_path(unit, which) returns (profile_path) against the unit's junctions into
// the junction profile block.  SHORTCUT and INFEASIBLE units like any other; a unit with a negative status or without a path
// gets zero counts and a summary that is zero but for the status.  Whole group.
template <class G>
AMBI_HD void junc_profile_unit(const G& g, const UnitIn* units, const JuncEnds* junc_ends, const double* junc_cn, const uint8_t* results, int u,
                               int which, int jwin, const JuncTable& T, uint8_t* block, const int64_t* off) {
    const UnitIn& U = units[u];
    const int m = U.n_junc;
    const ProfilePath Q = profile_path(units, results, u, which);
    int32_t* count = reinterpret_cast<int32_t*>(block + off[u]);
    UnitJuncProfile* out = reinterpret_cast<UnitJuncProfile*>(block) + u;
    if (Q.P == 0) {
        for (int j = g.tid(); j < m; j += g.size()) count[j] = 0;
        if (g.tid() == 0) { UnitJuncProfile z{}; z.status = Q.status; *out = z; }
        return;
    }
    stage_junc_profile(g, Q.cells, Q.P, U.n_seg, junc_ends + U.junc_off, junc_cn + U.junc_off, m, jwin, T, count, out);
    if (g.tid() == 0) out->status = Q.status;
}

}  // namespace ambi
