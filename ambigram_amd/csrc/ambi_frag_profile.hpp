// ambi_frag_profile.hpp -- fragment support profile of a unit's path: how often the path contains every fragment of the unit's
// .juncs evidence (a signed chain of segments read off one barcode group, long read or optical-map contig), in either direction,
// and where it does so first.
//
// The reference cuts every .juncs line at its strand changes, sorts the pieces into unordered id sets and adds the breakpoints as
// junctions (readComponents, LocalGenomicMap.cpp:5096-5156): the chain's ORDER never reaches the ILP, and nothing checks that a
// printed path contains the chains that were given as evidence for it.  Here that check is done on the device.  Everything is an
// exact integer; nothing depends on the order of a reduction:
//   fragment f        f_0 .. f_{L-1}, local signed ids, L >= 2;   rc(f) = -f_{L-1} .. -f_0
//   occurrence at i   c[i + k] == f_k for all k, 0 <= i <= P - L; occurrences may overlap
//   fwd[f]            occurrences of f;   rev[f]: occurrences of rc(f), 0 when rc(f) == f (a palindrome is counted once)
//   first[f]          smallest i over both directions, -1 if none
//   UnitFragProfile   status, cells, fragments, supported, first unsupported, max count, longest supported, occurrences
//
// Patterns.  Fragment f contributes the patterns 2f (f itself) and 2f + 1 (rc(f); idle when f is a palindrome, when L < 2 or when
// L > P).  A pass serves a WINDOW of pattern indices -- not a partition of the key space, because thousands of fragments may
// share their first step and a pattern's count needs no state across passes: pattern p is counted in exactly one window.
// The pass inserts every pattern's first step (p_0, p_1) into a hash table in group memory (the exact 32-bit junc_key, not the
// canonical one: direction matters; load factor <= 1/2); a slot heads a chain through the per-pattern `next` array.  Then the
// cells are swept as stage_junc_profile sweeps them: the step (c[i], c[i + 1]) of every i <= P - 2 is probed, on a hit the chain
// is walked and the remaining L - 2 cells are compared with the fragment image, cell by cell -- a hash alone never counts -- and
// i + L > P is rejected before anything is read (cells behind P are stale data of earlier runs).  A match is a group-memory add
// on the pattern's count and a group-memory min on its first position.  After the sweep the window's counts go to the block.
// A fragment is always written by the same thread (f modulo the group size), whichever window holds its patterns, so the thread
// that completes a fragment with pattern 2f + 1 reads back what itself wrote for 2f.
//
// The window set-up and the sweep are frag_window_build / frag_window_sweep, which the evidence depth profile
// (ambi_evidence_profile.hpp) runs as well with another action on a match.
// Only group-memory atomics are used, no atomic on device memory.  SPMD over the group policies of ambi_group.hpp: BlockGroup in
// ambi_frag_profile_kernel, HostGroup in Backend::profile's default (the host simulation) and in
// tests/tools/frag_profile_stage_check.cpp.
#pragma once
#include <vector>

#include "ambi_batch.hpp"
#include "ambi_group.hpp"
#include "ambi_junc_profile.hpp"
#include "ambi_profile.hpp"

namespace ambi {

// per-unit summary; the layout of ambi_unit_frag_profile_t (include/ambigram_hip.h)
struct UnitFragProfile {
    int32_t status;             // the unit's status, copied
    int32_t cells;              // P of the profiled path
    int32_t frags;              // F
    int32_t frags_supported;    // fragments with fwd + rev > 0
    int32_t first_unsupported;  // lowest fragment index without an occurrence, -1 if none
    int32_t max_count;          // max over f of fwd + rev
    int32_t longest_supported;  // cells of the longest supported fragment, 0 if none
    int32_t reserved;
    int64_t occurrences;        // sum over f of fwd + rev
};
static_assert(sizeof(UnitFragProfile) == 40, "UnitFragProfile is ambi_unit_frag_profile_t");

// the fragment image of a batch where the stage reads it (FragImage of ambi_pack.hpp, on the host or on the device)
struct FragArgs {
    const rcell_t* cells;       // the units' fragment cells back to back, local signed ids
    const int32_t* frag_off;    // all units' prefixes one after the other: F + 1 offsets each, relative to the unit's first cell
    const int64_t* cell_off;    // [U] index of a unit's first cell
    const int64_t* pref_off;    // [U] index of a unit's frag_off[0]
    const int32_t* n_frag;      // [U] F
};

// Patterns per window: twice the most fragments of a unit, capped so that table (8 bytes per slot, two slots per pattern) and the
// three per-pattern arrays (12 bytes) take 32 + 24 KB of group memory: the kernel stays below the 64 KB a launch gets without
// raising the function's ceiling.  AMBI_FPROFILE_FRAG_WINDOW (tests) can only shrink it.
constexpr int kFragWindowCap = 2048, kFragMinSlots = 8;
constexpr int kFragCompare = 8;   // cells of a candidate compared per round
AMBI_HD int frag_window(int max_f, int asked) { return capped_window(max_f > kFragWindowCap / 2 ? kFragWindowCap : 2 * max_f, kFragWindowCap, asked); }
AMBI_HD int frag_slots(int pwin) {   // load factor <= 1/2
    int t = kFragMinSlots;
    while (t < 2 * pwin) t <<= 1;
    return t;
}
AMBI_HD int64_t frag_profile_lds_bytes(int slots, int pwin) { return int64_t(8) * slots + int64_t(12) * pwin; }

// Fragment profile block: [UnitFragProfile[U]] [per unit: fwd i32 (F), rev i32 (F), first i32 (F)], every array on a 16-byte boundary
// and padded to 16 bytes.  off[u] = byte offset of unit u's fwd; rev and first follow at frag_profile_arr_bytes(F) each.
AMBI_HD int64_t frag_profile_arr_bytes(int F) { return pad16(int64_t(4) * F); }
inline int64_t frag_profile_block_layout(const int32_t* n_frag, size_t U, std::vector<int64_t>& off) {
    int64_t o = pad16(int64_t(sizeof(UnitFragProfile)) * (int64_t)U);
    off.resize(U);
    for (size_t u = 0; u < U; u++) { off[u] = o; o += 3 * frag_profile_arr_bytes(n_frag[u]); }
    return o;
}

// the table and the per-pattern arrays in group memory (frag_profile_lds_bytes)
struct FragTable {
    uint32_t* key;   // [slots] junc_key of a first step, 0 = empty (a cell is never 0)
    int32_t* head;   // [slots] first pattern of the slot's chain (index in the window), -1 = none
    int32_t* next;   // [pwin]  the next pattern with the same first step, -1 = none
    int32_t* cnt;    // [pwin]  occurrences of the pattern
    int32_t* first;  // [pwin]  smallest position of an occurrence
    int slots, pwin;
};
AMBI_HD FragTable frag_table(void* lds, int slots, int pwin) {
    FragTable T;
    T.key = reinterpret_cast<uint32_t*>(lds);
    T.head = reinterpret_cast<int32_t*>(lds) + slots;
    T.next = reinterpret_cast<int32_t*>(lds) + 2 * slots;
    T.cnt = T.next + pwin;
    T.first = T.cnt + pwin;
    T.slots = slots; T.pwin = pwin;
    return T;
}
// pattern j of the window in front of the chain of its first step (lds_claim, ambi_junc_profile.hpp); false: the table is full of
// other keys (never: <= pwin keys)
AMBI_HD bool frag_insert(const FragTable& T, uint32_t key, int j) {
    const int s = lds_claim(T.key, T.slots, key);
    if (s < 0) return false;
    int old = T.head[s];
    for (;;) {   // (nobody walks a chain before the barrier behind the insertions)
        T.next[j] = old;
        const int got = atomic_cas_i32(T.head + s, old, j);
        if (got == old) return true;
        old = got;
    }
}

// cell k of pattern (f, dir): fc = the unit's fragment cells, [a, b) = the fragment's cells
AMBI_HD int frag_cell(const rcell_t* fc, int a, int b, int dir, int k) { return dir ? -(int)fc[b - 1 - k] : (int)fc[a + k]; }
AMBI_HD bool frag_palindrome(const rcell_t* fc, int a, int b) {
    for (int k = 0; 2 * k < b - a; k++) if ((int)fc[a + k] != -(int)fc[b - 1 - k]) return false;
    return true;
}

// The windowed match, shared by the fragment profile below and the evidence depth profile (ambi_evidence_profile.hpp): the two
// differ only in what a verified occurrence does.
// frag_window_build: the patterns [w0, w0 + wn) of the unit into the cleared table; true when the window holds a live pattern (a
// barrier: the table is complete behind it) -- a window without one needs no sweep.  Whole group.
template <class G>
AMBI_HD bool frag_window_build(const G& g, int P, const rcell_t* fc, const int32_t* foff, int w0, int wn, const FragTable& T) {
    const int tid = g.tid(), sz = g.size();
    for (int s = tid; s < T.slots; s += sz) { T.key[s] = 0; T.head[s] = -1; }
    for (int j = tid; j < wn; j += sz) { T.next[j] = -1; T.cnt[j] = 0; T.first[j] = 0x7fffffff; }
    g.sync();
    bool mine_any = false;
    for (int j = tid; j < wn; j += sz) {
        const int p = w0 + j, f = p >> 1, dir = p & 1;
        const int a = foff[f], b = foff[f + 1], L = b - a;
        if (L < 2 || L > P) continue;                       // (no occurrence is possible)
        if (dir && frag_palindrome(fc, a, b)) continue;     // rc(f) == f: counted once, as f
        if (frag_insert(T, junc_key(frag_cell(fc, a, b, dir, 0), frag_cell(fc, a, b, dir, 1)), j)) mine_any = true;
    }
    return g.any(mine_any);
}
// frag_window_sweep: every step of the path against the window's table; match(j, i, L) for every verified occurrence at cell i of the
// window's pattern j (L cells).  Whole group; no barrier inside.
template <class G, class M>
AMBI_HD void frag_window_sweep(const G& g, const rcell_t* cells, int P, bool vec, const rcell_t* fc, const int32_t* foff, int w0, const FragTable& T,
                               const M& match) {
    const int tid = g.tid(), sz = g.size();
    for (int base = 0; base < P; base += sz * kProfileChunk) {
        const int s = base + tid * kProfileChunk;
        if (s >= P) continue;
        rcell_t c[kProfileChunk];
        int prev;
        const int e = path_load_chunk(cells, P, vec, s, c, prev);
        for (int k = 0; k < e; k++) {
            const int cur = c[k];
            if (s + k > 0) {
                const int i = s + k - 1;            // the step (c[i], c[i + 1])
                const int slot = lds_find(T.key, T.slots, junc_key(prev, cur));
                for (int j = slot >= 0 ? T.head[slot] : -1; j >= 0; j = T.next[j]) {
                    const int p = w0 + j, dir = p & 1;
                    const int a = foff[p >> 1], b = foff[(p >> 1) + 1], L = b - a;
                    if (i + L > P) continue;        // before anything is read: cells behind P are stale
                    // eight cells per round, their loads independent of one another: a chain of L dependent 2-byte loads
                    // was 15 times the junction profile's time on the bench batch (profiles/r20_notes.md)
                    bool same = true;
                    for (int q = 2; q < L && same; q += kFragCompare) {
                        int diff = 0;
#pragma unroll
                        for (int t = 0; t < kFragCompare; t++)
                            if (q + t < L) diff |= (int)cells[i + q + t] ^ frag_cell(fc, a, b, dir, q + t);
                        same = diff == 0;
                    }
                    if (same) match(j, i, L);
                }
            }
            prev = cur;
        }
    }
}

// cells: the unit's path (local signed ids), P > 0 cells, readable up to the next multiple of four cells; fc / foff: the unit's F
// fragments (foff: F + 1 offsets into fc); T: group memory; out_fwd / out_rev / out_first: F values each; out: every field but
// `status`.  Whole group.
template <class G>
AMBI_HD void stage_frag_profile(const G& g, const rcell_t* cells, int P, const rcell_t* fc, const int32_t* foff, int F, const FragTable& T,
                                int32_t* out_fwd, int32_t* out_rev, int32_t* out_first, UnitFragProfile* out) {
    const int tid = g.tid(), sz = g.size();
    const bool vec = (reinterpret_cast<uintptr_t>(cells) & 7) == 0;
    const int kNone = 0x7fffffff;
    int supported = 0, first_unsup = kNone, max_count = 0, longest = 0;
    int64_t occ = 0;
    const int NP = 2 * F;
    for (int w0 = 0; w0 < NP; w0 += T.pwin) {
        const int wn = NP - w0 < T.pwin ? NP - w0 : T.pwin;
        // a match is a group-memory add on the pattern's count and a group-memory min on its first position
        if (frag_window_build(g, P, fc, foff, w0, wn, T))
            frag_window_sweep(g, cells, P, vec, fc, foff, w0, T, [cnt = T.cnt, first = T.first](int j, int i, int) { atomic_add_i32(cnt + j, 1); atomic_min_i32(first + j, i); });
        g.sync();
        // the window's counts to the block: fragment f by thread f mod size, in every window
        const int flo = w0 >> 1, fhi = (w0 + wn - 1) >> 1;
        for (int f = flo + ((tid - flo % sz + sz) % sz); f <= fhi; f += sz) {
            for (int dir = 0; dir < 2; dir++) {
                const int j = 2 * f + dir - w0;
                if (j < 0 || j >= wn) continue;
                const int c = T.cnt[j], at = T.first[j];
                if (dir == 0) { out_fwd[f] = c; out_first[f] = at; continue; }
                out_rev[f] = c;
                const int before = out_first[f], fst = before < at ? before : at;
                out_first[f] = fst == kNone ? -1 : fst;
                const int tot = out_fwd[f] + c;             // (< 2^31: at most P positions in each direction, P <= 2^22)
                if (tot > 0) { supported++; const int L = foff[f + 1] - foff[f]; if (L > longest) longest = L; }
                else if (f < first_unsup) first_unsup = f;
                if (tot > max_count) max_count = tot;
                occ += tot;
            }
        }
        g.sync();   // the table is cleared for the next window
    }
    supported = g.sum_i32(supported); first_unsup = g.min_i32(first_unsup); max_count = g.max_i32(max_count); longest = g.max_i32(longest);
    int64_t occ_all;
    (void)g.exscan_i64(occ, &occ_all);
    if (tid == 0) {
        out->cells = P; out->frags = F; out->frags_supported = supported; out->first_unsupported = first_unsup == kNone ? -1 : first_unsup;
        out->max_count = max_count; out->longest_supported = longest; out->reserved = 0; out->occurrences = occ_all;
    }
}

// One unit of a batch: profiles the path ambi_batch_unit_path(unit, which) returns (profile_path) against the unit's fragments into
// the fragment profile block.  SHORTCUT and INFEASIBLE units like any other; a unit with a negative status or without a path
// gets zero counts, first = -1 and a summary that is zero but for the status and the number of fragments.  Whole group.
template <class G>
AMBI_HD void frag_profile_unit(const G& g, const UnitIn* units, const FragArgs& I, const uint8_t* results, int u, int which, const FragTable& T,
                               uint8_t* block, const int64_t* off) {
    const int F = I.n_frag[u];
    const ProfilePath Q = profile_path(units, results, u, which);
    const int64_t arr = frag_profile_arr_bytes(F);
    int32_t* fwd = reinterpret_cast<int32_t*>(block + off[u]);
    int32_t* rev = reinterpret_cast<int32_t*>(block + off[u] + arr);
    int32_t* first = reinterpret_cast<int32_t*>(block + off[u] + 2 * arr);
    UnitFragProfile* out = reinterpret_cast<UnitFragProfile*>(block) + u;
    if (Q.P == 0) {
        for (int f = g.tid(); f < F; f += g.size()) { fwd[f] = 0; rev[f] = 0; first[f] = -1; }
        if (g.tid() == 0) { UnitFragProfile z{}; z.status = Q.status; z.frags = F; *out = z; }
        return;
    }
    stage_frag_profile(g, Q.cells, Q.P, I.cells + I.cell_off[u], I.frag_off + I.pref_off[u], F, T, fwd, rev, first, out);
    if (g.tid() == 0) out->status = Q.status;
}

}  // namespace ambi
