// ambi_exchange.hpp -- the final paths of a batch packed for the end-of-batch exchange, and unpacked on the receiving rank.
//
// Two forms (include/ambigram_hip.h: ambi_batch_pack_paths, ambi_batch_pack_runs, ambi_expand_runs):
//   cells   lengths[u], the cells of all units back to back as absolute signed ids
//             pack_scan (lengths -> offsets, total)  ->  pack_copy_unit
//   runs    a run is a stretch of cells counting up by one and starts where a cell is not its predecessor + 1; per unit
//           lengths[u], run_counts[u], and {start value, length} of all runs back to back
//             pack_runs_count_unit  ->  pack_runs_scan (offsets, {runs, cells})  ->  pack_runs_write_unit
//           expand_run turns one run back into cells at a given offset.
// Buffers that are too small: counts, offsets and totals are always complete; pack_copy_unit clamps cell by cell,
// pack_runs_write_unit writes a unit whole or not at all; nothing is written at or past the capacity.
//
// SPMD over the group policies of ambi_group.hpp like the stages of ambi_stages.hpp: BlockGroup (WaveGroup for expand_run) in
// the kernels of ambi_engine.hip, HostGroup in the host simulation, which calls them in the kernels' order.
#pragma once
#include "ambi_batch.hpp"
#include "ambi_group.hpp"

namespace ambi {

// The path the exchange carries is unit_path (ambi_batch.hpp), its length as stored.
// lengths[u] and pack_off[0 .. n_units] (prefix sum of the lengths), *total = all cells.  One group for the whole batch.
template <class G>
AMBI_HD void pack_scan(const G& g, const BatchArgs& A, int which, int32_t* lengths, int64_t* pack_off, int64_t* total) {
    int64_t carry = 0;
    for (int base = 0; base < A.n_units; base += g.size()) {
        const int u = base + g.tid();
        int64_t len = 0;
        if (u < A.n_units) {
            const UnitOut* h = unit_out(A.results, u);
            len = which ? h->path_indel_len : h->path_len;
            lengths[u] = (int32_t)len;
        }
        int64_t tot;
        int64_t ex = g.exscan_i64(len, &tot);
        if (u < A.n_units) pack_off[u] = carry + ex;
        carry += tot;
    }
    if (g.tid() == 0) { pack_off[A.n_units] = carry; if (total) *total = carry; }
}
// the cells of unit u to cells[pack_off[u] ..), those below `cap` only.  One group per unit.
template <class G>
AMBI_HD void pack_copy_unit(const G& g, const BatchArgs& A, int u, int which, const int64_t* pack_off, int32_t* cells, int64_t cap) {
    const rcell_t* src = unit_path(A.units, A.results, u, which).cells;
    const int seg_base = A.units[u].seg_base;
    const int64_t off = pack_off[u], len = pack_off[u + 1] - off;
    for (int64_t i = g.tid(); i < len; i += g.size())
        if (off + i < cap) cells[off + i] = abs_cell(src[i], seg_base);
}

// ---- run-length form: two passes over the path in the result blob, one group per unit each ----
template <class G>
AMBI_HD void pack_runs_count_unit(const G& g, const BatchArgs& A, int u, int which, int32_t* lengths, int32_t* run_counts) {
    const UnitPath Q = unit_path(A.units, A.results, u, which);
    const rcell_t* src = Q.cells;
    const int P = Q.len;
    int mine = 0;
    for (int i = g.tid(); i < P; i += g.size()) mine += (i == 0 || src[i] != src[i - 1] + 1) ? 1 : 0;
    const int total = g.sum_i32(mine);
    if (g.tid() == 0) { run_counts[u] = total; lengths[u] = P; }
}
// run_off[0 .. n_units] (prefix sum of the run counts), totals = {runs, cells}.  One group for the whole batch.
template <class G>
AMBI_HD void pack_runs_scan(const G& g, const BatchArgs& A, const int32_t* lengths, const int32_t* run_counts, int64_t* run_off, int64_t* totals) {
    int64_t carry = 0, cells = 0;
    for (int base = 0; base < A.n_units; base += g.size()) {
        const int u = base + g.tid();
        const int64_t c = u < A.n_units ? run_counts[u] : 0, l = u < A.n_units ? lengths[u] : 0;
        int64_t tot, totl;
        const int64_t ex = g.exscan_i64(c, &tot);
        (void)g.exscan_i64(l, &totl);
        if (u < A.n_units) run_off[u] = carry + ex;
        carry += tot; cells += totl;
    }
    if (g.tid() == 0) { run_off[A.n_units] = carry; if (totals) { totals[0] = carry; totals[1] = cells; } }
}
template <class G>
AMBI_HD void pack_runs_write_unit(const G& g, const BatchArgs& A, int u, int which, const int64_t* run_off, int32_t* run_start, int32_t* run_len,
                                  int64_t cap) {
    const UnitPath Q = unit_path(A.units, A.results, u, which);
    const rcell_t* src = Q.cells;
    const int P = Q.len;
    const int64_t off = run_off[u];
    const int n = (int)(run_off[u + 1] - off);
    if (off + n > cap) return;   // the caller's buffers are too small: nothing is written for this unit (totals tell)
    int done = 0;
    for (int base = 0; base < P; base += g.size()) {      // run starts in path order: value and, for now, position
        const int i = base + g.tid();
        const int flag = (i < P && (i == 0 || src[i] != src[i - 1] + 1)) ? 1 : 0;
        int tot;
        const int ex = g.exscan_i32(flag, &tot);
        if (flag) { run_start[off + done + ex] = abs_cell(src[i], A.units[u].seg_base); run_len[off + done + ex] = i; }
        done += tot;
    }
    g.sync();
    // positions -> lengths (the next run's position is read before anyone overwrites it: two phases)
    for (int base = 0; base < n; base += g.size()) {
        const int k = base + g.tid();
        int len = 0;
        if (k < n) len = (k + 1 < n ? run_len[off + k + 1] : P) - run_len[off + k];
        g.sync();
        if (k < n) run_len[off + k] = len;
        g.sync();
    }
}

// run r -> cells[cell_off[r] ..), those below `cap` only.  One wavefront (or the host's one thread) per run; cell_off is trusted:
// by contract the prefix sum of the non-negative lengths.
template <class G>
AMBI_HD void expand_run(const G& g, const int32_t* run_start, const int32_t* run_len, const int64_t* cell_off, int64_t r, int32_t* cells, int64_t cap) {
    const int32_t s = run_start[r], len = run_len[r];
    const int64_t o = cell_off[r];
    for (int k = g.tid(); k < len; k += g.size()) if (o + k < cap) cells[o + k] = s + k;
}

}  // namespace ambi
