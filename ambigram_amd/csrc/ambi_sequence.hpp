// ambi_sequence.hpp -- the nucleotide sequence of a unit's path: the bases of the segments the path crosses, joined in path order,
// a segment crossed on the '-' strand as its reverse complement.
//
// What the reference leaves to scripts around bedtools (script/main.py:537-588 bfb2fasta, :709-740 seg2fasta,
// script/bfb_scripts.py:31-49 getFasta: a BED line per path cell through `bedtools getfasta -s`, the records joined).
// Conventions (the contract of ambi_batch_sequence, include/ambigram_hip.h):
//   bases of segment i   chrom[start .. end) of the FASTA record named like the segment's chromosome: 0-based, half-open,
//                        end - start bytes (seg2fasta writes `chr start end` of the .lh unchanged into a BED line)
//   complement           ACGTUMRWSYKVHDBN -> TGCAAKYWSRMBDHVN and the same in lower case; every other byte value maps to itself
//
// The segments of a unit lie back to back in local id order in the batch's sequence image (SeqImage, ambi_pack.hpp), with an
// int64 prefix seg_pos[0..n] per unit.  A run of the path (`a, a+1, .., b` or `-b, .., -a`) is therefore ONE contiguous byte range
// [seg_pos[a-1], seg_pos[b]) of the unit's store, copied forward or reversed and complemented: no look-up per cell.
//
// Two stages over the units [first, first + count) of a request (SeqPlan):
//   extents  one group per unit, two passes.  Pass 0 counts the unit's runs and bytes (totals: the host sizes the extent arrays
//            and the output block from them).  Pass 1 writes per run its extent -- ext_src: the byte offset of its range in the
//            image, one's complement (~offset) for a '-' run; ext_out: the exclusive 64-bit scan of the runs' byte counts, so a
//            run's byte count is ext_out[k + 1] - ext_out[k] and ext_out[runs] the unit's length.
//   fill     a work item is a tile of kSeqTile output bytes of one unit (every unit's output starts on a 16-byte boundary of
//            the block, tiles do not span units).  Unit and first / last run of a tile: bisection for the first tile a group takes,
//            a step or two on from the tile before for the consecutive ones (SeqCursor).  A lane owns 16 output
//            bytes and issues one 16-byte store; a group inside one run takes a 16-byte load at the source's own alignment
//            (forward) or the mirrored 16 source bytes, byte-reversed in registers and complemented (reverse); a group that
//            straddles a run boundary or the unit's end goes byte by byte (runs can be one base long).  Bytes between a unit's
//            length and the next multiple of 16 are written as zero; nothing else is written.
//
// SPMD over the group policies of ambi_group.hpp: BlockGroup in ambi_seq_extents_kernel / ambi_seq_fill_kernel, HostGroup in
// Backend::sequence's default (the host simulation).
#pragma once
#include <vector>

#include "ambi_batch.hpp"
#include "ambi_group.hpp"

namespace ambi {

constexpr int kSeqLaneBytes = 16, kSeqTileLanes = 256, kSeqTile = kSeqLaneBytes * kSeqTileLanes;
constexpr int kSeqTooLarge = -34;   // AMBI_ERR_TOO_LARGE: the request's bytes exceed the caller's limit

// the sequence image where the stages read it
struct SeqArgs {
    const uint8_t* bases;       // the stores of all units
    const int64_t* seg_pos;     // per unit n + 1 entries: seg_pos[i] = bytes of the segments 1..i (relative to the unit's store)
    const int64_t* store_off;   // [U] byte offset of a unit's store in bases
    const int64_t* pos_off;     // [U] index of a unit's seg_pos[0]
};
// one request: the units [first, first + count); index r = unit - first
struct SeqPlan {
    int32_t first, count;
    int64_t* totals;            // [2 count] {bytes, runs} of every unit (written by pass 0, read by pass 1)
    const int64_t* ext_off;     // [count + 1] first extent slot of every unit (runs + 1 slots each)
    int64_t* ext_src;           // per slot: source offset in bases, ~offset for a '-' run
    int64_t* ext_out;           // per slot: exclusive scan of the byte counts; slot `runs` = the unit's length
    const int64_t* out_off;     // [count] byte offset of every unit's sequence in `out` (multiples of 16)
    const int64_t* tile_off;    // [count + 1] first tile of every unit
    uint8_t* out;
    int64_t out_bytes;          // capacity of out
};

AMBI_HD uint8_t seq_complement(uint8_t c) {
    const uint8_t up = (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c;
    uint8_t r;
    switch (up) {
        case 'A': r = 'T'; break; case 'C': r = 'G'; break; case 'G': r = 'C'; break; case 'T': r = 'A'; break;
        case 'U': r = 'A'; break; case 'M': r = 'K'; break; case 'R': r = 'Y'; break; case 'W': r = 'W'; break;
        case 'S': r = 'S'; break; case 'Y': r = 'R'; break; case 'K': r = 'M'; break; case 'V': r = 'B'; break;
        case 'H': r = 'D'; break; case 'D': r = 'H'; break; case 'B': r = 'V'; break; case 'N': r = 'N'; break;
        default: return c;
    }
    return up == c ? r : (uint8_t)(r + 32);
}
// the 256-entry table in group memory.  Whole group; sync before use.
template <class G>
AMBI_HD void seq_build_table(const G& g, uint8_t* table) {
    for (int i = g.tid(); i < 256; i += g.size()) table[i] = seq_complement((uint8_t)i);
}

// last index k in [0, n) with off[k] <= key (off ascending, off[0] <= key): prefix_find of ambi_stages.hpp, which this header
// does not pull in; of equal offsets (empty units, empty runs) the last one, the one that holds bytes
AMBI_HD int seq_prefix_find(const int64_t* off, int lo, int hi, int64_t key) {
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= key) lo = mid; else hi = mid; }
    return lo;
}

// the path ambi_batch_unit_path(unit, which) returns, or P = 0 for a unit with a negative status or without a path
AMBI_HD const rcell_t* seq_unit_path(const UnitIn* units, const uint8_t* results, int u, int which, int* len) {
    const UnitPath Q = unit_path(units, results, u, which);
    *len = (Q.status < 0 || Q.len < 0 || Q.len > Q.path_cap) ? 0 : Q.len;
    return Q.cells;
}

// byte range of the run of `len` cells that starts with cell c: [lo, hi) relative to the unit's store (ids outside 1..n, which no
// finish stage writes, give an empty range instead of a read outside the prefix)
AMBI_HD void seq_run_range(const int64_t* pos, int n, int c, int len, int64_t* lo, int64_t* hi) {
    int a = c > 0 ? c - 1 : -c - len, b = c > 0 ? c - 1 + len : -c;   // segments a+1 .. b
    if (a < 0) a = 0;
    if (b > n) b = n;
    if (c == 0 || b < a) { *lo = 0; *hi = 0; return; }
    *lo = pos[a]; *hi = pos[b];
}

// Extents of unit first + r.  Whole group; scratch of a BlockGroup on a 16-byte boundary (exscan_i64).
template <class G>
AMBI_HD void seq_extents_unit(const G& g, const UnitIn* units, const uint8_t* results, const SeqArgs& S, const SeqPlan& Q, int r, int which, int pass) {
    const int u = Q.first + r, tid = g.tid(), sz = g.size();
    const int n = units[u].n_seg;
    int P;
    const rcell_t* cells = seq_unit_path(units, results, u, which, &P);
    const int64_t* pos = S.seg_pos + S.pos_off[u];
    if (pass == 0) {
        // a cell's bytes are its segment's: no run structure needed for the total
        int runs = 0; int64_t bytes = 0;
        for (int i = tid; i < P; i += sz) {
            const int c = cells[i];
            runs += (i == 0 || c != cells[i - 1] + 1) ? 1 : 0;
            const int s = c < 0 ? -c : c;
            if (s >= 1 && s <= n) bytes += pos[s] - pos[s - 1];
        }
        runs = g.sum_i32(runs);
        int64_t total;
        (void)g.exscan_i64(bytes, &total);
        if (tid == 0) { Q.totals[2 * r] = total; Q.totals[2 * r + 1] = runs; }
        return;
    }
    const int64_t e0 = Q.ext_off[r];
    const int R = (int)(Q.ext_off[r + 1] - e0) - 1;   // the runs pass 0 counted
    int64_t* src = Q.ext_src + e0;
    int64_t* out = Q.ext_out + e0;
    // run starts in path order: first cell and, for now, position
    int done = 0;
    for (int base = 0; base < P; base += sz) {
        const int i = base + tid;
        const int flag = (i < P && (i == 0 || cells[i] != cells[i - 1] + 1)) ? 1 : 0;
        int tot;
        const int k = done + g.exscan_i32(flag, &tot);
        if (flag && k < R) { src[k] = cells[i]; out[k] = i; }
        done += tot;
    }
    g.sync();
    // position -> extent; the next run's position is read before the scan's barrier, and overwritten behind it
    const int64_t store = S.store_off[u];
    int64_t carry = 0;
    for (int base = 0; base < R; base += sz) {
        const int k = base + tid;
        int64_t lo = 0, hi = 0; int c = 0;
        if (k < R) {
            c = (int)src[k];
            const int len = (int)((k + 1 < R ? out[k + 1] : (int64_t)P) - out[k]);
            seq_run_range(pos, n, c, len, &lo, &hi);
        }
        int64_t tot;
        const int64_t ex = g.exscan_i64(hi - lo, &tot);
        g.sync();
        if (k < R) { src[k] = c > 0 ? store + lo : ~(store + lo); out[k] = carry + ex; }
        carry += tot;
        g.sync();
    }
    // the unit's length; 0 -- the fill stage then skips the unit -- if the path is no longer the one pass 0 counted (a caller that
    // starts the next run on another stream while this request is in flight): the output block was sized for that one
    if (tid == 0) out[R] = (done == R && carry == Q.totals[2 * r]) ? carry : 0;
}

struct Seq16 { uint32_t w[4]; };
struct __attribute__((aligned(16))) Seq16A { uint32_t w[4]; };
AMBI_HD uint32_t seq_revcomp4(uint32_t v, const uint8_t* table) {   // bytes 0 1 2 3 -> comp(3) comp(2) comp(1) comp(0)
    return (uint32_t)table[v >> 24] | ((uint32_t)table[(v >> 16) & 255u] << 8) | ((uint32_t)table[(v >> 8) & 255u] << 16) | ((uint32_t)table[v & 255u] << 24);
}

// Where the tile before left off: a group that takes consecutive tiles finds the next tile's unit and first run a step or two
// further on instead of by three bisections -- chains of dependent loads that bounded the kernel at 0.45 of a copy's byte rate
// (profiles/r13_notes.md).  r < 0: no tile yet.
struct SeqCursor { int r = -1, k = 0; };
// last index k' in [k, R) with eo[k'] <= key, from a k with eo[k] <= key: a few steps forward, else the bisection (key < eo[R])
AMBI_HD int seq_advance(const int64_t* eo, int k, int R, int64_t key) {
    for (int i = 0; i < 4 && eo[k + 1] <= key; i++) k++;
    return eo[k + 1] <= key ? seq_prefix_find(eo, k, R, key) : k;
}

// Tile t of the request; `cur` carries over to tile t + 1 (any tile may follow with a fresh cursor).  Whole group (no exchange
// between the threads; cur is uniform over the group); table: seq_build_table's.
template <class G>
AMBI_HD void seq_fill_tile(const G& g, const SeqArgs& S, const SeqPlan& Q, const uint8_t* table, int64_t t, SeqCursor& cur) {
    const bool fresh = cur.r < 0 || t < Q.tile_off[cur.r];
    if (fresh) { cur.r = seq_prefix_find(Q.tile_off, 0, Q.count, t); cur.k = 0; }
    else while (t >= Q.tile_off[cur.r + 1]) { cur.r++; cur.k = 0; }   // (t < tile_off[count])
    const int r = cur.r;
    const int64_t e0 = Q.ext_off[r];
    const int R = (int)(Q.ext_off[r + 1] - e0) - 1;
    if (R <= 0) return;
    const int64_t* src = Q.ext_src + e0;
    const int64_t* eo = Q.ext_out + e0;
    const int64_t len = eo[R], padded = pad16(len);
    const int64_t tb = (t - Q.tile_off[r]) * kSeqTile;
    if (tb >= padded || Q.out_off[r] + padded > Q.out_bytes) return;
    const int64_t last = (tb + kSeqTile < len ? tb + kSeqTile : len) - 1;   // last sequence byte of the tile
    if (cur.k >= R || eo[cur.k] > tb) cur.k = 0;   // (a cursor of another request, or of a tile further on)
    const int k0 = cur.k == 0 ? seq_prefix_find(eo, 0, R, tb) : seq_advance(eo, cur.k, R, tb), k1 = seq_advance(eo, k0, R, last);
    cur.k = k1;
    uint8_t* dst = Q.out + Q.out_off[r];
    for (int lane = g.tid(); lane < kSeqTileLanes; lane += g.size()) {
        const int64_t o = tb + (int64_t)lane * kSeqLaneBytes;
        if (o >= padded) break;
        int k = seq_prefix_find(eo, k0, k1 + 1, o < len ? o : len - 1);
        Seq16A v;
        if (o + kSeqLaneBytes <= eo[k + 1]) {   // the whole group inside run k
            const int64_t j = o - eo[k], s = src[k];
            Seq16 x;
            if (s >= 0) {
                memcpy(&x, S.bases + s + j, kSeqLaneBytes);
                for (int q = 0; q < 4; q++) v.w[q] = x.w[q];
            } else {
                const int64_t bytes = eo[k + 1] - eo[k];
                memcpy(&x, S.bases + ~s + (bytes - kSeqLaneBytes - j), kSeqLaneBytes);   // output j .. j + 15 = source bytes - 1 - j downwards
                for (int q = 0; q < 4; q++) v.w[q] = seq_revcomp4(x.w[3 - q], table);
            }
        } else {
            for (int q = 0; q < 4; q++) {
                uint32_t w = 0;
                for (int b = 0; b < 4; b++) {
                    const int64_t p = o + 4 * q + b;
                    if (p >= len) break;   // padding: zero
                    while (p >= eo[k + 1]) k++;   // (p < len = eo[R]: k stays below R)
                    const int64_t j = p - eo[k], s = src[k];
                    const uint8_t c = s >= 0 ? S.bases[s + j] : table[S.bases[~s + (eo[k + 1] - eo[k] - 1 - j)]];
                    w |= (uint32_t)c << (8 * b);
                }
                v.w[q] = w;
            }
        }
        *reinterpret_cast<Seq16A*>(dst + o) = v;
    }
}

// host code, every backend: what follows from the totals of pass 0 -- the extent slots, every unit's place in the output block
// (16-byte aligned) and its tiles
struct SeqLayout {
    std::vector<int64_t> len, ext_off, out_off, tile_off;
    int64_t seq_bytes = 0, out_bytes = 0, slots = 0, tiles = 0;   // sum of the lengths; bytes of the block; extent slots; tiles
};
inline void seq_layout(const int64_t* totals, int count, SeqLayout& L) {
    L.len.assign((size_t)count, 0); L.ext_off.assign((size_t)count + 1, 0); L.out_off.assign((size_t)count, 0); L.tile_off.assign((size_t)count + 1, 0);
    L.seq_bytes = 0; L.out_bytes = 0;
    for (int r = 0; r < count; r++) {
        const int64_t bytes = totals[2 * r], runs = totals[2 * r + 1];
        L.len[r] = bytes; L.seq_bytes += bytes;
        L.ext_off[r + 1] = L.ext_off[r] + runs + 1;
        L.out_off[r] = L.out_bytes; L.out_bytes += pad16(bytes);
        L.tile_off[r + 1] = L.tile_off[r] + (pad16(bytes) + kSeqTile - 1) / kSeqTile;
    }
    L.slots = L.ext_off[count]; L.tiles = L.tile_off[count];
}

}  // namespace ambi
