// ambi_pack.hpp -- host-side packing of units into the flat batch layout (ambi_batch.hpp).
// Pure host C++ (no HIP): shared by the HIP engine (ambi_engine.hip) and the CPU host simulation.
#pragma once
#include <string>
#include <vector>

#include "ambi_batch.hpp"
#include "lh_graph.hpp"

namespace ambi {

constexpr int kPathCapLimit = 1 << 22;   // cells per unit in the result blob (the lean finish stage streams them; only the full stage,
                                         // which edits the path in LDS, is limited to kPathLdsCells)
constexpr int kDefaultIdealCap = 4096; // slots per unit (holds up to 2048 order ideals)

// Sequence image of a batch (ambi_sequence.hpp): the bases of every unit's segments back to back in local id order, and per
// unit the int64 prefix seg_pos[0..n] of the segment lengths.  Host memory; a backend takes it to the device at the first
// sequence request.  A unit without attached bases has an empty store and a prefix of zeros.
struct SeqImage {
    std::vector<uint8_t> bases;
    std::vector<int64_t> seg_pos;      // all units' prefixes one after the other
    std::vector<int64_t> store_off;    // [U] byte offset of a unit's store in bases
    std::vector<int64_t> pos_off;      // [U] index of a unit's seg_pos[0]
    bool any = false;                  // some unit has bases
    int64_t version = 0;               // moves with every change (a backend re-sends an image it has already taken to the device)
    // the bases of unit `unit`: local segment i + 1 = src[seg_off[i] .. seg_off[i + 1]) (seg_off ascending); a second call replaces the first
    void set(size_t unit, int n_seg, const uint8_t* src, const int64_t* seg_off) {
        if (store_off.size() <= unit) { store_off.resize(unit + 1, 0); pos_off.resize(unit + 1, -1); }
        store_off[unit] = (int64_t)bases.size();
        pos_off[unit] = (int64_t)seg_pos.size();
        for (int i = 0; i <= n_seg; i++) seg_pos.push_back(seg_off[i] - seg_off[0]);
        if (seg_off[n_seg] > seg_off[0]) bases.insert(bases.end(), src + seg_off[0], src + seg_off[n_seg]);
        any = true; version++;
    }
    // every unit has a prefix afterwards (zeros where nothing was attached); idempotent
    void seal(const std::vector<UnitIn>& units) {
        if (store_off.size() < units.size()) { store_off.resize(units.size(), 0); pos_off.resize(units.size(), -1); }
        for (size_t u = 0; u < units.size(); u++)
            if (pos_off[u] < 0) { pos_off[u] = (int64_t)seg_pos.size(); seg_pos.insert(seg_pos.end(), (size_t)units[u].n_seg + 1, 0); version++; }
    }
    // unit u of another image (ambi_batch_run_sharded deals units to shares)
    void copy_unit(size_t unit, int n_seg, const SeqImage& from, size_t u) {
        if (u >= from.pos_off.size() || from.pos_off[u] < 0) return;
        const int64_t* p = from.seg_pos.data() + from.pos_off[u];
        std::vector<int64_t> off(p, p + n_seg + 1);
        for (auto& o : off) o += from.store_off[u];
        set(unit, n_seg, from.bases.data(), off.data());
    }
};

// Fragment image of a batch (ambi_frag_profile.hpp): the units' .juncs fragments as chains of LOCAL signed ids back to back, per
// unit the int32 prefix frag_off[0..F] of the fragments' lengths (relative to the unit's first cell) and the map from the unit's
// fragment index to the graph's.  Host memory, with the life of the sequence image: nothing of it travels with the batch; a backend
// takes it to the device at the first fragment profile request and again when its version has moved.  A unit nobody gave
// fragments has F = 0.
constexpr int kMaxUnitFrags = 65535;
struct FragImage {
    std::vector<rcell_t> cells;
    std::vector<int32_t> frag_off;     // all units' prefixes one after the other
    std::vector<int64_t> cell_off;     // [U] index of a unit's first cell in cells
    std::vector<int64_t> pref_off;     // [U] index of a unit's frag_off[0], -1: not set yet
    std::vector<int32_t> n_frag;       // [U] F
    std::vector<std::vector<int32_t>> graph_index;   // [U] local fragment index -> index in the graph's list (empty: a raw unit)
    bool any = false;                  // some unit has fragments
    int max_f = 0;                     // most fragments of a unit
    int64_t version = 0;               // moves with every change
    // the fragments of unit `unit`: fragment f = src[off[f] .. off[f + 1]) (off ascending, every fragment two cells at least, the
    // whole below 2^31 cells: the callers check); a second call replaces the first
    void set(size_t unit, const rcell_t* src, const int64_t* off, int n, const int32_t* gidx) {
        if (pref_off.size() <= unit) { cell_off.resize(unit + 1, 0); pref_off.resize(unit + 1, -1); n_frag.resize(unit + 1, 0); graph_index.resize(unit + 1); }
        cell_off[unit] = (int64_t)cells.size();
        pref_off[unit] = (int64_t)frag_off.size();
        n_frag[unit] = n;
        for (int f = 0; f <= n; f++) frag_off.push_back((int32_t)(n > 0 ? off[f] - off[0] : 0));
        if (n > 0) cells.insert(cells.end(), src + off[0], src + off[n]);
        graph_index[unit].assign(gidx, gidx + (gidx ? n : 0));
        if (n > 0) any = true;
        if (n > max_f) max_f = n;
        version++;
    }
    // every unit has a prefix afterwards (F = 0 where nothing was attached); idempotent
    void seal(const std::vector<UnitIn>& units) {
        if (pref_off.size() < units.size()) { cell_off.resize(units.size(), 0); pref_off.resize(units.size(), -1); n_frag.resize(units.size(), 0); graph_index.resize(units.size()); }
        for (size_t u = 0; u < units.size(); u++)
            if (pref_off[u] < 0) { cell_off[u] = (int64_t)cells.size(); pref_off[u] = (int64_t)frag_off.size(); frag_off.push_back(0); version++; }
    }
    // unit u of another image (ambi_batch_run_sharded deals units to shares)
    void copy_unit(size_t unit, const FragImage& from, size_t u) {
        if (u >= from.pref_off.size() || from.pref_off[u] < 0) return;
        const int n = from.n_frag[u];
        std::vector<int64_t> off((size_t)n + 1);
        for (int f = 0; f <= n; f++) off[(size_t)f] = from.cell_off[u] + from.frag_off[(size_t)from.pref_off[u] + (size_t)f];
        set(unit, from.cells.data(), off.data(), n, from.graph_index[u].empty() ? nullptr : from.graph_index[u].data());
    }
};

// Length image of a batch (ambi_path_coords.hpp): per unit its n_seg segment lengths in base pairs, int32, in local id order.  Host
// memory, with the life of the other two images: nothing of it travels with the batch; a backend takes it to the device at the first
// path-coordinates request and again when its version has moved.  A unit nobody gave lengths has lengths of zero, as a unit without
// bases has an empty store: its amplicon is 0 bp long.
struct LenImage {
    std::vector<int32_t> len;          // all units' lengths one after the other
    std::vector<int64_t> len_off;      // [U] index of a unit's first length, -1: not set yet
    int64_t version = 0;               // moves with every change
    // the lengths of unit `unit`: local segment i + 1 is src[i] base pairs long (0 .. 2^31 - 1: the callers check); a second call replaces the first
    void set(size_t unit, int n_seg, const int32_t* src) {
        if (len_off.size() <= unit) len_off.resize(unit + 1, -1);
        len_off[unit] = (int64_t)len.size();
        len.insert(len.end(), src, src + n_seg);
        version++;
    }
    // every unit has lengths afterwards (zeros where nothing was attached); idempotent
    void seal(const std::vector<UnitIn>& units) {
        if (len_off.size() < units.size()) len_off.resize(units.size(), -1);
        for (size_t u = 0; u < units.size(); u++)
            if (len_off[u] < 0) { len_off[u] = (int64_t)len.size(); len.insert(len.end(), (size_t)units[u].n_seg, 0); version++; }
    }
};

struct HostBatch {
    std::vector<UnitIn> units;
    SeqImage seq;                      // bases of the units' segments (empty unless sequences were attached)
    FragImage frag;                    // .juncs fragments of the units (empty unless fragments were attached)
    LenImage len;                      // base-pair lengths of the units' segments (zeros unless lengths were attached)
    std::vector<double> seg_cn;
    std::vector<Junction> juncs;
    std::vector<JuncEnds> junc_ends;   // junc_ends(juncs[i]) of every record
    std::vector<double> junc_cn;       // juncs[i].cn: ends + copy number (12 bytes) are all the device reads of a junction
    std::vector<Element> elems;
    std::vector<int64_t> scratch_off;       // per unit, ints
    std::vector<int64_t> run_slot;          // [U+1] slots of the units' final paths in run-length form (BatchArgs::run_slot); filled by finalize()
    std::vector<std::vector<int32_t>> junc_global;   // per unit: local junction index -> index in the sample's graph
    int64_t result_bytes = 0, ideal_slots = 0, scratch_ints = 0;
    int max_n = 0, max_m = 0, max_k = 0, max_bkp = 0, max_path = 0, max_out = 0;
    int ideal_cap = kDefaultIdealCap;
    int n_wide = 0;                         // units with 64..127 DAG nodes (ambi_wide.hpp)
    std::vector<int32_t> wide_index;        // [U] index among the wide units or -1; filled by finalize()
    bool any_sv = false;                    // some unit has a junction indelBFB would look at (neither adjacency nor fold-back): the full finish stage may be needed
    // diagnostics hook (ambi_batch_debug_inject_validity): verdict overrides per unit, see BatchArgs::inject_valid
    std::vector<int8_t> inject;             // [n_armed][kDebugOrderBytes] slots (zero), then the verdicts
    std::vector<int64_t> inject_off;        // [U][kInjectStride] {offset of the verdicts in `inject` or -1, count, slot or -1}; filled by finalize()
    int n_armed = 0;                        // units with injected verdicts (= slots at the front of `inject`)
    std::vector<std::vector<int8_t>> inject_unit;

    // Raw unit: local ids 1..n_seg, junctions already restricted to the unit.  Returns unit index or negative Status.
    int add_unit(int n_seg, int seg_base, const double* cn_local /*[n_seg], id 1 first*/, int n_junc, const int32_t* j_src,
                 const int32_t* j_tgt, const int8_t* j_sdir, const int8_t* j_tdir, const double* j_cn, int n_elem,
                 const int32_t* e_is_loop, const int32_t* e_a, const int32_t* e_b, const int32_t* e_cn, int infeasible,
                 int has_components);
    // One chromosome of a parsed .lh plus the .sol columns of that chromosome (localhap.cpp:111-232).
    // block / n_blocks: `--op sc_bfb` (localhap.cpp:540-566): the solution of graph `block` sits in the columns
    // [block*numComp, (block+1)*numComp) of a joint .sol; such a unit never takes the no-fold-back shortcut (that decision
    // is the caller's, from the first graph alone, localhap.cpp:505-512).
    int add_graph_chr(const LhGraph& g, int chr, const SolFile* sol, int block = 0, int n_blocks = 0);
    // Appends a copy of unit `u` of another batch (its packed inputs, capacities, junction map, injected verdicts): how a batch
    // is dealt over several devices (ambi_batch_run_sharded).  Returns the new unit's index.
    int add_unit_from(const HostBatch& src, int u);
    void finalize();                          // computes result/ideal/scratch offsets
    int64_t header_bytes() const { return int64_t(sizeof(UnitOut)) * (int64_t)units.size(); }
};

}  // namespace ambi
