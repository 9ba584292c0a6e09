// ambi_backend.hpp -- what the C-ABI layer (ambi_capi.cpp) needs from an execution backend.
// The product links exactly one implementation: the HIP engine (ambi_engine.hip).  tests/hostsim links the same
// C-ABI layer against a 1-thread host simulation of the SAME stage code for CPU-only checks; it is never shipped
// in ambigram_amd/ and never selected at run time.
#pragma once
#include <stdint.h>
#include <initializer_list>
#include <vector>

#include "ambi_pack.hpp"
#include "ambi_evidence_profile.hpp"
#include "ambi_fold_profile.hpp"
#include "ambi_frag_profile.hpp"
#include "ambi_junc_profile.hpp"
#include "ambi_path_align.hpp"
#include "ambi_path_compare.hpp"
#include "ambi_path_coords.hpp"
#include "ambi_profile.hpp"
#include "ambi_sequence.hpp"

namespace ambi {

struct EngineConfig {
    int64_t order_arena_bytes = 0;   // 0: sized from the first run
    int32_t first_budget = 64;
    int32_t block_lds = 49152;       // LDS bytes per workgroup for a unit's block-emission image (env AMBI_BLOCK_LDS overrides)
    int32_t block_scratch_lds = 16384;   // LDS of the image-build kernel (automaton copy; env AMBI_BLOCK_SCRATCH_LDS overrides)
    int32_t block_max = 256;         // largest suffix block in rows (env AMBI_BLOCK_MAX overrides; rows of a byte per node: 128 / 192 / 256 / 320 measure the same, profiles/r01_slices.md; 5-bit rows: 64 / 96 / 128 / 192 / 256 / 320 / 384 / 512 = 1.47 / 1.01 / 0.918 / 0.92 / 0.900 / 0.903 / 0.914 / 1.00 ms per step, profiles/r03_notes.md; an image that does not fit the LDS budget sends the unit down the general path)
    int32_t target_lanes = 524288;   // enumerate kernel: rows of the batch are spread over about this many lanes
};

struct KernelTime { const char* name; float ms; float start_ms = -1.f, end_ms = -1.f; };   // start / end: from the start of the run's first kernel (mean over the timed runs; -1: not known)
// the final paths of a batch in run-length form, in HOST memory (Backend::runs_wait): per unit its cells and runs, then the runs of
// all units one after the other (start value = absolute signed segment id, length); headers: UnitOut[U] or nullptr
struct RunsView {
    int64_t n_runs, n_cells;
    const int32_t* lengths; const int32_t* run_counts; const int32_t* run_start; const int32_t* run_len;
    const int64_t* run_off;      // [U+1] unit u's runs are run_start / run_len [run_off[u] .. run_off[u] + run_counts[u])
    const void* headers;
    int64_t bytes, copied_bytes;
};

class Backend {
  public:
    virtual ~Backend() {}
    virtual const char* name() const = 0;
    virtual int device_count(int* n) = 0;
    virtual int set_device(int d) = 0;
    virtual int upload(const HostBatch& hb, const EngineConfig& cfg) = 0;
    virtual int run(uint32_t flags, void* stream) = 0;
    // a stream of the backend's own on its device (process lifetime), for callers that have none to pass: nullptr = none (the host
    // simulation); and a counter that moves whenever the results on the device change after run() has returned (the first run of a
    // batch done again with a larger arena, units finished by the parallel search at wait())
    virtual void* own_stream() { return nullptr; }
    virtual int64_t results_epoch() const { return 0; }
    virtual int wait() = 0;
    virtual int wait_results() { return wait(); }   // results complete; order tables may still be in flight (express path)
    virtual int download(std::vector<uint8_t>& blob) = 0;
    // Header, final path(s) and output junctions of a unit where the HOST can read them without a copy command (MailLayout,
    // ambi_batch.hpp), valid after wait_results() / wait() of a small batch; nullptr: download the blob instead
    virtual const uint8_t* mail_slot(int unit) { (void)unit; return nullptr; }
    virtual int device_results(void** ptr, int64_t* bytes) = 0;
    virtual int pack_runs(int which, int32_t* dev_lengths, int32_t* dev_run_counts, int32_t* dev_run_start, int32_t* dev_run_len,
                          int64_t run_cap, int64_t* dev_totals, void* stream) = 0;
    virtual int pack_paths(int which, int32_t* dev_lengths, int32_t* dev_cells, int64_t cell_cap, int64_t* dev_total,
                           void* stream) = 0;
    // final paths (which: 0 getBFB, 1 after indelBFB) packed into run-length form and copied to pinned host memory behind `stream`,
    // without blocking it: slot 0 / 1 alternate so that the copy of one run travels while the next run computes
    virtual int runs_to_host(int which, int slot, int with_headers, void* stream) { (void)which; (void)slot; (void)with_headers; (void)stream; return ST_ERR_BAD_INPUT; }
    virtual int runs_wait(int slot, RunsView* out) { (void)slot; (void)out; return ST_ERR_BAD_INPUT; }
    virtual int copy_orders(int unit, int64_t first, int64_t count, uint8_t* out) = 0;
    // diagnostics: the kDebugOrderBytes of BatchArgs::debug_order of a unit with injected verdicts (all zero: no stage stored a row)
    virtual int copy_debug_order(int unit, uint8_t* out) { (void)unit; (void)out; return ST_ERR_BAD_INPUT; }
    virtual int copy_dag(int unit, Dag* out) = 0;
    // the same for a wide unit (64..127 nodes): node records [K][3] each, successor sets as [K][2] 64-bit words
    virtual int copy_dag_wide(int unit, int32_t* pat, int32_t* loop, uint64_t* succ2) { (void)unit; (void)pat; (void)loop; (void)succ2; return ST_ERR_BAD_INPUT; }
    virtual void set_timing(bool on) = 0;
    virtual void set_timing_mask(uint32_t mask) { set_timing(mask != 0); }
    virtual const std::vector<KernelTime>& kernel_times() = 0;
    virtual int64_t order_bytes_written() const = 0;
    virtual size_t object_bytes() const = 0;   // sizeof the concrete backend (diagnostics: ambi_batch_destroy's quarantine mode)
    virtual int slice_count() const { return 1; }   // launches of every kernel per run (ambi_batch_slices: always one)
    // --all (run with FLAG_ALL, after wait): valid orders of pass 0 (first orientation) / pass 1 (flipped orientation,
    // empty unless the last order of pass 0 is invalid), and the paths of a range of them (cells: count x stride int32)
    virtual int all_count(int unit, int pass, int64_t* count) = 0;
    virtual int all_orders(int unit, int pass, int64_t first, int64_t count, int64_t* idx) = 0;
    // --all with the orders of a unit dealt over `world` ranks (see BatchArgs::all_rank): set before run; after wait() every
    // rank merges the pool all_device() names (bitmaps + flags, bytes: MAX over the ranks) and calls all_finish()
    virtual int set_shard(int rank, int world) = 0;
    virtual int all_device(void** ptr, int64_t* bytes) = 0;
    virtual int all_finish() = 0;
    virtual int all_paths(int unit, int pass, int64_t first, int64_t count, int32_t* lengths, int32_t* cells, int64_t stride) = 0;

    // ---- on-request profiles of every unit's path (which: 0 getBFB, 1 after indelBFB) ----
    // Eight kinds, one life cycle.  A kind is a block that travels to the host, a tail behind it that travels up once per layout (int64
    // offsets per unit, or the request's entries), a side area that stays where it was computed, an image that goes up when the device
    // holds another version of it, and its kernels (U: units; [..]: arrays padded to 16 bytes):
    //   kind         block                                               tail                  side area                   image      kernels (ambi_*_kernel)
    //   kCopyNumber  [UnitProfile[U]] per unit [fwd][rev]                off[U]                -                           -          path_profile
    //   kJunction    [UnitJuncProfile[U]] per unit [count]               off[U]                -                           -          junc_profile
    //   kFragment    [UnitFragProfile[U]] per unit [fwd][rev][first]     off[U]                -                           fragment   frag_profile
    //   kEvidence    [UnitEvidenceProfile[U]] per unit [count][covered]  off[U], depth_off[U]  depth: int32 per cell of    fragment   evidence_mark, evidence_scan
    //                [min_depth]                                                               every unit's path capacity
    //   kFold        [UnitFoldProfile[U]] per unit [folds][max_arm]      off[U], plane_off[U]  fold plane, then cover      -          fold_arm, fold_scan
    //                                                                                          plane, each as the depth
    //   kCompare     [PathCompare[n]]                                    n pairs (A, B)        -                           its given  path_compare
    //   kAlign       [PathAlign[n]] [AlignRun[n * dmax]]                 n triples (A, B, o)   a history area per          its given  path_align
    //                                                                                          workgroup
    //   kCoords      [UnitCoords[U]] [PathLift[n]]                       plane_off[U],         plane: int64 per cell of    length     path_coords, path_lift
    //                                                                    n queries             every unit's path capacity
    //                                                                                          plus one
    // (stage code: ambi_profile.hpp, ambi_junc_profile.hpp, ambi_frag_profile.hpp, ambi_evidence_profile.hpp, ambi_fold_profile.hpp,
    // ambi_path_compare.hpp, ambi_path_align.hpp, ambi_path_coords.hpp.)
    // The last three bring their entries with the request (compare(), align() and coords() below) and are laid out with every request.
    // profile() queues the block of the last run's results behind that run, profile_wait() waits for it in host memory; the typed
    // getters below then answer from that copy.  The default runs the stage on the host over the downloaded blob (the host
    // simulation); the HIP engine overrides the virtual entries with its kernels and never reaches it.
    // profile_bind: the packed inputs the backend was (or will be) uploaded with; they outlive the backend.
    enum ProfileKind { kCopyNumber = 0, kJunction = 1, kFragment = 2, kEvidence = 3, kFold = 4, kCompare = 5, kAlign = 6, kCoords = 7 };
    static constexpr int kProfileKinds = 8;
    void profile_bind(const HostBatch* hb) { prof_hb_ = hb; for (ProfileState& P : prof_) P.view = nullptr; }
    virtual int profile(ProfileKind kind, int which, void* stream) {
        (void)stream;
        if (!prof_hb_ || which < 0 || which > 1) return ST_ERR_BAD_INPUT;
        std::vector<uint8_t> blob;
        if (int rc = download(blob)) return rc;
        ProfileState& P = prof_[kind];
        profile_layout(kind);
        P.blob.assign((size_t)P.bytes, 0);
        switch (kind) {
            case kCopyNumber: host_profile(blob.data(), which, P); break;
            case kJunction: host_junc_profile(blob.data(), which, P); break;
            case kFragment: host_frag_profile(blob.data(), which, P); break;
            case kEvidence: host_evidence_profile(blob.data(), which, P); break;
            case kFold: host_fold_profile(blob.data(), which, P); break;
            case kCompare: host_compare(blob.data(), P); break;
            case kAlign: host_align(blob.data(), P); break;
            case kCoords: host_coords(blob.data(), which, P); break;
        }
        P.view = nullptr;
        return 0;
    }
    virtual int profile_wait(ProfileKind kind) {
        ProfileState& P = prof_[kind];
        if (P.blob.empty()) return ST_ERR_BAD_INPUT;
        // (the coords kind promises the LAST run's paths whatever ran between request and wait: the engine queues it again when the
        // results' epoch has moved; here, where nothing counts epochs, the request is simply answered once more from its own copy)
        if (kind == kCoords) { if (int rc = profile(kCoords, coords_which_, nullptr)) return rc; }
        P.view = P.blob.data();
        return 0;
    }
    // the block where the collectives of the caller can read it (device memory of the HIP engine), valid after profile_wait()
    virtual int profile_device(ProfileKind kind, void** ptr, int64_t* bytes) {
        ProfileState& P = prof_[kind];
        if (!P.view) return ST_ERR_BAD_INPUT;
        if (ptr) *ptr = P.blob.data();
        if (bytes) *bytes = P.bytes;
        return 0;
    }
    // The typed getters: a unit's summary, and `n` int32 values from each of the unit's arrays (arr_bytes apart) to every destination
    // that is not nullptr; counts_of returns n, and refuses n < 0 (unit_n: the bound batch has no such unit) and cap < n.
    template <class T> int summary_of(ProfileKind kind, int unit, T* out) const {
        const ProfileState& P = prof_[kind];
        if (!P.view || unit < 0 || unit >= (int)P.off.size() || !out) return ST_ERR_BAD_INPUT;
        *out = reinterpret_cast<const T*>(P.view)[unit];
        return 0;
    }
    int counts_of(ProfileKind kind, int unit, int n, int cap, int64_t arr_bytes, std::initializer_list<int32_t*> to) const {
        const ProfileState& P = prof_[kind];
        if (!P.view || unit < 0 || unit >= (int)P.off.size() || n < 0 || cap < n) return ST_ERR_BAD_INPUT;
        const uint8_t* p = P.view + P.off[(size_t)unit];
        for (int32_t* dst : to) { if (dst && n > 0) memcpy(dst, p, sizeof(int32_t) * (size_t)n); p += arr_bytes; }
        return n;
    }
    int unit_n(int unit, int32_t UnitIn::*what, int more = 0) const { return prof_hb_ && unit >= 0 && (size_t)unit < prof_hb_->units.size() ? prof_hb_->units[(size_t)unit].*what + more : -1; }
    int unit_frags(int unit) const { return prof_hb_ && unit >= 0 && (size_t)unit < prof_hb_->frag.n_frag.size() ? prof_hb_->frag.n_frag[(size_t)unit] : -1; }
    int profile_summary(int unit, UnitProfile* out) const { return summary_of(kCopyNumber, unit, out); }
    int profile_counts(int unit, int32_t* fwd, int32_t* rev, int cap) const {   // n + 1 counts each; returns n + 1
        const int n1 = unit_n(unit, &UnitIn::n_seg, 1);
        return counts_of(kCopyNumber, unit, n1, cap, profile_rev_off(n1 - 1), {fwd, rev});
    }
    int junc_profile_summary(int unit, UnitJuncProfile* out) const { return summary_of(kJunction, unit, out); }
    int junc_profile_counts(int unit, int32_t* count, int cap) const { return counts_of(kJunction, unit, unit_n(unit, &UnitIn::n_junc), cap, 0, {count}); }   // m counts; returns m
    int frag_profile_summary(int unit, UnitFragProfile* out) const { return summary_of(kFragment, unit, out); }
    int frag_profile_counts(int unit, int32_t* fwd, int32_t* rev, int32_t* first, int cap) const {   // F values each; returns F
        const int F = unit_frags(unit);
        return counts_of(kFragment, unit, F, cap, frag_profile_arr_bytes(F), {fwd, rev, first});
    }
    int evidence_summary(int unit, UnitEvidenceProfile* out) const { return summary_of(kEvidence, unit, out); }
    int evidence_counts(int unit, int32_t* count, int32_t* covered, int32_t* min_depth, int cap) const {   // m values each; returns m
        const int m = unit_n(unit, &UnitIn::n_junc);
        return counts_of(kEvidence, unit, m, cap, evidence_arr_bytes(m), {count, covered, min_depth});
    }
    // the depths of the steps [first, first + n) of a unit to host memory (nothing else of the depth area travels), and the area where
    // it was computed (device memory of the HIP engine) with every unit's byte offset in it; valid after profile_wait(kEvidence)
    virtual int evidence_depth_copy(int unit, int64_t first, int64_t n, int32_t* out) {
        const ProfileState& P = prof_[kEvidence];
        if (!P.view || unit < 0 || unit >= (int)P.off.size() || n < 0 || (n > 0 && !out)) return ST_ERR_BAD_INPUT;
        if (n > 0) memcpy(out, reinterpret_cast<const uint8_t*>(depth_.data()) + depth_off_[(size_t)unit] + 4 * first, (size_t)(4 * n));
        return 0;
    }
    virtual int evidence_depth_device(void** ptr, int64_t* bytes, int64_t* unit_off, int cap) {
        if (!prof_[kEvidence].view) return ST_ERR_BAD_INPUT;
        if (ptr) *ptr = depth_.data();
        return evidence_depth_offsets(bytes, unit_off, cap);
    }

    int fold_summary(int unit, UnitFoldProfile* out) const { return summary_of(kFold, unit, out); }
    int fold_counts(int unit, int32_t* folds, int32_t* max_arm, int cap) const {   // m values each; returns m
        const int m = unit_n(unit, &UnitIn::n_junc);
        return counts_of(kFold, unit, m, cap, fold_arr_bytes(m), {folds, max_arm});
    }
    // the entries [first, first + n) of a unit's plane (0: fold, 1: cover) to host memory (nothing else of the plane area travels),
    // and the area where it was computed (device memory of the HIP engine: both planes, `bytes` in all, plane p of unit u at
    // p * bytes / 2 + unit_off[u]); valid after profile_wait(kFold)
    virtual int fold_plane_copy(int unit, int plane, int64_t first, int64_t n, int32_t* out) {
        const ProfileState& P = prof_[kFold];
        if (!P.view || unit < 0 || unit >= (int)P.off.size() || plane < 0 || plane > 1 || n < 0 || (n > 0 && !out)) return ST_ERR_BAD_INPUT;
        if (n > 0) memcpy(out, reinterpret_cast<const uint8_t*>(planes_.data()) + plane * plane_bytes_ + plane_off_[(size_t)unit] + 4 * first, (size_t)(4 * n));
        return 0;
    }
    virtual int fold_planes_device(void** ptr, int64_t* bytes, int64_t* unit_off, int cap) {
        if (!prof_[kFold].view) return ST_ERR_BAD_INPUT;
        if (ptr) *ptr = planes_.data();
        return fold_plane_offsets(bytes, unit_off, cap);
    }

    // ---- the requests that bring their entries: path comparison (ambi_path_compare.hpp, kCompare) and alignment (ambi_path_align.hpp, kAlign) ----
    // A PairRequest is the WHOLE request -- the entries (compare: pairs of sides, 2 * unit + which or ~t for the t-th given path;
    // align: triples (A, B, orient)), the cap and a copy of the given paths as they were when it was made -- queued as the other
    // kinds are queued (profile(kind)).  A request that profile_wait() has to queue again finds all of it here: the caller may replace
    // its set of given paths between a request and its wait, and the request still works on what it named.  The copy is taken only
    // when the caller's set has another version, and each kind has a copy of its own: the two never share one, so neither a new set
    // nor the other kind's request reaches a queued one.  A given side beyond the copied set is refused here as well, whatever the
    // caller checked.
    struct PairRequest {
        ComparePaths given;              // (version 0: the empty set, as the caller's before its first set)
        std::vector<int32_t> entries;
        int width;                       // int32 per entry: 2 (compare) or 3 (align)
        int dmax = kCompareDmaxDefault;
        int n() const { return (int)(entries.size() / (size_t)width); }
    };
    int compare(const ComparePaths* given, const int32_t* pairs, int n_pairs, int dmax, void* stream) { return pair_request(kCompare, given, pairs, n_pairs, dmax, stream); }
    int align(const ComparePaths* given, const int32_t* triples, int n_pairs, int dmax, void* stream) { return pair_request(kAlign, given, triples, n_pairs, dmax, stream); }
    static constexpr int kAlignTooLarge = kSeqTooLarge;   // AMBI_ERR_TOO_LARGE, as the sequence request's refusal
    int compare_pairs() const { return pair_of(kCompare).n(); }
    int align_pairs() const { return pair_of(kAlign).n(); }
    int compare_result(int pair, PathCompare* out) const { return pair_result(kCompare, pair, out); }
    int align_result(int pair, PathAlign* out) const { return pair_result(kAlign, pair, out); }
    const AlignRun* align_runs(int pair) const {   // the pair's align_stride(dmax) slots, nullptr without a waited-for request
        const ProfileState& P = prof_[kAlign];
        if (!P.view || pair < 0 || pair >= align_pairs()) return nullptr;
        return reinterpret_cast<const AlignRun*>(P.view + align_runs_off(align_pairs())) + (int64_t)pair * align_stride(pair_of(kAlign).dmax);
    }

    // ---- path coordinates (ambi_path_coords.hpp, kCoords): every request scans every unit's path into the plane and answers its queries ----
    // The request owns a copy of its queries, as a PairRequest owns its entries: a request that profile_wait() has to queue again
    // answers what it was asked.  A unit index outside the bound batch is refused here, never on the device.  n = 0 is "just the
    // coordinates".  The bound batch's length image (HostBatch::len) must be sealed.
    int coords(int which, const LiftQuery* queries, int n, void* stream) {
        if (!prof_hb_ || n < 0 || (n > 0 && !queries)) return ST_ERR_BAD_INPUT;
        for (int i = 0; i < n; i++) if (queries[i].unit < 0 || (size_t)queries[i].unit >= prof_hb_->units.size()) return ST_ERR_BAD_INPUT;
        lift_.assign(queries, queries + n);
        coords_which_ = which;
        return profile(kCoords, which, stream);
    }
    int coords_queries() const { return (int)lift_.size(); }
    int coords_summary(int unit, UnitCoords* out) const {
        const ProfileState& P = prof_[kCoords];
        if (!P.view || unit < 0 || unit >= (int)cplane_off_.size() || !out) return ST_ERR_BAD_INPUT;
        *out = reinterpret_cast<const UnitCoords*>(P.view)[unit];
        return 0;
    }
    int coords_result(int query, PathLift* out) const {
        const ProfileState& P = prof_[kCoords];
        if (!P.view || query < 0 || query >= coords_queries() || !out) return ST_ERR_BAD_INPUT;
        *out = reinterpret_cast<const PathLift*>(P.view + coords_results_off((int64_t)cplane_off_.size()))[query];
        return 0;
    }
    // the entries [first, first + n) of a unit's plane to host memory (nothing else of the plane area travels), and the area where it
    // was computed (device memory of the HIP engine) with every unit's byte offset in it; valid after profile_wait(kCoords)
    virtual int coords_copy(int unit, int64_t first, int64_t n, int64_t* out) {
        const ProfileState& P = prof_[kCoords];
        if (!P.view || unit < 0 || unit >= (int)cplane_off_.size() || n < 0 || (n > 0 && !out)) return ST_ERR_BAD_INPUT;
        if (n > 0) memcpy(out, reinterpret_cast<const uint8_t*>(cplanes_.data()) + cplane_off_[(size_t)unit] + 8 * first, (size_t)(8 * n));
        return 0;
    }
    virtual int coords_device(void** ptr, int64_t* bytes, int64_t* unit_off, int cap) {
        if (!prof_[kCoords].view) return ST_ERR_BAD_INPUT;
        if (ptr) *ptr = cplanes_.data();
        return coords_plane_offsets(bytes, unit_off, cap);
    }

    // ---- nucleotide sequence of every unit's path (ambi_sequence.hpp; which as above) over the units [first, first + count) ----
    // sequence() runs pass 0 of the extents stage behind the last run and fetches its totals (count x {bytes, runs}: the one small
    // device-to-host trip of a request), sizes the extent arrays and the output block from them, and queues pass 1 and the fill
    // stage; kSeqTooLarge, with nothing assembled and the lengths readable, when the lengths sum to more than max_bytes > 0.
    // sequence_wait() makes the results final and assembles once more if that moved them.  The default runs the stages on the host
    // over the downloaded blob (the host simulation); the HIP engine overrides the four virtual entries.  The batch's sequence
    // image (HostBatch::seq of the bound inputs) must be sealed.
    virtual int sequence(int which, int first, int count, int64_t max_bytes, void* stream) {
        (void)stream;
        seq_state_ = 0; seq_queued_ = false;
        if (!prof_hb_ || !prof_hb_->seq.any || which < 0 || which > 1 || first < 0 || count < 1 || (size_t)first + (size_t)count > prof_hb_->units.size()) return ST_ERR_BAD_INPUT;
        std::vector<uint8_t> blob;
        if (int rc = download(blob)) return rc;
        const SeqImage& I = prof_hb_->seq;
        const SeqArgs S{I.bases.data(), I.seg_pos.data(), I.store_off.data(), I.pos_off.data()};
        std::vector<int64_t> totals((size_t)(2 * count));
        SeqPlan Q{};
        Q.first = first; Q.count = count; Q.totals = totals.data();
        HostGroup g;
        for (int r = 0; r < count; r++) seq_extents_unit(g, prof_hb_->units.data(), blob.data(), S, Q, r, which, 0);
        seq_layout(totals.data(), count, seq_lay_);
        seq_first_ = first; seq_count_ = count; seq_state_ = 1;
        if (max_bytes > 0 && seq_lay_.seq_bytes > max_bytes) return kSeqTooLarge;
        std::vector<int64_t> ext_src((size_t)seq_lay_.slots), ext_out((size_t)seq_lay_.slots);
        seq_out_.assign((size_t)(seq_lay_.out_bytes / 16), Seq16A{});
        Q.ext_off = seq_lay_.ext_off.data(); Q.ext_src = ext_src.data(); Q.ext_out = ext_out.data();
        Q.out_off = seq_lay_.out_off.data(); Q.tile_off = seq_lay_.tile_off.data();
        Q.out = reinterpret_cast<uint8_t*>(seq_out_.data()); Q.out_bytes = seq_lay_.out_bytes;
        for (int r = 0; r < count; r++) seq_extents_unit(g, prof_hb_->units.data(), blob.data(), S, Q, r, which, 1);
        uint8_t table[256];
        seq_build_table(g, table);
        SeqCursor cur;
        for (int64_t t = 0; t < seq_lay_.tiles; t++) seq_fill_tile(g, S, Q, table, t, cur);
        seq_queued_ = true;
        return 0;
    }
    virtual int sequence_wait() {
        if (seq_state_ < 1 || !seq_queued_) return ST_ERR_BAD_INPUT;
        seq_state_ = 2;
        return 0;
    }
    // bytes [first, first + count) of a unit's sequence to host memory; valid after sequence_wait()
    virtual int sequence_copy(int unit, int64_t first, int64_t count, uint8_t* out) {
        const int r = unit - seq_first_;
        if (seq_state_ < 2 || r < 0 || r >= seq_count_ || first < 0 || count < 0 || first + count > seq_lay_.len[(size_t)r] || (count > 0 && !out)) return ST_ERR_BAD_INPUT;
        if (count > 0) memcpy(out, reinterpret_cast<const uint8_t*>(seq_out_.data()) + seq_lay_.out_off[(size_t)r] + first, (size_t)count);
        return 0;
    }
    // the output block where it was assembled (device memory of the HIP engine) and every unit's byte offset in it (-1: a unit
    // outside the request); valid after sequence_wait()
    virtual int sequence_device(void** ptr, int64_t* bytes, int64_t* unit_off, int cap) {
        if (seq_state_ < 2 || !prof_hb_) return ST_ERR_BAD_INPUT;
        if (ptr) *ptr = seq_out_.data();
        return sequence_offsets(bytes, unit_off, cap);
    }
    // a unit's length: readable from sequence() on (also behind kSeqTooLarge), final after sequence_wait()
    int sequence_len(int unit, int64_t* len) const {
        const int r = unit - seq_first_;
        if (seq_state_ < 1 || r < 0 || r >= seq_count_ || !len) return ST_ERR_BAD_INPUT;
        *len = seq_lay_.len[(size_t)r];
        return 0;
    }
    void sequence_reset() { seq_state_ = 0; seq_queued_ = false; }
    void sequence_drop() { seq_queued_ = false; if (seq_state_ > 1) seq_state_ = 1; }   // the lengths stay, what was assembled is not read
    bool sequence_known() const { return seq_state_ >= 1; }

  protected:
    // one on-request profile block on the host side: where every unit's counts start in it, its size, the block in host memory once
    // profile_wait() has returned (nullptr: nothing to read), and the default implementation's own block
    struct ProfileState {
        std::vector<int64_t> off;
        int64_t bytes = 0;
        const uint8_t* view = nullptr;
        std::vector<uint8_t> blob;
    };
    ProfileState prof_[kProfileKinds];   // [ProfileKind]
    void profile_layout(ProfileKind kind) {   // off and bytes of the bound batch's block
        ProfileState& P = prof_[kind];
        const std::vector<UnitIn>& units = prof_hb_->units;
        switch (kind) {
            case kCopyNumber: P.bytes = profile_block_layout(units, P.off); break;
            case kJunction: P.bytes = junc_profile_block_layout(units, P.off); break;
            case kFragment: P.bytes = frag_profile_block_layout(prof_hb_->frag.n_frag.data(), units.size(), P.off); break;   // (sealed: the C-ABI layer does it before a request)
            case kEvidence: P.bytes = evidence_block_layout(units, P.off); depth_bytes_ = evidence_depth_layout(units, depth_off_); break;
            case kFold: P.bytes = fold_block_layout(units, P.off); plane_bytes_ = fold_plane_layout(units, plane_off_); break;
            case kCompare: P.bytes = compare_block_bytes(compare_pairs()); P.off.clear(); break;
            case kAlign: P.bytes = align_block_bytes(align_pairs(), pair_of(kAlign).dmax); P.off.clear(); break;
            case kCoords: P.bytes = coords_block_bytes((int64_t)units.size(), coords_queries()); P.off.clear(); cplane_bytes_ = coords_plane_layout(units, cplane_off_); break;
        }
    }
    // The windows of the bound batch; the environment variables (tests) can only shrink them (capped_window).
    static int env_int(const char* name) { const char* e = ambi_env(name); return e ? atoi(e) : 0; }   // 0 when unset
    void frag_profile_windows(int* pwin, int* slots) const {   // patterns per window and table slots
        *pwin = frag_window(prof_hb_->frag.max_f, env_int("AMBI_FPROFILE_FRAG_WINDOW"));
        *slots = frag_slots(*pwin);
    }
    int profile_window_of() const { return profile_window(prof_hb_->max_n, env_int("AMBI_PROFILE_WINDOW")); }   // segments per window
    void junc_profile_windows(int* jwin, int* slots, int* swin) const {   // junctions per pass, table slots and segments per window
        *jwin = junc_window(prof_hb_->max_m, env_int("AMBI_JPROFILE_JUNC_WINDOW"));
        *slots = junc_slots(*jwin);
        *swin = junc_seg_window(prof_hb_->max_n, env_int("AMBI_JPROFILE_SEG_WINDOW"));
    }
    void evidence_windows(int* jwin, int* slots) const {   // junctions per pass and table slots of the evidence scan stage
        *jwin = evidence_junc_window(prof_hb_->max_m, env_int("AMBI_JPROFILE_JUNC_WINDOW"));
        *slots = junc_slots(*jwin);
    }
    std::vector<int64_t> depth_off_;     // the evidence kind's depth area: every unit's byte offset and the size (profile_layout)
    int64_t depth_bytes_ = 0;
    int evidence_depth_offsets(int64_t* bytes, int64_t* unit_off, int cap) const {
        const int U = (int)depth_off_.size();
        if (unit_off && cap < U) return ST_ERR_BAD_INPUT;
        if (bytes) *bytes = depth_bytes_;
        if (unit_off) for (int u = 0; u < U; u++) unit_off[u] = depth_off_[(size_t)u];
        return 0;
    }
    void fold_windows(int* fwin, int* jwin, int* slots) const {   // folds per round, junctions per pass and table slots of the fold stages
        *fwin = fold_window(env_int("AMBI_FOLD_WINDOW"));
        *jwin = fold_junc_window(prof_hb_->max_m, env_int("AMBI_JPROFILE_JUNC_WINDOW"));
        *slots = junc_slots(*jwin);
    }
    std::vector<int64_t> plane_off_;     // the fold kind's planes: every unit's byte offset in a plane and ONE plane's size (profile_layout)
    int64_t plane_bytes_ = 0;
    int fold_plane_offsets(int64_t* bytes, int64_t* unit_off, int cap) const {
        const int U = (int)plane_off_.size();
        if (unit_off && cap < U) return ST_ERR_BAD_INPUT;
        if (bytes) *bytes = 2 * plane_bytes_;
        if (unit_off) for (int u = 0; u < U; u++) unit_off[u] = plane_off_[(size_t)u];
        return 0;
    }
    std::vector<int64_t> cplane_off_;    // the coords kind's plane: every unit's byte offset and the size (profile_layout)
    int64_t cplane_bytes_ = 0;
    std::vector<LiftQuery> lift_;        // the queries of the last coords(), and its `which`
    int coords_which_ = 1;
    int lift_grid_of(int threads) const { return lift_grid(coords_queries(), threads, env_int("AMBI_LIFT_GRID")); }
    int coords_plane_offsets(int64_t* bytes, int64_t* unit_off, int cap) const {
        const int U = (int)cplane_off_.size();
        if (unit_off && cap < U) return ST_ERR_BAD_INPUT;
        if (bytes) *bytes = cplane_bytes_;
        if (unit_off) for (int u = 0; u < U; u++) unit_off[u] = cplane_off_[(size_t)u];
        return 0;
    }
    int sequence_offsets(int64_t* bytes, int64_t* unit_off, int cap) const {
        const int U = (int)prof_hb_->units.size();
        if (unit_off && cap < U) return ST_ERR_BAD_INPUT;
        if (bytes) *bytes = seq_lay_.out_bytes;
        if (unit_off) for (int u = 0; u < U; u++) unit_off[u] = (u < seq_first_ || u >= seq_first_ + seq_count_) ? -1 : seq_lay_.out_off[(size_t)(u - seq_first_)];
        return 0;
    }
    SeqLayout seq_lay_;                  // of the last request
    int seq_first_ = 0, seq_count_ = 0;
    int seq_state_ = 0;                  // 0: no request; 1: lengths known; 2: sequence_wait() has returned, the getters answer
    bool seq_queued_ = false;            // the stages of the last request have been queued (false behind kSeqTooLarge)
    const HostBatch* prof_hb_ = nullptr;
    // the last compare() and align(), [kind - kCompare]; the workgroups of a request (for the align kind each with a history area):
    // AMBI_COMPARE_GRID and AMBI_ALIGN_GRID (tests) can only shrink them
    PairRequest pair_[2] = {{{}, {}, 2}, {{}, {}, 3}};
    const PairRequest& pair_of(ProfileKind kind) const { return pair_[kind - kCompare]; }
    int compare_grid() const { return capped_window(compare_pairs(), kCompareGridCap, env_int("AMBI_COMPARE_GRID")); }
    int align_grid_of() const { return align_grid(align_pairs(), pair_of(kAlign).dmax, env_int("AMBI_ALIGN_GRID")); }
  private:
    int pair_request(ProfileKind kind, const ComparePaths* given, const int32_t* entries, int n, int dmax, void* stream) {
        PairRequest& Q = pair_[kind - kCompare];
        if (!given || n < 0 || (n > 0 && !entries) || dmax < 0 || dmax > kCompareDmaxCap) return ST_ERR_BAD_INPUT;
        for (int64_t i = 0; i < (int64_t)n; i++)
            for (int q = 0; q < 2; q++) if (entries[Q.width * i + q] < 0 && ~entries[Q.width * i + q] >= given->n()) return ST_ERR_BAD_INPUT;
        if (kind == kAlign) {   // (its own two, behind the shared ones: the orientation, and a run area above kAlignRunAreaCap, refused in front of any allocation)
            for (int64_t i = 0; i < (int64_t)n; i++) if (entries[3 * i + 2] < 0 || entries[3 * i + 2] > 1) return ST_ERR_BAD_INPUT;
            if (align_run_area_bytes(n, dmax) > kAlignRunAreaCap) return kAlignTooLarge;
        }
        if (Q.given.version != given->version) Q.given = *given;
        Q.dmax = dmax;
        Q.entries.assign(entries, entries + (size_t)Q.width * (size_t)n);
        return profile(kind, 1, stream);
    }
    template <class T> int pair_result(ProfileKind kind, int pair, T* out) const {
        const ProfileState& P = prof_[kind];
        if (!P.view || pair < 0 || pair >= pair_of(kind).n() || !out) return ST_ERR_BAD_INPUT;
        *out = reinterpret_cast<const T*>(P.view)[pair];
        return 0;
    }
    // a request's given set as the stages read it (ComparePaths::image), in host memory
    static CompareGiven host_given(const PairRequest& Q, std::vector<Seq16A>& image) {
        image.resize((size_t)(Q.given.image_bytes() / 16) + 1);
        uint8_t* img = reinterpret_cast<uint8_t*>(image.data());
        Q.given.image(img);
        return compare_given(img, Q.given);
    }
    void host_profile(const uint8_t* blob, int which, ProfileState& P) {
        const std::vector<UnitIn>& units = prof_hb_->units;
        const int window = profile_window_of();
        std::vector<int32_t> bins((size_t)(2 * window));
        HostGroup g;
        for (size_t u = 0; u < units.size(); u++) profile_unit(g, units.data(), blob, (int)u, which, window, bins.data(), P.blob.data(), P.off.data());
    }
    void host_junc_profile(const uint8_t* blob, int which, ProfileState& P) {
        const std::vector<UnitIn>& units = prof_hb_->units;
        int jwin, slots, swin;
        junc_profile_windows(&jwin, &slots, &swin);
        std::vector<int32_t> lds((size_t)(junc_profile_lds_bytes(slots, swin) / 4));
        const JuncTable T = junc_table(lds.data(), slots, swin);
        HostGroup g;
        for (size_t u = 0; u < units.size(); u++)
            junc_profile_unit(g, units.data(), prof_hb_->junc_ends.data(), prof_hb_->junc_cn.data(), blob, (int)u, which, jwin, T, P.blob.data(), P.off.data());
    }
    void host_frag_profile(const uint8_t* blob, int which, ProfileState& P) {
        const std::vector<UnitIn>& units = prof_hb_->units;
        const FragImage& I = prof_hb_->frag;
        int pwin, slots;
        frag_profile_windows(&pwin, &slots);
        std::vector<int32_t> lds((size_t)(frag_profile_lds_bytes(slots, pwin) / 4));
        const FragTable T = frag_table(lds.data(), slots, pwin);
        const FragArgs A{I.cells.data(), I.frag_off.data(), I.cell_off.data(), I.pref_off.data(), I.n_frag.data()};
        HostGroup g;
        for (size_t u = 0; u < units.size(); u++) frag_profile_unit(g, units.data(), A, blob, (int)u, which, T, P.blob.data(), P.off.data());
    }
    void host_evidence_profile(const uint8_t* blob, int which, ProfileState& P) {
        const std::vector<UnitIn>& units = prof_hb_->units;
        const FragImage& I = prof_hb_->frag;
        int pwin, fslots, jwin, slots;
        frag_profile_windows(&pwin, &fslots);
        evidence_windows(&jwin, &slots);
        std::vector<int32_t> lds((size_t)(frag_profile_lds_bytes(fslots, pwin) / 4)), lds2((size_t)(evidence_scan_lds_bytes(slots, 1) / 4));
        const FragTable T = frag_table(lds.data(), fslots, pwin);
        const EvidenceTable E = evidence_table(lds2.data(), slots);
        const FragArgs A{I.cells.data(), I.frag_off.data(), I.cell_off.data(), I.pref_off.data(), I.n_frag.data()};
        depth_.resize((size_t)(depth_bytes_ / 16) + 1);   // (kept between requests as the device keeps its area: stale values behind it)
        uint8_t* area = reinterpret_cast<uint8_t*>(depth_.data());
        HostGroup g;
        for (size_t u = 0; u < units.size(); u++) evidence_mark_unit(g, units.data(), A, blob, (int)u, which, T, area, depth_off_.data());
        for (size_t u = 0; u < units.size(); u++)
            evidence_scan_unit(g, units.data(), prof_hb_->junc_ends.data(), blob, (int)u, which, jwin, E, area, depth_off_.data(), P.blob.data(), P.off.data());
    }
    void host_fold_profile(const uint8_t* blob, int which, ProfileState& P) {
        const std::vector<UnitIn>& units = prof_hb_->units;
        int fwin, jwin, slots;
        fold_windows(&fwin, &jwin, &slots);
        std::vector<int32_t> lds((size_t)(fold_arm_lds_bytes(fwin) / 4)), lds2((size_t)(fold_scan_lds_bytes(slots) / 4));
        const FoldList L = fold_list(lds.data(), fwin);
        const FoldTable T = fold_table(lds2.data(), slots);
        planes_.resize((size_t)(2 * plane_bytes_ / 16) + 1);   // (kept between requests as the device keeps its area: stale values behind it)
        uint8_t* area = reinterpret_cast<uint8_t*>(planes_.data());
        HostGroup g;
        for (size_t u = 0; u < units.size(); u++) fold_arms_unit(g, units.data(), blob, (int)u, which, L, area, plane_bytes_, plane_off_.data());
        for (size_t u = 0; u < units.size(); u++)
            fold_scan_unit(g, units.data(), prof_hb_->junc_ends.data(), blob, (int)u, which, jwin, T, area, plane_bytes_, plane_off_.data(), P.blob.data(), P.off.data());
    }
    void host_compare(const uint8_t* blob, ProfileState& P) {
        const PairRequest& Q = pair_of(kCompare);
        std::vector<Seq16A> image;
        const CompareGiven given = host_given(Q, image);
        std::vector<int32_t> V((size_t)(compare_lds_bytes(Q.dmax) / 4));
        HostGroup g;
        for (int i = 0; i < Q.n(); i++)
            compare_pair(g, prof_hb_->units.data(), blob, given, Q.entries.data(), i, Q.dmax, V.data(), reinterpret_cast<PathCompare*>(P.blob.data()));
    }
    void host_align(const uint8_t* blob, ProfileState& P) {
        const PairRequest& Q = pair_of(kAlign);
        std::vector<Seq16A> image;
        const CompareGiven given = host_given(Q, image);
        std::vector<int32_t> lds((size_t)(align_lds_bytes(Q.dmax) / 4)), hist((size_t)align_history_ints(Q.dmax));
        HostGroup g;
        for (int i = 0; i < Q.n(); i++)
            align_pair(g, prof_hb_->units.data(), blob, given, Q.entries.data(), i, Q.dmax, lds.data(), lds.data() + compare_lds_bytes(Q.dmax) / 4, hist.data(),
                       reinterpret_cast<PathAlign*>(P.blob.data()), reinterpret_cast<AlignRun*>(P.blob.data() + align_runs_off(Q.n())));
    }
    void host_coords(const uint8_t* blob, int which, ProfileState& P) {
        const std::vector<UnitIn>& units = prof_hb_->units;
        const LenImage& I = prof_hb_->len;
        const LenArgs A{I.len.data(), I.len_off.data()};
        cplanes_.resize((size_t)(cplane_bytes_ / 16) + 1);   // (kept between requests as the device keeps its area: stale values behind it)
        uint8_t* area = reinterpret_cast<uint8_t*>(cplanes_.data());
        HostGroup g;
        for (size_t u = 0; u < units.size(); u++) coords_unit(g, units.data(), blob, A, (int)u, which, area, cplane_off_.data(), P.blob.data());
        PathLift* out = reinterpret_cast<PathLift*>(P.blob.data() + coords_results_off((int64_t)units.size()));
        for (int64_t i = 0; i < (int64_t)lift_.size(); i++) lift_query(units.data(), blob, A, which, area, cplane_off_.data(), P.blob.data(), lift_.data(), i, out);
    }
    std::vector<Seq16A> depth_;          // the default implementation's depth area (16-byte aligned)
    std::vector<Seq16A> cplanes_;        // the default implementation's coordinate plane (16-byte aligned)
    std::vector<Seq16A> planes_;         // the default implementation's fold and cover planes (16-byte aligned)
    std::vector<Seq16A> seq_out_;        // the default implementation's output block (16-byte aligned)
};

Backend* make_backend();   // defined by the linked backend
// diagnostics: microseconds until a tiny kernel on stream b has run while a kernel with a long backlog of workgroups occupies stream a
int backend_stream_probe(void* stream_a, void* stream_b, float* us);

// ILP entries (ambi_ilp_rows.hpp) written by the linked backend: the HIP engine launches ambi_ilp_fill_kernel and copies
// col/val back, the host simulation runs the same entry function on the CPU.  kernel_ms: device time of the fill (0 on the host).
struct IlpRowDesc;
// runs -> cells in the backend's memory space (ambi_expand_runs of the C ABI)
int backend_expand_runs(const int32_t* run_start, const int32_t* run_len, const int64_t* cell_off, int64_t n_runs, int32_t* cells,
                        int64_t cell_cap, void* stream);
int backend_ilp_fill(const IlpRowDesc* rows, int64_t n_rows, const int64_t* row_ptr, int start_id, int end_id, const int32_t* lit_col,
                     const double* lit_val, int64_t n_lit, int32_t* col, double* val, float* kernel_ms);

}  // namespace ambi
