// ambi_engine.hip -- the HIP (gfx950 / MI355X) backend: kernels + stream orchestration.
//
// Kernels (all integer / index work, no MFMA; bound by HBM writes of the order table and by LDS latency / issue):
//   ambi_prepare_kernel           1 wave  / unit   junction ends staged into LDS; getJuncCN, bias, getIndelBias,
//                                                  targetCN, constructDAG; order-ideal lattice (level-synchronous
//                                                  search in LDS), completion counts, frozen automaton; R
//   ambi_plan_kernel              1 block / batch  64-bit scans: order-table offsets, enumerate work blocks
//                                                  (ambi_plan_reset_kernel in front of a second pass over the same headers)
//   ambi_blocks_build_kernel      1 block / unit   block-emission image (block directory + suffix rows) -> HBM
//   ambi_enumerate_blocks_kernel  1 block / work block: image -> LDS, rows streamed block by block with fully
//                                                  coalesced 16-byte stores                       <- HBM-bound
//   ambi_enumerate_kernel         general path (per-lane unrank + lexicographic successor) for units whose image
//                                                  does not fit the LDS budget
//   ambi_first_kernel             1 wave  / unit   getBFB scan for the first valid order, bkp in LDS
//   ambi_search/resolve_kernel    1 wave  / chunk of orders (only for units whose scan budget ran out)
//   ambi_finish_kernel            1 block / unit   bkp -> path (LDS int16), indelBFB, output junctions
//   ambi_pack_scan/copy_kernel    optional end-of-batch packing of the paths for an RCCL gather, as cells ...
//   ambi_pack_runs_count/scan/write_kernel          ... or as runs {start value, length}; ambi_expand_runs_kernel (1 wave /
//                                                  run) turns runs back into cells on the receiving rank (ambi_exchange.hpp)
//   ambi_path_profile_kernel      1 block / unit   on request: per-segment traversal counts of the path + summary
//                                                  (ambi_profile.hpp)                              <- read-bound, 2 bytes / cell
//   ambi_junc_profile_kernel      1 block / unit   on request: per-junction traversal counts of the path + summary
//                                                  (ambi_junc_profile.hpp)                         <- the same cells + a hash table in LDS
//   ambi_frag_profile_kernel      1 block / unit   on request: occurrences of every .juncs fragment in the path, both directions,
//                                                  + summary (ambi_frag_profile.hpp)               <- the same cells + chained patterns in LDS
//   ambi_evidence_mark_kernel     1 block / unit   on request: the fragment profile's match; every occurrence posts +1 / -1 into the
//                                                  unit's depth area (ambi_evidence_profile.hpp)   <- the same cells, device-memory atomics
//   ambi_evidence_scan_kernel     1 block / unit   on request, behind the mark kernel: depth per step by a scan in place, summary,
//                                                  per junction covered traversals                 <- 4 bytes / step + the cells per pass
//   ambi_fold_arm_kernel          1 block / unit   on request: the folds of the path and the palindrome arm around each, short arms per
//                                                  lane, long ones by whole wavefronts; fold plane and the spans' ends into the cover
//                                                  plane (ambi_fold_profile.hpp)                   <- the same cells, 2 atomics / fold
//   ambi_fold_scan_kernel         1 block / unit   on request, behind the arm kernel: cover per step by a scan in place, summary, per
//                                                  junction its folds and longest arm              <- 8 bytes / step
//   ambi_path_compare_kernel      1 block / pair   on request: common ends and indel distance of pairs of paths, both orientations:
//                                                  trim by whole-group sweeps, then Myers' greedy rounds up to dmax, long snakes by
//                                                  whole wavefronts (ambi_path_compare.hpp)        <- both paths twice when the trim ends it
//   ambi_path_align_kernel        1 block / pair   on request: the edit script of pairs of paths in one orientation as maximal runs:
//                                                  the comparison's trim and rounds with every round's V kept in the workgroup's
//                                                  history area, a one-thread traceback, a whole-group run merge
//                                                  (ambi_path_align.hpp)                           <- the history: D^2 / 2 ints a pair
//   ambi_path_coords_kernel       1 block / unit   on request: the base-pair offset of every cell of the path by a 64-bit scan, two cells
//                                                  and one 16-byte store per thread and round, + summary
//                                                  (ambi_path_coords.hpp)                          <- store-bound, 8 bytes / cell
//   ambi_path_lift_kernel         1 thread / query on request, behind the scan: amplicon position -> cell, segment, offset in the
//                                                  segment by a bisection over the unit's slice    <- 23 dependent loads at most
//                                                  (the profile kernels share unit prologue, chunked cell read and window rule --
//                                                  profile_path, path_load_chunk, capped_window of ambi_profile.hpp -- and the two tables
//                                                  their probe, lds_find / lds_claim of ambi_junc_profile.hpp; every reader of a unit's
//                                                  path in the result blob selects it with unit_path of ambi_batch.hpp)
// Every kernel but the two plan kernels is a wrapper around the stage functions of ambi_stages.hpp (ambi_exchange.hpp,
// ambi_profile.hpp for the pack / expand and profile kernels), which the host simulation runs as well, the four table kernels
// (blocks_build, enumerate_blocks, enumerate, enumerate_wide; their logic is under stage_enumerate's banner) included.  The
// plan kernel has a serial twin for the host simulation (plan_serial).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "ambi_backend.hpp"
#include "ambi_exchange.hpp"
#include "ambi_ilp_rows.hpp"
#include "ambi_stages.hpp"

namespace ambi {

#define HIP_CK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) {                                                                     \
            fprintf(stderr, "ambigram_hip: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return -31;                                                                             \
        }                                                                                           \
    } while (0)

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
extern __shared__ __align__(16) uint8_t ambi_lds[];

// Register budgets of the kernels that share the CUs during a step.  A SIMD holds 512 vector registers per lane and 800 scalar
// registers: five wavefronts of the order-table kernel at 96 vector registers (what the compiler takes when left alone) fill 480
// of them, and a finish wavefront (96) then only fits where an order-table workgroup has been pushed off the CU.  Asking for
// AMBI_*_WAVES wavefronts per SIMD caps the kernel's vector registers at 512 / waves (in granules of 8).
// Measured on the bench batch, builds interleaved on one box (profiles/r04_notes.md): left alone (96 / 95 / 112 registers)
// 0.865 ms per step; order table 80 alone 0.91-0.92 (six of its workgroups then fit a CU and squeeze the finish kernels out);
// order table 80 + lean finish 80 + direct full finish 96: 0.824-0.830.
#ifndef AMBI_ENUM_WAVES
#define AMBI_ENUM_WAVES 6
#endif
#ifndef AMBI_LEAN_WAVES
#define AMBI_LEAN_WAVES 6
#endif
#ifndef AMBI_EXT_WAVES
#define AMBI_EXT_WAVES 5
#endif
#ifndef AMBI_FIRST_WAVES
#define AMBI_FIRST_WAVES 0
#endif
#ifndef AMBI_PREP_WAVES
#define AMBI_PREP_WAVES 0
#endif
#define AMBI_WAVES_ATTR_(n) __attribute__((amdgpu_waves_per_eu(n)))
#define AMBI_WAVES_ATTR(n) AMBI_WAVES_ATTR_(n)
#if AMBI_ENUM_WAVES > 0
#define AMBI_ENUM_ATTR AMBI_WAVES_ATTR(AMBI_ENUM_WAVES)
#else
#define AMBI_ENUM_ATTR
#endif
#if AMBI_LEAN_WAVES > 0
#define AMBI_LEAN_ATTR AMBI_WAVES_ATTR(AMBI_LEAN_WAVES)
#else
#define AMBI_LEAN_ATTR
#endif
#ifndef AMBI_EDIT_WAVES
#define AMBI_EDIT_WAVES 6
#endif
#if AMBI_EDIT_WAVES > 0
#define AMBI_EDIT_ATTR AMBI_WAVES_ATTR(AMBI_EDIT_WAVES)
#else
#define AMBI_EDIT_ATTR
#endif
#if AMBI_EXT_WAVES > 0
#define AMBI_EXT_ATTR AMBI_WAVES_ATTR(AMBI_EXT_WAVES)
#else
#define AMBI_EXT_ATTR
#endif
#if AMBI_FIRST_WAVES > 0
#define AMBI_FIRST_ATTR AMBI_WAVES_ATTR(AMBI_FIRST_WAVES)
#else
#define AMBI_FIRST_ATTR
#endif
#if AMBI_PREP_WAVES > 0
#define AMBI_PREP_ATTR AMBI_WAVES_ATTR(AMBI_PREP_WAVES)
#else
#define AMBI_PREP_ATTR
#endif

constexpr uint32_t kGuardWord = 0xA5B1C3D7u;
// results of one unit as the express kernel mirrors them into the pinned mailbox (MailLayout); whole workgroup
__device__ inline void mail_unit(const BatchArgs& A, int u, bool path_there = false) {   // path_there: the finish stage wrote the path into the slot already
    const UnitIn& U = A.units[u];
    const UnitOut* h = unit_out(A.results, u);
    const UnitLayout L = unit_layout(U.n_seg, U.bkp_cap, U.path_cap, U.out_cap);
    const MailLayout M = mail_layout(U.path_cap, U.out_cap);
    uint8_t* slot = A.mail + A.mail_off[u];
    const uint8_t* res = A.results + U.res_off;
    auto copy8 = [&](uint8_t* dst, const uint8_t* src, int64_t bytes) {   // (every part is padded to 8 bytes on both sides)
        for (int64_t i = threadIdx.x; i < (bytes + 7) / 8; i += blockDim.x) reinterpret_cast<uint64_t*>(dst)[i] = reinterpret_cast<const uint64_t*>(src)[i];
    };
    copy8(slot, reinterpret_cast<const uint8_t*>(h), (int64_t)sizeof(UnitOut));
    if (!path_there) copy8(slot + M.path, res + L.path, (int64_t)sizeof(rcell_t) * h->path_len);
    if (h->path_ind_stored) copy8(slot + M.path_ind, res + L.path_ind, (int64_t)sizeof(rcell_t) * h->path_indel_len);
    copy8(slot + M.out_junc, res + L.out_junc, (int64_t)sizeof(OutJunc) * h->n_out_junc);
    __threadfence_system();
}
// A small batch's input image goes from pinned host memory to HBM and its zero-filled region is cleared by ONE kernel (the
// threads read host memory over the link): a copy command + a fill command cost two engine hand-overs in front of the
// first kernel, several times what moving 15 KB takes.
__global__ __launch_bounds__(256) void ambi_ingest_kernel(const uint4* src, uint4* dst, int64_t n16, uint4* zero, int64_t z16) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = i; k < n16; k += stride) dst[k] = src[k];
    const uint4 z = {0u, 0u, 0u, 0u};
    for (int64_t k = i; k < z16; k += stride) zero[k] = z;
}
// guard words on both sides of every path area of the direct full-finish launch (AMBI_DEBUG: does that kernel leave its slot?)
constexpr int kCellGuardBytes = 64;
__global__ void ambi_guard_fill_kernel(uint8_t* cells, int64_t stride, int slots) {
    const int s = blockIdx.x, t = threadIdx.x;   // 32 threads: 16 words in front of the area, 16 behind
    if (s >= slots) return;
    uint32_t* w = reinterpret_cast<uint32_t*>(cells + (int64_t)s * stride + (t < 16 ? 0 : stride - kCellGuardBytes));
    w[t & 15] = kGuardWord;
}
__global__ void ambi_guard_check_kernel(const uint8_t* cells, int64_t stride, int slots, int32_t* bad) {
    const int s = blockIdx.x, t = threadIdx.x;
    if (s >= slots) return;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(cells + (int64_t)s * stride + (t < 16 ? 0 : stride - kCellGuardBytes));
    if (w[t & 15] != kGuardWord) atomicAdd(bad, 1);
}


__global__ __launch_bounds__(64) AMBI_PREP_ATTR void ambi_prepare_kernel(BatchArgs A) {
    WaveGroup g;
    if (A.zero_pending && blockIdx.x == 0 && threadIdx.x == 0) { *A.n_pending = 0; A.refin_count[0] = 0; A.refin_count[1] = 0; }   // nothing counts pending / handed-over units before the scan
    stage_prepare(g, A, A.unit_base + (int)blockIdx.x, ambi_lds);
}

// Small batches: the whole reconstruction of a unit whose first order assembles, one workgroup per unit (ambi_stages.hpp:
// stage_express) -- junction side and DAG side on two wavefronts at once, then imperfectFBI, then the finish stage on the
// workgroup.  The lattice / order table follow in the kernels behind (ambi_lattice_kernel, plan, enumerate).
__global__ __launch_bounds__(1024) void ambi_express_kernel(BatchArgs A) {
    __shared__ int scratch[40];
    BlockGroup gb(scratch);
    WaveGroup gw;
    if (A.zero_pending && blockIdx.x == 0 && threadIdx.x == 0) *A.n_pending = 0;
    const int wave = threadIdx.x >> 6, u = A.unit_base + (int)blockIdx.x;
    const bool path_there = stage_express(gw, gb, wave < 2 ? wave : 2, A, u, ambi_lds);
    __syncthreads();
    if (A.mail && unit_out(A.results, u)->reserved) { mail_unit(A, u, path_there); __syncthreads(); }   // header, final path(s), output junctions -> pinned host memory
    AMBI_MARK(A, gb, u, 25);
    if (threadIdx.x == 0 && A.express_left) {
        if (!unit_out(A.results, u)->reserved) *A.express_left = 1;
        __threadfence_system();
        if (atomicAdd(A.blocks_done, 1) == (int)gridDim.x - 1) {   // last workgroup: tell the host (it spins on this word)
            *A.blocks_done = 0;
            __threadfence_system();
            *(volatile int32_t*)A.express_seq = A.run_seq;
        }
    }
}
__global__ __launch_bounds__(64) void ambi_lattice_kernel(BatchArgs A) {
    WaveGroup g;
    if (A.zero_pending && blockIdx.x == 0 && threadIdx.x == 0) { A.refin_count[0] = 0; A.refin_count[1] = 0; }   // the lean finish kernel behind fills the list ([1]: the edit kernel's hand-over list)
    stage_lattice(g, A, A.unit_base + (int)blockIdx.x, ambi_lds);
}

__global__ __launch_bounds__(64) void ambi_lattice_own_kernel(BatchArgs A) {
    WaveGroup g;
    if (A.zero_pending && blockIdx.x == 0 && threadIdx.x == 0) { A.refin_count[0] = 0; A.refin_count[1] = 0; }   // (as ambi_lattice_kernel)
    const int u = A.unit_base + (int)blockIdx.x;
    stage_lattice_own(g, A, u, ambi_lds);
    // the verdict the host waits for on a fresh batch: no lattice failed and the tables of ALL units fit the arena together
    // (then every prefix fits, whatever subset the plan kernel ends up placing)
    if (threadIdx.x == 0 && A.lat_seq) {
        const bool ok = A.lat_status[u] == ST_OK || A.lat_status[u] == ST_ERR_NO_ELEMENTS;   // (no elements: the express stage reports that itself)
        const bool toobig = A.lat_status[u] == ST_OK && order_table_too_big((int64_t)A.lat_R[u], A.units[u].n_elem);   // (the plan kernel will refuse it)
        const int64_t bytes = A.lat_status[u] == ST_OK && !toobig ? order_bytes((int64_t)A.lat_R[u], A.units[u].n_elem, A.order_align) : 0;
        if (!ok || toobig) *A.lat_unsure = 1;
        __threadfence_system();
        const unsigned long long total = atomicAdd(reinterpret_cast<unsigned long long*>(A.lat_sum), (unsigned long long)bytes) + (unsigned long long)bytes;
        (void)total;
        __threadfence();
        if (atomicAdd(reinterpret_cast<unsigned long long*>(A.lat_sum + 1), 1ull) == (unsigned long long)gridDim.x - 1) {   // last wave
            const int64_t all = (int64_t)atomicAdd(reinterpret_cast<unsigned long long*>(A.lat_sum), 0ull);
            if (all > A.order_arena_bytes) *A.lat_unsure = 1;
            A.lat_sum[0] = 0; A.lat_sum[1] = 0;
            __threadfence_system();
            *(volatile int32_t*)A.lat_seq = A.run_seq;
        }
    }
}

// before the plan kernel is run a SECOND time over the same headers (tables written on demand, or after the arena grew): every
// unit that has or was refused rows wants rows again
__global__ void ambi_plan_reset_kernel(BatchArgs A) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= A.n_units) return;
    UnitOut* out = unit_out(A.results, A.unit_base + i);
    if (out->order_off >= 0 || out->order_off == kOrderOffNoRoom) out->order_off = kOrderOffWanted;
}

// Parallel form of plan_serial (ambi_stages.hpp): same prefix-sum semantics; its body stays here (profiles/r11_notes.md: in the shared
// form the kernel was 0.5 us slower).
__global__ __launch_bounds__(1024) void ambi_plan_kernel(BatchArgs A) {
    __shared__ __align__(16) int scratch[40];   // (exscan_i64 needs 8; 16 lets it read the wave totals as 16-byte words)
    BlockGroup g(scratch);
    if (A.lat_R) {   // the lattice ran beside the express kernel: its outcome goes into the headers first
        for (int i = threadIdx.x; i < A.n_units; i += blockDim.x) plan_merge_lattice(A, A.unit_base + i);
        __threadfence();
        __syncthreads();
    }
    // Every thread takes kPlanPer CONSECUTIVE units of a chunk of kPlanPer * blockDim.x: their headers are read together (one round
    // trip to memory per chunk and pass instead of one per unit), the prefix sums inside a thread are serial, and a chunk costs two
    // block scans (offsets; work blocks, which depend on what fits) -- round 3's form read and scanned blockDim.x units at a time: nine
    // scans and five dependent round trips for the bench batch's 4096 units, 27 us with the chip otherwise idle.
    constexpr int kPlanPer = 4;
    const int chunk = kPlanPer * (int)blockDim.x;
    const bool one_chunk = A.n_units <= chunk;
    int64_t R_[kPlanPer]; int K_[kPlanPer]; bool wanted_[kPlanPer];
    auto load_chunk = [&](int base) {
#pragma unroll
        for (int k = 0; k < kPlanPer; k++) {
            const int i = base + (int)threadIdx.x * kPlanPer + k;
            R_[k] = 0; K_[k] = 0; wanted_[k] = false;
            if (i < A.n_units) {
                const UnitOut* o = unit_out(A.results, A.unit_base + i);
                wanted_[k] = o->order_off == kOrderOffWanted;   // (not the status: the scan for the first valid order may be rewriting it)
                R_[k] = o->num_orders; K_[k] = o->K;
            }
        }
    };
    // pass 1: rows of the whole batch -> rows per lane of the enumerate kernel
    int64_t my_rows = 0;
    for (int base = 0; base < A.n_units; base += chunk) {
        load_chunk(base);
#pragma unroll
        for (int k = 0; k < kPlanPer; k++) if (wanted_[k] && !order_table_too_big(R_[k], K_[k])) my_rows += R_[k];
    }
    int64_t total_rows;
    (void)g.exscan_i64(my_rows, &total_rows);
    const int TL = rows_per_lane_for(total_rows, A.target_lanes);
    int64_t off_carry = 0, blk_carry = 0;
    for (int base = 0; base < A.n_units; base += chunk) {
        if (!one_chunk) load_chunk(base);
        const int T = TL;
        int64_t bytes[kPlanPer], blocks[kPlanPer], sum_b = 0;
        bool live[kPlanPer], toobig[kPlanPer];
#pragma unroll
        for (int k = 0; k < kPlanPer; k++) {
            bytes[k] = 0; blocks[k] = 0; live[k] = false; toobig[k] = false;
            if (wanted_[k]) {
                if (order_table_too_big(R_[k], K_[k])) toobig[k] = true;   // (the rule and its bound: ambi_stages.hpp, next to order_bytes)
                else {
                    live[k] = true;
                    bytes[k] = order_bytes(R_[k], K_[k], A.order_align);
                    blocks[k] = (R_[k] + 256ll * T - 1) / (256ll * T);   // one work block = one workgroup = 4 waves x 64*T rows
                }
            }
            sum_b += bytes[k];
        }
        int64_t tot_b, tot_k;
        int64_t off = off_carry + g.exscan_i64(sum_b, &tot_b);
        // a unit that does not fit contributes no work blocks (and still advances the offset: orders_needed is the true total)
        bool fits[kPlanPer];
        int64_t offs_[kPlanPer], sum_k = 0;
#pragma unroll
        for (int k = 0; k < kPlanPer; k++) {
            offs_[k] = off;
            fits[k] = live[k] && (off + bytes[k] <= A.order_arena_bytes);
            off += bytes[k];
            sum_k += fits[k] ? blocks[k] : 0;
        }
        int64_t blk = blk_carry + g.exscan_i64(sum_k, &tot_k);
#pragma unroll
        for (int k = 0; k < kPlanPer; k++) {
            const int i = base + (int)threadIdx.x * kPlanPer + k;
            if (i < A.n_units) {
                const int u = A.unit_base + i;
                UnitOut* out = unit_out(A.results, u);
                A.blk_off[i] = blk;
                A.rows_per_lane[u] = T;
                if (toobig[k]) out->order_off = kOrderOffNoRoom;
                else if (live[k]) out->order_off = fits[k] ? A.arena_base + offs_[k] : kOrderOffNoRoom;   // (no room: the finish stage turns the status into ORDERS_CAPACITY)
                if ((toobig[k] || (live[k] && !fits[k])) && A.late_flag) { *A.late_flag = 1; __threadfence_system(); }   // a result the express stage published is void
            }
            blk += fits[k] ? blocks[k] : 0;
        }
        off_carry = order_bytes_add(off_carry, tot_b);
        blk_carry += tot_k;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        A.blk_off[A.n_units] = blk_carry;
        *A.orders_needed = off_carry;
        if (A.host_needed) *A.host_needed = off_carry;
        if (A.plan_seq) { __threadfence_system(); *(volatile int32_t*)A.plan_seq = A.run_seq; }   // orders_needed and late_flag of this run are final
    }
}

// The four table kernels: group set-up, the grid-stride loop over the work blocks and the filters in front; what a workgroup or
// wave does with a work block is in ambi_stages.hpp (stage_enumerate), which the host simulation runs as well.
// General path (enumerate_general_block): one wavefront per 64*T consecutive ranks of one unit, rows leave the registers as 16-byte stores.
// LDS per wave: [enum_stack_lds] per-lane DFS stacks | [enum_auto_lds] compact copy of the unit's automaton when it fits.
template <int CLS>
__global__ __launch_bounds__(256) void ambi_enumerate_kernel(BatchArgs A) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint8_t* stacks = ambi_lds + (size_t)wave * (A.enum_stack_lds + A.enum_auto_lds);
    WaveGroup g;
    const int64_t total = A.blk_off[A.n_units];
    StagedAuto S;
    // only units whose block tables did not fit (flagged by ambi_blocks_build_kernel / ambi_enumerate_blocks_kernel)
    for (int64_t b = (int64_t)blockIdx.x; b < total; b += (int64_t)gridDim.x) {
        const int lo = unit_of_work_block(A, b), u = A.unit_base + lo;
        if (enum_class_of(unit_out(A.results, u)->K) != CLS) continue;   // rows of this width belong to another instantiation
        if (!A.unit_fallback[u]) continue;
        enumerate_general_block<CLS>(g, A, u, b - A.blk_off[lo], S, stacks, stacks + A.enum_stack_lds, wave, lane);
    }
}

// Builds the block-emission image (build_unit_image) of every unit whose table is written by MORE THAN ONE workgroup and parks
// it in HBM (a unit with a single work block gets its image built in LDS by the enumerate workgroup itself, stage_unit_image).
__global__ __launch_bounds__(256) void ambi_blocks_build_kernel(BatchArgs A) {
    __shared__ int scratch[40];
    BlockGroup g(scratch);
    const int u = A.unit_base + (int)blockIdx.x;
    const UnitOut* out = unit_out(A.results, u);
    const int64_t nblocks = A.blk_off[blockIdx.x + 1] - A.blk_off[blockIdx.x];
    // (order_off, not status: the scan for the first valid order runs beside this kernel and rewrites the status; the
    // plan kernel gave order_off >= 0 to exactly the units that have rows to write)
    if (out->order_off < 0 || nblocks <= 0 || (nblocks == 1 && A.build_in_emit)) {   // no rows to write / image built by the enumerate kernel
        if (threadIdx.x == 0) A.unit_fallback[u] = 0;
        return;
    }
    const IdealTable tbl = unit_ideal_table(A, u);
    BlockImageHeader H;
    // the build tables sit in LDS, the image is assembled word by word straight in its HBM slot; a directory-free image leaves
    // room in front for the tables, which the walk reads and which therefore travel with the suffix rows
    uint8_t* slot = A.block_img + (int64_t)u * A.block_lds;
    BuildTables dummy;
    const int64_t scr = carve_build_tables(ambi_lds, tbl.counter[0], tbl.counter[1], dummy);
    const int kind = build_unit_image(g, tbl, out->K, out->num_orders, A.block_max, A.block_dfs, ambi_lds, A.block_scratch_lds, slot, A.block_lds,
                                      scr, (int64_t)A.block_lds - kDfsStateBytes - scr, H, A.stage_clk ? A.stage_clk + (int64_t)u * kStageSlots : nullptr);
    if (kind == 2) {
        copy_words(g, reinterpret_cast<uint32_t*>(slot), reinterpret_cast<const uint32_t*>(ambi_lds), scr / 4);
        H.pad = (int32_t)scr;
        H.image_bytes += (int32_t)scr;
    }
    if (threadIdx.x == 0) {
        *reinterpret_cast<BlockImageHeader*>(A.block_hdr + 8 * (int64_t)u) = H;
        A.unit_fallback[u] = kind ? 0 : 1;
    }
}

// Fast path: block emission (ambi_enum_blocks.hpp).  One workgroup per work block of 256*T rows; the workgroup brings the
// unit's image (block directory + suffix rows) into LDS (stage_unit_image), then every wave streams its share of the rows
// block by block (emit_work_block): four LDS reads, four ORs and one fully coalesced 16-byte store per lane and step.
// A unit with ONE work block has no image in HBM: its workgroup builds the image right here in LDS (automaton copy in
// front, image behind it) -- the build is a latency-bound chain that hides under the store stream of the other
// workgroups of the CU -- and the separate build kernel only serves the units that several workgroups share.
// LDS: [block_lds] image (+ automaton copy while building); the directory-free walk's state (per wave) in its last kDfsStateBytes.
template <int CLS>
__global__ __launch_bounds__(1024) AMBI_ENUM_ATTR void ambi_enumerate_blocks_kernel(BatchArgs A) {
    __shared__ int scratch[40];
    BlockGroup g(scratch);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint8_t* tmem = ambi_lds;
    const int64_t total = A.blk_off[A.n_units];
    int staged_unit = -1;
    StagedUnit S;
    uint8_t* wave_state = tmem + A.block_lds - kDfsStateBytes + wave * kDfsWaveStride;
    for (int64_t b = (int64_t)blockIdx.x; b < total; b += (int64_t)gridDim.x) {
        const int lo = unit_of_work_block(A, b), u = A.unit_base + lo;
        const UnitOut* out = unit_out(A.results, u);
        const int K = out->K, T = A.rows_per_lane[u];
        if (enum_class_of(K) != CLS) continue;
        if (A.first_rows && out->num_orders <= A.first_budget) {   // the table is among the rows unranked for the scan
            copy_first_rows(g, A.first_rows + (int64_t)u * A.first_budget * kFirstRowStride, K, out->num_orders, A.order_arena + out->order_off);
            continue;
        }
        if (u != staged_unit) { stage_unit_image(g, A, lo, tmem, S); staged_unit = u; }
        if (!S.fits) continue;
        emit_work_block<CLS>(S, K, out->num_orders, T, b - A.blk_off[lo], A.order_arena + out->order_off, A.emit_interleave, wave,
                             (int)(blockDim.x >> 6), lane, lane + 1, wave_state);
    }
}

// Order tables of the wide units (64..127 nodes, row class 3): 64 workgroups per wide unit, one thread per row (write_wide_row).
// Rare units, at most kWideMaxOrders rows each: written for correctness, not for the roofline.
__global__ __launch_bounds__(256) void ambi_enumerate_wide_kernel(BatchArgs A, const int32_t* wide_units, int n_wide) {
    const int w = blockIdx.y;
    if (w >= n_wide) return;
    const int u = wide_units[w];
    if (u < A.unit_base || u >= A.unit_base + A.n_units) return;   // not a unit of this launch
    const UnitOut* out = unit_out(A.results, u);
    if (out->order_off < 0 || out->num_orders <= 0) return;
    const WideUnit& X = A.wide[A.wide_index[u]];
    uint8_t* rows = A.order_arena + out->order_off;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < out->num_orders; r += (int64_t)gridDim.x * blockDim.x)
        write_wide_row(X, r, out->K, rows);
}

__global__ __launch_bounds__(64) AMBI_FIRST_ATTR void ambi_first_kernel(BatchArgs A) {
    WaveGroup g;
    stage_first(g, A, A.unit_base + (int)blockIdx.x, ambi_lds);
}

// Slow path: units whose first-valid scan ran out of budget.  One wave per chunk of `chunk` consecutive orders
// (ambi_stages.hpp: search_item / stage_resolve).
__global__ __launch_bounds__(256) void ambi_search_kernel(BatchArgs A, SearchArgs S) {
    const int wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    uint8_t* work = ambi_lds + (size_t)wave * S.wave_lds;
    WaveGroup g;
    const int64_t total = S.chunk_off[S.np];
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < total; c += (int64_t)gridDim.x * wpb) search_item(g, A, S, c, work);
}
__global__ void ambi_search_init_kernel(SearchSlot* slots, int np) {
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p < np) { slots[p].found = kSearchNone; slots[p].err_key = kSearchNone; }
}
// after a search pass: re-evaluate the winning order to materialise its bkp and fill the header
__global__ __launch_bounds__(64) void ambi_resolve_kernel(BatchArgs A, SearchArgs S, int pass) {
    WaveGroup g;
    const int p = blockIdx.x;
    stage_resolve(g, A, S.pending[p], ambi_lds, &S.slots[p], S.forward != 0, pass);
}

// --all (LGM.cpp:3672-3695), fused enumerate + evaluate (ambi_stages.hpp: all_lanes_item / all_wave_item): one wave per 64
// consecutive orders of a unit, all units of the batch in ONE launch per pass.  One thread per order for units whose breakpoint
// path has at most lane_cap cells -- the rule on real inputs (a path of ~100 cells at 256 segments); ambi_all_kernel keeps the
// longer ones.  LDS per wave: AllLaneGeom::wave_lds here, first-work area + 64 unranked rows in ambi_all_kernel.
__global__ __launch_bounds__(256) void ambi_all_lanes_kernel(BatchArgs A, AllLaneGeom geom, int pass, int64_t total_chunks, int lane_cap) {
    const int wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    uint8_t* work = ambi_lds + (size_t)wave * geom.wave_lds;
    WaveGroup g;
    AllLaneState state;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < total_chunks; c += (int64_t)gridDim.x * wpb) all_lanes_item(g, A, geom, c, pass, work, lane_cap, state);
}
__global__ __launch_bounds__(256) void ambi_all_kernel(BatchArgs A, int pass, int wave_lds, int64_t total_chunks, int lane_cap) {
    const int wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    uint8_t* work = ambi_lds + (size_t)wave * wave_lds;
    WaveGroup g;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < total_chunks; c += (int64_t)gridDim.x * wpb) all_wave_item(g, A, c, pass, work, lane_cap);
}
__global__ __launch_bounds__(256) void ambi_all_finalize_kernel(BatchArgs A) {
    const int u = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (u < A.n_units) all_finalize_unit(A, u);
}
// Paths of a list of orders of one unit (the valid ones, in print order): one wave per order, breakpoints in LDS
// (ambi_stages.hpp: order_path_item).
__global__ __launch_bounds__(64) void ambi_order_paths_kernel(BatchArgs A, int u, int forward, const int64_t* order_idx, int32_t* lengths,
                                                              int32_t* cells, int64_t stride) {
    WaveGroup g;
    order_path_item(g, A, u, forward != 0, order_idx, (int64_t)blockIdx.x, gridDim.x == 1, lengths, cells, stride, ambi_lds);
}

// Full finish stage.  unit_list == nullptr: every unit of the batch (one workgroup each).  With a list: the listed units;
// list_count == nullptr: one workgroup per entry (host-built list of the slow path), else the list is the one the lean
// kernel in front of this launch filled on the device (refin_list / refin_count) and the workgroups share it in strides
// -- no host round trip between the two kernels.
__global__ __launch_bounds__(1024) void ambi_finish_kernel(BatchArgs A, const int32_t* unit_list, const int32_t* list_count, int fixed_count = -1) {
    __shared__ int scratch[40];
    BlockGroup g(scratch);
    if (unit_list && (list_count || fixed_count >= 0)) {
        const int n = list_count ? *list_count : fixed_count;
        for (int i = (int)blockIdx.x; i < n; i += (int)gridDim.x) {
            if (!plan_refused(g, unit_out(A.results, unit_list[i])) && !unit_out(A.results, unit_list[i])->reserved) stage_finish(g, A, unit_list[i], ambi_lds);   // (reserved: done by the express kernel; refusal first, as in the lean stage)
            __syncthreads();
        }
        return;
    }
    const int u = unit_list ? unit_list[blockIdx.x] : A.unit_base + (int)blockIdx.x;
    // the scan kernel is complete (stream order): its count of units left for the parallel search goes to the host
    if (A.host_pending && !unit_list && blockIdx.x == 0 && threadIdx.x == 0) *A.host_pending = *A.n_pending;
    stage_finish(g, A, u, ambi_lds);
}
// The direct full-stage launch with the path cells in device memory (stage_finish<true>): a workgroup works in its own
// slot of `cells` (stride bytes apart; gridDim.x slots) for every unit it takes.
__global__ __launch_bounds__(1024) AMBI_EXT_ATTR void ambi_finish_ext_kernel(BatchArgs A, const int32_t* unit_list, int count, uint8_t* cells, int64_t stride,
                                                                             const int32_t* count_ptr = nullptr) {
    __shared__ int scratch[40];
    BlockGroup g(scratch);
    if (count_ptr) count = *count_ptr;   // a list the kernel in front of this one filled on the device (ambi_finish_edit_kernel)
    for (int i = (int)blockIdx.x; i < count; i += (int)gridDim.x) {
        if (!plan_refused(g, unit_out(A.results, unit_list[i])) && !unit_out(A.results, unit_list[i])->reserved)
            stage_finish<true>(g, A, unit_list[i], ambi_lds, reinterpret_cast<cell_t*>(cells + (int64_t)blockIdx.x * stride + kCellGuardBytes));
        __syncthreads();
    }
}

// The direct launch for units whose SVs may edit the path, on the runs of the path (stage_finish_edit); what it hands on goes
// to `hand_list` for an ambi_finish_ext_kernel launch behind it.
__global__ __launch_bounds__(256) AMBI_EDIT_ATTR void ambi_finish_edit_kernel(BatchArgs A, const int32_t* unit_list, int count, int32_t* hand_list, int32_t* hand_count) {
    __shared__ int scratch[40];
    BlockGroup g(scratch);
    for (int i = (int)blockIdx.x; i < count; i += (int)gridDim.x) {
        stage_finish_edit(g, A, unit_list[i], ambi_lds, hand_list, hand_count);
        __syncthreads();
    }
}

// Lean finish (ambi_stages.hpp: stage_finish_lean): every unit of the batch; units it cannot take are counted in
// n_pending with status ST_REFINISH.  The last workgroup to finish reports n_pending to the host.
__global__ __launch_bounds__(256) AMBI_LEAN_ATTR void ambi_finish_lean_kernel(BatchArgs A, const int32_t* unit_list = nullptr, int list_count = 0) {
    __shared__ int scratch[40];
    BlockGroup g(scratch);
    if (unit_list) {   // the listed units only (the units the parallel search has just resolved)
        for (int i = (int)blockIdx.x; i < list_count; i += (int)gridDim.x) {
            stage_finish_lean(g, A, unit_list[i], ambi_lds);
            __syncthreads();
        }
        return;
    }
    // a workgroup takes every gridDim.x-th unit: the grid is sized to the number of workgroups that should be resident
    // at a time (one per CU fits beside the enumerate workgroups), not to the batch
    for (int i = (int)blockIdx.x; i < A.n_units; i += (int)gridDim.x) {
        stage_finish_lean(g, A, A.unit_base + i, ambi_lds);
        __syncthreads();
    }
    if (A.host_pending) {
        __syncthreads();
        if (threadIdx.x == 0) {
            __threadfence();
            if (atomicAdd(A.blocks_done, 1) == (int)gridDim.x - 1) {
                *A.host_pending = atomicAdd(A.n_pending, 0);
                *A.blocks_done = 0;
            }
        }
    }
}

// ---- the final paths packed for the end-of-batch exchange (ambi_exchange.hpp): cells, or runs {start value, length} ----
// Cells: one scan of the lengths, then one workgroup per unit copies.  Runs: one workgroup per unit counts, one scan, one
// workgroup per unit writes.
__global__ __launch_bounds__(1024) void ambi_pack_scan_kernel(BatchArgs A, int which, int32_t* lengths, int64_t* pack_off, int64_t* total) {
    __shared__ __align__(16) int scratch[40];   // (exscan_i64 needs 8; 16 lets it read the wave totals as 16-byte words)
    BlockGroup g(scratch);
    pack_scan(g, A, which, lengths, pack_off, total);
}
__global__ __launch_bounds__(256) void ambi_pack_copy_kernel(BatchArgs A, int which, const int64_t* pack_off, int32_t* cells, int64_t cap) {
    BlockGroup g(nullptr);   // (strided copy: no exchange between the threads)
    pack_copy_unit(g, A, (int)blockIdx.x, which, pack_off, cells, cap);
}
__global__ __launch_bounds__(256) void ambi_pack_runs_count_kernel(BatchArgs A, int which, int32_t* lengths, int32_t* run_counts) {
    __shared__ int scratch[40];
    BlockGroup g(scratch);
    pack_runs_count_unit(g, A, (int)blockIdx.x, which, lengths, run_counts);
}
__global__ __launch_bounds__(1024) void ambi_pack_runs_scan_kernel(BatchArgs A, const int32_t* lengths, const int32_t* run_counts, int64_t* run_off,
                                                                   int64_t* totals) {
    __shared__ __align__(16) int scratch[40];   // (exscan_i64 needs 8; 16 lets it read the wave totals as 16-byte words)
    BlockGroup g(scratch);
    pack_runs_scan(g, A, lengths, run_counts, run_off, totals);
}
__global__ __launch_bounds__(256) void ambi_pack_runs_write_kernel(BatchArgs A, int which, const int64_t* run_off, int32_t* run_start,
                                                                   int32_t* run_len, int64_t cap) {
    __shared__ int scratch[40];
    BlockGroup g(scratch);
    pack_runs_write_unit(g, A, (int)blockIdx.x, which, run_off, run_start, run_len, cap);
}
// ---- copy-number profile of the paths (ambi_profile.hpp; launched by HipBackend::profile_queue only) ----
// One workgroup of 256 threads per unit, grid-stride over the units.  Group memory: 256 bytes for the group's reductions, then
// the two difference arrays of `window` segments.
constexpr int kProfileThreads = 256, kProfileScratchBytes = 256;
__global__ __launch_bounds__(kProfileThreads) void ambi_path_profile_kernel(BatchArgs A, int which, int window, uint8_t* block, const int64_t* off) {
    BlockGroup g(reinterpret_cast<int*>(ambi_lds));
    int32_t* bins = reinterpret_cast<int32_t*>(ambi_lds + kProfileScratchBytes);
    for (int u = (int)blockIdx.x; u < A.n_units; u += (int)gridDim.x) {
        profile_unit(g, A.units, A.results, u, which, window, bins, block, off);
        __syncthreads();
    }
}
// ---- junction usage profile of the paths (ambi_junc_profile.hpp; launched by HipBackend::profile_queue only) ----
// One workgroup of 256 threads per unit, grid-stride over the units.  Group memory: 256 bytes for the group's reductions, then
// the hash table of `slots` slots (key, lowest index, count: 12 bytes each) and the difference array of `swin` segments.
__global__ __launch_bounds__(kProfileThreads) void ambi_junc_profile_kernel(BatchArgs A, int which, int jwin, int slots, int swin, uint8_t* block, const int64_t* off) {
    BlockGroup g(reinterpret_cast<int*>(ambi_lds));
    const JuncTable T = junc_table(ambi_lds + kProfileScratchBytes, slots, swin);
    for (int u = (int)blockIdx.x; u < A.n_units; u += (int)gridDim.x) {
        junc_profile_unit(g, A.units, A.junc_ends, A.junc_cn, A.results, u, which, jwin, T, block, off);
        __syncthreads();
    }
}
// ---- fragment support profile of the paths (ambi_frag_profile.hpp; launched by HipBackend::profile_queue only) ----
// One workgroup of 256 threads per unit, grid-stride over the units.  Group memory: 256 bytes for the group's reductions, then
// the hash table of `slots` first steps (key, chain head: 8 bytes each) and the window's `pwin` patterns (next, count, first: 12 bytes).
__global__ __launch_bounds__(kProfileThreads) void ambi_frag_profile_kernel(BatchArgs A, FragArgs I, int which, int pwin, int slots, uint8_t* block, const int64_t* off) {
    BlockGroup g(reinterpret_cast<int*>(ambi_lds));
    const FragTable T = frag_table(ambi_lds + kProfileScratchBytes, slots, pwin);
    for (int u = (int)blockIdx.x; u < A.n_units; u += (int)gridDim.x) {
        frag_profile_unit(g, A.units, I, A.results, u, which, T, block, off);
        __syncthreads();
    }
}
// ---- evidence depth profile of the paths (ambi_evidence_profile.hpp; launched by HipBackend::profile_queue only) ----
// Two launches, one workgroup of 256 threads per unit each, grid-stride over the units.  The mark kernel posts the occurrences into
// the depth area with device-memory atomics; the scan kernel reads the area with plain loads, and the kernel boundary between the
// two is what makes the atomics' results visible to them (the phases are NOT fused: a CU's vector L1 is not refreshed by atomics
// that went to L2).  Group memory: 256 bytes for the group's reductions, then the fragment profile's table (mark) or the junction
// table of `slots` slots (key, lowest index, steps, covered steps, minimum depth: 20 bytes each) and 24 bytes per thread (scan).
__global__ __launch_bounds__(kProfileThreads) void ambi_evidence_mark_kernel(BatchArgs A, FragArgs I, int which, int pwin, int slots, uint8_t* depth, const int64_t* depth_off) {
    BlockGroup g(reinterpret_cast<int*>(ambi_lds));
    const FragTable T = frag_table(ambi_lds + kProfileScratchBytes, slots, pwin);
    for (int u = (int)blockIdx.x; u < A.n_units; u += (int)gridDim.x) {
        evidence_mark_unit(g, A.units, I, A.results, u, which, T, depth, depth_off);
        __syncthreads();
    }
}
__global__ __launch_bounds__(kProfileThreads) void ambi_evidence_scan_kernel(BatchArgs A, int which, int jwin, int slots, uint8_t* depth, const int64_t* depth_off, uint8_t* block, const int64_t* off) {
    BlockGroup g(reinterpret_cast<int*>(ambi_lds));
    const EvidenceTable T = evidence_table(ambi_lds + kProfileScratchBytes, slots);
    for (int u = (int)blockIdx.x; u < A.n_units; u += (int)gridDim.x) {
        evidence_scan_unit(g, A.units, A.junc_ends, A.results, u, which, jwin, T, depth, depth_off, block, off);
        __syncthreads();
    }
}
// ---- fold-back arm profile of the paths (ambi_fold_profile.hpp; launched by HipBackend::profile_queue only) ----
// Two launches as for the evidence kind and for its reason: the arm kernel posts the spans' ends into the cover plane with
// device-memory atomics, the scan kernel reads the plane with plain loads behind the kernel boundary.  Group memory: 256 bytes for
// the group's reductions, then the list of `fwin` folds (step, packed value: 8 bytes each) in the arm kernel or the junction table of
// `slots` slots (key, lowest index, folds, longest arm: 16 bytes each) in the scan kernel.
__global__ __launch_bounds__(kProfileThreads) void ambi_fold_arm_kernel(BatchArgs A, int which, int fwin, uint8_t* planes, int64_t plane_bytes, const int64_t* plane_off) {
    BlockGroup g(reinterpret_cast<int*>(ambi_lds));
    const FoldList L = fold_list(ambi_lds + kProfileScratchBytes, fwin);
    for (int u = (int)blockIdx.x; u < A.n_units; u += (int)gridDim.x) {
        fold_arms_unit(g, A.units, A.results, u, which, L, planes, plane_bytes, plane_off);
        __syncthreads();
    }
}
__global__ __launch_bounds__(kProfileThreads) void ambi_fold_scan_kernel(BatchArgs A, int which, int jwin, int slots, uint8_t* planes, int64_t plane_bytes, const int64_t* plane_off, uint8_t* block, const int64_t* off) {
    BlockGroup g(reinterpret_cast<int*>(ambi_lds));
    const FoldTable T = fold_table(ambi_lds + kProfileScratchBytes, slots);
    for (int u = (int)blockIdx.x; u < A.n_units; u += (int)gridDim.x) {
        fold_scan_unit(g, A.units, A.junc_ends, A.results, u, which, jwin, T, planes, plane_bytes, plane_off, block, off);
        __syncthreads();
    }
}
// ---- path comparison (ambi_path_compare.hpp; launched by HipBackend::profile_queue only) ----
// One workgroup of 256 threads per pair, grid-stride over the pairs.  Group memory: 256 bytes for the group's reductions, then the
// diagonal array V of 2 * dmax + 3 ints (8204 bytes at the cap of 1024).
__global__ __launch_bounds__(kProfileThreads) void ambi_path_compare_kernel(BatchArgs A, CompareGiven given, const int32_t* pairs, int n_pairs, int dmax, PathCompare* out) {
    BlockGroup g(reinterpret_cast<int*>(ambi_lds));
    int32_t* V = reinterpret_cast<int32_t*>(ambi_lds + kProfileScratchBytes);
    for (int i = (int)blockIdx.x; i < n_pairs; i += (int)gridDim.x) {
        compare_pair(g, A.units, A.results, given, pairs, i, dmax, V, out);
        __syncthreads();
    }
}
// ---- path alignment (ambi_path_align.hpp; launched by HipBackend::profile_queue only) ----
// One workgroup of 256 threads per pair, grid-stride over the pairs.  Group memory: 256 bytes for the group's reductions, the diagonal
// array V (2 * dmax + 3 ints) and the edit list (2 * dmax ints): 16652 bytes at the cap of 1024.  hist: one history area of
// hist_bytes per workgroup, written and read by that workgroup only.
__global__ __launch_bounds__(kProfileThreads) void ambi_path_align_kernel(BatchArgs A, CompareGiven given, const int32_t* triples, int n_pairs, int dmax, uint8_t* hist,
                                                                          int64_t hist_bytes, PathAlign* head, AlignRun* runs) {
    BlockGroup g(reinterpret_cast<int*>(ambi_lds));
    int32_t* V = reinterpret_cast<int32_t*>(ambi_lds + kProfileScratchBytes);
    int32_t* E = V + (2 * dmax + 3);
    int32_t* H = reinterpret_cast<int32_t*>(hist + (int64_t)blockIdx.x * hist_bytes);
    for (int i = (int)blockIdx.x; i < n_pairs; i += (int)gridDim.x) {
        align_pair(g, A.units, A.results, given, triples, i, dmax, V, E, H, head, runs);
        __syncthreads();
    }
}
// ---- path coordinates (ambi_path_coords.hpp; launched by HipBackend::profile_queue only) ----
// The scan: one workgroup of 256 threads per unit, grid-stride over the units, 512 cells a round; 256 bytes of group memory for the
// group's scans.  Store-bound: 8 bytes per cell out, as one 16-byte store per thread and round, for 2 bytes in.  The lift, behind it
// on the same stream: one thread per query, grid-stride; a query costs a bisection over its unit's slice (23 dependent 8-byte loads
// at most) -- latency-bound, and hidden by the number of queries in flight.
__global__ __launch_bounds__(kProfileThreads) void ambi_path_coords_kernel(BatchArgs A, LenArgs I, int which, uint8_t* planes, const int64_t* plane_off, uint8_t* block) {
    BlockGroup g(reinterpret_cast<int*>(ambi_lds));
    for (int u = (int)blockIdx.x; u < A.n_units; u += (int)gridDim.x) {
        coords_unit(g, A.units, A.results, I, u, which, planes, plane_off, block);
        __syncthreads();
    }
}
__global__ __launch_bounds__(kProfileThreads) void ambi_path_lift_kernel(BatchArgs A, LenArgs I, int which, const uint8_t* planes, const int64_t* plane_off, const uint8_t* block,
                                                                         const LiftQuery* queries, int64_t n, PathLift* out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        lift_query(A.units, A.results, I, which, planes, plane_off, block, queries, i, out);
}
// ---- nucleotide sequence of the paths (ambi_sequence.hpp; launched by HipBackend::sequence only) ----
// Extents: one workgroup of 256 threads per unit of the request, grid-stride; 160 bytes of group memory for the group's
// reductions and scans (read-bound: 2 bytes per cell, twice -- pass 0 counts, pass 1 writes the extents).
__global__ __launch_bounds__(kSeqTileLanes) void ambi_seq_extents_kernel(BatchArgs A, SeqArgs S, SeqPlan Q, int which, int pass) {
    __shared__ __align__(16) int scratch[40];   // (exscan_i64: 16 wave totals of 8 bytes)
    BlockGroup g(scratch);
    for (int r = (int)blockIdx.x; r < Q.count; r += (int)gridDim.x) {
        seq_extents_unit(g, A.units, A.results, S, Q, r, which, pass);
        __syncthreads();
    }
}
// Fill: workgroups of 256 threads, each over a CONTIGUOUS span of tiles of 4 KB of output (the cursor of ambi_sequence.hpp finds a
// tile's unit and runs from the tile before); 256 bytes of group memory for the complement table.
// Store-bound by design: one 16-byte store per lane, the source mostly an L2 hit (a unit's store is read once per crossing).
__global__ __launch_bounds__(kSeqTileLanes) void ambi_seq_fill_kernel(SeqArgs S, SeqPlan Q, int64_t n_tiles) {
    __shared__ __align__(16) uint8_t table[256];
    BlockGroup g(nullptr);   // (no exchange between the threads behind the table)
    seq_build_table(g, table);
    __syncthreads();
    const int64_t per = (n_tiles + (int64_t)gridDim.x - 1) / (int64_t)gridDim.x, t0 = (int64_t)blockIdx.x * per;
    const int64_t t1 = t0 + per < n_tiles ? t0 + per : n_tiles;
    SeqCursor cur;
    for (int64_t t = t0; t < t1; t++) seq_fill_tile(g, S, Q, table, t, cur);
}
// one wavefront per run
__global__ __launch_bounds__(256) void ambi_expand_runs_kernel(const int32_t* run_start, const int32_t* run_len, const int64_t* cell_off, int64_t n_runs,
                                                               int32_t* cells, int64_t cap) {
    WaveGroup g;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t r = wave; r < n_runs; r += nwaves) expand_run(g, run_start, run_len, cell_off, r, cells, cap);
}

// ---- do two streams dispatch side by side? ----
// A kernel with a backlog of workgroups on stream a, one tiny workgroup on stream b: if b's workgroup only starts when a's backlog
// has been handed out, the two streams feed the same dispatch pipe of the command processor (queues of one pipe hand out their
// workgroups one kernel after the other), and a finish kernel on b would run BEHIND an order-table kernel on a instead of beside
// it (measured: 1.28 instead of 0.86 ms per step, profiles/r04_notes.md).  The engine asks this question about the caller's
// stream and its own side streams instead of assuming a mapping of streams to hardware queues.
__global__ __launch_bounds__(256) void ambi_spin_kernel(int64_t ticks, int32_t* sink) {
    const int64_t t0 = (int64_t)wall_clock64();
    while ((int64_t)wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
    if (sink && threadIdx.x == 0 && blockIdx.x == 0x7fffffff) *sink = 1;
}
__global__ void ambi_touch_kernel(int32_t* sink) { if (sink && blockIdx.x == 0x7fffffff) *sink = 1; }
// What the engine keeps per device ordinal, with PROCESS lifetime (DevicePool::context creates it on first use, on that device;
// nothing in it is destroyed): the probe's events and the device figures it needs, the dispatch classes of the candidate side
// streams (side_streams below) and whether the dynamic-LDS ceiling has been set.  `mu` is held by every probe and every look-up.
struct DeviceContext {
    std::mutex mu;
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;    // the probe's events
    int64_t ticks_per_us = 100; int ncu = 256;              // wall-clock rate, compute units
    std::vector<hipStream_t> cand; std::vector<int> cls;    // candidate side streams in creation order, and their classes
    std::vector<hipStream_t> rep;                           // one stream per class (class index = position)
    std::vector<std::pair<hipStream_t, uint32_t>> callers;  // callers' streams seen so far, with the SET of classes each collides with
    bool classed = false;                                   // cls and rep are built
    bool lds_ceiling = false;                               // every kernel's dynamic-LDS ceiling is set (upload())
};
// microseconds from the start of the backlog kernel on a to the end of the tiny kernel on b (both streams of C's device and idle
// before and after; C.mu held)
static int stream_probe_us(DeviceContext& C, hipStream_t a, hipStream_t b, float* us) {
    HIP_CK(hipStreamSynchronize(a)); HIP_CK(hipStreamSynchronize(b));
    // 16 rounds of workgroups that hold a CU slot for ~6 us each: ~100 us of backlog
    HIP_CK(hipEventRecord(C.e0, a));
    hipLaunchKernelGGL(ambi_spin_kernel, dim3(C.ncu * 8 * 16), dim3(256), 0, a, (int64_t)(6 * C.ticks_per_us), (int32_t*)nullptr);
    HIP_CK(hipEventRecord(C.e2, a));   // (b must not start before a's kernel has been queued: it waits for nothing of a's, only the host order matters)
    hipLaunchKernelGGL(ambi_touch_kernel, dim3(1), dim3(64), 0, b, (int32_t*)nullptr);
    HIP_CK(hipEventRecord(C.e1, b));
    HIP_CK(hipStreamSynchronize(a)); HIP_CK(hipStreamSynchronize(b));
    float ms = 0;
    HIP_CK(hipEventElapsedTime(&ms, C.e0, C.e1));
    *us = ms * 1e3f;
    return 0;
}

// The dynamic-LDS ceiling of a kernel is a per-function, process-wide attribute: every batch asks for the device limit,
// so that a second batch with smaller units cannot lower it under a first batch that is still launching (the launches
// themselves request only what their units need).
constexpr int kLdsMaxDynamic = 160 * 1024 - 1024;

// Every backend entry that touches the GPU runs on the device of the batch's lease, whatever device the calling thread has
// current (a batch dealt over several devices answers its per-unit getters from the device that holds the unit; a host
// program working on another device finds its current device unchanged afterwards).  dev < 0: nothing to select.
struct DeviceGuard {
    int prev = -1; bool switched = false;
    explicit DeviceGuard(int dev) {
        if (dev < 0 || hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); return; }
        if (prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete; DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// ------------------------------------------------------------------------------------------------
// Per-device resources with PROCESS lifetime.
//
// Round 2 created and destroyed 3-4 streams (one of them with a dispatch priority), 6+ events and three pinned allocations
// with every batch, and a long create / run / destroy loop showed rare stray writes into host memory of the process
// (DESIGN.md 8b).  Nothing the HIP runtime hands out is destroyed per batch any more: a batch LEASES a context -- events,
// the pinned words the kernels report through, a pinned staging block, a pinned result mailbox, grow-only device blocks, a
// copy stream -- from a per-device free list and gives it back when it is destroyed (after synchronising every stream it
// used).  Its side streams come from the device's context (side_streams).  Leases and contexts are never destroyed; at
// process exit they are left to the runtime.
// ------------------------------------------------------------------------------------------------
struct PinnedWords {                    // what kernels write into host memory (BatchArgs::host_pending, host_needed, express_*, plan_seq, late_flag)
    uint32_t guard_lo[16];
    int32_t npending, express_left, express_seq, plan_seq, late_flag, lat_seq, lat_unsure, pad_[9];
    int64_t needed[16];
    uint32_t guard_hi[16];
};
struct TimingEvents { const char* name; hipEvent_t a, b; };
// grow-only block of the lease (device memory, or pinned host memory with its device address)
static int lease_device_block(uint8_t** p, int64_t* have, int64_t want) {
    if (*have >= want && *p) return 0;
    if (*p) { (void)hipFree(*p); *p = nullptr; *have = 0; }
    want = (want + 4095) & ~int64_t(4095);
    HIP_CK(hipMalloc((void**)p, (size_t)want));
    *have = want;
    return 0;
}
static int lease_pinned_block(uint8_t** p, uint8_t** dp, int64_t* have, int64_t want) {
    if (*have >= want && *p) return 0;
    if (*p) { (void)hipHostFree(*p); *p = nullptr; *have = 0; }
    want = (want + 4095) & ~int64_t(4095);
    HIP_CK(hipHostMalloc((void**)p, (size_t)want));
    if (dp) HIP_CK(hipHostGetDevicePointer((void**)dp, *p, 0));
    *have = want;
    return 0;
}
static void trim_device_block(uint8_t*& p, int64_t& have, int64_t keep) { if (have > keep) { (void)hipFree(p); p = nullptr; have = 0; } }   // what is larger than `keep` goes back when the batch is destroyed
static void trim_pinned_block(uint8_t*& p, int64_t& have, int64_t keep) { if (have > keep) { (void)hipHostFree(p); p = nullptr; have = 0; } }
// The lease's part of one on-request result (HipBackend::profile_queue; the kinds' table: Backend::ProfileKind): the block with its
// tail behind it, its pinned twin, the kind's side area, which stays on the device, and three events (the run's stream reached /
// kernel done / block arrived)
struct RequestBlock {
    uint8_t* d = nullptr; int64_t d_bytes = 0;
    uint8_t* h = nullptr; int64_t h_bytes = 0;
    uint8_t* side = nullptr; int64_t side_bytes = 0;
    hipEvent_t ev_src = nullptr, ev_packed = nullptr, ev_done = nullptr;
    void trim(int64_t keep, int64_t keep_side) { trim_device_block(d, d_bytes, keep); trim_pinned_block(h, h_bytes, keep); trim_device_block(side, side_bytes, keep_side); }
};
// An input of the on-request kernels that does not travel with the batch: a device block of its own, the pinned twin that carries it
// up, the event behind the last upload and the version the device holds (-1: nothing).  Which kernels still read the old image is
// the caller's to know: it waits for them before it asks for another version.
struct DeviceImage {
    uint8_t* d = nullptr; int64_t d_bytes = 0;
    uint8_t* h = nullptr; int64_t h_bytes = 0;
    hipEvent_t ev_up = nullptr;
    int64_t version = -1;
    bool holds(int64_t want) const { return version == want && d; }
    // `s` is ordered behind the upload of version `want` when this returns, whichever stream carried it: the image goes up on `s`
    // (fill(twin), one copy of `total` bytes) when the device holds another version
    template <class Fill> int upload(hipStream_t s, int64_t want, int64_t total, Fill fill) {
        if (holds(want)) { HIP_CK(hipStreamWaitEvent(s, ev_up, 0)); return 0; }   // (the upload may have gone up on another stream)
        if (!ev_up) HIP_CK(hipEventCreateWithFlags(&ev_up, hipEventDisableTiming));
        else HIP_CK(hipEventSynchronize(ev_up));   // (an earlier upload still reads the twin)
        if (int rc = lease_device_block(&d, &d_bytes, total)) return rc;
        if (int rc = lease_pinned_block(&h, nullptr, &h_bytes, total)) return rc;
        fill(h);
        HIP_CK(hipMemcpyAsync(d, h, (size_t)total, hipMemcpyHostToDevice, s));
        HIP_CK(hipEventRecord(ev_up, s));
        version = want;
        return 0;
    }
    void trim(int64_t keep) { trim_device_block(d, d_bytes, keep); trim_pinned_block(h, h_bytes, keep); }
};
struct Lease {
    int device = 0;
    DeviceContext* ctx = nullptr;   // the device's
    hipEvent_t ev_fork = nullptr, ev_prep = nullptr, ev_back = nullptr, ev_first = nullptr, ev_full = nullptr, ev_plan = nullptr, ev_express = nullptr, ev_lat = nullptr, ev_tail = nullptr;
    PinnedWords* h_words = nullptr; PinnedWords* dh_words = nullptr;
    uint8_t* d_block = nullptr; int64_t d_block_bytes = 0;      // inputs + working set + result blob of the batch
    uint8_t* d_arena = nullptr; int64_t d_arena_bytes = 0;      // order tables
    uint8_t* d_cells = nullptr; int64_t d_cells_bytes = 0;      // path areas of the direct full-finish launch
    uint8_t* h_stage = nullptr; uint8_t* dh_stage = nullptr; int64_t h_stage_bytes = 0;   // pinned image of the inputs (one H2D copy, or read by the ingest kernel)
    uint8_t* h_mail = nullptr; uint8_t* dh_mail = nullptr; int64_t h_mail_bytes = 0;   // pinned result mailbox (express path)
    // final paths in run-length form on their way to the host (runs_to_host): two slots, each a device block and its pinned mirror,
    // a copy stream of the lease's own and two events per slot (packed / arrived)
    uint8_t* d_runs[2] = {nullptr, nullptr}; int64_t d_runs_bytes[2] = {0, 0};
    uint8_t* h_runs[2] = {nullptr, nullptr}; int64_t h_runs_bytes[2] = {0, 0};
    hipStream_t run_stream = nullptr;   // own_stream(): for callers without a stream (ambi_batch_run_sharded's shares)
    hipStream_t copy_stream = nullptr; hipEvent_t ev_runs_packed[2] = {nullptr, nullptr}, ev_runs_done[2] = {nullptr, nullptr};
    RequestBlock prof[Backend::kProfileKinds];   // [Backend::ProfileKind]
    // the batch's fragment image (HipBackend::fragment_image: [cells][frag_off][cell_off][pref_off][n_frag]) and the given paths of
    // the compare and of the align kind (ComparePaths::image: [off][len][cells]; each kind its request's own copy of the set)
    // and the batch's length image (HipBackend::length_image: [len][len_off])
    enum { kFragImage = 0, kGivenImage = 1, kLenImage = 3 };   // (the given sets: kGivenImage + kind - kCompare)
    DeviceImage img[4];
    // path sequences (HipBackend::sequence): the batch's sequence image [bases][seg_pos][store_off][pos_off], the working block of a
    // request [totals][ext_off, out_off, tile_off][ext_src][ext_out] and the output block; the pinned twin carries the image up, the
    // totals down and the three offset tables up.  Events: the run's stream reached / all queued work done / timing pairs
    uint8_t* d_seq_img = nullptr; int64_t d_seq_img_bytes = 0;
    uint8_t* d_seq_work = nullptr; int64_t d_seq_work_bytes = 0;
    uint8_t* d_seq_out = nullptr; int64_t d_seq_out_bytes = 0;
    uint8_t* h_seq = nullptr; int64_t h_seq_bytes = 0;
    hipEvent_t ev_seq_src = nullptr, ev_seq_done = nullptr, ev_seq_t[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // pass 0: [0, 1]; pass 1: [2, 3]; fill: [3, 4]
    std::vector<TimingEvents> evs;
    long uses = 0;
    int32_t seq = 0;   // run sequence numbers (the kernels report completion by storing the run's number into a pinned word)
};
// what stays cached in a lease between batches (larger blocks go back to the device when the batch is destroyed)
constexpr int64_t kKeepBlock = 64ll << 20, kKeepArena = 256ll << 20, kKeepCells = 64ll << 20, kKeepStage = 16ll << 20, kKeepMail = 8ll << 20, kKeepRuns = 16ll << 20, kKeepProfile = 16ll << 20, kKeepSeq = 64ll << 20;

class DevicePool {
    std::mutex mu_;                       // the free list and the contexts' table: never held during a probe
    std::vector<Lease*> free_;
    std::vector<DeviceContext*> ctx_;     // one per device ordinal
    DevicePool() { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess || n < 0) n = 0; ctx_.assign((size_t)n, nullptr); }
  public:
    static DevicePool& get() { static DevicePool* p = new DevicePool(); return *p; }   // (never destroyed: no HIP call from a static destructor)
    int context(int dev, DeviceContext** out) {
        std::lock_guard<std::mutex> lk(mu_);
        if (dev < 0 || dev >= (int)ctx_.size()) return -31;
        if (!ctx_[dev]) {
            DeviceGuard dg(dev);
            DeviceContext* C = new DeviceContext();
            HIP_CK(hipEventCreate(&C->e0)); HIP_CK(hipEventCreate(&C->e1)); HIP_CK(hipEventCreateWithFlags(&C->e2, hipEventDisableTiming));
            int khz = 0, ncu = 0;
            if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && khz / 1000 > 0) C->ticks_per_us = khz / 1000;
            if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0) C->ncu = ncu;
            ctx_[dev] = C;
        }
        *out = ctx_[dev];
        return 0;
    }
    int acquire(Lease** out) {
        int dev = 0;
        HIP_CK(hipGetDevice(&dev));
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (size_t i = 0; i < free_.size(); i++)
                if (free_[i]->device == dev) { *out = free_[i]; free_.erase(free_.begin() + (long)i); (*out)->uses++; return 0; }
        }
        {   // the engine's streams want hardware queues of their own: say so when the runtime was started without them
            static std::once_flag warned;
            std::call_once(warned, [] {
                const char* q = getenv("GPU_MAX_HW_QUEUES");
                if (!q || atoi(q) < 8)
                    fprintf(stderr, "ambigram_hip: warning: GPU_MAX_HW_QUEUES is %s when the engine creates its streams; with fewer than 8 hardware queues two of "
                                    "them can share one and the finish kernels then run behind the order-table kernel instead of beside it (measured: 1.55 "
                                    "instead of 1.10 ms per 4096-sample step).  Set GPU_MAX_HW_QUEUES=8 in the environment before the HIP runtime starts.\n", q ? q : "unset");
            });
        }
        DeviceContext* C = nullptr;
        if (int rc = context(dev, &C)) return rc;
        Lease* L = new Lease();
        L->device = dev; L->ctx = C;
        hipEvent_t* evs[] = {&L->ev_fork, &L->ev_prep, &L->ev_back, &L->ev_first, &L->ev_full, &L->ev_plan, &L->ev_express, &L->ev_lat, &L->ev_tail};
        for (hipEvent_t* e : evs) HIP_CK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        HIP_CK(hipHostMalloc((void**)&L->h_words, sizeof(PinnedWords)));
        memset(L->h_words, 0, sizeof(PinnedWords));
        for (int i = 0; i < 16; i++) { L->h_words->guard_lo[i] = kGuardWord; L->h_words->guard_hi[i] = kGuardWord; }
        HIP_CK(hipHostGetDevicePointer((void**)&L->dh_words, L->h_words, 0));
        L->uses = 1;
        *out = L;
        return 0;
    }
    void release(Lease* L) {
        if (!L) return;
        std::lock_guard<std::mutex> lk(mu_);
        free_.push_back(L);
    }
};
// ---- side streams that really run beside the caller's stream ----
// The command processor hands out workgroups through four dispatch pipes; the streams of a process are spread over them in
// creation order, and two streams on one pipe hand out their kernels' workgroups one kernel after the other.  Which pipe a stream
// got cannot be asked, only observed (stream_probe_us), so the device's context keeps eight candidate streams, sorted into
// classes of streams that do NOT run side by side, learns the class of every caller's stream when it first sees it, and gives a
// batch side streams from the other classes.  (Round 3 relied on the creation order: correct for the legacy default stream in a
// process that creates no other streams first, 1.28 instead of 0.86 ms per step on a stream of torch's pool.)
constexpr float kProbeSharedUs = 55.f;   // measured: 10-17 us side by side, 105-125 us behind the backlog
struct SideStreams { hipStream_t lean = nullptr, full = nullptr, scan = nullptr; };   // lean finish, direct full finish, scan for the first valid order + lattice kernel
static int add_candidates(DeviceContext& C, size_t n) {   // the first n candidates exist
    while (C.cand.size() < n) { hipStream_t t; HIP_CK(hipStreamCreateWithFlags(&t, hipStreamNonBlocking)); C.cand.push_back(t); }
    return 0;
}
static int stream_class_of(DeviceContext& C, hipStream_t s, int* out) {   // -1: runs beside every known class
    for (size_t c = 0; c < C.rep.size(); c++) {
        float us = 0;
        if (int rc = stream_probe_us(C, C.rep[c], s, &us)) return rc;
        if (us > kProbeSharedUs) { *out = (int)c; return 0; }
    }
    *out = -1;
    return 0;
}
static int build_stream_classes(DeviceContext& C) {
    if (C.classed) return 0;
    C.cls.clear(); C.rep.clear();
    { float us;   // first use of the probe kernels (code loading) outside the measurements
      if (int rc = add_candidates(C, 2)) return rc;
      if (int rc = stream_probe_us(C, C.cand[0], C.cand[1], &us)) return rc; }
    // eight candidates; up to sixteen while fewer than four classes have shown up (other libraries' streams -- RCCL's -- sit between
    // the engine's in creation order)
    for (size_t i = 0; i < 16; i++) {
        if (i >= 8 && C.rep.size() >= 4) break;
        if (int rc = add_candidates(C, i + 1)) return rc;
        int c = -1;
        if (int rc = stream_class_of(C, C.cand[i], &c)) return rc;
        if (c < 0) { c = (int)C.rep.size(); C.rep.push_back(C.cand[i]); }
        C.cls.push_back(c);
    }
    C.classed = true;
    if (ambi_env("AMBI_DEBUG")) { fprintf(stderr, "ambigram_hip: %zu dispatch classes among %zu candidate streams:", C.rep.size(), C.cand.size()); for (int c : C.cls) fprintf(stderr, " %d", c); fprintf(stderr, "\n"); }
    return 0;
}
// The side streams of a batch whose kernels start on `caller`: from classes other than the caller's and, while there are enough
// classes, from different ones; `set`: which of the candidates of a class.  Never a null stream on success.
static int side_streams(DeviceContext& C, hipStream_t caller, int set, bool classes_on, SideStreams* out) {
    std::lock_guard<std::mutex> lk(C.mu);
    if (classes_on) { if (int rc = build_stream_classes(C)) return rc; }
    // Every class the caller's stream collides with, in either direction: a stream can sit on the dispatch pipe of one class AND share a
    // hardware queue with a candidate of another (the legacy default stream of a process that creates it after the candidates: the lattice
    // kernel of a single sample then ran BEHIND the express kernel on one queue, 142 instead of 89 us end to end from a C caller).
    const int nc = classes_on ? (int)C.rep.size() : 0;   // (classes off: none, and no probe)
    uint32_t mask = 0; bool known = nc == 0;
    for (auto& pr : C.callers) if (pr.first == caller) { mask = pr.second; known = true; }
    if (!known) {
        for (size_t i = 0; i < C.cls.size(); i++) if (C.cand[i] == caller) { mask = 1u << C.cls[i]; known = true; }
        if (!known) {
            for (int c = 0; c < nc; c++) {
                float ab = 0, ba = 0;
                if (int rc = stream_probe_us(C, C.rep[c], caller, &ab)) return rc;
                if (ab <= kProbeSharedUs) { if (int rc = stream_probe_us(C, caller, C.rep[c], &ba)) return rc; }
                if (ab > kProbeSharedUs || ba > kProbeSharedUs) mask |= 1u << c;
            }
        }
        C.callers.push_back({caller, mask});
        if (ambi_env("AMBI_DEBUG")) fprintf(stderr, "ambigram_hip: caller's stream %p collides with the dispatch classes 0x%x (of %d)\n", (void*)caller, mask, nc);
    }
    int cc = -1;
    for (int c = 0; c < nc; c++) if ((mask >> c) & 1u) { cc = c; break; }
    hipStream_t s[3];
    int k = 0;
    for (int step = 1; step <= nc && k < 3; step++) {
        const int c = ((cc < 0 ? 0 : cc) + step) % nc;
        if ((mask >> c) & 1u) continue;
        // the set-th candidate of class c (wrapping)
        std::vector<hipStream_t> of;
        for (size_t i = 0; i < C.cls.size(); i++) if (C.cls[i] == c) of.push_back(C.cand[i]);
        if (of.empty()) continue;
        s[k++] = of[(size_t)set % of.size()];
    }
    if (k == 0) {   // every class behaves like the caller's stream (a profiler that serialises the kernels), or classes off: creation order
        if (int rc = add_candidates(C, 3)) return rc;
        for (; k < 3; k++) s[k] = C.cand[k];
    }
    for (int j = k; j < 3; j++) s[j] = s[j % k];   // fewer classes than streams: some share
    *out = SideStreams{s[0], s[1], s[2]};
    return 0;
}
// ambi_debug_stream_probe: on the current device, serialised with the engine's own probes there
int backend_stream_probe(void* a, void* b, float* us) {
    int dev = 0;
    HIP_CK(hipGetDevice(&dev));
    DeviceContext* C = nullptr;
    if (int rc = DevicePool::get().context(dev, &C)) return rc;
    std::lock_guard<std::mutex> lk(C->mu);
    return stream_probe_us(*C, (hipStream_t)a, (hipStream_t)b, us);
}

// scoped device allocation / event pair for the helpers that allocate per call (freed on every return path)
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

// ------------------------------------------------------------------------------------------------
// backend
// ------------------------------------------------------------------------------------------------
class HipBackend : public Backend {
    const HostBatch* hbp_ = nullptr;   // the batch's packed inputs (owned by the ambi_batch that owns this backend)
    const HostBatch& hb() const { return *hbp_; }
    EngineConfig cfg_;
    bool uploaded_ = false, timing_ = false, arena_checked_ = false, ran_ = false;
    bool inflight_ = false;            // a run has been queued and not yet waited for
    bool upload_pending_ = false;      // the input image sits in pinned staging: the first run queues its copy (and the zero fill) ahead of the kernels
    bool late_refusal_ = false;        // a unit of this batch is refused by the lattice / plan stage (known after one complete run: inputs are immutable)
    bool tuned_ = false;               // the launch parameters that depend on the first run's outcome have been chosen
    uint32_t timing_mask_ = ~0u;   // kernels that get events (bit = kernel index)
    hipStream_t stream_ = nullptr;
    Lease* lease_ = nullptr;
    int device_ = -1;                  // the device of the lease (set at upload): every entry below selects it for its duration
    // device buffers: all carved from ONE block of the lease (layout()); inputs first, in the order of the staging image
    UnitIn* d_units_ = nullptr; double* d_seg_cn_ = nullptr; double* d_junc_cn_ = nullptr; JuncEnds* d_junc_ends_ = nullptr; Element* d_elems_ = nullptr;
    Dag* d_dags_ = nullptr; uint8_t* d_results_ = nullptr;
    uint64_t* d_ikeys_ = nullptr; uint64_t* d_icnt_ = nullptr; uint32_t* d_ilink_ = nullptr; int32_t* d_ilvl_off_ = nullptr; int32_t* d_icounter_ = nullptr;
    int32_t* d_ipos_ = nullptr; uint64_t* d_aavail_ = nullptr; uint64_t* d_acnt_ = nullptr; int32_t* d_acbase_ = nullptr; uint16_t* d_achild_ = nullptr;
    int enum_stack_lds_ = 0, enum_auto_lds_ = 4096, enum_classes_ = 0, block_lds_ = 49152, lds_blocks_ = 0, block_scratch_lds_ = 32768, lds_build_ = 0, block_max_ = 256;
    int64_t* d_stage_clk_ = nullptr;
    int32_t* d_fallback_ = nullptr; uint8_t* d_blk_img_ = nullptr; int32_t* d_blk_hdr_ = nullptr;
    uint8_t* d_arena_ = nullptr; int64_t arena_bytes_ = 0;
    int64_t* d_blk_off_ = nullptr; int32_t* d_rows_ = nullptr; int32_t* d_npending_ = nullptr; int64_t* d_needed_ = nullptr;
    int32_t* d_scratch_ = nullptr; int64_t* d_scratch_off_ = nullptr; int64_t* d_pack_off_ = nullptr;
    int64_t* d_mail_off_ = nullptr; int32_t* d_guard_bad_ = nullptr;
    int64_t* d_run_slot_ = nullptr; int32_t* d_run_blk_[2] = {nullptr, nullptr}; int64_t run_total_ = 0; int runs_parity_ = -1;   // finish-stage runs: [cnt U][cells U][start total][len total] per run parity
    WideUnit* d_wide_ = nullptr; int32_t* d_wide_index_ = nullptr; int32_t* d_wide_units_ = nullptr; int n_wide_ = 0;   // units with 64..127 nodes (ambi_wide.hpp)
    int32_t* h_npending_ = nullptr; int64_t* h_needed_ = nullptr;   // pinned (words of the lease)
    int32_t* dh_npending_ = nullptr; int64_t* dh_needed_ = nullptr; // the same two, as the device addresses them
    int64_t in_bytes_ = 0, zero_off_ = 0, zero_bytes_ = 0;          // input image / zero-filled region of the block
    std::vector<uint8_t> stage_big_;                                // input image of a batch too large for the pinned staging block
    std::vector<int64_t> mail_off_; int64_t mail_bytes_ = 0; bool mail_on_ = false, mail_valid_ = false;
    BatchArgs A_{};
    int lds_prepare_ = 0, lds_first_ = 0, lds_finish_ = 0, lds_finish_lean_ = 0, lds_enum_ = 0;
    bool lean_finish_ = true;   // env AMBI_LEAN_FINISH=0: every unit through the full finish stage
    int finish_grid_ = 0;       // workgroups of the lean finish kernel; 0 = sized per run (env AMBI_FINISH_GRID overrides)
    int32_t* d_blocks_done_ = nullptr; int32_t* d_refin_list_ = nullptr; int32_t* d_refin_count_ = nullptr;
    uint32_t* d_anblk_ = nullptr; uint8_t* d_adepth_ = nullptr;
    int finish_path_cells_ = 0;
    std::vector<KernelTime> times_;
    typedef TimingEvents Ev;
    std::vector<Ev>& evs() { return lease_->evs; }
    int64_t last_needed_ = 0;
    int general_path_ = -1;   // units that take the general enumerate path: -1 unknown (first run), else the count (inputs are immutable)
    int shared_units_ = -1;   // units whose table is written by several workgroups: -1 unknown, else the count
    long timed_runs_ = 0;
    hipEvent_t ev_fork_ = nullptr;
    // overlap of [first valid order, finish] with the enumerate kernel: side streams + events (the lease's)
    bool overlap_back_ = false, want_overlap_ = true;
    SideStreams side_; hipStream_t side_for_ = (hipStream_t)-1;   // side streams of the step (side_streams) and the caller's stream they were chosen for
    hipEvent_t ev_prep_ = nullptr, ev_back_ = nullptr, ev_first_ = nullptr, ev_full_ = nullptr;
    bool first_launched_ = false; hipEvent_t ev_plan_ = nullptr;
    uint8_t* d_direct_cells_ = nullptr; int64_t direct_stride_ = 0; int direct_slots_ = 0; int lds_finish_ext_ = 0; bool direct_ext_ = true;   // env AMBI_DIRECT_EXT: the direct launch keeps its path cells in device memory
    int direct_cells_ = 0; bool direct_retry_ = false;   // path area of the direct full-finish launch (0: the batch's capacity bound); env AMBI_DIRECT_CELLS
    int full_threads_ = 1024;  // env AMBI_FULL_THREADS: threads per workgroup of the direct full-finish launch (256 / 512 / 1024)
    int32_t* d_direct_list_ = nullptr; int direct_n_ = 0, direct_grid_ = 1024;
    int32_t* d_edit_list_ = nullptr; bool direct_edit_ = true; int lds_finish_edit_ = 0, edit_grid_ = 1024;   // env AMBI_DIRECT_EDIT: these units through stage_finish_edit first (ambi_finish_edit_kernel), the ext launch behind it for what that hands on
    // express path (small batches): one kernel reconstructs every unit whose first order assembles; results are complete at ev_express_
    // (measured, one 256-segment sample: 256 / 512 / 1024 threads = 79.7 / 76.8 / 79.2 us run -> results)
    static constexpr int kExpressThreads = 512;   // the serial stages use three wavefronts, the finish stage and the mailbox copy all of them
    int express_units_ = 32, lds_express_ = 0, lds_lattice_ = 0, lds_lattice_own_ = 0;
    bool lazy_ = false, tables_written_ = false;   // FLAG_LAZY_ORDERS: the run leaves the order tables out; they are written on demand
    bool side_lattice_ = false, flushed_ = false;   // small batches: the lattice kernel beside the express kernel
    uint64_t* d_lat_R_ = nullptr; int32_t* d_lat_status_ = nullptr; int64_t* d_lat_sum_ = nullptr;
    bool express_ = false;
    hipEvent_t ev_express_ = nullptr;
    int32_t* h_express_left_ = nullptr; int32_t* dh_express_left_ = nullptr;   // [0] left flag, [1] sequence word (words of the lease)
    int32_t run_seq_ = 0;
    uint8_t* d_first_rows_ = nullptr;
    int build_in_emit_ = 1;   // env AMBI_BUILD_IN_EMIT=0: every image through the build kernel and HBM
    int order_align_ = 4096;  // env AMBI_ORDER_ALIGN: every unit's table starts on a 4 KB boundary of the arena (a store stream whose 1 KB pieces are
                              // line-aligned: 5.4 -> 5.7 TB/s on a pure store stream of this shape, profiles/tools/hbm_write_pat5.hip)
    int emit_interleave_ = 1; // env AMBI_EMIT_INTERLEAVE=0: every wave a contiguous quarter of the work block instead of every fourth block
    int block_dfs_ = 1;       // env AMBI_BLOCK_DFS=0: no directory-free images (units whose directory does not fit take the general path)
    std::vector<std::vector<int64_t>> all_idx_[2];   // --all: valid order indices per pass and unit (filled when asked for)
    std::vector<std::vector<uint64_t>> all_cache_;   // --all: a unit's bitmap words once fetched
    std::vector<int64_t> all_off_, all_R_;
    std::vector<int32_t> all_counts_;
    uint64_t* d_all_bits_ = nullptr; int64_t* d_all_off_ = nullptr; int32_t* d_all_count_ = nullptr; int32_t* d_all_flags_ = nullptr;
    int8_t* d_inject_ = nullptr; int64_t* d_inject_off_ = nullptr;
    float all_kernel_ms_ = -1.f;
    int64_t all_bits_cap_ = 0, all_pool_bytes_ = 0;
    int all_rank_ = 0, all_world_ = 1;
    bool all_done_ = false;
    int enum_grid_ = 2048;
    bool emit_lds_auto_ = true;
    bool emit_lds_tight_ = true;   // env AMBI_EMIT_LDS_TIGHT=0: the whole 160 KB / k share
    double avg_path_ = 0;
    static constexpr int kEnumThreads = 256;   // threads per workgroup of the block-emission kernel (512 / 1024 measured slower)
    std::chrono::steady_clock::time_point t_run_; double t_launched_ = 0;   // env AMBI_DEBUG_LATENCY
    bool debug_ = false;      // env AMBI_DEBUG: budgets and grids chosen; guard words of the direct path areas checked at wait()

    // per-batch state of one on-request profile (profile_queue): a request is in flight or waited for, the block is laid out and its
    // offsets are on the device (d_off), and what profile_wait() needs to queue it again
    struct Request {
        bool queued = false, laid_out = false;
        int which = 1; int64_t epoch = -1; hipStream_t stream = nullptr;
        int64_t* d_off = nullptr;
    };
    Request req_[kProfileKinds];   // [ProfileKind]
    void requests_reset() { for (int k = 0; k < kProfileKinds; k++) { req_[k] = Request{}; prof_[k].view = nullptr; } }

    // Everything this batch queued is complete when this returns: the caller's stream (only if a run is still in flight -- the
    // stream must outlive its work), the side streams this batch used and the lease's copy and run streams, each synchronised
    // EXPLICITLY (round 2 relied on hipFree's implicit device synchronisation and destroyed streams it had never synchronised).
    void sync_all() {
        if (!lease_) return;
        if (inflight_) { (void)hipStreamSynchronize(stream_); inflight_ = false; }
        for (hipStream_t s : {side_.lean, side_.full, side_.scan, lease_->copy_stream, lease_->run_stream}) if (s) (void)hipStreamSynchronize(s);
        for (const Request& R : req_) if (R.queued && R.stream != stream_) (void)hipStreamSynchronize(R.stream);   // (a profile queued on another stream than the run's)
        if (seq_busy_ && seq_stream_ != stream_) (void)hipStreamSynchronize(seq_stream_);          // (and a sequence request)
        seq_busy_ = false;
        requests_reset();
        (void)hipGetLastError();
    }
    // guard words around the pinned words the kernels write through (always) and around the path areas of the direct
    // full-finish launch (AMBI_DEBUG); called with every stream idle
    int check_guards(const char* when) {
        if (!lease_) return 0;
        int bad = 0;
        for (int i = 0; i < 16; i++) bad += (lease_->h_words->guard_lo[i] != kGuardWord) + (lease_->h_words->guard_hi[i] != kGuardWord);
        if (bad) fprintf(stderr, "ambigram_hip: GUARD: %d guard words around the pinned status words overwritten (%s)\n", bad, when);
        if (debug_ && d_direct_cells_ && d_guard_bad_ && direct_slots_ > 0) {
            int32_t n = 0;
            hipLaunchKernelGGL(ambi_guard_check_kernel, dim3(direct_slots_), dim3(32), 0, nullptr, (const uint8_t*)d_direct_cells_, direct_stride_, direct_slots_, d_guard_bad_);
            if (hipMemcpy(&n, d_guard_bad_, sizeof(n), hipMemcpyDeviceToHost) == hipSuccess && n) {
                fprintf(stderr, "ambigram_hip: GUARD: %d guard words around the path areas of the direct full-finish launch overwritten (%s)\n", n, when);
                bad += n;
                (void)hipMemset(d_guard_bad_, 0, sizeof(int32_t));
            }
        }
        return bad;
    }
    void free_all() {
        DeviceGuard dg_(device_);
        sync_all();
        (void)check_guards("release");
        // per-batch allocations outside the lease's blocks (--all bitmaps, stage profile)
        void* ptrs[] = {d_all_bits_, d_all_off_, d_all_count_, d_stage_clk_};
        for (void* p : ptrs) if (p) (void)hipFree(p);
        d_all_bits_ = nullptr; d_all_off_ = nullptr; d_all_count_ = nullptr; d_all_flags_ = nullptr; d_stage_clk_ = nullptr; all_bits_cap_ = 0;
        d_units_ = nullptr; d_results_ = nullptr; d_arena_ = nullptr; d_direct_cells_ = nullptr; direct_n_ = 0;
        if (lease_) {
            Lease* L = lease_;
            // what a large batch grew goes back to the device; small blocks stay with the lease for the next batch
            if (L->d_block_bytes > kKeepBlock) { (void)hipFree(L->d_block); L->d_block = nullptr; L->d_block_bytes = 0; }
            if (L->d_arena_bytes > kKeepArena) { (void)hipFree(L->d_arena); L->d_arena = nullptr; L->d_arena_bytes = 0; }
            if (L->d_cells_bytes > kKeepCells) { (void)hipFree(L->d_cells); L->d_cells = nullptr; L->d_cells_bytes = 0; }
            if (L->h_stage_bytes > kKeepStage) { (void)hipHostFree(L->h_stage); L->h_stage = nullptr; L->dh_stage = nullptr; L->h_stage_bytes = 0; }
            if (L->h_mail_bytes > kKeepMail) { (void)hipHostFree(L->h_mail); L->h_mail = nullptr; L->dh_mail = nullptr; L->h_mail_bytes = 0; }
            for (int k = 0; k < 2; k++) {
                if (L->d_runs_bytes[k] > kKeepRuns) { (void)hipFree(L->d_runs[k]); L->d_runs[k] = nullptr; L->d_runs_bytes[k] = 0; }
                if (L->h_runs_bytes[k] > kKeepRuns) { (void)hipHostFree(L->h_runs[k]); L->h_runs[k] = nullptr; L->h_runs_bytes[k] = 0; }
            }
            for (int k = 0; k < kProfileKinds; k++) L->prof[k].trim(kKeepProfile, k == kAlign ? kKeepProfile : kKeepCells);   // (side areas: depth and planes as the path areas)
            for (DeviceImage& I : L->img) { I.version = -1; I.trim(kKeepProfile); }
            for (auto pb : {std::make_pair(&L->d_seq_img, &L->d_seq_img_bytes), std::make_pair(&L->d_seq_work, &L->d_seq_work_bytes), std::make_pair(&L->d_seq_out, &L->d_seq_out_bytes)})
                if (*pb.second > kKeepSeq) { (void)hipFree(*pb.first); *pb.first = nullptr; *pb.second = 0; }
            if (L->h_seq_bytes > kKeepSeq) { (void)hipHostFree(L->h_seq); L->h_seq = nullptr; L->h_seq_bytes = 0; }
            lease_ = nullptr;
            DevicePool::get().release(L);
        }
        stage_big_.clear(); stage_big_.shrink_to_fit();
        mail_valid_ = false;
        requests_reset();
        sequence_reset(); seq_img_version_ = -1; seq_busy_ = false;
        device_ = -1;
    }

    // Layout of the device block: [inputs, in the order of the staging image] [zero-filled: result blob, image headers, flags,
    // counters] [working set].  pass 0 measures, pass 1 assigns the pointers.
    struct Carver {
        uint8_t* base; int64_t off = 0;
        template <class T> void take(T** p, size_t count) {
            if (base) *p = reinterpret_cast<T*>(base + off);
            off = (off + (int64_t)((count ? count : 1) * sizeof(T)) + 255) & ~int64_t(255);
        }
    };
    int64_t layout(uint8_t* base, const std::vector<int32_t>& direct_list) {
        const HostBatch& H = hb();
        const size_t U = H.units.size();
        Carver c{base};
        c.take(&d_units_, U); c.take(&d_seg_cn_, H.seg_cn.size()); c.take(&d_junc_cn_, H.junc_cn.size()); c.take(&d_junc_ends_, H.junc_ends.size());
        c.take(&d_elems_, H.elems.size()); c.take(&d_scratch_off_, U); c.take(&d_direct_list_, direct_list.size()); c.take(&d_mail_off_, U);
        c.take(&d_wide_index_, U); c.take(&d_wide_units_, (size_t)H.n_wide);
        c.take(&d_inject_, H.inject.size()); c.take(&d_inject_off_, H.inject.empty() ? 0 : kInjectStride * U);
        c.take(&d_run_slot_, U + 1);
        in_bytes_ = c.off;
        zero_off_ = c.off;
        c.take(&d_results_, (size_t)H.result_bytes); c.take(&d_blk_hdr_, U * 8); c.take(&d_fallback_, U);
        c.take(&d_refin_count_, 2); c.take(&d_blocks_done_, 1); c.take(&d_npending_, 1); c.take(&d_guard_bad_, 1); c.take(&d_lat_sum_, 2);
        zero_bytes_ = c.off - zero_off_;
        c.take(&d_dags_, U);
        c.take(&d_ikeys_, (size_t)H.ideal_slots); c.take(&d_icnt_, (size_t)H.ideal_slots); c.take(&d_ilink_, (size_t)H.ideal_slots * 4 + 8);
        c.take(&d_ilvl_off_, U * (kMaxNodes + 3)); c.take(&d_icounter_, 2 * U); c.take(&d_ipos_, (size_t)H.ideal_slots);
        c.take(&d_aavail_, (size_t)H.ideal_slots / 2 + 1); c.take(&d_acnt_, (size_t)H.ideal_slots / 2 + 1); c.take(&d_acbase_, (size_t)H.ideal_slots / 2 + U + 1);
        c.take(&d_achild_, (size_t)H.ideal_slots * 4 + 8); c.take(&d_anblk_, (size_t)H.ideal_slots / 2 + 1); c.take(&d_adepth_, (size_t)H.ideal_slots / 2 + 8);
        c.take(&d_edit_list_, direct_list.size()); c.take(&d_blk_off_, U + 1); c.take(&d_rows_, U); c.take(&d_needed_, 1); c.take(&d_lat_R_, U); c.take(&d_lat_status_, U);
        c.take(&d_scratch_, (size_t)H.scratch_ints + 8); c.take(&d_pack_off_, U + 1); c.take(&d_refin_list_, U);
        c.take(&d_first_rows_, U * (size_t)(cfg_.first_budget > 0 ? cfg_.first_budget : 1) * kFirstRowStride);
        const size_t img_stride = (size_t)std::max(block_lds_, ((160 * 1024) / 3) & ~15);   // (the budget per workgroup may be re-chosen after the first run)
        c.take(&d_blk_img_, U * img_stride);
        c.take(&d_wide_, (size_t)H.n_wide);
        run_total_ = H.run_slot.empty() ? 0 : H.run_slot.back();
        for (int k = 0; k < 2; k++) c.take(&d_run_blk_[k], 2 * U + 2 * (size_t)run_total_);
        return c.off;
    }

  public:
    ~HipBackend() override { free_all(); }
    const char* name() const override { return "hip"; }
    int device_count(int* n) override {
        int c = 0;
        hipError_t e = hipGetDeviceCount(&c);
        if (e != hipSuccess) c = 0;
        if (n) *n = c;
        return 0;
    }
    int set_device(int d) override { HIP_CK(hipSetDevice(d)); return 0; }

    template <class T> int dalloc(T** p, size_t count) {
        HIP_CK(hipMalloc((void**)p, (count ? count : 1) * sizeof(T)));
        return 0;
    }

    int upload(const HostBatch& hb_in, const EngineConfig& cfg) override {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return -30;   // AMBI_ERR_NO_DEVICE: no CPU fallback
        if (uploaded_) { free_all(); uploaded_ = false; }   // a second upload replaces the first (every stream idle first)
        ran_ = false; general_path_ = -1; timed_runs_ = 0; tuned_ = false; late_refusal_ = false; last_needed_ = 0;
        requests_reset();
        sequence_reset(); seq_img_version_ = -1; seq_busy_ = false;
        express_ = false;
        shared_units_ = -1;
        hbp_ = &hb_in; cfg_ = cfg;
        const HostBatch& H = hb();
        const size_t U = H.units.size();
        int rc;
        debug_ = ambi_env("AMBI_DEBUG") != nullptr;
        if ((rc = DevicePool::get().acquire(&lease_))) return rc;
        Lease* L = lease_;
        device_ = L->device;
        side_ = SideStreams{}; side_for_ = (hipStream_t)-1;   // (chosen by the first run)
        h_npending_ = &L->h_words->npending; h_needed_ = L->h_words->needed;
        dh_npending_ = &L->dh_words->npending; dh_needed_ = L->dh_words->needed;
        h_express_left_ = &L->h_words->express_left; dh_express_left_ = &L->dh_words->express_left;
        L->h_words->npending = 0; L->h_words->express_left = 1; L->h_words->late_flag = 0;
        ev_fork_ = L->ev_fork; ev_prep_ = L->ev_prep; ev_back_ = L->ev_back; ev_first_ = L->ev_first; ev_full_ = L->ev_full; ev_plan_ = L->ev_plan; ev_express_ = L->ev_express;
        if (ambi_env("AMBI_STAGE_PROFILE")) { if ((rc = dalloc(&d_stage_clk_, U * kStageSlots))) return rc; HIP_CK(hipMemset(d_stage_clk_, 0, U * kStageSlots * sizeof(int64_t))); }
        { const char* e9 = ambi_env("AMBI_ORDER_ALIGN"); order_align_ = e9 ? atoi(e9) : 4096; if (order_align_ < 16 || (order_align_ & (order_align_ - 1))) order_align_ = 4096; }
        // LDS budgets (dynamic shared memory), sized for the largest unit of the batch
        lds_prepare_ = (int)prepare_work_bytes(H.max_n, H.max_m, H.max_k);
        n_wide_ = H.n_wide;
        lds_first_ = (int)first_work_bytes(H.max_n, H.max_bkp, n_wide_ > 0);
        // the full finish stage keeps the path cells in LDS: as many as fit beside its other arrays (longer paths are
        // served by the lean stage alone)
        finish_path_cells_ = H.max_path < kPathLdsCells ? H.max_path : kPathLdsCells;
        while (finish_path_cells_ > 4096 && finish_work_bytes(H.max_n, H.max_m, H.max_bkp, finish_path_cells_, H.max_out) > 160 * 1024 - 1024)
            finish_path_cells_ -= 2048;
        lds_finish_ = (int)finish_work_bytes(H.max_n, H.max_m, H.max_bkp, finish_path_cells_, H.max_out);
        lds_finish_lean_ = (int)finish_lean_work_bytes(H.max_n, H.max_m, H.max_bkp);
        { const char* e = ambi_env("AMBI_LEAN_FINISH"); lean_finish_ = e ? atoi(e) != 0 : true; }
        { const char* e = ambi_env("AMBI_FINISH_GRID"); finish_grid_ = e ? atoi(e) : 0; if (finish_grid_ < 0) finish_grid_ = 0; }
        {   // the general enumerate kernel serves ordinary units only (wide ones have their own table kernel): its per-lane stacks are
            // sized by the largest ORDINARY unit -- with the wide units' node count they outgrew a CU's group memory at 255 nodes
            int mk = 1;
            for (const UnitIn& un : H.units) if (un.n_elem <= kMaxNodes && un.n_elem > mk) mk = un.n_elem;
            enum_stack_lds_ = (int)enum_stack_bytes(mk);
        }
        lds_enum_ = 4 * (enum_stack_lds_ + enum_auto_lds_);
        { const BlockLimits bl = block_limits(cfg.block_max, cfg.block_lds); block_max_ = bl.block_max; block_lds_ = bl.block_lds; }
        lds_blocks_ = block_lds_;
        const int kLdsLimit = 160 * 1024 - 1024;
        emit_lds_auto_ = !ambi_env("AMBI_BLOCK_LDS");
        { const char* e = ambi_env("AMBI_EMIT_LDS_TIGHT"); emit_lds_tight_ = e ? atoi(e) != 0 : true; }
        { const char* env = ambi_env("AMBI_BLOCK_SCRATCH_LDS"); block_scratch_lds_ = ((env ? atoi(env) : cfg.block_scratch_lds) + 15) & ~15; }
        if (block_scratch_lds_ > kLdsLimit) block_scratch_lds_ = kLdsLimit & ~15;
        lds_build_ = block_scratch_lds_;   // the image itself is assembled in HBM
        if (lds_prepare_ > kLdsLimit || lds_first_ > kLdsLimit || lds_finish_ > kLdsLimit || lds_enum_ > kLdsLimit || lds_blocks_ > kLdsLimit) {
            fprintf(stderr, "ambigram_hip: a unit needs more LDS than one CU has (prepare %d, first %d, finish %d, general enumerate %d, block emission %d bytes)\n",
                    lds_prepare_, lds_first_, lds_finish_, lds_enum_, lds_blocks_);
            return ST_ERR_BAD_INPUT;
        }
        {   // the dynamic-LDS ceiling of every kernel: a per-function, process-wide attribute, set once per device
            hipError_t err = hipSuccess;
            std::lock_guard<std::mutex> lk(L->ctx->mu);
            if (!L->ctx->lds_ceiling) {
                const void* fns[] = {(const void*)ambi_blocks_build_kernel, (const void*)ambi_prepare_kernel, (const void*)ambi_first_kernel, (const void*)ambi_resolve_kernel,
                                     (const void*)ambi_finish_kernel, (const void*)ambi_finish_ext_kernel, (const void*)ambi_finish_edit_kernel, (const void*)ambi_finish_lean_kernel,
                                     (const void*)ambi_enumerate_kernel<0>, (const void*)ambi_enumerate_kernel<1>, (const void*)ambi_enumerate_kernel<2>,
                                     (const void*)ambi_enumerate_blocks_kernel<0>, (const void*)ambi_enumerate_blocks_kernel<1>, (const void*)ambi_enumerate_blocks_kernel<2>,
                                     (const void*)ambi_express_kernel, (const void*)ambi_lattice_kernel, (const void*)ambi_lattice_own_kernel, (const void*)ambi_search_kernel, (const void*)ambi_all_kernel,
                                     (const void*)ambi_all_lanes_kernel, (const void*)ambi_order_paths_kernel};
                for (const void* f : fns) { hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMaxDynamic); if (e != hipSuccess) err = e; }
                L->ctx->lds_ceiling = err == hipSuccess;   // (a failed attempt is tried again by the next upload)
            }
            HIP_CK(err);
        }
        enum_classes_ = 0;
        for (const UnitIn& un : H.units) if (un.n_elem > 0) enum_classes_ |= 1 << enum_class_of(un.n_elem);
        avg_path_ = 0;
        for (const UnitIn& un : H.units) avg_path_ += un.path_cap;
        avg_path_ /= (double)(U > 0 ? U : 1);
        { const char* e3 = ambi_env("AMBI_ENUM_GRID"); enum_grid_ = e3 ? atoi(e3) : 16384; if (enum_grid_ < 1) enum_grid_ = 1; }   // >= work blocks: one block per workgroup, the rest exit (measured: 2048 -> 16384 workgroups = -8 % kernel time)
        { const char* e9 = ambi_env("AMBI_BUILD_IN_EMIT"); build_in_emit_ = e9 ? (atoi(e9) != 0) : 1; }
        { const char* e9 = ambi_env("AMBI_BLOCK_DFS"); block_dfs_ = e9 ? (atoi(e9) != 0) : 1; }
        { const char* e9 = ambi_env("AMBI_EMIT_INTERLEAVE"); emit_interleave_ = e9 ? (atoi(e9) != 0) : 1; }
        { const char* e5 = ambi_env("AMBI_OVERLAP_BACK"); want_overlap_ = e5 ? atoi(e5) != 0 : true; }
        direct_n_ = 0; d_direct_cells_ = nullptr; direct_slots_ = 0;
        std::vector<int32_t> dl;
        if (want_overlap_) {
            // (direct full-stage launch: 512 threads with the path cells in device memory, 1024 with the cells in group memory --
            // measured, four interleaved runs: cells in group memory 1.151 ms per step; in device memory 256 / 512 / 1024
            // threads = 1.133 / 1.110 / 1.200)
            { const char* ee = ambi_env("AMBI_DIRECT_EXT"); direct_ext_ = ee ? atoi(ee) != 0 : true; }
            { const char* e = ambi_env("AMBI_FULL_THREADS"); full_threads_ = e ? atoi(e) : (direct_ext_ ? 512 : 1024); if (full_threads_ != 256 && full_threads_ != 512 && full_threads_ != 1024) full_threads_ = direct_ext_ ? 512 : 1024; }
            {   // units that go straight to the full finish stage (env AMBI_DIRECT_FULL=0: none, they pass through the lean stage first)
                const char* e7 = ambi_env("AMBI_DIRECT_FULL"); const bool on = e7 ? atoi(e7) != 0 : true;
                const char* e8 = ambi_env("AMBI_DIRECT_GRID"); direct_grid_ = e8 ? atoi(e8) : 1024; if (direct_grid_ < 1) direct_grid_ = 1;   // one workgroup per unit up to 1024 (measured: 64 / 128 / 256 / 512 workgroups for 512 units = 1.63 / 1.37 / 1.25 / 1.23 ms per step; without this launch 1.30)
                if (on && lean_finish_) for (size_t u2 = 0; u2 < U; u2++) if (H.units[u2].direct_full) dl.push_back((int32_t)u2);
                direct_n_ = (int)dl.size();
                if (direct_n_ > 0) {
                    if (direct_ext_) lds_finish_ext_ = (int)finish_work_bytes(H.max_n, H.max_m, H.max_bkp, 0, H.max_out);
                    { const char* ed = ambi_env("AMBI_DIRECT_EDIT"); direct_edit_ = (ed ? atoi(ed) != 0 : true) && direct_ext_; }
                    { const char* eg = ambi_env("AMBI_EDIT_GRID"); edit_grid_ = eg ? atoi(eg) : 1024; if (edit_grid_ < 1) edit_grid_ = 1; }
                    lds_finish_edit_ = (int)finish_edit_work_bytes(H.max_n, H.max_m, H.max_bkp);
                    if (lds_finish_edit_ > kLdsLimit) direct_edit_ = false;
                }
            }
        }
        {   // express path: small batches only, and only if a unit's whole working set fits one workgroup's group memory
            const char* e9 = ambi_env("AMBI_EXPRESS_UNITS"); express_units_ = e9 ? atoi(e9) : 32;
            lds_express_ = (int)express_work_bytes(H.max_n, H.max_m, H.max_k, H.max_bkp, finish_path_cells_, H.max_out) + 64;
            lds_lattice_ = (int)(64 * 8 + kPrepLatticeBytes + 64);
            lds_lattice_own_ = (int)lattice_own_bytes(H.max_k) + 64;
            side_lattice_ = (int)U <= express_units_;
        }
        // result mailbox in pinned host memory: batches that can take the express path, while the slots stay small
        mail_off_.assign(U, 0); mail_bytes_ = 0; mail_on_ = false; mail_valid_ = false;
        if ((int)U <= express_units_) {
            for (size_t u2 = 0; u2 < U; u2++) { mail_off_[u2] = mail_bytes_; mail_bytes_ += mail_layout(H.units[u2].path_cap, H.units[u2].out_cap).total; }
            mail_on_ = mail_bytes_ <= kKeepMail;
            if (mail_on_ && (rc = lease_pinned_block(&L->h_mail, &L->dh_mail, &L->h_mail_bytes, mail_bytes_))) return rc;
        }
        // ---- the device block and the input image ----
        const int64_t total = layout(nullptr, dl);
        if ((rc = lease_device_block(&L->d_block, &L->d_block_bytes, total))) return rc;
        (void)layout(L->d_block, dl);
        if (H.inject.empty()) { d_inject_ = nullptr; d_inject_off_ = nullptr; }
        if (dl.empty()) d_direct_list_ = nullptr;
        if (direct_n_ > 0 && direct_ext_) {   // one path area per workgroup of the direct launch, guard words on both sides of each
            direct_stride_ = ((2ll * H.max_path + 16 + 15) & ~int64_t(15)) + 2 * kCellGuardBytes;
            direct_slots_ = direct_n_ < direct_grid_ ? direct_n_ : direct_grid_;
            if ((rc = lease_device_block(&L->d_cells, &L->d_cells_bytes, direct_stride_ * direct_slots_))) return rc;
            d_direct_cells_ = L->d_cells;
        }
        arena_bytes_ = cfg.order_arena_bytes > 0 ? cfg.order_arena_bytes : (int64_t)1 << 20;
        { const char* cap = ambi_env("AMBI_ARENA_MAX_BYTES"); const bool capped = cap && atoll(cap) > 0;
          // a configured size or a memory budget is taken literally; otherwise whatever the lease already holds is used
          if (cfg.order_arena_bytes <= 0 && !capped && L->d_arena_bytes > arena_bytes_) arena_bytes_ = L->d_arena_bytes;
          if (capped && arena_bytes_ > atoll(cap)) arena_bytes_ = atoll(cap); }
        if ((rc = lease_device_block(&L->d_arena, &L->d_arena_bytes, arena_bytes_))) return rc;
        d_arena_ = L->d_arena;
        // input image: same layout as the front of the device block; pinned staging (one asynchronous copy, queued by the
        // first run ahead of its kernels) or, for large batches, a plain buffer copied at once
        uint8_t* img;
        const bool pinned = in_bytes_ <= kKeepStage;
        if (pinned) { if ((rc = lease_pinned_block(&L->h_stage, &L->dh_stage, &L->h_stage_bytes, in_bytes_))) return rc; img = L->h_stage; }
        else { stage_big_.assign((size_t)in_bytes_, 0); img = stage_big_.data(); }
        auto put = [&](const void* dptr, const void* src, size_t bytes) { if (bytes) memcpy(img + (reinterpret_cast<const uint8_t*>(dptr) - L->d_block), src, bytes); };
        put(d_units_, H.units.data(), U * sizeof(UnitIn));
        put(d_seg_cn_, H.seg_cn.data(), H.seg_cn.size() * sizeof(double));
        put(d_junc_cn_, H.junc_cn.data(), H.junc_cn.size() * sizeof(double));
        put(d_junc_ends_, H.junc_ends.data(), H.junc_ends.size() * sizeof(JuncEnds));
        put(d_elems_, H.elems.data(), H.elems.size() * sizeof(Element));
        put(d_scratch_off_, H.scratch_off.data(), U * sizeof(int64_t));
        if (!dl.empty()) put(d_direct_list_, dl.data(), dl.size() * sizeof(int32_t));
        put(d_mail_off_, mail_off_.data(), U * sizeof(int64_t));
        put(d_run_slot_, H.run_slot.data(), (U + 1) * sizeof(int64_t));
        put(d_wide_index_, H.wide_index.data(), U * sizeof(int32_t));
        {
            std::vector<int32_t> wu;
            for (size_t u2 = 0; u2 < U; u2++) if (H.wide_index[u2] >= 0) wu.push_back((int32_t)u2);
            if (!wu.empty()) put(d_wide_units_, wu.data(), wu.size() * sizeof(int32_t));
        }
        if (!H.inject.empty()) { put(d_inject_, H.inject.data(), H.inject.size()); put(d_inject_off_, H.inject_off.data(), kInjectStride * U * sizeof(int64_t)); }
        if (pinned) upload_pending_ = true;
        else {
            HIP_CK(hipMemcpy(L->d_block, img, (size_t)in_bytes_, hipMemcpyHostToDevice));
            HIP_CK(hipMemset(L->d_block + zero_off_, 0, (size_t)zero_bytes_));
            if (d_direct_cells_) { hipLaunchKernelGGL(ambi_guard_fill_kernel, dim3(direct_slots_), dim3(32), 0, nullptr, d_direct_cells_, direct_stride_, direct_slots_); HIP_CK(hipDeviceSynchronize()); }
            stage_big_.clear(); stage_big_.shrink_to_fit();
            upload_pending_ = false;
        }
        uploaded_ = true; arena_checked_ = false;
        return 0;
    }
    // the input image and the zero fill of a freshly uploaded batch, queued on the caller's stream ahead of the first kernels
    int flush_upload(hipStream_t st) {
        if (!upload_pending_) return 0;
        Lease* L = lease_;
        if (in_bytes_ + zero_bytes_ <= (8ll << 20) && L->dh_stage && !ambi_env("AMBI_NO_INGEST")) {   // (every part of the block is 256-byte aligned)
            const int64_t n16 = in_bytes_ / 16, z16 = zero_bytes_ / 16;
            int64_t blocks = (std::max(n16, z16) + 255) / 256;
            if (blocks > 1024) blocks = 1024;
            hipLaunchKernelGGL(ambi_ingest_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const uint4*)L->dh_stage, (uint4*)L->d_block, n16,
                               (uint4*)(L->d_block + zero_off_), z16);
        } else {
            HIP_CK(hipMemcpyAsync(L->d_block, L->h_stage, (size_t)in_bytes_, hipMemcpyHostToDevice, st));
            HIP_CK(hipMemsetAsync(L->d_block + zero_off_, 0, (size_t)zero_bytes_, st));
        }
        if (d_direct_cells_) hipLaunchKernelGGL(ambi_guard_fill_kernel, dim3(direct_slots_), dim3(32), 0, st, d_direct_cells_, direct_stride_, direct_slots_);
        upload_pending_ = false;
        return 0;
    }

    // whole-batch argument block (pack kernels, slow path); args() adds what a run's kernels take on top
    void bind(uint32_t flags) {
        A_.n_units = (int32_t)hb().units.size(); A_.unit_base = 0; A_.arena_base = 0;
        A_.flags = flags; A_.first_budget = cfg_.first_budget; A_.target_lanes = cfg_.target_lanes;
        A_.enum_stack_lds = enum_stack_lds_; A_.enum_auto_lds = enum_auto_lds_;
        A_.block_lds = block_lds_; A_.block_scratch_lds = block_scratch_lds_; A_.block_max = block_max_; A_.build_in_emit = build_in_emit_; A_.emit_interleave = emit_interleave_; A_.order_align = order_align_; A_.block_dfs = block_dfs_; A_.finish_path_cells = finish_path_cells_; A_.unit_fallback = d_fallback_; A_.block_img = d_blk_img_; A_.block_hdr = d_blk_hdr_;
        A_.ideal_pos = d_ipos_; A_.auto_avail = d_aavail_; A_.auto_cnt = d_acnt_; A_.auto_cbase = d_acbase_; A_.auto_child = d_achild_; A_.auto_nblk = d_anblk_; A_.auto_depth = d_adepth_;
        A_.units = d_units_; A_.seg_cn = d_seg_cn_; A_.junc_cn = d_junc_cn_; A_.junc_ends = d_junc_ends_; A_.elems = d_elems_;
        A_.dags = d_dags_; A_.results = d_results_;
        A_.ideal_keys = d_ikeys_; A_.ideal_cnt = d_icnt_; A_.ideal_link = d_ilink_; A_.ideal_lvl_off = d_ilvl_off_; A_.ideal_counter = d_icounter_;
        A_.first_rows = d_first_rows_;
        A_.order_arena = d_arena_; A_.order_arena_bytes = arena_bytes_;
        A_.blk_off = d_blk_off_; A_.rows_per_lane = d_rows_; A_.n_pending = d_npending_; A_.orders_needed = d_needed_;
        A_.scratch_i32 = d_scratch_; A_.scratch_off = d_scratch_off_; A_.stage_clk = d_stage_clk_;
        A_.zero_pending = 0; A_.host_pending = nullptr; A_.host_needed = nullptr; A_.blocks_done = d_blocks_done_;
        A_.inject_valid = d_inject_; A_.inject_off = d_inject_off_; A_.refin_list = d_refin_list_; A_.refin_count = d_refin_count_; A_.direct_full_on = 0; A_.finish_retry = 0;
        { const char* ec = ambi_env("AMBI_EDIT_RUN_CAP"); A_.edit_cap_limit = ec ? atoi(ec) : 0; }
        A_.wide = n_wide_ > 0 ? d_wide_ : nullptr; A_.wide_index = n_wide_ > 0 ? d_wide_index_ : nullptr;
        A_.mail = mail_on_ ? lease_->dh_mail : nullptr; A_.mail_off = d_mail_off_;
        {   // the finish stages leave the final paths in run-length form in the block of this run's parity (the other one may still be on its way to the host)
            const int64_t U = (int64_t)hb().units.size();
            int32_t* blk = d_run_blk_[run_seq_ & 1];
            A_.run_cnt = blk; A_.run_cells = blk + U; A_.run_start = blk + 2 * U; A_.run_len = blk + 2 * U + run_total_; A_.run_slot = d_run_slot_;
        }
        A_.lat_R = d_lat_R_; A_.lat_status = d_lat_status_; A_.lat_sum = d_lat_sum_; A_.lat_seq = &lease_->dh_words->lat_seq; A_.lat_unsure = &lease_->dh_words->lat_unsure;
        A_.plan_seq = &lease_->dh_words->plan_seq; A_.late_flag = &lease_->dh_words->late_flag; A_.run_seq = run_seq_;
        A_.all_bits = d_all_bits_; A_.all_off = d_all_off_; A_.all_count = d_all_count_; A_.all_flags = d_all_flags_; A_.all_rank = all_rank_; A_.all_world = all_world_; { const char* e = ambi_env("AMBI_ALL_TABLE"); A_.all_rows_from_table = (e && atoi(e) != 0) ? 1 : 0; }
    }
    // the order arena as the tables use it: whole alignment units
    int64_t arena_usable() const { return arena_bytes_ & ~int64_t(order_align_ - 1); }
    BatchArgs args() const {   // the argument block of a run's kernels
        BatchArgs A = A_;
        A.order_arena_bytes = arena_usable();
        A.target_lanes = cfg_.target_lanes > 0 ? cfg_.target_lanes : 1;
        return A;
    }

    // Per-kernel HIP events on the caller's stream (or `on`).  A ring of kTimingSlots event sets lets a timed region of many
    // runs be averaged without a host sync per run: run r records into slot r % kTimingSlots.
    static constexpr int kTimingSlots = 64, kTimedKernels = 7;
    void tick(const char* name, size_t idx, bool begin, hipStream_t on = (hipStream_t)-1) {
        if (!timing_ || !((timing_mask_ >> idx) & 1u)) return;
        const size_t slot = (size_t)(timed_runs_ % kTimingSlots);
        const size_t at = slot * kTimedKernels + idx;
        while (evs().size() <= at) {
            Ev e{name, nullptr, nullptr};
            (void)hipEventCreate(&e.a); (void)hipEventCreate(&e.b);
            evs().push_back(e);
        }
        evs()[at].name = name;
        (void)hipEventRecord(begin ? evs()[at].a : evs()[at].b, on == (hipStream_t)-1 ? stream_ : on);
    }

    void launch_front(const BatchArgs& A) {   // prepare + plan
        hipStream_t st = stream_;
        first_launched_ = false;
        if (express_) {
            // express kernel (whole reconstruction of the units whose first order assembles; results complete at ev_express_),
            // then the lattice stage of every unit; the express kernel hands units over by status, not through the list
            BatchArgs Ax = A;
            Ax.refin_list = nullptr;
            Ax.express_left = dh_express_left_;
            Ax.express_seq = dh_express_left_ + 1;
            Ax.run_seq = run_seq_;
            h_express_left_[0] = 0;
            // the lattice kernel starts beside the express kernel: behind the input image of a fresh batch, else behind the END of the
            // previous run (an event recorded then: no marker in front of the express kernel now)
            const bool side = side_lattice_ && !lazy_;
            if (side) {
                lease_->h_words->lat_unsure = 0;
                if (flushed_) (void)hipEventRecord(ev_fork_, st);
                (void)hipStreamWaitEvent(side_.scan, flushed_ ? ev_fork_ : lease_->ev_tail, 0);
            }
            tick("ambi_express_kernel", 0, true);
            hipLaunchKernelGGL(ambi_express_kernel, dim3(A.n_units), dim3(kExpressThreads), lds_express_, st, Ax);
            tick("ambi_express_kernel", 0, false);
            (void)hipEventRecord(ev_express_, st);
            tick("ambi_plan_kernel", 1, true);
            if (side) {   // the lattice beside the express kernel, on a stream of its own; the plan kernel behind both
                hipLaunchKernelGGL(ambi_lattice_own_kernel, dim3(A.n_units), dim3(64), lds_lattice_own_, side_.scan, A);
                (void)hipEventRecord(lease_->ev_lat, side_.scan);
                (void)hipStreamWaitEvent(st, lease_->ev_lat, 0);
            } else
            hipLaunchKernelGGL(ambi_lattice_kernel, dim3(A.n_units), dim3(64), lds_lattice_, st, A);
        } else {
            tick("ambi_prepare_kernel", 0, true);
            hipLaunchKernelGGL(ambi_prepare_kernel, dim3(A.n_units), dim3(64), lds_prepare_, st, A);
            tick("ambi_prepare_kernel", 0, false);
            // The scan for the first valid order reads what the prepare stage left (first rows, DAG) and rewrites the status;
            // the plan stage reads and writes UnitOut::order_off only.  With overlap the scan therefore starts HERE, beside the
            // plan kernel (one workgroup, 25 us during which the chip is otherwise idle) and the ramp of the enumerate kernel,
            // instead of queueing behind 4096 enumerate workgroups for group memory.
            if (overlap_back_) {
                (void)hipEventRecord(ev_prep_, st);
                (void)hipStreamWaitEvent(side_.scan, ev_prep_, 0);
                tick("ambi_first_kernel", 4, true, side_.scan);
                hipLaunchKernelGGL(ambi_first_kernel, dim3(A.n_units), dim3(64), lds_first_, side_.scan, A);
                tick("ambi_first_kernel", 4, false, side_.scan);
                (void)hipEventRecord(ev_first_, side_.scan);
                first_launched_ = true;
            }
            tick("ambi_plan_kernel", 1, true);
        }
        if (lazy_) {}   // no tables in this run: nothing to plan
        else if (express_ && side_lattice_) hipLaunchKernelGGL(ambi_plan_kernel, dim3(1), dim3(1024), 0, st, A);
        else { BatchArgs Ap = A; Ap.lat_R = nullptr; hipLaunchKernelGGL(ambi_plan_kernel, dim3(1), dim3(1024), 0, st, Ap); }
        tick("ambi_plan_kernel", 1, false);
        // (express chain: the lattice kernel reads the status, so the scan of the units the express kernel left stays behind
        // the plan kernel there)
        if (overlap_back_) (void)hipEventRecord(first_launched_ ? ev_plan_ : ev_prep_, st);
    }
    void launch_build(const BatchArgs& A) {   // block-emission images
        tick("ambi_blocks_build_kernel", 2, true);
        hipLaunchKernelGGL(ambi_blocks_build_kernel, dim3(A.n_units), dim3(256), lds_build_, stream_, A);
        tick("ambi_blocks_build_kernel", 2, false);
    }
    // Workgroups of the lean finish kernel.  Beside a long enumerate kernel the finish stage only has to be done when the
    // table is: the fewer of its workgroups are resident, the less they take from the enumerate workgroups (issue slots,
    // group-memory bandwidth), so the grid is sized to finish in time with a margin: too few workgroups and the finish
    // kernel becomes the tail of the step (a steep loss), too many cost a little (measured on one MI355X,
    // profiles/r01_slices.md: 112 / 128 / 144 / 160 / 176 / 256 / 4096 workgroups for the 4096 units of the bench workload
    // = 1.25 / 1.17 / 1.125 / 1.126 / 1.13 / 1.14 / 1.39 ms per step).  Without a long enumerate kernel (small order
    // tables, first run) every unit gets its own workgroup.
    int finish_grid_for(int U) const {
        if (finish_grid_ > 0) return U < finish_grid_ ? U : finish_grid_;          // env AMBI_FINISH_GRID
        if (!overlap_back_ || lazy_) return U;   // (no order table being written: nothing to hide behind, every unit its own workgroup)
        // order-table bytes of the previous run at the rate the enumerate kernel reaches: an optimistic 5.2 TB/s for rows of a byte
        // per node; packed rows of up to 32 nodes leave slower -- fewer bytes per row for the same work per row
        // (measured on the bench batch, 12-byte rows of 5 bits per node: 160 / 176 / 192 / 208 / 240 / 272 workgroups = 0.92-0.93 / 0.916-0.938 /
        // 0.903-0.919 / 0.914-0.933 / 0.93-0.94 / 0.95 ms per step with the 16-byte-group emission; with one row per lane the
        // table is done earlier and the finish kernels want more room: 192 / 208 / 224 / 256 / 288 = 0.887 / 0.864 / 0.857 / 0.876 /
        // 0.885 (means of 3-6 runs, the build before: 0.867); this rule gives 210 -> 224).  Lehmer rows (8 bytes at K = 19 instead of
        // 12) carry the same work per row in two thirds of the bytes: 224 / 288 / 352 / 416 workgroups = 0.709-0.710 / 0.657-0.670 /
        // 0.635-0.653 / 0.684-0.685 ms per step, two runs each on one box; at 4.1e6 the rule gave 400 (0.666-0.713), at 3.6e6 it gives 352
        // (profiles/r05_notes.md)
        const double enum_us = (double)last_needed_ / ((enum_classes_ & 3) ? 3.6e6 : 5.2e6);
        const double unit_us = 4.0 + avg_path_ / 900.0 + hb().max_m / 64.0;          // one unit through the lean finish stage (mean path capacity of the batch)
        if (enum_us < 8.0 * unit_us) return U;
        // (measured with the SV-carrying bench batch, 40 KB images: 160 / 192 / 256 / 320 workgroups = 1.24 / 1.17 / 1.20 / 1.24 ms
        // per step in round 2, profiles/r02_notes.md; with round 3's shorter lean stage 128 / 144 / 160 / 176 / 192 / 224 / 288 =
        // 1.16 / 1.14 / 1.09-1.11 / 1.087-1.091 / 1.10-1.13 / 1.10-1.14 / 1.13-1.15, profiles/r03_notes.md: the rule gives 164 there,
        // rounded up to a multiple of 16 = 176; round 2 rounded to 32 = 192)
        // (with the direct launch's units edited on their runs -- ambi_finish_edit_kernel, done well before the table -- the lean kernel
        // gets some of the room the full-stage workgroups used to take.  First build of that stage: 224 (this rule) / 256 / 288 / 320 / 384
        // workgroups = 0.877 / 0.836 / 0.802 / 0.792 / 0.813 ms per step on one box, against 0.844-0.855 with the full-stage launch; with the
        // shorter lean stage of the final code (hashed synthesis, run emission beside it): 192 / 208 / 224 / 240 / 256 / 272 / 288 / 304 / 320 /
        // 336 = 0.82-0.86 / 0.78-0.83 / 0.82 / 0.78-0.81 / 0.77-0.81 / 0.826 / 0.830 / 0.847 / 0.847 / 0.848 on two boxes, three runs each
        // (profiles/r04_notes.md): one lean workgroup per CU; a fifth more than the rule's own figure)
        const double room = (direct_edit_ && direct_n_ > 0 && direct_ext_ && d_direct_cells_) ? 1.2 : 1.0;
        int64_t grid = (int64_t)((double)U * unit_us * room / enum_us) + 1;
        grid = (grid + 15) & ~int64_t(15);
        if (grid < 32) grid = 32;
        return grid < U ? (int)grid : U;
    }
    // the table kernels of a run: block emission per row class, the general path for the units it flagged, the wide units
    void launch_tables(hipStream_t st, const BatchArgs& A, int lds_emit, bool general) {
        const int grid = enum_grid_;
        if (enum_classes_ & 1) hipLaunchKernelGGL(ambi_enumerate_blocks_kernel<0>, dim3(grid), dim3(kEnumThreads), lds_emit, st, A);
        if (enum_classes_ & 2) hipLaunchKernelGGL(ambi_enumerate_blocks_kernel<1>, dim3(grid), dim3(kEnumThreads), lds_emit, st, A);
        if (enum_classes_ & 4) hipLaunchKernelGGL(ambi_enumerate_blocks_kernel<2>, dim3(grid), dim3(kEnumThreads), lds_emit, st, A);
        if ((enum_classes_ & 1) && general) hipLaunchKernelGGL(ambi_enumerate_kernel<0>, dim3(grid), dim3(256), lds_enum_, st, A);
        if ((enum_classes_ & 2) && general) hipLaunchKernelGGL(ambi_enumerate_kernel<1>, dim3(grid), dim3(256), lds_enum_, st, A);
        if ((enum_classes_ & 4) && general) hipLaunchKernelGGL(ambi_enumerate_kernel<2>, dim3(grid), dim3(256), lds_enum_, st, A);
        if (n_wide_ > 0) hipLaunchKernelGGL(ambi_enumerate_wide_kernel, dim3(64, n_wide_), dim3(256), 0, st, A, (const int32_t*)d_wide_units_, n_wide_);
    }
    void launch_back(const BatchArgs& A) {    // enumerate, first valid order, finish
        hipStream_t st = stream_;
        const int U = A.n_units;
        const int grid = enum_grid_;
        // The scan for the first valid order (reads the first rows the prepare stage left, not the table).  Beside a long
        // enumerate kernel it is launched AHEAD of it: behind the enumerate kernel in launch order its 4096 one-wave
        // workgroups only get group memory as enumerate workgroups retire (0.06 ms alone, 0.5-0.6 ms beside), and the
        // finish kernels behind it then start half-way through the table and end after it.
        hipStream_t sb = overlap_back_ ? side_.lean : st;
        auto launch_first = [&]() {
            tick("ambi_first_kernel", 4, true, sb);
            hipLaunchKernelGGL(ambi_first_kernel, dim3(U), dim3(64), lds_first_, sb, A);
            tick("ambi_first_kernel", 4, false, sb);
        };
        if (first_launched_) {   // started beside the plan kernel (launch_front): the finish kernels wait for both
            (void)hipStreamWaitEvent(sb, ev_first_, 0); (void)hipStreamWaitEvent(sb, ev_plan_, 0);
            if (direct_n_ > 0) (void)hipStreamWaitEvent(side_.full, ev_plan_, 0);
        } else if (overlap_back_) {   // (express chain) on the back stream behind the plan kernel, ahead of the enumerate launch
            (void)hipStreamWaitEvent(sb, ev_prep_, 0);
            launch_first();
            (void)hipEventRecord(ev_first_, sb);
        }
        tick("ambi_enumerate_kernel", 3, true);
        if (!lazy_) launch_tables(st, A, lds_blocks_, general_path_ != 0);   // (lazy: the tables are written on demand, materialise_tables)
        tick("ambi_enumerate_kernel", 3, false);
        if (!overlap_back_) launch_first();   // behind the enumerate kernel on the caller's stream
        // units with deletion / duplication candidates go straight to the full finish stage, on a stream of their own beside
        // the lean kernel (both behind the scan, both beside the enumerate kernel); few workgroups, each taking units in turn
        if (direct_n_ > 0 && overlap_back_) {
            (void)hipStreamWaitEvent(side_.full, ev_first_, 0);
            const int dgrid = direct_n_ < direct_grid_ ? direct_n_ : direct_grid_;
            // path area of this launch: the capacity bound of the batch, or (experiment switch AMBI_DIRECT_CELLS, see wait())
            // fewer cells -- a path that does not fit then goes through the list kernel behind, which has the full area
            BatchArgs Ad = A;
            int lds_direct = lds_finish_;
            if (direct_cells_ > 0 && direct_cells_ < finish_path_cells_) {
                Ad.finish_path_cells = direct_cells_; Ad.finish_retry = 1;
                lds_direct = (int)finish_work_bytes(hb().max_n, hb().max_m, hb().max_bkp, direct_cells_, hb().max_out);
            }
            direct_retry_ = Ad.finish_retry != 0;
            tick("ambi_finish_ext_kernel", 6, true, side_.full);
            if (direct_ext_ && d_direct_cells_ && direct_edit_) {
                // the edits of lone SVs on the runs of the path; what that stage hands on (chaining SVs, lists that outgrow their room)
                // to the launch with the path cells in device memory, over the list the first one leaves on the device
                direct_retry_ = false;
                const int egrid = direct_n_ < edit_grid_ ? direct_n_ : edit_grid_;
                hipLaunchKernelGGL(ambi_finish_edit_kernel, dim3(egrid), dim3(256), lds_finish_edit_, side_.full, A, (const int32_t*)d_direct_list_, direct_n_, d_edit_list_, d_refin_count_ + 1);
                hipLaunchKernelGGL(ambi_finish_ext_kernel, dim3(dgrid < 64 ? dgrid : 64), dim3(full_threads_), lds_finish_ext_, side_.full, A, (const int32_t*)d_edit_list_, 0, d_direct_cells_, direct_stride_,
                                   (const int32_t*)(d_refin_count_ + 1));
            } else
            if (direct_ext_ && d_direct_cells_) {   // path cells in device memory: a 13 KB workgroup that fits where a lean one fits
                direct_retry_ = false;
                hipLaunchKernelGGL(ambi_finish_ext_kernel, dim3(dgrid), dim3(full_threads_), lds_finish_ext_, side_.full, A, (const int32_t*)d_direct_list_, direct_n_, d_direct_cells_, direct_stride_);
            } else
            hipLaunchKernelGGL(ambi_finish_kernel, dim3(dgrid), dim3(full_threads_), lds_direct, side_.full, Ad, (const int32_t*)d_direct_list_, (const int32_t*)nullptr, direct_n_);
            tick("ambi_finish_ext_kernel", 6, false, side_.full);
            (void)hipEventRecord(ev_full_, side_.full);
        }
        tick("ambi_finish_kernel", 5, true, sb);
        const int fgrid = finish_grid_for(U);
        if (debug_) fprintf(stderr, "ambigram_hip: lean finish grid %d, image budget %d, mean path capacity %.0f, order bytes %lld\n", fgrid, block_lds_, avg_path_, (long long)last_needed_);
        if (lean_finish_) {
            hipLaunchKernelGGL(ambi_finish_lean_kernel, dim3(fgrid), dim3(256), lds_finish_lean_, sb, A, (const int32_t*)nullptr, 0);
            // units whose SVs chain or edit the path: the full stage right behind, over the list the lean kernel left on the
            // device (an empty list costs one launch of workgroups that exit at once)
            if (hb().any_sv) {
                if (direct_retry_ && direct_n_ > 0 && overlap_back_) (void)hipStreamWaitEvent(sb, ev_full_, 0);   // the direct launch may add to the list
                hipLaunchKernelGGL(ambi_finish_kernel, dim3(U < 256 ? U : 256), dim3(256), lds_finish_, sb, A, (const int32_t*)d_refin_list_, (const int32_t*)d_refin_count_, -1);   // (at most one such workgroup fits a CU: more than 256 gain nothing)
            }
        } else hipLaunchKernelGGL(ambi_finish_kernel, dim3(U), dim3(256), lds_finish_, sb, A, (const int32_t*)nullptr, (const int32_t*)nullptr, -1);
        tick("ambi_finish_kernel", 5, false, sb);
        if (overlap_back_) {
            (void)hipEventRecord(ev_back_, sb); (void)hipStreamWaitEvent(st, ev_back_, 0);
            if (direct_n_ > 0) (void)hipStreamWaitEvent(st, ev_full_, 0);
        }
    }

    // Everything of one run, queued on the caller's stream and the lease's side streams.  The FIRST run of a batch takes what
    // arena the lease has: the plan kernel reports what the tables need, and wait() grows the arena and runs the batch again
    // if that was not enough (round 2 ran prepare + plan, synchronised, sized the arena and only then queued the run --
    // two host round trips in front of every fresh batch).
    int64_t epoch_ = 0;
    int64_t results_epoch() const override { return epoch_; }
    void* own_stream() override {
        DeviceGuard dg_(device_);
        if (!lease_) return nullptr;
        if (!lease_->run_stream && hipStreamCreateWithFlags(&lease_->run_stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return lease_->run_stream;
    }
    int run(uint32_t flags, void* stream) override {
        DeviceGuard dg_(device_);
        epoch_++;
        if (!uploaded_) return -32;
        if (ran_ && !tuned_ && tables_written_) { if (int rc = tune_after_first_run()) return rc; }
        stream_ = (hipStream_t)stream;
        if ((want_overlap_ || side_lattice_) && stream_ != side_for_) {
            // side streams that dispatch beside THIS caller's stream (learnt once per stream and device: a few probe launches; a
            // stream seen before costs a look-up).  env AMBI_STREAM_CLASSES=0: by creation order, without probes
            const char* e = ambi_env("AMBI_STREAM_CLASSES");
            if (int rc = side_streams(*lease_->ctx, stream_, (int)(lease_->uses & 1), e ? atoi(e) != 0 : true, &side_)) return rc;
            side_for_ = stream_;
        }
        t_run_ = std::chrono::steady_clock::now();
        flushed_ = upload_pending_;
        if (int rc = flush_upload(stream_)) return rc;
        run_seq_ = ++lease_->seq;
        runs_parity_ = run_seq_ & 1;
        mail_valid_ = false;
        bind(flags);
        if (d_inject_) HIP_CK(hipMemsetAsync(d_inject_, 0, (size_t)hb().n_armed * kDebugOrderBytes, stream_));   // (diagnostics: the slots in front of the verdicts hold a row stored by THIS run)
        all_done_ = false;
        const int U = A_.n_units;
        lazy_ = (flags & FLAG_LAZY_ORDERS) != 0;
        overlap_back_ = want_overlap_;
        A_.direct_full_on = (overlap_back_ && direct_n_ > 0) ? 1 : 0;
        express_ = U <= express_units_ && lds_express_ <= kLdsMaxDynamic && dh_express_left_ != nullptr && n_wide_ == 0;
        // no copy commands around the kernels: they zero their counters and store the two words the host reads into pinned
        // memory themselves (see BatchArgs::zero_pending)
        A_.zero_pending = 1; A_.host_pending = dh_npending_; A_.host_needed = dh_needed_;
        const BatchArgs A = args();
        if (A.n_units > 0) {
            launch_front(A);
            if (lazy_ || (build_in_emit_ && shared_units_ == 0)) { tick("ambi_blocks_build_kernel", 2, true); tick("ambi_blocks_build_kernel", 2, false); }   // nothing to build
            else launch_build(A);
            launch_back(A);
        }
        HIP_CK(hipGetLastError());
        if (side_lattice_) (void)hipEventRecord(lease_->ev_tail, stream_);   // where the NEXT run's side lattice kernel may start
        tables_written_ = !lazy_;
        ran_ = true; inflight_ = true;
        t_launched_ = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_run_).count();
        if (timing_) timed_runs_++;
        return 0;
    }
    // A larger arena: the new one first, the old one goes only when that worked -- a failed growth leaves the batch as it was,
    // and the units whose tables do not fit the old arena end with ORDERS_CAPACITY (plan kernel), one by one.
    // AMBI_ARENA_MAX_BYTES: an upper limit for the arena (a memory budget; the tests use it to reach this path).  Every stream idle.
    bool grow_arena(int64_t total) {
        int64_t want = total;
        { const char* cap = ambi_env("AMBI_ARENA_MAX_BYTES"); if (cap && atoll(cap) > 0 && want > atoll(cap)) want = atoll(cap); }
        bool grown = false;
        uint8_t* fresh = nullptr;
        want = (want + 4095) & ~int64_t(4095);
        if (want > arena_bytes_ && hipMalloc((void**)&fresh, (size_t)want) == hipSuccess) {
            (void)hipFree(lease_->d_arena);
            lease_->d_arena = fresh; lease_->d_arena_bytes = want;
            d_arena_ = fresh; arena_bytes_ = want;
            grown = true;
        } else if (want > arena_bytes_) (void)hipGetLastError();
        if (arena_bytes_ < total)
            fprintf(stderr, "ambigram_hip: order-table arena of %lld bytes not available; keeping %lld bytes (units beyond it report ORDERS_CAPACITY)\n",
                    (long long)total, (long long)arena_bytes_);
        return grown;
    }
    // FLAG_LAZY_ORDERS: the order tables of the last run, now (plan -> image build -> enumerate on the caller's stream, waited
    // for; the arena grows first if it must).  Every stream idle.
    int materialise_tables() {
        if (tables_written_ || !ran_) return 0;
        for (int attempt = 0; attempt < 2; attempt++) {
            BatchArgs A = args();
            A.zero_pending = 1; A.host_pending = dh_npending_; A.host_needed = dh_needed_; A.lat_R = nullptr; A.plan_seq = nullptr; A.late_flag = nullptr;
            hipLaunchKernelGGL(ambi_plan_reset_kernel, dim3((A.n_units + 255) / 256), dim3(256), 0, stream_, A);
            hipLaunchKernelGGL(ambi_plan_kernel, dim3(1), dim3(1024), 0, stream_, A);
            hipLaunchKernelGGL(ambi_blocks_build_kernel, dim3(A.n_units), dim3(256), lds_build_, stream_, A);
            launch_tables(stream_, A, lds_blocks_, true);
            HIP_CK(hipGetLastError());
            HIP_CK(hipStreamSynchronize(stream_));
            const int64_t need = h_needed_[0];
            if (need <= arena_usable() || attempt == 1) break;
            const int64_t total = (need + (need >> 4) + 4096 + order_align_ - 1) & ~int64_t(order_align_ - 1);
            if (!grow_arena(total)) break;
            bind(A_.flags);
        }
        tables_written_ = true;
        return 0;
    }
    // the first complete run of a batch (every stream idle): did its tables fit the arena the lease had?
    int settle_first_run() {
        if (arena_checked_) return 0;
        arena_checked_ = true;
        const int64_t need = h_needed_[0];
        if (need > arena_bytes_) {
            const int64_t total = (need + (need >> 4) + 4096 + order_align_ - 1) & ~int64_t(order_align_ - 1);
            if (grow_arena(total)) {   // the whole batch again, now with room for every table (prepare resets what the first pass refused)
                lease_->h_words->late_flag = 0;
                ran_ = false;   // (the run below is still this batch's FIRST complete one: nothing is tuned from the refused pass)
                const bool t = timing_; timing_ = false;
                int rc = run(A_.flags, (void*)stream_);
                timing_ = t;
                if (rc) return rc;
                HIP_CK(hipStreamSynchronize(stream_));
                inflight_ = false;
            }
        }
        return 0;
    }
    // Launch parameters that depend on what the first run found (the batch is resident and immutable): which units need the
    // general enumerate kernel, whether any table is shared by several workgroups, the group-memory budget of the emission
    // workgroups.  Called before the SECOND run: a batch that is run once (one sample through the CLI) never pays for it.
    int tune_after_first_run() {
        if (int rc = wait()) return rc;
        tuned_ = true;
        {
            std::vector<int32_t> fb(hb().units.size());
            HIP_CK(hipMemcpy(fb.data(), d_fallback_, fb.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            general_path_ = 0;
            for (int32_t f : fb) general_path_ += f != 0;
            if (direct_n_ > 0) {
                // Path area of the direct full-finish launch.  Default: the capacity bound of the batch (82 KB of group memory
                // per workgroup on the bench batch, one per CU).  AMBI_DIRECT_CELLS=n: n cells, -1: what the paths of these
                // units needed in this first run plus a quarter (53 KB there, three per CU; longer paths then go through the
                // list kernel) -- measured SLOWER, 1.18 vs 1.155 ms per step: more of these 16-wave workgroups get onto the
                // CUs while the table is being written and take the places of enumerate workgroups.
                const char* e = ambi_env("AMBI_DIRECT_CELLS");
                direct_cells_ = e ? atoi(e) : 0;
                if (direct_cells_ < 0) {
                    std::vector<UnitOut> hdr(hb().units.size());
                    HIP_CK(hipMemcpy(hdr.data(), d_results_, hdr.size() * sizeof(UnitOut), hipMemcpyDeviceToHost));
                    int mx = 0;
                    for (size_t u2 = 0; u2 < hdr.size(); u2++)
                        if (hb().units[u2].direct_full) { mx = std::max(mx, hdr[u2].path_len); mx = std::max(mx, hdr[u2].path_indel_len); }
                    direct_cells_ = mx > 0 ? ((mx + mx / 4 + 256 + 2047) & ~2047) : 0;
                }
            }
            // ... and whether any unit's table is shared by several workgroups (only those go through the build kernel
            // when single-block units build their image in the enumerate workgroup): if none, later runs do not launch it
            std::vector<int64_t> bo(hb().units.size() + 1);
            HIP_CK(hipMemcpy(bo.data(), d_blk_off_, bo.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
            shared_units_ = 0;
            for (size_t u2 = 0; u2 + 1 < bo.size(); u2++) shared_units_ += (bo[u2 + 1] - bo[u2] > 1) ? 1 : 0;
            // Group memory per enumerate workgroup for the runs to come.  k workgroups share a CU's 160 KB and its store
            // bandwidth, so W work blocks take about ceil(W / (CUs * k)) * k "slot rounds": pick the k in 3..5 with the
            // fewest, among those whose budget 160 KB / k still holds every image of this batch (measured on the bench
            // batch, 4096 work blocks on 256 CUs: k = 3 (48 KB) 0.92-0.95 ms, k = 4 (40 KB) 0.86-0.87 ms).
            if (emit_lds_auto_ && general_path_ == 0 && bo.back() > 0) {
                std::vector<int32_t> hd(hb().units.size() * 8);
                HIP_CK(hipMemcpy(hd.data(), d_blk_hdr_, hd.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
                int need = 0;
                for (size_t u2 = 0; u2 < hb().units.size(); u2++) if (hd[8 * u2] > 0 && hd[8 * u2 + 3] > need) need = hd[8 * u2 + 3];
                int ncu = 256;
                { hipDeviceProp_t pr; int dev = 0; if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ncu = pr.multiProcessorCount; }
                const int64_t W = bo.back();
                int best_k = 0; int64_t best = 0;
                for (int k = 3; k <= 5; k++) {
                    const int budget = ((160 * 1024) / k) & ~15;
                    if (need <= 0 || need > budget) continue;
                    const int64_t rounds = ((W + (int64_t)ncu * k - 1) / ((int64_t)ncu * k)) * k;
                    if (!best_k || rounds < best) { best_k = k; best = rounds; }
                }
                if (debug_) fprintf(stderr, "ambigram_hip: image need %d bytes, %lld work blocks on %d CUs -> %d workgroups per CU\n", need, (long long)W, ncu, best_k);
                // ... and ask for no more than the images need (512-byte granules): what the k enumerate workgroups leave of
                // the CU's group memory is where the scan / finish workgroups run WITHOUT pushing an enumerate workgroup out
                if (best_k) {
                    block_lds_ = ((160 * 1024) / best_k) & ~15;
                    const int tight = (need + 511) & ~511;
                    if (emit_lds_tight_ && tight < block_lds_) block_lds_ = tight;
                    lds_blocks_ = block_lds_;
                }
            }
        }
        return 0;
    }

    // parallel search for units whose sequential scan ran out of budget (rare)
    int slow_path() {
        epoch_++;
        const int U = A_.n_units;
        std::vector<UnitOut> hdr(U);
        HIP_CK(hipMemcpy(hdr.data(), d_results_, U * sizeof(UnitOut), hipMemcpyDeviceToHost));
        // two kinds of leftovers: units whose scan ran out of budget (parallel search, then the full finish stage) and units
        // the lean finish stage handed over (full finish stage only)
        std::vector<int32_t> pend, refin;
        for (int u = 0; u < U; u++) {
            if (hdr[u].status == ST_PENDING) {
                if (hdr[u].order_off < 0) {   // cannot happen (the scan only takes units the plan kernel gave rows): never search a table that is not there
                    const int32_t st = ST_ERR_ORDERS_CAPACITY;
                    HIP_CK(hipMemcpy(reinterpret_cast<uint8_t*>(d_results_) + sizeof(UnitOut) * (size_t)u + offsetof(UnitOut, status), &st, sizeof(int32_t), hipMemcpyHostToDevice));
                    continue;
                }
                pend.push_back(u);
            } else if (hdr[u].status == ST_REFINISH) refin.push_back(u);
        }
        if (pend.empty() && refin.empty()) return 0;
        const int np = (int)pend.size(), nfin = np + (int)refin.size(), chunk = 16;
        const std::vector<int64_t> coff = search_chunk_prefix(hdr.data(), pend, chunk);
        std::vector<int32_t> fin(pend);
        fin.insert(fin.end(), refin.begin(), refin.end());
        DevBuf b_pend, b_coff, b_slots;
        HIP_CK(b_pend.alloc(nfin * sizeof(int32_t)));
        HIP_CK(b_coff.alloc((np + 1) * sizeof(int64_t)));
        HIP_CK(b_slots.alloc((np + 1) * sizeof(SearchSlot)));
        int32_t* d_pend = b_pend.as<int32_t>(); int64_t* d_coff = b_coff.as<int64_t>(); SearchSlot* d_slots = b_slots.as<SearchSlot>();
        HIP_CK(hipMemcpy(d_pend, fin.data(), nfin * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_CK(hipMemcpy(d_coff, coff.data(), (np + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        int waves = (4 * lds_first_ <= 150 * 1024) ? 4 : 1;
        bool fwd = !(A_.flags & FLAG_REVERSED);
        // both passes are queued back to back: a unit resolved by pass 0 is skipped by pass 1 (its status is no longer PENDING)
        for (int pass = 0; pass < 2 && np > 0; pass++) {
            hipLaunchKernelGGL(ambi_search_init_kernel, dim3((np + 255) / 256), dim3(256), 0, stream_, d_slots, np);
            SearchArgs S{d_pend, d_coff, d_slots, np, chunk, fwd ? 1 : 0, lds_first_};
            int64_t nblk = (coff[np] + waves - 1) / waves;
            if (nblk > 65535 * 16) nblk = 65535 * 16;
            if (nblk < 1) nblk = 1;
            hipLaunchKernelGGL(ambi_search_kernel, dim3((unsigned)nblk), dim3(64 * waves), waves * lds_first_, stream_, A_, S);
            hipLaunchKernelGGL(ambi_resolve_kernel, dim3(np), dim3(64), lds_first_, stream_, A_, S, pass);
            HIP_CK(hipGetLastError());
            fwd = !fwd;
        }
        // finish: the units the search resolved go through the lean stage first (any path length) and through the full stage only
        // when their SVs chain or edit the path (the list the lean kernel leaves on the device); the units the main chain's lean
        // stage had handed over already go straight to the full stage
        if (np > 0) {
            BatchArgs Al = A_;
            Al.host_pending = nullptr; Al.direct_full_on = 0;
            HIP_CK(hipMemsetAsync(d_refin_count_, 0, sizeof(int32_t), stream_));
            hipLaunchKernelGGL(ambi_finish_lean_kernel, dim3(np < 1024 ? np : 1024), dim3(256), lds_finish_lean_, stream_, Al, (const int32_t*)d_pend, np);
            // ... with the path cells in device memory where the batch has such areas (units with deletion / duplication candidates:
            // any path length), else in group memory (up to kPathLdsCells cells)
            int32_t handed = 0;
            HIP_CK(hipMemcpyAsync(&handed, d_refin_count_, sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
            HIP_CK(hipStreamSynchronize(stream_));
            if (handed > 0 && d_direct_cells_ && direct_slots_ > 0)
                hipLaunchKernelGGL(ambi_finish_ext_kernel, dim3(handed < direct_slots_ ? handed : direct_slots_), dim3(full_threads_), lds_finish_ext_, stream_, Al,
                                   (const int32_t*)d_refin_list_, (int)handed, d_direct_cells_, direct_stride_);
            else if (handed > 0)
                hipLaunchKernelGGL(ambi_finish_kernel, dim3(handed < 256 ? handed : 256), dim3(256), lds_finish_, stream_, Al, (const int32_t*)d_refin_list_, (const int32_t*)d_refin_count_, -1);
        }
        if (nfin > np) hipLaunchKernelGGL(ambi_finish_kernel, dim3(nfin - np), dim3(256), lds_finish_, stream_, A_, (const int32_t*)(d_pend + np), (const int32_t*)nullptr, -1);
        HIP_CK(hipGetLastError());
        HIP_CK(hipStreamSynchronize(stream_));
        return 0;
    }

    int wait() override {
        DeviceGuard dg_(device_);
        if (!ran_) return 0;
        HIP_CK(hipStreamSynchronize(stream_));
        inflight_ = false;
        if (tables_written_) { if (int rc = settle_first_run()) return rc; }
        if (check_guards("wait")) return -31;
        if (tables_written_) last_needed_ = *h_needed_;
        late_refusal_ = lease_->h_words->late_flag != 0;
        if (*h_npending_ > 0) {
            if (int rc = materialise_tables()) return rc;   // (FLAG_LAZY_ORDERS: the parallel search reads the tables)
            int rc = slow_path();
            if (rc) return rc;
            *h_npending_ = 0;
        }
        if ((A_.flags & FLAG_ALL) && !all_done_) {
            int rc = compute_all();
            if (rc) return rc;
            all_done_ = true;
        }
        // the mailbox of a small batch holds what the express kernel published; nothing behind it changed a header
        mail_valid_ = express_ && mail_on_ && !(A_.flags & FLAG_ALL) && *(volatile int32_t*)h_express_left_ == 0 && !late_refusal_;
        if (timing_ && timed_runs_ > 0) {
            // average duration of ONE launch of every kernel over the slots filled since timing was switched on
            const long filled = timed_runs_ < kTimingSlots ? timed_runs_ : kTimingSlots;
            times_.clear();
            static const char* const kKernelNames[kTimedKernels] = {"ambi_prepare_kernel", "ambi_plan_kernel", "ambi_blocks_build_kernel",
                                                                    "ambi_enumerate_kernel", "ambi_first_kernel", "ambi_finish_kernel", "ambi_finish_ext_kernel"};
            for (int k = 0; k < kTimedKernels; k++) {
                double sum = 0, s0 = 0, s1 = 0; int cnt = 0, cnt_span = 0; const char* nm = kKernelNames[k];
                if (!((timing_mask_ >> k) & 1u)) { times_.push_back({nm, -1.0f}); continue; }
                for (long sl = 0; sl < filled; sl++) {
                    const size_t at = (size_t)sl * kTimedKernels + k;
                    if (at >= evs().size() || !evs()[at].a) continue;
                    float ms = 0;
                    if (hipEventElapsedTime(&ms, evs()[at].a, evs()[at].b) == hipSuccess) { sum += ms; cnt++; nm = evs()[at].name; }
                    // where the kernel sits in its run: from the event in front of the run's first kernel (the events of one slot
                    // belong to one run; they sit on different streams of one device)
                    const size_t at0 = (size_t)sl * kTimedKernels;
                    float a = 0, b = 0;
                    if ((timing_mask_ & 1u) && at0 < evs().size() && evs()[at0].a && hipEventElapsedTime(&a, evs()[at0].a, evs()[at].a) == hipSuccess &&
                        hipEventElapsedTime(&b, evs()[at0].a, evs()[at].b) == hipSuccess) { s0 += a; s1 += b; cnt_span++; }
                }
                KernelTime kt{nm, cnt ? (float)(sum / cnt) : -1.0f};
                if (cnt_span) { kt.start_ms = (float)(s0 / cnt_span); kt.end_ms = (float)(s1 / cnt_span); }
                times_.push_back(kt);
            }
            (void)hipGetLastError();   // an event pair that was never recorded reports an error above: not one of ours
        }
        if (timing_ && (A_.flags & FLAG_ALL) && all_kernel_ms_ >= 0) {   // both passes of the --all evaluation of the last run
            if (!times_.empty() && !strcmp(times_.back().name, "ambi_all_kernel")) times_.pop_back();
            times_.push_back({"ambi_all_kernel", all_kernel_ms_});
        }
        return 0;
    }
    // Results complete (paths, breakpoints, output junctions of every unit) -- which, for a small batch on the express path,
    // is before the order tables behind them are written.  Returns early only when NOTHING behind the express kernel can
    // still void a result it published: no unit left to the ordinary kernels, and no unit that the lattice or plan stage
    // refuses afterwards (more order ideals than the table holds, an order table the arena has no room for).  For a batch
    // that has completed a run that is known (inputs are immutable); for a fresh batch the host also waits for the plan
    // kernel's verdict, which reaches it through pinned memory like the express kernel's.  Otherwise the same as wait().
    int wait_results() override {
        DeviceGuard dg_(device_);
        if (!ran_) return 0;
        static const bool lat = ambi_env("AMBI_DEBUG_LATENCY") != nullptr;   // diagnostics: when the two pinned words arrived, from the start of run()
        auto since = [&]() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_run_).count(); };
        if (express_ && !(A_.flags & FLAG_ALL) && ev_express_ && !late_refusal_ && (!lazy_ || arena_checked_)) {
            // the kernel's last workgroup stores the run's sequence number into pinned host memory: a short spin on it
            // returns microseconds before an event wait would; the event wait is the fallback
            volatile int32_t* seq = h_express_left_ + 1;
            bool seen = false;
            for (int spin = 0; spin < 400000 && !(seen = (*seq == run_seq_)); spin++) __builtin_ia32_pause();
            if (!seen) HIP_CK(hipEventSynchronize(ev_express_));
            const double t_express = lat ? since() : 0;
            if (*(volatile int32_t*)h_express_left_ == 0) {
                if (arena_checked_) { mail_valid_ = mail_on_; if (lat) fprintf(stderr, "ambigram latency: run() returned %.1f us, express word %.1f us\n", t_launched_, t_express); return 0; }
                // fresh batch: the verdict of the side lattice kernel (every lattice fine, all tables together fit the arena), or
                // else the plan kernel's
                volatile int32_t* pseq = side_lattice_ ? &lease_->h_words->lat_seq : &lease_->h_words->plan_seq;
                seen = false;
                for (int spin = 0; spin < 400000 && !(seen = (*pseq == run_seq_)); spin++) __builtin_ia32_pause();
                const bool fine = side_lattice_ ? *(volatile int32_t*)&lease_->h_words->lat_unsure == 0
                                                : (*(volatile int32_t*)&lease_->h_words->late_flag == 0 && *(volatile int64_t*)h_needed_ <= arena_usable());
                if (seen && fine) {
                    arena_checked_ = true;     // every table of this batch fits the arena: true for all its runs
                    mail_valid_ = mail_on_;
                    if (lat) fprintf(stderr, "ambigram latency: run() returned %.1f us, express word %.1f us, plan word %.1f us (fresh batch)\n", t_launched_, t_express, since());
                    return 0;
                }
            }
        }
        return wait();
    }
    // header + final paths + output junctions of a unit on the HOST without a copy command: the pinned mailbox slot the
    // express kernel filled (nullptr: not available -- the caller downloads the result blob instead)
    const uint8_t* mail_slot(int unit) override {
        if (!mail_valid_ || !lease_ || unit < 0 || unit >= (int)mail_off_.size()) return nullptr;
        return lease_->h_mail + mail_off_[unit];
    }
    int download(std::vector<uint8_t>& blob) override {
        DeviceGuard dg_(device_);
        int rc = wait();
        if (rc) return rc;
        if (upload_pending_) { if ((rc = flush_upload(nullptr))) return rc; HIP_CK(hipStreamSynchronize(nullptr)); }   // never run: the blob is all zeroes
        blob.resize((size_t)hb().result_bytes);
        HIP_CK(hipMemcpy(blob.data(), d_results_, (size_t)hb().result_bytes, hipMemcpyDeviceToHost));
        if (d_stage_clk_) dump_stage_profile();
        return 0;
    }
    // AMBI_STAGE_PROFILE=1: mean shader-clock distance between consecutive marks of the per-unit stages (last run)
    void dump_stage_profile() {
        const size_t U = hb().units.size();
        std::vector<int64_t> clk(U * kStageSlots);
        if (hipMemcpy(clk.data(), d_stage_clk_, clk.size() * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess) return;
        // marks 0-8 and 22-31: prepare (22-24 inside constructDAG, 26-28 inside the lattice); 9-12: scan; 16-21: finish.
        // Express kernel: 9 = start, 6 = junction side done, 7 = DAG built, 8 = order 0 found, 10 = both sides done (placement
        // included), 11 = imperfectFBI done, 12 = finish stage done
        fprintf(stderr, "ambigram_hip stage profile (mean cycles from the first mark of the stage, %zu units):", U);
        for (int s = 1; s < kStageSlots; s++) {
            const int base = ((s >= 13 && s <= 15) || s == 29 || s == 30) ? 31 : (s == 25 ? 9 : ((s <= 8 || s >= 22) ? 0 : (s <= 12 ? 9 : 16)));   // 13-15, 29, 30: image build (from 31)
            if (s == base) continue;
            double sum = 0; size_t cnt = 0;
            for (size_t u = 0; u < U; u++) {
                int64_t a = clk[u * kStageSlots + base];
                const int64_t b = clk[u * kStageSlots + s];
                if (!a && (base == 0 || base == 31)) a = clk[u * kStageSlots + 9];   // express kernel: the marks of the prepare pieces count from its own first mark
                if (a && b && b >= a) { sum += (double)(b - a); cnt++; }
            }
            if (cnt) fprintf(stderr, " [%d]=%.0f", s, sum / cnt);
        }
        fprintf(stderr, "\n");
    }
    int device_results(void** ptr, int64_t* bytes) override {
        if (ptr) *ptr = d_results_;
        if (bytes) *bytes = hb().result_bytes;
        return 0;
    }
    int pack_paths(int which, int32_t* dev_lengths, int32_t* dev_cells, int64_t cell_cap, int64_t* dev_total, void* stream) override {
        DeviceGuard dg_(device_);
        hipStream_t s = (hipStream_t)stream;
        bind(A_.flags);
        hipLaunchKernelGGL(ambi_pack_scan_kernel, dim3(1), dim3(1024), 0, s, A_, which, dev_lengths, d_pack_off_, dev_total);
        hipLaunchKernelGGL(ambi_pack_copy_kernel, dim3(A_.n_units), dim3(256), 0, s, A_, which, (const int64_t*)d_pack_off_, dev_cells, cell_cap);
        HIP_CK(hipGetLastError());
        return 0;
    }
    int pack_runs(int which, int32_t* dev_lengths, int32_t* dev_run_counts, int32_t* dev_run_start, int32_t* dev_run_len, int64_t run_cap,
                  int64_t* dev_totals, void* stream) override {
        DeviceGuard dg_(device_);
        hipStream_t s = (hipStream_t)stream;
        bind(A_.flags);
        hipLaunchKernelGGL(ambi_pack_runs_count_kernel, dim3(A_.n_units), dim3(256), 0, s, A_, which, dev_lengths, dev_run_counts);
        hipLaunchKernelGGL(ambi_pack_runs_scan_kernel, dim3(1), dim3(1024), 0, s, A_, (const int32_t*)dev_lengths, (const int32_t*)dev_run_counts,
                           d_pack_off_, dev_totals);
        hipLaunchKernelGGL(ambi_pack_runs_write_kernel, dim3(A_.n_units), dim3(256), 0, s, A_, which, (const int64_t*)d_pack_off_, dev_run_start,
                           dev_run_len, run_cap);
        HIP_CK(hipGetLastError());
        return 0;
    }
    // ---- final paths to the HOST in run-length form (the timed region ends with the "final path buffers on host";
    // the reference prints every path, LGM.cpp:3684-3689) ----
    // Slot layout (int32 words, device block and pinned mirror alike):
    //   [0..3] totals {runs, cells} as two int64 | lengths[U] | run_counts[U] | run_start[cap] | run_len[cap] | (headers: UnitOut[U])
    // runs_to_host queues, behind everything already on `stream`: the three pack kernels into the slot's device block, then ONE
    // device-to-host copy of the block on the lease's copy stream (so the caller's stream is free for the next run at once).
    // runs_wait waits for that copy; a slot whose capacity was too small is packed again with the capacity the totals name.
    int64_t runs_cap_[2] = {0, 0}; int runs_which_[2] = {0, 0}; bool runs_hdr_[2] = {false, false}, runs_queued_[2] = {false, false};
    int64_t runs_words(int64_t cap) const { return 4 + 2 * (int64_t)hb().units.size() + 2 * cap; }
    int runs_queue(int which, int slot, bool headers, void* stream, int64_t cap) {
        Lease* L = lease_;
        const int64_t U = (int64_t)hb().units.size();
        const int64_t words = runs_words(cap), hdr_bytes = headers ? U * (int64_t)sizeof(UnitOut) : 0;
        const int64_t bytes = ((words * 4 + 15) & ~int64_t(15)) + hdr_bytes;
        if (int rc = lease_device_block(&L->d_runs[slot], &L->d_runs_bytes[slot], bytes)) return rc;
        if (int rc = lease_pinned_block(&L->h_runs[slot], nullptr, &L->h_runs_bytes[slot], bytes)) return rc;
        if (!L->copy_stream) HIP_CK(hipStreamCreateWithFlags(&L->copy_stream, hipStreamNonBlocking));
        for (int k = 0; k < 2; k++) {
            if (!L->ev_runs_packed[k]) HIP_CK(hipEventCreateWithFlags(&L->ev_runs_packed[k], hipEventDisableTiming));
            if (!L->ev_runs_done[k]) HIP_CK(hipEventCreateWithFlags(&L->ev_runs_done[k], hipEventDisableTiming));
        }
        hipStream_t s = (hipStream_t)stream;
        int32_t* w = reinterpret_cast<int32_t*>(L->d_runs[slot]);
        if (int rc = pack_runs(which, w + 4, w + 4 + U, w + 4 + 2 * U, w + 4 + 2 * U + cap, cap, reinterpret_cast<int64_t*>(w), stream)) return rc;
        HIP_CK(hipEventRecord(L->ev_runs_packed[slot], s));
        HIP_CK(hipStreamWaitEvent(L->copy_stream, L->ev_runs_packed[slot], 0));
        HIP_CK(hipMemcpyAsync(L->h_runs[slot], L->d_runs[slot], (size_t)(words * 4), hipMemcpyDeviceToHost, L->copy_stream));
        if (headers) HIP_CK(hipMemcpyAsync(L->h_runs[slot] + ((words * 4 + 15) & ~int64_t(15)), d_results_, (size_t)hdr_bytes, hipMemcpyDeviceToHost, L->copy_stream));
        HIP_CK(hipEventRecord(L->ev_runs_done[slot], L->copy_stream));
        runs_cap_[slot] = cap; runs_which_[slot] = which; runs_hdr_[slot] = headers; runs_queued_[slot] = true;
        return 0;
    }
    // which = 1 (the final path): the finish stages of the last run left the runs in the block of that run's parity (BatchArgs::run_*),
    // so there is nothing to compute -- ONE copy of that block on the copy stream, behind an event on the caller's stream.  which = 0, or
    // a batch with a unit whose runs overflowed its slots: the pack kernels (runs_queue).
    bool runs_direct_[2] = {false, false}; std::vector<int64_t> runs_off_[2];
    int runs_to_host(int which, int slot, int with_headers, void* stream) override {
        DeviceGuard dg_(device_);
        if (!ran_ || slot < 0 || slot > 1) return ST_ERR_BAD_INPUT;
        static const bool no_direct = ambi_env("AMBI_RUNS_PACK") != nullptr;   // env AMBI_RUNS_PACK=1: always through the pack kernels
        if (which == 1 && run_total_ > 0 && runs_parity_ >= 0 && !no_direct) {
            Lease* L = lease_;
            const int64_t U = (int64_t)hb().units.size();
            const int64_t words = 2 * U + 2 * run_total_, hdr_bytes = with_headers ? U * (int64_t)sizeof(UnitOut) : 0;
            const int64_t bytes = ((words * 4 + 15) & ~int64_t(15)) + hdr_bytes;
            if (int rc = lease_pinned_block(&L->h_runs[slot], nullptr, &L->h_runs_bytes[slot], bytes)) return rc;
            if (!L->copy_stream) HIP_CK(hipStreamCreateWithFlags(&L->copy_stream, hipStreamNonBlocking));
            for (int k = 0; k < 2; k++) {
                if (!L->ev_runs_packed[k]) HIP_CK(hipEventCreateWithFlags(&L->ev_runs_packed[k], hipEventDisableTiming));
                if (!L->ev_runs_done[k]) HIP_CK(hipEventCreateWithFlags(&L->ev_runs_done[k], hipEventDisableTiming));
            }
            HIP_CK(hipEventRecord(L->ev_runs_packed[slot], (hipStream_t)stream));
            HIP_CK(hipStreamWaitEvent(L->copy_stream, L->ev_runs_packed[slot], 0));
            HIP_CK(hipMemcpyAsync(L->h_runs[slot], d_run_blk_[runs_parity_], (size_t)(words * 4), hipMemcpyDeviceToHost, L->copy_stream));
            if (with_headers) HIP_CK(hipMemcpyAsync(L->h_runs[slot] + ((words * 4 + 15) & ~int64_t(15)), d_results_, (size_t)hdr_bytes, hipMemcpyDeviceToHost, L->copy_stream));
            HIP_CK(hipEventRecord(L->ev_runs_done[slot], L->copy_stream));
            runs_which_[slot] = which; runs_hdr_[slot] = with_headers != 0; runs_queued_[slot] = true; runs_direct_[slot] = true;
            return 0;
        }
        // capacity: what the last complete pack of this batch needed, else a bound from the breakpoint capacities (a run per
        // breakpoint pair, a few more where indelBFB edits the path)
        int64_t cap = std::max(runs_cap_[0], runs_cap_[1]);
        if (cap <= 0) { for (const UnitIn& un : hb().units) cap += un.bkp_cap / 2 + 8; cap += 64; }
        runs_direct_[slot] = false;
        return runs_queue(which, slot, with_headers != 0, stream, cap);
    }
    int runs_wait(int slot, RunsView* out) override {
        DeviceGuard dg_(device_);
        if (slot < 0 || slot > 1 || !runs_queued_[slot] || !out) return ST_ERR_BAD_INPUT;
        Lease* L = lease_;
        const int64_t U = (int64_t)hb().units.size();
        if (runs_direct_[slot]) {
            HIP_CK(hipEventSynchronize(L->ev_runs_done[slot]));
            const int32_t* w = reinterpret_cast<const int32_t*>(L->h_runs[slot]);
            int64_t nr = 0, nc = 0; bool over = false;
            for (int64_t u = 0; u < U; u++) { if (w[u] < 0) over = true; else nr += w[u]; nc += w[U + u]; }
            if (!over) {
                const int64_t words = 2 * U + 2 * run_total_;
                out->n_runs = nr; out->n_cells = nc;
                out->run_counts = w; out->lengths = w + U; out->run_start = w + 2 * U; out->run_len = w + 2 * U + run_total_;
                out->run_off = hb().run_slot.data();
                out->headers = runs_hdr_[slot] ? L->h_runs[slot] + ((words * 4 + 15) & ~int64_t(15)) : nullptr;
                out->bytes = (2 * U + 2 * nr) * 4 + (runs_hdr_[slot] ? U * (int64_t)sizeof(UnitOut) : 0);
                out->copied_bytes = words * 4 + (runs_hdr_[slot] ? U * (int64_t)sizeof(UnitOut) : 0);
                return 0;
            }
            // a unit's runs did not fit its slots: this batch through the pack kernels (results are still those of the last run)
            runs_direct_[slot] = false;
            int64_t cap = 0; for (const UnitIn& un : hb().units) cap += un.bkp_cap / 2 + 8; cap += 64;
            if (int rc = runs_queue(runs_which_[slot], slot, runs_hdr_[slot], stream_, cap)) return rc;
        }
        for (int attempt = 0; attempt < 2; attempt++) {
            HIP_CK(hipEventSynchronize(L->ev_runs_done[slot]));
            const int64_t* tot = reinterpret_cast<const int64_t*>(L->h_runs[slot]);
            if (tot[0] <= runs_cap_[slot]) break;
            if (attempt == 1) return ST_ERR_BAD_INPUT;
            // more runs than the slot holds (the kernels wrote none beyond it): once more with room for all of them
            if (int rc = runs_queue(runs_which_[slot], slot, runs_hdr_[slot], stream_, tot[0] + (tot[0] >> 3) + 64)) return rc;
        }
        const int32_t* w = reinterpret_cast<const int32_t*>(L->h_runs[slot]);
        const int64_t cap = runs_cap_[slot], words = runs_words(cap);
        out->n_runs = reinterpret_cast<const int64_t*>(w)[0]; out->n_cells = reinterpret_cast<const int64_t*>(w)[1];
        out->lengths = w + 4; out->run_counts = w + 4 + U; out->run_start = w + 4 + 2 * U; out->run_len = w + 4 + 2 * U + cap;
        runs_off_[slot].assign((size_t)U + 1, 0);
        for (int64_t u = 0; u < U; u++) runs_off_[slot][(size_t)u + 1] = runs_off_[slot][(size_t)u] + out->run_counts[u];
        out->run_off = runs_off_[slot].data();
        out->headers = runs_hdr_[slot] ? L->h_runs[slot] + ((words * 4 + 15) & ~int64_t(15)) : nullptr;
        out->bytes = (4 + 2 * U + 2 * out->n_runs) * 4 + (runs_hdr_[slot] ? U * (int64_t)sizeof(UnitOut) : 0);   // what the payload needs (the copy moves the slot's capacity)
        out->copied_bytes = words * 4 + (runs_hdr_[slot] ? U * (int64_t)sizeof(UnitOut) : 0);
        return 0;
    }
    // ---- on-request results: the profiles (ambi_profile.hpp, ambi_junc_profile.hpp, ambi_frag_profile.hpp, ambi_evidence_profile.hpp, ambi_fold_profile.hpp) and the sequences below ----
    // A request works on `stream` behind everything that writes the result blob in the last run: the caller's stream of that run,
    // which has waited for every side stream at the end of run(), and -- for a caller that asks on another stream -- explicitly the
    // events "results complete" of the side streams (lean / list finish kernels, direct edit + full launch) and of the express
    // kernel.  behind_results() holds these waits for all three requests; src: the request's own event for the run's stream.
    int behind_results(hipStream_t s, hipEvent_t src) {
        if (s != stream_) { HIP_CK(hipEventRecord(src, stream_)); HIP_CK(hipStreamWaitEvent(s, src, 0)); }
        if (overlap_back_) {
            HIP_CK(hipStreamWaitEvent(s, ev_back_, 0));
            if (direct_n_ > 0) HIP_CK(hipStreamWaitEvent(s, ev_full_, 0));
        }
        if (express_) HIP_CK(hipStreamWaitEvent(s, ev_express_, 0));
        return 0;
    }
    // The fragment image of the batch (FragImage, ambi_pack.hpp) on the device: nothing of it travels with the batch; it goes up on
    // the request's stream when the device does not hold this version of it (DeviceImage::upload).
    FragArgs frag_args_{};
    int fragment_image(hipStream_t s) {
        DeviceImage& D = lease_->img[Lease::kFragImage];
        const FragImage& I = hb().frag;
        const int64_t U = (int64_t)hb().units.size();
        if ((int64_t)I.pref_off.size() != U || (int64_t)I.cell_off.size() != U || (int64_t)I.n_frag.size() != U) return ST_ERR_BAD_INPUT;   // (not sealed)
        const int64_t b0 = pad16(2 * (int64_t)I.cells.size()), b1 = b0 + pad16(4 * (int64_t)I.frag_off.size()), b2 = b1 + 8 * U, b3 = b2 + 8 * U, total = b3 + pad16(4 * U);
        if (int rc = D.upload(s, I.version, total, [&](uint8_t* h) {
                if (!I.cells.empty()) memcpy(h, I.cells.data(), 2 * I.cells.size());
                memcpy(h + b0, I.frag_off.data(), 4 * I.frag_off.size());
                memcpy(h + b1, I.cell_off.data(), (size_t)(8 * U));
                memcpy(h + b2, I.pref_off.data(), (size_t)(8 * U));
                memcpy(h + b3, I.n_frag.data(), (size_t)(4 * U));
            })) return rc;
        frag_args_ = FragArgs{reinterpret_cast<const rcell_t*>(D.d), reinterpret_cast<const int32_t*>(D.d + b0), reinterpret_cast<const int64_t*>(D.d + b1),
                              reinterpret_cast<const int64_t*>(D.d + b2), reinterpret_cast<const int32_t*>(D.d + b3)};
        return 0;
    }
    // The given paths of a pair request (PairRequest::given: the request's copy of the set) in a device buffer of the kind's own, in
    // the same way.  The batch image is not touched.
    CompareGiven given_args_[2] = {};   // [kind - kCompare]
    int given_image(ProfileKind kind, hipStream_t s) {
        DeviceImage& D = lease_->img[Lease::kGivenImage + kind - kCompare];
        const ComparePaths& I = pair_of(kind).given;
        if (int rc = D.upload(s, I.version, I.image_bytes(), [&](uint8_t* h) { I.image(h); })) return rc;
        given_args_[kind - kCompare] = compare_given(D.d, I);
        return 0;
    }
    // The length image of the batch (LenImage, ambi_pack.hpp) on the device, in the same way.
    LenArgs len_args_{};
    int length_image(hipStream_t s) {
        DeviceImage& D = lease_->img[Lease::kLenImage];
        const LenImage& I = hb().len;
        const int64_t U = (int64_t)hb().units.size();
        if ((int64_t)I.len_off.size() != U) return ST_ERR_BAD_INPUT;   // (not sealed)
        const int64_t b0 = pad16(4 * (int64_t)I.len.size()), total = b0 + pad16(8 * U) + 16;
        if (int rc = D.upload(s, I.version, total, [&](uint8_t* h) {
                if (!I.len.empty()) memcpy(h, I.len.data(), 4 * I.len.size());
                if (U > 0) memcpy(h + b0, I.len_off.data(), (size_t)(8 * U));
            })) return rc;
        len_args_ = LenArgs{reinterpret_cast<const int32_t*>(D.d), reinterpret_cast<const int64_t*>(D.d + b0)};
        return 0;
    }
    // The on-request results are instances of one block (Lease::prof, req_, Backend::prof_); a kind has its own inputs, its own layout,
    // its own kernels with their LDS sizes, and nothing else: each of these is one switch below, and the table of the kinds is above
    // Backend::ProfileKind.  profile() queues the kind's kernels behind the run, then ONE device-to-host copy of the block on the
    // lease's copy stream, as runs_to_host does it: `stream` is free for the next run at once.  profile_wait() makes the results final
    // (wait(): the first run done again with a larger arena, units finished by the parallel search) and, if that moved the results'
    // epoch after the kernels were queued, queues kernels and copy once more.
    int profile_queue(ProfileKind kind, int which, hipStream_t s) {
        Lease* L = lease_;
        RequestBlock& B = L->prof[kind]; Request& R = req_[kind]; ProfileState& P = prof_[kind];
        const int64_t U = (int64_t)hb().units.size();
        // 1. inputs: the kind's image, behind the kernels that still read another version of it
        switch (kind) {
            case kCopyNumber: case kJunction: case kFold: break;
            case kFragment: case kEvidence:   // (the image can change between requests, and with it the fragment kind's layout)
                if (!L->img[Lease::kFragImage].holds(hb().frag.version)) {
                    for (ProfileKind k : {kFragment, kEvidence}) if (req_[k].queued) HIP_CK(hipEventSynchronize(L->prof[k].ev_done));
                    req_[kFragment].laid_out = false; R.laid_out = false;
                }
                if (int rc = fragment_image(s)) return rc;
                break;
            case kCompare: case kAlign:   // (entries and cap come with the request: laid out every time, once the last request's kernel, copy and upload have left image, block and twin)
                if (R.queued) HIP_CK(hipEventSynchronize(B.ev_done));
                R.laid_out = false;
                if (int rc = given_image(kind, s)) return rc;
                break;
            case kCoords:   // (the queries come with the request: laid out every time, as above; nothing of the kind reads the image any more by then)
                if (R.queued) HIP_CK(hipEventSynchronize(B.ev_done));
                R.laid_out = false;
                if (int rc = length_image(s)) return rc;
                break;
        }
        // 2. layout: the block and its twin, the tail that travels up behind the block once per layout (the block's copies never touch
        // it), and the side area
        if (!R.laid_out) {
            profile_layout(kind);
            struct { const void* p; int64_t bytes; } tail[2] = {{P.off.data(), 8 * U}, {nullptr, 0}};
            int64_t side_bytes = 0;
            switch (kind) {
                case kCopyNumber: case kJunction: case kFragment: break;
                case kEvidence: tail[1] = {depth_off_.data(), 8 * U}; side_bytes = depth_bytes_ > 0 ? depth_bytes_ : 16; break;
                case kFold: tail[1] = {plane_off_.data(), 8 * U}; side_bytes = plane_bytes_ > 0 ? 2 * plane_bytes_ : 16; break;
                case kCompare: tail[0] = {pair_of(kind).entries.data(), 8 * (int64_t)compare_pairs()}; break;
                case kAlign: tail[0] = {pair_of(kind).entries.data(), 12 * (int64_t)align_pairs()}; side_bytes = align_grid_of() * align_history_bytes(pair_of(kind).dmax); break;
                case kCoords: tail[0] = {cplane_off_.data(), 8 * U}; tail[1] = {lift_.data(), 16 * (int64_t)coords_queries()}; side_bytes = cplane_bytes_ > 0 ? cplane_bytes_ : 16; break;
            }
            const int64_t n_off = (tail[0].bytes + tail[1].bytes + 7) / 8;
            const int64_t total = P.bytes + n_off * (int64_t)sizeof(int64_t);   // (P.bytes is a multiple of 16)
            if (side_bytes > 0) { if (int rc = lease_device_block(&B.side, &B.side_bytes, side_bytes)) return rc; }   // (no kernel of the kind is in flight that the layout would move it under)
            if (int rc = lease_device_block(&B.d, &B.d_bytes, total)) return rc;
            if (int rc = lease_pinned_block(&B.h, nullptr, &B.h_bytes, total)) return rc;
            if (!L->copy_stream) HIP_CK(hipStreamCreateWithFlags(&L->copy_stream, hipStreamNonBlocking));
            for (hipEvent_t* e : {&B.ev_src, &B.ev_packed, &B.ev_done}) if (!*e) HIP_CK(hipEventCreateWithFlags(e, hipEventDisableTiming));
            if (tail[0].bytes > 0) memcpy(B.h + P.bytes, tail[0].p, (size_t)tail[0].bytes);
            if (tail[1].bytes > 0) memcpy(B.h + P.bytes + tail[0].bytes, tail[1].p, (size_t)tail[1].bytes);
            R.d_off = reinterpret_cast<int64_t*>(B.d + P.bytes);
            if (n_off > 0) HIP_CK(hipMemcpyAsync(R.d_off, B.h + P.bytes, (size_t)n_off * sizeof(int64_t), hipMemcpyHostToDevice, s));
            R.laid_out = true;
        }
        // 3. ordering: behind the results, and behind an earlier request nobody waited for (its copy still reads the block)
        if (int rc = behind_results(s, B.ev_src)) return rc;
        if (R.queued) HIP_CK(hipStreamWaitEvent(s, B.ev_done, 0));
        // 4. launch: the kind's windows, LDS sizes and kernels (A_: units and result blob as the last run bound them)
        const dim3 grid((unsigned)(U < 16384 ? U : 16384)), threads(kProfileThreads);
        const int64_t* off = R.d_off; const int64_t* side_off = R.d_off + U;
        const int scratch = kProfileScratchBytes;
        switch (kind) {
            case kCopyNumber: {
                const int window = profile_window_of();
                hipLaunchKernelGGL(ambi_path_profile_kernel, grid, threads, scratch + (int)profile_bins_bytes(window), s, A_, which, window, B.d, off);
                break;
            }
            case kJunction: {
                int jwin, slots, swin; junc_profile_windows(&jwin, &slots, &swin);
                hipLaunchKernelGGL(ambi_junc_profile_kernel, grid, threads, scratch + (int)junc_profile_lds_bytes(slots, swin), s, A_, which, jwin, slots, swin, B.d, off);
                break;
            }
            case kFragment: {
                int pwin, slots; frag_profile_windows(&pwin, &slots);
                hipLaunchKernelGGL(ambi_frag_profile_kernel, grid, threads, scratch + (int)frag_profile_lds_bytes(slots, pwin), s, A_, frag_args_, which, pwin, slots, B.d, off);
                break;
            }
            case kEvidence: {   // (the scan kernel behind the mark kernel on one stream: the boundary orders atomics and loads)
                int pwin, fslots, jwin, slots; frag_profile_windows(&pwin, &fslots); evidence_windows(&jwin, &slots);
                hipLaunchKernelGGL(ambi_evidence_mark_kernel, grid, threads, scratch + (int)frag_profile_lds_bytes(fslots, pwin), s, A_, frag_args_, which, pwin, fslots, B.side, side_off);
                HIP_CK(hipGetLastError());
                hipLaunchKernelGGL(ambi_evidence_scan_kernel, grid, threads, scratch + (int)evidence_scan_lds_bytes(slots, kProfileThreads), s, A_, which, jwin, slots, B.side, side_off, B.d, off);
                break;
            }
            case kFold: {   // (the scan kernel behind the arm kernel on one stream, as above)
                int fwin, jwin, slots; fold_windows(&fwin, &jwin, &slots);
                hipLaunchKernelGGL(ambi_fold_arm_kernel, grid, threads, scratch + (int)fold_arm_lds_bytes(fwin), s, A_, which, fwin, B.side, plane_bytes_, side_off);
                HIP_CK(hipGetLastError());
                hipLaunchKernelGGL(ambi_fold_scan_kernel, grid, threads, scratch + (int)fold_scan_lds_bytes(slots), s, A_, which, jwin, slots, B.side, plane_bytes_, side_off, B.d, off);
                break;
            }
            case kCompare: {   // (a workgroup per pair; a request without pairs launches nothing)
                const PairRequest& Q = pair_of(kind);
                if (Q.n() > 0) hipLaunchKernelGGL(ambi_path_compare_kernel, dim3(compare_grid()), threads, scratch + (int)compare_lds_bytes(Q.dmax), s, A_, given_args_[kind - kCompare],
                                                  reinterpret_cast<const int32_t*>(off), Q.n(), Q.dmax, reinterpret_cast<PathCompare*>(B.d));
                break;
            }
            case kAlign: {   // (a workgroup and a history area per pair in flight; a request without pairs launches nothing)
                const PairRequest& Q = pair_of(kind);
                if (Q.n() > 0) hipLaunchKernelGGL(ambi_path_align_kernel, dim3(align_grid_of()), threads, scratch + (int)align_lds_bytes(Q.dmax), s, A_, given_args_[kind - kCompare],
                                                  reinterpret_cast<const int32_t*>(off), Q.n(), Q.dmax, B.side, align_history_bytes(Q.dmax), reinterpret_cast<PathAlign*>(B.d),
                                                  reinterpret_cast<AlignRun*>(B.d + align_runs_off(Q.n())));
                break;
            }
            case kCoords: {   // (the lift kernel behind the scan on one stream; a request without queries launches the scan alone)
                const int64_t n = coords_queries();
                hipLaunchKernelGGL(ambi_path_coords_kernel, grid, threads, scratch, s, A_, len_args_, which, B.side, off, B.d);
                HIP_CK(hipGetLastError());
                if (n > 0) hipLaunchKernelGGL(ambi_path_lift_kernel, dim3(lift_grid_of(kProfileThreads)), threads, 0, s, A_, len_args_, which, B.side, off, B.d,
                                              reinterpret_cast<const LiftQuery*>(side_off), n, reinterpret_cast<PathLift*>(B.d + coords_results_off(U)));
                break;
            }
        }
        HIP_CK(hipGetLastError());
        // 5. copy: the block to its twin on the lease's copy stream
        HIP_CK(hipEventRecord(B.ev_packed, s));
        HIP_CK(hipStreamWaitEvent(L->copy_stream, B.ev_packed, 0));
        HIP_CK(hipMemcpyAsync(B.h, B.d, (size_t)P.bytes, hipMemcpyDeviceToHost, L->copy_stream));
        HIP_CK(hipEventRecord(B.ev_done, L->copy_stream));
        R.which = which; R.stream = s; R.epoch = epoch_; R.queued = true;
        P.view = nullptr;
        return 0;
    }
    int profile(ProfileKind kind, int which, void* stream) override {
        DeviceGuard dg_(device_);
        if (!ran_ || !lease_ || which < 0 || which > 1) return ST_ERR_BAD_INPUT;
        prof_hb_ = hbp_;
        return profile_queue(kind, which, (hipStream_t)stream);
    }
    int profile_wait(ProfileKind kind) override {
        DeviceGuard dg_(device_);
        const Request& R = req_[kind];
        if (!R.queued) return ST_ERR_BAD_INPUT;
        if (int rc = wait()) return rc;
        if (epoch_ != R.epoch) { if (int rc = profile_queue(kind, R.which, R.stream)) return rc; }
        HIP_CK(hipEventSynchronize(lease_->prof[kind].ev_done));
        prof_[kind].view = lease_->prof[kind].h;
        return 0;
    }
    int profile_device(ProfileKind kind, void** ptr, int64_t* bytes) override {
        if (!prof_[kind].view || !lease_) return ST_ERR_BAD_INPUT;
        if (ptr) *ptr = lease_->prof[kind].d;
        if (bytes) *bytes = prof_[kind].bytes;
        return 0;
    }
    // the evidence kind's depth area: a range of one unit's depths to the host (everything queued is complete: profile_wait has
    // returned), and the area itself
    int evidence_depth_copy(int unit, int64_t first, int64_t n, int32_t* out) override {
        DeviceGuard dg_(device_);
        if (!prof_[kEvidence].view || !lease_ || !lease_->prof[kEvidence].side || unit < 0 || unit >= (int)depth_off_.size() || n < 0 || (n > 0 && !out)) return ST_ERR_BAD_INPUT;
        if (n > 0) HIP_CK(hipMemcpy(out, lease_->prof[kEvidence].side + depth_off_[(size_t)unit] + 4 * first, (size_t)(4 * n), hipMemcpyDeviceToHost));
        return 0;
    }
    int evidence_depth_device(void** ptr, int64_t* bytes, int64_t* unit_off, int cap) override {
        if (!prof_[kEvidence].view || !lease_) return ST_ERR_BAD_INPUT;
        if (ptr) *ptr = lease_->prof[kEvidence].side;
        return evidence_depth_offsets(bytes, unit_off, cap);
    }
    // the fold kind's planes: a range of one unit's plane to the host, and the area itself
    int fold_plane_copy(int unit, int plane, int64_t first, int64_t n, int32_t* out) override {
        DeviceGuard dg_(device_);
        if (!prof_[kFold].view || !lease_ || !lease_->prof[kFold].side || unit < 0 || unit >= (int)plane_off_.size() || plane < 0 || plane > 1 || n < 0 || (n > 0 && !out)) return ST_ERR_BAD_INPUT;
        if (n > 0) HIP_CK(hipMemcpy(out, lease_->prof[kFold].side + plane * plane_bytes_ + plane_off_[(size_t)unit] + 4 * first, (size_t)(4 * n), hipMemcpyDeviceToHost));
        return 0;
    }
    int fold_planes_device(void** ptr, int64_t* bytes, int64_t* unit_off, int cap) override {
        if (!prof_[kFold].view || !lease_) return ST_ERR_BAD_INPUT;
        if (ptr) *ptr = lease_->prof[kFold].side;
        return fold_plane_offsets(bytes, unit_off, cap);
    }
    // the coords kind's plane: a range of one unit's offsets to the host, and the area itself
    int coords_copy(int unit, int64_t first, int64_t n, int64_t* out) override {
        DeviceGuard dg_(device_);
        if (!prof_[kCoords].view || !lease_ || !lease_->prof[kCoords].side || unit < 0 || unit >= (int)cplane_off_.size() || n < 0 || (n > 0 && !out)) return ST_ERR_BAD_INPUT;
        if (n > 0) HIP_CK(hipMemcpy(out, lease_->prof[kCoords].side + cplane_off_[(size_t)unit] + 8 * first, (size_t)(8 * n), hipMemcpyDeviceToHost));
        return 0;
    }
    int coords_device(void** ptr, int64_t* bytes, int64_t* unit_off, int cap) override {
        if (!prof_[kCoords].view || !lease_) return ST_ERR_BAD_INPUT;
        if (ptr) *ptr = lease_->prof[kCoords].side;
        return coords_plane_offsets(bytes, unit_off, cap);
    }
    // ---- nucleotide sequence of the paths (ambi_sequence.hpp) ----
    // sequence() works on `stream` behind everything that writes the result blob in the last run (behind_results): the
    // sequence image if the device does not hold this version of it (pinned twin, one copy), pass 0 of the extents kernel, the
    // totals to the pinned twin and ONE stream synchronisation -- the small device-to-host trip that sizes the extent arrays and the
    // output block (an on-request call: the run it follows is complete by then) -- the three offset tables up, pass 1 and the fill
    // kernel.  sequence_wait() makes the results final (wait()) and, if that moved their epoch, does all of it once more.
    bool seq_busy_ = false, seq_timed_ = false;
    int64_t seq_img_version_ = -1, seq_epoch_ = -1, seq_max_ = 0;
    int seq_which_ = 1; hipStream_t seq_stream_ = nullptr;
    SeqArgs seq_args_{};
    int sequence_image(hipStream_t s) {
        Lease* L = lease_;
        const SeqImage& I = hb().seq;
        const int64_t U = (int64_t)hb().units.size();
        if ((int64_t)I.store_off.size() != U || (int64_t)I.pos_off.size() != U) return ST_ERR_BAD_INPUT;   // (not sealed)
        const int64_t b0 = pad16((int64_t)I.bases.size()), b1 = b0 + 8 * (int64_t)I.seg_pos.size(), b2 = b1 + 8 * U, total = b2 + 8 * U;
        if (seq_img_version_ != I.version || !L->d_seq_img) {
            if (int rc = lease_device_block(&L->d_seq_img, &L->d_seq_img_bytes, total)) return rc;
            if (int rc = lease_pinned_block(&L->h_seq, nullptr, &L->h_seq_bytes, std::max<int64_t>(total, 40 * U + 64))) return rc;
            if (!I.bases.empty()) memcpy(L->h_seq, I.bases.data(), I.bases.size());
            memcpy(L->h_seq + b0, I.seg_pos.data(), 8 * I.seg_pos.size());
            memcpy(L->h_seq + b1, I.store_off.data(), (size_t)(8 * U));
            memcpy(L->h_seq + b2, I.pos_off.data(), (size_t)(8 * U));
            HIP_CK(hipMemcpyAsync(L->d_seq_img, L->h_seq, (size_t)total, hipMemcpyHostToDevice, s));
            seq_img_version_ = I.version;
        }
        seq_args_ = SeqArgs{L->d_seq_img, reinterpret_cast<const int64_t*>(L->d_seq_img + b0), reinterpret_cast<const int64_t*>(L->d_seq_img + b1),
                            reinterpret_cast<const int64_t*>(L->d_seq_img + b2)};
        return 0;
    }
    int sequence_queue(int which, int first, int count, int64_t max_bytes, hipStream_t s) {
        Lease* L = lease_;
        for (hipEvent_t* e : {&L->ev_seq_src, &L->ev_seq_done}) if (!*e) HIP_CK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        // an earlier request nobody waited for still uses the blocks, and its table upload reads the pinned twin the host writes below
        if (seq_busy_) { HIP_CK(hipEventSynchronize(L->ev_seq_done)); seq_busy_ = false; }
        seq_state_ = 0; seq_queued_ = false;
        seq_which_ = which; seq_first_ = first; seq_count_ = count; seq_max_ = max_bytes; seq_stream_ = s; seq_epoch_ = epoch_;
        if (int rc = sequence_image(s)) return rc;
        if (int rc = behind_results(s, L->ev_seq_src)) return rc;
        // working block: [totals: 2 count] [ext_off: count + 1] [out_off: count] [tile_off: count + 1] | [ext_src: slots] [ext_out: slots]
        const int64_t c = count, tab = 16 * c, head = pad16(tab + 8 * (3 * c + 2));
        if (int rc = lease_device_block(&L->d_seq_work, &L->d_seq_work_bytes, head)) return rc;
        SeqPlan Q{};
        Q.first = first; Q.count = count; Q.totals = reinterpret_cast<int64_t*>(L->d_seq_work);
        const int ugrid = (int)(c < 16384 ? c : 16384);
        seq_timed_ = timing_;
        if (seq_timed_) { for (int k = 0; k < 5; k++) if (!L->ev_seq_t[k]) HIP_CK(hipEventCreate(&L->ev_seq_t[k])); HIP_CK(hipEventRecord(L->ev_seq_t[0], s)); }
        hipLaunchKernelGGL(ambi_seq_extents_kernel, dim3(ugrid), dim3(kSeqTileLanes), 0, s, A_, seq_args_, Q, which, 0);
        HIP_CK(hipGetLastError());
        if (seq_timed_) HIP_CK(hipEventRecord(L->ev_seq_t[1], s));
        seq_busy_ = true;
        HIP_CK(hipMemcpyAsync(L->h_seq, L->d_seq_work, (size_t)tab, hipMemcpyDeviceToHost, s));
        HIP_CK(hipStreamSynchronize(s));
        seq_busy_ = false;
        seq_layout(reinterpret_cast<const int64_t*>(L->h_seq), count, seq_lay_);
        seq_state_ = 1;
        if (max_bytes > 0 && seq_lay_.seq_bytes > max_bytes) return kSeqTooLarge;
        // (s is idle and nothing of an earlier request is in flight: the blocks may move)
        if (int rc = lease_device_block(&L->d_seq_work, &L->d_seq_work_bytes, head + 16 * seq_lay_.slots)) return rc;
        if (int rc = lease_device_block(&L->d_seq_out, &L->d_seq_out_bytes, seq_lay_.out_bytes + 16)) return rc;
        int64_t* ht = reinterpret_cast<int64_t*>(L->h_seq + tab);
        memcpy(ht, seq_lay_.ext_off.data(), (size_t)(8 * (c + 1)));
        memcpy(ht + c + 1, seq_lay_.out_off.data(), (size_t)(8 * c));
        memcpy(ht + 2 * c + 1, seq_lay_.tile_off.data(), (size_t)(8 * (c + 1)));
        // (the totals travel back with the tables: growing the working block above has dropped the device's copy)
        HIP_CK(hipMemcpyAsync(L->d_seq_work, L->h_seq, (size_t)(tab + 8 * (3 * c + 2)), hipMemcpyHostToDevice, s));
        int64_t* dt = reinterpret_cast<int64_t*>(L->d_seq_work + tab);
        Q.totals = reinterpret_cast<int64_t*>(L->d_seq_work);
        Q.ext_off = dt; Q.out_off = dt + c + 1; Q.tile_off = dt + 2 * c + 1;
        Q.ext_src = reinterpret_cast<int64_t*>(L->d_seq_work + head); Q.ext_out = Q.ext_src + seq_lay_.slots;
        Q.out = L->d_seq_out; Q.out_bytes = seq_lay_.out_bytes;
        if (seq_timed_) HIP_CK(hipEventRecord(L->ev_seq_t[2], s));
        hipLaunchKernelGGL(ambi_seq_extents_kernel, dim3(ugrid), dim3(kSeqTileLanes), 0, s, A_, seq_args_, Q, which, 1);
        HIP_CK(hipGetLastError());
        if (seq_timed_) HIP_CK(hipEventRecord(L->ev_seq_t[3], s));
        if (seq_lay_.tiles > 0) {
            const int64_t fgrid = seq_lay_.tiles < 4096 ? seq_lay_.tiles : 4096;   // (16 workgroups per CU; a workgroup builds its table once)
            hipLaunchKernelGGL(ambi_seq_fill_kernel, dim3((unsigned)fgrid), dim3(kSeqTileLanes), 0, s, seq_args_, Q, seq_lay_.tiles);
            HIP_CK(hipGetLastError());
        }
        if (seq_timed_) HIP_CK(hipEventRecord(L->ev_seq_t[4], s));
        HIP_CK(hipEventRecord(L->ev_seq_done, s));
        seq_busy_ = true; seq_queued_ = true;
        return 0;
    }
    int sequence(int which, int first, int count, int64_t max_bytes, void* stream) override {
        DeviceGuard dg_(device_);
        seq_state_ = 0; seq_queued_ = false;
        if (!ran_ || !lease_ || !hb().seq.any || which < 0 || which > 1 || first < 0 || count < 1 || (size_t)first + (size_t)count > hb().units.size()) return ST_ERR_BAD_INPUT;
        prof_hb_ = hbp_;
        return sequence_queue(which, first, count, max_bytes, (hipStream_t)stream);
    }
    int sequence_wait() override {
        DeviceGuard dg_(device_);
        if (seq_state_ < 1 || !seq_queued_) return ST_ERR_BAD_INPUT;
        if (int rc = wait()) return rc;
        if (epoch_ != seq_epoch_) { if (int rc = sequence_queue(seq_which_, seq_first_, seq_count_, seq_max_, seq_stream_)) return rc; }
        HIP_CK(hipEventSynchronize(lease_->ev_seq_done));
        seq_busy_ = false;
        seq_state_ = 2;
        if (seq_timed_) {
            // the extents kernel's figure is the SUM of its two launches (pass 0 + pass 1)
            float p0 = -1.f, p1 = -1.f, fill = -1.f;
            if (hipEventElapsedTime(&p0, lease_->ev_seq_t[0], lease_->ev_seq_t[1]) != hipSuccess) p0 = -1.f;
            if (hipEventElapsedTime(&p1, lease_->ev_seq_t[2], lease_->ev_seq_t[3]) != hipSuccess) p1 = -1.f;
            if (hipEventElapsedTime(&fill, lease_->ev_seq_t[3], lease_->ev_seq_t[4]) != hipSuccess) fill = -1.f;
            const float ext = (p0 >= 0 && p1 >= 0) ? p0 + p1 : -1.f;
            (void)hipGetLastError();
            while (!times_.empty() && !strncmp(times_.back().name, "ambi_seq_", 9)) times_.pop_back();
            times_.push_back({"ambi_seq_extents_kernel", ext});
            times_.push_back({"ambi_seq_fill_kernel", fill});
        }
        return 0;
    }
    int sequence_copy(int unit, int64_t first, int64_t count, uint8_t* out) override {
        DeviceGuard dg_(device_);
        const int r = unit - seq_first_;
        if (seq_state_ < 2 || !lease_ || r < 0 || r >= seq_count_ || first < 0 || count < 0 || first + count > seq_lay_.len[(size_t)r] || (count > 0 && !out)) return ST_ERR_BAD_INPUT;
        if (count > 0) HIP_CK(hipMemcpy(out, lease_->d_seq_out + seq_lay_.out_off[(size_t)r] + first, (size_t)count, hipMemcpyDeviceToHost));
        return 0;
    }
    int sequence_device(void** ptr, int64_t* bytes, int64_t* unit_off, int cap) override {
        if (seq_state_ < 2 || !lease_ || !prof_hb_) return ST_ERR_BAD_INPUT;
        if (ptr) *ptr = lease_->d_seq_out;
        return sequence_offsets(bytes, unit_off, cap);
    }
    int copy_orders(int unit, int64_t first, int64_t count, uint8_t* out) override {
        DeviceGuard dg_(device_);
        if (int rc = wait()) return rc;
        if (int rc = materialise_tables()) return rc;
        UnitOut h;
        HIP_CK(hipMemcpy(&h, d_results_ + sizeof(UnitOut) * (size_t)unit, sizeof(UnitOut), hipMemcpyDeviceToHost));
        if (h.order_off < 0 || first < 0 || first + count > h.num_orders) return ST_ERR_BAD_INPUT;
        // rows are row_stride(K) bytes apart on the device; the caller gets count x K
        const int stride = row_stride(h.K);
        std::vector<uint8_t> tmp((size_t)(count * stride));
        HIP_CK(hipMemcpy(tmp.data(), d_arena_ + h.order_off + first * stride, tmp.size(), hipMemcpyDeviceToHost));
        // (Lehmer codes up to 63 nodes, a byte per node above: row_unpack decodes either)
        for (int64_t r = 0; r < count; r++) row_unpack(tmp.data() + r * stride, h.K, out + r * h.K);
        return 0;
    }
    int copy_debug_order(int unit, uint8_t* out) override {
        DeviceGuard dg_(device_);
        if (int rc = wait()) return rc;
        const HostBatch& H = hb();
        const int64_t slot = (H.inject.empty() || !d_inject_) ? -1 : H.inject_off[kInjectStride * (size_t)unit + 2];
        if (slot < 0) return ST_ERR_BAD_INPUT;
        HIP_CK(hipMemcpy(out, d_inject_ + slot * kDebugOrderBytes, kDebugOrderBytes, hipMemcpyDeviceToHost));
        return 0;
    }
    int copy_dag(int unit, Dag* out) override {
        DeviceGuard dg_(device_);
        HIP_CK(hipMemcpy(out, d_dags_ + unit, sizeof(Dag), hipMemcpyDeviceToHost));
        return 0;
    }
    int copy_dag_wide(int unit, int32_t* pat, int32_t* loop, uint64_t* succ2) override {
        DeviceGuard dg_(device_);
        if (unit < 0 || unit >= (int)hb().units.size() || hb().wide_index[unit] < 0) return ST_ERR_BAD_INPUT;
        const WideUnit* X = d_wide_ + hb().wide_index[unit];
        const uint8_t* base = reinterpret_cast<const uint8_t*>(X);
        HIP_CK(hipMemcpy(pat, base + offsetof(WideUnit, dag) + offsetof(WideDag, pat), sizeof(int32_t) * kWideNodeCap * 3, hipMemcpyDeviceToHost));
        HIP_CK(hipMemcpy(loop, base + offsetof(WideUnit, dag) + offsetof(WideDag, loop), sizeof(int32_t) * kWideNodeCap * 3, hipMemcpyDeviceToHost));
        HIP_CK(hipMemcpy(succ2, base + offsetof(WideUnit, succ), sizeof(WideSet) * kWideNodeCap, hipMemcpyDeviceToHost));
        return 0;
    }
    void set_timing(bool on) override { timing_ = on; timing_mask_ = ~0u; timed_runs_ = 0; }
    void set_timing_mask(uint32_t mask) override { timing_ = mask != 0; timing_mask_ = mask; timed_runs_ = 0; }
    const std::vector<KernelTime>& kernel_times() override { return times_; }
    int64_t order_bytes_written() const override { return last_needed_; }
    size_t object_bytes() const override { return sizeof(HipBackend); }

    // ---- --all (LGM.cpp:3672-3695): every valid order of every unit, in the reference's print order ----
    // pass 0 = the first orientation (forward unless --reversed), pass 1 = the flipped one, run only for units whose LAST
    // order of pass 0 is invalid (LGM.cpp:3691-3695).  Device-side and batched: at wait() ONE launch per pass over all
    // (unit, 64-order chunk) work items (ambi_all_kernel: fused unrank + evaluate), validity bitmaps of R bits per pass
    // and unit stay in HBM, the host reads the per-unit counts (one copy) and a unit's bitmap only when its indices are
    // asked for; the paths are produced on demand by all_paths().
    int compute_all() {
        epoch_++;   // (the finalize kernel rewrites `evaluated` and the statuses of units with an undefined order)
        const int U = (int)hb().units.size();
        std::vector<UnitOut> hdr(U);
        HIP_CK(hipMemcpy(hdr.data(), d_results_, U * sizeof(UnitOut), hipMemcpyDeviceToHost));
        const AllPlan plan = all_plan(hdr.data(), U, all_off_);
        all_R_.resize(U);
        for (int u = 0; u < U; u++) all_R_[u] = hdr[u].num_orders;
        all_cache_.assign(U, {});
        all_idx_[0].assign(U, {}); all_idx_[1].assign(U, {});
        all_counts_.assign(2 * (size_t)U, 0);
        const int64_t words = plan.words, chunks = words / 2, pool_words = plan.pool_words;
        if (d_all_bits_ && all_bits_cap_ < pool_words) { (void)hipFree(d_all_bits_); d_all_bits_ = nullptr; }
        if (!d_all_off_) { if (int rc = dalloc(&d_all_off_, (size_t)U + 1)) return rc; if (int rc = dalloc(&d_all_count_, 2 * (size_t)U)) return rc; }
        if (!d_all_bits_) { HIP_CK(hipMalloc((void**)&d_all_bits_, (size_t)pool_words * sizeof(uint64_t))); all_bits_cap_ = pool_words; }
        d_all_flags_ = reinterpret_cast<int32_t*>(d_all_bits_ + words);
        all_pool_bytes_ = plan.pool_bytes;
        HIP_CK(hipMemcpyAsync(d_all_off_, all_off_.data(), (U + 1) * sizeof(int64_t), hipMemcpyHostToDevice, stream_));
        HIP_CK(hipMemsetAsync(d_all_bits_, 0, (size_t)pool_words * sizeof(uint64_t), stream_));
        HIP_CK(hipMemsetAsync(d_all_count_, 0, 2 * (size_t)U * sizeof(int32_t), stream_));
        bind(A_.flags);
        all_kernel_ms_ = -1.f;
        if (chunks > 0) {
            const int wave_lds = (int)((lds_first_ + 64 * kFirstRowStride + 15) & ~15);
            const int waves = (4 * wave_lds <= 64 * 1024) ? 4 : ((2 * wave_lds <= 150 * 1024) ? 2 : 1);
            int64_t nblk = (chunks + waves - 1) / waves;
            if (nblk > (1 << 20)) nblk = 1 << 20;   // grid-stride beyond
            EventPair ev;
            hipEvent_t& ea = ev.a; hipEvent_t& eb = ev.b;
            if (timing_) { HIP_CK(hipEventCreate(&ea)); HIP_CK(hipEventCreate(&eb)); HIP_CK(hipEventRecord(ea, stream_)); }
            // units with a short breakpoint path (the rule): one thread per order; the others: one wavefront per order
            const int lane_cap = all_lane_cap();
            int lanes_units = 0, wave_units = 0;
            for (int u = 0; u < U; u++) if (all_off_[u + 1] > all_off_[u]) { if (all_lane_unit(hb().units[u], lane_cap)) lanes_units++; else wave_units++; }
            const AllLaneGeom geom = all_lane_geom(hb().units, hb().max_n, lane_cap);
            int lane_waves = 1;   // wavefronts per workgroup (measured 1 / 2 / 4 = 563 / 553 / 379 M orders/s: group-memory allocation granularity)
            { const char* e = ambi_env("AMBI_ALL_WAVES"); if (e && atoi(e) >= 1 && atoi(e) <= 4) lane_waves = atoi(e); }
            int64_t lblk = (chunks + lane_waves - 1) / lane_waves;
            if (lblk > (1 << 20)) lblk = 1 << 20;
            for (int pass = 0; pass < 2; pass++) {
                if (lanes_units) hipLaunchKernelGGL(ambi_all_lanes_kernel, dim3((unsigned)lblk), dim3(64 * lane_waves), lane_waves * geom.wave_lds, stream_, A_, geom, pass, chunks, lane_cap);
                if (wave_units) hipLaunchKernelGGL(ambi_all_kernel, dim3((unsigned)nblk), dim3(64 * waves), waves * wave_lds, stream_, A_, pass, wave_lds, chunks, lane_cap);
            }
            if (timing_) HIP_CK(hipEventRecord(eb, stream_));
            hipLaunchKernelGGL(ambi_all_finalize_kernel, dim3((U + 255) / 256), dim3(256), 0, stream_, A_);
            HIP_CK(hipGetLastError());
            HIP_CK(hipMemcpyAsync(all_counts_.data(), d_all_count_, 2 * (size_t)U * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
            HIP_CK(hipStreamSynchronize(stream_));
            if (timing_) (void)hipEventElapsedTime(&all_kernel_ms_, ea, eb);
        }
        return 0;
    }
    // --all over several ranks: which chunks this rank evaluates; the pool the ranks merge; counts / headers after the merge
    int set_shard(int rank, int world) override {
        if (world < 1 || rank < 0 || rank >= world) return ST_ERR_BAD_INPUT;
        all_rank_ = rank; all_world_ = world;
        return 0;
    }
    int all_device(void** ptr, int64_t* bytes) override {
        if (ptr) *ptr = d_all_bits_;
        if (bytes) *bytes = d_all_bits_ ? all_pool_bytes_ : 0;
        return 0;
    }
    int all_finish() override {
        DeviceGuard dg_(device_);
        if (!d_all_bits_) return 0;
        const int U = (int)hb().units.size();
        hipLaunchKernelGGL(ambi_all_finalize_kernel, dim3((U + 255) / 256), dim3(256), 0, stream_, A_);
        HIP_CK(hipGetLastError());
        HIP_CK(hipMemcpyAsync(all_counts_.data(), d_all_count_, 2 * (size_t)U * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
        HIP_CK(hipStreamSynchronize(stream_));
        all_cache_.assign(U, {});
        all_idx_[0].assign(U, {}); all_idx_[1].assign(U, {});
        return 0;
    }
    // valid order indices of one pass of a unit, from its bitmap (fetched once per unit)
    int all_indices(int unit, int pass, const std::vector<int64_t>** out) {
        if (all_cache_[unit].empty() && all_off_[unit + 1] > all_off_[unit]) {
            all_cache_[unit].resize((size_t)(all_off_[unit + 1] - all_off_[unit]));
            HIP_CK(hipMemcpy(all_cache_[unit].data(), d_all_bits_ + all_off_[unit], all_cache_[unit].size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
            const int64_t nw = all_words(all_R_[unit]);
            for (int ps = 0; ps < 2; ps++) all_bits_to_indices(all_cache_[unit].data() + ps * nw, nw, all_idx_[ps][unit]);
        }
        *out = &all_idx_[pass][unit];
        return 0;
    }
    int all_count(int unit, int pass, int64_t* count) override {
        if (pass < 0 || pass > 1 || unit < 0) { if (count) *count = 0; return ST_ERR_BAD_INPUT; }
        if (count) *count = (size_t)(2 * unit + pass) < all_counts_.size() ? (int64_t)all_counts_[2 * (size_t)unit + pass] : 0;
        return 0;
    }
    int all_orders(int unit, int pass, int64_t first, int64_t count, int64_t* idx) override {
        DeviceGuard dg_(device_);
        if (pass < 0 || pass > 1 || unit < 0 || unit >= (int)all_idx_[pass].size()) return ST_ERR_BAD_INPUT;
        const std::vector<int64_t>* vp = nullptr;
        if (int rc = all_indices(unit, pass, &vp)) return rc;
        const auto& v = *vp;
        if (first < 0 || count < 0 || first + count > (int64_t)v.size()) return ST_ERR_BAD_INPUT;
        for (int64_t i = 0; i < count; i++) idx[i] = v[first + i];
        return 0;
    }
    int all_paths(int unit, int pass, int64_t first, int64_t count, int32_t* lengths, int32_t* cells, int64_t stride) override {
        DeviceGuard dg_(device_);
        if (pass < 0 || pass > 1 || unit < 0 || unit >= (int)all_idx_[pass].size()) return ST_ERR_BAD_INPUT;
        const std::vector<int64_t>* vp = nullptr;
        if (int rc = all_indices(unit, pass, &vp)) return rc;
        const auto& v = *vp;
        if (first < 0 || count < 0 || first + count > (int64_t)v.size() || stride <= 0) return ST_ERR_BAD_INPUT;
        if (count == 0) return 0;
        const UnitIn& Uin = hb().units[unit];
        const bool fwd0 = !(A_.flags & FLAG_REVERSED), fwd = pass == 0 ? fwd0 : !fwd0;
        DevBuf b_idx, b_len, b_cells;
        HIP_CK(b_idx.alloc((size_t)count * sizeof(int64_t)));
        HIP_CK(b_len.alloc((size_t)count * sizeof(int32_t)));
        HIP_CK(b_cells.alloc((size_t)count * (size_t)stride * sizeof(int32_t)));
        int64_t* d_idx = b_idx.as<int64_t>(); int32_t* d_len = b_len.as<int32_t>(); int32_t* d_cells = b_cells.as<int32_t>();
        HIP_CK(hipMemcpy(d_idx, v.data() + first, (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice));
        const int lds = (int)order_path_work_bytes(Uin);
        hipLaunchKernelGGL(ambi_order_paths_kernel, dim3((unsigned)count), dim3(64), lds, stream_, A_, unit, fwd ? 1 : 0, (const int64_t*)d_idx, d_len,
                           d_cells, stride);
        HIP_CK(hipGetLastError());
        HIP_CK(hipMemcpyAsync(lengths, d_len, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
        HIP_CK(hipMemcpyAsync(cells, d_cells, (size_t)count * (size_t)stride * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
        HIP_CK(hipStreamSynchronize(stream_));
        return 0;
    }
};

Backend* make_backend() { return new HipBackend(); }

// ILP entries on the device (LocalGenomicMap::BFB_ILP, LGM.cpp:4397-4752: int32 column + f64 coefficient per non-zero, 56.5 M
// non-zeros = 0.68 GB at 256 segments).  The non-zero space is cut into chunks of 1024 consecutive positions, one workgroup each, and
// every thread owns FOUR consecutive positions: one 16-byte store of columns and two of coefficients per thread, 1 KB + 2 KB
// contiguous per wavefront, every lane busy.  Rows differ in length by three orders of magnitude (2 n^2 / 3 entries for a segment row,
// one for the innermost nesting rows), so positions, not rows, are dealt out: the host names the first row of every chunk (a merge
// walk, O(rows + chunks)), the workgroup stages the offsets and descriptors of the rows that reach into its chunk in group memory
// (at most 1025), a thread finds its row by bisection there; when its four positions lie in one row (almost always) the row family is
// decided once and the four entries share the piece bounds and the triangle arithmetic (ilp_row_entries<4>), else entry by entry.
// What bounds it (profiles/r04_notes.md): NOT the stores -- a plain two-array store stream of this very shape runs at 5.76 TB/s
// (profiles/tools/hbm_write_two_streams.hip), this kernel at 3.4-3.6 -- but instructions per entry: 65.7 M vector instructions in the
// entry-by-entry form = 122 us of issue time alone.  Rounds 1-3 (one entry per thread, 4- / 8-byte stores) and a form with one
// wavefront-uniform row piece per step (scalar family dispatch, half the lanes idle on the short pieces) measure 0.190-0.199 and 0.22 ms.
#ifndef AMBI_ILP_PER
#define AMBI_ILP_PER 4
#endif
constexpr int kIlpChunk = 1024, kIlpStage = kIlpChunk + 4, kIlpPer = AMBI_ILP_PER, kIlpThreads = kIlpChunk / kIlpPer;   // entries per thread (4 or 8), threads per workgroup
static_assert(kIlpPer == 4 || kIlpPer == 8, "the 16-byte stores below take the entries of a thread four columns / two coefficients at a time");
// JOINT: the rows may be those of the joint model of `--op sc_bfb` (BFB_ILP_SC; descriptor layout in ambi_ilp_rows.hpp) -- the same chunked
// fill with the column fix-up per entry; its linking rows are three entries long, so the entry-by-entry branch serves them (under 1 % of the
// entries).  JOINT = false is the single-graph kernel, instruction for instruction what it was before the joint rows existed.
template <bool JOINT>
__global__ __launch_bounds__(kIlpThreads) void ambi_ilp_fill_kernel(const IlpRowDesc* rows, const int64_t* row_ptr, const int32_t* chunk_row, int64_t nnz, IlpGeom G,
                                                            const int32_t* lit_col, const double* lit_val, int32_t* col, double* val) {
    __shared__ int32_t rel[kIlpStage];          // row offsets relative to the chunk's first position (rows are far shorter than 2^31)
    __shared__ IlpRowDesc desc[kIlpStage];
    const int64_t P0 = (int64_t)blockIdx.x * kIlpChunk;
    const int r_lo = chunk_row[blockIdx.x], R = chunk_row[blockIdx.x + 1] - r_lo + 1;   // rows r_lo .. r_lo + R - 1 reach into the chunk
    for (int i = threadIdx.x; i <= R; i += blockDim.x) {
        const int64_t d = row_ptr[r_lo + i] - P0;
        rel[i] = (int32_t)(d > (int64_t)0x3fffffff ? (int64_t)0x3fffffff : d);
    }
    for (int i = threadIdx.x; i < R; i += blockDim.x) desc[i] = rows[r_lo + i];
    __syncthreads();
    const int p = kIlpPer * (int)threadIdx.x;
    const int64_t left = nnz - P0;
    const int lim = left < (int64_t)kIlpChunk ? (int)left : kIlpChunk;   // positions of this chunk that exist
    if (p >= lim) return;
    int lo = 0, hi = R;                         // last staged row that starts at or before p
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (rel[mid] <= p) lo = mid; else hi = mid; }
    int r = lo;
    while (p >= rel[r + 1]) r++;                // (empty rows are stepped over)
    int32_t c4[kIlpPer]; double v4[kIlpPer];
#pragma unroll
    for (int k = 0; k < kIlpPer; k++) { c4[k] = 0; v4[k] = 0; }
    const int want = lim - p < kIlpPer ? lim - p : kIlpPer;
#if defined(AMBI_ILP_NOCOMPUTE)   // timing experiment: the stores without the entries
    if (true) { for (int k = 0; k < kIlpPer; k++) { c4[k] = p + k + r; v4[k] = 1.0; } }
#else
    if (want == kIlpPer && rel[r + 1] - p >= kIlpPer) ilp_row_entries<kIlpPer, JOINT>(desc[r], G, p - rel[r], kIlpPer, lit_col, lit_val, c4, v4);
#endif
    else {
#pragma unroll
        for (int k = 0; k < kIlpPer; k++) {
            const int q = p + k;
            if (k < want) {
                while (q >= rel[r + 1]) r++;
                ilp_row_entry<JOINT>(desc[r], G, (int64_t)(q - rel[r]), lit_col, lit_val, &c4[k], &v4[k]);
            }
        }
    }
    if (want == kIlpPer) {
#pragma unroll
        for (int k = 0; k < kIlpPer; k += 4) *reinterpret_cast<int4*>(col + P0 + p + k) = make_int4(c4[k], c4[k + 1], c4[k + 2], c4[k + 3]);
#pragma unroll
        for (int k = 0; k < kIlpPer; k += 2) *reinterpret_cast<double2*>(val + P0 + p + k) = make_double2(v4[k], v4[k + 1]);
    } else {
        for (int k = 0; k < want; k++) { col[P0 + p + k] = c4[k]; val[P0 + p + k] = v4[k]; }
    }
}

int backend_expand_runs(const int32_t* run_start, const int32_t* run_len, const int64_t* cell_off, int64_t n_runs, int32_t* cells,
                        int64_t cell_cap, void* stream) {
    int64_t blocks = (n_runs + 3) / 4;
    if (blocks > 65536) blocks = 65536;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(ambi_expand_runs_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, run_start, run_len, cell_off, n_runs, cells,
                       cell_cap);
    HIP_CK(hipGetLastError());
    return 0;
}

int backend_ilp_fill(const IlpRowDesc* rows, int64_t n_rows, const int64_t* row_ptr, int s, int e, const int32_t* lit_col, const double* lit_val,
                     int64_t n_lit, int32_t* col, double* val, float* kernel_ms) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return -30;   // AMBI_ERR_NO_DEVICE: no CPU fallback
    const int64_t nnz = row_ptr[n_rows];
    // the first row of every chunk of kIlpChunk positions (last row that starts at or before the chunk's first position), and the
    // last row behind the last chunk
    const int64_t n_chunks = (nnz + kIlpChunk - 1) / kIlpChunk;
    std::vector<int32_t> chunk_row((size_t)n_chunks + 1, 0);
    {
        int64_t r = 0;
        for (int64_t c = 0; c < n_chunks; c++) {
            const int64_t pos = c * kIlpChunk;
            while (r + 1 < n_rows && row_ptr[r + 1] <= pos) r++;
            chunk_row[(size_t)c] = (int32_t)r;
        }
        chunk_row[(size_t)n_chunks] = (int32_t)(n_rows > 0 ? n_rows - 1 : 0);
        for (int64_t c = 0; c < n_chunks; c++)
            if (chunk_row[(size_t)c + 1] - chunk_row[(size_t)c] + 2 > kIlpStage) return ST_ERR_BAD_INPUT;   // (more than 1024 rows inside 1024 positions: rows are not empty)
    }
    int32_t* d_chunk = nullptr;
    IlpRowDesc* d_rows = nullptr; int64_t* d_ptr = nullptr; int32_t* d_lc = nullptr; double* d_lv = nullptr; int32_t* d_col = nullptr; double* d_val = nullptr;
    HIP_CK(hipMalloc((void**)&d_rows, (size_t)(n_rows > 0 ? n_rows : 1) * sizeof(IlpRowDesc)));
    HIP_CK(hipMalloc((void**)&d_ptr, (size_t)(n_rows + 1) * sizeof(int64_t)));
    HIP_CK(hipMalloc((void**)&d_lc, (size_t)(n_lit > 0 ? n_lit : 1) * sizeof(int32_t)));
    HIP_CK(hipMalloc((void**)&d_lv, (size_t)(n_lit > 0 ? n_lit : 1) * sizeof(double)));
    HIP_CK(hipMalloc((void**)&d_col, (size_t)(nnz > 0 ? nnz : 1) * sizeof(int32_t)));
    HIP_CK(hipMalloc((void**)&d_val, (size_t)(nnz > 0 ? nnz : 1) * sizeof(double)));
    HIP_CK(hipMalloc((void**)&d_chunk, chunk_row.size() * sizeof(int32_t)));
    HIP_CK(hipMemcpy(d_chunk, chunk_row.data(), chunk_row.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_CK(hipMemcpy(d_rows, rows, (size_t)n_rows * sizeof(IlpRowDesc), hipMemcpyHostToDevice));
    HIP_CK(hipMemcpy(d_ptr, row_ptr, (size_t)(n_rows + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (n_lit > 0) { HIP_CK(hipMemcpy(d_lc, lit_col, (size_t)n_lit * sizeof(int32_t), hipMemcpyHostToDevice)); HIP_CK(hipMemcpy(d_lv, lit_val, (size_t)n_lit * sizeof(double), hipMemcpyHostToDevice)); }
    hipEvent_t ea, eb;
    HIP_CK(hipEventCreate(&ea)); HIP_CK(hipEventCreate(&eb));
    const int64_t grid = n_chunks > 0 ? n_chunks : 1;
    const int reps = kernel_ms ? 5 : 1;   // the timed figure is the mean of the last 4 of 5 launches
    const bool joint = n_rows > 0 && (rows[0].family >> 8) != 0;   // a joint model opens with a row of its first graph
    auto* kernel = joint ? ambi_ilp_fill_kernel<true> : ambi_ilp_fill_kernel<false>;
    float total = 0;
    for (int r = 0; r < reps; r++) {
        HIP_CK(hipEventRecord(ea, nullptr));
        if (n_chunks > 0)
            hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kIlpThreads), 0, nullptr, (const IlpRowDesc*)d_rows, (const int64_t*)d_ptr, (const int32_t*)d_chunk, nnz,
                               ilp_geom(s, e), (const int32_t*)d_lc, (const double*)d_lv, d_col, d_val);
        HIP_CK(hipEventRecord(eb, nullptr));
        HIP_CK(hipEventSynchronize(eb));
        float ms = 0;
        HIP_CK(hipEventElapsedTime(&ms, ea, eb));
        if (r > 0) total += ms;
    }
    HIP_CK(hipGetLastError());
    if (kernel_ms) *kernel_ms = reps > 1 ? total / (reps - 1) : 0;
    HIP_CK(hipMemcpy(col, d_col, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_CK(hipMemcpy(val, d_val, (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost));
    (void)hipEventDestroy(ea); (void)hipEventDestroy(eb);
    (void)hipFree(d_chunk); (void)hipFree(d_rows); (void)hipFree(d_ptr); (void)hipFree(d_lc); (void)hipFree(d_lv); (void)hipFree(d_col); (void)hipFree(d_val);
    return 0;
}

}  // namespace ambi
