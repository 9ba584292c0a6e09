/* ambigram_hip.h -- C ABI of libambigram_hip.so, the MI355X-native BFB path-reconstruction engine.
 *
 * Drop-in boundary for the `--op bfb` path of deepomicslab/Ambigram.  The reference has no plugin/FFI interface
 * (SURVEY.md 8b): the path is reached through C++ member calls on pointer-graph objects from main()
 * (localhap.cpp:49-388).  Each entry point below names the reference call(s) it replaces; INTEGRATION.md shows
 * the binding a maintainer adds to localhap.cpp and the ctypes stub used by ambigram_amd/.
 *
 * Conventions: plain pointers and sizes, caller-owned arrays, int32 unless noted; return 0 on success or a negative
 * code (ambi_error_string); no exceptions cross the boundary; a handle is not thread-safe, different handles are.
 * Vertices are signed ABSOLUTE segment ids: +id = (id,'+'), -id = (id,'-').
 */
#ifndef AMBIGRAM_HIP_H
#define AMBIGRAM_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMBI_ABI_VERSION 1

/* run flags */
#define AMBI_FLAG_REVERSED 1u /* --reversed (localhap.cpp:37,55) */
#define AMBI_FLAG_ALL 2u      /* --all      (localhap.cpp:38,56) */
/* Extension (no counterpart in the reference, which always materialises every topological order, LocalGenomicMap.cpp:3380-3409):
 * the run does not WRITE the order tables.  Results are identical (the scan for the first valid order reads the first orders the
 * lattice stage unranks, --all unranks in the kernel); the tables are written on demand -- when a unit's scan runs out of
 * budget and the parallel search needs them, or when ambi_batch_unit_orders asks for rows.  bench.py reports the step with
 * and without the tables (91 % of the default step's HBM bytes are this by-product). */
#define AMBI_FLAG_LAZY_ORDERS 4u

/* per-unit status (ambi_unit_result_t.status); negative values are errors */
#define AMBI_ST_OK 0
#define AMBI_ST_SHORTCUT 1        /* no fold-back inversion: path 1+..n+ (localhap.cpp:164-170) */
#define AMBI_ST_INFEASIBLE 2      /* .sol Infeasible: path 1+..n+ + "ILP is unsolvable." (localhap.cpp:213-220) */
#define AMBI_ST_NO_VALID_ORDER 3  /* no order assembles in either orientation (reference leaves the path empty) */
#define AMBI_ERR_TOO_MANY_NODES (-10)  /* more than 255 selected patterns + loops in one chromosome */
#define AMBI_ERR_NO_ELEMENTS (-11)
#define AMBI_ERR_REF_UB (-12)     /* the reference reads out of bounds on this input; refused instead of guessed */
#define AMBI_ERR_BKP_CAPACITY (-13)
#define AMBI_ERR_PATH_CAPACITY (-14)
#define AMBI_ERR_ORDERS_CAPACITY (-15)  /* the unit's order table does not fit the arena (it could not grow: out of memory, or the
                                        * limit AMBI_ARENA_MAX_BYTES of the environment); units are given rows in unit order, the
                                        * others end with this status and carry no results */
#define AMBI_ERR_IDEALS_CAPACITY (-16)
#define AMBI_ERR_BAD_INPUT (-17)
#define AMBI_ERR_OUTJUNC_CAPACITY (-18)
/* host / runtime errors */
#define AMBI_ERR_OPEN (-1)
#define AMBI_ERR_MALFORMED (-2)
#define AMBI_ERR_UNKNOWN_SEG (-3)
#define AMBI_ERR_SOURCE_SINK (-4)
#define AMBI_ERR_PLOIDY (-5)
#define AMBI_ERR_SEG_IDS (-6)
#define AMBI_ERR_SOL_OPEN (-7)
#define AMBI_ERR_LINE_TOO_LONG (-8)
#define AMBI_ERR_UNSUPPORTED (-9)
#define AMBI_ERR_NO_DEVICE (-30)  /* no HIP device: the engine has NO CPU fallback */
#define AMBI_ERR_HIP (-31)
#define AMBI_ERR_STATE (-32)      /* call order violated (e.g. run before upload) */
#define AMBI_ERR_ARG (-33)
#define AMBI_ERR_TOO_LARGE (-34)  /* ambi_batch_sequence: the unit range's sequences exceed max_bytes; ambi_batch_evidence_profile: a depth bound of 2^31; ambi_batch_path_align: a run area above 1 GiB */
/* ambi_graph_read_fasta */
#define AMBI_ERR_FASTA_OPEN (-40)   /* cannot open the FASTA file */
#define AMBI_ERR_FASTA_CHROM (-41)  /* a segment's chromosome is not a record of the file */
#define AMBI_ERR_FASTA_RANGE (-42)  /* a segment ends beyond its record */
#define AMBI_ERR_FASTA_ORDER (-43)  /* a segment with end < start */

const char* ambi_error_string(int code);
int ambi_abi_version(void);
/* "hip" for libambigram_hip.so.  (The test-only host simulation built under tests/hostsim reports "hostsim".) */
const char* ambi_backend_name(void);
int ambi_device_count(int* count);
int ambi_set_device(int device);
/* Diagnostics: do two HIP streams dispatch side by side?  A kernel with ~100 us of workgroups waiting is put on stream_a and one tiny
 * workgroup on stream_b; *us = microseconds from the start of the former to the end of the latter -- a few microseconds when the
 * streams feed different dispatch pipes, ~the whole backlog when they share one (the engine asks the same question about the
 * caller's stream when it picks its side streams). */
int ambi_debug_stream_probe(void* stream_a, void* stream_b, float* us);

/* ------------------------------------------------------------------------------------------------
 * Graph: replaces `new Graph(lh)` + calculateHapDepth + calculateCopyNum + readBFBProps
 * (localhap.cpp:65-75; Graph.cpp:36-49,109-237,312-405; LocalGenomicMap.cpp:3941-3987).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ambi_graph ambi_graph_t;
int ambi_graph_read_lh(const char* lh_path, ambi_graph_t** out);
void ambi_graph_destroy(ambi_graph_t* g);
int ambi_graph_sizes(const ambi_graph_t* g, int32_t* n_seg, int32_t* n_junc, int32_t* n_chr);
/* any output pointer may be NULL */
int ambi_graph_segments(const ambi_graph_t* g, int32_t* id, int32_t* chr_id, int32_t* start, int32_t* end, double* cov, double* cn);
int ambi_graph_junctions(const ambi_graph_t* g, int32_t* src, int8_t* sdir, int32_t* tgt, int8_t* tdir, double* cov,
                         double* cn, uint8_t* inferred, uint8_t* bounded);
int ambi_graph_chromosome(const ambi_graph_t* g, int32_t chr, int32_t* source_id, int32_t* sink_id);
/* chromosome name of segment `seg_id` (the SEG line's H:id:<chrom>:start:end); returns the length needed */
int64_t ambi_graph_chrom_name(const ambi_graph_t* g, int32_t seg_id, char* buf, int64_t cap);
/* replaces LocalGenomicMap::readComponents (LocalGenomicMap.cpp:5096-5156, localhap.cpp:102); may add junctions */
int ambi_graph_read_juncs(ambi_graph_t* g, const char* juncs_path);
/* stdout lines the reference prints while loading (progress, SEG echoes, .juncs breakpoints), '\n' separated.
 * Returns the number of bytes needed (excluding the terminator); copies at most cap-1 bytes. */
int64_t ambi_graph_log(const ambi_graph_t* g, char* buf, int64_t cap);
/* PROP line: ins_mode / con_mode as in localhap.cpp:72-75, main chromosome name copied into main_chr[cap] */
int ambi_graph_props(const ambi_graph_t* g, int32_t* ins_mode, int32_t* con_mode, char* main_chr, int64_t cap);
/* Components collected by ambi_graph_read_juncs (the `res` of readComponents, LocalGenomicMap.cpp:5096-5156, after its
 * sort/unique): component c = ids[offsets[c] .. offsets[c+1]).  Returns the number of components; copies at most
 * ids_cap ids and off_cap offsets (offsets needs count+1 entries). */
/* calculateHapDepth + calculateCopyNum once more (`--op sc_bfb` does that to its first graph, localhap.cpp:438-439): entries
 * whose copy number is still <= 0 are recomputed and echoed again; new lines are appended to the graph's log. */
int ambi_graph_recalculate(ambi_graph_t* g);
/* TRX-BFB, `PROP I1:...` / `PROP C1:...` (a translocation BEFORE the BFB cycles; localhap.cpp:79-88 and :263).  ambi_graph_load does
 * what the reference does between the PROP line and the chromosome loop: insertBeforeBFB / concatBeforeBFB (LocalGenomicMap.cpp:
 * 4195-4295 / 4297-4395) rebuild the graph -- so every other entry point (chromosomes, batch units, ILP) sees the REBUILT graph, and
 * ambi_graph_log holds the lines the reference prints while rebuilding.  The reference's `new Graph(mSegs, mJuncs, mSources, mSinks)`
 * assigns through pointers it never initialises (Graph.cpp:25-34); its evident meaning -- a graph made of copies of the four
 * vectors -- is what is implemented.
 * ambi_graph_trx_before: 0 for an ordinary graph; else the number of entries of the map rebuilt segment id -> id in the file
 *   (entry 0 unused), copied to original_of.
 * ambi_graph_trx_restore = LocalGenomicMap::virusBFB (LocalGenomicMap.cpp:3839-3939), called on every reconstructed chromosome's
 *   path after indelBFB (localhap.cpp:263): path (signed rebuilt ids, `len` cells, room for `cap`) becomes the path over the
 *   segments of the file; text receives the lines the reference prints (caption + path of the first stage and, when an unused
 *   junction cuts the path, of the second stage), *text_len its full length.  Returns the new number of cells, or
 *   AMBI_ERR_UNSUPPORTED where the reference aborts or leaves a vertex of the rebuilt graph in the path.
 * ambi_graph_trx_original: a handle of its own (ambi_graph_destroy) on the graph of the FILE -- chromosome names and coordinates of
 *   the vertices of restored paths (the reference's simulation_sv.txt rows, localhap.cpp:326-337). */
int ambi_graph_trx_before(const ambi_graph_t* g, int32_t* original_of, int32_t cap);
int ambi_graph_trx_original(const ambi_graph_t* g, ambi_graph_t** out);
int ambi_graph_trx_restore(const ambi_graph_t* g, int32_t* path, int32_t len, int32_t cap, char* text, int64_t text_cap, int64_t* text_len);
/* replaces Graph::writeGraph (Graph.cpp:239-266): the graph as it stands -- after the copy-number maths and any junctions
 * ambi_graph_read_juncs added -- as .lh text, byte for byte what the reference writes (fixed SAMPLE_NAME TEST, its seven
 * header keys, numbers in %g form, a 'B' behind every segment); "write seg", which the reference prints to stdout, is
 * appended to the graph's log. */
int ambi_graph_write_lh(ambi_graph_t* g, const char* lh_path);

int ambi_graph_components(const ambi_graph_t* g, int32_t* ids, int32_t ids_cap, int32_t* offsets, int32_t off_cap);
/* Bases of the segments, for ambi_batch_sequence.  Replaces what the reference's scripts ask bedtools for (script/main.py:709-740
 * seg2fasta, script/bfb_scripts.py:31-49 getFasta).
 * ambi_graph_set_sequences: segment id i + 1 = bases[seg_off[i] .. seg_off[i + 1]), seg_off[0 .. n_seg] ascending; any byte values.
 * ambi_graph_read_fasta: segment i = chrom[start .. end) of the record whose name (the first word behind '>') is the segment's
 *   chromosome in the .lh: 0-BASED, HALF-OPEN, end - start bytes -- seg2fasta writes `chr start end` of the .lh unchanged into a BED
 *   line, and BED is half-open.  The reader is plain text and needs no index: any and irregular line widths, "\n" and "\r\n", a
 *   last line without a newline, several records; bytes are kept as they are (lower case included).  AMBI_ERR_FASTA_OPEN / _CHROM /
 *   _RANGE / _ORDER; after an error the graph keeps the sequences it had.
 * ambi_graph_sequences: the store back (seg_off: n_seg + 1 entries from 0; at most cap bytes to bases); returns its bytes,
 *   AMBI_ERR_STATE without sequences.
 * Attach them before the graph's chromosomes are added to a batch: ambi_batch_add_chromosome* copies a unit's bases. */
int ambi_graph_set_sequences(ambi_graph_t* g, const uint8_t* bases, const int64_t* seg_off);
int ambi_graph_read_fasta(ambi_graph_t* g, const char* fasta_path);
int64_t ambi_graph_sequences(const ambi_graph_t* g, uint8_t* bases, int64_t cap, int64_t* seg_off);
/* Fragments: every non-empty line of a .juncs file as ONE signed chain of segment ids, kept in the order of the line -- the
 * evidence a path is checked against (ambi_batch_frag_profile).  The reference's README calls these lines "possible fragments on
 * BFB paths"; readComponents (LocalGenomicMap.cpp:5096-5156) throws the order away before the ILP sees it.
 * ambi_graph_read_fragments: the token form and the return codes of ambi_graph_read_juncs (a file that cannot be read holds no line;
 *   an id outside the graph, which is also what a malformed token gives: AMBI_ERR_UNKNOWN_SEG).  It does NOT change the graph: no
 *   junction, no component, no line of the log.  A second call replaces the fragments of the first.
 * ambi_graph_set_fragments: the same from memory: fragment f = cells[frag_off[f] .. frag_off[f + 1]), frag_off[0 .. n] ascending from
 *   0, cells = signed segment ids of the file.  AMBI_ERR_MALFORMED for offsets that do not ascend from 0.
 * Both return AMBI_ERR_UNSUPPORTED on a graph rebuilt for PROP I1 / C1, as ambi_graph_read_juncs does.
 * ambi_graph_fragments: the fragments back (at most cap cells, off_cap offsets: n + 1 are needed) and, in unit_chr (n entries when
 *   off_cap > n), the chromosome every fragment belongs to: the one whose [source, sink] id range holds all of its segments, -1
 *   for a fragment of fewer than two cells or one that spans chromosomes (it keeps its index and belongs to no unit).  Returns n.
 * Attach them before the graph's chromosomes are added to a batch: ambi_batch_add_chromosome* copies a unit's fragments. */
int ambi_graph_read_fragments(ambi_graph_t* g, const char* juncs_path);
int ambi_graph_set_fragments(ambi_graph_t* g, const int32_t* cells, const int64_t* frag_off, int32_t n);
int32_t ambi_graph_fragments(const ambi_graph_t* g, int32_t* cells, int64_t cap, int64_t* frag_off, int32_t off_cap, int32_t* unit_chr);

/* ------------------------------------------------------------------------------------------------
 * Batch of units.  A unit = one chromosome of one sample = one iteration of the loop localhap.cpp:111-265:
 *   getJuncCN (:136-139), bias (:141-146), getIndelBias (:147), no-FBI shortcut (:164-170), [ILP + cbc on the host],
 *   targetCN (:222-232), constructDAG (:236), allTopologicalOrders (:254), getBFB (:261), indelBFB (:262)
 * plus the unit's share of the output-junction loop (:267-289).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ambi_batch ambi_batch_t;
int ambi_batch_create(ambi_batch_t** out);
void ambi_batch_destroy(ambi_batch_t* b);

/* Adds chromosome `chr` of `g` with the ILP solution of that chromosome: n_cols (column index, value) pairs as read
 * from `<prefix>.sol` (column numbering of localhap.cpp:122-133; epsilon/bias columns and non-positive values are
 * ignored), or infeasible != 0.  Returns the unit index (>= 0) or a negative code. */
int ambi_batch_add_chromosome(ambi_batch_t* b, const ambi_graph_t* g, int32_t chr, int32_t n_cols, const int32_t* col,
                              const int32_t* val, int32_t infeasible);
/* Same, reading the .sol text (localhap.cpp:184-212).  A missing file returns AMBI_ERR_SOL_OPEN. */
int ambi_batch_add_chromosome_sol(ambi_batch_t* b, const ambi_graph_t* g, int32_t chr, const char* sol_path);
/* `--op sc_bfb` (localhap.cpp:390-679): several graphs share ONE joint .sol per chromosome; graph `block` of `n_blocks`
 * owns the columns [block*numComp, (block+1)*numComp) (localhap.cpp:540-566).  The unit reconstructs with that block's
 * elements and never takes the no-fold-back shortcut by itself (the driver decides it from the first graph, :505-512). */
int ambi_batch_add_chromosome_sol_block(ambi_batch_t* b, const ambi_graph_t* g, int32_t chr, const char* sol_path, int32_t block,
                                        int32_t n_blocks);
/* Raw unit: LOCAL segment ids 1..n_seg (absolute id = local + seg_base), junctions with both ends inside the unit,
 * elements (is_loop, a, b, cn) of the decomposition. */
int ambi_batch_add_unit(ambi_batch_t* b, int32_t n_seg, int32_t seg_base, const double* seg_cn, int32_t n_junc,
                        const int32_t* j_src, const int32_t* j_tgt, const int8_t* j_sdir, const int8_t* j_tdir,
                        const double* j_cn, int32_t n_elem, const int32_t* e_is_loop, const int32_t* e_a,
                        const int32_t* e_b, const int32_t* e_cn, int32_t infeasible, int32_t has_components);
int ambi_batch_size(const ambi_batch_t* b, int32_t* n_units);

/* Tunables (before upload): order-table arena bytes (0 = size it from the first run), ideal-table slots per unit,
 * first-valid scan budget, number of lanes the enumerate kernel spreads the order-table rows over. */
int ambi_batch_configure(ambi_batch_t* b, int64_t order_arena_bytes, int32_t ideal_cap, int32_t first_budget, int32_t target_lanes);

/* Diagnostics hook, not part of the drop-in path (the reference has nothing like it).  Replaces, for one unit, the
 * OUTCOME of evaluating an order (getBFB's per-order body, LGM.cpp:3519-3658) by a given verdict, so that the control
 * flow around it -- scan budget, parallel search for the minimum index, orientation flip (LGM.cpp:3686-3695), --all --
 * can be exercised at places no known input reaches.  verdicts[0..R) = orders in the "forward seed"
 * orientation, verdicts[R..2R) = "reversed seed"; 1 valid, 0 invalid, a negative AMBI_ERR_* code, 127 = evaluate as
 * usual.  Call after the unit was added and before ambi_batch_upload; the breakpoints of a "valid" order are those the
 * real assembly leaves. */
int ambi_batch_debug_inject_validity(ambi_batch_t* b, int32_t unit, const int8_t* verdicts, int64_t count);
/* The other half of that hook: which ORDER the engine made the result of such a unit from.  After a run (waited for), the
 * node numbers of the order whose evaluation the unit's header reports (first_valid / first_forward), exactly as the stage that
 * published it decoded them from its source -- the first rows in group memory (scan inside the budget) or the unit's row of
 * the order table in device memory (parallel search) -- so that a test can tell row f from any other valid row.  A verdict
 * of 64 + {0, 1} means that verdict and, under AMBI_FLAG_ALL on a unit with more than 63 nodes (the only --all form that
 * reads the table), "leave the decoded row of THIS order here" (mark one order per run); ambi_batch_all_paths with count == 1
 * leaves the row it made that path from.  Returns the number of nodes
 * written to out[0..cap) (0: no stage stored a row in the last run), AMBI_ERR_ARG for a unit without injected verdicts. */
int ambi_batch_debug_unit_order(ambi_batch_t* b, int32_t unit, uint8_t* out, int32_t cap);

/* Packs the units and hands the inputs to the current device (they stay resident in HBM across runs).  Streams, events,
 * pinned words and device blocks come from a per-device pool with process lifetime (created on first use, reused by every
 * later batch, never destroyed per batch).  Small batches: the input image is written into pinned host memory here and its
 * ONE copy to HBM is queued by the first ambi_batch_run ahead of that run's kernels. */
int ambi_batch_upload(ambi_batch_t* b);
/* Enqueues one pass of the whole pipeline over the batch on `hip_stream` (a hipStream_t; NULL = default stream; it must
 * stay alive until the run has been waited for).  Asynchronous: the first run of a batch takes the order-table arena the
 * pool holds, and ambi_batch_wait grows it and repeats the run if the tables did not fit. */
int ambi_batch_run(ambi_batch_t* b, uint32_t flags, void* hip_stream);
int ambi_batch_wait(ambi_batch_t* b);
/* Returns as soon as the RECONSTRUCTION results of the enqueued run are complete in HBM (paths, breakpoints, output
 * junctions, headers): for small batches the engine reconstructs every unit whose first order assembles in one kernel and
 * builds the order tables (LocalGenomicMap::allTopologicalOrders' by-product) behind it, still in flight when this call
 * returns.  ambi_batch_wait / ambi_batch_download / the next ambi_batch_run wait for everything.  Same as ambi_batch_wait
 * whenever the fast path does not apply. */
int ambi_batch_wait_results(ambi_batch_t* b);
/* Copies the result blob to the host (implies wait).  After this the getters below are valid. */
int ambi_batch_download(ambi_batch_t* b);
/* What the caller of ONE sample needs -- localhap.cpp:261-289: the path of getBFB, the path after indelBFB, the output
 * junctions -- on the host with the least traffic (implies ambi_batch_wait_results).  A small batch on the fast path has
 * had them written into pinned host memory by the reconstruction kernel itself: no copy command at all.  Otherwise the same
 * as ambi_batch_download.  Afterwards ambi_batch_unit_result (num_orders = -1 when the order count is not part of what
 * was fetched), ambi_batch_unit_path and ambi_batch_unit_out_juncs are valid; the other getters need ambi_batch_download. */
int ambi_batch_fetch_paths(ambi_batch_t* b);

/* Several GPUs from C (`ambi_bfb_reconstruct_batch(..., device_or_minus1_for_all)`; north star: "independent .lh
 * samples shard embarrassingly across the 8 GPUs of one node").  The units of a batch are the iterations of the loop
 * localhap.cpp:111-265 and do not depend on each other: this call deals them round-robin over the devices, runs every share
 * on its device from a host thread of its own (upload -> run(flags) -> download) and merges the results on the host.  Takes
 * the place of ambi_batch_upload + _run + _download: all getters are valid afterwards (the per-unit device-side ones -- DAG,
 * order rows, --all lists -- are answered by the device that holds the unit).  devices: n_devices device ordinals (an ordinal
 * may repeat: several shares on one device), or NULL for the first n_devices visible devices (all of them if n_devices <= 0).
 * May be called again (the shares stay resident).  A batch is either uploaded to one device or sharded, not both. */
int ambi_batch_run_sharded(ambi_batch_t* b, uint32_t flags, const int32_t* devices, int32_t n_devices);

/* Device-side view for collectives: the result blob (header [n_units] + per-unit arrays) lives in device memory.  Its
 * layout is the engine's own (csrc/ambi_batch.hpp: UnitOut, unit_layout; path cells are 2-byte LOCAL signed segment ids --
 * absolute id = id +- the chromosome's first segment id - 1); portable consumers use ambi_batch_pack_paths / _pack_runs, which
 * deliver absolute ids, or the getters after ambi_batch_download. */
int ambi_batch_device_results(ambi_batch_t* b, void** dev_ptr, int64_t* bytes);
/* Packs the final paths of all units into caller-provided DEVICE buffers: lengths[n_units] (int32) and the
 * concatenation of the paths (int32, absolute signed ids) -- the payload of the end-of-batch RCCL gather.
 * which: 0 = getBFB path, 1 = path after indelBFB.  dev_total_cells receives the number of cells the paths have (device
 * int64), whatever cell_cap is; dev_lengths is always complete.  Capacity rule: the cells are clamped one by one -- of the
 * concatenation exactly the first min(cell_cap, total) cells are written, and no word of dev_cells at or past cell_cap. */
int ambi_batch_pack_paths(ambi_batch_t* b, int32_t which, int32_t* dev_lengths, int32_t* dev_cells, int64_t cell_cap,
                          int64_t* dev_total_cells, void* hip_stream);

/* The same payload in run-length form: a path is a sequence of runs whose cells count up by one (a stretch of
 * consecutive segments on one strand: `3+4+5+` = start 3, length 3; `5-4-3-` = start -5, length 3), a few dozen runs for
 * thousands of cells, so the exchange moves kilobytes instead of megabytes per sample and the receiving rank expands
 * the runs in its own memory (ambi_expand_runs).  Per unit: dev_lengths[u] = cells, dev_run_counts[u] = runs; the runs
 * of all units follow each other in dev_run_start / dev_run_len (int32 each, at most run_cap).  dev_totals (device,
 * int64[2]) receives {runs, cells} the paths have, whatever run_cap is; dev_lengths and dev_run_counts are always complete.
 * Capacity rule: a unit is written whole or not at all -- unit u, whose runs start at off = the sum of the run counts before
 * it, is written when off + dev_run_counts[u] <= run_cap; of any other unit not one word is written, nor any word at or past
 * run_cap (so run_cap = 0 only counts, and a caller that finds totals[0] > run_cap packs again with room for all). */
int ambi_batch_pack_runs(ambi_batch_t* b, int32_t which, int32_t* dev_lengths, int32_t* dev_run_counts, int32_t* dev_run_start,
                         int32_t* dev_run_len, int64_t run_cap, int64_t* dev_totals, void* hip_stream);
/* The final paths of every unit ON THE HOST, in that run-length form, without stopping the stream (the reference
 * ends with its paths in host memory and prints every one, LocalGenomicMap.cpp:3684-3689, localhap.cpp:262).
 * ambi_batch_runs_to_host queues, behind the work already on hip_stream, ONE device-to-host copy of {lengths, run counts, runs} into
 * pinned memory on a copy stream of the engine's own -- the caller's stream is free for the next ambi_batch_run at once.  For the
 * final path (which = 1) nothing is computed for it: the finish kernels write every unit's runs beside its cells, into one of two
 * blocks that alternate from run to run; which = 0 (the path before indelBFB) goes through the packing kernels first.  slot 0 / 1: two blocks, so that the copy of step i travels while
 * step i+1 computes.  ambi_batch_runs_wait blocks until that copy has arrived and describes it (pointers into the engine's pinned
 * block, valid until the slot is queued again or the batch is destroyed); bytes = what the payload needs, copied_bytes = what
 * the copy moved (the slot's capacity).  ambi_batch_runs_unit_path expands one unit's runs into cells (absolute signed ids):
 * exactly what ambi_batch_unit_path returns after a download. */
typedef struct {
    int64_t n_runs, n_cells, bytes, copied_bytes;
    const int32_t* lengths;      /* [n_units] cells of the path */
    const int32_t* run_counts;   /* [n_units] runs of the path */
    const int32_t* run_start;    /* first cell of a run (absolute signed segment id) */
    const int32_t* run_len;      /* cells of the run, counting up by one */
    const int64_t* run_off;      /* [n_units + 1] unit u's runs are entries run_off[u] .. run_off[u] + run_counts[u] - 1 of run_start / run_len
                                  * (the finish kernels leave every unit's runs in slots of its own: the entries are not packed) */
} ambi_runs_view_t;
int ambi_batch_runs_to_host(ambi_batch_t* b, int32_t which, int32_t slot, void* hip_stream);
int ambi_batch_runs_wait(ambi_batch_t* b, int32_t slot, ambi_runs_view_t* out);
int ambi_batch_runs_unit_path(ambi_batch_t* b, int32_t slot, int32_t unit, int32_t* out, int32_t cap);

/* The copy-number profile of every unit's path, computed ON THE DEVICE: how often the path crosses each segment on either strand,
 * and how that compares with the decomposition's target copy numbers and the input copy numbers.  Replaces what the reference
 * meant to report and left unfinished: localhap.cpp:318-324 computes an `isResolved` verdict from the sum of |CN - targetCN|,
 * localhap.cpp:340-351 is a commented-out CN.txt writer whose fallback for a segment counts the segment's occurrences in the path.
 * (The reference's own sum truncates a running int after every add and feeds commented-out code only: it is not reproduced; all
 * fields here are exact integers.)  Per unit 2 (n + 1) int32 travel to the host instead of the path's cells.
 * l1_target / n_off_target: what imperfectFBI and indelBFB did to the path after the decomposition fixed target_cn; n_off_input:
 * the fit to the data (seg_cn after getIndelBias, as ambi_batch_unit_prepare returns it). */
typedef struct {
    int32_t status;        /* the unit's status (ambi_unit_result_t::status) */
    int32_t cells;         /* cells of the profiled path; 0 for a unit with a negative status or without a path (all counts zero) */
    int32_t runs;          /* stretches of cells counting up by one */
    int32_t turns;         /* steps with path[i+1] == -path[i]: fold-back turns actually taken */
    int32_t max_cn;        /* max over the segments of fwd + rev */
    int32_t n_uncovered;   /* segments with fwd + rev == 0 */
    int32_t n_off_target;  /* segments with fwd + rev != target_cn */
    int32_t n_off_input;   /* segments with |fwd + rev - seg_cn| >= 0.5 */
    int64_t l1_target;     /* sum over the segments of |fwd + rev - target_cn| (localhap.cpp:318-324, without its truncation) */
} ambi_unit_profile_t;
/* Queues the profile of the LAST run's results behind that run on hip_stream (which: 0 = the getBFB path, 1 = the path after indelBFB:
 * exactly the cells ambi_batch_unit_path(unit, which) returns; localhap.cpp:340-351 counts the printed path), then one device-to-host
 * copy of the profile block on the engine's copy stream: hip_stream is not blocked.  AMBI_ERR_STATE before any run, AMBI_ERR_ARG
 * for another `which`.  After ambi_batch_run_sharded the call goes to every share, on the share's own stream. */
int ambi_batch_profile(ambi_batch_t* b, int32_t which, void* hip_stream);
/* Blocks until the profile is in host memory.  Makes the run's results final first (ambi_batch_wait: a first run repeated with a
 * larger arena, units finished by the parallel search) and profiles once more if that changed them after the profile was queued. */
int ambi_batch_profile_wait(ambi_batch_t* b);
/* A unit's summary (localhap.cpp:318-324: the reference's per-chromosome verdict); AMBI_ERR_STATE without a waited-for profile of
 * the last run. */
int ambi_batch_unit_profile(const ambi_batch_t* b, int32_t unit, ambi_unit_profile_t* out);
/* A unit's traversal counts per LOCAL segment id (localhap.cpp:340-351: the CN.txt column): fwd[i] / rev[i] = crossings of segment
 * i on the '+' / '-' strand, i = 1..n, slot 0 zero.  Returns n + 1; AMBI_ERR_ARG when cap < n + 1. */
int ambi_batch_unit_path_cn(const ambi_batch_t* b, int32_t unit, int32_t* fwd, int32_t* rev, int32_t cap);
/* The profile block in DEVICE memory, for collectives (localhap.cpp:318-351 for a whole cohort without a host round trip):
 * [ambi_unit_profile_t[n_units]] padded to 16 bytes, then per unit fwd int32[n + 1] and rev int32[n + 1], each array padded to 16
 * bytes.  Valid after ambi_batch_profile_wait until the next ambi_batch_profile; not available for a sharded batch. */
int ambi_batch_profile_device(ambi_batch_t* b, void** dev_ptr, int64_t* bytes);

/* The junction usage profile of every unit's path, computed ON THE DEVICE (ambi_junc_profile_kernel): which of the unit's input
 * junctions (SVs, fold-backs, adjacencies) the path takes, how often, and how that compares with their input copy numbers.  The
 * reference leaves the raw material in simulation_sv.txt (localhap.cpp:326-337: every input junction with its copy number as an
 * `input` row, every non-adjacent step of the paths with its count as an `output` row) and the join to the user; the join test is
 * its own (localhap.cpp:277-278): a step u -> v belongs to a junction when it equals the junction's edge A or its complement edge
 * B (Junction.cpp:27-39).  With the path cells c[0..P) that ambi_batch_unit_path(unit, which) returns (as local ids) and the
 * unit's junctions j = 0..m-1 in the unit's order (the graph's order restricted to junctions with both ends inside the unit):
 *   step i = (c[i], c[i+1]), i = 0..P-2; junction j with strand-signed ends (s, t) matches a step (x, y) when (x, y) == (s, t) or
 *   (x, y) == (-t, -s); a fold-back (s, -s) has equal edges and is credited once per step; when several junctions match (raw units
 *   only: lh_graph.cpp:81 drops a second copy) the LOWEST index is credited and the others get nothing.
 * All fields are exact integers.  Per unit m int32 travel to the host instead of the path's cells. */
typedef struct {
    int32_t status;           /* the unit's status (ambi_unit_result_t::status) */
    int32_t steps;            /* P - 1; a unit with a negative status or without a path has every field but status zero */
    int32_t steps_matched;    /* steps credited to a junction = sum of the counts */
    int32_t steps_unmatched;  /* steps that match no junction of the unit (localhap.cpp:277-289 finds no input row for them) */
    int32_t first_unmatched;  /* smallest i whose step matches nothing, -1 if none */
    int32_t juncs;            /* m */
    int32_t juncs_used;       /* junctions with count > 0 */
    int32_t max_count;        /* max over the junctions of count */
    int32_t n_over;           /* junctions with count - cn >= 0.5 (cn: the junction's input copy number as uploaded) */
    int32_t n_under;          /* junctions with cn - count >= 0.5 */
} ambi_unit_junc_profile_t;
/* Queues the junction profile of the LAST run's results behind that run on hip_stream (which as for ambi_batch_profile;
 * localhap.cpp:267-289 walks the printed paths), then one device-to-host copy of the block on the engine's copy stream: hip_stream
 * is not blocked.  AMBI_ERR_STATE before any run, AMBI_ERR_ARG for another `which`.  After ambi_batch_run_sharded the call goes to
 * every share, on the share's own stream. */
int ambi_batch_junc_profile(ambi_batch_t* b, int32_t which, void* hip_stream);
/* Blocks until the junction profile is in host memory.  Makes the run's results final first (ambi_batch_wait) and profiles once
 * more if that changed them after the request was queued (localhap.cpp:267-289 runs after the last path is final). */
int ambi_batch_junc_profile_wait(ambi_batch_t* b);
/* A unit's summary (localhap.cpp:326-337: input rows against output rows); AMBI_ERR_STATE without a waited-for junction profile
 * of the last run. */
int ambi_batch_unit_junc_profile(const ambi_batch_t* b, int32_t unit, ambi_unit_junc_profile_t* out);
/* A unit's counts per junction (localhap.cpp:277-278 joined with :326-337): count[j] = steps credited to the unit's junction j,
 * graph_index[j] = its index into the arrays of ambi_graph_junctions (j itself for a raw unit).  Either pointer may be NULL.
 * Returns m; AMBI_ERR_ARG when cap < m. */
int ambi_batch_unit_junc_usage(const ambi_batch_t* b, int32_t unit, int32_t* count, int32_t* graph_index, int32_t cap);
/* The junction profile block in DEVICE memory, for collectives (localhap.cpp:326-337 for a whole cohort without a host round
 * trip): [ambi_unit_junc_profile_t[n_units]] padded to 16 bytes, then per unit count int32[m] padded to 16 bytes.  Valid after
 * ambi_batch_junc_profile_wait until the next ambi_batch_junc_profile; not available for a sharded batch. */
int ambi_batch_junc_profile_device(ambi_batch_t* b, void** dev_ptr, int64_t* bytes);

/* The fragment support profile of every unit's path, computed ON THE DEVICE (ambi_frag_profile_kernel): how often the path contains
 * every fragment of the unit's .juncs evidence (ambi_graph_read_fragments; README of the reference: "possible fragments on BFB
 * paths"), in either direction, and where first.  With the path cells c[0..P) that ambi_batch_unit_path(unit, which) returns (as
 * local ids) and the unit's fragments f = 0..F-1 in the graph's order:
 *   a fragment (f_0 .. f_{L-1}), L >= 2, occurs at i when c[i + k] == f_k for all k, 0 <= i <= P - L; occurrences may overlap;
 *   fwd[f] = occurrences of f, rev[f] = occurrences of its reverse complement (-f_{L-1} .. -f_0), 0 when that equals f (a
 *   palindrome such as 3+ 3- is counted once), first[f] = the smallest i over both directions, -1 when there is none.
 * All fields are exact integers.  Per unit 3 F int32 travel to the host instead of the path's cells.  The fragments go to the
 * device with the first request (and again after they changed), never with ambi_batch_upload. */
typedef struct {
    int32_t status;             /* the unit's status (ambi_unit_result_t::status) */
    int32_t cells;              /* P; a unit with a negative status or without a path has every field but status and frags zero */
    int32_t frags;              /* F */
    int32_t frags_supported;    /* fragments with fwd + rev > 0 */
    int32_t first_unsupported;  /* lowest fragment index without an occurrence, -1 if none */
    int32_t max_count;          /* max over the fragments of fwd + rev */
    int32_t longest_supported;  /* cells of the longest supported fragment, 0 if none */
    int32_t reserved;
    int64_t occurrences;        /* sum over the fragments of fwd + rev */
} ambi_unit_frag_profile_t;
/* The fragments of a raw unit (ambi_batch_add_unit): fragment f = cells[frag_off[f] .. frag_off[f + 1]), LOCAL signed ids, frag_off
 * ascending from 0; a second call replaces the first.  AMBI_ERR_ARG for a fragment of fewer than two cells, an id outside
 * 1..n_seg, more than 65535 fragments or 2^31 cells and more; AMBI_ERR_STATE after ambi_batch_run_sharded (the shares hold copies). */
int ambi_batch_set_unit_fragments(ambi_batch_t* b, int32_t unit, const int32_t* cells, const int64_t* frag_off, int32_t n);
/* Queues the fragment profile of the LAST run's results behind that run on hip_stream (which as for ambi_batch_profile), then one
 * device-to-host copy of the block on the engine's copy stream: hip_stream is not blocked.  A batch without any fragment is
 * served: every unit gets frags = 0.  AMBI_ERR_STATE before any run, AMBI_ERR_ARG for another `which`.  After
 * ambi_batch_run_sharded the call goes to every share, on the share's own stream. */
int ambi_batch_frag_profile(ambi_batch_t* b, int32_t which, void* hip_stream);
/* Blocks until the fragment profile is in host memory.  Makes the run's results final first (ambi_batch_wait) and profiles once
 * more if that changed them after the request was queued. */
int ambi_batch_frag_profile_wait(ambi_batch_t* b);
/* A unit's summary; AMBI_ERR_STATE without a waited-for fragment profile of the last run. */
int ambi_batch_unit_frag_profile(const ambi_batch_t* b, int32_t unit, ambi_unit_frag_profile_t* out);
/* A unit's values per fragment: fwd, rev and first as above, graph_index[f] = the fragment's index in the graph's list
 * (ambi_graph_fragments; f itself for a raw unit).  Any pointer may be NULL.  Returns F; AMBI_ERR_ARG when cap < F. */
int ambi_batch_unit_frag_support(const ambi_batch_t* b, int32_t unit, int32_t* fwd, int32_t* rev, int32_t* first, int32_t* graph_index, int32_t cap);
/* The fragment profile block in DEVICE memory, for collectives: [ambi_unit_frag_profile_t[n_units]] padded to 16 bytes, then per
 * unit fwd int32[F], rev int32[F] and first int32[F], each array padded to 16 bytes.  Valid after ambi_batch_frag_profile_wait until
 * the next ambi_batch_frag_profile; not available for a sharded batch. */
int ambi_batch_frag_profile_device(ambi_batch_t* b, void** dev_ptr, int64_t* bytes);

/* The evidence depth profile of every unit's path, computed ON THE DEVICE (ambi_evidence_mark_kernel, ambi_evidence_scan_kernel):
 * how many occurrences of the unit's fragments lie over every step of the path, and which junction traversals none spans.  With
 * the path cells c[0..P) that ambi_batch_unit_path(unit, which) returns (as local ids), the fragments and their occurrences as for
 * ambi_batch_frag_profile and the junctions j = 0..m-1 with the crediting rule of ambi_batch_junc_profile:
 *   step k = (c[k], c[k+1]), k = 0 .. P-2; an occurrence at i of a pattern of L cells covers the steps i .. i+L-2;
 *   depth[k] = occurrences, over all fragments and both directions, that cover step k;
 *   count[j] = steps credited to junction j (the junction profile's count), covered[j] = those of them with depth > 0,
 *   min_depth[j] = the minimum of depth over them, -1 when count[j] == 0.
 * All fields are exact integers.  depth is int32 and at most 2 * (fragment cells - F) of the unit; a request is refused with
 * AMBI_ERR_TOO_LARGE when that bound reaches 2^31 for some unit.  The depths stay on the device (4 bytes per cell of every unit's
 * path capacity); per unit 3 m int32 travel to the host. */
typedef struct {
    int32_t status;                /* the unit's status (ambi_unit_result_t::status) */
    int32_t steps;                 /* P - 1; a unit with a negative status or without a path has every field but status and juncs zero
                                      and first_uncovered = longest_uncovered_at = -1 */
    int32_t steps_covered;         /* steps with depth > 0 */
    int32_t max_depth;             /* max over the steps of depth */
    int32_t first_uncovered;       /* smallest k with depth[k] == 0, -1 if none */
    int32_t longest_uncovered;     /* steps of the longest stretch of consecutive steps with depth 0 */
    int32_t longest_uncovered_at;  /* the smallest start of such a stretch, -1 if none */
    int32_t juncs;                 /* m */
    int32_t juncs_used;            /* junctions with count > 0 */
    int32_t juncs_covered;         /* junctions with count > 0 and covered == count */
    int32_t juncs_uncovered;       /* junctions with count > 0 and covered == 0 */
    int32_t unmatched_covered;     /* steps credited to no junction that have depth > 0 */
    int64_t depth_sum;             /* sum over the steps of depth */
} ambi_unit_evidence_profile_t;
/* Queues the evidence profile of the LAST run's results behind that run on hip_stream (which as for ambi_batch_profile): the
 * fragments go up first when the device does not hold this version of them, then the two kernels, then one device-to-host copy
 * of the block on the engine's copy stream: hip_stream is not blocked.  A batch without any fragment is served: every depth is 0.
 * AMBI_ERR_STATE before any run, AMBI_ERR_ARG for another `which`, AMBI_ERR_TOO_LARGE as above (nothing is queued then, and an
 * earlier evidence profile of this run is no longer readable: the call clears it first).  After ambi_batch_run_sharded the
 * call goes to every share, on the share's own stream. */
int ambi_batch_evidence_profile(ambi_batch_t* b, int32_t which, void* hip_stream);
/* Blocks until the evidence profile is in host memory.  Makes the run's results final first (ambi_batch_wait) and profiles once
 * more if that changed them after the request was queued. */
int ambi_batch_evidence_profile_wait(ambi_batch_t* b);
/* A unit's summary; AMBI_ERR_STATE without a waited-for evidence profile of the last run. */
int ambi_batch_unit_evidence_profile(const ambi_batch_t* b, int32_t unit, ambi_unit_evidence_profile_t* out);
/* A unit's values per junction: count, covered and min_depth as above, graph_index[j] = the junction's index in the graph's list
 * (j itself for a raw unit).  Any pointer may be NULL.  Returns m; AMBI_ERR_ARG when cap < m. */
int ambi_batch_unit_evidence_juncs(const ambi_batch_t* b, int32_t unit, int32_t* count, int32_t* covered, int32_t* min_depth, int32_t* graph_index, int32_t cap);
/* The depths of the steps [first, first + n) of a unit to host memory; nothing else is downloaded.  AMBI_ERR_ARG for a range
 * outside [0, P-1] (a unit without a step takes n = 0 only). */
int ambi_batch_unit_evidence_depth(ambi_batch_t* b, int32_t unit, int64_t first, int64_t n, int32_t* out);
/* The evidence profile block in DEVICE memory, for collectives: [ambi_unit_evidence_profile_t[n_units]] padded to 16 bytes, then
 * per unit count int32[m], covered int32[m] and min_depth int32[m], each array padded to 16 bytes.  Valid after
 * ambi_batch_evidence_profile_wait until the next ambi_batch_evidence_profile; not available for a sharded batch. */
int ambi_batch_evidence_profile_device(ambi_batch_t* b, void** dev_ptr, int64_t* bytes);
/* The depth area in DEVICE memory: unit u's depths are int32[steps] at byte unit_off[u] (a multiple of 16; cap >= n_units entries,
 * or NULL), the slice of a unit without a path holds nothing of meaning.  Valid as the block above; not available for a sharded
 * batch. */
int ambi_batch_evidence_depth_device(ambi_batch_t* b, void** dev_ptr, int64_t* bytes, int64_t* unit_off, int32_t cap);

/* The fold-back arm profile of every unit's path, computed ON THE DEVICE (ambi_fold_arm_kernel, ambi_fold_scan_kernel): where the
 * path folds back, how long the reverse-complement palindrome around every fold is, and how deeply the palindromes nest -- the
 * structure that makes a path a breakage-fusion-bridge path.  With the path cells c[0..P) that ambi_batch_unit_path(unit, which)
 * returns (as local ids), the steps k = 0 .. P-2 and the junctions j = 0..m-1 with the crediting rule of ambi_batch_junc_profile:
 *   fold: a step whose two cells have opposite sign (where printBFB prints `|`);
 *   alignments a = 0..4 with (dl, dr) = (0,1) (-1,1) (0,2) (-2,1) (0,3): the perfect fold-back, then one or two unpaired cells on the
 *   left or on the right.  With i = k + dl and j = k + dr, arm_a is the largest r >= 0 with i-t >= 0, j+t < P and c[i-t] == -c[j+t]
 *   for all t < r; 0 when i < 0 or j >= P;
 *   a fold's alignment and arm: the smallest a with arm_a > 0 and that arm; alignment -1 and arm 0 when there is none;
 *   span: a fold with arm r > 0 covers the steps i-r+1 .. j+r-2, k among them;
 *   cover[s] = folds whose span covers step s; the nesting of a fold at k is cover[k] - 1;
 *   folds[j] = folds credited to junction j, max_arm[j] = the longest arm among them (0 when there are none).
 * All fields are exact integers.  Two int32 planes stay on the device (4 bytes each per cell of every unit's path capacity):
 *   plane 0, fold[k]: 0 for a step that is no fold, else (alignment + 2) << 24 | arm (arms stay below 2^22);
 *   plane 1, cover[k].
 * Per unit 2 m int32 travel to the host. */
#define AMBI_FOLD_ARM(v) ((int32_t)((v) & 0xffffff))
#define AMBI_FOLD_ALIGN(v) ((int32_t)(((v) >> 24) - 2))
typedef struct {
    int32_t status;           /* the unit's status (ambi_unit_result_t::status) */
    int32_t steps;            /* P - 1; a unit with a negative status or without a path has every field but status zero and
                                 max_arm_at = max_cover_at = -1 */
    int32_t folds;            /* steps whose two cells have opposite sign */
    int32_t folds_perfect;    /* folds with alignment 0 */
    int32_t folds_gapped;     /* folds with alignment 1..4 */
    int32_t folds_open;       /* folds with alignment -1: no arm */
    int32_t folds_unmatched;  /* folds credited to no junction */
    int32_t max_arm;          /* the longest arm */
    int32_t max_arm_at;       /* the smallest k of a fold with that arm, -1 if max_arm == 0 */
    int32_t max_cover;        /* max over the steps of cover */
    int32_t max_cover_at;     /* the smallest step with that cover, -1 if max_cover == 0 */
    int32_t steps_covered;    /* steps with cover > 0 */
    int64_t arm_sum;          /* sum of the arms of all folds */
} ambi_unit_fold_profile_t;
/* Queues the fold profile of the LAST run's results behind that run on hip_stream (which as for ambi_batch_profile): the two
 * kernels, then one device-to-host copy of the block on the engine's copy stream: hip_stream is not blocked.  The planes are
 * allocated at the first request; a failure to allocate them is this call's error.  AMBI_ERR_STATE before any run, AMBI_ERR_ARG for
 * another `which`.  After ambi_batch_run_sharded the call goes to every share, on the share's own stream. */
int ambi_batch_fold_profile(ambi_batch_t* b, int32_t which, void* hip_stream);
/* Blocks until the fold profile is in host memory.  Makes the run's results final first (ambi_batch_wait) and profiles once more
 * if that changed them after the request was queued. */
int ambi_batch_fold_profile_wait(ambi_batch_t* b);
/* A unit's summary; AMBI_ERR_STATE without a waited-for fold profile of the last run. */
int ambi_batch_unit_fold_profile(const ambi_batch_t* b, int32_t unit, ambi_unit_fold_profile_t* out);
/* A unit's values per junction: folds and max_arm as above, graph_index[j] = the junction's index in the graph's list (j itself
 * for a raw unit).  Any pointer may be NULL.  Returns m; AMBI_ERR_ARG when cap < m. */
int ambi_batch_unit_fold_juncs(const ambi_batch_t* b, int32_t unit, int32_t* folds, int32_t* max_arm, int32_t* graph_index, int32_t cap);
/* The entries [first, first + n) of a unit's plane (0: fold, 1: cover) to host memory; nothing else is downloaded.  AMBI_ERR_ARG
 * for another plane or a range outside [0, P-1] (a unit without a step takes n = 0 only). */
int ambi_batch_unit_fold_plane(ambi_batch_t* b, int32_t unit, int32_t plane, int64_t first, int64_t n, int32_t* out);
/* The fold profile block in DEVICE memory, for collectives: [ambi_unit_fold_profile_t[n_units]] padded to 16 bytes, then per unit
 * folds int32[m] and max_arm int32[m], each array padded to 16 bytes.  Valid after ambi_batch_fold_profile_wait until the next
 * ambi_batch_fold_profile; not available for a sharded batch. */
int ambi_batch_fold_profile_device(ambi_batch_t* b, void** dev_ptr, int64_t* bytes);
/* Both planes in DEVICE memory, `bytes` in all: the fold planes of all units in the first half, the cover planes in the second;
 * plane p of unit u is int32[steps] at byte p * (bytes / 2) + unit_off[u] (a multiple of 16; cap >= n_units entries, or NULL), the
 * slices of a unit without a path hold nothing of meaning.  Valid as the block above; not available for a sharded batch. */
int ambi_batch_fold_planes_device(ambi_batch_t* b, void** dev_ptr, int64_t* bytes, int64_t* unit_off, int32_t cap);

/* Path comparison ON THE DEVICE (ambi_path_compare_kernel): how close are two paths -- a reconstructed path against the simulated
 * truth, a unit's path before indelBFB against the path after it, one cell's path against another cell's under --op sc_bfb.  A
 * pair is two sides (A, B); a side is a unit's path ambi_batch_unit_path(unit, which), AMBI_COMPARE_UNIT(unit, which), or a path
 * GIVEN by the caller in the local signed ids of whatever it is compared with, AMBI_COMPARE_GIVEN(t).  With the cells a[0..la) and
 * b[0..lb) and the two orientations o = 0: B0 = b and o = 1: the reverse complement B1[i] = -b[lb-1-i]:
 *   prefix[o]: the largest p with a[t] == Bo[t] for all t < p;
 *   suffix[o]: the largest s <= min(la, lb) - prefix[o] with a[la-1-t] == Bo[lb-1-t] for all t < s;
 *   dist[o]:   the fewest single-cell insertions plus deletions that turn a into Bo if that is <= dmax, otherwise -1;
 *   lcs[o]:    (la + lb - dist[o]) / 2, the longest common subsequence, or -1 when dist[o] is -1.
 * All fields are exact integers.  The common ends are trimmed and the rest goes through Myers' greedy diff, at most dmax rounds:
 * the cost of a pair grows with its distance, not with the product of the lengths. */
#define AMBI_COMPARE_UNIT(u, which) ((int32_t)(2 * (u) + (which)))
#define AMBI_COMPARE_GIVEN(t) ((int32_t)~(t))
#define AMBI_COMPARE_DMAX_CAP 1024
#define AMBI_COMPARE_DMAX_DEFAULT 64
typedef struct {
    int32_t status;      /* 0; or the status of the first side that is a unit with a negative status or without a path
                            (AMBI_ERR_BAD_INPUT for a unit without a path whose own status is not negative: a failure is never
                            0): every field below but the lengths is then 0, dist and lcs are -1 */
    int32_t len_a;       /* la (0 for a side that failed) */
    int32_t len_b;       /* lb */
    int32_t dmax;        /* the request's cap */
    int32_t prefix[2];   /* [orientation] */
    int32_t suffix[2];
    int32_t dist[2];
    int32_t lcs[2];
} ambi_path_compare_t;
/* The given paths of the batch: n paths, path t = cells[off[t] .. off[t+1]) in local signed ids (off has n + 1 entries, off[0] = 0).
 * Replaces the earlier set; n = 0 drops it.  They are kept on the host and travel to a device buffer of their own with the next
 * request; the batch image is not touched.  A request keeps the set it was made with: replacing the set between
 * ambi_batch_path_compare and its wait does not change what that request compares.  AMBI_ERR_ARG for a cell that is 0 or beyond +-32767, or a path without a cell or with
 * more than 4 194 304. */
int ambi_batch_set_compare_paths(ambi_batch_t* b, const int32_t* cells, const int64_t* off, int32_t n);
/* Queues the comparison of n_pairs pairs (pairs[2 i], pairs[2 i + 1]: the sides of pair i) over the LAST run's results behind
 * that run on hip_stream: the given paths if the device does not hold them, the pairs, one kernel (a workgroup per pair), then one
 * device-to-host copy of the block on the engine's copy stream: hip_stream is not blocked.  dmax: 0 .. AMBI_COMPARE_DMAX_CAP.
 * AMBI_ERR_STATE before any run; AMBI_ERR_ARG for a side that names no unit, no `which` or no given path, or another dmax;
 * AMBI_ERR_UNSUPPORTED after ambi_batch_run_sharded (a pair may span shares). */
int ambi_batch_path_compare(ambi_batch_t* b, const int32_t* pairs, int32_t n_pairs, int32_t dmax, void* hip_stream);
/* Blocks until the results are in host memory.  Makes the run's results final first (ambi_batch_wait) and compares once more if
 * that changed them after the request was queued. */
int ambi_batch_path_compare_wait(ambi_batch_t* b);
/* The result of pair `pair` of the last request; AMBI_ERR_STATE without a waited-for comparison of the last run. */
int ambi_batch_path_compare_result(const ambi_batch_t* b, int32_t pair, ambi_path_compare_t* out);
/* The results in DEVICE memory, for collectives: ambi_path_compare_t[n_pairs], padded to 16 bytes.  Valid after
 * ambi_batch_path_compare_wait until the next ambi_batch_path_compare. */
int ambi_batch_path_compare_device(ambi_batch_t* b, void** dev_ptr, int64_t* bytes);

/* Path alignment ON THE DEVICE (ambi_path_align_kernel): WHERE do two paths differ, and by which cells -- a canonical shortest
 * insert / delete script of every pair, in ONE orientation per pair, as maximal runs.  An entry is a triple (A, B, orient): A and B
 * are sides as in the path comparison (AMBI_COMPARE_UNIT / AMBI_COMPARE_GIVEN over the set of ambi_batch_set_compare_paths), orient
 * is 0 (as is) or 1 (against the reverse complement Bo[i] = -b[lb-1-i]).  A caller who does not know the orientation asks the
 * comparison first and takes the smaller dist.  prefix, suffix and dist are the comparison's for that orientation.  The script is
 * the traceback of Myers' greedy rounds over the windows between the common ends, ties to the insertion; a unit edit either deletes
 * a[a_pos] (kind 0; b_pos: the cell of Bo in front of which it would stand) or inserts Bo[b_pos] in front of a[a_pos] (kind 1), in
 * the coordinates of the whole a and the whole Bo.  Consecutive unit edits of one kind with no matched cell between them form one
 * maximal run: a_pos advances through a deletion run and b_pos stays; the other way round for insertions.  A deletion directly
 * followed by an insertion stays two runs.  Applying the runs to a in order gives Bo; the lengths sum to dist; a pair has at most
 * dist runs. */
#define AMBI_ALIGN_DMAX_CAP 1024
typedef struct {
    int32_t status;      /* as ambi_path_compare_t: 0, or the first failing side's status (never 0 for a failure); prefix and suffix
                            are then 0, dist is -1 and n_runs 0 */
    int32_t len_a;       /* la (0 for a side that failed) */
    int32_t len_b;       /* lb */
    int32_t orient;      /* the entry's orientation */
    int32_t prefix;
    int32_t suffix;
    int32_t dist;        /* insertions plus deletions if that is <= dmax, otherwise -1 */
    int32_t n_runs;      /* 0 when dist is -1 */
} ambi_path_align_t;
typedef struct {
    int32_t a_pos;       /* the first cell of a the run deletes / the cell of a in front of which it inserts */
    int32_t b_pos;       /* the cell of Bo in front of which the deleted cells would stand / the first cell of Bo it inserts */
    int32_t len;
    int32_t kind;        /* 0: deletion, 1: insertion */
} ambi_align_run_t;
/* Queues the alignment of n_pairs entries (triples[3 i .. 3 i + 3) = A, B, orient) over the LAST run's results behind that run on
 * hip_stream, as ambi_batch_path_compare queues its pairs: the given paths if the device does not hold them, the triples, one kernel
 * (a workgroup per pair, each with a history area of (dmax + 1)(dmax + 2) / 2 ints in device memory), then one device-to-host copy of
 * the block on the engine's copy stream.  dmax: 0 .. AMBI_ALIGN_DMAX_CAP (AMBI_COMPARE_DMAX_DEFAULT is a good default).  The request
 * keeps the set of given paths it was made with.  AMBI_ERR_STATE before any run; AMBI_ERR_ARG for a side that names no unit, no
 * `which` or no given path, an orientation other than 0 and 1, or another dmax; AMBI_ERR_TOO_LARGE when the run area,
 * 16 * n_pairs * max(dmax, 1) bytes, exceeds 1 GiB (nothing is queued); AMBI_ERR_UNSUPPORTED after ambi_batch_run_sharded. */
int ambi_batch_path_align(ambi_batch_t* b, const int32_t* triples, int32_t n_pairs, int32_t dmax, void* hip_stream);
/* Blocks until the results are in host memory.  Makes the run's results final first (ambi_batch_wait) and aligns once more if that
 * changed them after the request was queued. */
int ambi_batch_path_align_wait(ambi_batch_t* b);
/* The header of entry `pair` of the last request; AMBI_ERR_STATE without a waited-for alignment of the last run. */
int ambi_batch_path_align_result(const ambi_batch_t* b, int32_t pair, ambi_path_align_t* out);
/* The runs of entry `pair`: *n_runs = their number; out[0 .. n_runs) are written when cap >= n_runs (AMBI_ERR_ARG for a smaller
 * cap with *n_runs set, so a caller can ask with cap = 0 first; out may be NULL then). */
int ambi_batch_path_align_runs(const ambi_batch_t* b, int32_t pair, ambi_align_run_t* out, int32_t cap, int32_t* n_runs);
/* The results in DEVICE memory, for collectives: ambi_path_align_t[n_pairs] padded to 16 bytes, then at *runs_off
 * ambi_align_run_t[n_pairs * max(dmax, 1)] -- a fixed stride of max(dmax, 1) runs per entry, so the layout does not depend on the
 * results; the slots at and behind n_runs are zero.  Valid after ambi_batch_path_align_wait until the next ambi_batch_path_align. */
int ambi_batch_path_align_device(ambi_batch_t* b, void** dev_ptr, int64_t* bytes, int64_t* runs_off);

/* Path coordinates ON THE DEVICE (ambi_path_coords_kernel, ambi_path_lift_kernel): every other result speaks of a path in cells; this
 * one speaks in base pairs.  With len(c) the length of segment |c|, a request scans every unit's path into a 64-bit plane,
 *   plane[k] = base pairs in front of cell k, k = 0 .. P, plane[P] = the amplicon's length,
 * which stays on the device, and answers a batch of lift-over queries from it: amplicon position -> cell, segment, offset in the
 * segment.  Position p is byte p of ambi_batch_sequence's output for the same unit (the lengths follow its convention: 0-based,
 * half-open, end - start), so this is also where byte p of an amplicon FASTA comes from.  It replaces downloading every path
 * (ambi_batch_unit_path) and walking it on the host with a table of segment lengths, once per read when reads are aligned to the
 * amplicon; 32 bytes per unit and 32 bytes per query travel to the host.  Limits: a length is 0 .. 2^31 - 1 and a path has at most
 * 2^22 cells, so every offset is below 2^53. */
typedef struct {
    int32_t status;        /* the unit's status; for a unit with a negative status or without a path the status of a failed side of
                              the path comparison (AMBI_ERR_BAD_INPUT when the unit's own status is not negative): cells and all
                              that follows are then 0 */
    int32_t cells;         /* P of the scanned path */
    int32_t runs;          /* maximal stretches of cells counting up by one, as the sequence request counts them */
    int32_t empty_cells;   /* cells of length 0 */
    int64_t bp_len;        /* the amplicon's length, plane[P] */
    int64_t bp_minus;      /* base pairs crossed on the '-' strand */
} ambi_unit_coords_t;
typedef struct {
    int32_t unit;
    int32_t reserved;      /* 0 */
    int64_t pos;           /* position in the unit's amplicon, 0-based */
} ambi_lift_query_t;
typedef struct {
    int32_t status;        /* 0, or the failed unit's ambi_unit_coords_t::status */
    int32_t cell;          /* the LAST k in [0, P) with plane[k] <= pos: of cells of length 0 none is ever named; -1 for pos < 0,
                              pos >= bp_len or a failed unit */
    int32_t seg;           /* the signed LOCAL segment id of that cell (+: '+' strand), 0 where cell is -1 */
    int32_t reserved;      /* 0 */
    int64_t seg_off;       /* offset from the segment's start in GENOME orientation: pos - cell_start on a '+' cell,
                              len - 1 - (pos - cell_start) on a '-' cell; the segment's start + seg_off is the genomic coordinate and
                              the base there, complemented on '-', is byte pos of the sequence.  -1 where cell is -1 */
    int64_t cell_start;    /* plane[cell], -1 where cell is -1 */
} ambi_lift_t;
/* A unit's segment lengths in base pairs, len[i] for local segment i + 1; n must be the unit's n_seg and every length 0 .. 2^31 - 1
 * (what a .lh can express), otherwise AMBI_ERR_ARG.  A second call replaces the first.  Units built from a graph
 * (ambi_batch_add_graph_chr) have end - start of their SEG lines already; a unit nobody gave lengths has lengths of 0: its bp_len is
 * 0 and every query into it is out of range.  AMBI_ERR_STATE after ambi_batch_run_sharded. */
int ambi_batch_set_unit_seg_lengths(ambi_batch_t* b, int32_t unit, const int64_t* len, int32_t n);
/* Queues the scan of EVERY unit's path ambi_batch_unit_path(unit, which) of the LAST run and, behind it, the n queries q[0 .. n) on
 * hip_stream: the length image if the device does not hold this version of it, the queries, two kernels, then one device-to-host
 * copy of the block on the engine's copy stream; hip_stream is not blocked.  n = 0 is "just the coordinates" (q may be NULL).  The
 * request keeps a copy of the queries; no request ever answers from the plane of another run or another `which`.  The plane
 * (8 bytes per cell of every unit's path capacity plus one) is allocated at the first request; a failure to allocate it is this
 * call's error.  AMBI_ERR_STATE before any run; AMBI_ERR_ARG for another `which`, n < 0 or a query whose unit is not in the batch;
 * AMBI_ERR_UNSUPPORTED after ambi_batch_run_sharded. */
int ambi_batch_path_coords(ambi_batch_t* b, int32_t which, const ambi_lift_query_t* q, int32_t n, void* hip_stream);
/* Blocks until the results are in host memory.  Makes the run's results final first (ambi_batch_wait) and scans and lifts once more,
 * with the request's own copy of the queries, if that changed them after the request was queued. */
int ambi_batch_path_coords_wait(ambi_batch_t* b);
/* A unit's summary / the answer to query i of the last request; AMBI_ERR_STATE without a waited-for request of the last run. */
int ambi_batch_path_coords_summary(const ambi_batch_t* b, int32_t unit, ambi_unit_coords_t* out);
int ambi_batch_path_coords_result(const ambi_batch_t* b, int32_t query, ambi_lift_t* out);
/* The entries [first, first + n) of a unit's plane to host memory, first + n <= cells + 1; nothing else is downloaded.  Two reads
 * turn a fold's arm (ambi_batch_unit_fold_plane) or an uncovered stretch (ambi_batch_unit_evidence_depth) into base pairs: it
 * replaces a host-side prefix sum over the downloaded path.  AMBI_ERR_ARG for a range outside 0 .. cells + 1. */
int ambi_batch_path_coords_copy(ambi_batch_t* b, int32_t unit, int64_t first, int64_t n, int64_t* out);
/* The plane area where it was computed (DEVICE memory): *bytes in all, unit u's slice of int64 at unit_off[u] (a multiple of 16),
 * entries 0 .. cells valid and stale values behind them; unit_off may be NULL, else cap >= the batch's units.  Valid after
 * ambi_batch_path_coords_wait until the next ambi_batch_path_coords. */
int ambi_batch_path_coords_plane_device(ambi_batch_t* b, void** dev_ptr, int64_t* bytes, int64_t* unit_off, int32_t cap);
/* The block in DEVICE memory, for collectives: ambi_unit_coords_t[units], then at *results_off ambi_lift_t[n].  Valid as above. */
int ambi_batch_path_coords_device(ambi_batch_t* b, void** dev_ptr, int64_t* bytes, int64_t* results_off);

/* The nucleotide sequence of every unit's path, assembled ON THE DEVICE (ambi_seq_extents_kernel, ambi_seq_fill_kernel): the
 * reference's last step, which it leaves to scripts around bedtools (script/main.py:537-588 bfb2fasta: a BED line per path cell
 * through `bedtools getfasta -s`, all records joined).
 *   sequence of a path = the concatenation over its cells c of seq(|c|) for c > 0 and of the reverse complement of seq(|c|) for
 *     c < 0; `which` selects the cells ambi_batch_unit_path(unit, which) returns; a unit with a negative status or without a path
 *     has length 0.
 *   complement = one byte-to-byte table: ACGTUMRWSYKVHDBN -> TGCAAKYWSRMBDHVN and the same in lower case; every other byte value
 *     (0-255) maps to itself; case is preserved.
 * The bases come from the graph (ambi_graph_set_sequences / ambi_graph_read_fasta, copied by ambi_batch_add_chromosome*) or from
 * ambi_batch_set_unit_sequences (local segment i + 1 = bases[seg_off[i] .. seg_off[i + 1]); not after ambi_batch_run_sharded).  They
 * form a host-side image of the batch that travels to the device at the first request: ambi_batch_upload and ambi_batch_run are
 * what they are without it.
 * ambi_batch_sequence assembles the units [first_unit, first_unit + n_units) of the LAST run behind that run on hip_stream.  It
 *   fetches the units' lengths (one small device-to-host trip: it blocks until the run's kernels have finished) and sizes the
 *   output block from them; when they sum to more than max_bytes > 0 it returns AMBI_ERR_TOO_LARGE and assembles nothing -- the
 *   lengths stay readable, so a caller can split the range.  AMBI_ERR_STATE before any run or without sequences, AMBI_ERR_ARG
 *   for another `which` or a range outside the batch.  After ambi_batch_run_sharded the call goes to every share on its own
 *   stream (the limit holds for the sum over the shares).
 * ambi_batch_sequence_wait blocks until the request is done; it makes the run's results final first (ambi_batch_wait) and
 *   assembles once more if that changed them (it can then return AMBI_ERR_TOO_LARGE itself).
 * ambi_batch_unit_sequence_len: a unit's length in bytes, from ambi_batch_sequence on (final after the wait); AMBI_ERR_ARG for a
 *   unit outside the request.
 * ambi_batch_unit_sequence: bytes [first, first + count) of one unit's sequence to host memory; nothing else is downloaded.
 * ambi_batch_sequence_device: the block in DEVICE memory and, in unit_off[0 .. n_units of the batch) (cap entries), every unit's
 *   byte offset in it (a multiple of 16; -1 for a unit outside the request); valid until the next ambi_batch_sequence or run; not
 *   available for a sharded batch. */
int ambi_batch_set_unit_sequences(ambi_batch_t* b, int32_t unit, const uint8_t* bases, const int64_t* seg_off);
int ambi_batch_sequence(ambi_batch_t* b, int32_t which, int32_t first_unit, int32_t n_units, int64_t max_bytes, void* hip_stream);
int ambi_batch_sequence_wait(ambi_batch_t* b);
int ambi_batch_unit_sequence_len(const ambi_batch_t* b, int32_t unit, int64_t* bases);
int ambi_batch_unit_sequence(ambi_batch_t* b, int32_t unit, int64_t first, int64_t count, uint8_t* out);
int ambi_batch_sequence_device(ambi_batch_t* b, void** dev_ptr, int64_t* bytes, int64_t* unit_off, int32_t cap);

/* Expands runs into cells: run r writes dev_cells[dev_cell_off[r] + k] = dev_run_start[r] + k, k < dev_run_len[r]
 * (dev_cell_off = exclusive prefix sum of the lengths, int64).  All pointers are device memory of the current device. */
int ambi_expand_runs(const int32_t* dev_run_start, const int32_t* dev_run_len, const int64_t* dev_cell_off, int64_t n_runs,
                     int32_t* dev_cells, int64_t cell_cap, void* hip_stream);

typedef struct {
    int32_t status;
    int32_t bias;             /* localhap.cpp:141-146 */
    int32_t n_nodes;          /* K */
    int32_t bkp_len;
    int32_t path_len;         /* getBFB result */
    int32_t path_indel_len;   /* after indelBFB */
    int32_t indel_printed;    /* reference prints the indel caption + path */
    int32_t n_out_junc;
    int32_t first_forward;    /* 1 forward seed / 0 reversed seed / -1 */
    int32_t evaluated;        /* order evaluations of the reference's sequential scan */
    int64_t num_orders;       /* R */
    int64_t first_valid;      /* index of the first valid order, -1 if none */
    double inv_cn_sum;        /* localhap.cpp:150-153 */
    int32_t path_indel_stored; /* 1: indelBFB changed the path (a second path is held); 0: it equals the getBFB path */
    int32_t reserved;
} ambi_unit_result_t;
int ambi_batch_unit_result(const ambi_batch_t* b, int32_t unit, ambi_unit_result_t* out);
/* which: 0 = getBFB path (LocalGenomicMap.cpp:3660-3671), 1 = after indelBFB (:3746-3837). Returns length or <0. */
int ambi_batch_unit_path(const ambi_batch_t* b, int32_t unit, int32_t which, int32_t* out, int32_t cap);
int ambi_batch_unit_bkp(const ambi_batch_t* b, int32_t unit, int32_t* out, int32_t cap);
/* per local segment id 0..n (slot 0 unused): junction CN (2 per id), CN after getIndelBias, targetCN, fold-back map */
int ambi_batch_unit_prepare(const ambi_batch_t* b, int32_t unit, double* junc_cn, double* seg_cn, int32_t* target_cn,
                            int32_t* inv_junc_global);
/* DAG of the unit: node2pat / node2loop as [K][3] (absolute ids; a==0 empty), successor bit masks [K] */
int ambi_batch_unit_dag(const ambi_batch_t* b, int32_t unit, int32_t* node2pat, int32_t* node2loop, uint64_t* succ);
/* successor sets of the unit's K nodes as [K][nwords] 64-bit words (bit j of word j/64): a unit may have up to 255 nodes (64..255: a
 * "wide" unit, served by the plain four-word form of the DAG / lattice stages of LocalGenomicMap.cpp:3276-3409; ambi_batch_unit_dag's
 * succ[] carries the low word).  ambi_batch_unit_dag_words = the same with nwords = 2 (enough up to 127 nodes; kept from round 3). */
int ambi_batch_unit_dag_nwords(const ambi_batch_t* b, int32_t unit, int32_t nwords, uint64_t* succ);
int ambi_batch_unit_dag_words(const ambi_batch_t* b, int32_t unit, uint64_t* succ2);
int ambi_batch_unit_out_juncs(const ambi_batch_t* b, int32_t unit, int32_t* u, int32_t* v, int32_t* count, int32_t cap);
/* --all (localhap.cpp:38, LocalGenomicMap.cpp:3672-3695): after ambi_batch_run(b, AMBI_FLAG_ALL, ...) + wait, every
 * valid order of a unit in the reference's print order.  pass 0 = the first orientation (forward unless
 * AMBI_FLAG_REVERSED), pass 1 = the flipped orientation, which the reference runs only when the LAST order of pass 0
 * is invalid (count 0 otherwise).  all_orders: indices into the order table; all_paths: the expanded paths (absolute
 * signed ids) of valid orders [first, first+count) of the pass, cells[j*stride ...], lengths[j] (negative: capacity).
 * The unit's ordinary results (first valid order, path, indelBFB, output junctions) are those of the default mode;
 * ambi_unit_result_t.evaluated counts every order of the executed passes. */
int ambi_batch_all_count(ambi_batch_t* b, int32_t unit, int32_t pass, int64_t* count);
int ambi_batch_all_orders(ambi_batch_t* b, int32_t unit, int32_t pass, int64_t first, int64_t count, int64_t* order_idx);
int ambi_batch_all_paths(ambi_batch_t* b, int32_t unit, int32_t pass, int64_t first, int64_t count, int32_t* lengths, int32_t* cells,
                         int64_t stride);
/* --all for ONE wide sample on several GPUs (orders of a chromosome block-partitioned over ranks).  Every
 * rank holds the same batch; ambi_batch_all_set_shard(rank, world) before ambi_batch_run(AMBI_FLAG_ALL) makes a rank evaluate
 * the 64-order chunks c with c % world == rank (plus the last chunk of every unit, so that every rank knows by itself
 * whether the orientation flips, LocalGenomicMap.cpp:3691-3695).  After ambi_batch_wait the ranks merge the pool that
 * ambi_batch_all_device names -- validity bitmaps and undefined-order flags, as BYTES with MAX (disjoint contributions,
 * zero elsewhere): one all-reduce over RCCL -- and call ambi_batch_all_finish, which recounts and finalises the headers;
 * ambi_batch_all_count / _orders / _paths then answer on every rank as after a single-GPU run. */
int ambi_batch_all_set_shard(ambi_batch_t* b, int32_t rank, int32_t world);
int ambi_batch_all_device(ambi_batch_t* b, void** ptr, int64_t* bytes);
int ambi_batch_all_finish(ambi_batch_t* b);
/* Rows [first,first+count) of the unit's order table -- the reference's `orders` (LocalGenomicMap.cpp:3380-3409), row r = the r-th
 * topological order it pushes -- as count x K uint8 node ids.  (On the device a row of up to 63 nodes is the order's Lehmer code,
 * sum ceil(log2 m) bits for m = 1..K -- 8 bytes at 19 nodes -- and a byte per node above; this call unpacks.) */
int ambi_batch_unit_orders(ambi_batch_t* b, int32_t unit, int64_t first, int64_t count, uint8_t* out);

/* Per-kernel timing (HIP events on the streams the kernels are launched on, milliseconds): the average duration of
 * ONE launch of the kernel over the runs since timing was enabled; names are static strings.  A run launches every
 * kernel once (ambi_batch_slices: launches of every kernel per run, always 1; kept for compatibility).  Enable with
 * ambi_batch_set_timing(b, 1) before run. */
int ambi_batch_slices(const ambi_batch_t* b);
int ambi_batch_set_timing(ambi_batch_t* b, int32_t on);
/* The same for a subset of the kernels: bit k of `mask` = kernel index k of ambi_batch_kernel_time (0 prepare, 1 plan,
 * 2 image build, 3 enumerate, 4 scan, 5 finish (lean + list), 6 direct full finish); the others report -1.  Every pair of events is a marker in the
 * stream, and twelve of them per run cost ~4 % on the bench workload -- a timed region that needs one kernel's duration
 * asks for that kernel only. */
int ambi_batch_set_timing_mask(ambi_batch_t* b, uint32_t mask);
int ambi_batch_kernel_count(const ambi_batch_t* b);
int ambi_batch_kernel_time(const ambi_batch_t* b, int32_t idx, const char** name, float* ms);
/* Where the kernel sits in its run: start / end in ms from the start of the run's first kernel (mean over the timed runs; the
 * kernels run on several streams side by side, so these spans -- not the durations -- give the step's critical path); -1 when the
 * first kernel is not among the timed ones. */
int ambi_batch_kernel_span(const ambi_batch_t* b, int32_t idx, float* start_ms, float* end_ms);
/* bytes: inputs resident in HBM, order-table bytes written by the last run, result blob bytes */
int ambi_batch_traffic(const ambi_batch_t* b, int64_t* input_bytes, int64_t* order_bytes, int64_t* result_bytes);

/* ------------------------------------------------------------------------------------------------
 * Whole-sample helpers used by the CLI (host side, tiny): path text (printBFB, LocalGenomicMap.cpp:3411-3429),
 * BFB-TRX stitching (translocationBFB, :4052-4193), output-junction merge (localhap.cpp:267-316).
 * ---------------------------------------------------------------------------------------------- */
int64_t ambi_format_path(const ambi_graph_t* g, const int32_t* path, int32_t len, char* buf, int64_t cap);
/* paths: concatenated per-chromosome paths with offsets[n_chr+1]; result written to out (cap cells). Returns length. */
int ambi_translocation_bfb(const ambi_graph_t* g, int32_t* paths, const int64_t* offsets, int32_t n_chr, int32_t* out, int32_t cap);

/* ------------------------------------------------------------------------------------------------
 * ILP model of one chromosome (host side; the solve stays with the external `cbc`, localhap.cpp:179-181).
 * Replaces LocalGenomicMap::BFB_ILP (LocalGenomicMap.cpp:4397-4752): same rows, same row order, same in-row entry
 * order, generated in O(nnz) instead of the reference's O(n * numPat^2) assembly loop (:4464-4477).
 * seg_cn / junc_cn: the arrays ambi_batch_unit_prepare returns for the chromosome (local ids, slot 0 unused);
 * max_cn_total: sum of the CN of ALL segments of the graph at that point (:4708-4711).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ambi_ilp ambi_ilp_t;
int ambi_ilp_build(const ambi_graph_t* g, int32_t chr, const double* seg_cn, const double* junc_cn, int32_t bias,
                   double max_cn_total, int32_t juncs_info, ambi_ilp_t** out);
/* The same model with its entries written ON THE DEVICE: the host lists the rows (O(rows)),
 * ambi_ilp_fill_kernel writes the 12 bytes per non-zero (int32 column + f64 coefficient) with one thread per entry,
 * the arrays come back to the host.  Bit-identical to ambi_ilp_build.  kernel_ms (optional): mean device time of the
 * fill kernel, for the roofline (algorithmic bytes = 12 * nnz). */
int ambi_ilp_build_device(const ambi_graph_t* g, int32_t chr, const double* seg_cn, const double* junc_cn, int32_t bias,
                          double max_cn_total, int32_t juncs_info, float* kernel_ms, ambi_ilp_t** out);
/* Joint model of `--op sc_bfb` (LocalGenomicMap::BFB_ILP_SC, LocalGenomicMap.cpp:4754-5093) for chromosome `chr` of
 * n_graphs graphs with the same segmentation: seg_cn / fold_cn are n_graphs x n (graph-major; n = segments of the
 * chromosome): the segment copy numbers (first graph after its getIndelBias, localhap.cpp:497) and the fold-back copy
 * numbers juncCN[i][1] of every graph's own getJuncCN (LocalGenomicMap.cpp:4794).  Linking rows for every pair of graphs
 * (localhap.cpp:430-434).  The matrix is the one the reference builds, including its use of the running row counter in
 * the epsilon columns (LocalGenomicMap.cpp:4815) -- see DESIGN.md. */
int ambi_ilp_build_sc(const ambi_graph_t* g0, int32_t chr, int32_t n_graphs, const double* seg_cn, const double* fold_cn, ambi_ilp_t** out);
/* The joint model with its entries written ON THE DEVICE: the host lists the rows (O(rows)), ambi_ilp_fill_kernel writes
 * the 12 bytes per non-zero, the arrays come back to the host.  Bit-identical to ambi_ilp_build_sc.  kernel_ms as in
 * ambi_ilp_build_device (optional; mean of the last 4 of 5 launches).  AMBI_ERR_NO_DEVICE without a GPU.  AMBI_ERR_ARG
 * (and *out = NULL) beyond the limits of the row descriptor: n_graphs < 1 or > 2^23 - 1, a model of more than INT32_MAX
 * rows, a model with 2 * n_cols >= 2^31. */
int ambi_ilp_build_sc_device(const ambi_graph_t* g0, int32_t chr, int32_t n_graphs, const double* seg_cn, const double* fold_cn,
                             float* kernel_ms, ambi_ilp_t** out);
void ambi_ilp_destroy(ambi_ilp_t* p);
int ambi_ilp_sizes(const ambi_ilp_t* p, int64_t* n_rows, int64_t* nnz, int32_t* n_cols, int32_t* n_int);
/* CSR copy-out; infinity is +-DBL_MAX (OsiClp getInfinity()); any pointer may be NULL */
int ambi_ilp_copy(const ambi_ilp_t* p, int64_t* row_ptr, int32_t* col, double* val, double* row_lo, double* row_up,
                  double* col_lo, double* col_up, double* obj);
/* writes <path> as CPLEX-LP text with CoinUtils column names x<j> (what `cbc <prefix>.lp solve solu <prefix>.sol` reads) */
int ambi_ilp_write_lp(const ambi_ilp_t* p, const char* path);
/* <prefix>.mps beside <prefix>.lp, as the reference leaves it (LGM.cpp:4749): free-format MPS of the same model. */
int ambi_ilp_write_mps(const ambi_ilp_t* p, const char* path);

#ifdef __cplusplus
}
#endif
#endif /* AMBIGRAM_HIP_H */
