// ambigram_cli.cpp -- drop-in for `Ambigram --op bfb` (localhap.cpp:19-388) on top of the C ABI of the HIP engine.
//
// Same flags (localhap.cpp:22-40), same stdout lines in the same order, same side files (<prefix>.lp, <prefix>.sol via
// the external `cbc`, appended simulation_sv.txt and time.csv), same exit codes for unreadable .lh / missing .sol.
// The per-chromosome stages run on the GPU through libambigram_hip.so; the ILP model is built on the host
// (ambi_ilp_build) and solved by whatever `cbc` is on PATH, exactly as the reference shells out (localhap.cpp:179-181).
#include <algorithm>
#include <cctype>
#include <chrono>
#include <cstdint>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <sys/wait.h>
#include <string>
#include <vector>

#include "../../include/ambigram_hip.h"

namespace {

struct Args { std::map<std::string, std::string> kv; bool help = false; };

Args parse(int argc, char** argv) {
    Args a;
    for (int i = 1; i < argc; i++) {
        std::string t = argv[i];
        if (t == "--help") { a.help = true; continue; }
        if (t.rfind("--", 0) != 0) continue;
        std::string k = t.substr(2), v;
        size_t eq = k.find('=');
        if (eq != std::string::npos) { v = k.substr(eq + 1); k = k.substr(0, eq); }
        else if (i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0) v = argv[++i];
        else v = "true";
        a.kv[k] = v;
    }
    return a;
}
bool truthy(const std::string& s) { return s == "true" || s == "1" || s == "True"; }

void print_log(const ambi_graph_t* g, size_t* printed) {
    int64_t n = ambi_graph_log(g, nullptr, 0);
    std::string buf((size_t)n + 1, '\0');
    ambi_graph_log(g, &buf[0], n + 1);
    buf.resize((size_t)n);
    std::cout << buf.substr(*printed);
    *printed = buf.size();
}

std::string path_text(const ambi_graph_t* g, const std::vector<int32_t>& p) {
    int64_t n = ambi_format_path(g, p.data(), (int32_t)p.size(), nullptr, 0);
    std::string s((size_t)n + 1, '\0');
    ambi_format_path(g, p.data(), (int32_t)p.size(), &s[0], n + 1);
    s.resize((size_t)n);
    return s;
}

struct OutJ { int u, v; double cn; };
void merge_steps(std::vector<OutJ>& acc, int u, int v, double c, bool increase) {
    for (auto& j : acc)
        if ((j.u == u && j.v == v) || (j.u == -v && j.v == -u)) { if (increase) j.cn += c; return; }
    acc.push_back({u, v, c});
}

int die(const std::string& msg) { std::cerr << msg << std::endl; return 1; }

// `--op sc_bfb` (localhap.cpp:390-679): --in_lh is a comma-separated list of .lh files over the same segmentation; one
// joint ILP per chromosome (BFB_ILP_SC), the block k*numComp..(k+1)*numComp of its solution belongs to graph k.  All
// graphs x chromosomes are ONE reconstruct batch.  --juncdb / --junc_info are accepted and ignored, as in the reference.
int run_sc_bfb(Args& A) {
    auto t_begin = std::chrono::steady_clock::now();
    const std::string lh_list = A.kv["in_lh"], prefix = A.kv["lp_prefix"];
    const bool reversed = truthy(A.kv["reversed"]), all = truthy(A.kv["all"]);
    std::vector<std::string> files;
    { std::stringstream ss(lh_list); std::string t; while (std::getline(ss, t, ',')) if (!t.empty()) files.push_back(t); }   // strtok_r(.., ","): empty fields skipped
    if (files.empty()) return die("Cannot open file ");
    const int G = (int)files.size();
    std::vector<ambi_graph_t*> gs(G, nullptr);
    int rc;
    for (int k = 0; k < G; k++) {
        rc = ambi_graph_read_lh(files[k].c_str(), &gs[k]);
        if (rc == AMBI_ERR_OPEN) return die("Cannot open file " + files[k]);
        if (rc != 0) return die(std::string("input error: ") + ambi_error_string(rc));
        size_t printed = 0;
        print_log(gs[k], &printed);
    }
    {   // localhap.cpp:438-439: calculateHapDepth / calculateCopyNum a second time on the first graph
        int64_t before = ambi_graph_log(gs[0], nullptr, 0);
        if ((rc = ambi_graph_recalculate(gs[0])) != 0) return die(ambi_error_string(rc));
        size_t printed = (size_t)before;
        print_log(gs[0], &printed);
    }
    ambi_graph_t* g0 = gs[0];
    int32_t n_seg, n_junc, n_chr, ins_mode, con_mode;
    char main_chr[256];
    ambi_graph_sizes(g0, &n_seg, &n_junc, &n_chr);
    ambi_graph_props(g0, &ins_mode, &con_mode, main_chr, sizeof(main_chr));   // PROP of the first file (lhRawFn is cut at the first comma)
    for (int k = 1; k < G; k++) {
        int32_t ns, nj, nc;
        ambi_graph_sizes(gs[k], &ns, &nj, &nc);
        if (ns != n_seg || nc != n_chr) return die("sc_bfb: the graphs do not share one segmentation");
    }
    // probe batch: every graph x chromosome -- fold-back CNs of every graph (BFB_ILP_SC calls getJuncCN per graph,
    // LGM.cpp:4794), the first graph's getIndelBias (localhap.cpp:497) and its shortcut decision (:505)
    ambi_batch_t* probe; ambi_batch_create(&probe);
    for (int c = 0; c < n_chr; c++) for (int k = 0; k < G; k++)
        if ((rc = ambi_batch_add_chromosome(probe, gs[k], c, 0, nullptr, nullptr, 0)) < 0) return die(ambi_error_string(rc));
    if ((rc = ambi_batch_upload(probe)) != 0 || (rc = ambi_batch_run(probe, 0, nullptr)) != 0 || (rc = ambi_batch_download(probe)) != 0)
        return die(std::string("engine: ") + ambi_error_string(rc));
    std::vector<std::vector<double>> cn(G, std::vector<double>(n_seg));
    for (int k = 0; k < G; k++) ambi_graph_segments(gs[k], nullptr, nullptr, nullptr, nullptr, nullptr, cn[k].data());
    ambi_batch_t* b; ambi_batch_create(&b);
    std::vector<std::string> head(n_chr);
    std::vector<int> first_unit(n_chr, -1);   // unit of (chromosome c, graph 0) in the reconstruct batch; graph k follows at +k
    std::vector<char> plain(n_chr, 0);
    const double solver_timeout = A.kv.count("solver_timeout") ? atof(A.kv["solver_timeout"].c_str()) : 0;
    int units = 0;
    for (int c = 0; c < n_chr; c++) {
        int32_t s, e;
        ambi_graph_chromosome(g0, c, &s, &e);
        const int n = e - s + 1;
        std::vector<double> seg(G * (size_t)n), fold(G * (size_t)n), junc_cn(2 * (n + 1)), seg_cn(n + 1);
        ambi_unit_result_t pr0{};
        for (int k = 0; k < G; k++) {
            ambi_unit_result_t pr; ambi_batch_unit_result(probe, c * G + k, &pr);
            if (k == 0) pr0 = pr;
            ambi_batch_unit_prepare(probe, c * G + k, junc_cn.data(), seg_cn.data(), nullptr, nullptr);
            if (k == 0) for (int i = 1; i <= n; i++) cn[0][s - 1 + i - 1] = seg_cn[i];   // getIndelBias edits the first graph only
            for (int i = 0; i < n; i++) { seg[(size_t)k * n + i] = cn[k][s - 1 + i]; fold[(size_t)k * n + i] = junc_cn[2 * (i + 1) + 1]; }
        }
        if (pr0.status == AMBI_ST_SHORTCUT) { plain[c] = 1; continue; }   // no fold-back in the first graph: reference paths, nothing printed (:505-512)
        ambi_ilp_t* ilp = nullptr;
        // BFB_ILP_SC (LGM.cpp:4754-5093): from 32 segments up the entries are written on the device, as for `--op bfb`
        if (n >= 32) rc = ambi_ilp_build_sc_device(g0, c, G, seg.data(), fold.data(), nullptr, &ilp);
        else rc = ambi_ilp_build_sc(g0, c, G, seg.data(), fold.data(), &ilp);
        if (rc != 0) return die(ambi_error_string(rc));
        head[c] = "Declare done\n";
        for (int k = 0; k < G; k++) head[c] += "ILP formula done\n";
        head[c] += "Variable constrains done\n";
        ambi_ilp_write_mps(ilp, (prefix + ".mps").c_str());
        ambi_ilp_write_lp(ilp, (prefix + ".lp").c_str());
        ambi_ilp_destroy(ilp);
        (void)remove(("./" + prefix + ".sol").c_str());
        std::string cmd = "cbc " + prefix + ".lp solve solu " + prefix + ".sol";   // localhap.cpp:527-529
        if (solver_timeout > 0) { char t[64]; snprintf(t, sizeof(t), "timeout -k 5 %.0f ", solver_timeout); cmd = t + cmd; }
        std::cout.flush();
        const int solver_rc = system(cmd.c_str());
        if (solver_rc != 0) std::cerr << "ILP warning: `" << cmd << "` ended with status " << (WIFEXITED(solver_rc) ? WEXITSTATUS(solver_rc) : -1) << std::endl;
        first_unit[c] = units;
        for (int k = 0; k < G; k++) {
            rc = ambi_batch_add_chromosome_sol_block(b, gs[k], c, ("./" + prefix + ".sol").c_str(), k, G);
            if (rc == AMBI_ERR_SOL_OPEN) return die("ILP error: cannot open file ./" + prefix + ".sol");   // localhap.cpp:533-536
            if (rc < 0) return die(ambi_error_string(rc));
            units++;
        }
    }
    ambi_batch_destroy(probe);
    if (units > 0 && ((rc = ambi_batch_upload(b)) != 0 ||
                      (rc = ambi_batch_run(b, (reversed ? AMBI_FLAG_REVERSED : 0u) | (all ? AMBI_FLAG_ALL : 0u), nullptr)) != 0 ||
                      (rc = ambi_batch_download(b)) != 0))
        return die(std::string("engine: ") + ambi_error_string(rc));
    std::vector<std::vector<std::vector<int32_t>>> paths(G, std::vector<std::vector<int32_t>>(n_chr));
    int refused = 0;
    for (int c = 0; c < n_chr; c++) {
        int32_t s, e;
        ambi_graph_chromosome(g0, c, &s, &e);
        auto reference_path = [&](int k) { paths[k][c].clear(); for (int i = s; i <= e; i++) paths[k][c].push_back(i); };
        if (plain[c]) { for (int k = 0; k < G; k++) reference_path(k); continue; }
        std::cout << head[c];
        ambi_unit_result_t r0; ambi_batch_unit_result(b, first_unit[c], &r0);
        if (r0.status == AMBI_ST_INFEASIBLE) {   // localhap.cpp:543-551
            std::cout << "ILP is unsolvable.\n";
            for (int k = 0; k < G; k++) reference_path(k);
            continue;
        }
        for (int k = 0; k < G; k++) {
            const int u = first_unit[c] + k;
            ambi_unit_result_t r; ambi_batch_unit_result(b, u, &r);
            if (r.status != AMBI_ST_OK) {
                std::cout.flush();
                std::cerr << "sc_bfb: graph " << k << " chromosome " << c << ": " << ambi_error_string(r.status) << std::endl;
                refused++;
                continue;
            }
            std::vector<int32_t> p(r.path_len), q(r.path_indel_len);
            ambi_batch_unit_path(b, u, 0, p.data(), r.path_len);
            ambi_batch_unit_path(b, u, 1, q.data(), r.path_indel_len);
            if (all) {
                const int64_t stride = 2ll * r.path_len + 64;
                for (int pass = 0; pass < 2; pass++) {
                    int64_t nv = 0;
                    ambi_batch_all_count(b, u, pass, &nv);
                    for (int64_t lo = 0; lo < nv; lo += 64) {
                        const int64_t cnt = nv - lo < 64 ? nv - lo : 64;
                        std::vector<int32_t> len((size_t)cnt), cells((size_t)(cnt * stride));
                        if ((rc = ambi_batch_all_paths(b, u, pass, lo, cnt, len.data(), cells.data(), stride)) != 0) return die(std::string("sc_bfb --all: ") + ambi_error_string(rc));
                        for (int64_t j = 0; j < cnt; j++) {
                            if (len[j] < 0) return die(std::string("sc_bfb --all: ") + ambi_error_string(len[j]));
                            std::vector<int32_t> pj(cells.begin() + j * stride, cells.begin() + j * stride + len[j]);
                            std::cout << path_text(gs[k], pj) << std::endl;
                        }
                    }
                }
            } else
                std::cout << path_text(gs[k], p) << std::endl;
            if (r.indel_printed) std::cout << "BFB path with insertion, deletion, or duplication:\n" << path_text(gs[k], q) << std::endl;
            paths[k][c] = q;
        }
    }
    ambi_batch_destroy(b);
    if (refused) return die("sc_bfb: " + std::to_string(refused) + " unit(s) without a path");
    int path_len = 0, cn_sum = 0, max_cn_i = 0;
    for (int k = 0; k < G; k++) {   // localhap.cpp:654-660
        for (auto& p : paths[k]) path_len += (int)p.size();
        for (double v : cn[k]) { cn_sum += v; max_cn_i = (max_cn_i > v) ? max_cn_i : v; }
    }
    if (ins_mode == 2 || con_mode == 2) {   // :661-664: every graph
        if (!main_chr[0]) return die("BFB-TRX needs PROP M:<chr>");
        for (int k = 0; k < G; k++) {
            std::cout << "BFB with translocation:\n";
            std::vector<int64_t> offs(n_chr + 1, 0);
            for (int c = 0; c < n_chr; c++) offs[c + 1] = offs[c] + (int64_t)paths[k][c].size();
            std::vector<int32_t> flat((size_t)offs[n_chr] + 1), out((size_t)offs[n_chr] * 2 + 16);
            for (int c = 0; c < n_chr; c++) std::copy(paths[k][c].begin(), paths[k][c].end(), flat.begin() + offs[c]);
            int len = ambi_translocation_bfb(gs[k], flat.data(), offs.data(), n_chr, out.data(), (int32_t)out.size());
            if (len < 0) return die(ambi_error_string(len));
            out.resize(len);
            std::cout << path_text(gs[k], out) << std::endl;
        }
    }
    {   // time.csv (localhap.cpp:666-678): name of the first file up to its first '.', first graph's sizes, sums over all graphs
        auto t_end = std::chrono::steady_clock::now();
        std::ofstream tf("time.csv", std::ios_base::app);
        tf << files[0].substr(0, files[0].find(".")) << "," << n_seg << "," << 0 << "," << n_junc << "," << cn_sum << "," << path_len << ","
           << max_cn_i << "," << std::chrono::duration_cast<std::chrono::microseconds>(t_end - t_begin).count() / 1000000.0 << "\n";
    }
    for (auto* g : gs) ambi_graph_destroy(g);
    return 0;
}


// `--op bfb` (localhap.cpp:49-388).  One sample = the reference's behaviour, line for line.  Extensions (no counterpart in the
// reference, whose --in_lh names one file for this op): --in_lh may be a comma-separated LIST of samples -- every sample goes
// through its own ILP / solver stage in turn, then the chromosomes of ALL samples are reconstructed as ONE batch -- and
// --devices N|all deals that batch over several GPUs (ambi_batch_run_sharded: one host thread per device, round-robin).
// Every sample's stdout lines and side-file rows are what a run on that sample alone prints, in sample order.
// --cn_profile <file> (what the reference's commented-out CN.txt writer meant to report, localhap.cpp:318-351): after the run, one
// tab-separated row per segment -- sample, chromosome name, segment id, start, end, input CN, target CN, forward count, reverse
// count, count - target -- from the device's copy-number profile of the final paths (ambi_batch_profile); stdout is unchanged.
// --junc_profile <file> (the join the reference leaves to the reader of simulation_sv.txt, localhap.cpp:267-289 and :326-337): after
// the run, one tab-separated row per junction of the graph in file order -- sample, chromosome index (-1 for a junction between
// chromosomes, which belongs to no unit: count 0), source chromosome name, source segment id, source strand, target chromosome
// name, target segment id, target strand, input CN, count in the final path, count - CN -- from the device's junction usage
// profile of the final paths (ambi_batch_junc_profile); stdout and the side files are unchanged.
// --frag_profile <file> [--frags <file>] (the check a user with long reads does first: does the printed path contain the fragments that
// were given as evidence for it?): the lines of the fragment file (--frags; by default the file of --juncdb) are read as signed
// chains (ambi_graph_read_fragments: the graph stays as it is) and, after the run, one tab-separated row per fragment in file order --
// sample, chromosome index (-1 for a fragment of fewer than two cells or one that spans chromosomes, which belongs to no unit:
// 0 0 -1), fragment index, cells, occurrences, occurrences of the reverse complement, first position -- comes from the device's
// fragment support profile of the final paths (ambi_batch_frag_profile); stdout and the side files are unchanged.
// --evidence_profile <file> / --evidence_depth <file> (which parts of the printed path are backed by the fragments, and which junction
// traversals are not?): the fragment file as for --frag_profile; after the run the device's evidence depth profile of the final paths
// (ambi_batch_evidence_profile) gives one tab-separated row per junction in file order -- sample, chromosome index (-1 for a junction
// between chromosomes: 0 0 -1), junction index, count in the final path, those of them under at least one fragment occurrence, the
// smallest depth over them or -1 -- and the depth of every final path in run-length form -- sample, chromosome index, first step,
// steps, depth --; stdout and the side files are unchanged.
// --fold_profile <file> / --fold_arms <file> (where does the printed path fold back, how long are the palindromes and how deeply do
// they nest?): after the run the device's fold-back arm profile of the final paths (ambi_batch_fold_profile) gives, in
// --fold_profile, one tab-separated `U` row per chromosome -- U, sample, chromosome index, status, steps, folds, perfect, gapped and
// open folds, folds of no junction, longest arm and its step, largest cover and its step, covered steps, sum of the arms -- and
// one `J` row per junction in file order -- J, sample, chromosome index (-1 for a junction between chromosomes: 0 0), junction
// index, folds, longest arm --; in --fold_arms one row per fold -- sample, chromosome index, step k, alignment (-1: no arm, 0:
// perfect, 1..4), arm, nesting (cover[k] - 1) --; stdout and the side files are unchanged.
// --path_compare <file> [--truth <file>] [--compare_dmax N] (how close are two paths?): after the run the device's path comparison
// (ambi_batch_path_compare) gives one tab-separated `P` row per chromosome, the path of getBFB against the path after indelBFB -- P,
// sample, chromosome index, status, len_a, len_b, dmax, prefix, suffix, dist and lcs, each for the orientation as is and for the
// reverse complement --; with --truth also one `T` row per chromosome that has a truth line, the final path against that line.  A
// truth file has one line per chromosome in printing order: a path as it is printed here (`|` is ignored, ids are global), or `.`
// for none; an id outside the chromosome, a missing line or a line that is no path is an error found when the sample is read, in front of the run.  N: 0 .. 1024, default 64; a distance above it is -1.  stdout and the side
// files are unchanged.
// --path_align <file> (with --path_compare; where do the two paths differ?): behind the comparison every P and T row is aligned on the
// device (ambi_batch_path_align, one request, the cap of --compare_dmax) in the orientation with the smaller dist, ties as is.  Per
// row a header line -- A, the row's tag, chromosome index, orient, dist, n_runs -- then one line per run: D or I, a_pos, b_pos, len
// and the run's cells (of a for D, of Bo for I) as a printed path with global ids.  A row whose two dist are both -1 gets the header
// alone, with orient -1, dist -1 and 0 runs.
// --path_coords <file> / --lift <queries> --lift_out <file> (where in the genome does position p of the amplicon come from?): after the
// run the device's path coordinates of the final paths (ambi_batch_path_coords, one request) give, in --path_coords, one tab-separated
// row per chromosome -- cells, runs, cells of length 0, the amplicon's length in base pairs, the base pairs crossed on the '-' strand
// --; and in --lift_out one row per line `<chromosome index> <pos>` of the query file, in its order -- pos, cell, segment id, strand,
// the segment's chromosome name, genomic position (0-based: the segment's start + its offset) --, with `-1 0 . . -1` behind pos for
// a position outside the amplicon.  pos is the 0-based position in the chromosome's record of --out_fasta.  One sample, one device;
// a query file that cannot be read, a line that is no query or a chromosome index outside the sample is an error found when the
// sample is read, in front of the run.  stdout and the side files are unchanged.
// --ref_fasta <file> --out_fasta <file> (what script/main.py:537-588 bfb2fasta does with bedtools): the nucleotide sequence of every
// chromosome's final path, assembled on the device (ambi_batch_sequence) from the segments' bases chrom[start .. end) of the
// reference FASTA (0-based, half-open).  One record per chromosome that has a path, `>BFBPATH` when the sample has one chromosome
// and `>BFBPATH_<chromosome name>` otherwise, the sequence on ONE line.  Every line ends in "\n": the reference's script omits
// the newline behind the last line (main.py:579-588), a deviation on purpose (a text file ends in a newline; `cat` of two outputs
// stays a FASTA file).  The units are assembled in chunks of at most --fasta_chunk_bytes (default 256 MiB; a single unit beyond
// it goes alone); stdout is unchanged.
struct Sample {
    std::string lh;
    ambi_graph_t* g = nullptr;
    int32_t n_seg = 0, n_junc = 0, n_chr = 0, ins_mode = 0, con_mode = 0;
    char main_chr[256] = {0};
    std::vector<double> cn_all, cn_file;   // cn_file: the copy numbers as the .lh gives them (cn_all takes getIndelBias' edits)
    std::vector<int32_t> seg_start, seg_end;
    std::vector<std::string> head;       // lines the reference prints before a chromosome's path lines
    std::vector<int> unit;               // chromosome -> unit of the reconstruct batch
    int num_inv = 0;
    bool trx_before = false;             // PROP I1 / C1: g is the rebuilt graph, g_file the graph of the file (chromosome names / positions of restored paths)
    ambi_graph_t* g_file = nullptr;
    std::chrono::steady_clock::time_point t_begin;
};

int run_bfb(Args& A) {
    const std::string prefix = A.kv["lp_prefix"], juncs = A.kv.count("juncdb") ? A.kv["juncdb"] : "";
    const bool junc_info = truthy(A.kv["junc_info"]), reversed = truthy(A.kv["reversed"]), all = truthy(A.kv["all"]);
    const double solver_timeout = A.kv.count("solver_timeout") ? atof(A.kv["solver_timeout"].c_str()) : 0;   // extension: seconds, 0 = none
    const std::string cn_profile = A.kv.count("cn_profile") ? A.kv["cn_profile"] : "";
    const std::string junc_profile = A.kv.count("junc_profile") ? A.kv["junc_profile"] : "";
    const std::string frag_profile = A.kv.count("frag_profile") ? A.kv["frag_profile"] : "";
    const std::string frags = A.kv.count("frags") ? A.kv["frags"] : juncs;
    if (!frag_profile.empty() && frags.empty()) { std::cerr << "--frag_profile needs a fragment file: --frags <file> or --juncdb <file>" << std::endl; return 2; }
    const std::string evidence_profile = A.kv.count("evidence_profile") ? A.kv["evidence_profile"] : "";
    const std::string evidence_depth = A.kv.count("evidence_depth") ? A.kv["evidence_depth"] : "";
    const std::string evidence_opt = !evidence_profile.empty() ? "--evidence_profile" : !evidence_depth.empty() ? "--evidence_depth" : "";
    if (!evidence_opt.empty() && frags.empty()) { std::cerr << evidence_opt << " needs a fragment file: --frags <file> or --juncdb <file>" << std::endl; return 2; }
    const std::string fold_profile = A.kv.count("fold_profile") ? A.kv["fold_profile"] : "";
    const std::string fold_arms = A.kv.count("fold_arms") ? A.kv["fold_arms"] : "";
    const std::string fold_opt = !fold_profile.empty() ? "--fold_profile" : !fold_arms.empty() ? "--fold_arms" : "";
    const std::string path_compare = A.kv.count("path_compare") ? A.kv["path_compare"] : "", truth = A.kv.count("truth") ? A.kv["truth"] : "";
    const int compare_dmax = A.kv.count("compare_dmax") ? atoi(A.kv["compare_dmax"].c_str()) : AMBI_COMPARE_DMAX_DEFAULT;
    if (path_compare.empty() && (!truth.empty() || A.kv.count("compare_dmax"))) { std::cerr << "--truth and --compare_dmax go with --path_compare <file>" << std::endl; return 2; }
    if (!path_compare.empty() && (compare_dmax < 0 || compare_dmax > AMBI_COMPARE_DMAX_CAP)) { std::cerr << "--compare_dmax: 0 .. " << AMBI_COMPARE_DMAX_CAP << std::endl; return 2; }
    const std::string path_align = A.kv.count("path_align") ? A.kv["path_align"] : "";
    if (path_compare.empty() && !path_align.empty()) { std::cerr << "--path_align goes with --path_compare <file>" << std::endl; return 2; }
    if (!path_compare.empty() && A.kv.count("devices")) { std::cerr << "--path_compare: not available with --devices (a pair may span shares)" << std::endl; return 2; }
    const std::string path_coords = A.kv.count("path_coords") ? A.kv["path_coords"] : "", lift = A.kv.count("lift") ? A.kv["lift"] : "", lift_out = A.kv.count("lift_out") ? A.kv["lift_out"] : "";
    const std::string coords_opt = !path_coords.empty() ? "--path_coords" : !lift.empty() ? "--lift" : !lift_out.empty() ? "--lift_out" : "";
    if (lift.empty() != lift_out.empty()) { std::cerr << "--lift <queries> and --lift_out <file> go together" << std::endl; return 2; }
    if (!coords_opt.empty() && A.kv.count("devices")) { std::cerr << coords_opt << ": not available with --devices (one plane per share)" << std::endl; return 2; }
    const std::string ref_fasta = A.kv.count("ref_fasta") ? A.kv["ref_fasta"] : "", out_fasta = A.kv.count("out_fasta") ? A.kv["out_fasta"] : "";
    if (ref_fasta.empty() != out_fasta.empty()) { std::cerr << "--ref_fasta and --out_fasta go together" << std::endl; return 2; }
    const int64_t fasta_chunk = A.kv.count("fasta_chunk_bytes") ? atoll(A.kv["fasta_chunk_bytes"].c_str()) : (256ll << 20);
    int n_devices = 0;                   // 0: one device, the classic path; > 0: that many; -1: all visible
    std::vector<int32_t> device_list;    // or an explicit list of ordinals "0,1,1" (an ordinal may repeat: several shares on one device)
    if (A.kv.count("devices")) {
        const std::string d = A.kv["devices"];
        if (d.find(',') != std::string::npos) {
            std::stringstream ss(d);
            std::string t;
            while (std::getline(ss, t, ',')) if (!t.empty()) device_list.push_back(atoi(t.c_str()));
            n_devices = (int)device_list.size();
        } else n_devices = (d == "all") ? -1 : atoi(d.c_str());
    }
    std::vector<std::string> files;
    {
        std::stringstream ss(A.kv["in_lh"]);
        std::string f;
        while (std::getline(ss, f, ',')) if (!f.empty()) files.push_back(f);
        if (files.empty()) files.push_back(A.kv["in_lh"]);
    }
    if (!truth.empty() && files.size() > 1) { std::cerr << "--truth: one sample only (a truth file has one line per chromosome of one sample)" << std::endl; return 2; }
    if (!coords_opt.empty() && files.size() > 1) { std::cerr << coords_opt << ": one sample only (a query names a chromosome of one sample)" << std::endl; return 2; }
    std::vector<ambi_lift_query_t> lift_q;           // --lift: the queries in file order, unit = chromosome index until the units are known
    std::vector<std::vector<int32_t>> truth_cells;   // --truth: [chromosome] the line's path in local ids, empty for `.`
    int rc;
    std::vector<Sample> samples(files.size());
    ambi_batch_t* b; ambi_batch_create(&b);
    int n_units = 0;
    for (size_t si = 0; si < files.size(); si++) {
        Sample& S = samples[si];
        S.lh = files[si];
        S.t_begin = std::chrono::steady_clock::now();
        rc = ambi_graph_read_lh(S.lh.c_str(), &S.g);
        if (rc == AMBI_ERR_OPEN) return die("Cannot open file " + S.lh);            // Graph.cpp:111-114
        if (rc != 0) return die(std::string("input error: ") + ambi_error_string(rc));
        ambi_graph_t* g = S.g;
        size_t printed = 0;
        if (!cn_profile.empty()) {
            // PROP I1 / C1 / I2 / C2: the printed paths are rebuilt on the host (virusBFB, translocationBFB) and are not the device's paths
            ambi_graph_props(g, &S.ins_mode, &S.con_mode, S.main_chr, sizeof(S.main_chr));
            if (ambi_graph_trx_before(g, nullptr, 0) > 0 || S.ins_mode == 2 || S.con_mode == 2) {
                std::cerr << "--cn_profile: " << S.lh << " is a PROP I1 / C1 / I2 / C2 sample; its printed paths are rebuilt on the host and have no device profile" << std::endl;
                return 2;
            }
        }
        if (!junc_profile.empty()) {
            ambi_graph_props(g, &S.ins_mode, &S.con_mode, S.main_chr, sizeof(S.main_chr));
            if (ambi_graph_trx_before(g, nullptr, 0) > 0 || S.ins_mode == 2 || S.con_mode == 2) {
                std::cerr << "--junc_profile: " << S.lh << " is a PROP I1 / C1 / I2 / C2 sample; its printed paths are rebuilt on the host and have no device profile" << std::endl;
                return 2;
            }
        }
        if (!frag_profile.empty()) {
            ambi_graph_props(g, &S.ins_mode, &S.con_mode, S.main_chr, sizeof(S.main_chr));
            if (ambi_graph_trx_before(g, nullptr, 0) > 0 || S.ins_mode == 2 || S.con_mode == 2) {
                std::cerr << "--frag_profile: " << S.lh << " is a PROP I1 / C1 / I2 / C2 sample; its printed paths are rebuilt on the host and have no device profile" << std::endl;
                return 2;
            }
            if ((rc = ambi_graph_read_fragments(g, frags.c_str())) != 0) return die("--frags " + frags + ": " + ambi_error_string(rc));
        }
        if (!evidence_opt.empty()) {
            ambi_graph_props(g, &S.ins_mode, &S.con_mode, S.main_chr, sizeof(S.main_chr));
            if (ambi_graph_trx_before(g, nullptr, 0) > 0 || S.ins_mode == 2 || S.con_mode == 2) {
                std::cerr << evidence_opt << ": " << S.lh << " is a PROP I1 / C1 / I2 / C2 sample; its printed paths are rebuilt on the host and have no device profile" << std::endl;
                return 2;
            }
            if (frag_profile.empty() && (rc = ambi_graph_read_fragments(g, frags.c_str())) != 0) return die("--frags " + frags + ": " + ambi_error_string(rc));
        }
        if (!fold_opt.empty()) {
            ambi_graph_props(g, &S.ins_mode, &S.con_mode, S.main_chr, sizeof(S.main_chr));
            if (ambi_graph_trx_before(g, nullptr, 0) > 0 || S.ins_mode == 2 || S.con_mode == 2) {
                std::cerr << fold_opt << ": " << S.lh << " is a PROP I1 / C1 / I2 / C2 sample; its printed paths are rebuilt on the host and have no device profile" << std::endl;
                return 2;
            }
        }
        if (!coords_opt.empty()) {
            ambi_graph_props(g, &S.ins_mode, &S.con_mode, S.main_chr, sizeof(S.main_chr));
            if (ambi_graph_trx_before(g, nullptr, 0) > 0 || S.ins_mode == 2 || S.con_mode == 2) {
                std::cerr << coords_opt << ": " << S.lh << " is a PROP I1 / C1 / I2 / C2 sample; its printed paths are rebuilt on the host and have no device coordinates" << std::endl;
                return 2;
            }
            if (!lift.empty()) {   // the query file is read here, in front of anything printed or run: `<chromosome index> <pos>` per line
                std::ifstream qf(lift);
                if (!qf) return die("Cannot open file " + lift);
                int32_t ns, nj, nc;
                ambi_graph_sizes(g, &ns, &nj, &nc);
                std::string line;
                for (int ln = 1; std::getline(qf, line); ln++) {
                    long long c = 0, pos = 0; char tail = 0;
                    if (sscanf(line.c_str(), "%lld %lld %c", &c, &pos, &tail) != 2) { std::cerr << "--lift: line " << ln << " of " << lift << " is no query (<chromosome index> <pos>)" << std::endl; return 2; }
                    if (c < 0 || c >= nc) { std::cerr << "--lift: chromosome " << c << " on line " << ln << " of " << lift << " lies outside the sample (0 .. " << nc - 1 << ")" << std::endl; return 2; }
                    lift_q.push_back(ambi_lift_query_t{(int32_t)c, 0, (int64_t)pos});
                }
            }
        }
        if (!path_compare.empty()) {
            ambi_graph_props(g, &S.ins_mode, &S.con_mode, S.main_chr, sizeof(S.main_chr));
            if (ambi_graph_trx_before(g, nullptr, 0) > 0 || S.ins_mode == 2 || S.con_mode == 2) {
                std::cerr << "--path_compare: " << S.lh << " is a PROP I1 / C1 / I2 / C2 sample; its printed paths are rebuilt on the host and have no device comparison" << std::endl;
                return 2;
            }
            if (!truth.empty()) {   // the truth file is read here, in front of anything printed or run: one line per chromosome, in printing order
                std::ifstream tf(truth);
                if (!tf) return die("Cannot open file " + truth);
                int32_t ns, nj, nc;
                ambi_graph_sizes(g, &ns, &nj, &nc);
                truth_cells.assign((size_t)nc, std::vector<int32_t>());
                for (int c = 0; c < nc; c++) {
                    std::string line;
                    if (!std::getline(tf, line)) { std::cerr << "--truth: " << truth << " has no line for chromosome " << c << std::endl; return 2; }
                    while (!line.empty() && isspace((unsigned char)line.back())) line.pop_back();
                    if (line == ".") continue;
                    int32_t s, e;
                    ambi_graph_chromosome(g, c, &s, &e);
                    // a path as it is printed: <id><+|->..., `|` between fold-back arms ignored, ids global
                    size_t at = 0;
                    while (at < line.size()) {
                        if (line[at] == '|' || isspace((unsigned char)line[at])) { at++; continue; }
                        long id = 0; size_t digits = 0;
                        while (at < line.size() && isdigit((unsigned char)line[at]) && digits < 9) { id = id * 10 + (line[at] - '0'); at++; digits++; }
                        if (digits == 0 || at >= line.size() || (line[at] != '+' && line[at] != '-')) { std::cerr << "--truth: line " << c + 1 << " of " << truth << " is no path (<id><+|-> ...)" << std::endl; return 2; }
                        if (id < s || id > e) { std::cerr << "--truth: segment " << id << " on line " << c + 1 << " of " << truth << " lies outside chromosome " << c << " (" << s << " .. " << e << ")" << std::endl; return 2; }
                        truth_cells[(size_t)c].push_back((int32_t)(line[at] == '+' ? id - s + 1 : -(id - s + 1)));
                        at++;
                    }
                    if (truth_cells[(size_t)c].empty()) { std::cerr << "--truth: line " << c + 1 << " of " << truth << " is empty (`.`: no truth for the chromosome)" << std::endl; return 2; }
                }
            }
        }
        if (!out_fasta.empty()) {
            ambi_graph_props(g, &S.ins_mode, &S.con_mode, S.main_chr, sizeof(S.main_chr));
            if (ambi_graph_trx_before(g, nullptr, 0) > 0 || S.ins_mode == 2 || S.con_mode == 2) {
                std::cerr << "--out_fasta: " << S.lh << " is a PROP I1 / C1 / I2 / C2 sample; its printed paths are rebuilt on the host and have no device sequence" << std::endl;
                return 2;
            }
            if ((rc = ambi_graph_read_fasta(g, ref_fasta.c_str())) != 0) return die("--ref_fasta " + ref_fasta + ": " + ambi_error_string(rc));
        }
        // PROP I1 / C1 (TRX-BFB, localhap.cpp:79-88): the graph has been rebuilt while loading; the reference leaves it in ./new.lh
        S.trx_before = ambi_graph_trx_before(g, nullptr, 0) > 0;
        if (S.trx_before) { (void)ambi_graph_write_lh(g, "./new.lh"); if ((rc = ambi_graph_trx_original(g, &S.g_file)) != 0) return die(ambi_error_string(rc)); }
        print_log(g, &printed);
        if (!juncs.empty()) { if ((rc = ambi_graph_read_juncs(g, juncs.c_str())) != 0) return die(ambi_error_string(rc)); print_log(g, &printed); }
        ambi_graph_sizes(g, &S.n_seg, &S.n_junc, &S.n_chr);
        ambi_graph_props(g, &S.ins_mode, &S.con_mode, S.main_chr, sizeof(S.main_chr));
        S.cn_all.resize(S.n_seg); S.seg_start.resize(S.n_seg); S.seg_end.resize(S.n_seg);
        ambi_graph_segments(g, nullptr, nullptr, S.seg_start.data(), S.seg_end.data(), nullptr, S.cn_all.data());
        S.cn_file = S.cn_all;
        S.head.assign(S.n_chr, ""); S.unit.assign(S.n_chr, -1);
        // Two batches, every chromosome a unit:
        //   probe batch   -- localhap.cpp:136-170 for all chromosomes of the sample at once: junction CNs, bias, getIndelBias, shortcut;
        //   solve         -- per chromosome, in order: ILP model -> <prefix>.lp/.mps -> `cbc` -> <prefix>.sol (the reference
        //                    reuses the same file names for every chromosome, so each .sol is taken in right after its solve);
        //   reconstruct batch -- localhap.cpp:222-262 for all chromosomes (of all samples) at once.
        // This program's own stdout lines come out in the reference's order (per chromosome: the three ILP progress lines, then
        // the path lines); they are held back until the reconstruct batch is done, so only the solver's own chatter, which
        // the reference interleaves between them, moves to the front.  Both batches take their streams, events, pinned words and
        // device blocks from the engine's per-device pool: one resident context serves them in turn.
        ambi_batch_t* probe; ambi_batch_create(&probe);
        for (int c = 0; c < S.n_chr; c++)
            if ((rc = ambi_batch_add_chromosome(probe, g, c, 0, nullptr, nullptr, 0)) < 0) return die(ambi_error_string(rc));
        if ((rc = ambi_batch_upload(probe)) != 0 || (rc = ambi_batch_run(probe, 0, nullptr)) != 0 || (rc = ambi_batch_download(probe)) != 0)
            return die(std::string("engine: ") + ambi_error_string(rc));
        for (int c = 0; c < S.n_chr; c++) {
            int32_t s, e;
            ambi_graph_chromosome(g, c, &s, &e);
            const int n = e - s + 1;
            ambi_unit_result_t pr; ambi_batch_unit_result(probe, c, &pr);
            std::vector<double> junc_cn(2 * (n + 1)), seg_cn(n + 1);
            std::vector<int32_t> inv(n + 1);
            ambi_batch_unit_prepare(probe, c, junc_cn.data(), seg_cn.data(), nullptr, inv.data());
            // getIndelBias of chromosome c has edited its segment CNs (localhap.cpp:147); the ILP of chromosome c sees the
            // edits of chromosomes <= c only (its loop bound is the CN sum over ALL segments, LGM.cpp:4708-4711)
            for (int i = 1; i <= n; i++) { S.cn_all[s - 1 + i - 1] = seg_cn[i]; if (inv[i] >= 0) S.num_inv++; }
            if (pr.status == AMBI_ST_SHORTCUT) {
                if ((rc = ambi_batch_add_chromosome(b, g, c, 0, nullptr, nullptr, 0)) < 0) return die(ambi_error_string(rc));
                S.unit[c] = rc; n_units++;
                continue;
            }
            double max_cn = 0;
            for (double v : S.cn_all) max_cn += v;
            ambi_ilp_t* ilp = nullptr;
            // BFB_ILP (LGM.cpp:4397-4752): the rows are listed on the host, the non-zeros (56.5 M at 256 segments) written by
            // ambi_ilp_fill_kernel on the device; small chromosomes are not worth the launch and take the host generator
            if (n >= 32) rc = ambi_ilp_build_device(g, c, seg_cn.data(), junc_cn.data(), pr.bias, max_cn, junc_info ? 1 : 0, nullptr, &ilp);
            else rc = ambi_ilp_build(g, c, seg_cn.data(), junc_cn.data(), pr.bias, max_cn, junc_info ? 1 : 0, &ilp);
            if (rc != 0) return die(ambi_error_string(rc));
            S.head[c] = "Declare done\nILP formula done\nVariable constrains done\n";
            ambi_ilp_write_mps(ilp, (prefix + ".mps").c_str());   // LGM.cpp:4749-4750: both side files
            ambi_ilp_write_lp(ilp, (prefix + ".lp").c_str());
            ambi_ilp_destroy(ilp);
            (void)remove(("./" + prefix + ".sol").c_str());        // a stale .sol of an earlier chromosome or run must not pass for this solve
            std::string cmd = "cbc " + prefix + ".lp solve solu " + prefix + ".sol";   // localhap.cpp:179-181
            if (solver_timeout > 0) { char t[64]; snprintf(t, sizeof(t), "timeout -k 5 %.0f ", solver_timeout); cmd = t + cmd; }
            std::cout.flush();
            const int solver_rc = system(cmd.c_str());
            // the reference ignores the exit status (a missing .sol is what it notices, localhap.cpp:187-190); say what happened
            if (solver_rc != 0) {
                const int code = WIFEXITED(solver_rc) ? WEXITSTATUS(solver_rc) : -1;
                if (solver_timeout > 0 && code == 124) std::cerr << "ILP error: cbc did not finish within " << solver_timeout << " s (chromosome " << c << ")" << std::endl;
                else std::cerr << "ILP warning: `" << cmd << "` ended with status " << code << std::endl;
            }
            rc = ambi_batch_add_chromosome_sol(b, g, c, ("./" + prefix + ".sol").c_str());
            if (rc == AMBI_ERR_SOL_OPEN) return die("ILP error: cannot open file ./" + prefix + ".sol");   // localhap.cpp:187-190
            if (rc < 0) return die(ambi_error_string(rc));
            S.unit[c] = rc; n_units++;
        }
        ambi_batch_destroy(probe);
    }
    const uint32_t flags = (reversed ? AMBI_FLAG_REVERSED : 0u) | (all ? AMBI_FLAG_ALL : 0u);
    if (n_devices != 0) rc = ambi_batch_run_sharded(b, flags, device_list.empty() ? nullptr : device_list.data(), n_devices);
    else if ((rc = ambi_batch_upload(b)) == 0 && (rc = ambi_batch_run(b, flags, nullptr)) == 0) rc = ambi_batch_download(b);
    if (rc != 0) return die(std::string("engine: ") + ambi_error_string(rc));
    if (!cn_profile.empty()) {
        if ((rc = ambi_batch_profile(b, 1, nullptr)) != 0 || (rc = ambi_batch_profile_wait(b)) != 0) return die(std::string("engine: ") + ambi_error_string(rc));
        FILE* pf = fopen(cn_profile.c_str(), "w");
        if (!pf) return die("Cannot open file " + cn_profile);
        for (Sample& S : samples)
            for (int c = 0; c < S.n_chr; c++) {
                int32_t s, e;
                ambi_graph_chromosome(S.g, c, &s, &e);
                const int n = e - s + 1;
                std::vector<int32_t> fwd(n + 1), rev(n + 1), target(n + 1);
                if ((rc = ambi_batch_unit_path_cn(b, S.unit[c], fwd.data(), rev.data(), n + 1)) < 0 ||
                    (rc = ambi_batch_unit_prepare(b, S.unit[c], nullptr, nullptr, target.data(), nullptr)) < 0) { fclose(pf); return die(std::string("engine: ") + ambi_error_string(rc)); }
                for (int i = 1; i <= n; i++) {
                    const int id = s + i - 1;
                    char nm[256]; ambi_graph_chrom_name(S.g, id, nm, sizeof(nm));
                    fprintf(pf, "%s\t%s\t%d\t%d\t%d\t%g\t%d\t%d\t%d\t%d\n", S.lh.c_str(), nm, id, S.seg_start[id - 1], S.seg_end[id - 1], S.cn_file[id - 1],
                            target[i], fwd[i], rev[i], fwd[i] + rev[i] - target[i]);
                }
            }
        fclose(pf);
    }
    if (!junc_profile.empty()) {
        if ((rc = ambi_batch_junc_profile(b, 1, nullptr)) != 0 || (rc = ambi_batch_junc_profile_wait(b)) != 0) return die(std::string("engine: ") + ambi_error_string(rc));
        FILE* pf = fopen(junc_profile.c_str(), "w");
        if (!pf) return die("Cannot open file " + junc_profile);
        for (Sample& S : samples) {
            const int m = S.n_junc;
            std::vector<int32_t> src(m), tgt(m), count(m, 0), chr_of(m, -1);
            std::vector<int8_t> sdir(m), tdir(m);
            std::vector<double> cn(m);
            ambi_graph_junctions(S.g, src.data(), sdir.data(), tgt.data(), tdir.data(), nullptr, cn.data(), nullptr, nullptr);
            for (int c = 0; c < S.n_chr; c++) {
                const int mu = ambi_batch_unit_junc_usage(b, S.unit[c], nullptr, nullptr, INT32_MAX);
                if (mu < 0) { fclose(pf); return die(std::string("engine: ") + ambi_error_string(mu)); }
                std::vector<int32_t> cnt(mu), idx(mu);
                if ((rc = ambi_batch_unit_junc_usage(b, S.unit[c], cnt.data(), idx.data(), mu)) < 0) { fclose(pf); return die(std::string("engine: ") + ambi_error_string(rc)); }
                for (int j = 0; j < mu; j++) if (idx[j] >= 0 && idx[j] < m) { count[idx[j]] = cnt[j]; chr_of[idx[j]] = c; }
            }
            for (int j = 0; j < m; j++) {
                char ns[256], nt[256];
                ambi_graph_chrom_name(S.g, src[j], ns, sizeof(ns)); ambi_graph_chrom_name(S.g, tgt[j], nt, sizeof(nt));
                fprintf(pf, "%s\t%d\t%s\t%d\t%c\t%s\t%d\t%c\t%g\t%d\t%g\n", S.lh.c_str(), chr_of[j], ns, src[j], sdir[j] > 0 ? '+' : '-', nt, tgt[j],
                        tdir[j] > 0 ? '+' : '-', cn[j], count[j], (double)count[j] - cn[j]);
            }
        }
        fclose(pf);
    }
    if (!frag_profile.empty()) {
        if ((rc = ambi_batch_frag_profile(b, 1, nullptr)) != 0 || (rc = ambi_batch_frag_profile_wait(b)) != 0) return die(std::string("engine: ") + ambi_error_string(rc));
        FILE* pf = fopen(frag_profile.c_str(), "w");
        if (!pf) return die("Cannot open file " + frag_profile);
        for (Sample& S : samples) {
            const int nf = ambi_graph_fragments(S.g, nullptr, 0, nullptr, 0, nullptr);
            std::vector<int64_t> off((size_t)nf + 1, 0);
            std::vector<int32_t> chr_of((size_t)nf + 1, -1), fwd((size_t)nf, 0), rev((size_t)nf, 0), first((size_t)nf, -1);
            ambi_graph_fragments(S.g, nullptr, 0, off.data(), nf + 1, chr_of.data());
            for (int c = 0; c < S.n_chr; c++) {
                const int fu = ambi_batch_unit_frag_support(b, S.unit[c], nullptr, nullptr, nullptr, nullptr, INT32_MAX);
                if (fu < 0) { fclose(pf); return die(std::string("engine: ") + ambi_error_string(fu)); }
                std::vector<int32_t> uf(fu), ur(fu), ui(fu), idx(fu);
                if ((rc = ambi_batch_unit_frag_support(b, S.unit[c], uf.data(), ur.data(), ui.data(), idx.data(), fu)) < 0) { fclose(pf); return die(std::string("engine: ") + ambi_error_string(rc)); }
                for (int f = 0; f < fu; f++) if (idx[f] >= 0 && idx[f] < nf) { fwd[idx[f]] = uf[f]; rev[idx[f]] = ur[f]; first[idx[f]] = ui[f]; }
            }
            for (int f = 0; f < nf; f++)
                fprintf(pf, "%s\t%d\t%d\t%lld\t%d\t%d\t%d\n", S.lh.c_str(), chr_of[f], f, (long long)(off[f + 1] - off[f]), fwd[f], rev[f], first[f]);
        }
        fclose(pf);
    }
    if (!evidence_opt.empty()) {
        if ((rc = ambi_batch_evidence_profile(b, 1, nullptr)) != 0 || (rc = ambi_batch_evidence_profile_wait(b)) != 0) return die(std::string("engine: ") + ambi_error_string(rc));
        if (!evidence_profile.empty()) {
            FILE* pf = fopen(evidence_profile.c_str(), "w");
            if (!pf) return die("Cannot open file " + evidence_profile);
            for (Sample& S : samples) {
                const int m = S.n_junc;
                std::vector<int32_t> count(m, 0), covered(m, 0), min_depth(m, -1), chr_of(m, -1);
                for (int c = 0; c < S.n_chr; c++) {
                    const int mu = ambi_batch_unit_evidence_juncs(b, S.unit[c], nullptr, nullptr, nullptr, nullptr, INT32_MAX);
                    if (mu < 0) { fclose(pf); return die(std::string("engine: ") + ambi_error_string(mu)); }
                    std::vector<int32_t> cnt(mu), cov(mu), mind(mu), idx(mu);
                    if ((rc = ambi_batch_unit_evidence_juncs(b, S.unit[c], cnt.data(), cov.data(), mind.data(), idx.data(), mu)) < 0) { fclose(pf); return die(std::string("engine: ") + ambi_error_string(rc)); }
                    for (int j = 0; j < mu; j++) if (idx[j] >= 0 && idx[j] < m) { count[idx[j]] = cnt[j]; covered[idx[j]] = cov[j]; min_depth[idx[j]] = mind[j]; chr_of[idx[j]] = c; }
                }
                for (int j = 0; j < m; j++) fprintf(pf, "%s\t%d\t%d\t%d\t%d\t%d\n", S.lh.c_str(), chr_of[j], j, count[j], covered[j], min_depth[j]);
            }
            fclose(pf);
        }
        if (!evidence_depth.empty()) {
            FILE* pf = fopen(evidence_depth.c_str(), "w");
            if (!pf) return die("Cannot open file " + evidence_depth);
            for (Sample& S : samples)
                for (int c = 0; c < S.n_chr; c++) {
                    ambi_unit_evidence_profile_t e;
                    if ((rc = ambi_batch_unit_evidence_profile(b, S.unit[c], &e)) != 0) { fclose(pf); return die(std::string("engine: ") + ambi_error_string(rc)); }
                    std::vector<int32_t> depth((size_t)e.steps);
                    if ((rc = ambi_batch_unit_evidence_depth(b, S.unit[c], 0, e.steps, depth.data())) != 0) { fclose(pf); return die(std::string("engine: ") + ambi_error_string(rc)); }
                    for (int k = 0; k < e.steps;) {
                        int q = k + 1;
                        while (q < e.steps && depth[q] == depth[k]) q++;
                        fprintf(pf, "%s\t%d\t%d\t%d\t%d\n", S.lh.c_str(), c, k, q - k, depth[k]);
                        k = q;
                    }
                }
            fclose(pf);
        }
    }
    if (!fold_opt.empty()) {
        if ((rc = ambi_batch_fold_profile(b, 1, nullptr)) != 0 || (rc = ambi_batch_fold_profile_wait(b)) != 0) return die(std::string("engine: ") + ambi_error_string(rc));
        if (!fold_profile.empty()) {
            FILE* pf = fopen(fold_profile.c_str(), "w");
            if (!pf) return die("Cannot open file " + fold_profile);
            for (Sample& S : samples) {
                const int m = S.n_junc;
                std::vector<int32_t> folds(m, 0), max_arm(m, 0), chr_of(m, -1);
                for (int c = 0; c < S.n_chr; c++) {
                    ambi_unit_fold_profile_t e;
                    if ((rc = ambi_batch_unit_fold_profile(b, S.unit[c], &e)) != 0) { fclose(pf); return die(std::string("engine: ") + ambi_error_string(rc)); }
                    fprintf(pf, "U\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%lld\n", S.lh.c_str(), c, e.status, e.steps, e.folds, e.folds_perfect,
                            e.folds_gapped, e.folds_open, e.folds_unmatched, e.max_arm, e.max_arm_at, e.max_cover, e.max_cover_at, e.steps_covered, (long long)e.arm_sum);
                    const int mu = ambi_batch_unit_fold_juncs(b, S.unit[c], nullptr, nullptr, nullptr, INT32_MAX);
                    if (mu < 0) { fclose(pf); return die(std::string("engine: ") + ambi_error_string(mu)); }
                    std::vector<int32_t> cnt(mu), arm(mu), idx(mu);
                    if ((rc = ambi_batch_unit_fold_juncs(b, S.unit[c], cnt.data(), arm.data(), idx.data(), mu)) < 0) { fclose(pf); return die(std::string("engine: ") + ambi_error_string(rc)); }
                    for (int j = 0; j < mu; j++) if (idx[j] >= 0 && idx[j] < m) { folds[idx[j]] = cnt[j]; max_arm[idx[j]] = arm[j]; chr_of[idx[j]] = c; }
                }
                for (int j = 0; j < m; j++) fprintf(pf, "J\t%s\t%d\t%d\t%d\t%d\n", S.lh.c_str(), chr_of[j], j, folds[j], max_arm[j]);
            }
            fclose(pf);
        }
        if (!fold_arms.empty()) {
            FILE* pf = fopen(fold_arms.c_str(), "w");
            if (!pf) return die("Cannot open file " + fold_arms);
            for (Sample& S : samples)
                for (int c = 0; c < S.n_chr; c++) {
                    ambi_unit_fold_profile_t e;
                    if ((rc = ambi_batch_unit_fold_profile(b, S.unit[c], &e)) != 0) { fclose(pf); return die(std::string("engine: ") + ambi_error_string(rc)); }
                    std::vector<int32_t> fold((size_t)e.steps), cover((size_t)e.steps);
                    if ((rc = ambi_batch_unit_fold_plane(b, S.unit[c], 0, 0, e.steps, fold.data())) != 0 || (rc = ambi_batch_unit_fold_plane(b, S.unit[c], 1, 0, e.steps, cover.data())) != 0) {
                        fclose(pf); return die(std::string("engine: ") + ambi_error_string(rc));
                    }
                    for (int k = 0; k < e.steps; k++)
                        if (fold[k]) fprintf(pf, "%s\t%d\t%d\t%d\t%d\t%d\n", S.lh.c_str(), c, k, AMBI_FOLD_ALIGN(fold[k]), AMBI_FOLD_ARM(fold[k]), cover[k] - 1);
                }
            fclose(pf);
        }
    }
    if (!coords_opt.empty()) {
        Sample& S = samples[0];
        std::vector<int> chr_of_query(lift_q.size());
        for (size_t i = 0; i < lift_q.size(); i++) { chr_of_query[i] = lift_q[i].unit; lift_q[i].unit = S.unit[(size_t)chr_of_query[i]]; }
        if ((rc = ambi_batch_path_coords(b, 1, lift_q.empty() ? nullptr : lift_q.data(), (int32_t)lift_q.size(), nullptr)) != 0 || (rc = ambi_batch_path_coords_wait(b)) != 0)
            return die(std::string("engine: ") + ambi_error_string(rc));
        if (!path_coords.empty()) {
            FILE* pf = fopen(path_coords.c_str(), "w");
            if (!pf) return die("Cannot open file " + path_coords);
            for (int c = 0; c < S.n_chr; c++) {
                ambi_unit_coords_t e;
                if ((rc = ambi_batch_path_coords_summary(b, S.unit[c], &e)) != 0) { fclose(pf); return die(std::string("engine: ") + ambi_error_string(rc)); }
                fprintf(pf, "%d\t%d\t%d\t%lld\t%lld\n", e.cells, e.runs, e.empty_cells, (long long)e.bp_len, (long long)e.bp_minus);
            }
            fclose(pf);
        }
        if (!lift_out.empty()) {
            FILE* pf = fopen(lift_out.c_str(), "w");
            if (!pf) return die("Cannot open file " + lift_out);
            for (size_t i = 0; i < lift_q.size(); i++) {
                ambi_lift_t r;
                if ((rc = ambi_batch_path_coords_result(b, (int32_t)i, &r)) != 0) { fclose(pf); return die(std::string("engine: ") + ambi_error_string(rc)); }
                if (r.cell < 0) { fprintf(pf, "%lld\t-1\t0\t.\t.\t-1\n", (long long)lift_q[i].pos); continue; }
                int32_t s, e;
                ambi_graph_chromosome(S.g, chr_of_query[i], &s, &e);
                const int id = s - 1 + (r.seg < 0 ? -r.seg : r.seg);
                char nm[256]; ambi_graph_chrom_name(S.g, id, nm, sizeof(nm));
                fprintf(pf, "%lld\t%d\t%d\t%c\t%s\t%lld\n", (long long)lift_q[i].pos, r.cell, id, r.seg > 0 ? '+' : '-', nm, (long long)S.seg_start[id - 1] + (long long)r.seg_off);
            }
            fclose(pf);
        }
    }
    if (!path_compare.empty()) {
        // pairs in row order: per chromosome `P` (path against path_indel), then `T` (final path against the truth line) if it has one
        struct Row { char tag; size_t si; int c; };
        std::vector<Row> rows;
        std::vector<int32_t> pairs, given;
        std::vector<int64_t> given_off(1, 0);
        for (size_t si = 0; si < samples.size(); si++) {
            Sample& S = samples[si];
            for (int c = 0; c < S.n_chr; c++) {
                pairs.push_back(AMBI_COMPARE_UNIT(S.unit[c], 0)); pairs.push_back(AMBI_COMPARE_UNIT(S.unit[c], 1));
                rows.push_back(Row{'P', si, c});
                if (truth.empty() || truth_cells[(size_t)c].empty()) continue;   // (--truth: one sample; `.`: no truth for the chromosome)
                given.insert(given.end(), truth_cells[(size_t)c].begin(), truth_cells[(size_t)c].end());
                given_off.push_back((int64_t)given.size());
                pairs.push_back(AMBI_COMPARE_UNIT(S.unit[c], 1)); pairs.push_back(AMBI_COMPARE_GIVEN((int32_t)given_off.size() - 2));
                rows.push_back(Row{'T', si, c});
            }
        }
        if ((rc = ambi_batch_set_compare_paths(b, given.data(), given_off.data(), (int32_t)given_off.size() - 1)) != 0 ||
            (rc = ambi_batch_path_compare(b, pairs.data(), (int32_t)rows.size(), compare_dmax, nullptr)) != 0 || (rc = ambi_batch_path_compare_wait(b)) != 0)
            return die(std::string("engine: ") + ambi_error_string(rc));
        FILE* pf = fopen(path_compare.c_str(), "w");
        if (!pf) return die("Cannot open file " + path_compare);
        for (size_t i = 0; i < rows.size(); i++) {
            ambi_path_compare_t r;
            if ((rc = ambi_batch_path_compare_result(b, (int32_t)i, &r)) != 0) { fclose(pf); return die(std::string("engine: ") + ambi_error_string(rc)); }
            fprintf(pf, "%c\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", rows[i].tag, samples[rows[i].si].lh.c_str(), rows[i].c, r.status, r.len_a, r.len_b, r.dmax,
                    r.prefix[0], r.prefix[1], r.suffix[0], r.suffix[1], r.dist[0], r.dist[1], r.lcs[0], r.lcs[1]);
        }
        fclose(pf);
        if (!path_align.empty()) {
            // every row in the orientation with the smaller dist (ties as is), one request; a row with both dist -1 is not aligned
            std::vector<int32_t> triples;
            std::vector<int> entry(rows.size(), -1);   // row -> entry of the request
            for (size_t i = 0; i < rows.size(); i++) {
                ambi_path_compare_t r;
                if ((rc = ambi_batch_path_compare_result(b, (int32_t)i, &r)) != 0) return die(std::string("engine: ") + ambi_error_string(rc));
                if (r.dist[0] < 0 && r.dist[1] < 0) continue;
                entry[i] = (int)(triples.size() / 3);
                triples.insert(triples.end(), {pairs[2 * i], pairs[2 * i + 1], r.dist[0] < 0 || (r.dist[1] >= 0 && r.dist[1] < r.dist[0]) ? 1 : 0});
            }
            if ((rc = ambi_batch_path_align(b, triples.data(), (int32_t)(triples.size() / 3), compare_dmax, nullptr)) != 0 || (rc = ambi_batch_path_align_wait(b)) != 0)
                return die(std::string("engine: ") + ambi_error_string(rc));
            FILE* af = fopen(path_align.c_str(), "w");
            if (!af) return die("Cannot open file " + path_align);
            auto fail = [&](int code) { fclose(af); return die(std::string("engine: ") + ambi_error_string(code)); };
            for (size_t i = 0; i < rows.size(); i++) {
                const Row& W = rows[i];
                Sample& S = samples[W.si];
                if (entry[i] < 0) { fprintf(af, "A\t%c\t%d\t-1\t-1\t0\n", W.tag, W.c); continue; }
                ambi_path_align_t h;
                if ((rc = ambi_batch_path_align_result(b, entry[i], &h)) != 0) return fail(rc);
                fprintf(af, "A\t%c\t%d\t%d\t%d\t%d\n", W.tag, W.c, h.orient, h.dist, h.n_runs);
                if (h.n_runs == 0) continue;
                std::vector<ambi_align_run_t> runs((size_t)h.n_runs);
                int32_t nr = 0;
                if ((rc = ambi_batch_path_align_runs(b, entry[i], runs.data(), h.n_runs, &nr)) != 0) return fail(rc);
                // the two sides in global ids: a, and Bo (b, or its reverse complement)
                int32_t s0, e0;
                ambi_graph_chromosome(S.g, W.c, &s0, &e0);
                ambi_unit_result_t ur; ambi_batch_unit_result(b, S.unit[W.c], &ur);
                std::vector<int32_t> pa((size_t)(W.tag == 'P' ? ur.path_len : ur.path_indel_len)), pb;
                ambi_batch_unit_path(b, S.unit[W.c], W.tag == 'P' ? 0 : 1, pa.data(), (int32_t)pa.size());
                if (W.tag == 'P') { pb.resize((size_t)ur.path_indel_len); ambi_batch_unit_path(b, S.unit[W.c], 1, pb.data(), (int32_t)pb.size()); }
                else for (int32_t v : truth_cells[(size_t)W.c]) pb.push_back(v > 0 ? v + s0 - 1 : v - s0 + 1);
                if (h.orient) { std::reverse(pb.begin(), pb.end()); for (int32_t& v : pb) v = -v; }
                for (const ambi_align_run_t& q : runs) {
                    const std::vector<int32_t>& from = q.kind ? pb : pa;
                    const int32_t at = q.kind ? q.b_pos : q.a_pos;
                    if (at < 0 || q.len < 1 || (size_t)at + (size_t)q.len > from.size()) return fail(AMBI_ERR_STATE);
                    fprintf(af, "%c\t%d\t%d\t%d\t%s\n", q.kind ? 'I' : 'D', q.a_pos, q.b_pos, q.len, path_text(S.g, std::vector<int32_t>(from.begin() + at, from.begin() + at + q.len)).c_str());
                }
            }
            fclose(af);
        }
    }
    if (!out_fasta.empty()) {
        FILE* ff = fopen(out_fasta.c_str(), "w");
        if (!ff) return die("Cannot open file " + out_fasta);
        auto fail = [&](int code) { fclose(ff); return die(std::string("engine: ") + ambi_error_string(code)); };
        std::vector<std::string> name((size_t)n_units);   // unit -> record name
        for (Sample& S : samples)
            for (int c = 0; c < S.n_chr; c++) {
                int32_t s, e;
                ambi_graph_chromosome(S.g, c, &s, &e);
                char nm[256]; ambi_graph_chrom_name(S.g, s, nm, sizeof(nm));
                name[(size_t)S.unit[c]] = S.n_chr == 1 ? "BFBPATH" : std::string("BFBPATH_") + nm;
            }
        std::vector<uint8_t> buf((size_t)(1 << 22));
        // one request for everything; if that exceeds the budget it assembles nothing and leaves EVERY unit's length readable: the
        // chunks are planned from them once, each the longest range that fits (a single unit beyond the budget goes alone)
        std::vector<int64_t> ulen;
        rc = ambi_batch_sequence(b, 1, 0, n_units, fasta_chunk, nullptr);
        const bool whole = rc == 0;
        if (rc == AMBI_ERR_TOO_LARGE) {
            ulen.resize((size_t)n_units);
            for (int u = 0; u < n_units; u++) if ((rc = ambi_batch_unit_sequence_len(b, u, &ulen[(size_t)u])) != 0) return fail(rc);
        } else if (rc != 0) return fail(rc);
        for (int first = 0; first < n_units;) {
            int count = n_units - first;
            if (!whole) {
                int64_t sum = 0; int fit = 0;
                for (; fit < count; fit++) {
                    if (fit > 0 && sum + ulen[(size_t)(first + fit)] > fasta_chunk) break;
                    sum += ulen[(size_t)(first + fit)];
                }
                count = fit;
                rc = ambi_batch_sequence(b, 1, first, count, 0, nullptr);
            }
            if (rc != 0 || (rc = ambi_batch_sequence_wait(b)) != 0) return fail(rc);
            for (int u = first; u < first + count; u++) {
                ambi_unit_result_t r; ambi_batch_unit_result(b, u, &r);
                int64_t len = 0;
                if ((rc = ambi_batch_unit_sequence_len(b, u, &len)) != 0) return fail(rc);
                if (r.status < 0 || r.path_indel_len <= 0) continue;   // no path: no record
                fprintf(ff, ">%s\n", name[(size_t)u].c_str());
                for (int64_t at = 0; at < len; at += (int64_t)buf.size()) {
                    const int64_t k = len - at < (int64_t)buf.size() ? len - at : (int64_t)buf.size();
                    if ((rc = ambi_batch_unit_sequence(b, u, at, k, buf.data())) != 0) return fail(rc);
                    fwrite(buf.data(), 1, (size_t)k, ff);
                }
                fputc('\n', ff);
            }
            first += count;
        }
        fclose(ff);
    }
    int refused_total = 0;
    for (Sample& S : samples) {
        ambi_graph_t* g = S.g;
        std::vector<std::vector<int32_t>> paths(S.n_chr);
        std::vector<OutJ> out_acc;
        int refused = 0;
        for (int c = 0; c < S.n_chr; c++) {
            const int u = S.unit[c];
            std::cout << S.head[c];
            ambi_unit_result_t r; ambi_batch_unit_result(b, u, &r);
            if (r.status < 0 || r.status == AMBI_ST_NO_VALID_ORDER) {
                // where the reference would print this chromosome's path.  AMBI_ERR_REF_UB: the reference itself reads past the
                // end of its breakpoint vector on this input (LGM.cpp:3436-3442) -- whatever it prints there is not defined by
                // its source, so nothing is printed here; the other chromosomes follow, the exit status is 1.
                std::cout.flush();
                std::cerr << "bfb: chromosome " << c << ": " << ambi_error_string(r.status) << std::endl;
                refused++;
                continue;
            }
            std::vector<int32_t> p(r.path_len), q(r.path_indel_len);
            ambi_batch_unit_path(b, u, 0, p.data(), r.path_len);
            ambi_batch_unit_path(b, u, 1, q.data(), r.path_indel_len);
            if (all && r.status == AMBI_ST_OK) {
                // --all: one line per valid order; the flipped orientation only if the last order was invalid (LGM.cpp:3672-3695)
                const int64_t stride = 2ll * r.path_len + 64;
                for (int pass = 0; pass < 2; pass++) {
                    int64_t nv = 0;
                    ambi_batch_all_count(b, u, pass, &nv);
                    for (int64_t lo = 0; lo < nv; lo += 64) {
                        const int64_t cnt = nv - lo < 64 ? nv - lo : 64;
                        std::vector<int32_t> len((size_t)cnt), cells((size_t)(cnt * stride));
                        if ((rc = ambi_batch_all_paths(b, u, pass, lo, cnt, len.data(), cells.data(), stride)) != 0)
                            return die(std::string("bfb --all: ") + ambi_error_string(rc));
                        for (int64_t j = 0; j < cnt; j++) {
                            if (len[j] < 0) return die(std::string("bfb --all: ") + ambi_error_string(len[j]));
                            std::vector<int32_t> pj(cells.begin() + j * stride, cells.begin() + j * stride + len[j]);
                            std::cout << path_text(g, pj) << std::endl;
                        }
                    }
                }
            } else
                std::cout << path_text(g, p) << std::endl;                               // printBFB (LGM.cpp:3411-3429)
            if (r.status == AMBI_ST_INFEASIBLE) std::cout << "ILP is unsolvable.\n";    // localhap.cpp:217
            else if (r.indel_printed) std::cout << "BFB path with insertion, deletion, or duplication:\n" << path_text(g, q) << std::endl;
            if (S.trx_before && r.status == AMBI_ST_OK) {
                // virusBFB (localhap.cpp:263): the path goes back to the segments of the file; its junction steps are counted there
                std::vector<int32_t> back(q);
                back.resize(q.size() + 8);
                std::string text(64 + 16 * (q.size() + 8) * 2, '\0');
                int64_t tl = 0;
                const int nl = ambi_graph_trx_restore(g, back.data(), (int32_t)q.size(), (int32_t)back.size(), &text[0], (int64_t)text.size(), &tl);
                if (nl < 0) { std::cout.flush(); std::cerr << "bfb: chromosome " << c << ": " << ambi_error_string(nl) << std::endl; refused++; continue; }
                back.resize(nl);
                text.resize((size_t)std::min<int64_t>(tl, (int64_t)text.size() - 1));
                std::cout << text;
                paths[c] = back;
                for (int i = 0; i + 1 < nl; i++) {
                    const int uu = back[i], vv = back[i + 1];
                    if (!(std::abs(std::abs(uu) - std::abs(vv)) == 1 && (uu > 0) == (vv > 0))) merge_steps(out_acc, uu, vv, 1, true);   // localhap.cpp:267-289
                }
                continue;
            }
            paths[c] = q;
            std::vector<int32_t> ju(r.n_out_junc), jv(r.n_out_junc), jc(r.n_out_junc);
            ambi_batch_unit_out_juncs(b, u, ju.data(), jv.data(), jc.data(), r.n_out_junc);
            for (int k = 0; k < r.n_out_junc; k++) merge_steps(out_acc, ju[k], jv[k], jc[k], true);   // localhap.cpp:267-289
        }
        if (refused) { refused_total += refused; continue; }     // (this sample has no translocation stage and leaves no side-file rows)
        int path_len = 0, cn_sum = 0, max_cn_i = 0;
        for (auto& p : paths) path_len += (int)p.size();
        for (double v : S.cn_all) { cn_sum += v; max_cn_i = (max_cn_i > v) ? max_cn_i : v; }   // localhap.cpp:290-293 (int fed with doubles)
        if (S.ins_mode == 2 || S.con_mode == 2) {   // localhap.cpp:295-316
            if (!S.main_chr[0]) return die("BFB-TRX needs PROP M:<chr>");
            std::cout << "BFB with translocation:\n";
            std::vector<int64_t> offs(S.n_chr + 1, 0);
            for (int c = 0; c < S.n_chr; c++) offs[c + 1] = offs[c] + (int64_t)paths[c].size();
            std::vector<int32_t> flat((size_t)offs[S.n_chr] + 1), out((size_t)offs[S.n_chr] * 2 + 16);
            for (int c = 0; c < S.n_chr; c++) std::copy(paths[c].begin(), paths[c].end(), flat.begin() + offs[c]);
            int len = ambi_translocation_bfb(g, flat.data(), offs.data(), S.n_chr, out.data(), (int32_t)out.size());
            if (len < 0) return die(ambi_error_string(len));
            out.resize(len);
            std::cout << path_text(g, out) << std::endl;
            for (int i = 0; i + 1 < len; i++) {
                int u = out[i], v = out[i + 1];
                if (!(std::abs(std::abs(u) - std::abs(v)) == 1 && (u > 0) == (v > 0))) merge_steps(out_acc, u, v, 1, false);
            }
        }
        // side files (localhap.cpp:326-337, 382-388)
        {
            int32_t n_seg = S.n_seg, n_junc = S.n_junc, n_chr = S.n_chr;
            ambi_graph_sizes(g, &n_seg, &n_junc, &n_chr);
            std::vector<int32_t> js(n_junc), jt(n_junc); std::vector<int8_t> jsd(n_junc), jtd(n_junc); std::vector<double> jcn(n_junc);
            ambi_graph_junctions(g, js.data(), jsd.data(), jt.data(), jtd.data(), nullptr, jcn.data(), nullptr, nullptr);
            auto chrom = [&](int id) { char nm[256]; ambi_graph_chrom_name(g, id, nm, sizeof(nm)); return std::string(nm); };
            auto vend = [&](int id, int dir) { return dir > 0 ? S.seg_end[id - 1] : S.seg_start[id - 1]; };      // Vertex::getEnd
            auto vstart = [&](int id, int dir) { return dir > 0 ? S.seg_start[id - 1] : S.seg_end[id - 1]; };    // Vertex::getStart
            std::ofstream sv("simulation_sv.txt", std::ios_base::app);
            for (int j = 0; j < n_junc; j++)
                sv << S.lh << "\t" << juncs << "\t" << chrom(js[j]) << "\t" << vend(js[j], jsd[j]) << "\t" << (jsd[j] > 0 ? '+' : '-') << "\t"
                   << chrom(jt[j]) << "\t" << vstart(jt[j], jtd[j]) << "\t" << (jtd[j] > 0 ? '+' : '-') << "\t" << jcn[j] << "\tinput\n";
            // (PROP I1 / C1: the vertices of the restored paths are segments of the FILE)
            std::vector<int32_t> fs, fe;
            if (S.trx_before) {
                int32_t fn = 0, fj = 0, fc = 0;
                ambi_graph_sizes(S.g_file, &fn, &fj, &fc);
                fs.resize(fn); fe.resize(fn);
                ambi_graph_segments(S.g_file, nullptr, nullptr, fs.data(), fe.data(), nullptr, nullptr);
            }
            auto ochrom = [&](int id) { if (!S.trx_before) return chrom(id); char nm[256]; ambi_graph_chrom_name(S.g_file, id, nm, sizeof(nm)); return std::string(nm); };
            auto ovend = [&](int id, int dir) { return !S.trx_before ? vend(id, dir) : (dir > 0 ? fe[id - 1] : fs[id - 1]); };
            auto ovstart = [&](int id, int dir) { return !S.trx_before ? vstart(id, dir) : (dir > 0 ? fs[id - 1] : fe[id - 1]); };
            for (auto& j : out_acc) {
                int a = std::abs(j.u), bb = std::abs(j.v), ad = j.u > 0 ? 1 : -1, bd = j.v > 0 ? 1 : -1;
                sv << S.lh << "\t" << juncs << "\t" << ochrom(a) << "\t" << ovend(a, ad) << "\t" << (ad > 0 ? '+' : '-') << "\t"
                   << ochrom(bb) << "\t" << ovstart(bb, bd) << "\t" << (bd > 0 ? '+' : '-') << "\t" << j.cn << "\toutput\n";
            }
            auto t_end = std::chrono::steady_clock::now();
            std::ofstream tf("time.csv", std::ios_base::app);
            tf << S.lh.substr(0, S.lh.find(".")) << "," << n_seg << "," << S.num_inv << "," << n_junc - S.num_inv << "," << cn_sum << "," << path_len << ","
               << max_cn_i << "," << std::chrono::duration_cast<std::chrono::microseconds>(t_end - S.t_begin).count() / 1000000.0 << "\n";
        }
    }
    ambi_batch_destroy(b);
    for (Sample& S : samples) { ambi_graph_destroy(S.g); if (S.g_file) ambi_graph_destroy(S.g_file); }
    if (refused_total) return die("bfb: " + std::to_string(refused_total) + " chromosome(s) without a path");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    setenv("GPU_MAX_HW_QUEUES", "8", 0);   // the engine's four streams on hardware queues of their own (before the HIP runtime starts)
    Args A = parse(argc, argv);
    if (A.help) {
        std::cout << "Local Haplotype constructer\nUsage:\n  Ambigram --op bfb|sc_bfb --in_lh <file[,file...]> --lp_prefix <name> [--juncdb <file> --junc_info true] "
                     "[--reversed true] [--all true] [--solver_timeout <seconds>] [--devices N|all|<ordinal,ordinal,...>] [--cn_profile <file>] "
                     "[--junc_profile <file>] [--frag_profile <file> [--frags <file>]] [--evidence_profile <file>] [--evidence_depth <file>] [--fold_profile <file>] [--fold_arms <file>] "
                     "[--path_compare <file> [--truth <file>] [--compare_dmax N] [--path_align <file>]] [--path_coords <file>] [--lift <queries> --lift_out <file>] "
                     "[--ref_fasta <file> --out_fasta <file>]\n"
                     "  --op bfb: --in_lh may list several samples; their chromosomes are reconstructed as one batch, over the devices named by --devices\n"
                     "  --cn_profile <file> (--op bfb): one tab-separated row per segment after the run: sample, chromosome, segment id, start, end, input CN, "
                     "target CN, forward count, reverse count, count - target (PROP I1 / C1 / I2 / C2 samples are refused, exit status 2)\n"
                     "  --junc_profile <file> (--op bfb): one tab-separated row per junction after the run, in file order: sample, chromosome index (-1 between "
                     "chromosomes), source chromosome, source segment id, source strand, target chromosome, target segment id, target strand, input CN, count in "
                     "the final path, count - CN (PROP I1 / C1 / I2 / C2 samples are refused, exit status 2)\n"
                     "  --frag_profile <file> (--op bfb): one tab-separated row per fragment (line of the fragment file read as one signed chain) after the run, "
                     "in file order: sample, chromosome index (-1: no unit), fragment index, cells, occurrences in the final path, occurrences of the reverse "
                     "complement, first position or -1 (PROP I1 / C1 / I2 / C2 samples are refused, exit status 2)\n"
                     "  --frags <file>: the fragment file of --frag_profile, --evidence_profile and --evidence_depth (default: the file of --juncdb)\n"
                     "  --evidence_profile <file> (--op bfb): one tab-separated row per junction after the run, in file order: sample, chromosome index (-1 between "
                     "chromosomes), junction index, count in the final path, those of them under at least one fragment occurrence, smallest fragment depth "
                     "over them or -1 (PROP I1 / C1 / I2 / C2 samples are refused, exit status 2)\n"
                     "  --evidence_depth <file> (--op bfb): the number of fragment occurrences over every step of the final paths in run-length form: sample, "
                     "chromosome index, first step, steps, depth (PROP I1 / C1 / I2 / C2 samples are refused, exit status 2)\n"
                     "  --fold_profile <file> (--op bfb): the fold-back structure of the final paths after the run: one tab-separated U row per chromosome "
                     "(U, sample, chromosome index, status, steps, folds, perfect, gapped, open, folds of no junction, longest arm, its step, largest cover, its "
                     "step, covered steps, sum of arms) and one J row per junction in file order (J, sample, chromosome index or -1, junction index, folds, "
                     "longest arm) (PROP I1 / C1 / I2 / C2 samples are refused, exit status 2)\n"
                     "  --fold_arms <file> (--op bfb): one tab-separated row per fold of the final paths: sample, chromosome index, step, alignment (-1 no arm, "
                     "0 perfect, 1..4 one or two unpaired cells), arm in cells, nesting (PROP I1 / C1 / I2 / C2 samples are refused, exit status 2)\n"
                     "  --path_compare <file> [--truth <file>] [--compare_dmax N] (--op bfb): one tab-separated P row per chromosome after the run, the path "
                     "before indelBFB against the path after it: P, sample, chromosome index, status, len_a, len_b, dmax, then prefix, suffix, dist, lcs for the "
                     "orientation as is and for the reverse complement (dist: insertions plus deletions, -1 above N; N 0..1024, default 64); with --truth a T row "
                     "per chromosome, the final path against that chromosome's line of the truth file (a printed path with global ids, or `.`; one sample only) "
                     "(PROP I1 / C1 / I2 / C2 samples and --devices are refused, exit status 2)\n"
                     "  --path_coords <file> (--op bfb): one tab-separated row per chromosome after the run: cells, runs, cells of length 0, the amplicon's length "
                     "in base pairs, base pairs on the '-' strand, from the device's path coordinates of the final paths\n"
                     "  --lift <queries> --lift_out <file> (--op bfb): per line `<chromosome index> <pos>` of the query file one tab-separated row: pos, cell, segment id, "
                     "strand, chromosome name, genomic position (0-based) of position pos of the chromosome's amplicon (its record of --out_fasta); "
                     "`-1 0 . . -1` for a position outside it (one sample; PROP I1 / C1 / I2 / C2 samples and --devices are refused, exit status 2)\n"
                     "  --path_align <file> (with --path_compare): where the two paths of every P and T row differ, aligned on the device in the orientation with "
                     "the smaller dist (ties as is) at the cap of --compare_dmax: per row a header line A, tag, chromosome index, orient, dist, n_runs, then one "
                     "line per maximal run of insertions or deletions: D or I, a_pos, b_pos, len and the run's cells as a printed path (a row with both dist -1: "
                     "the header alone, orient -1, dist -1, 0 runs)\n"
                     "  --ref_fasta <file> --out_fasta <file> (--op bfb): the nucleotide sequence of every chromosome's final path, one record per chromosome "
                     "(>BFBPATH, or >BFBPATH_<chromosome> when the sample has several), from the segments' bases chrom[start..end) of the reference FASTA "
                     "(0-based, half-open); PROP I1 / C1 / I2 / C2 samples are refused, exit status 2; --fasta_chunk_bytes <n>: bytes assembled per request\n";
        return 0;
    }
    const std::string op = A.kv.count("op") ? A.kv["op"] : "";
    std::cout << op << std::endl;   // localhap.cpp:47
    if (op == "sc_bfb" && (A.kv.count("out_fasta") || A.kv.count("ref_fasta"))) {
        std::cerr << "--ref_fasta / --out_fasta: --op bfb only" << std::endl;
        return 2;
    }
    if (op == "sc_bfb") return run_sc_bfb(A);
    if (op != "bfb") return 0;   // the reference does nothing for any other op (localhap.cpp:49, :390)
    return run_bfb(A);
}
