// tests/tools/path_profile_stage_check.cpp -- stand-alone check of the copy-number profile stage and of the chunked cell read the
// three profile stages share (ambi_profile.hpp) on the CPU with the one-thread HostGroup, for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wno-unknown-pragmas
//       -I ambigram_amd/csrc tests/tools/path_profile_stage_check.cpp -o path_profile_stage_check && ./path_profile_stage_check
// Paths of every shape below go through stage_path_profile; what it leaves is compared with a plain transcription written here: the
// path walked cell by cell, every segment counted per strand, the summary computed from those counts.  path_load_chunk is checked
// on its own, chunk by chunk, against the same cells.  A HostGroup has one thread, so a tile is kProfileChunk = 8 cells.
// Every buffer has exactly its stated size, so a read or write past one is the sanitizer's to report: the cells end at the next
// multiple of four when they are 8-byte aligned (the two-load path) and exactly at P when they start 1, 2 or 3 cells behind an
// 8-byte boundary (the cell-by-cell path); the difference arrays are 2 * window ints; the counts n + 1 ints each.
// Covered on purpose: P = 1 .. 17 around the tile and half-tile edges and random P up to 300; n = 1, 2 and random up to 40;
// windows of 1, 2, n - 1, n and n + 1; a single run, single-cell runs only, -n .. -1, a last cell that ends a run at segment n
// (its event at index n + 1 is dropped), fold-back turns c, -c.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ambi_profile.hpp"

using namespace ambi;

static int fails = 0, g_case = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s (case %d)\n", __FILE__, __LINE__, #x, g_case); fails++; } } while (0)
static int n_turn_units = 0, n_multi_window = 0, n_scalar = 0, n_end_at_n = 0, n_begin_at_minus_n = 0, n_chunks = 0, n_partial_chunks = 0;   // what the cases reached

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 11); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }   // inclusive

// ---- the transcription -----------------------------------------------------------------------------------------------------
static void ref_profile(const std::vector<int>& path, int n, const std::vector<int32_t>& target, const std::vector<double>& seg_cn,
                        std::vector<int32_t>& fwd, std::vector<int32_t>& rev, UnitProfile& s) {
    fwd.assign((size_t)n + 1, 0); rev.assign((size_t)n + 1, 0);
    memset(&s, 0, sizeof(s));
    s.cells = (int)path.size();
    for (size_t i = 0; i < path.size(); i++) {
        const int c = path[i];
        if (c > 0) fwd[(size_t)c]++; else rev[(size_t)-c]++;
        if (i == 0 || c != path[i - 1] + 1) s.runs++;
        if (i > 0 && c == -path[i - 1]) s.turns++;
    }
    for (int i = 1; i <= n; i++) {
        const int t = fwd[(size_t)i] + rev[(size_t)i];
        s.max_cn = std::max(s.max_cn, t);
        s.n_uncovered += t == 0;
        s.n_off_target += t != target[(size_t)i];
        s.l1_target += std::abs((int64_t)t - target[(size_t)i]);
        const double d = (double)t - seg_cn[(size_t)i];
        s.n_off_input += (d < 0 ? -d : d) >= 0.5;
    }
}

// the cells of a path `off` cells behind an 8-byte boundary: readable up to the next multiple of four (off = 0) or exactly P long
struct Cells {
    std::vector<rcell_t> store;
    const rcell_t* p;
    Cells(const std::vector<int>& path, int off) {
        const size_t P = path.size();
        store.assign(off == 0 ? ((P + 3) & ~(size_t)3) : P + (size_t)off, (rcell_t)0x5a5a);
        CHECK((reinterpret_cast<uintptr_t>(store.data()) & 7) == 0);
        for (size_t i = 0; i < P; i++) store[(size_t)off + i] = (rcell_t)path[i];
        p = store.data() + off;
    }
};

// ---- the chunk reader, chunk by chunk ----------------------------------------------------------------------------------------
static void check_chunks(const std::vector<int>& path, int off) {
    const Cells C(path, off);
    const int P = (int)path.size();
    const bool vec = (reinterpret_cast<uintptr_t>(C.p) & 7) == 0;
    CHECK(vec == (off == 0));
    for (int s = 0; s < P; s += kProfileChunk) {
        rcell_t c[kProfileChunk];
        for (int k = 0; k < kProfileChunk; k++) c[k] = (rcell_t)0x7777;
        int prev = 0x7777;
        const int e = path_load_chunk(C.p, P, vec, s, c, prev);
        CHECK(e == std::min(kProfileChunk, P - s));
        CHECK(prev == (s > 0 ? path[(size_t)s - 1] : 0));
        for (int k = 0; k < kProfileChunk; k++) {
            if (s + k < P) CHECK((int)c[k] == path[(size_t)(s + k)]);
            else if (!vec || ((s + k) & ~3) >= P) CHECK(c[k] == 0);   // zero behind P, but for the padding of the 8-byte word that holds cell P - 1
        }
        n_chunks++; n_partial_chunks += e < kProfileChunk;
    }
}

// ---- one case of the stage -------------------------------------------------------------------------------------------------
static void run_case(const std::vector<int>& path, int n, int window, int off) {
    const int P = (int)path.size();
    const Cells C(path, off);
    std::vector<int32_t> target((size_t)n + 1, 0), bins((size_t)(2 * window), -1), got_f((size_t)n + 1, -7), got_r((size_t)n + 1, -7), want_f, want_r;
    std::vector<double> seg_cn((size_t)n + 1, 0.0);
    for (int i = 1; i <= n; i++) { target[(size_t)i] = rnd_in(0, 6); seg_cn[(size_t)i] = rnd_in(0, 12) * 0.5; }
    CHECK((int64_t)bins.size() * 4 == profile_bins_bytes(window));
    UnitProfile gs, ws;
    memset(&gs, 0x5a, sizeof(gs));
    HostGroup g;
    stage_path_profile(g, C.p, P, n, target.data(), seg_cn.data(), window, bins.data(), got_f.data(), got_r.data(), &gs);
    ref_profile(path, n, target, seg_cn, want_f, want_r, ws);
    gs.status = 0;   // (the stage writes every field but this one)
    CHECK(got_f == want_f);
    CHECK(got_r == want_r);
    CHECK(memcmp(&gs, &ws, sizeof(gs)) == 0);
    if (fails && fails < 4) printf("  P %d n %d window %d off %d: runs %d/%d turns %d/%d max %d/%d unc %d/%d off_t %d/%d off_in %d/%d l1 %lld/%lld\n", P, n, window, off, gs.runs,
                                   ws.runs, gs.turns, ws.turns, gs.max_cn, ws.max_cn, gs.n_uncovered, ws.n_uncovered, gs.n_off_target, ws.n_off_target, gs.n_off_input,
                                   ws.n_off_input, (long long)gs.l1_target, (long long)ws.l1_target);
    n_turn_units += ws.turns > 0; n_multi_window += window < n; n_scalar += off != 0;
    n_end_at_n += path.back() == n;
    bool minus_n = false;
    for (size_t i = 0; i < path.size(); i++) minus_n = minus_n || (path[i] == -n && (i == 0 || path[i] != path[i - 1] + 1));
    n_begin_at_minus_n += minus_n;
}

// ---- the paths -------------------------------------------------------------------------------------------------------------
enum Kind { kRandomRuns, kSingleCells, kSingleRun, kMinusAll, kEndsAtN, kFoldBacks, kKinds };
static void push_run(std::vector<int>& p, int a, int b, bool plus) {   // the segments a..b on a strand
    if (plus) for (int v = a; v <= b; v++) p.push_back(v);
    else for (int v = b; v >= a; v--) p.push_back(-v);
}
// a path of P cells over the segments 1..n, or of the length its kind dictates (a single run has at most n cells, -n .. -1 has n)
static std::vector<int> make_path(Kind kind, int n, int P) {
    std::vector<int> p;
    if (kind == kSingleRun) { const int L = std::min(P, n), a = rnd_in(1, n - L + 1); push_run(p, a, a + L - 1, (rnd() & 1) != 0); return p; }
    if (kind == kMinusAll) { push_run(p, 1, n, false); return p; }
    if (kind == kSingleCells) {
        while ((int)p.size() < P) { const int c = rnd() & 1 ? rnd_in(1, n) : -rnd_in(1, n); if (p.empty() || c != p.back() + 1) p.push_back(c); }
        return p;
    }
    if (kind == kFoldBacks) {   // up a..b, the turn b, -b, down to another a, the turn -a, a, up again
        int a = rnd_in(1, n);
        while ((int)p.size() < P) {
            const int b = rnd_in(a, n);
            push_run(p, a, b, true);
            a = rnd_in(1, b);
            push_run(p, a, b, false);
        }
        p.resize((size_t)P);
        return p;
    }
    const int tail = kind == kEndsAtN ? std::min(P, rnd_in(1, n)) : 0;   // the last run: n - tail + 1 .. n on the '+' strand
    while ((int)p.size() < P - tail) { const int a = rnd_in(1, n), b = rnd_in(a, std::min(n, a + rnd_in(0, 12))); push_run(p, a, b, (rnd() & 1) != 0); }
    p.resize((size_t)(P - tail));
    if (tail) push_run(p, n - tail + 1, n, true);
    return p;
}

static void run_shapes(Kind kind, int n, int P) {
    const int wins[5] = {1, 2, n - 1, n, n + 1};
    for (int off = 0; off < 4; off++) {
        const std::vector<int> path = make_path(kind, n, P);
        check_chunks(path, off);
        for (int w = 0; w < 5; w++) {
            if (wins[w] < 1 || std::find(wins, wins + w, wins[w]) != wins + w) continue;
            run_case(path, n, wins[w], off);
            g_case++;
        }
    }
}

int main() {
    static const int fixed_P[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17};
    // every tile-edge length with every n choice and every kind of path
    for (int P : fixed_P)
        for (int nc = 0; nc < 3; nc++)
            for (int kind = 0; kind < kKinds; kind++) run_shapes((Kind)kind, nc == 0 ? 1 : nc == 1 ? 2 : rnd_in(3, 40), P);
    // random lengths
    for (int i = 0; i < 300; i++) run_shapes((Kind)(i % kKinds), i % 17 == 0 ? 1 : i % 19 == 0 ? 2 : rnd_in(3, 40), rnd_in(1, 300));
    printf("cases %d: with fold-back turns %d, in several windows %d, cell by cell %d, last cell at n %d, a run from -n %d; chunks %d, partial %d\n", g_case,
           n_turn_units, n_multi_window, n_scalar, n_end_at_n, n_begin_at_minus_n, n_chunks, n_partial_chunks);
    if (g_case < 5000 || n_turn_units < 500 || n_multi_window < 2000 || n_scalar < 3000 || n_end_at_n < 500 || n_begin_at_minus_n < 500 || n_chunks < 10000 ||
        n_partial_chunks < 1000) { printf("FAIL: a class of cases was not reached\n"); fails++; }
    if (fails) { printf("path_profile_stage_check: %d FAILURES\n", fails); return 1; }
    printf("path_profile_stage_check: ok\n");
    return 0;
}
