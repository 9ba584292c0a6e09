// tests/tools/path_compare_stage_check.cpp -- stand-alone check of the path comparison stage (ambi_path_compare.hpp) on the CPU with
// the one-thread HostGroup, for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wno-unknown-pragmas
//       -I ambigram_amd/csrc tests/tools/path_compare_stage_check.cpp -o path_compare_stage_check && ./path_compare_stage_check
// Hand-built and random pairs of paths over the cells {+-1 .. +-3} go through compare_pair as GIVEN paths; what it leaves is compared
// with a naive transcription written here: prefix and suffix by plain loops, the LCS by the quadratic table, dist = la + lb - 2 LCS
// replaced by -1 above dmax.  The cells of both sides lie in ONE heap block of exactly their size, at offsets that are and are not
// multiples of four cells, with stale non-zero cells between the paths; the side named B ends at the block's last cell, so a read
// behind a path is either a wrong result or the sanitizer's to report.  V has exactly 2 * dmax + 3 ints.  Covered on purpose: paths
// of 1 and 2 cells, equal paths, proper prefix and suffix, one changed cell at the first, a middle and the last position, x^5 against
// x^7, the reverse complement, a palindrome, snakes of 7 / 8 / 9 and 63 / 64 / 65 cells, a distance of exactly dmax and dmax + 1,
// dmax = 0, |la - lb| > dmax, 3 cells against 200 at dmax = 1024.
// What this program does NOT reach: on HostGroup a sub-group is one thread, so a snake that is handed over grows one pair per ballot
// round here and a sweep's tile is 8 cells.  The 64-lane hand-over and the 2048-cell tile run on the device only; the GPU half of
// tests/test_path_compare.py covers them with the same shapes and with snakes of more than 1024 cells.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ambi_path_compare.hpp"

using namespace ambi;

static int fails = 0, g_case = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s (case %d)\n", __FILE__, __LINE__, #x, g_case); fails++; } } while (0)
// what the cases reached
static int n_equal = 0, n_over = 0, n_exact = 0, n_exact1 = 0, n_rounds = 0, n_trim_only = 0, n_rc_equal = 0, n_aligned = 0, n_unaligned = 0, n_offgrid = 0;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 11); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }   // inclusive
static int rnd_cell() { const int v = rnd_in(1, 3); return rnd() & 1 ? v : -v; }

typedef std::vector<int> Path;
static Path rc(const Path& f) { Path r(f.rbegin(), f.rend()); for (int& v : r) v = -v; return r; }
static Path rnd_path(int n) { Path p((size_t)n); for (int& v : p) v = rnd_cell(); return p; }
static Path cat(const Path& a, const Path& b) { Path r(a); r.insert(r.end(), b.begin(), b.end()); return r; }
static Path rep(const Path& x, int k) { Path r; for (int i = 0; i < k; i++) r.insert(r.end(), x.begin(), x.end()); return r; }

// ---- the transcription -----------------------------------------------------------------------------------------------------
static int ref_lcs(const Path& a, const Path& b) {
    std::vector<int> prev(b.size() + 1, 0), cur(b.size() + 1, 0);
    for (size_t i = 1; i <= a.size(); i++) {
        for (size_t j = 1; j <= b.size(); j++) cur[j] = a[i - 1] == b[j - 1] ? prev[j - 1] + 1 : std::max(prev[j], cur[j - 1]);
        prev.swap(cur);
    }
    return prev[b.size()];
}
static PathCompare ref_compare(const Path& a, const Path& b, int dmax) {
    PathCompare R{};
    const int la = (int)a.size(), lb = (int)b.size();
    R.len_a = la; R.len_b = lb; R.dmax = dmax;
    for (int o = 0; o < 2; o++) {
        const Path B = o ? rc(b) : b;
        int p = 0, s = 0;
        while (p < la && p < lb && a[(size_t)p] == B[(size_t)p]) p++;
        while (s < std::min(la, lb) - p && a[(size_t)(la - 1 - s)] == B[(size_t)(lb - 1 - s)]) s++;
        const int l = ref_lcs(a, B), d = la + lb - 2 * l;
        R.prefix[o] = p; R.suffix[o] = s; R.dist[o] = d <= dmax ? d : -1; R.lcs[o] = d <= dmax ? l : -1;
        n_equal += d == 0; n_over += d > dmax; n_exact += d == dmax && d > 0; n_exact1 += d == dmax + 1;
        n_rounds += d > 0 && d <= dmax && la - p - s > 0 && lb - p - s > 0; n_trim_only += la - p - s == 0 || lb - p - s == 0;
        n_rc_equal += o == 1 && d == 0;
        n_offgrid += d <= dmax && d > std::min(la - p - s, lb - p - s) && std::min(la - p - s, lb - p - s) > 0;
    }
    return R;
}

// ---- one case --------------------------------------------------------------------------------------------------------------
static void run_case(const Path& a, const Path& b, int dmax, int pad_a, int pad_b) {
    g_case++;
    // one block: [pad_a stale cells][a][pad_b stale cells][b], b ends the block
    const size_t oa = (size_t)pad_a, ob = oa + a.size() + (size_t)pad_b, total = ob + b.size();
    rcell_t* block = static_cast<rcell_t*>(malloc(total * sizeof(rcell_t)));
    for (size_t i = 0; i < total; i++) block[i] = (rcell_t)(i % 2 ? 3 : -2);
    for (size_t i = 0; i < a.size(); i++) block[oa + i] = (rcell_t)a[i];
    for (size_t i = 0; i < b.size(); i++) block[ob + i] = (rcell_t)b[i];
    const int64_t off[2] = {(int64_t)oa, (int64_t)ob};
    const int32_t len[2] = {(int32_t)a.size(), (int32_t)b.size()};
    n_aligned += ((reinterpret_cast<uintptr_t>(block + oa) & 7) == 0) + ((reinterpret_cast<uintptr_t>(block + ob) & 7) == 0);
    n_unaligned += ((reinterpret_cast<uintptr_t>(block + oa) & 7) != 0) + ((reinterpret_cast<uintptr_t>(block + ob) & 7) != 0);
    const CompareGiven given{block, off, len, 2};
    const int32_t pairs[6] = {~0, ~1, ~1, ~0, ~0, ~0};
    int32_t* V = static_cast<int32_t*>(malloc((size_t)compare_lds_bytes(dmax)));
    PathCompare* out = static_cast<PathCompare*>(malloc(3 * sizeof(PathCompare)));
    memset(out, 0x5a, 3 * sizeof(PathCompare));
    HostGroup g;
    for (int i = 0; i < 3; i++) compare_pair(g, nullptr, nullptr, given, pairs, i, dmax, V, out);
    const PathCompare want[3] = {ref_compare(a, b, dmax), ref_compare(b, a, dmax), ref_compare(a, a, dmax)};
    for (int i = 0; i < 3; i++) {
        const bool same = memcmp(&out[i], &want[i], sizeof(PathCompare)) == 0;
        if (!same)
            printf("  pair %d la %d lb %d dmax %d: got p %d %d s %d %d d %d %d l %d %d, want p %d %d s %d %d d %d %d l %d %d\n", i, want[i].len_a, want[i].len_b, dmax,
                   out[i].prefix[0], out[i].prefix[1], out[i].suffix[0], out[i].suffix[1], out[i].dist[0], out[i].dist[1], out[i].lcs[0], out[i].lcs[1],
                   want[i].prefix[0], want[i].prefix[1], want[i].suffix[0], want[i].suffix[1], want[i].dist[0], want[i].dist[1], want[i].lcs[0], want[i].lcs[1]);
        CHECK(same);
    }
    CHECK(out[2].dist[0] == 0 && out[2].prefix[0] == (int)a.size() && out[2].suffix[0] == 0);   // the pair (a, a)
    free(out); free(V); free(block);
}
static void run_all(const Path& a, const Path& b) {
    static const int dmaxs[] = {0, 1, 2, 4, 16, 64, 1024};
    for (int dmax : dmaxs) run_case(a, b, dmax, g_case % 5, (g_case / 5) % 4);
}
// a at every distance around its own: dist exactly dmax and dmax + 1
static void run_at_own_distance(const Path& a, const Path& b) {
    const int d = (int)a.size() + (int)b.size() - 2 * ref_lcs(a, b);
    for (int dmax : {d - 1, d, d + 1}) if (dmax >= 0 && dmax <= kCompareDmaxCap) run_case(a, b, dmax, 0, g_case % 4);
}

int main() {
    const Path x = {1, 2, -3};
    // paths of 1 and 2 cells
    for (int c1 : {1, -1, 2}) for (int c2 : {1, -1, -2}) { run_all({c1}, {c2}); run_all({c1}, {c2, c1}); run_all({c1, c2}, {c2, c1}); run_all({c1, c2}, {-c2, -c1}); }
    for (int n : {3, 8, 9, 17, 64, 100}) {
        const Path a = rnd_path(n), t = rnd_path(5);
        run_all(a, a);                                  // equal
        run_all(a, cat(a, t)); run_all(cat(a, t), a);   // a proper prefix
        run_all(a, cat(t, a)); run_all(cat(t, a), a);   // a proper suffix
        for (int at : {0, n / 2, n - 1}) { Path b = a; b[(size_t)at] = b[(size_t)at] == 3 ? -3 : 3; run_all(a, b); run_at_own_distance(a, b); }   // one changed cell
        run_all(a, rc(a));                              // the reverse complement
        run_all(cat(a, rc(a)), cat(a, rc(a)));          // a palindrome: both orientations 0
    }
    run_all(rep(x, 5), rep(x, 7)); run_all(rep(x, 7), rep(x, 5)); run_all(rep({2}, 5), rep({2}, 7));   // periodic: the suffix stops at min - prefix
    // snakes of 7, 8, 9 and 63, 64, 65 cells between two edits (the hand-over and ballot edges)
    for (int snake : {7, 8, 9, 63, 64, 65}) {
        const Path s = rnd_path(snake), h = rnd_path(4), t = rnd_path(4);
        run_all(cat(cat(cat(h, {1}), s), cat({2}, t)), cat(cat(cat(h, {-1}), s), cat({-2}, t)));
        run_all(cat(cat(cat(h, {1, 1}), s), t), cat(cat(h, s), cat({3}, t)));
        run_at_own_distance(cat(cat({1}, s), {2}), cat(cat({-1}, s), {-2}));
    }
    // |la - lb| > dmax; 3 cells against 200 at dmax 1024: diagonals leave the grid
    run_all(rnd_path(3), rnd_path(200)); run_all(rnd_path(200), rnd_path(3)); run_all({1, 2, 3}, cat(cat(rnd_path(90), {1, 2, 3}), rnd_path(107)));
    run_all(rnd_path(40), rnd_path(140));
    // random pairs: a path and an edited copy, and unrelated paths
    for (int it = 0; it < 400; it++) {
        const int n = rnd_in(1, 60);
        const Path a = rnd_path(n);
        Path b = a;
        const int edits = rnd_in(0, 6);
        for (int e = 0; e < edits && !b.empty(); e++) {
            const size_t at = (size_t)rnd_in(0, (int)b.size() - 1);
            const int kind = rnd_in(0, 2);
            if (kind == 0) b[at] = rnd_cell(); else if (kind == 1) b.insert(b.begin() + (long)at, rnd_cell()); else if (b.size() > 1) b.erase(b.begin() + (long)at);
        }
        if (it % 3 == 0) b = rc(b);
        if (it % 7 == 0) b = rnd_path(rnd_in(1, 60));
        static const int caps[5] = {0, 1, 4, 16, 64};
        run_case(a, b, caps[it % 5], it % 4, (it / 4) % 4);
        if (it % 10 == 0) run_at_own_distance(a, b);
    }
    CHECK(n_equal > 50 && n_over > 50 && n_exact > 10 && n_exact1 > 10 && n_rounds > 200 && n_trim_only > 50 && n_rc_equal > 10);
    CHECK(n_aligned > 100 && n_unaligned > 100 && n_offgrid > 10);
    printf("cases %d: equal %d over %d exact %d exact+1 %d rounds %d trim-only %d rc-equal %d aligned %d unaligned %d off-grid %d\n", g_case, n_equal, n_over, n_exact,
           n_exact1, n_rounds, n_trim_only, n_rc_equal, n_aligned, n_unaligned, n_offgrid);
    if (fails) { printf("path_compare_stage_check: %d FAILED\n", fails); return 1; }
    printf("path_compare_stage_check: ok\n");
    return 0;
}
