// tests/tools/path_align_stage_check.cpp -- stand-alone check of the path alignment stage (ambi_path_align.hpp) on the CPU with the
// one-thread HostGroup, for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wno-unknown-pragmas
//       -I ambigram_amd/csrc tests/tools/path_align_stage_check.cpp -o path_align_stage_check && ./path_align_stage_check
// Hand-built and random pairs of paths over the cells {+-1 .. +-3} go through align_pair as GIVEN paths, in both orientations; what
// it leaves is compared with a naive transcription written here: prefix and suffix by plain loops, the distance from the quadratic
// LCS table (-1 above dmax), and the script by applying it -- the runs, taken in order, must turn a into Bo, their lengths must sum to
// the distance, they must be ordered and maximal, and every slot behind n_runs must be zero.  The cells of both sides lie in ONE
// heap block of exactly their size, with stale non-zero cells between the paths and the side named B at the block's end; V has
// exactly 2 * dmax + 3 ints, the edit list exactly 2 * dmax, the history exactly (dmax + 1)(dmax + 2) / 2, the headers 32 bytes and
// the runs 16 * max(dmax, 1) bytes an entry: a read or write behind any of them is the sanitizer's to report.
// What this program does NOT reach: on HostGroup the merge's tile is one edit and a sub-group one thread.  The 256-edit tile and the
// 64-lane hand-over run on the device only; the GPU half of tests/test_path_align.py covers them (293 runs, one run of 300 cells).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ambi_path_align.hpp"

using namespace ambi;

static int fails = 0, g_case = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s (case %d)\n", __FILE__, __LINE__, #x, g_case); fails++; } } while (0)
// what the cases reached
static int n_equal = 0, n_over = 0, n_exact = 0, n_exact1 = 0, n_traced = 0, n_one_run = 0, n_merged = 0, n_del_ins = 0, n_offgrid = 0, n_both = 0;

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
// one entry: the header against plain loops and the table, the runs by applying them
static void check_entry(const Path& a, const Path& b, int o, int dmax, const PathAlign& H, const AlignRun* runs) {
    const Path B = o ? rc(b) : b;
    const int la = (int)a.size(), lb = (int)B.size();
    int p = 0, s = 0;
    while (p < la && p < lb && a[(size_t)p] == B[(size_t)p]) p++;
    while (s < std::min(la, lb) - p && a[(size_t)(la - 1 - s)] == B[(size_t)(lb - 1 - s)]) s++;
    const int d = la + lb - 2 * ref_lcs(a, B), n = la - p - s, m = lb - p - s, stride = align_stride(dmax);
    CHECK(H.status == 0 && H.len_a == la && H.len_b == lb && H.orient == o && H.prefix == p && H.suffix == s);
    CHECK(H.dist == (d <= dmax ? d : -1));
    CHECK(H.n_runs >= 0 && H.n_runs <= stride && (H.dist > 0 ? H.n_runs >= 1 && H.n_runs <= H.dist : H.n_runs == 0));
    n_equal += d == 0; n_over += d > dmax; n_exact += d == dmax && d > 0; n_exact1 += d == dmax + 1;
    n_traced += d > 0 && d <= dmax && n > 0 && m > 0; n_one_run += d > 0 && d <= dmax && (n == 0 || m == 0);
    n_offgrid += d <= dmax && n > 0 && m > 0 && d > std::min(n, m);
    if (H.n_runs < 0 || H.n_runs > stride) return;
    for (int r = H.n_runs; r < stride; r++) CHECK(runs[r].a_pos == 0 && runs[r].b_pos == 0 && runs[r].len == 0 && runs[r].kind == 0);
    if (H.dist < 0) return;
    // apply the script
    Path out;
    int ai = 0, sum = 0;
    bool del = false, ins = false;
    for (int r = 0; r < H.n_runs; r++) {
        const AlignRun& R = runs[r];
        const bool sane = R.len >= 1 && (R.kind == 0 || R.kind == 1) && R.a_pos >= ai && R.a_pos <= la && (R.kind == 0 ? R.a_pos + R.len <= la : R.b_pos >= 0 && R.b_pos + R.len <= lb);
        CHECK(sane);
        if (!sane) return;
        out.insert(out.end(), a.begin() + ai, a.begin() + R.a_pos);
        CHECK(R.b_pos == (int)out.size());
        if (R.kind == 0) ai = R.a_pos + R.len;
        else { out.insert(out.end(), B.begin() + R.b_pos, B.begin() + R.b_pos + R.len); ai = R.a_pos; }
        sum += R.len; del = del || R.kind == 0; ins = ins || R.kind == 1;
        n_merged += R.len > 1;
        if (r > 0) {   // maximal: two runs of one kind have a matched cell between them
            const AlignRun& Q = runs[r - 1];
            const int ea = Q.kind == 0 ? Q.a_pos + Q.len : Q.a_pos;
            CHECK(Q.kind != R.kind || R.a_pos > ea);
            n_del_ins += Q.kind == 0 && R.kind == 1 && R.a_pos == ea;
        }
    }
    out.insert(out.end(), a.begin() + ai, a.end());
    CHECK(out == B);
    CHECK(sum == H.dist);
    n_both += del && ins;
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
    const CompareGiven given{block, off, len, 2};
    const int kEntries = 6, stride = align_stride(dmax);
    const int32_t triples[3 * kEntries] = {~0, ~1, 0, ~0, ~1, 1, ~1, ~0, 0, ~1, ~0, 1, ~0, ~0, 0, ~1, ~1, 1};
    int32_t* V = static_cast<int32_t*>(malloc((size_t)compare_lds_bytes(dmax)));
    int32_t* E = static_cast<int32_t*>(malloc(dmax > 0 ? (size_t)(8 * dmax) : 1));
    int32_t* H = static_cast<int32_t*>(malloc((size_t)(4 * align_history_ints(dmax))));
    PathAlign* head = static_cast<PathAlign*>(malloc(kEntries * sizeof(PathAlign)));
    AlignRun* runs = static_cast<AlignRun*>(malloc((size_t)kEntries * (size_t)stride * sizeof(AlignRun)));
    memset(head, 0x5a, kEntries * sizeof(PathAlign));
    memset(runs, 0x5a, (size_t)kEntries * (size_t)stride * sizeof(AlignRun));
    memset(H, 0x5a, (size_t)(4 * align_history_ints(dmax)));
    HostGroup g;
    for (int i = 0; i < kEntries; i++) align_pair(g, nullptr, nullptr, given, triples, i, dmax, V, E, H, head, runs);
    const Path* side[2] = {&a, &b};
    for (int i = 0; i < kEntries; i++) check_entry(*side[~triples[3 * i]], *side[~triples[3 * i + 1]], triples[3 * i + 2], dmax, head[i], runs + (size_t)i * (size_t)stride);
    CHECK(head[4].dist == 0 && head[4].prefix == (int)a.size() && head[4].n_runs == 0);   // the entry (a, a, as is)
    free(runs); free(head); free(H); free(E); free(V); free(block);
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
    for (int c1 : {1, -1, 2}) for (int c2 : {1, -1, -2}) { run_all({c1}, {c2}); run_all({c1}, {c2, c1}); run_all({c1, c2}, {c2, c1}); run_all({c1, c2}, {-c2, -c1}); }
    for (int n : {3, 8, 9, 17, 64, 100}) {
        const Path a = rnd_path(n), t = rnd_path(5);
        run_all(a, a);                                  // equal
        run_all(a, cat(a, t)); run_all(cat(a, t), a);   // a proper prefix: one run by the shortcut
        run_all(a, cat(t, a)); run_all(cat(t, a), a);   // a proper suffix
        for (int at : {0, n / 2, n - 1}) { Path b = a; b[(size_t)at] = b[(size_t)at] == 3 ? -3 : 3; run_all(a, b); run_at_own_distance(a, b); }   // one substituted cell: D then I
        run_all(a, rc(a));
        run_all(cat(a, rc(a)), cat(a, rc(a)));          // a palindrome: both orientations 0
        Path gone;                                      // every third cell deleted: many runs of one kind
        for (int i = 0; i < n; i++) if (i % 3 != 1) gone.push_back(a[(size_t)i]);
        run_all(a, gone); run_at_own_distance(a, gone);
        if (n >= 17) { Path cut(a.begin(), a.begin() + 4); cut.insert(cut.end(), a.begin() + n - 6, a.end()); run_all(a, cut); run_at_own_distance(cut, a); }   // one long run
    }
    run_all(rep(x, 5), rep(x, 7)); run_all(rep(x, 7), rep(x, 5)); run_all(rep({2}, 5), rep({2}, 7));   // periodic: many shortest scripts, the tie rule decides
    for (int snake : {7, 8, 9, 63, 64, 65}) {
        const Path s = rnd_path(snake), h = rnd_path(4), t = rnd_path(4);
        run_all(cat(cat(cat(h, {1}), s), cat({2}, t)), cat(cat(cat(h, {-1}), s), cat({-2}, t)));
        run_all(cat(cat(cat(h, {1, 1}), s), t), cat(cat(h, s), cat({3}, t)));
        run_at_own_distance(cat(cat({1}, s), {2}), cat(cat({-1}, s), {-2}));
    }
    // 3 cells against 200 at dmax 1024: history rows clipped by the grid
    run_all(rnd_path(3), rnd_path(200)); run_all(rnd_path(200), rnd_path(3)); run_all({1, 2, 3}, cat(cat(rnd_path(90), {1, 2, 3}), rnd_path(107)));
    run_all(rnd_path(40), rnd_path(140));
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
    CHECK(n_equal > 50 && n_over > 50 && n_exact > 10 && n_exact1 > 10 && n_traced > 200 && n_one_run > 50);
    CHECK(n_merged > 50 && n_del_ins > 50 && n_offgrid > 10 && n_both > 100);
    printf("cases %d: equal %d over %d exact %d exact+1 %d traced %d one-run %d merged runs %d D-then-I %d off-grid %d both kinds %d\n", g_case, n_equal, n_over, n_exact, n_exact1,
           n_traced, n_one_run, n_merged, n_del_ins, n_offgrid, n_both);
    if (fails) { printf("path_align_stage_check: %d FAILED\n", fails); return 1; }
    printf("path_align_stage_check: ok\n");
    return 0;
}
