// tests/tools/fold_profile_stage_check.cpp -- stand-alone check of the two fold-back arm profile stages (ambi_fold_profile.hpp) on the
// CPU with the one-thread HostGroup, for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wno-unknown-pragmas
//       -I ambigram_amd/csrc tests/tools/fold_profile_stage_check.cpp -o fold_profile_stage_check && ./fold_profile_stage_check
// Hand-built and random paths over the cells {+-1 .. +-3} and random junction lists over the same cells go through stage_fold_arms
// and stage_fold_scan; what they leave is compared with a naive transcription of the definitions written here (every alignment
// tried in turn, the arm extended pair by pair, +1 on every step of the span; the first junction whose edge A or B equals the
// fold).  Every buffer has exactly the size the stages are told -- both planes P entries, filled with stale values before the
// call; the fold list 8 bytes per fold of the window --, so a read or write past one is the sanitizer's to report.  Covered on
// purpose: P = 1 and 2, folds at step 0 and at step P - 2, arms that end at the path's first and last cell, arms of 7 / 8 / 9
// (around the hand-over length kFoldHandover = 8) and 63 / 64 / 65, every alignment 1..4 alone, folds without an arm, fully
// alternating paths, fold windows of 1 and junction windows of 1.
// What this program does NOT reach: on HostGroup a sub-group is one thread (sub_size() = 1, the ballot is one bit), so an arm that is
// handed over grows one pair per round here.  The 64-lane form of the hand-over (r + lane, the ballot's lowest set bit, r += 64) runs
// on the device only; the GPU tests of tests/test_fold_profile.py cover it with arms of 63, 64 and more than 1024 cells.  The arms of
// 63 / 64 / 65 here check the arm length and the span's ends, not the wavefront.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ambi_fold_profile.hpp"

using namespace ambi;

static int fails = 0, g_case = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s (case %d)\n", __FILE__, __LINE__, #x, g_case); fails++; } } while (0)
// what the cases reached
static int n_align[6], n_arm[70], n_fold_first = 0, n_fold_last = 0, n_end_first = 0, n_end_last = 0, n_all_folds = 0, n_fwin1 = 0, n_jwin1 = 0,
           n_rounds = 0, n_shared_class = 0, n_unmatched = 0, n_nested = 0, n_long = 0;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 11); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }   // inclusive
static int rnd_cell() { const int v = rnd_in(1, 3); return rnd() & 1 ? v : -v; }

typedef std::vector<int> Path;
static Path rc(const Path& f) { Path r(f.rbegin(), f.rend()); for (int& v : r) v = -v; return r; }

// ---- the transcription -----------------------------------------------------------------------------------------------------
static const int DL[5] = {0, -1, 0, -2, 0}, DR[5] = {1, 1, 2, 1, 3};
static void ref_profile(const Path& c, const std::vector<JuncEnds>& ends, std::vector<int32_t>& fold, std::vector<int32_t>& cover, std::vector<int32_t>& folds,
                        std::vector<int32_t>& max_arm, UnitFoldProfile& s) {
    const int P = (int)c.size(), steps = P - 1, m = (int)ends.size();
    memset(&s, 0, sizeof(s));
    fold.assign((size_t)steps, 0); cover.assign((size_t)steps, 0); folds.assign((size_t)m, 0); max_arm.assign((size_t)m, 0);
    s.steps = steps; s.max_arm_at = -1; s.max_cover_at = -1;
    for (int k = 0; k < steps; k++) {
        if ((c[(size_t)k] > 0) == (c[(size_t)k + 1] > 0)) continue;
        int al = -1, arm = 0;
        for (int a = 0; a < 5 && al < 0; a++) {
            const int i = k + DL[a], j = k + DR[a];
            int r = 0;
            while (i - r >= 0 && j + r < P && c[(size_t)(i - r)] == -c[(size_t)(j + r)]) r++;
            if (r == 0) continue;
            al = a; arm = r;
            for (int t = i - r + 1; t <= j + r - 2; t++) cover[(size_t)t]++;
            n_end_first += i - r + 1 == 0; n_end_last += j + r - 1 == P - 1;
        }
        fold[(size_t)k] = ((al + 2) << 24) | arm;
        s.folds++; s.folds_perfect += al == 0; s.folds_gapped += al > 0; s.folds_open += al < 0; s.arm_sum += arm;
        if (arm > s.max_arm) { s.max_arm = arm; s.max_arm_at = k; }
        n_align[al + 1]++; n_arm[std::min(arm, 69)]++; n_long += arm >= 200;
        n_fold_first += k == 0; n_fold_last += k == P - 2;
        const int x = c[(size_t)k], y = c[(size_t)k + 1];
        int j = 0;
        while (j < m && !((ends[(size_t)j].s == x && ends[(size_t)j].t == y) || (-ends[(size_t)j].t == x && -ends[(size_t)j].s == y))) j++;
        if (j == m) { s.folds_unmatched++; n_unmatched++; continue; }
        folds[(size_t)j]++; max_arm[(size_t)j] = std::max(max_arm[(size_t)j], arm);
    }
    for (int k = 0; k < steps; k++) {
        const int x = cover[(size_t)k];
        s.steps_covered += x > 0;
        if (x > s.max_cover) { s.max_cover = x; s.max_cover_at = k; }
    }
    n_all_folds += steps > 3 && s.folds == steps; n_nested += s.max_cover >= 4;
}

// ---- one case --------------------------------------------------------------------------------------------------------------
static std::vector<int32_t> g_fold;   // the fold plane of the last case, for the hand-built expectations
static void run_case(const Path& path, const std::vector<JuncEnds>& ends, int fwin, int jwin, bool aligned) {
    g_case++;
    const int P = (int)path.size(), m = (int)ends.size();
    // the cells: 8-byte aligned and readable up to the next multiple of four, or off by one cell and exactly P long
    std::vector<rcell_t> store(aligned ? (size_t)((P + 3) & ~3) : (size_t)P + 1, (rcell_t)0);
    rcell_t* cells = store.data() + (aligned ? 0 : 1);
    for (int i = 0; i < P; i++) cells[i] = (rcell_t)path[(size_t)i];
    if (aligned) for (int i = P; i < (int)store.size(); i++) store[(size_t)i] = (rcell_t)(-path[(size_t)(P - 1)]);   // stale cells behind P: a complement of the last cell
    // the planes: exactly P entries each (aligned: heap blocks of their own; else off by one entry: the entry-by-entry form), stale inside
    std::vector<int32_t> fstore(aligned ? (size_t)P : (size_t)P + 1, 0x03000007), cstore(aligned ? (size_t)P : (size_t)P + 1, 0x12345);
    int32_t* fold = fstore.data() + (aligned ? 0 : 1);
    int32_t* cover = cstore.data() + (aligned ? 0 : 1);
    std::vector<int32_t> lds((size_t)(fold_arm_lds_bytes(fwin) / 4), 0x5a5a5a5a);
    const FoldList L = fold_list(lds.data(), fwin);
    CHECK(L.val + fwin == lds.data() + lds.size());
    const int slots = junc_slots(jwin);
    std::vector<int32_t> lds2((size_t)(fold_scan_lds_bytes(slots) / 4), 0x5a5a5a5a);
    const FoldTable T = fold_table(lds2.data(), slots);
    CHECK(T.arm + slots == lds2.data() + lds2.size());
    std::vector<int32_t> gf((size_t)m, -7), gm((size_t)m, -7), wfold, wcover, wf, wm;
    UnitFoldProfile gs, ws;
    memset(&gs, 0x5a, sizeof(gs));
    HostGroup g;
    stage_fold_arms(g, cells, P, L, fold, cover);
    long long total = 0;
    for (int i = 0; i < P; i++) total += cover[i];
    CHECK(total == 0);                                  // a difference array: every +1 has its -1
    stage_fold_scan(g, cells, P, ends.data(), m, jwin, T, fold, cover, gf.data(), gm.data(), &gs);
    gs.status = 0;
    ref_profile(path, ends, wfold, wcover, wf, wm, ws);
    CHECK(std::vector<int32_t>(fold, fold + P - 1) == wfold);
    CHECK(std::vector<int32_t>(cover, cover + P - 1) == wcover);
    CHECK(fold[P - 1] == 0 && cover[P - 1] == 0);
    CHECK(gf == wf); CHECK(gm == wm);
    CHECK(memcmp(&gs, &ws, sizeof(gs)) == 0);
    n_fwin1 += fwin == 1 && ws.folds > 1; n_rounds += ws.folds > fwin; n_jwin1 += jwin == 1 && m > 1;
    for (int a = 0; a < m; a++) for (int b = a + 1; b < m; b++) if (junc_canon(ends[(size_t)a].s, ends[(size_t)a].t) == junc_canon(ends[(size_t)b].s, ends[(size_t)b].t)) { n_shared_class++; a = m; break; }
    g_fold = wfold;
}

static Path random_path(int P) { Path p((size_t)P); for (int& v : p) v = rnd_cell(); return p; }
static Path alternating_path(int P, bool ones) { Path p((size_t)P); for (int i = 0; i < P; i++) { const int v = ones ? 1 : rnd_in(1, 3); p[(size_t)i] = i & 1 ? -v : v; } return p; }
static std::vector<JuncEnds> junctions(int m) {
    std::vector<JuncEnds> out((size_t)m);
    for (JuncEnds& e : out) { e = JuncEnds{}; e.s = rnd_cell(); e.t = rnd() & 3 ? -e.s : rnd_cell(); }   // mostly fold-backs, as the folds are
    return out;
}
// [stop] L_r .. L_1 [ul x 2] | [ur x -2] -L_1 .. -L_r [stop]: one fold with alignment `a` and arm r at step *k.  L_1 = 1 and L_2, L_3 != 2
// keep the lower alignments from matching; a stop cell is one that is no complement of the cell across.
static Path palindrome(int r, int a, bool stop_l, bool stop_r, int* k) {
    Path L((size_t)r);
    for (int t = 0; t < r; t++) L[(size_t)t] = t == 0 ? 1 : t < 3 ? (rnd() & 1 ? 1 : 3) : rnd_in(1, 3);
    const int ul = a == 1 ? 1 : a == 3 ? 2 : 0, ur = a == 2 ? 1 : a == 4 ? 2 : 0;
    Path p;
    if (stop_l) p.push_back(1);
    for (int t = r - 1; t >= 0; t--) p.push_back(L[(size_t)t]);
    for (int t = 0; t < ul; t++) p.push_back(2);
    *k = (int)p.size() - 1;
    for (int t = 0; t < ur; t++) p.push_back(-2);
    for (int t = 0; t < r; t++) p.push_back(-L[(size_t)t]);
    if (stop_r) p.push_back(-3);
    return p;
}
// a breakage-fusion-bridge like path: a random start, then cycles that append the reverse complement of a suffix
static Path bfb_path(int cycles) {
    Path p;
    for (int i = rnd_in(2, 6); i > 0; i--) p.push_back(rnd_in(1, 3));
    for (int c = 0; c < cycles; c++) {
        const int n = rnd_in(1, (int)p.size());
        Path tail(p.end() - n, p.end());
        tail = rc(tail);
        if (rnd() % 4 == 0) tail.erase(tail.begin());                       // an imperfect fold-back
        if (rnd() % 5 == 0) tail.insert(tail.begin(), tail.empty() ? -1 : (tail[0] > 0 ? 3 : -3));
        p.insert(p.end(), tail.begin(), tail.end());
    }
    return p;
}

int main() {
    memset(n_align, 0, sizeof(n_align)); memset(n_arm, 0, sizeof(n_arm));
    CHECK(fold_align(fold_pack(-1, 0)) == -1 && fold_align(fold_pack(4, 12345)) == 4 && fold_arm(fold_pack(4, 12345)) == 12345 && fold_arm(fold_pack(0, (1 << 22) - 1)) == (1 << 22) - 1);
    // the edges by hand
    run_case({1}, {}, 1, 1, true);
    run_case({-2}, junctions(3), 4, 2, false);
    run_case({1, -1}, junctions(4), 1, 4, true);      CHECK(g_fold[0] == fold_pack(0, 1));    // a fold at step 0 = P - 2, its arm the whole path
    run_case({1, 1}, junctions(2), 2, 1, false);      CHECK(g_fold[0] == 0);
    run_case({1, -2}, junctions(2), 1, 1, true);      CHECK(g_fold[0] == fold_pack(-1, 0));   // a fold without an arm
    run_case({1, -2, 3}, {}, 1, 1, false);            CHECK(g_fold[0] == fold_pack(-1, 0) && g_fold[1] == fold_pack(-1, 0));
    run_case({1, -2, -2, -1}, junctions(3), 1, 2, true);   CHECK(g_fold[0] == fold_pack(4, 1));    // alignment 4 at step 0
    run_case({1, 2, 2, -1}, junctions(3), 1, 2, false);    CHECK(g_fold[2] == fold_pack(3, 1));    // alignment 3 at step P - 2
    // one fold per path: every alignment, arms around the hand-over length and around a sub-group's round, with and without stops
    const int arms[] = {1, 2, 3, 7, 8, 9, 10, 15, 16, 17, 63, 64, 65, 66, 71, 72, 73, 127, 128, 129, 200, 700};
    for (int r : arms)
        for (int a = 0; a < 5; a++)
            for (int stops = 0; stops < 4; stops++) {
                int k;
                const Path p = palindrome(r, a, stops & 1, stops & 2, &k);
                run_case(p, junctions(rnd_in(0, 6)), 1 + (r + a) % 3, 1 + stops, (r + a + stops) & 1);
                CHECK(g_fold[(size_t)k] == fold_pack(a, r));
            }
    // fully alternating paths: every step is a fold
    for (int P : {2, 3, 4, 5, 8, 9, 17, 50, 300}) {
        run_case(alternating_path(P, true), junctions(3), 1, 1, true);
        run_case(alternating_path(P, true), junctions(5), 7, 2, false);
        run_case(alternating_path(P, false), junctions(8), 1, 3, P & 1);
        run_case(alternating_path(P, false), junctions(0), 2048, 1, !(P & 1));
    }
    // nested palindromes as the cycles of a breakage-fusion-bridge leave them
    for (int c = 0; c < 120; c++) {
        const Path p = bfb_path(rnd_in(1, 9));
        const int m = rnd_in(0, 10);
        const int fwins[4] = {1, 2, 5, 2048}, jwins[3] = {1, 3, std::max(m, 1)};
        run_case(p, junctions(m), fwins[c % 4], jwins[c % 3], c & 1);
    }
    // random paths: short arms, many alignments, arm-less folds
    for (int c = 0; c < 300; c++) {
        const int P = c % 7 == 0 ? rnd_in(1, 4) : rnd_in(5, 600);
        const int m = rnd_in(0, 14);
        const int fwins[5] = {1, 2, 3, 64, 2048}, jwins[4] = {1, 3, 8, std::max(m, 1)};
        run_case(random_path(P), junctions(m), fwins[c % 5], jwins[c % 4], (c & 1) == 0);
    }
    printf("cases %d: align", g_case);
    for (int a = 0; a < 6; a++) printf(" %d", n_align[a]);
    printf("; arms 7/8/9 %d %d %d, 63/64/65 %d %d %d, long %d; fold at 0 %d, at P-2 %d; arm to first cell %d, to last %d; all folds %d; fwin1 %d rounds %d jwin1 %d "
           "shared_class %d unmatched %d nested %d\n", n_arm[7], n_arm[8], n_arm[9], n_arm[63], n_arm[64], n_arm[65], n_long, n_fold_first, n_fold_last, n_end_first,
           n_end_last, n_all_folds, n_fwin1, n_rounds, n_jwin1, n_shared_class, n_unmatched, n_nested);
    for (int a = 0; a < 6; a++) CHECK(n_align[a] > 0);
    for (int r : {1, 7, 8, 9, 63, 64, 65}) CHECK(n_arm[r] > 0);
    CHECK(n_long > 0); CHECK(n_fold_first > 0); CHECK(n_fold_last > 0); CHECK(n_end_first > 0); CHECK(n_end_last > 0); CHECK(n_all_folds > 0);
    CHECK(n_fwin1 > 0); CHECK(n_rounds > 0); CHECK(n_jwin1 > 0); CHECK(n_shared_class > 0); CHECK(n_unmatched > 0); CHECK(n_nested > 0);
    if (fails) { printf("fold_profile_stage_check: %d FAILED\n", fails); return 1; }
    printf("fold_profile_stage_check: ok\n");
    return 0;
}
