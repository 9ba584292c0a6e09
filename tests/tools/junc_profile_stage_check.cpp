// tests/tools/junc_profile_stage_check.cpp -- stand-alone check of the junction usage profile stage (ambi_junc_profile.hpp) on the
// CPU with the one-thread HostGroup, for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wno-unknown-pragmas
//       -I ambigram_amd/csrc tests/tools/junc_profile_stage_check.cpp -o junc_profile_stage_check && ./junc_profile_stage_check
// Random paths (runs on either strand, joined by random steps) and random junction lists -- adjacencies, the path's own boundary
// steps from either side, fold-backs, random pairs, copies of all of them -- go through stage_junc_profile; what it leaves is compared
// with a std::map transcription of the join (localhap.cpp:277-278 over Junction.cpp:27-39, lowest index first) written here.
// Every buffer has exactly the size the stage is told (the cells end at the next multiple of four, or exactly at P when they are
// not 8-byte aligned), so a read or write past one is the sanitizer's to report.  Covered on purpose: m = 0, P = 1, duplicate
// edges, windows of size 1, tables with exactly as many classes as slots, and tables with more (the stage doubles its passes).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "ambi_junc_profile.hpp"

using namespace ambi;

static int fails = 0, g_case = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s (case %d)\n", __FILE__, __LINE__, #x, g_case); fails++; } } while (0)
static int n_unmatched_units = 0, n_dup_units = 0, n_multi_pass = 0, n_full = 0, n_over_full = 0, n_inrun_lost = 0;   // what the cases reached

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 11); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }   // inclusive

// ---- the transcription -----------------------------------------------------------------------------------------------------
static void ref_profile(const std::vector<int>& path, const std::vector<JuncEnds>& ends, const std::vector<double>& cn,
                        std::vector<int32_t>& count, UnitJuncProfile& s) {
    std::map<std::pair<int, int>, int> edge;
    for (int j = 0; j < (int)ends.size(); j++) {
        edge.insert({{ends[j].s, ends[j].t}, j});       // (insert keeps the first: the lowest index)
        edge.insert({{-ends[j].t, -ends[j].s}, j});
    }
    count.assign(ends.size(), 0);
    memset(&s, 0, sizeof(s));
    s.steps = (int)path.size() - 1; s.first_unmatched = -1; s.juncs = (int)ends.size();
    for (int i = 0; i + 1 < (int)path.size(); i++) {
        auto it = edge.find({path[(size_t)i], path[(size_t)i + 1]});
        if (it == edge.end()) { s.steps_unmatched++; if (s.first_unmatched < 0) s.first_unmatched = i; }
        else { count[(size_t)it->second]++; s.steps_matched++; }
    }
    for (size_t j = 0; j < ends.size(); j++) {
        s.juncs_used += count[j] > 0;
        s.max_count = std::max(s.max_count, count[j]);
        s.n_over += (double)count[j] - cn[j] >= 0.5;
        s.n_under += cn[j] - (double)count[j] >= 0.5;
    }
}

// ---- one case --------------------------------------------------------------------------------------------------------------
static void run_case(const std::vector<int>& path, int n, const std::vector<JuncEnds>& ends, const std::vector<double>& cn, int jwin, int slots,
                     int swin, bool aligned) {
    const int P = (int)path.size(), m = (int)ends.size();
    // the cells: 8-byte aligned and readable up to the next multiple of four, or off by one cell and exactly P long
    std::vector<rcell_t> store(aligned ? (size_t)((P + 3) & ~3) : (size_t)P + 1, (rcell_t)0);
    rcell_t* cells = store.data() + (aligned ? 0 : 1);
    for (int i = 0; i < P; i++) cells[i] = (rcell_t)path[(size_t)i];
    std::vector<int32_t> lds((size_t)(junc_profile_lds_bytes(slots, swin) / 4), -1);
    const JuncTable T = junc_table(lds.data(), slots, swin);
    std::vector<int32_t> got((size_t)m, -7), want;
    std::vector<JuncEnds> e(ends);     // (exactly m records each)
    std::vector<double> c(cn);
    UnitJuncProfile gs, ws;
    memset(&gs, 0x5a, sizeof(gs));
    HostGroup g;
    stage_junc_profile(g, cells, P, n, e.data(), c.data(), m, jwin, T, got.data(), &gs);
    ref_profile(path, ends, cn, want, ws);
    gs.status = 0;
    CHECK(got == want);
    CHECK(memcmp(&gs, &ws, sizeof(gs)) == 0);
    if (fails && fails < 4) printf("  P %d n %d m %d jwin %d slots %d swin %d: steps %d/%d matched %d/%d unmatched %d/%d first %d/%d used %d/%d max %d/%d\n", P, n, m, jwin,
                                   slots, swin, gs.steps, ws.steps, gs.steps_matched, ws.steps_matched, gs.steps_unmatched, ws.steps_unmatched, gs.first_unmatched,
                                   ws.first_unmatched, gs.juncs_used, ws.juncs_used, gs.max_count, ws.max_count);
    n_unmatched_units += ws.steps_unmatched > 0;
}

static std::vector<int> random_path(int n, int runs) {
    std::vector<int> p;
    for (int r = 0; r < runs; r++) {
        const int a = rnd_in(1, n), b = rnd_in(a, std::min(n, a + rnd_in(0, 12)));
        if (rnd() & 1) for (int v = a; v <= b; v++) p.push_back(v);
        else for (int v = b; v >= a; v--) p.push_back(-v);
    }
    return p;
}

static int classes_of(const std::vector<JuncEnds>& ends) {
    std::vector<uint32_t> k;
    for (const JuncEnds& e : ends) k.push_back(junc_canon(e.s, e.t));
    std::sort(k.begin(), k.end());
    return (int)(std::unique(k.begin(), k.end()) - k.begin());
}

static void random_junctions(const std::vector<int>& path, int n, int want, std::vector<JuncEnds>& ends, std::vector<double>& cn) {
    ends.clear(); cn.clear();
    auto add = [&](int s, int t) { ends.push_back(JuncEnds{(int16_t)s, (int16_t)t}); cn.push_back(rnd_in(0, 8) * 0.5); };
    bool dup = false;
    while ((int)ends.size() < want) {
        const int kind = rnd_in(0, 9);
        if (kind <= 2 && n > 1) { const int i = rnd_in(1, n - 1); if (rnd() & 1) add(i, i + 1); else add(-(i + 1), -i); }     // an adjacency, from either side
        else if (kind <= 5 && path.size() > 1) {                                                                           // a step of the path, from either side
            const int i = rnd_in(0, (int)path.size() - 2);
            if (rnd() & 1) add(path[(size_t)i], path[(size_t)i + 1]); else add(-path[(size_t)i + 1], -path[(size_t)i]);
        }
        else if (kind == 6) { const int s = rnd_in(1, n); if (rnd() & 1) add(s, -s); else add(-s, s); }                     // a fold-back
        else if (kind == 7 && !ends.empty()) {                                                                             // a copy, from either side
            const JuncEnds e = ends[(size_t)rnd_in(0, (int)ends.size() - 1)];
            if (rnd() & 1) add(e.s, e.t); else add(-e.t, -e.s);
            dup = true;
        }
        else add(rnd() & 1 ? rnd_in(1, n) : -rnd_in(1, n), rnd() & 1 ? rnd_in(1, n) : -rnd_in(1, n));
    }
    n_dup_units += dup;
}

int main() {
    std::vector<JuncEnds> ends;
    std::vector<double> cn;
    // random units at random windows
    for (g_case = 0; g_case < 1500; g_case++) {
        const int n = rnd_in(1, g_case % 7 == 0 ? 300 : 40);
        const std::vector<int> path = random_path(n, g_case % 11 == 0 ? 1 : rnd_in(1, 60));
        random_junctions(path, n, g_case % 13 == 0 ? 0 : rnd_in(1, 3 * n), ends, cn);
        const int m = (int)ends.size();
        const int jwin = g_case % 3 == 0 ? junc_window(m, 0) : rnd_in(1, std::max(1, m));
        const int swin = g_case % 3 == 1 ? junc_seg_window(n, 0) : rnd_in(1, n);
        n_multi_pass += jwin < m || swin < n;
        run_case(path, n, ends, cn, jwin, junc_slots(jwin), swin, (g_case & 1) == 0);
    }
    // P = 1 and m = 0, each with and without the other
    for (g_case = 2000; g_case < 2040; g_case++) {
        const int n = rnd_in(1, 20);
        std::vector<int> one(1, rnd() & 1 ? rnd_in(1, n) : -rnd_in(1, n));
        random_junctions(one, n, g_case & 1 ? 0 : rnd_in(1, 10), ends, cn);
        run_case(one, n, ends, cn, 1, junc_slots(1), 1, (g_case & 2) == 0);
        const std::vector<int> path = random_path(n, rnd_in(1, 10));
        run_case(path, n, std::vector<JuncEnds>(), std::vector<double>(), 1, junc_slots(1), rnd_in(1, n), (g_case & 2) != 0);
    }
    // windows of size 1 on both sides
    for (g_case = 3000; g_case < 3100; g_case++) {
        const int n = rnd_in(2, 24);
        const std::vector<int> path = random_path(n, rnd_in(2, 20));
        random_junctions(path, n, rnd_in(1, 40), ends, cn);
        run_case(path, n, ends, cn, 1, junc_slots(1), 1, (g_case & 1) == 0);
    }
    // tables filled to their capacity: one pass asked for (jwin = m) with exactly as many classes as slots, and with more
    for (g_case = 4000; g_case < 4200; g_case++) {
        const int n = rnd_in(8, 60), slots = 8 << rnd_in(0, 3);
        const std::vector<int> path = random_path(n, rnd_in(4, 40));
        const bool over = (g_case & 1) != 0;
        do random_junctions(path, n, rnd_in(slots, 3 * slots), ends, cn); while (classes_of(ends) < slots);
        while (!over && classes_of(ends) > slots) { ends.pop_back(); cn.pop_back(); }
        (over ? n_over_full : n_full) += over ? classes_of(ends) > slots : classes_of(ends) == slots;
        run_case(path, n, ends, cn, (int)ends.size(), slots, rnd_in(1, n), (g_case & 2) == 0);
    }
    // every adjacency present but one: its in-run crossings are unmatched, the first of them is reported
    for (g_case = 5000; g_case < 5100; g_case++) {
        const int n = rnd_in(3, 80), gone = rnd_in(1, n - 1);
        const std::vector<int> path = random_path(n, rnd_in(2, 30));
        ends.clear(); cn.clear();
        for (int i = 1; i < n; i++) if (i != gone) { ends.push_back(JuncEnds{(int16_t)i, (int16_t)(i + 1)}); cn.push_back(1.0); }
        for (size_t i = 0; i + 1 < path.size(); i++) if (path[i + 1] != path[i] + 1) { ends.push_back(JuncEnds{(int16_t)path[i], (int16_t)path[i + 1]}); cn.push_back(2.0); }
        for (size_t i = 0; i + 1 < path.size(); i++) if (path[i + 1] == path[i] + 1 && std::min(std::abs(path[i]), std::abs(path[i + 1])) == gone) { n_inrun_lost++; break; }
        const int m = (int)ends.size();
        run_case(path, n, ends, cn, g_case & 1 ? std::max(1, m / 3) : std::max(1, m), junc_slots(g_case & 1 ? std::max(1, m / 3) : std::max(1, m)),
                 g_case & 2 ? rnd_in(1, n) : n, (g_case & 4) == 0);
    }
    printf("units with unmatched steps %d, with copies %d, in several passes %d, tables exactly full %d, over full %d, lost adjacency crossed %d\n",
           n_unmatched_units, n_dup_units, n_multi_pass, n_full, n_over_full, n_inrun_lost);
    if (n_unmatched_units < 100 || n_dup_units < 100 || n_multi_pass < 500 || n_full < 50 || n_over_full < 50 || n_inrun_lost < 30) { printf("FAIL: a class of cases was not reached\n"); fails++; }
    if (fails) { printf("junc_profile_stage_check: %d FAILURES\n", fails); return 1; }
    printf("junc_profile_stage_check: ok\n");
    return 0;
}
