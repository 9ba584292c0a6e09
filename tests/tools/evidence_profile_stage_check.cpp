// tests/tools/evidence_profile_stage_check.cpp -- stand-alone check of the two evidence depth profile stages
// (ambi_evidence_profile.hpp) on the CPU with the one-thread HostGroup, for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wno-unknown-pragmas
//       -I ambigram_amd/csrc tests/tools/evidence_profile_stage_check.cpp -o evidence_profile_stage_check && ./evidence_profile_stage_check
// Random and periodic paths over the cells {+-1, +-2}, fragments cut from them or drawn at random and random junction lists over
// the same cells go through stage_evidence_mark and stage_evidence_scan; what they leave is compared with a naive transcription
// of the definitions written here (a window compare at every position, +1 on every step under the window; the first junction
// whose edge A or B equals the step).  With four cell values the occurrences overlap heavily and most junctions share an edge
// class with another.  Every buffer has exactly the size the stages are told -- the depth array P entries, filled with stale
// values before the call --, so a read or write past one is the sanitizer's to report.  Covered on purpose: P = 1, 2, 3, 8, 9,
// 2048, 2049 (a thread's chunk and a sweep of 256 x 8, each exactly and with one more), F = 0, windows of 1 pattern and of 1
// junction, and the predicate of the 2^31 depth bound.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ambi_evidence_profile.hpp"

using namespace ambi;

static int fails = 0, g_case = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s (case %d)\n", __FILE__, __LINE__, #x, g_case); fails++; } } while (0)
static int n_deep = 0, n_gap = 0, n_tie = 0, n_partly = 0, n_unmatched_cov = 0, n_f0 = 0, n_window1 = 0, n_jwin1 = 0, n_shared_class = 0;   // what the cases reached

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 11); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }   // inclusive
static int rnd_cell() { static const int v[4] = {1, -1, 2, -2}; return v[rnd() & 3]; }

typedef std::vector<int> Frag;
static Frag rc(const Frag& f) { Frag r(f.rbegin(), f.rend()); for (int& v : r) v = -v; return r; }

// ---- the transcription -----------------------------------------------------------------------------------------------------
static void cover(const std::vector<int>& path, const Frag& f, std::vector<int32_t>& depth) {
    const int P = (int)path.size(), L = (int)f.size();
    for (int i = 0; i + L <= P; i++) {
        bool same = true;
        for (int k = 0; k < L && same; k++) same = path[(size_t)(i + k)] == f[(size_t)k];
        if (same) for (int k = i; k <= i + L - 2; k++) depth[(size_t)k]++;
    }
}
static void ref_profile(const std::vector<int>& path, const std::vector<Frag>& frags, const std::vector<JuncEnds>& ends, std::vector<int32_t>& depth,
                        std::vector<int32_t>& count, std::vector<int32_t>& covered, std::vector<int32_t>& mind, UnitEvidenceProfile& s) {
    const int P = (int)path.size(), steps = P - 1, m = (int)ends.size();
    memset(&s, 0, sizeof(s));
    depth.assign((size_t)steps, 0);
    for (const Frag& f : frags) { cover(path, f, depth); if (rc(f) != f) cover(path, rc(f), depth); }
    count.assign((size_t)m, 0); covered.assign((size_t)m, 0); mind.assign((size_t)m, -1);
    s.steps = steps; s.juncs = m; s.first_uncovered = -1; s.longest_uncovered_at = -1;
    for (int k = 0; k < steps; k++) {
        const int d = depth[(size_t)k], x = path[(size_t)k], y = path[(size_t)k + 1];
        s.steps_covered += d > 0; s.max_depth = std::max(s.max_depth, d); s.depth_sum += d;
        if (d == 0 && s.first_uncovered < 0) s.first_uncovered = k;
        int j = 0;
        while (j < m && !((ends[(size_t)j].s == x && ends[(size_t)j].t == y) || (-ends[(size_t)j].t == x && -ends[(size_t)j].s == y))) j++;
        if (j == m) { s.unmatched_covered += d > 0; continue; }
        count[(size_t)j]++; covered[(size_t)j] += d > 0;
        mind[(size_t)j] = mind[(size_t)j] < 0 ? d : std::min(mind[(size_t)j], d);
    }
    int ties = 0;
    for (int k = 0; k < steps;) {
        if (depth[(size_t)k]) { k++; continue; }
        int q = k;
        while (q < steps && depth[(size_t)q] == 0) q++;
        if (q - k > s.longest_uncovered) { s.longest_uncovered = q - k; s.longest_uncovered_at = k; ties = 0; }
        else if (q - k == s.longest_uncovered) ties++;
        k = q;
    }
    for (int j = 0; j < m; j++) {
        const int c = count[(size_t)j], v = covered[(size_t)j];
        s.juncs_used += c > 0; s.juncs_covered += c > 0 && v == c; s.juncs_uncovered += c > 0 && v == 0;
        n_partly += v > 0 && v < c;
    }
    n_deep += s.max_depth >= 3; n_gap += s.longest_uncovered > 1 && s.steps_covered > 0; n_tie += ties > 0 && s.longest_uncovered > 0;
    n_unmatched_cov += s.unmatched_covered > 0;
}

// ---- one case --------------------------------------------------------------------------------------------------------------
static void run_case(const std::vector<int>& path, const std::vector<Frag>& frags, const std::vector<JuncEnds>& ends, int pwin, int jwin, bool aligned) {
    g_case++;
    const int P = (int)path.size(), F = (int)frags.size(), m = (int)ends.size();
    // the cells: 8-byte aligned and readable up to the next multiple of four, or off by one cell and exactly P long
    std::vector<rcell_t> store(aligned ? (size_t)((P + 3) & ~3) : (size_t)P + 1, (rcell_t)0);
    rcell_t* cells = store.data() + (aligned ? 0 : 1);
    for (int i = 0; i < P; i++) cells[i] = (rcell_t)path[(size_t)i];
    std::vector<rcell_t> fc;
    std::vector<int32_t> foff(1, 0);
    for (const Frag& f : frags) { for (int v : f) fc.push_back((rcell_t)v); foff.push_back((int32_t)fc.size()); }
    // the depth array: exactly P entries (aligned: a heap block of its own, 16-byte aligned as a unit's slice is; else off by one
    // entry: the cell-by-cell form), stale values inside
    std::vector<int32_t> dstore(aligned ? (size_t)P : (size_t)P + 1, 0x12345);
    int32_t* depth = dstore.data() + (aligned ? 0 : 1);
    const int fslots = frag_slots(pwin);
    std::vector<int32_t> lds((size_t)(frag_profile_lds_bytes(fslots, pwin) / 4), 0x5a5a5a5a);
    const FragTable T = frag_table(lds.data(), fslots, pwin);
    const int slots = junc_slots(jwin);
    std::vector<int32_t> lds2((size_t)(evidence_scan_lds_bytes(slots, 1) / 4), 0x5a5a5a5a);
    const EvidenceTable E = evidence_table(lds2.data(), slots);
    CHECK(reinterpret_cast<int32_t*>(E.runs + 1) == lds2.data() + lds2.size());
    std::vector<int32_t> gc((size_t)m, -7), gv((size_t)m, -7), gm((size_t)m, -7), wd, wc, wv, wm;
    UnitEvidenceProfile gs, ws;
    memset(&gs, 0x5a, sizeof(gs));
    HostGroup g;
    stage_evidence_mark(g, cells, P, fc.data(), foff.data(), F, T, depth);
    long long total = 0;
    for (int i = 0; i < P; i++) total += depth[i];
    CHECK(total == 0);                                  // a difference array: every +1 has its -1
    stage_evidence_scan(g, cells, P, ends.data(), m, jwin, E, depth, gc.data(), gv.data(), gm.data(), &gs);
    gs.status = 0;
    ref_profile(path, frags, ends, wd, wc, wv, wm, ws);
    CHECK(std::vector<int32_t>(depth, depth + P - 1) == wd);
    CHECK(depth[P - 1] == 0);
    CHECK(gc == wc); CHECK(gv == wv); CHECK(gm == wm);
    CHECK(memcmp(&gs, &ws, sizeof(gs)) == 0);
    n_f0 += F == 0; n_window1 += pwin == 1 && F > 0; n_jwin1 += jwin == 1 && m > 1;
    for (int a = 0; a < m; a++) for (int b = a + 1; b < m; b++) if (junc_canon(ends[(size_t)a].s, ends[(size_t)a].t) == junc_canon(ends[(size_t)b].s, ends[(size_t)b].t)) { n_shared_class++; a = m; break; }
}

static std::vector<int> random_path(int P) { std::vector<int> p((size_t)P); for (int& v : p) v = rnd_cell(); return p; }
static std::vector<int> periodic_path(int P, int period) {
    const std::vector<int> unit = random_path(period);
    std::vector<int> p((size_t)P);
    for (int i = 0; i < P; i++) p[(size_t)i] = unit[(size_t)(i % period)];
    return p;
}
static std::vector<Frag> fragments_of(const std::vector<int>& path, int F) {
    const int P = (int)path.size();
    std::vector<Frag> out;
    for (int f = 0; f < F; f++) {
        Frag x;
        const int kind = rnd_in(0, 5);
        if (kind <= 2 && P >= 2) {            // cut from the path, sometimes reverse-complemented, sometimes mutated
            const int L = rnd_in(2, std::min(P, 12)), i = rnd_in(0, P - L);
            x.assign(path.begin() + i, path.begin() + i + L);
            if (kind == 1) x = rc(x);
            if (kind == 2) x[(size_t)rnd_in(0, L - 1)] = rnd_cell();
        } else if (kind == 3) {               // a palindrome
            Frag h = random_path(rnd_in(1, 3)), r = rc(h);
            x = h; x.insert(x.end(), r.begin(), r.end());
        } else if (kind == 4 && P <= 64) {    // longer than the path by one cell
            x = path; x.push_back(rnd_cell());
            if (x.size() < 2) x.push_back(rnd_cell());
        } else { x = random_path(rnd_in(5, 9)); }
        out.push_back(x);
    }
    return out;
}
static std::vector<JuncEnds> junctions(int m) {
    std::vector<JuncEnds> out((size_t)m);
    for (JuncEnds& e : out) { e = JuncEnds{}; e.s = rnd_cell(); e.t = rnd_cell(); }
    return out;
}

int main() {
    // the predicate of the depth bound: 2 * (cells - F) reaches 2^31
    CHECK(!evidence_depth_overflows(0, 0)); CHECK(!evidence_depth_overflows((int64_t(1) << 30) + 4, 5)); CHECK(evidence_depth_overflows((int64_t(1) << 30) + 5, 5));
    CHECK(evidence_depth_overflows((int64_t(1) << 31) - 1, 65535)); CHECK(!evidence_depth_overflows((int64_t(1) << 30) - 1, 0)); CHECK(evidence_depth_overflows(int64_t(1) << 30, 0));
    // the edges by hand
    run_case({1}, {{1, 1}, {1, -1}, {1, 2, 1}}, {}, 4, 1, true);
    run_case({1}, {}, junctions(3), 1, 2, false);
    run_case({1, -1}, {{1, -1}, {-1, 1}, {1, 1}, {1, -1, 1}}, junctions(4), 8, 4, true);
    run_case({2, 2}, {{2, 2}, {-2, -2}}, junctions(2), 1, 1, false);
    run_case({1, 1, 1, 1, 1, 1, 1}, {{1, 1}, {1, 1, 1}, {-1, -1, -1, -1}, {1, 1, 1, 1, 1, 1, 1}, {1, 1, 1, 1, 1, 1, 1, 1}}, junctions(5), 3, 2, true);
    // the shapes: a thread's chunk and a sweep, each exactly and with one more; periodic paths full of overlapping occurrences
    for (int P : {1, 2, 3, 8, 9, 2048, 2049})
        for (int v = 0; v < 6; v++) {
            const std::vector<int> path = v % 2 ? periodic_path(P, rnd_in(1, 7)) : random_path(P);
            const int F = v == 0 ? 0 : rnd_in(1, 10), m = v == 5 ? 0 : rnd_in(1, 12);
            const int pwins[3] = {1, 3, 2 * std::max(F, 1)}, jwins[3] = {1, 4, std::max(m, 1)};
            run_case(path, fragments_of(path, F), junctions(m), pwins[v % 3], jwins[(v / 2) % 3], (v & 1) == 0);
        }
    // gaps: a long random path and few long fragments leave uncovered stretches; two-cell fragments cover almost everything
    for (int c = 0; c < 300; c++) {
        const int P = c % 7 == 0 ? rnd_in(1, 4) : rnd_in(5, 500);
        const std::vector<int> path = c % 3 == 0 ? periodic_path(P, rnd_in(1, 9)) : random_path(P);
        const int F = c % 11 == 0 ? 0 : rnd_in(1, c % 5 == 0 ? 30 : 4), m = rnd_in(0, 14);
        const int pwins[5] = {1, 2, 7, 64, 2 * std::max(F, 1)}, jwins[4] = {1, 3, 8, std::max(m, 1)};
        run_case(path, fragments_of(path, F), junctions(m), pwins[c % 5], jwins[c % 4], (c & 1) == 0);
    }
    printf("cases %d: deep %d gap %d tie %d partly %d unmatched_cov %d f0 %d window1 %d jwin1 %d shared_class %d\n", g_case, n_deep, n_gap, n_tie, n_partly,
           n_unmatched_cov, n_f0, n_window1, n_jwin1, n_shared_class);
    CHECK(n_deep > 0); CHECK(n_gap > 0); CHECK(n_tie > 0); CHECK(n_partly > 0); CHECK(n_unmatched_cov > 0); CHECK(n_f0 > 0);
    CHECK(n_window1 > 0); CHECK(n_jwin1 > 0); CHECK(n_shared_class > 0);
    if (fails) { printf("evidence_profile_stage_check: %d FAILED\n", fails); return 1; }
    printf("evidence_profile_stage_check: ok\n");
    return 0;
}
