// tests/tools/frag_profile_stage_check.cpp -- stand-alone check of the fragment support profile stage (ambi_frag_profile.hpp) on the
// CPU with the one-thread HostGroup, for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wno-unknown-pragmas
//       -I ambigram_amd/csrc tests/tools/frag_profile_stage_check.cpp -o frag_profile_stage_check && ./frag_profile_stage_check
// Random and periodic paths over the cells {+-1, +-2} and fragments cut from them or drawn at random go through
// stage_frag_profile; what it leaves is compared with a naive transcription of the definitions written here (a window compare at
// every position, for the fragment and for its reverse complement unless the two are equal).  With four cell values the
// occurrences overlap, the chains on one first step are long, and palindromes are common.  Every buffer has exactly the size the
// stage is told (the cells end at the next multiple of four, or exactly at P when they are not 8-byte aligned), so a read or
// write past one is the sanitizer's to report.  Covered on purpose: P = 1, P = 2, F = 0, windows of 1, L > P, and a table with
// exactly as many first steps as half its slots (the load limit).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "ambi_frag_profile.hpp"

using namespace ambi;

static int fails = 0, g_case = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s (case %d)\n", __FILE__, __LINE__, #x, g_case); fails++; } } while (0)
static int n_overlap = 0, n_palindrome = 0, n_both = 0, n_long_chain = 0, n_load_limit = 0, n_window1 = 0, n_unsupported = 0, n_too_long = 0;   // what the cases reached

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 11); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }   // inclusive
static int rnd_cell() { static const int v[4] = {1, -1, 2, -2}; return v[rnd() & 3]; }

typedef std::vector<int> Frag;
static Frag rc(const Frag& f) { Frag r(f.rbegin(), f.rend()); for (int& v : r) v = -v; return r; }

// ---- the transcription -----------------------------------------------------------------------------------------------------
static std::vector<int> occurrences(const std::vector<int>& path, const Frag& f) {
    std::vector<int> at;
    const int P = (int)path.size(), L = (int)f.size();
    for (int i = 0; i + L <= P; i++) {
        bool same = true;
        for (int k = 0; k < L && same; k++) same = path[(size_t)(i + k)] == f[(size_t)k];
        if (same) at.push_back(i);
    }
    return at;
}
static void ref_profile(const std::vector<int>& path, const std::vector<Frag>& frags, std::vector<int32_t>& fwd, std::vector<int32_t>& rev,
                        std::vector<int32_t>& first, UnitFragProfile& s) {
    memset(&s, 0, sizeof(s));
    s.cells = (int)path.size(); s.frags = (int)frags.size(); s.first_unsupported = -1;
    fwd.clear(); rev.clear(); first.clear();
    for (size_t f = 0; f < frags.size(); f++) {
        const std::vector<int> a = occurrences(path, frags[f]);
        const std::vector<int> b = rc(frags[f]) == frags[f] ? std::vector<int>() : occurrences(path, rc(frags[f]));
        fwd.push_back((int)a.size()); rev.push_back((int)b.size());
        int at = -1;
        if (!a.empty()) at = a[0];
        if (!b.empty() && (at < 0 || b[0] < at)) at = b[0];
        first.push_back(at);
        const int tot = (int)(a.size() + b.size());
        if (tot > 0) { s.frags_supported++; s.longest_supported = std::max(s.longest_supported, (int)frags[f].size()); }
        else if (s.first_unsupported < 0) s.first_unsupported = (int)f;
        s.max_count = std::max(s.max_count, tot);
        s.occurrences += tot;
        // what the case offers
        const int L = (int)frags[f].size();
        for (size_t k = 1; k < a.size(); k++) if (a[k] - a[k - 1] < L) { n_overlap++; break; }
        n_palindrome += rc(frags[f]) == frags[f]; n_both += !a.empty() && !b.empty(); n_unsupported += tot == 0; n_too_long += L > (int)path.size();
    }
}

// ---- one case --------------------------------------------------------------------------------------------------------------
static void run_case(const std::vector<int>& path, const std::vector<Frag>& frags, int pwin, bool aligned) {
    g_case++;
    const int P = (int)path.size(), F = (int)frags.size();
    // the cells: 8-byte aligned and readable up to the next multiple of four, or off by one cell and exactly P long
    std::vector<rcell_t> store(aligned ? (size_t)((P + 3) & ~3) : (size_t)P + 1, (rcell_t)0);
    rcell_t* cells = store.data() + (aligned ? 0 : 1);
    for (int i = 0; i < P; i++) cells[i] = (rcell_t)path[(size_t)i];
    // the fragment image of the unit: exactly its cells and F + 1 offsets
    std::vector<rcell_t> fc;
    std::vector<int32_t> foff(1, 0);
    for (const Frag& f : frags) { for (int v : f) fc.push_back((rcell_t)v); foff.push_back((int32_t)fc.size()); }
    const int slots = frag_slots(pwin);
    std::vector<int32_t> lds((size_t)(frag_profile_lds_bytes(slots, pwin) / 4), 0x5a5a5a5a);
    const FragTable T = frag_table(lds.data(), slots, pwin);
    CHECK(T.first + pwin == lds.data() + lds.size());
    std::vector<int32_t> gf((size_t)F, -7), gr((size_t)F, -7), gi((size_t)F, -7), wf, wr, wi;
    UnitFragProfile gs, ws;
    memset(&gs, 0x5a, sizeof(gs));
    HostGroup g;
    stage_frag_profile(g, cells, P, fc.data(), foff.data(), F, T, gf.data(), gr.data(), gi.data(), &gs);
    gs.status = 0;
    ref_profile(path, frags, wf, wr, wi, ws);
    CHECK(gf == wf); CHECK(gr == wr); CHECK(gi == wi);
    CHECK(memcmp(&gs, &ws, sizeof(gs)) == 0);
    // first steps of the live patterns in the fullest window against the table's slots
    for (int w0 = 0; w0 < 2 * F; w0 += pwin) {
        std::set<std::pair<int, int>> keys;
        std::vector<int> per_key;
        for (int p = w0; p < std::min(2 * F, w0 + pwin); p++) {
            const Frag f = (p & 1) ? rc(frags[(size_t)(p >> 1)]) : frags[(size_t)(p >> 1)];
            if ((int)f.size() > P || ((p & 1) && rc(f) == f)) continue;
            keys.insert({f[0], f[1]});
        }
        if ((int)keys.size() * 2 == slots) n_load_limit++;
        if ((int)keys.size() == 1 && std::min(2 * F, w0 + pwin) - w0 >= 12) n_long_chain++;
    }
    n_window1 += pwin == 1 && F > 0;
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
        } else if (kind == 3) {               // a palindrome: a chain and its reverse complement behind it
            Frag h = random_path(rnd_in(1, 3)), r = rc(h);
            x = h; x.insert(x.end(), r.begin(), r.end());
        } else if (kind == 4) {               // longer than the path by one cell
            x = path; x.push_back(rnd_cell());
            if (x.size() < 2) x.push_back(rnd_cell());
        } else { x = random_path(rnd_in(2, 6)); }
        out.push_back(x);
    }
    return out;
}

int main() {
    // the edges by hand: P = 1, P = 2, F = 0
    run_case({1}, {{1, 1}, {1, -1}, {1, 2, 1}}, 4, true);
    run_case({1}, {}, 1, false);
    run_case({1, -1}, {{1, -1}, {-1, 1}, {1, 1}, {1, -1, 1}}, 8, true);
    run_case({2, 2}, {{2, 2}, {-2, -2}}, 1, false);
    run_case({1, 1, 1, 1, 1, 1, 1}, {{1, 1}, {1, 1, 1}, {-1, -1, -1, -1}, {1, 1, 1, 1, 1, 1, 1}, {1, 1, 1, 1, 1, 1, 1, 1}}, 3, true);   // overlapping occurrences
    for (int F : {0, 3}) for (int pwin : {1, 2, 5}) run_case(random_path(40), fragments_of(random_path(40), F), pwin, true);
    // a table at its load limit: 4 patterns of 4 distinct first steps in the 8 slots of a window of 4; 16 distinct steps in 32 slots
    run_case(random_path(64), {{1, 1, 2}, {1, 2, 2}}, 4, true);                      // + their reverse complements (-2,-1) (-2,-2)
    {
        std::vector<Frag> all;
        static const int v[4] = {1, -1, 2, -2};
        for (int a : v) for (int b : v) if (Frag{a, b} != rc(Frag{a, b})) all.push_back({a, b, 1});
        run_case(random_path(200), all, 16, false);
        run_case(random_path(200), all, 8, true);
    }
    // long chains on one first step: many fragments that all begin (1, 1), in one window and in windows of 1
    for (int pwin : {64, 1}) {
        std::vector<int> p = periodic_path(300, 3);
        p[0] = 1; p[1] = 1;
        std::vector<Frag> same;
        for (int L = 2; L < 26; L++) { Frag f = {1, 1}; for (int k = 2; k < L; k++) f.push_back(p[(size_t)k]); same.push_back(f); }
        for (int k = 0; k < 24; k++) { Frag f = {1, 1}; for (int q = rnd_in(0, 5); q > 0; q--) f.push_back(rnd_cell()); same.push_back(f); }
        run_case(p, same, pwin, true);
    }
    {   // a window that holds only patterns of one first step
        std::vector<Frag> pal;
        for (int k = 0; k < 16; k++) pal.push_back({2, 2, -2, -2});                   // palindromes: the odd patterns are idle
        run_case(periodic_path(500, 2), pal, 32, true);
        std::vector<Frag> chain;
        for (int k = 0; k < 8; k++) chain.push_back({2, 2, rnd_cell(), -2, -2});      // f and rc(f) both begin (2, 2)
        run_case(periodic_path(500, 5), chain, 16, false);
    }
    // random and periodic paths, random fragments, every window size
    for (int c = 0; c < 600; c++) {
        const int P = c % 7 == 0 ? rnd_in(1, 4) : rnd_in(5, 700);
        const std::vector<int> path = c % 3 == 0 ? periodic_path(P, rnd_in(1, 6)) : random_path(P);
        const int F = c % 11 == 0 ? 0 : rnd_in(1, 40);
        const int pwins[6] = {1, 2, 3, 7, 64, 2 * std::max(F, 1)};
        run_case(path, fragments_of(path, F), pwins[c % 6], (c & 1) == 0);
    }
    printf("cases %d: overlap %d palindrome %d both %d long_chain %d load_limit %d window1 %d unsupported %d too_long %d\n", g_case, n_overlap,
           n_palindrome, n_both, n_long_chain, n_load_limit, n_window1, n_unsupported, n_too_long);
    CHECK(n_overlap > 0); CHECK(n_palindrome > 0); CHECK(n_both > 0); CHECK(n_long_chain > 0); CHECK(n_load_limit > 0);
    CHECK(n_window1 > 0); CHECK(n_unsupported > 0); CHECK(n_too_long > 0);
    if (fails) { printf("frag_profile_stage_check: %d FAILED\n", fails); return 1; }
    printf("frag_profile_stage_check: ok\n");
    return 0;
}
