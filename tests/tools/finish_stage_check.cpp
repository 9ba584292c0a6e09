// tests/tools/finish_stage_check.cpp -- stand-alone check of the finish-stage functions (ambi_finish.hpp) on the CPU with the
// one-thread HostGroup, for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wno-unknown-pragmas
//       -I ambigram_amd/csrc tests/tools/finish_stage_check.cpp -o finish_stage_check && ./finish_stage_check
// Random paths (as run lists and as cells) and random junction-end lists -- near pairs of the path, backward pairs, chains of two to
// seven links with random middle vertices, random pairs, junctions that do not qualify -- go through indel_collect, indel_bfb,
// indel_bfb_runs (with runs_build, tables_from_runs and runs_find_first), synth_out_juncs and synth_out_juncs_runs; what they leave
// is compared with a std::vector transcription of LocalGenomicMap::indelBFB (LGM.cpp:3746-3837) and of the output-junction loop
// (localhap.cpp:267-289) written here.  Every buffer has exactly the size the stage is told, so a write at or past a capacity is the
// sanitizer's to report (the cells have 16 readable bytes behind their capacity: those hold a sentinel that is checked); the deque of
// chaining SVs ([2m + 4], head at m + 2) is filled to both of its ends.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ambi_finish.hpp"

using namespace ambi;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s (case %d)\n", __FILE__, __LINE__, #x, g_case); fails++; } } while (0)
static int g_case = 0;
static int n_edited = 0, n_capacity = 0, n_no_room = 0, n_chained = 0;   // what the cases reached (printed at the end)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 11); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }   // inclusive

typedef std::vector<int> Path;
struct Run { int a, len; };

// ---- the transcription -----------------------------------------------------------------------------------------------------
static bool qualifies(int s, int t, int n) {
    const int a = std::abs(s), b = std::abs(t);
    if (a < 1 || a > n || b < 1 || b > n) return false;
    const bool same = (s < 0) == (t < 0);
    if (!same && std::abs(a - b) <= 2) return false;
    if (same && ((s > 0 && b - a == 1) || (s < 0 && a - b == 1))) return false;
    return true;
}
static int find_in(const Path& p, int lo, int hi, int v) { for (int i = lo; i < hi; i++) if (p[(size_t)i] == v) return i; return hi; }

// returns 0 (no SV), 1, or ST_ERR_PATH_CAPACITY where an edit would grow the path beyond pcap (the engine's rule; the reference has none)
static int ref_indel(Path& path, const std::vector<JuncEnds>& ends, int n, int pcap, bool* edited) {
    std::vector<JuncEnds> sv;
    for (const JuncEnds& e : ends) if (qualifies(e.s, e.t, n)) sv.push_back(e);
    *edited = false;
    if (sv.empty()) return 0;
    while (!sv.empty()) {
        std::vector<int> group;
        for (size_t i = 0; i < sv.size(); i++) {
            const int as = sv[i].s, at = sv[i].t, bs = -sv[i].t, bt = -sv[i].s;
            if (group.empty()) { group.push_back(as); group.push_back(at); }
            else if (at == group.front()) group.insert(group.begin(), as);
            else if (bt == group.front()) group.insert(group.begin(), bs);
            else if (group.back() == as) group.push_back(at);
            else if (group.back() == bs) group.push_back(bt);
            else continue;
            sv.erase(sv.begin() + (long)i);
            i--;
        }
        const int P = (int)path.size();
        auto complement = [&]() { std::reverse(group.begin(), group.end()); for (int& v : group) v = -v; };
        auto after = [&](int pos1, int v) { return pos1 >= P ? P : find_in(path, pos1 + 1, P, v); };
        if (group.size() == 2) {
            const bool same = (group[0] > 0) == (group[1] > 0);
            const bool deletion = same && ((group[0] > 0 && std::abs(group[0]) < std::abs(group[1])) || (group[0] < 0 && std::abs(group[0]) > std::abs(group[1])));
            if (same && !deletion) {
                int pos1 = find_in(path, 0, P, group[0]), pos2 = find_in(path, 0, pos1, group[1]);
                if (pos1 == P || pos2 == pos1) { complement(); pos1 = find_in(path, 0, P, group[0]); pos2 = find_in(path, 0, pos1, group[1]); }
                if (pos1 == P || pos2 == pos1) continue;
                if (P + (pos1 + 1 - pos2) > pcap) return ST_ERR_PATH_CAPACITY;
                const Path copy(path.begin() + pos2, path.begin() + pos1 + 1);
                path.insert(path.begin() + pos1 + 1, copy.begin(), copy.end());
                *edited = true;
            } else {
                const int limit = same ? 3 : 5;
                int pos1 = find_in(path, 0, P, group[0]), pos2 = after(pos1, group[1]);
                if (pos1 == P || pos2 == P) { complement(); pos1 = find_in(path, 0, P, group[0]); pos2 = after(pos1, group[1]); }
                if (pos1 == P || pos2 == P || pos2 - pos1 > limit) continue;
                if (pos2 > pos1 + 1) *edited = true;      // (an erase of nothing leaves the engine's flag alone: the path is the same)
                path.erase(path.begin() + pos1 + 1, path.begin() + pos2);
            }
        } else {
            int pos1 = find_in(path, 0, P, group.front()), pos2 = after(pos1, group.back());
            if (pos1 == P || pos2 == P) { complement(); pos1 = find_in(path, 0, P, group.front()); pos2 = after(pos1, group.back()); }
            if (pos1 == P || pos2 == P) continue;
            if (P - (pos2 - pos1 - 1) + (int)group.size() - 2 > pcap) return ST_ERR_PATH_CAPACITY;
            path.erase(path.begin() + pos1 + 1, path.begin() + pos2);
            path.insert(path.begin() + pos1 + 1, group.begin() + 1, group.end() - 1);
            *edited = true;
        }
    }
    return 1;
}

static std::vector<OutJunc> ref_out_juncs(const Path& p, int base) {
    std::vector<OutJunc> acc;
    for (size_t i = 0; i + 1 < p.size(); i++) {
        const int a = p[i], b = p[i + 1];
        if (b - a == 1 || b - a == -1) continue;     // ids one apart on one strand (vertices are non-zero)
        bool found = false;
        for (OutJunc& j : acc) {
            const int ju = j.u > 0 ? j.u - base : j.u + base, jv = j.v > 0 ? j.v - base : j.v + base;
            if ((ju == a && jv == b) || (ju == -b && jv == -a)) { j.count++; found = true; break; }
        }
        if (!found) acc.push_back(OutJunc{a > 0 ? a + base : a - base, b > 0 ? b + base : b - base, 1});
    }
    return acc;
}

// ---- inputs ----------------------------------------------------------------------------------------------------------------
static std::vector<Run> random_runs(int n, int np, bool with_empty) {
    std::vector<Run> r;
    for (int j = 0; j < np; j++) {
        if (with_empty && rnd() % 7 == 0) { r.push_back(Run{rnd_in(1, n), 0}); continue; }
        if (rnd() & 1) { const int a = rnd_in(1, n); r.push_back(Run{a, rnd_in(1, std::min(n - a + 1, 9))}); }
        else { const int a = rnd_in(1, n); r.push_back(Run{-a, rnd_in(1, std::min(a, 9))}); }     // -a, -a + 1, .. stays below 0
    }
    return r;
}
static Path cells_of(const std::vector<Run>& r) { Path p; for (const Run& x : r) for (int k = 0; k < x.len; k++) p.push_back(x.a + k); return p; }
static int vertex(int n) { return (rnd() & 1 ? 1 : -1) * rnd_in(1, n); }

static std::vector<JuncEnds> random_ends(const Path& p, int n, int m) {
    std::vector<JuncEnds> e;
    const int P = (int)p.size();
    auto add = [&](int s, int t) { if (rnd() & 1) { const int x = s; s = -t; t = -x; } e.push_back(JuncEnds{(int16_t)s, (int16_t)t}); };
    while ((int)e.size() < m) {
        const uint32_t kind = rnd() % 8;
        if (P < 9 || kind == 0) add(vertex(n), vertex(n));                                    // random pair (some do not qualify)
        else if (kind == 1) { const int i = rnd_in(1, n - 1); add(i, i + 1); }                // a normal junction
        else if (kind <= 3) { const int q = rnd_in(0, P - 8); add(p[(size_t)q], p[(size_t)(q + rnd_in(1, 7))]); }       // near pair
        else if (kind == 4) { const int q = rnd_in(0, P - 8); add(p[(size_t)(q + rnd_in(1, 7))], p[(size_t)q]); }      // backward pair
        else {                                                                                // a chain, its links in random order
            const int L = rnd_in(2, 7), q = rnd_in(0, P - 8);
            std::vector<int> c;
            c.push_back(rnd() % 5 ? p[(size_t)q] : vertex(n));
            for (int k = 1; k < L; k++) c.push_back(vertex(n));
            c.push_back(rnd() % 5 ? p[(size_t)(q + rnd_in(1, 7))] : vertex(n));
            std::vector<int> order;
            for (int k = 0; k < L; k++) order.push_back(k);
            for (int k = L - 1; k > 0; k--) std::swap(order[(size_t)k], order[(size_t)rnd_in(0, k)]);
            for (int k : order) add(c[(size_t)k], c[(size_t)k + 1]);
        }
    }
    e.resize((size_t)m);
    return e;
}

// a buffer of cells, 16-byte aligned, with the 16 bytes of slack synth_out_juncs reads (never writes) behind `cap` cells.  The slack
// and the rounding behind it lie inside the allocation, where the sanitizer does not look: they hold a sentinel, and intact() says
// whether anything wrote at or behind the capacity.
struct Cells {
    static constexpr cell_t kSent = 0x5a5a;
    std::vector<uint64_t> mem;
    int cap;
    explicit Cells(int cap_) : mem((size_t)(2 * cap_ + 16 + 15) / 8 + 2, 0), cap(cap_) { for (cell_t* p = data() + cap; p < end(); p++) *p = kSent; }
    cell_t* data() { uint8_t* b = reinterpret_cast<uint8_t*>(mem.data()); while (reinterpret_cast<uintptr_t>(b) & 15) b++; return reinterpret_cast<cell_t*>(b); }
    cell_t* end() { return reinterpret_cast<cell_t*>(mem.data() + mem.size()); }
    bool intact() { for (cell_t* p = data() + cap; p < end(); p++) if (*p != kSent) return false; return true; }
};
struct Scratch {
    std::vector<int32_t> sv, grp, first, last;
    std::vector<uint8_t> taken, has_ext;
    Scratch(int n, int m) : sv((size_t)m), grp((size_t)(2 * m + 4)), first((size_t)(2 * n + 1)), last((size_t)(2 * n + 1)), taken((size_t)m), has_ext((size_t)m) {}
    IndelScratch get() { return IndelScratch{sv.data(), taken.data(), has_ext.data(), grp.data(), first.data(), last.data()}; }
};

static bool same_out(const std::vector<OutJunc>& a, const OutJunc* b, int nb) {
    if ((int)a.size() != nb) return false;
    for (int i = 0; i < nb; i++) if (a[(size_t)i].u != b[i].u || a[(size_t)i].v != b[i].v || a[(size_t)i].count != b[i].count) return false;
    return true;
}

// ---- one case through everything -------------------------------------------------------------------------------------------
static void check_case(int n, const std::vector<Run>& runs, const std::vector<JuncEnds>& ends, int pcap, int run_cap, int seg_base) {
    HostGroup g;
    const int m = (int)ends.size(), np = (int)runs.size();
    const Path start = cells_of(runs);
    const int P0 = (int)start.size();
    if (P0 > pcap) return;
    Path want = start;
    bool want_edited = false;
    const int want_rc = ref_indel(want, ends, n, pcap, &want_edited);
    n_edited += want_rc == 1 && want_edited; n_capacity += want_rc < 0;
    int want_nsv = 0;
    for (const JuncEnds& e : ends) want_nsv += qualifies(e.s, e.t, n);

    {   // indel_collect: the qualifying junctions in order
        Scratch S(n, m);
        const int nsv = indel_collect(g, n, ends.data(), m, S.get());
        CHECK(nsv == want_nsv);
        for (int k = 0; k < nsv; k++) if (S.has_ext[(size_t)k]) { n_chained++; break; }
        int k = 0;
        for (int j = 0; j < m; j++) if (qualifies(ends[(size_t)j].s, ends[(size_t)j].t, n)) { CHECK(k < nsv && S.sv[(size_t)k] == j && S.taken[(size_t)k] == 0); k++; }
    }
    int cells_edited = -1;
    {   // the cell form
        Scratch S(n, m);
        Cells C(pcap);
        cell_t* path = C.data();
        for (int i = 0; i < P0; i++) path[i] = (cell_t)start[(size_t)i];
        int P = P0;
        bool edited = true;
        const int rc = indel_bfb(g, n, ends.data(), m, path, &P, pcap, S.get(), &edited);
        CHECK(rc == want_rc);
        CHECK(C.intact() && P <= pcap);          // nothing at or behind the capacity, whether the edits fitted or not
        if (rc >= 0) {
            CHECK(P == (int)want.size() && (edited || !want_edited));   // (an applied group that erases nothing may set the flag: the path is then stored though it is the same)
            bool eq = P == (int)want.size();
            for (int i = 0; eq && i < P; i++) eq = path[i] == want[(size_t)i];
            CHECK(eq);
            // output junctions of the final cells, at the exact capacity, one short of it, and with room
            const std::vector<OutJunc> wo = ref_out_juncs(want, seg_base);
            int steps = 0;
            for (int i = 0; i + 1 < P; i++) steps += (want[(size_t)i + 1] - want[(size_t)i] != 1 && want[(size_t)i + 1] - want[(size_t)i] != -1);
            for (int cap : {(int)wo.size(), (int)wo.size() - 1, (int)wo.size() + 5}) {
                if (cap < 0) continue;
                for (int list : {steps, steps - 1}) {
                    if (list < 0) continue;
                    const int cand_cap = 3 * list + 1;                    // room for exactly `list` steps (finish_cand_cap's rule)
                    std::vector<int32_t> cand((size_t)cand_cap);
                    std::vector<OutJunc> out((size_t)cap);
                    const int nout = synth_out_juncs(g, path, P, out.data(), cap, cand.data(), cand_cap, seg_base);
                    if (list < steps || cap < (int)wo.size()) CHECK(nout == ST_ERR_OUTJUNC_CAPACITY);
                    else CHECK(nout == (int)wo.size() && same_out(wo, out.data(), nout));
                }
            }
            cells_edited = edited ? 1 : 0;
        }
    }
    {   // the run form
        Scratch S(n, m);
        std::vector<cell_t> val0((size_t)(2 * np)), val1((size_t)(2 * run_cap)), val2((size_t)(2 * run_cap));
        std::vector<int32_t> off0((size_t)np + 1), off1((size_t)run_cap + 1), off2((size_t)run_cap + 1), loc(8);
        int at = 0;
        for (int j = 0; j < np; j++) { val0[(size_t)(2 * j)] = (cell_t)runs[(size_t)j].a; off0[(size_t)j] = at; at += runs[(size_t)j].len; }
        off0[(size_t)np] = at;
        RunList cur{val0.data(), off0.data(), np, P0};
        RunList buf[2] = {{val1.data(), off1.data(), 0, 0}, {val2.data(), off2.data(), 0, 0}};
        bool edited = true;
        const int rc = indel_bfb_runs(g, n, ends.data(), m, cur, buf, run_cap, pcap, S.get(), loc.data(), &edited);
        n_no_room += rc == kRunsNoRoom;
        if (rc == kRunsNoRoom) CHECK(run_cap < pcap + 4 * np);           // (a list has no more runs than cells and empty runs)
        else if (want_rc < 0) CHECK(rc == want_rc);
        else {
            CHECK(rc == want_rc && (int)edited == cells_edited && cur.P == (int)want.size());    // the two forms agree on the flag
            Path got;
            for (int r = 0; r < cur.n; r++) for (int k = 0; k < cur.off[r + 1] - cur.off[r]; k++) got.push_back((int)cur.val[2 * r] + k);
            CHECK(got == want);
            // tables and finds of the final list against the cells
            std::vector<int32_t> first((size_t)(2 * n + 1), 12345), last((size_t)(2 * n + 1), 12345);
            tables_from_runs(g, n, cur, first.data(), last.data());
            for (int v = -n; v <= n; v++) {
                int f = 0x7fffffff, l = -1;
                for (int i = 0; i < (int)want.size(); i++) if (want[(size_t)i] == v) { if (f == 0x7fffffff) f = i; l = i; }
                CHECK(first[(size_t)(v + n)] == f && last[(size_t)(v + n)] == l);
            }
            for (int t = 0; t < 8 && !want.empty(); t++) {
                const int from = rnd_in(0, (int)want.size()), v = rnd() % 3 ? want[(size_t)rnd_in(0, (int)want.size() - 1)] : vertex(n);
                CHECK(runs_find_first(g, cur, from, v) == find_in(want, from, (int)want.size(), v));
                const RunPath RP{cur.val, cur.off, cur.n};
                const int hi = std::min((int)want.size() - 1, from + 5);
                const int q = find_in(want, from, hi + 1, v);
                CHECK(RP.scan_for(from, hi, v) == (q <= hi ? q : -1));
                if (from < (int)want.size()) CHECK(RP.at(from) == want[(size_t)from]);
            }
            // the output junctions from the runs, with and without the hash table
            const std::vector<OutJunc> wo = ref_out_juncs(want, seg_base);
            int steps = 0;                       // repeats included: a unit has room for as many steps as records
            for (size_t i = 0; i + 1 < want.size(); i++) steps += (want[i + 1] - want[i] != 1 && want[i + 1] - want[i] != -1);
            for (int cap : {steps, steps - 1, (int)wo.size(), (int)wo.size() - 1}) {
                if (cap < 0) continue;
                for (int table = 0; table < 2; table++) {
                    std::vector<int32_t> cand((size_t)(3 * (cur.n + 1))), htab((size_t)(table ? 2 * synth_hash_size(cur.n, 1 << 30) : 1));
                    std::vector<OutJunc> out((size_t)cap);
                    const int nout = synth_out_juncs_runs(g, cur.val, cur.n, cur.off, out.data(), cap, cand.data(), seg_base, table ? htab.data() : nullptr, table ? (int)htab.size() : 0);
                    if (cap < steps) CHECK(nout == ST_ERR_OUTJUNC_CAPACITY);
                    else CHECK(nout == (int)wo.size() && same_out(wo, out.data(), nout));
                }
            }
        }
    }
    {   // runs_build alone: three random slices and literal cells into a list of exactly the size it reports
        std::vector<cell_t> val0((size_t)(2 * np));
        std::vector<int32_t> off0((size_t)np + 1), loc(8);
        int at = 0;
        for (int j = 0; j < np; j++) { val0[(size_t)(2 * j)] = (cell_t)runs[(size_t)j].a; off0[(size_t)j] = at; at += runs[(size_t)j].len; }
        off0[(size_t)np] = at;
        const RunList S{val0.data(), off0.data(), np, P0};
        int x[3], y[3];
        for (int k = 0; k < 3; k++) { x[k] = rnd_in(0, P0); y[k] = rnd_in(0, P0); if (rnd() % 4 == 0) y[k] = x[k]; }
        const int nlit = rnd_in(0, 3), lit_at = rnd_in(0, 3);
        int32_t lit[3] = {vertex(n), vertex(n), vertex(n)};
        Path wantp;
        for (int k = 0; k < 3; k++) {
            if (k == lit_at) for (int i = 0; i < nlit; i++) wantp.push_back(lit[i]);
            for (int i = x[k]; i < y[k]; i++) wantp.push_back(start[(size_t)i]);
        }
        if (lit_at >= 3) for (int i = 0; i < nlit; i++) wantp.push_back(lit[i]);
        // first with no room at all (the count comes back through D.n), then with exactly that many runs
        RunList D0{nullptr, nullptr, 0, 0};
        CHECK(runs_build(g, S, D0, -1, loc.data(), 3, x, y, lit_at, lit, nlit) == -1);
        const int need = D0.n;
        std::vector<cell_t> dval((size_t)(2 * need) + 1);
        std::vector<int32_t> doff((size_t)need + 1);
        RunList D{dval.data(), doff.data(), 0, 0};
        CHECK(runs_build(g, S, D, need, loc.data(), 3, x, y, lit_at, lit, nlit) == need && D.P == (int)wantp.size());
        Path got;
        for (int r = 0; r < D.n; r++) for (int k = 0; k < D.off[r + 1] - D.off[r]; k++) got.push_back((int)D.val[2 * r] + k);
        CHECK(got == wantp);
    }
}

// the deque of chaining SVs filled to its front end and to its back end: m links of ONE chain, listed from the back of the chain to
// its front (every link joins at the front: head goes from m + 2 down to 3) or from the front to the back (tail up to 2m + 3)
static void check_deque(int m, bool to_front, bool complemented) {
    int n = m + 8;
    while (n % 5 == 0) n++;          // (the chain below steps by five segments: all its vertices distinct)
    std::vector<Run> runs = {Run{1, n}, Run{-n, n}};
    std::vector<JuncEnds> ends;
    // chain 1 -> -3 -> 5 -> -7 .. over distinct segments, every link a strand switch more than two segments wide where it can be
    std::vector<int> c;
    for (int k = 0; k <= m; k++) c.push_back((k & 1 ? -1 : 1) * (1 + (k * 5) % n));
    for (int k = 0; k < m; k++) {
        int s = c[(size_t)k], t = c[(size_t)k + 1];
        if (complemented) { const int x = s; s = -t; t = -x; }
        ends.push_back(JuncEnds{(int16_t)s, (int16_t)t});
    }
    if (to_front) std::reverse(ends.begin(), ends.end());
    check_case(n, runs, ends, 4 * n + m, 4 * n + m + 16, 0);
}

int main() {
    for (g_case = 0; g_case < 3000; g_case++) {
        const int n = g_case % 5 == 0 ? rnd_in(3, 9) : rnd_in(10, 70);
        const int np = g_case % 11 == 0 ? rnd_in(1, 3) : rnd_in(2, 40);
        const std::vector<Run> runs = random_runs(n, np, g_case % 3 == 0);
        const Path p = cells_of(runs);
        const int m = g_case % 13 == 0 ? 0 : rnd_in(1, 24);
        const std::vector<JuncEnds> ends = random_ends(p, n, m);
        const int P = (int)p.size();
        const int pcap = g_case % 4 == 0 ? P + rnd_in(0, 6) : 3 * P + 64;          // tight: duplications and insertions meet the capacity
        const int run_cap = g_case % 6 == 0 ? np + rnd_in(0, 4) : 4 * (pcap + 4 * np) + 64;
        check_case(n, runs, ends, pcap, run_cap, g_case % 2 ? 0 : 1000);
    }
    for (int m : {1, 2, 3, 17, 64, 200})
        for (int f = 0; f < 2; f++) for (int c = 0; c < 2; c++) { g_case = 100000 + m; check_deque(m, f != 0, c != 0); }
    printf("cases with an edited path %d, with a chaining SV %d, over the path capacity %d, run lists out of room %d\n", n_edited, n_chained, n_capacity, n_no_room);
    if (n_edited < 1000 || n_chained < 1000 || n_capacity < 50 || n_no_room < 50) { printf("FAIL: the inputs no longer reach what they are for\n"); fails++; }
    printf(fails ? "%d checks failed\n" : "finish_stage_check: ok\n", fails);
    return fails ? 1 : 0;
}
