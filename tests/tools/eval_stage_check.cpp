// tests/tools/eval_stage_check.cpp -- stand-alone check of the per-order evaluation (ambi_eval.hpp, ambi_eval_lane.hpp) on the CPU
// with the one-thread HostGroup, for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wno-unknown-pragmas
//       -I ambigram_amd/csrc tests/tools/eval_stage_check.cpp -o eval_stage_check && ./eval_stage_check
// Random DAG records (loops with copy numbers up to 70, patterns, empty slots) over a small alphabet of segments, so that slots are
// found, skipped by the nesting test and missed, and random fold-back maps go through eval_place + eval_finish (imperfect_fbi),
// through eval_order_lane with the cells 1 and 64 apart, and through expand_bkp; shift_up and shift_down move random stretches.  What
// they leave is compared with a std::vector transcription of LocalGenomicMap::getBFB's per-order body (LGM.cpp:3519-3646) and of
// imperfectFBI (:3431-3512) written here.  The cells live in heap blocks of exactly `cap` cells (for the lane form: cap x 64, the
// lane under test the last one), the fold-back map in blocks of exactly n + 1 entries, so that a read or write past a capacity is
// the sanitizer's to report.  Every case runs at the smallest capacity that holds it and one cell short of it, where the stage has to
// end with ST_ERR_BKP_CAPACITY (expand_bkp: ST_ERR_PATH_CAPACITY) without touching the missing cell.
// The register form (eval_place_regs_n, imperfect_fbi_regs_n) is device code and cannot be built here.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "ambi_eval_lane.hpp"

using namespace ambi;

static int fails = 0, g_case = 0;
#define CHECK(x) do { if (!(x)) { if (fails < 20) printf("FAIL %s:%d: %s (case %d)\n", __FILE__, __LINE__, #x, g_case); fails++; } } while (0)
static long n_valid = 0, n_broke = 0, n_ub = 0, n_capacity = 0, n_rewritten = 0, n_nest_skips = 0, n_big_inserts = 0;   // what the cases reached

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 11); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }   // inclusive

typedef std::vector<int> Cells;
struct Inv { std::vector<int> src, tgt; };   // [0..n]; src == 0: no entry

// ---- the transcription -----------------------------------------------------------------------------------------------------
// Placement.  Returns the number of elements placed, ST_ERR_REF_UB where the reference indexes an empty record, or
// ST_ERR_BKP_CAPACITY by the engine's rule (a step that would grow the path beyond `cap` ends the evaluation; *L_out = the length
// before it).  *need = the largest length any step asked for.
static int ref_place(const Dag& D, const std::vector<int>& order, bool forward, int cap, Cells& bkp, int* L_out, int* need) {
    bkp.clear();
    *L_out = 0; *need = 0;
    int x = order[0];
    const bool isPat = D.pat[x][0] != 0, isLoop = D.loop[x][0] != 0;
    if (!isPat && !isLoop) return ST_ERR_REF_UB;
    {
        const int start = isPat ? D.pat[x][0] : D.loop[x][0], end = isPat ? D.pat[x][1] : D.loop[x][1];
        const int len = isPat ? 2 : 4 * D.loop[x][2];
        *need = len;
        if (len > cap) return ST_ERR_BKP_CAPACITY;
        if (isPat) {
            if (forward) { bkp.push_back(start); bkp.push_back(end); } else { bkp.push_back(-end); bkp.push_back(-start); }
        } else {
            for (int num = 0; num < D.loop[x][2]; num++) {
                if (forward) { bkp.push_back(start); bkp.push_back(end); bkp.push_back(-end); bkp.push_back(-start); }
                else { bkp.push_back(-end); bkp.push_back(-start); bkp.push_back(start); bkp.push_back(end); }
            }
        }
    }
    size_t i;
    for (i = 1; i < order.size(); i++) {
        x = order[i];
        if (D.pat[x][0] != 0) {
            const int start = D.pat[x][0], end = D.pat[x][1];
            *need = std::max(*need, (int)bkp.size() + 2);
            if ((int)bkp.size() + 2 > cap) { *L_out = (int)bkp.size(); return ST_ERR_BKP_CAPACITY; }
            if (bkp.back() == -start) { bkp.push_back(start); bkp.push_back(end); }
            else if (bkp.back() == end) { bkp.push_back(-end); bkp.push_back(-start); }
            else break;
        } else if (D.loop[x][0] != 0) {
            const int start = D.loop[x][0], end = D.loop[x][1], cn = D.loop[x][2];
            const int v1 = -start, v2 = end;
            // reverse iterators: pos = rbegin + k stands on index size - 1 - k; rend - pos = index + 1
            auto rfind = [&](long k, int v) { for (; k < (long)bkp.size(); k++) if (bkp[bkp.size() - 1 - (size_t)k] == v) return k; return (long)bkp.size(); };
            const long rend = (long)bkp.size();
            auto at = [&](long k) { return std::abs(bkp[bkp.size() - 1 - (size_t)k]); };
            long pos = rfind(0, v1);
            while (pos != rend && ((rend - pos) % 2 == 1 || (pos > 1 && at(pos + 1) < at(pos - 2)))) {
                if ((rend - pos) % 2 != 1) n_nest_skips++;
                pos = rfind(pos + 1, v1);
            }
            if (pos == rend) {
                pos = rfind(0, v2);
                while (pos != rend && ((rend - pos) % 2 == 1 || (pos > 1 && at(pos + 1) > at(pos - 2)))) {
                    if ((rend - pos) % 2 != 1) n_nest_skips++;
                    pos = rfind(pos + 1, v2);
                }
            }
            if (pos == rend) break;
            *need = std::max(*need, (int)bkp.size() + 4 * cn);
            if ((int)bkp.size() + 4 * cn > cap) { *L_out = (int)bkp.size(); return ST_ERR_BKP_CAPACITY; }
            n_big_inserts += 4 * cn >= 64;
            const size_t temp = bkp.size() - 1 - (size_t)pos;      // pos.base() - 1
            Cells loop;
            if (bkp[temp] == v1) {
                for (int num = 0; num < cn; num++) { loop.push_back(start); loop.push_back(end); loop.push_back(-end); loop.push_back(-start); }
                bkp[temp] = -start;
                if (temp + 1 != bkp.size()) bkp[temp + 1] = start;
            } else {
                for (int num = 0; num < cn; num++) { loop.push_back(-end); loop.push_back(-start); loop.push_back(start); loop.push_back(end); }
                bkp[temp] = end;
                if (temp + 1 != bkp.size()) bkp[temp + 1] = -end;
            }
            bkp.insert(bkp.begin() + (long)temp + 1, loop.begin(), loop.end());
        }
    }
    *L_out = (int)bkp.size();
    return (int)i;
}

// imperfectFBI.  false: the reference would have touched a cell behind the end.
static bool ref_fbi(Cells& b, const Inv& inv) {
    const long L = (long)b.size();
    auto has = [&](int id) { return inv.src[(size_t)id] != 0; };
    long pos = 0;
    while (pos < L) {
        if (pos + 1 >= L) return false;
        long r = L;
        for (long q = pos + 3; q < L; q++) if (b[(size_t)q] == -b[(size_t)pos]) { r = q; break; }
        const long l = r - 1;
        if (r == L || b[(size_t)l] != -b[(size_t)pos + 1]) {
            int id = std::abs(b[(size_t)pos + 1]);
            if (has(id)) {
                const int s = inv.src[(size_t)id], t = inv.tgt[(size_t)id];
                if (b[(size_t)pos + 1] > 0) b[(size_t)pos + 1] = s < t ? s : t;
                else b[(size_t)pos + 1] = s < t ? -t : -s;
            }
            if (pos > 0) {
                id = std::abs(b[(size_t)pos]);
                if (has(id) && std::abs(b[(size_t)pos - 1]) == id) {
                    const int s = inv.src[(size_t)id], t = inv.tgt[(size_t)id];
                    const int other = s == id ? t : s;
                    b[(size_t)pos] = b[(size_t)pos] > 0 ? other : -other;
                }
            }
            if (b[(size_t)pos] > 0 && std::abs(b[(size_t)pos]) > std::abs(b[(size_t)pos + 1])) b[(size_t)pos + 1] = b[(size_t)pos];
            if (b[(size_t)pos] < 0 && std::abs(b[(size_t)pos]) < std::abs(b[(size_t)pos + 1])) b[(size_t)pos + 1] = b[(size_t)pos];
            pos += 2;
        } else {
            long p1 = pos + (l - pos) / 2, p2 = p1 + 1;
            while (p1 >= pos - 1 && p1 > 0) {
                const int id = std::abs(b[(size_t)p1]);
                if (has(id)) {
                    const int s = inv.src[(size_t)id], t = inv.tgt[(size_t)id];
                    if (p1 + 1 >= L) return false;
                    if (b[(size_t)p1] > 0) {
                        if (s < t) { b[(size_t)p1] = s; b[(size_t)p1 + 1] = -t; } else { b[(size_t)p1] = t; b[(size_t)p1 + 1] = -s; }
                    } else {
                        if (s < t) { b[(size_t)p1] = -t; b[(size_t)p1 + 1] = s; } else { b[(size_t)p1] = -s; b[(size_t)p1 + 1] = t; }
                    }
                    if (p2 != p1 + 1) {
                        if (p1 > pos - 1) { if (p2 >= L) return false; b[(size_t)p2] = -b[(size_t)p1]; }
                        b[(size_t)p2 - 1] = -b[(size_t)p1 + 1];
                    }
                }
                p1 -= 2; p2 += 2;
            }
            pos = r + 1;
        }
    }
    return true;
}

static Cells ref_expand(const Cells& bkp) {
    Cells path;
    for (size_t j = 1; j < bkp.size(); j += 2) {
        if (bkp[j - 1] > 0) { for (int k = bkp[j - 1]; k <= std::abs(bkp[j]); k++) path.push_back(k); }
        else { for (int k = -bkp[j - 1]; k >= std::abs(bkp[j]); k--) path.push_back(-k); }
    }
    return path;
}

// ---- inputs ----------------------------------------------------------------------------------------------------------------
static void random_dag(Dag& D, int n, int K, int max_cn) {
    memset(&D, 0, sizeof(D));
    D.K = K;
    for (int i = 0; i < K; i++) {
        const uint32_t kind = rnd() % 16;
        const int a = rnd_in(1, n - 1), b = rnd_in(a + 1, n);
        if (kind == 0 && (i > 0 || rnd() % 4 == 0)) continue;               // both slots empty: nothing is placed, the loop goes on (the first: the reference indexes an empty vector)
        if (kind <= 3) { D.pat[i][0] = a; D.pat[i][1] = b; D.pat[i][2] = 1; }
        else { D.loop[i][0] = a; D.loop[i][1] = b; D.loop[i][2] = (rnd() % 8 == 0) ? rnd_in(1, max_cn) : rnd_in(1, 4); }
    }
}
// a nest: every element shares an end with an earlier one, so that most of them find a slot
static void nested_dag(Dag& D, int n, int K, int max_cn) {
    memset(&D, 0, sizeof(D));
    D.K = K;
    int a = 1, b = n;
    for (int i = 0; i < K; i++) {
        if (i > 0 && rnd() % 6 == 0) { D.pat[i][0] = 1; D.pat[i][1] = rnd_in(2, n); D.pat[i][2] = 1; continue; }
        D.loop[i][0] = a; D.loop[i][1] = b; D.loop[i][2] = (rnd() % 4 == 0) ? rnd_in(1, max_cn) : rnd_in(1, 3);
        const uint32_t mv = rnd() % 4;
        if (mv == 0 && a + 1 < b) a++;
        else if (mv == 1 && a + 1 < b) b--;
        else if (mv == 2) { a = 1; b = n - rnd_in(0, 2); }
    }
}
static Inv random_inv(int n, int density_pct) {
    Inv v;
    v.src.assign((size_t)n + 1, 0); v.tgt.assign((size_t)n + 1, 0);
    for (int i = 1; i <= n; i++) {
        if ((int)(rnd() % 100) >= density_pct) continue;
        int j = i + rnd_in(-2, 2);
        if (j < 1 || j > n) j = i;
        const bool swap = rnd() & 1;
        const int s = swap ? j : i, t = swap ? i : j;
        // the junction enters the map at both of its segments that have no entry yet (LGM.cpp:4014-4048)
        if (v.src[(size_t)i] == 0) { v.src[(size_t)i] = s; v.tgt[(size_t)i] = t; }
        if (v.src[(size_t)j] == 0) { v.src[(size_t)j] = s; v.tgt[(size_t)j] = t; }
    }
    return v;
}

struct InvBlocks {      // the map as the stages read it: blocks of exactly n + 1 entries
    std::unique_ptr<int16_t[]> src, tgt;
    InvBlocks(const Inv& v) : src(new int16_t[v.src.size()]), tgt(new int16_t[v.tgt.size()]) {
        for (size_t i = 0; i < v.src.size(); i++) { src[i] = (int16_t)v.src[i]; tgt[i] = (int16_t)v.tgt[i]; }
    }
    InvMap get() const { return InvMap{src.get(), tgt.get()}; }
};

// ---- one case through the three forms --------------------------------------------------------------------------------------
static void check_eval(const Dag& D, const Inv& inv, bool forward, int cap, int want_rc, int want_L, const Cells& want_placed, bool want_ok, const Cells& want_cells) {
    HostGroup g;
    const int K = D.K;
    std::vector<uint8_t> ord((size_t)K);
    for (int i = 0; i < K; i++) ord[(size_t)i] = (uint8_t)i;
    const InvBlocks IB(inv);
    const int want_verdict = want_rc < 0 ? want_rc : (!want_ok && want_rc == K) ? (int)ST_ERR_REF_UB : (want_rc == K ? 1 : 0);
    {   // the wavefront form in group memory
        std::unique_ptr<cell_t[]> cells(new cell_t[(size_t)std::max(cap, 1)]);
        int L = -1;
        const int rc = eval_place(g, D, ord.data(), forward, cells.get(), cap, &L);
        CHECK(rc == want_rc && L == want_L);
        if (rc >= 0) {
            bool eq = L == (int)want_placed.size();
            for (int i = 0; eq && i < L; i++) eq = cells[(size_t)i] == want_placed[(size_t)i];
            CHECK(eq);
            const int verdict = eval_finish(g, rc, K, cells.get(), L, IB.get());
            CHECK(verdict == want_verdict);
            if (want_ok) {
                eq = true;
                for (int i = 0; eq && i < L; i++) eq = cells[(size_t)i] == want_cells[(size_t)i];
                CHECK(eq);
            }
        }
    }
    for (int stride : {1, 64}) {   // one thread per order: the lane's cells `stride` apart, the lane the last of its block
        const size_t total = (size_t)std::max(cap, 1) * (size_t)stride;
        std::unique_ptr<cell_t[]> block(new cell_t[total]);
        memset(block.get(), 0x11, total * sizeof(cell_t));
        std::vector<uint8_t> ords((size_t)K * (size_t)stride, 0xff);
        for (int i = 0; i < K; i++) ords[(size_t)i * (size_t)stride + (size_t)(stride - 1)] = (uint8_t)i;
        const LaneCells lc{block.get() + (stride - 1), stride};
        int L = -1;
        const int verdict = eval_order_lane(D, ords.data() + (stride - 1), stride, forward, IB.get(), lc, cap, &L);
        CHECK(verdict == want_verdict);
        if (want_rc >= 0) CHECK(L == want_L);
        if (want_rc >= 0 && want_ok) {
            bool eq = true;
            for (int i = 0; eq && i < L; i++) eq = lc.get(i) == want_cells[(size_t)i];
            CHECK(eq);
        }
        if (stride == 64) {          // the other lanes' cells are as they were
            bool clean = true;
            for (size_t i = 0; clean && i < total; i++) if (i % 64 != 63) clean = block[i] == (cell_t)0x1111;
            CHECK(clean);
        }
    }
}

static void eval_case(const Dag& D, int n, bool forward, int density_pct) {
    std::vector<int> order;
    for (int i = 0; i < D.K; i++) order.push_back(i);
    const Inv inv = random_inv(n, density_pct);
    Cells placed;
    int L = 0, need = 0;
    const int rc = ref_place(D, order, forward, INT_MAX, placed, &L, &need);
    if (rc == ST_ERR_REF_UB) { check_eval(D, inv, forward, 8, rc, 0, placed, false, placed); n_ub++; return; }
    Cells cells = placed;
    const bool ok = ref_fbi(cells, inv);
    n_valid += ok && rc == D.K; n_broke += rc < D.K; n_ub += !ok; n_rewritten += ok && cells != placed;
    check_eval(D, inv, forward, need, rc, L, placed, ok, cells);                    // the capacity met exactly
    check_eval(D, inv, forward, need + rnd_in(1, 9), rc, L, placed, ok, cells);
    {   // one cell short: the step that asks for the missing cell ends the evaluation
        Cells p2;
        int L2 = 0, need2 = 0;
        const int rc2 = ref_place(D, order, forward, need - 1, p2, &L2, &need2);
        CHECK(rc2 == ST_ERR_BKP_CAPACITY);
        check_eval(D, inv, forward, need - 1, rc2, L2, p2, false, p2);
        n_capacity++;
    }
    if (ok && !cells.empty()) {   // expand_bkp at the exact path capacity, one short of it, and with room
        HostGroup g;
        const Cells want = ref_expand(cells);
        const int Lc = (int)cells.size(), P = (int)want.size();
        std::unique_ptr<cell_t[]> b(new cell_t[(size_t)Lc]);
        for (int i = 0; i < Lc; i++) b[(size_t)i] = (cell_t)cells[(size_t)i];
        for (int pcap : {P, P - 1, P + 3}) {
            if (pcap < 0) continue;
            std::unique_ptr<cell_t[]> path(new cell_t[(size_t)std::max(pcap, 1)]);
            std::unique_ptr<int32_t[]> offs(new int32_t[(size_t)(Lc / 2 + 1)]);
            const int got = expand_bkp(g, b.get(), Lc, path.get(), pcap, offs.get());
            if (pcap < P) { CHECK(got == ST_ERR_PATH_CAPACITY); continue; }
            bool eq = got == P;
            for (int i = 0; eq && i < P; i++) eq = path[(size_t)i] == want[(size_t)i];
            CHECK(eq);
        }
    }
}

static void shift_case() {
    HostGroup g;
    const int L = rnd_in(0, 700), at = rnd_in(0, L), count = rnd_in(0, 300);
    Cells v((size_t)L);
    for (int& x : v) x = rnd_in(-3000, 3000);
    {   // shift_up: a block of exactly L + count cells
        std::unique_ptr<cell_t[]> a(new cell_t[(size_t)std::max(L + count, 1)]);
        for (int i = 0; i < L; i++) a[(size_t)i] = (cell_t)v[(size_t)i];
        shift_up(g, a.get(), L, at, count);
        bool eq = true;
        for (int i = 0; eq && i < at; i++) eq = a[(size_t)i] == v[(size_t)i];
        for (int i = at; eq && i < L; i++) eq = a[(size_t)(i + count)] == v[(size_t)i];
        CHECK(eq);
    }
    if (at + count <= L) {   // shift_down: a block of exactly L cells
        std::unique_ptr<cell_t[]> a(new cell_t[(size_t)std::max(L, 1)]);
        for (int i = 0; i < L; i++) a[(size_t)i] = (cell_t)v[(size_t)i];
        shift_down(g, a.get(), L, at, count);
        bool eq = true;
        for (int i = 0; eq && i < at; i++) eq = a[(size_t)i] == v[(size_t)i];
        for (int i = at + count; eq && i < L; i++) eq = a[(size_t)(i - count)] == v[(size_t)i];
        CHECK(eq);
    }
}

int main() {
    static Dag D;
    for (g_case = 0; g_case < 2500; g_case++) {
        const int n = rnd_in(3, 12), K = rnd_in(1, 10);
        if (g_case % 2) nested_dag(D, n, K, g_case % 10 == 1 ? 70 : 20); else random_dag(D, n, K, 40);
        eval_case(D, n, (g_case >> 1) & 1, (int)(rnd() % 4) * 30);
    }
    for (g_case = 10000; g_case < 10400; g_case++) shift_case();
    printf("cases: %ld valid, %ld broke off, %ld undefined in the reference, %ld one cell short, %ld rewritten by imperfectFBI, %ld nesting skips, %ld inserts of 64 cells and more\n",
           n_valid, n_broke, n_ub, n_capacity, n_rewritten, n_nest_skips, n_big_inserts);
    if (n_valid < 200 || n_broke < 200 || n_ub < 10 || n_rewritten < 200 || n_nest_skips < 100 || n_big_inserts < 50) { printf("FAIL: the cases do not reach what they are meant to\n"); fails++; }
    if (fails) { printf("eval_stage_check: %d FAILED\n", fails); return 1; }
    printf("eval_stage_check: ok\n");
    return 0;
}
