// tests/tools/wide_stage_check.cpp -- stand-alone check of the wide front (ambi_wide.hpp: construct_dag_wide, lattice_wide,
// unrank_wide; ambi_stages.hpp: write_wide_row) on the CPU with the one-thread HostGroup, for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wno-unknown-pragmas
//       -I ambigram_amd/csrc tests/tools/wide_stage_check.cpp -o wide_stage_check && ./wide_stage_check
// Inputs: dense random element sets with 64..255 elements (ends drawn from few shared points, loop shares 0 / 0.3 / 0.7 / 1, the
// absolute ids straddling 10 / 100 / 1000), nested chains with a few extras and patterns (lattices that are built), and the units at
// the capacities: 4095 / 4096 / 4097 / 4160 order ideals, 2^20 and more orders (counted), tables of 10^5 rows (written).
// What the stages leave is compared with a std::map / std::vector / std::set transcription, written here, of constructDAG
// (LGM.cpp:3276-3378: the keys of a std::map<std::string, int>, the library's own std::sort with compareLoops, the four edge
// rules with their parent lists) and with a plain recursive count of the completions of every order ideal; the rows with an
// unranking from that count and, for small tables, with a listing of all orders by the textbook recursion (LGM.cpp:3380-3409).
// WideUnit, the elements and the rows live in heap blocks of exactly their size, so that a read or write past one is the
// sanitizer's to report.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "ambi_stages.hpp"

using namespace ambi;

static int fails = 0, g_case = 0;
#define CHECK(x) do { if (!(x)) { if (fails < 20) printf("FAIL %s:%d: %s (case %d)\n", __FILE__, __LINE__, #x, g_case); fails++; } } while (0)
static long n_units = 0, n_refused = 0, n_over = 0, n_built = 0, n_cyclic = 0, n_rows = 0, n_listed = 0, n_inherited = 0, n_self = 0, n_too_many = 0;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 11); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }   // inclusive
static bool rnd_p(double p) { return (rnd() & 0xFFFFFF) < p * 0x1000000; }

// ---- the transcription -----------------------------------------------------------------------------------------------------
struct RefDag {
    int K = 0;
    std::vector<std::vector<int>> pat, loop;
    std::vector<std::set<int>> adj;
};

static bool ref_compare_loops(std::vector<int> a, std::vector<int> b) {
    int d1 = 0, d2 = 0;
    if (a.size() > 0 && b.size() > 0) { d1 = std::abs(a[0] - a[1]); d2 = std::abs(b[0] - b[1]); }
    return d1 > d2;
}

// The records hold LOCAL segment ids (as the engine's), the keys the absolute ones: only the key order depends on them.
static RefDag ref_construct(const std::vector<Element>& els, int seg_base) {
    std::map<std::string, Element> vars;
    for (const Element& e : els) vars[std::string(e.is_loop ? "l:" : "p:") + std::to_string(e.a + seg_base) + "," + std::to_string(e.b + seg_base)] = e;
    RefDag D;
    std::vector<std::vector<int>> adj, parents;
    for (const auto& kv : vars) {
        const Element& e = kv.second;
        adj.push_back({}); parents.push_back({});
        const std::vector<int> rec{e.a, e.b, e.cn};
        if (!e.is_loop) { D.pat.push_back(rec); D.loop.push_back({}); }
        else { D.loop.push_back(rec); D.pat.push_back({}); }
    }
    const int K = D.K = (int)adj.size();
    std::sort(D.loop.begin(), D.loop.end(), ref_compare_loops);      // the library's own algorithm: the comparator is no strict weak order
    auto has = [](const std::vector<int>& v, int x) { return std::find(v.begin(), v.end(), x) != v.end(); };
    auto len = [](const std::vector<int>& r) { return std::abs(r[0] - r[1]); };
    auto meet = [](const std::vector<int>& x, const std::vector<int>& y) { return x[0] == y[0] || x[1] == y[1]; };
    for (int i = 0; i < K; i++) {
        if (D.pat[i].empty()) continue;
        for (int j = 0; j < K; j++)
            if (!D.pat[j].empty() && meet(D.pat[i], D.pat[j]) && len(D.pat[i]) > len(D.pat[j])) { adj[i].push_back(j); parents[j].push_back(i); }
        for (int j = 0; j < K; j++)
            if (!D.loop[j].empty() && meet(D.pat[i], D.loop[j]) && len(D.pat[i]) > len(D.loop[j])) { adj[i].push_back(j); parents[j].push_back(i); }
    }
    for (int i = 0; i < K; i++) {
        if (D.loop[i].empty()) continue;
        for (int j = 0; j < K; j++) {
            if (has(parents[i], j)) continue;
            if (D.pat[j].empty() || !meet(D.loop[i], D.pat[j])) continue;
            if (len(D.loop[i]) > len(D.pat[j])) { adj[i].push_back(j); parents[j].push_back(i); }
            else {
                const std::vector<int> mine = parents[i];      // (a copy: the list itself may grow by i when j == i)
                for (int parent : mine)
                    if (has(adj[parent], j)) { adj[i].push_back(j); parents[j].push_back(i); n_inherited++; break; }
            }
        }
        for (int j = 0; j < K; j++)
            if (!D.loop[j].empty() && meet(D.loop[i], D.loop[j]) && len(D.loop[i]) > len(D.loop[j])) { adj[i].push_back(j); parents[j].push_back(i); }
    }
    D.adj.resize(K);
    for (int i = 0; i < K; i++) { D.adj[i].insert(adj[i].begin(), adj[i].end()); if (D.adj[i].count(i)) n_self++; }
    return D;
}

struct Set4 {
    uint64_t w[4] = {0, 0, 0, 0};
    bool operator<(const Set4& o) const { return std::lexicographical_compare(w, w + 4, o.w, o.w + 4); }
    bool has(int v) const { return (w[v >> 6] >> (v & 63)) & 1; }
    Set4 with(int v) const { Set4 s = *this; s.w[v >> 6] |= 1ull << (v & 63); return s; }
    bool holds(const Set4& o) const { for (int k = 0; k < 4; k++) if (o.w[k] & ~w[k]) return false; return true; }
};

struct RefLattice {
    int K;
    std::vector<Set4> pred;
    std::map<Set4, uint64_t> memo;
    explicit RefLattice(const RefDag& D) : K(D.K), pred((size_t)D.K) {
        for (int i = 0; i < K; i++) for (int j : D.adj[i]) pred[(size_t)j] = pred[(size_t)j].with(i);
    }
    std::vector<int> free_nodes(const Set4& I) const {
        std::vector<int> out;
        for (int v = 0; v < K; v++) if (!I.has(v) && I.holds(pred[(size_t)v])) out.push_back(v);
        return out;
    }
    // reachable ideals and child links, the walk given up beyond `limit` ideals
    bool sizes(long limit, long* ideals, long* links) const {
        std::set<Set4> seen{Set4()};
        std::vector<Set4> todo{Set4()};
        *links = 0;
        while (!todo.empty()) {
            const Set4 I = todo.back(); todo.pop_back();
            for (int v : free_nodes(I)) {
                ++*links;
                if (seen.insert(I.with(v)).second) { if ((long)seen.size() > limit) return false; todo.push_back(I.with(v)); }
            }
        }
        *ideals = (long)seen.size();
        return true;
    }
    int size_of(const Set4& I) const { int c = 0; for (int k = 0; k < 4; k++) c += __builtin_popcountll(I.w[k]); return c; }
    uint64_t count(const Set4& I) {
        if (size_of(I) == K) return 1;
        auto it = memo.find(I);
        if (it != memo.end()) return it->second;
        uint64_t c = 0;
        for (int v : free_nodes(I)) { c += count(I.with(v)); if (c > kCountSat) c = kCountSat; }
        return memo[I] = c;
    }
    std::vector<uint8_t> unrank(uint64_t r) {
        std::vector<uint8_t> row;
        Set4 I;
        for (int d = 0; d < K; d++)
            for (int v : free_nodes(I)) {
                const uint64_t c = count(I.with(v));
                if (r < c) { row.push_back((uint8_t)v); I = I.with(v); break; }
                r -= c;
            }
        return row;
    }
    // every order, lowest node first (the recursion of allTopologicalOrders), up to `cap` of them
    void list(std::vector<int>& indeg, std::vector<char>& used, std::vector<uint8_t>& cur, const RefDag& D, std::vector<std::vector<uint8_t>>& out, size_t cap) {
        if (out.size() >= cap) return;
        if ((int)cur.size() == K) { out.push_back(cur); return; }
        for (int v = 0; v < K; v++) {
            if (used[(size_t)v] || indeg[(size_t)v] != 0) continue;
            used[(size_t)v] = 1; cur.push_back((uint8_t)v);
            for (int j : D.adj[(size_t)v]) indeg[(size_t)j]--;
            list(indeg, used, cur, D, out, cap);
            for (int j : D.adj[(size_t)v]) indeg[(size_t)j]++;
            used[(size_t)v] = 0; cur.pop_back();
        }
    }
};

// ---- one unit through the stages ----------------------------------------------------------------------------------------------
constexpr uint64_t kRowsWritten = 20000, kRowsUnranked = 600, kRowsListed = 1500;   // per unit: rows written (unless asked for all), compared with the reference's unranking, with the listing

static void check_unit(const std::vector<Element>& els_in, int seg_base, long want_ideals = -1, int64_t want_R = -1, bool write_all = false, long want_links = -1) {
    g_case++; n_units++;
    const int K = (int)els_in.size();
    std::unique_ptr<Element[]> el(new Element[(size_t)K]);                       // exactly K elements
    std::copy(els_in.begin(), els_in.end(), el.get());
    std::unique_ptr<WideUnit> X(new WideUnit);                                    // exactly one working set
    std::memset(static_cast<void*>(X.get()), 0xA5, sizeof(WideUnit));            // (the stage must not rely on what it finds)
    HostGroup g;
    const int st = construct_dag_wide(g, el.get(), K, seg_base, *X);
    if (K > kMaxNodesWide) { CHECK(st == ST_ERR_TOO_MANY_NODES); n_too_many++; return; }
    if (st == ST_ERR_REF_UB) { n_refused++; return; }                             // the library's sort would leave its range: not asked of the real one
    CHECK(st == ST_OK);
    if (st != ST_OK) return;
    const RefDag D = ref_construct(els_in, seg_base);
    CHECK(D.K == K && X->dag.K == K);
    bool same = true;
    for (int i = 0; i < K; i++) {
        const std::vector<int> zero{0, 0, 0};
        const std::vector<int>& p = D.pat[(size_t)i].empty() ? zero : D.pat[(size_t)i];
        const std::vector<int>& l = D.loop[(size_t)i].empty() ? zero : D.loop[(size_t)i];
        for (int c = 0; c < 3; c++) same = same && X->dag.pat[i][c] == p[(size_t)c] && X->dag.loop[i][c] == l[(size_t)c];
        for (int j = 0; j < kWideNodeCap; j++) {
            const bool e = j < K && D.adj[(size_t)i].count(j) != 0;
            same = same && wset_has(X->succ[i], j) == e && (j >= K || wset_has(X->pred[j], i) == e);
        }
    }
    CHECK(same);
    if (!same) return;
    RefLattice L(D);
    long ideals = 0, links = 0;
    const bool fits = L.sizes(kWideIdealCap, &ideals, &links) && links <= kWideLinkCap;
    uint64_t R = 12345;
    const int ls = lattice_wide(g, *X, &R);
    if (want_ideals >= 0) CHECK(want_ideals > kWideIdealCap ? !fits : ideals == want_ideals);
    if (want_links >= 0) CHECK(links == want_links && (links > kWideLinkCap) == !fits);
    if (!fits) { CHECK(ls == ST_ERR_IDEALS_CAPACITY); n_over++; return; }
    CHECK(ls == ST_OK && X->nI == ideals && X->nC == links);
    if (ls != ST_OK) return;
    n_built++;
    const uint64_t want = L.count(Set4());
    CHECK(R == want);
    if (want_R >= 0) CHECK(want == (uint64_t)want_R);
    if (want == 0) n_cyclic++;
    if (R != want || R == 0 || R > (write_all ? (uint64_t)kWideMaxOrders : kRowsWritten)) return;
    // the table: every row written into a block of exactly R rows
    const int stride = row_stride(K);
    CHECK(stride == (K <= 127 ? 128 : 256));
    std::unique_ptr<uint8_t[]> rows(new uint8_t[(size_t)R * (size_t)stride]);
    for (uint64_t r = 0; r < R; r++) write_wide_row(*X, (int64_t)r, K, rows.get());
    n_rows += (long)R;
    const uint64_t step = R <= kRowsUnranked ? 1 : R / kRowsUnranked;
    bool rows_ok = true;
    for (uint64_t r = 0; r < R; r += step) {
        const std::vector<uint8_t> w = L.unrank(r);
        rows_ok = rows_ok && (int)w.size() == K && std::memcmp(w.data(), rows.get() + r * stride, (size_t)K) == 0;
        for (int d = K; d < stride; d++) rows_ok = rows_ok && rows[r * stride + d] == 0xFF;
    }
    for (uint64_t r = 1; r < R; r++) rows_ok = rows_ok && std::memcmp(rows.get() + (r - 1) * stride, rows.get() + r * stride, (size_t)K) < 0;
    {   // the last row through unrank_wide itself, into a block of exactly K bytes
        std::unique_ptr<uint8_t[]> one(new uint8_t[(size_t)K]);
        unrank_wide(*X, R - 1, one.get());
        rows_ok = rows_ok && std::memcmp(one.get(), rows.get() + (R - 1) * stride, (size_t)K) == 0;
    }
    CHECK(rows_ok);
    if (R <= kRowsListed) {
        std::vector<int> indeg((size_t)K, 0);
        for (int i = 0; i < K; i++) for (int j : D.adj[(size_t)i]) indeg[(size_t)j]++;
        std::vector<char> used((size_t)K, 0);
        std::vector<uint8_t> cur;
        std::vector<std::vector<uint8_t>> all;
        L.list(indeg, used, cur, D, all, kRowsListed + 1);
        bool listed = all.size() == R;
        for (uint64_t r = 0; listed && r < R; r++) listed = std::memcmp(all[(size_t)r].data(), rows.get() + r * stride, (size_t)K) == 0;
        CHECK(listed);
        n_listed++;
    }
}

// ---- inputs ----------------------------------------------------------------------------------------------------------------------
static std::vector<Element> dense_set(int n, int K, double share) {
    std::vector<int> pts{1, n};
    for (int i = 0; i < 2 + K / 8; i++) pts.push_back(rnd_in(2, n - 1));
    std::set<std::vector<int>> have;
    std::vector<Element> els;
    while ((int)els.size() < K) {
        int a = rnd_p(0.1) ? rnd_in(1, n) : pts[(size_t)rnd_in(0, (int)pts.size() - 1)], b = rnd_p(0.1) ? rnd_in(1, n) : pts[(size_t)rnd_in(0, (int)pts.size() - 1)];
        if (a > b) std::swap(a, b);
        const int is_loop = rnd_p(share) ? 1 : 0;
        if (have.insert({is_loop, a, b}).second) els.push_back(Element{is_loop, a, b, rnd_in(1, 2)});
    }
    for (size_t i = els.size(); i > 1; i--) std::swap(els[i - 1], els[(size_t)rnd_in(0, (int)i - 1)]);
    return els;
}

static std::vector<Element> chains(const std::vector<int>& lengths) {
    std::vector<Element> els;
    int lo = 1;
    for (int L : lengths) { std::vector<Element> c; int a = lo, b = lo + L - 1; for (int k = 0; k < L; k++) { c.push_back(Element{1, a, b, 1}); if (rnd_p(0.5)) a++; else b--; } els.insert(els.end(), c.begin(), c.end()); lo += L + 1; }
    return els;
}

static std::vector<Element> backbone(int L, int m, int n_pat) {
    std::vector<Element> els;
    const int lo = 2 + 2 * m, hi = lo + L - 1;
    {
        int a = lo, b = hi;
        for (int k = 0; k < L; k++) { els.push_back(Element{1, a, b, rnd_in(1, 2)}); if (rnd_p(0.5)) a++; else b--; }
    }
    std::set<std::pair<int, int>> have;
    for (const Element& e : els) have.insert({e.a, e.b});
    int left = lo - 2, right = hi + 2;
    while ((int)els.size() < L + m) {
        int a, b;
        const int kind = rnd_in(0, 3);
        if (kind >= 2) { if (rnd_p(0.5)) { a = b = left; left -= 2; } else { a = b = right; right += 2; } }
        else {
            const Element& mem = els[(size_t)rnd_in(0, L - 1)];
            if (kind == 0) { a = mem.a; b = rnd_in(mem.a, hi); } else { a = rnd_in(lo, mem.b); b = mem.b; }
        }
        if (have.insert({a, b}).second) els.push_back(Element{1, a, b, 1});
    }
    for (int k = 0; k < n_pat; k++) els[(size_t)(rnd_p(0.6) ? rnd_in(L, L + m - 1) : rnd_in(0, L + m - 1))].is_loop = 0;
    return els;
}

static std::vector<Element> vee(int a, int b) {
    const int N = a + b + 2;
    std::vector<Element> els{Element{1, 1, N, 1}};
    for (int k = 1; k <= a; k++) els.push_back(Element{1, 1, N - k, 1});
    for (int k = 1; k <= b; k++) els.push_back(Element{1, 1 + k, N, 1});
    return els;
}

static std::vector<Element> diamonds(int d, int c) {
    const int N = 2 * d + 2 + c;
    std::set<std::pair<int, int>> s;
    for (int i = 1; i <= d; i++) { s.insert({i, N + 1 - i}); s.insert({i, N - i}); s.insert({i + 1, N + 1 - i}); s.insert({i + 1, N - i}); }
    for (int k = 1; k <= c; k++) s.insert({d + 1, N - d - k});
    std::vector<Element> els;
    for (const auto& p : s) els.push_back(Element{1, p.first, p.second, 1});
    return els;
}

// a binary tree of loops over `leaves` segments, a chain of c loops around its root, m free loops
static void tree_of(std::vector<Element>& els, int a, int b) {
    els.push_back(Element{1, a, b, 1});
    if (b > a) { tree_of(els, a, (a + b) / 2); tree_of(els, (a + b) / 2 + 1, b); }
}
static std::vector<Element> tree_unit(int leaves, int c, int m) {
    const int lo = c + 2, hi = lo + leaves - 1;
    std::vector<Element> t, els;
    tree_of(t, lo, hi);
    std::set<std::pair<int, int>> have;
    for (const Element& e : t) if (have.insert({e.a, e.b}).second) els.push_back(e);
    for (int k = 1; k <= c; k++) els.push_back(Element{1, lo - k, hi, 1});
    for (int k = 0; k < m; k++) els.push_back(Element{1, hi + 2 + 2 * k, hi + 2 + 2 * k, 1});
    return els;
}

int main() {
    const auto t0 = std::chrono::steady_clock::now();
    const int Ks[] = {64, 65, 96, 100, 127, 128, 129, 160, 192, 200, 254, 255}, ns[] = {30, 45, 60, 90}, bases[] = {0, 5, 95, 990};
    const double shares[] = {0.0, 0.3, 0.7, 1.0};
    for (int t = 0; t < 240; t++)
        check_unit(dense_set(ns[t % 4], Ks[(t / 4) % 12], shares[(t / 48) % 4]), bases[(t / 7) % 4]);
    const long dense_refused = n_refused, dense_units = n_units;
    const auto t1 = std::chrono::steady_clock::now();
    for (int t = 0; t < 160; t++) {
        const int L = rnd_in(60, 250), m = std::max(std::min(t % 4 == 1 ? 1 : t % 4 == 3 ? 2 : rnd_in(2, 4), 255 - L), 64 - L);
        check_unit(backbone(L, m, t % 3 == 0 ? 0 : rnd_in(1, 3)), bases[t % 4]);
    }
    const auto t2 = std::chrono::steady_clock::now();
    // the capacities
    check_unit(chains({60, 4, 4, 1}), 0, 61 * 50);
    check_unit(chains({62, 64}), 0, 4095);
    check_unit(chains({63, 1, 1, 1, 1, 1, 1}), 3, 4096);
    check_unit(chains({127, 1, 1, 1, 1, 1}), 0, 4096);
    check_unit(vee(62, 64), 0, 4096);
    check_unit(vee(63, 63), 0, 4097);
    check_unit(vee(31, 127), 7, 4097);
    check_unit(chains({64, 1, 1, 1, 1, 1, 1}), 0, 4160);
    check_unit(chains({81, 4, 4, 1}), 0, 4100);
    check_unit(tree_unit(2, 59, 6), 0, 4096, -1, false, 16384);        // exactly kWideLinkCap links at 4096 ideals: built
    check_unit(tree_unit(3, 53, 6), 0, 4096, -1, false, 16704);        // 16704 links at 4096 ideals: refused by the link cap
    check_unit(chains({100, 1, 1, 1}), 0, -1, 101 * 102 * 103);        // one step past the row cap: counted, not written
    check_unit(chains({90, 3}), 0, -1, 129766, true);                   // written: 129 766 rows of 128 bytes
    check_unit(diamonds(20, 10), 0, -1, 1 << 20);                       // exactly the row cap: counted (the cap itself is stage_prepare_wide's)
    check_unit(diamonds(16, 111), 0, -1, 1 << 16, true);                // written: 65 536 rows of 256 bytes
    {
        std::vector<Element> big = chains({200, 56});                   // 256 elements
        check_unit(big, 0);
    }
    const auto t3 = std::chrono::steady_clock::now();
    auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    printf("seconds: dense sets %.1f, chains with extras %.1f, capacities %.1f\n", secs(t0, t1), secs(t1, t2), secs(t2, t3));
    printf("units %ld (dense %ld, refused there %ld), refused %ld, over capacity %ld, built %ld (cyclic %ld), rows written %ld, tables listed %ld, "
           "inherited edges %ld, self edges %ld, too many nodes %ld\n",
           n_units, dense_units, dense_refused, n_refused, n_over, n_built, n_cyclic, n_rows, n_listed, n_inherited, n_self, n_too_many);
    CHECK(n_refused * 50 <= n_units);                                  // at most 2 % of the inputs may go unasked
    CHECK(n_over >= 200 && n_built >= 100 && n_cyclic >= 3 && n_listed >= 20 && n_inherited >= 100 && n_too_many == 1 && n_rows > 250000);
    if (fails) { printf("wide_stage_check: %d FAILED\n", fails); return 1; }
    printf("wide_stage_check: ok\n");
    return 0;
}
