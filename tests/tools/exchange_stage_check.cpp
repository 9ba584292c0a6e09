// tests/tools/exchange_stage_check.cpp -- stand-alone check of the exchange stages (ambi_exchange.hpp) on the CPU with the
// one-thread HostGroup, for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Wno-unknown-pragmas -I ambigram_amd/csrc
//       tests/tools/exchange_stage_check.cpp -o exchange_stage_check && ./exchange_stage_check
// Hand-made result blobs and headers go through the very functions the kernels and the host simulation call; what they leave
// is compared with plain loops written here.  Every output buffer has exactly the capacity handed to the stage, so a write at
// or past the capacity is the sanitizer's to report.
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "ambi_exchange.hpp"

using namespace ambi;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); fails++; } } while (0)

static const int32_t SENT = -0x5a5a5a5a;
typedef std::vector<std::pair<int, int>> Runs;   // {first cell (local signed id), cells}

// a batch of units with the given paths (getBFB's; `edited[u]` non-empty: the path after indelBFB is stored and differs)
struct Blob {
    std::vector<UnitIn> units;
    std::vector<uint64_t> mem;   // (8-byte aligned)
    std::vector<std::vector<int>> path[2];
    BatchArgs A{};
    Blob(const std::vector<std::vector<int>>& paths, const std::vector<std::vector<int>>& edited, const std::vector<int>& seg_base) {
        const size_t U = paths.size();
        int64_t o = (int64_t)sizeof(UnitOut) * (int64_t)U;
        for (size_t u = 0; u < U; u++) {
            UnitIn in{};
            in.n_seg = 3; in.seg_base = seg_base[u]; in.bkp_cap = 2; in.out_cap = 1;
            in.path_cap = (int)(paths[u].size() > edited[u].size() ? paths[u].size() : edited[u].size());
            in.res_off = o;
            o += unit_layout(in.n_seg, in.bkp_cap, in.path_cap, in.out_cap).total;
            units.push_back(in);
        }
        mem.assign((size_t)(o + 7) / 8, 0);
        uint8_t* res = reinterpret_cast<uint8_t*>(mem.data());
        for (size_t u = 0; u < U; u++) {
            const UnitIn& in = units[u];
            const UnitLayout L = unit_layout(in.n_seg, in.bkp_cap, in.path_cap, in.out_cap);
            UnitOut* h = unit_out(res, (int)u);
            const bool stored = !edited[u].empty();
            h->path_len = (int)paths[u].size(); h->path_ind_stored = stored; h->path_indel_len = (int)(stored ? edited[u].size() : paths[u].size());
            rcell_t* p = reinterpret_cast<rcell_t*>(res + in.res_off + L.path);
            rcell_t* q = reinterpret_cast<rcell_t*>(res + in.res_off + L.path_ind);
            for (size_t i = 0; i < paths[u].size(); i++) p[i] = (rcell_t)paths[u][i];
            for (size_t i = 0; i < edited[u].size(); i++) q[i] = (rcell_t)edited[u][i];
            path[0].push_back(paths[u]); path[1].push_back(stored ? edited[u] : paths[u]);
        }
        A.n_units = (int32_t)U; A.units = units.data(); A.results = res;
    }
};

static std::vector<int> cells_of(const Runs& runs) {
    std::vector<int> c;
    for (const auto& r : runs) for (int k = 0; k < r.second; k++) c.push_back(r.first + k);
    return c;
}

// both pack forms of `B` at the capacities given, against plain loops
static void check_pack(Blob& B, int which, int64_t cell_cap, int64_t run_cap) {
    HostGroup g;
    const int U = B.A.n_units;
    // plain loops: absolute cells, runs {start, length}
    std::vector<int32_t> w_len, w_cnt, w_cells, w_start, w_rlen;
    for (int u = 0; u < U; u++) {
        const std::vector<int>& p = B.path[which][(size_t)u];
        const int base = B.units[(size_t)u].seg_base;
        int n = 0;
        for (size_t i = 0; i < p.size(); i++) {
            const int a = p[i] > 0 ? p[i] + base : p[i] - base;
            w_cells.push_back(a);
            if (i == 0 || p[i] != p[i - 1] + 1) { w_start.push_back(a); w_rlen.push_back(0); n++; }
            w_rlen.back()++;
        }
        w_len.push_back((int32_t)p.size()); w_cnt.push_back(n);
    }
    {   // cells: exactly the first cell_cap cells
        std::vector<int32_t> lengths((size_t)U, SENT), cells((size_t)cell_cap, SENT);
        std::vector<int64_t> off((size_t)U + 1, -1);
        int64_t total = -1;
        pack_scan(g, B.A, which, lengths.data(), off.data(), &total);
        for (int u = 0; u < U; u++) pack_copy_unit(g, B.A, u, which, off.data(), cells.data(), cell_cap);
        CHECK(lengths == w_len && total == (int64_t)w_cells.size() && off[(size_t)U] == total);
        for (int64_t i = 0; i < cell_cap; i++) CHECK(cells[(size_t)i] == (i < total ? w_cells[(size_t)i] : SENT));
    }
    {   // runs: a unit whole or not at all
        std::vector<int32_t> lengths((size_t)U, SENT), counts((size_t)U, SENT), start((size_t)run_cap, SENT), rlen((size_t)run_cap, SENT);
        std::vector<int64_t> off((size_t)U + 1, -1);
        int64_t totals[2] = {-1, -1};
        for (int u = 0; u < U; u++) pack_runs_count_unit(g, B.A, u, which, lengths.data(), counts.data());
        pack_runs_scan(g, B.A, lengths.data(), counts.data(), off.data(), totals);
        for (int u = 0; u < U; u++) pack_runs_write_unit(g, B.A, u, which, off.data(), start.data(), rlen.data(), run_cap);
        CHECK(lengths == w_len && counts == w_cnt && totals[0] == (int64_t)w_start.size() && totals[1] == (int64_t)w_cells.size());
        int64_t o = 0;
        for (int u = 0; u < U; u++) {
            CHECK(off[(size_t)u] == o);
            const bool whole = o + w_cnt[(size_t)u] <= run_cap;
            for (int64_t k = o; k < o + w_cnt[(size_t)u] && k < run_cap; k++) {
                CHECK(start[(size_t)k] == (whole ? w_start[(size_t)k] : SENT));
                CHECK(rlen[(size_t)k] == (whole ? w_rlen[(size_t)k] : SENT));
            }
            o += w_cnt[(size_t)u];
        }
        for (int64_t k = o; k < run_cap; k++) CHECK(start[(size_t)k] == SENT && rlen[(size_t)k] == SENT);
    }
}

static void check_expand(const std::vector<int32_t>& start, const std::vector<int32_t>& len, int64_t cap) {
    std::vector<int64_t> off;
    std::vector<int32_t> want;
    for (size_t r = 0; r < len.size(); r++) { off.push_back((int64_t)want.size()); for (int k = 0; k < len[r]; k++) want.push_back(start[r] + k); }
    std::vector<int32_t> cells((size_t)cap, SENT);
    for (size_t r = 0; r < len.size(); r++) expand_run(HostGroup{}, start.data(), len.data(), off.data(), (int64_t)r, cells.data(), cap);
    for (int64_t i = 0; i < cap; i++) CHECK(cells[(size_t)i] == (i < (int64_t)want.size() ? want[(size_t)i] : SENT));
}

int main() {
    {   // three units, the middle one without a path, both strands, a one-cell run, an edited path for unit 2
        Blob B({{1, 2, 3, -3, -2, 2}, {}, {2, 3, 1}}, {{}, {}, {2, 3, 3, 1, 2}}, {0, 32, 64});
        for (int which = 0; which < 2; which++) {
            const int64_t cells = which ? 11 : 9, runs = which ? 6 : 5;
            check_pack(B, which, cells, runs);           // exact
            check_pack(B, which, cells - 1, runs - 1);   // one short: the last cell clamped, the last unit's runs not written
            check_pack(B, which, 4, 2);                  // inside unit 0
            check_pack(B, which, 0, 0);
            check_pack(B, which, cells + 3, runs + 3);
        }
    }
    {   // a unit of 300 runs of one to three cells between two small ones
        Runs r;
        for (int i = 0; i < 300; i++) r.push_back({(i % 2 ? -3 : 1), 1 + i % 3});
        const std::vector<int> big = cells_of(r);
        Blob B({{1, 2}, big, {3}}, {{}, {}, {}}, {5, 0, 7});
        check_pack(B, 0, (int64_t)big.size() + 3, 302);
        check_pack(B, 1, (int64_t)big.size() + 2, 301);   // one short
        check_pack(B, 0, 100, 300);                       // the 300-run unit does not fit behind unit 0's run
    }
    {   // expand: lengths 0, 1, 64, 65 (the wavefront's stride), a negative start, capacities exact, cut inside a run, zero
        const std::vector<int32_t> start = {7, -9, 100, -200, 5, 40}, len = {0, 1, 64, 65, 0, 3};
        for (int64_t cap : {133, 132, 70, 1, 0, 140}) check_expand(start, len, cap);
        check_expand({}, {}, 4);
    }
    printf(fails ? "%d checks failed\n" : "exchange stages == plain loops: ok\n", fails);
    return fails ? 1 : 0;
}
