// tests/tools/path_coords_stage_check.cpp -- stand-alone check of the path coordinates stages (ambi_path_coords.hpp) on the CPU with the
// one-thread HostGroup, for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wno-unknown-pragmas
//       -I ambigram_amd/csrc tests/tools/path_coords_stage_check.cpp -o path_coords_stage_check && ./path_coords_stage_check
// Hand-built and random paths over the cells {+-1 .. +-3}, with segment lengths drawn from {0, 1, 2, 3, 1000, 2^31 - 1}, go through
// coords_unit and lift_query as the path of a one-unit batch; what they leave is compared with a naive transcription written here:
// a running sum for the plane and the summary, a linear search from the end for the lift.  Every buffer is a heap block of exactly
// its stated size: the result blob is one header plus unit_layout().total with the scanned path (which = 1, stored) as its LAST
// array, the plane slice pad16(8 * (path_cap + 1)), the length image n ints, the block UnitCoords + the answers -- so a read behind
// a path's capacity, a store behind the slice or a query answered from a neighbour is either a wrong result or the sanitizer's to
// report.  Covered on purpose: P = 0 with a negative status and with status 0, P = 1, 2, 3, both parities, P = path_cap (the 16-byte
// store must not reach entry P + 1), a length in the header above the capacity (clamped), zero-length runs at the front, the middle
// and the end, all lengths zero, a plane above 2^32, a cell id outside 1..n (length 0), which = 0 and 1, and the queries -1, 0,
// every cell's first, last and middle base, bp_len - 1, bp_len, 2^62.
// What this program does NOT reach: on HostGroup a round is two cells and exscan_i64 is the identity.  The 512-cell round, the
// scan across 256 threads and its 64-bit carry run on the device only; the GPU half of tests/test_path_coords.py covers them.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ambi_path_coords.hpp"

using namespace ambi;

static int fails = 0, g_case = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s (case %d)\n", __FILE__, __LINE__, #x, g_case); fails++; } } while (0)
// what the cases reached
static int n_failed = 0, n_big = 0, n_zero_front = 0, n_zero_mid = 0, n_zero_end = 0, n_full = 0, n_clamped = 0, n_odd = 0, n_even = 0, n_minus = 0, n_outside = 0;
static int64_t n_queries = 0;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 11); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }   // inclusive

typedef std::vector<int> Path;
static const int64_t kLens[6] = {0, 1, 2, 3, 1000, 0x7fffffff};

// one case: the unit has n = 3 segments of the lengths `len`, a capacity of `cap` cells, the header says `said` cells and `status`
static void run_case(const Path& path, const int64_t (&len)[3], int cap, int said, int status, int which) {
    g_case++;
    const int n = 3;
    UnitIn U{};
    U.n_seg = n; U.path_cap = cap; U.res_off = (int64_t)sizeof(UnitOut);
    const UnitLayout L = unit_layout(n, 0, cap, 0);
    const size_t blob_bytes = sizeof(UnitOut) + (size_t)L.total;
    uint8_t* blob = static_cast<uint8_t*>(malloc(blob_bytes));
    memset(blob, 0x11, blob_bytes);   // (stale cells: 0x1111, an id outside 1..n)
    UnitOut* h = reinterpret_cast<UnitOut*>(blob);
    memset(h, 0, sizeof(UnitOut));
    h->status = status;
    h->path_len = which ? 0 : said; h->path_indel_len = which ? said : 0; h->path_ind_stored = 1;
    rcell_t* cells = reinterpret_cast<rcell_t*>(blob + U.res_off + (which ? L.path_ind : L.path));
    for (size_t i = 0; i < path.size() && (int)i < cap; i++) cells[i] = (rcell_t)path[i];
    int32_t* image = static_cast<int32_t*>(malloc(n * sizeof(int32_t)));
    for (int i = 0; i < n; i++) image[i] = (int32_t)len[i];
    const int64_t len_off[1] = {0}, plane_off[1] = {0};
    const LenArgs I{image, len_off};
    const size_t plane_bytes = (size_t)pad16(int64_t(8) * (cap + 1));
    uint8_t* plane_raw = static_cast<uint8_t*>(malloc(plane_bytes));
    memset(plane_raw, 0x5a, plane_bytes);
    // ---- the transcription ----
    const int P = (status < 0 || said <= 0) ? 0 : std::min(said, cap);
    std::vector<int64_t> want((size_t)P + 1, 0);
    UnitCoords ws{};
    ws.status = P > 0 || status < 0 ? status : (int)ST_ERR_BAD_INPUT; ws.cells = P;
    auto len_of = [&](int c) -> int64_t { const int id = c < 0 ? -c : c; return id >= 1 && id <= n ? len[id - 1] : 0; };
    for (int k = 0; k < P; k++) {
        const int c = cells[k];
        want[(size_t)k + 1] = want[(size_t)k] + len_of(c);
        ws.runs += k == 0 || c != cells[k - 1] + 1;
        ws.empty_cells += len_of(c) == 0;
        if (c < 0) ws.bp_minus += len_of(c);
        n_outside += (c < 0 ? -c : c) > n;
    }
    ws.bp_len = want[(size_t)P];
    // the queries
    std::vector<LiftQuery> q;
    auto ask = [&](int64_t pos) { q.push_back(LiftQuery{0, 0, pos}); };
    for (int64_t pos : {int64_t(-1), int64_t(0), ws.bp_len - 1, ws.bp_len, ws.bp_len + 1, int64_t(1) << 62, -(int64_t(1) << 62)}) ask(pos);
    for (int k = 0; k < P; k++) { ask(want[(size_t)k]); ask(want[(size_t)k] - 1); ask((want[(size_t)k] + want[(size_t)k + 1]) / 2); ask(want[(size_t)k + 1] - 1); }
    const size_t block_bytes = (size_t)coords_block_bytes(1, (int64_t)q.size());
    uint8_t* block = static_cast<uint8_t*>(malloc(block_bytes));
    memset(block, 0x5a, block_bytes);
    LiftQuery* queries = static_cast<LiftQuery*>(malloc(q.size() * sizeof(LiftQuery)));
    memcpy(queries, q.data(), q.size() * sizeof(LiftQuery));
    // ---- the stages ----
    HostGroup g;
    coords_unit(g, &U, blob, I, 0, which, plane_raw, plane_off, block);
    PathLift* out = reinterpret_cast<PathLift*>(block + coords_results_off(1));
    for (int64_t i = 0; i < (int64_t)q.size(); i++) lift_query(&U, blob, I, which, plane_raw, plane_off, block, queries, i, out);
    // ---- the comparison ----
    const UnitCoords got = *reinterpret_cast<const UnitCoords*>(block);
    CHECK(memcmp(&got, &ws, sizeof(UnitCoords)) == 0);
    const int64_t* plane = reinterpret_cast<const int64_t*>(plane_raw);
    for (int k = 0; k <= P; k++) CHECK(plane[k] == want[(size_t)k]);
    for (size_t at = 8 * ((size_t)P + 1); at < plane_bytes; at++) CHECK(plane_raw[at] == 0x5a);   // nothing written behind entry P
    for (size_t i = 0; i < q.size(); i++) {
        PathLift w{};
        w.status = ws.status < 0 ? ws.status : 0; w.cell = -1; w.seg_off = -1; w.cell_start = -1;
        const int64_t pos = q[i].pos;
        if (ws.status >= 0 && pos >= 0 && pos < ws.bp_len) {
            int k = P - 1;
            while (want[(size_t)k] > pos) k--;   // the LAST k with plane[k] <= pos
            const int c = cells[k];
            const int64_t j = pos - want[(size_t)k];
            w.cell = k; w.seg = c; w.cell_start = want[(size_t)k]; w.seg_off = c > 0 ? j : len_of(c) - 1 - j;
            CHECK(j < len_of(c));   // (of the transcription itself: the cell holds the base)
        }
        const bool same = memcmp(&out[i], &w, sizeof(PathLift)) == 0;
        if (!same) printf("  query %zu pos %lld: got %d %d %d %lld %lld, want %d %d %d %lld %lld\n", i, (long long)pos, out[i].status, out[i].cell, out[i].seg,
                          (long long)out[i].seg_off, (long long)out[i].cell_start, w.status, w.cell, w.seg, (long long)w.seg_off, (long long)w.cell_start);
        CHECK(same);
    }
    n_queries += (int64_t)q.size();
    n_failed += ws.status < 0; n_big += ws.bp_len > (int64_t(1) << 32); n_full += P == cap && P > 0; n_clamped += said > cap && status >= 0;
    n_odd += P & 1; n_even += P > 0 && !(P & 1); n_minus += ws.bp_minus > 0;
    if (P >= 3 && ws.bp_len > 0) {
        n_zero_front += want[1] == 0;
        n_zero_end += want[(size_t)P - 1] == want[(size_t)P];
        for (int k = 1; k + 1 < P; k++) if (want[(size_t)k] == want[(size_t)k + 1] && want[(size_t)k] > 0 && want[(size_t)k] < ws.bp_len) { n_zero_mid++; break; }
    }
    free(queries); free(block); free(plane_raw); free(image); free(blob);
}

int main() {
    const int64_t ones[3] = {1, 1, 1}, zeros[3] = {0, 0, 0}, big[3] = {0x7fffffff, 0x7fffffff, 1000}, mixed[3] = {0, 3, 1000}, mid0[3] = {2, 0, 0x7fffffff};
    // no path: a negative status (with cells in the header), status 0 and 3 without cells
    for (int which : {0, 1}) {
        run_case({1, 2, 3}, ones, 8, 3, ST_ERR_NO_ELEMENTS, which);
        run_case({}, ones, 8, 0, ST_OK, which);
        run_case({}, big, 1, 0, ST_NO_VALID_ORDER, which);
        run_case({1}, ones, 4, -5, ST_OK, which);
    }
    // P = 1, 2, 3, at and below the capacity, every set of lengths
    for (const auto* L : {&ones, &zeros, &big, &mixed, &mid0})
        for (int which : {0, 1}) {
            for (int c : {1, -1, 2, -3}) { run_case({c}, *L, 1, 1, ST_OK, which); run_case({c}, *L, 5, 1, ST_SHORTCUT, which); }
            run_case({1, 2}, *L, 2, 2, ST_OK, which); run_case({2, -2}, *L, 3, 2, ST_OK, which);
            run_case({1, 2, 3}, *L, 3, 3, ST_OK, which); run_case({-3, -2, -1}, *L, 4, 3, ST_OK, which); run_case({1, 2, -2}, *L, 8, 3, ST_OK, which);
            run_case({1, 2, 3, -3, -2, -1, 1, 2, 3}, *L, 9, 9, ST_OK, which);
            run_case({1, 2, 3, -3, -2, -1, 1, 2, 3}, *L, 6, 9, ST_OK, which);   // the header says more than the capacity: clamped
            run_case({1, 2, 3, -3, -2, -1, 1, 2, 3}, *L, 5, 1 << 22, ST_OK, which);
        }
    // zero-length runs at the front, the middle and the end; a cell id outside 1..n
    run_case({1, 1, 2, 3, 1, 1, 3, 2, 1, 1}, mixed, 12, 10, ST_OK, 1);
    run_case({-1, -1, -2, -3, -1, -1, -3, 2, -1, -1}, mixed, 10, 10, ST_OK, 0);
    run_case({1, 2, 2, 3, 1}, mid0, 5, 5, ST_OK, 1);
    run_case({1, 4, -7, 2, 3}, ones, 6, 5, ST_OK, 1);
    // random paths, lengths and capacities
    for (int it = 0; it < 600; it++) {
        const int P = it % 7 == 0 ? rnd_in(1, 4) : rnd_in(1, 70);
        Path p((size_t)P);
        for (int& v : p) { v = rnd_in(1, 3); if (rnd() & 1) v = -v; }
        if (it % 5 == 0) for (int k = 1; k < P; k++) if (rnd() % 3) p[(size_t)k] = p[(size_t)k - 1] + 1 <= 3 && p[(size_t)k - 1] + 1 != 0 ? p[(size_t)k - 1] + 1 : p[(size_t)k];   // runs
        int64_t len[3];
        for (int64_t& l : len) l = kLens[rnd_in(0, 5)];
        const int cap = it % 3 == 0 ? P : P + rnd_in(1, 9);
        run_case(p, len, cap, it % 11 == 0 ? P + rnd_in(1, 100) : P, it % 13 == 0 ? (int)ST_INFEASIBLE : (int)ST_OK, it & 1);
    }
    CHECK(n_failed >= 2 && n_big > 50 && n_zero_front > 10 && n_zero_mid > 10 && n_zero_end > 10 && n_full > 100 && n_clamped > 20);
    CHECK(n_odd > 100 && n_even > 100 && n_minus > 100 && n_outside > 0 && n_queries > 10000);
    printf("cases %d queries %lld: failed %d big %d zero front %d mid %d end %d full %d clamped %d odd %d even %d minus %d outside %d\n", g_case, (long long)n_queries,
           n_failed, n_big, n_zero_front, n_zero_mid, n_zero_end, n_full, n_clamped, n_odd, n_even, n_minus, n_outside);
    if (fails) { printf("path_coords_stage_check: %d FAILED\n", fails); return 1; }
    printf("path_coords_stage_check: ok\n");
    return 0;
}
