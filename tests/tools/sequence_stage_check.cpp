// tests/tools/sequence_stage_check.cpp -- stand-alone check of the sequence stages (ambi_sequence.hpp) on the CPU with the
// one-thread HostGroup, for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Wno-unknown-pragmas
//       tests/tools/sequence_stage_check.cpp -o sequence_stage_check && ./sequence_stage_check
// Hand-made result blobs and sequence images go through the very functions the kernels and the host simulation call (both
// passes of seq_extents_unit, seq_layout, seq_fill_tile); what they leave is compared with a plain loop over the cells written
// here.  Every buffer -- the image, the totals, the extent arrays, the output block -- has exactly the size the stage is told, so
// a read or write outside it is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <vector>

#include "../../ambigram_amd/csrc/ambi_sequence.hpp"

using namespace ambi;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); fails++; } } while (0)

static uint32_t rng_state = 12345;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

struct Unit { int n; std::vector<int> path, edited; int status; std::vector<int> seg_len; };

// exact-size heap arrays (a std::vector's capacity may exceed its size)
template <class T> struct Exact {
    T* p; size_t n;
    explicit Exact(size_t count) : p(count ? new T[count]() : nullptr), n(count) {}
    ~Exact() { delete[] p; }
    Exact(const Exact&) = delete; Exact& operator=(const Exact&) = delete;
};

static uint8_t plain_complement(uint8_t c) {
    static const char* from = "ACGTUMRWSYKVHDBNacgtumrwsykvhdbn";
    static const char* to = "TGCAAKYWSRMBDHVNtgcaakywsrmbdhvn";
    for (int i = 0; from[i]; i++) if ((uint8_t)from[i] == c) return (uint8_t)to[i];
    return c;
}

static void check_batch(const std::vector<Unit>& units, int which, int first, int count) {
    HostGroup g;
    const size_t U = units.size();
    // result blob
    std::vector<UnitIn> in(U);
    int64_t o = (int64_t)sizeof(UnitOut) * (int64_t)U;
    for (size_t u = 0; u < U; u++) {
        UnitIn& I = in[u];
        I = UnitIn{};
        I.n_seg = units[u].n; I.seg_base = 100 * (int)u; I.bkp_cap = 2; I.out_cap = 1;
        I.path_cap = (int)std::max<size_t>(std::max(units[u].path.size(), units[u].edited.size()), 1);
        I.res_off = o;
        o += unit_layout(I.n_seg, I.bkp_cap, I.path_cap, I.out_cap).total;
    }
    Exact<uint64_t> mem((size_t)(o + 7) / 8);
    uint8_t* res = reinterpret_cast<uint8_t*>(mem.p);
    for (size_t u = 0; u < U; u++) {
        const UnitLayout L = unit_layout(in[u].n_seg, in[u].bkp_cap, in[u].path_cap, in[u].out_cap);
        UnitOut* h = unit_out(res, (int)u);
        const bool stored = !units[u].edited.empty();
        h->status = units[u].status;
        h->path_len = (int)units[u].path.size(); h->path_ind_stored = stored;
        h->path_indel_len = (int)(stored ? units[u].edited.size() : units[u].path.size());
        rcell_t* p = reinterpret_cast<rcell_t*>(res + in[u].res_off + L.path);
        rcell_t* q = reinterpret_cast<rcell_t*>(res + in[u].res_off + L.path_ind);
        for (size_t i = 0; i < units[u].path.size(); i++) p[i] = (rcell_t)units[u].path[i];
        for (size_t i = 0; i < units[u].edited.size(); i++) q[i] = (rcell_t)units[u].edited[i];
    }
    // sequence image: the stores in REVERSE unit order (a unit's store may lie anywhere), every byte value
    std::vector<int64_t> store_off(U), pos_off(U);
    int64_t nb = 0, np = 0;
    for (size_t k = U; k-- > 0;) { store_off[k] = nb; for (int l : units[k].seg_len) nb += l; }
    for (size_t u = 0; u < U; u++) { pos_off[u] = np; np += units[u].n + 1; }
    Exact<uint8_t> bases((size_t)nb);
    Exact<int64_t> seg_pos((size_t)np);
    for (int64_t i = 0; i < nb; i++) bases.p[i] = (rnd() % 5 == 0) ? (uint8_t)rnd() : (uint8_t)"ACGTNacgtnRYKMryk"[rnd() % 17];
    for (size_t u = 0; u < U; u++) { int64_t a = 0; for (int i = 0; i <= units[u].n; i++) { seg_pos.p[pos_off[u] + i] = a; if (i < units[u].n) a += units[u].seg_len[(size_t)i]; } }
    const SeqArgs S{bases.p, seg_pos.p, store_off.data(), pos_off.data()};
    // the plain expectation
    std::vector<std::vector<uint8_t>> want((size_t)count);
    for (int r = 0; r < count; r++) {
        const Unit& N = units[(size_t)(first + r)];
        if (N.status < 0) continue;
        const std::vector<int>& p = (which && !N.edited.empty()) ? N.edited : N.path;
        for (int c : p) {
            const int s = c < 0 ? -c : c;
            const uint8_t* b = bases.p + store_off[(size_t)(first + r)] + seg_pos.p[pos_off[(size_t)(first + r)] + s - 1];
            const int len = N.seg_len[(size_t)(s - 1)];
            if (c > 0) want[(size_t)r].insert(want[(size_t)r].end(), b, b + len);
            else for (int i = len - 1; i >= 0; i--) want[(size_t)r].push_back(plain_complement(b[i]));
        }
    }
    // the stages
    Exact<int64_t> totals((size_t)(2 * count));
    SeqPlan Q{};
    Q.first = first; Q.count = count; Q.totals = totals.p;
    for (int r = 0; r < count; r++) seq_extents_unit(g, in.data(), res, S, Q, r, which, 0);
    SeqLayout L;
    seq_layout(totals.p, count, L);
    for (int r = 0; r < count; r++) CHECK(L.len[(size_t)r] == (int64_t)want[(size_t)r].size());
    Exact<int64_t> ext_src((size_t)L.slots), ext_out((size_t)L.slots);
    uint8_t* out = L.out_bytes ? static_cast<uint8_t*>(aligned_alloc(16, (size_t)L.out_bytes)) : nullptr;
    if (out) memset(out, 0xEE, (size_t)L.out_bytes);
    Q.ext_off = L.ext_off.data(); Q.ext_src = ext_src.p; Q.ext_out = ext_out.p;
    Q.out_off = L.out_off.data(); Q.tile_off = L.tile_off.data(); Q.out = out; Q.out_bytes = L.out_bytes;
    for (int r = 0; r < count; r++) seq_extents_unit(g, in.data(), res, S, Q, r, which, 1);
    for (int r = 0; r < count; r++) {
        const int64_t e0 = L.ext_off[(size_t)r], R = L.ext_off[(size_t)r + 1] - e0 - 1;
        CHECK(ext_out.p[e0] == 0 || R == 0);
        CHECK(ext_out.p[e0 + R] == L.len[(size_t)r]);
        for (int64_t k = 0; k < R; k++) CHECK(ext_out.p[e0 + k] <= ext_out.p[e0 + k + 1]);
    }
    uint8_t table[256];
    seq_build_table(g, table);
    for (int i = 0; i < 256; i++) CHECK(table[i] == plain_complement((uint8_t)i));
    // tiles in order with one cursor, then again from the last tile down with the cursor kept (every tile must find its place
    // whatever the cursor holds), then every third tile with fresh cursors
    SeqCursor cur;
    for (int64_t t = 0; t < L.tiles; t++) seq_fill_tile(g, S, Q, table, t, cur);
    if (out) memset(out, 0xEE, (size_t)L.out_bytes);
    for (int64_t t = L.tiles; t-- > 0;) seq_fill_tile(g, S, Q, table, t, cur);
    for (int64_t t = 0; t < L.tiles; t += 3) { SeqCursor c2; seq_fill_tile(g, S, Q, table, t, c2); }
    for (int r = 0; r < count; r++) {
        const std::vector<uint8_t>& w = want[(size_t)r];
        const uint8_t* got = out + L.out_off[(size_t)r];
        CHECK(L.out_off[(size_t)r] % 16 == 0);
        if (!w.empty()) CHECK(memcmp(got, w.data(), w.size()) == 0);
        for (int64_t i = (int64_t)w.size(); i < pad16((int64_t)w.size()); i++) CHECK(got[i] == 0);   // the padding: zero
    }
    free(out);
}

static std::vector<int> run(int start, int cells) { std::vector<int> c; for (int k = 0; k < cells; k++) c.push_back(start + k); return c; }
static std::vector<int> cat(std::initializer_list<std::vector<int>> parts) { std::vector<int> c; for (auto& p : parts) c.insert(c.end(), p.begin(), p.end()); return c; }

int main() {
    // hand-made units: one-base runs on both strands, empty segments, a run ending on a 16-byte boundary, three runs in one
    // group, a unit shorter than 16 bytes, an empty unit, a refused unit, a segment longer than two tiles crossed on both strands
    std::vector<Unit> units;
    units.push_back({4, cat({run(1, 4), run(-4, 3), run(2, 1), run(-2, 1), run(3, 2)}), {}, 0, {1, 1, 14, 16}});
    units.push_back({3, run(1, 3), {}, 1, {2, 0, 5}});                                            // 7 bytes in all
    units.push_back({3, {}, {}, 3, {4, 4, 4}});                                                   // no path
    units.push_back({3, run(1, 3), {}, -11, {4, 4, 4}});                                          // refused: length 0
    units.push_back({5, cat({run(1, 5), run(-5, 5), run(3, 1), run(-3, 1), run(3, 3)}), cat({run(1, 5), run(-5, 2), run(2, 2)}), 0, {3, 2 * kSeqTile + 37, 1, 0, 16}});
    units.push_back({2, cat({run(1, 2), run(-2, 2), run(1, 1), run(-1, 1), run(1, 1), run(-1, 1), run(2, 1)}), {}, 0, {1, 1}});   // one-base runs only
    units.push_back({6, cat({run(-6, 6), run(1, 6)}), {}, 0, {16, 16, 32, 15, 1, kSeqTile}});       // everything on 16-byte boundaries
    // random units: run starts at every offset, every strand
    for (int k = 0; k < 24; k++) {
        Unit N;
        N.n = 1 + (int)(rnd() % 12); N.status = (k % 7 == 6) ? 2 : 0;
        for (int i = 0; i < N.n; i++) N.seg_len.push_back((int)(rnd() % 4 == 0 ? rnd() % 3 : 1 + rnd() % 40));
        for (int pass = 0; pass < 2; pass++) {
            std::vector<int>& p = pass ? N.edited : N.path;
            if (pass && k % 3) break;
            const int nruns = 1 + (int)(rnd() % 30);
            for (int q = 0; q < nruns; q++) {
                const int a = 1 + (int)(rnd() % N.n), len = 1 + (int)(rnd() % (N.n - a + 1));
                std::vector<int> rr = (rnd() & 1) ? run(a, len) : run(-(a + len - 1), len);
                if (!p.empty() && rr[0] == p.back() + 1) continue;   // (would merge with the run before)
                p.insert(p.end(), rr.begin(), rr.end());
            }
        }
        units.push_back(N);
    }
    const int U = (int)units.size();
    for (int which = 0; which < 2; which++) {
        check_batch(units, which, 0, U);
        check_batch(units, which, 4, 1);
        check_batch(units, which, U - 1, 1);
        check_batch(units, which, 2, 2);      // nothing to assemble: no output block at all
        check_batch(units, which, 3, 9);
    }
    if (fails) { printf("sequence_stage_check: %d failures\n", fails); return 1; }
    printf("sequence_stage_check: ok (%d units)\n", U);
    return 0;
}
