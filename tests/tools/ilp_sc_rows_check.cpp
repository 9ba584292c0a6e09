// tests/tools/ilp_sc_rows_check.cpp -- stand-alone check of the joint model's row-descriptor form on the CPU, for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I ambigram_amd/csrc
//       tests/tools/ilp_sc_rows_check.cpp ambigram_amd/csrc/ambi_ilp.cpp -o ilp_sc_rows_check && ./ilp_sc_rows_check
// For G = 1..4 graphs, n = 1..24 segments and two start ids it builds build_bfb_ilp_sc_rows + the host fill (ilp_fill_rows, ilp_fill_span,
// ilp_row_entries<4> over every 4-entry span inside a row) and compares with the loop generator build_bfb_ilp_sc; then the refusals.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ambi_ilp.hpp"
#include "ambi_ilp_rows.hpp"

using namespace ambi;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); fails++; } } while (0)

int main() {
    for (int G = 1; G <= 4; G++) for (int n = 1; n <= 24; n++) for (int s : {1, 7}) {
        const int e = s + n - 1;
        std::vector<double> seg((size_t)G * n), fold((size_t)G * n);
        for (size_t i = 0; i < seg.size(); i++) { seg[i] = 2 + (double)((i * 7) % 5); fold[i] = (double)((i * 3) % 4); }
        std::vector<std::pair<int, int>> evolution;
        for (int i = 0; i < G; i++) for (int j = i + 1; j < G; j++) evolution.push_back({i, j});
        IlpModel want, got;
        build_bfb_ilp_sc(s, e, G, seg.data(), fold.data(), evolution, want);
        std::vector<IlpRowDesc> rows;
        CHECK(build_bfb_ilp_sc_rows(s, e, G, seg.data(), fold.data(), got, rows));
        const IlpGeom geom = ilp_geom(s, e);
        CHECK(got.n_cols == want.n_cols && got.n_int == want.n_int && got.row_ptr == want.row_ptr);
        CHECK(got.row_lo == want.row_lo && got.row_up == want.row_up && got.col_lo == want.col_lo && got.col_up == want.col_up && got.obj == want.obj);
        if (got.row_ptr != want.row_ptr) continue;
        ilp_fill_rows(rows.data(), got.row_ptr.data(), 0, (int64_t)rows.size(), 1, geom, nullptr, nullptr, 0, 1, got.col.data(), got.val.data());
        CHECK(got.col == want.col && got.val == want.val);
        std::vector<int32_t> col(want.col.size(), -1); std::vector<double> val(want.val.size(), -1);
        for (int64_t p = 0; p < got.nnz(); p += 1000)    // spans that cut rows anywhere
            ilp_fill_span(rows.data(), got.row_ptr.data(), (int64_t)rows.size(), p, p + 1000 < got.nnz() ? p + 1000 : got.nnz(), geom, nullptr, nullptr, 0, 1,
                          col.data(), val.data());
        CHECK(col == want.col && val == want.val);
        for (size_t r = 0; r < rows.size(); r++) {       // the four-at-once form at every offset of every row
            const int64_t p0 = got.row_ptr[r], len = got.row_ptr[r + 1] - p0;
            for (int64_t j = 0; j + 4 <= len; j++) {
                int32_t c4[4]; double v4[4];
                ilp_row_entries<4>(rows[r], geom, (int)j, 4, nullptr, nullptr, c4, v4);
                for (int k = 0; k < 4; k++) if (c4[k] != want.col[p0 + j + k] || v4[k] != want.val[p0 + j + k]) { CHECK(!"ilp_row_entries<4>"); j = len; break; }
            }
        }
    }
    {   // limits: every one refused before anything is built (one segment: rows = columns = 2 G^2 + 2 G)
        IlpModel m; std::vector<IlpRowDesc> rows;
        std::vector<double> cn((size_t)1 << 23, 1.0);
        CHECK(!build_bfb_ilp_sc_rows(1, 1, 0, cn.data(), cn.data(), m, rows));
        CHECK(!build_bfb_ilp_sc_rows(1, 1, 1 << 23, cn.data(), cn.data(), m, rows));
        CHECK(!build_bfb_ilp_sc_rows(1, 1, 40000, cn.data(), cn.data(), m, rows));
        CHECK(!build_bfb_ilp_sc_rows(1, 1, 23171, cn.data(), cn.data(), m, rows));
        CHECK(m.n_rows() == 0 && rows.empty());
    }
    printf(fails ? "%d checks failed\n" : "joint row form == loop generator: ok\n", fails);
    return fails ? 1 : 0;
}
