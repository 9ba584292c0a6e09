"""Order-table rows are Lehmer codes (csrc/ambi_orders.hpp): field d holds the rank of the row's node d among the nodes not yet
placed, in ceil(log2(K - d)) bits.  A small host probe compiled against ambi_orders.hpp checks the encoder (row_pack) and the
decoders (row_unpack, row_node) against an independent encoding written here, the row width against sum ceil(log2 m), and the
property the block emission relies on: a prefix with zeros behind it ORed with a suffix with zeros in front of it is the row."""
import itertools
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ambigram_amd", "csrc")

PROBE = r'''
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <vector>
#include "ambi_orders.hpp"
using namespace ambi;

static std::vector<uint32_t> pack(const std::vector<uint8_t>& p) {
    const int K = (int)p.size();
    std::vector<uint32_t> row(row_stride(K) / 4 + 1, 0xA5A5A5A5u);   // one guard dword behind the row
    row_pack(p.data(), K, row.data());
    return row;
}

// prefix [0, t) with zeros behind it (the directory's prefix words), suffix [t, K) with zeros in front of it and ones behind the
// last field (a suffix row of the block image), both from the same primitives the image builder uses
static std::vector<uint32_t> split_or(const std::vector<uint8_t>& p, int t) {
    const int K = (int)p.size(), nw = row_stride(K) / 4;
    std::vector<uint32_t> pre(nw, 0), suf(nw, 0), out(nw);
    uint64_t free_nodes = all_nodes(K);
    {
        RowBits rb;
        auto flush = [&](int wi, uint32_t w) { pre[wi] = w; };
        for (int d = 0; d < t; d++) { rb.put(lehmer_digit(free_nodes, p[d]), row_field_bits(K, d), flush); free_nodes &= ~(1ull << p[d]); }
        if (rb.n != 0) flush(rb.wi, (uint32_t)rb.acc);
    }
    {
        uint64_t rest = 0;                                   // the nodes still free at t: those of the suffix
        for (int d = t; d < K; d++) rest |= 1ull << p[d];
        if (rest != free_nodes) return {};
        RowBits rb;
        rb.start(row_field_off(K, t));
        auto flush = [&](int wi, uint32_t w) { suf[wi] = w; };
        for (int d = t; d < K; d++) { rb.put(lehmer_digit(rest, p[d]), row_field_bits(K, d), flush); rest &= ~(1ull << p[d]); }
        rb.finish(nw, flush);
    }
    for (int i = 0; i < nw; i++) out[i] = pre[i] | suf[i];
    return out;
}

static int check_row(const std::vector<uint8_t>& p) {
    const int K = (int)p.size(), nw = row_stride(K) / 4;
    const std::vector<uint32_t> row = pack(p);
    if (row[nw] != 0xA5A5A5A5u) return 1;                    // wrote behind the row
    uint8_t out[64];
    row_unpack(row.data(), K, out);
    for (int d = 0; d < K; d++) {
        if (out[d] != p[d]) return 2;
        if (row_node(row.data(), K, d) != p[d]) return 3;
    }
    return 0;
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "stride")) {
        for (int K = 1; K <= 63; K++) printf("%d %d %d\n", K, row_stride(K), lehmer_bits(K));
        return 0;
    }
    if (!strcmp(mode, "small")) {   // every permutation of up to 7 nodes
        long n = 0;
        for (int K = 1; K <= 7; K++) {
            std::vector<uint8_t> p(K);
            for (int i = 0; i < K; i++) p[i] = (uint8_t)i;
            std::vector<std::vector<uint32_t>> seen;
            do {
                if (int rc = check_row(p)) { printf("FAIL %d K=%d\n", rc, K); return 1; }
                seen.push_back(pack(p));
                for (int t = 0; t <= K; t++) {
                    std::vector<uint32_t> r = pack(p);
                    r.pop_back();
                    if (split_or(p, t) != r) { printf("FAIL or K=%d t=%d\n", K, t); return 1; }
                }
                n++;
            } while (std::next_permutation(p.begin(), p.end()));
            std::sort(seen.begin(), seen.end());
            if (std::unique(seen.begin(), seen.end()) != seen.end()) { printf("FAIL distinct K=%d\n", K); return 1; }
        }
        printf("OK %ld\n", n);
        return 0;
    }
    // one permutation per input line: "K v0 .. vK-1 t" -> the packed dwords, then "|", the OR of the split at t
    int K;
    while (scanf("%d", &K) == 1) {
        std::vector<uint8_t> p(K);
        for (int i = 0; i < K; i++) { int v; if (scanf("%d", &v) != 1) return 2; p[i] = (uint8_t)v; }
        int t;
        if (scanf("%d", &t) != 1) return 2;
        const int rc = check_row(p);
        std::vector<uint32_t> row = pack(p);
        row.pop_back();
        printf("%d", rc);
        for (uint32_t w : row) printf(" %u", w);
        printf(" |");
        for (uint32_t w : split_or(p, t)) printf(" %u", w);
        printf("\n");
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.fail("g++ is needed to build the row-format probe")
    d = tmp_path_factory.mktemp("lehmer_probe")
    src, exe = str(d / "probe.cpp"), str(d / "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", CSRC, "-o", exe, src])
    return exe


def _ceil_log2(m):
    return (m - 1).bit_length() if m > 1 else 0


def _expected_words(perm):
    """The row as the format defines it, written independently of the engine's code: digits at their offsets, ones behind."""
    K = len(perm)
    bits, free, off = 0, sorted(range(K)), 0
    for d, v in enumerate(perm):
        bits |= free.index(v) << off
        free.remove(v)
        off += _ceil_log2(K - d)
    nw = max(1, (off + 31) // 32)
    bits |= ((1 << (32 * nw)) - 1) & ~((1 << off) - 1)
    return [(bits >> (32 * i)) & 0xFFFFFFFF for i in range(nw)]


def test_row_stride_is_sum_of_field_widths(probe):
    out = subprocess.check_output([probe, "stride"], text=True).split("\n")
    rows = [list(map(int, l.split())) for l in out if l.strip()]
    assert [r[0] for r in rows] == list(range(1, 64))
    for K, stride, total in rows:
        want = sum(_ceil_log2(m) for m in range(1, K + 1))
        assert total == want, K
        assert stride == 4 * max(1, (want + 31) // 32), K
    stride = {K: s for K, s, _ in rows}
    assert stride[19] == 8 and stride[11] == 4 and stride[25] == 12 and stride[63] == 40


def test_every_permutation_up_to_7_nodes(probe):
    out = subprocess.check_output([probe, "small"], text=True).strip()
    assert out == "OK %d" % sum(len(list(itertools.permutations(range(K)))) for K in range(1, 8)), out


def test_random_permutations_every_node_count(probe):
    rng = random.Random(19)
    cases = []
    for K in range(1, 64):
        for _ in range(40):
            p = list(range(K))
            rng.shuffle(p)
            cases.append((p, rng.randint(0, K)))
    inp = "".join("%d %s %d\n" % (len(p), " ".join(map(str, p)), t) for p, t in cases)
    out = subprocess.run([probe, "rows"], input=inp, capture_output=True, text=True, check=True).stdout.split("\n")
    assert len([l for l in out if l.strip()]) == len(cases)
    for (p, t), line in zip(cases, out):
        whole, split = line.split("|")
        f = list(map(int, whole.split()))
        rc, words = f[0], f[1:]
        assert rc == 0, (p, rc)                                  # row_unpack and row_node give the permutation back
        assert words == _expected_words(p), p                    # the encoder writes the format
        assert list(map(int, split.split())) == words, (p, t)    # prefix | suffix = the row
