// slot_host_main.cpp -- the host coder core (csrc/ac_core.h: AcBitWriter / AcBitReader, what the host leg of the fused codec and the drop-in
// Coder run) at the edges of its slot, as a stand-alone program for an AddressSanitizer + UBSan build (tests/test_slot_cases_cpu.py compiles
// and runs it; tests/slot_cases.py holds the cases).
//
// Input (argv[1], int32 little-endian): ncases, then per case  ncode, n, L, ncaps, caps[ncaps], tables[n][ncode + 1], labels[n], coded[n],
// stream[L] (one byte per int32).  Every encode writes into a malloc'd slot of EXACTLY cap bytes, the decode reads from one of EXACTLY L
// bytes, so a write past the capacity or a read past the length is a heap-buffer-overflow report.
// Output: one line "enc <case> <cap> <len> <error> <crc32 of the min(len, cap) bytes written>" per capacity and one line
// "dec <case> <error> <crc32 of the symbols, one byte each, 0 where not coded>" per case.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ac_core.h"

static uint32_t crc32(const uint8_t *p, size_t n) {
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return ~c;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int32_t> in;
    int32_t chunk[4096];
    size_t got;
    while ((got = fread(chunk, sizeof(int32_t), 4096, f)) > 0) in.insert(in.end(), chunk, chunk + got);
    fclose(f);
    size_t at = 0;
    auto take = [&](size_t k) { const int32_t *p = in.data() + at; at += k; if (at > in.size()) { fprintf(stderr, "short input\n"); exit(2); } return p; };
    const int ncases = *take(1);
    for (int c = 0; c < ncases; ++c) {
        const int32_t *hd = take(4);
        const int ncode = hd[0], n = hd[1], L = hd[2], ncaps = hd[3];
        const int32_t *caps = take(ncaps), *tables = take((size_t)n * (ncode + 1)), *labels = take(n), *coded = take(n), *stream = take(L);
        for (int k = 0; k < ncaps; ++k) {
            const long cap = caps[k];
            uint8_t *slot = (uint8_t *)malloc((size_t)cap);
            AcState st;
            ac_init(st);
            AcBitWriter bw;
            ac_bw_init(bw, slot, cap);
            for (int i = 0; i < n; ++i) {
                if (!coded[i]) continue;
                const int32_t *t = tables + (size_t)i * (ncode + 1);
                ac_encode_symbol(st, bw, (uint32_t)t[labels[i]], (uint32_t)t[labels[i] + 1], (uint32_t)t[ncode]);
            }
            ac_encode_finish(st, bw);
            printf("enc %d %ld %ld %d %u\n", c, cap, bw.len, st.error | (bw.len > cap ? 16 : 0), crc32(slot, (size_t)(bw.len < cap ? bw.len : cap)));
            free(slot);
        }
        uint8_t *slot = (uint8_t *)malloc(L ? (size_t)L : 1);
        for (int i = 0; i < L; ++i) slot[i] = (uint8_t)stream[i];
        AcBitReader rd;
        ac_br_init(rd, slot, L);
        AcState st;
        ac_init(st);
        ac_decode_start(st, rd);
        std::vector<uint8_t> sym((size_t)n, 0);
        int error = 0;
        for (int i = 0; i < n; ++i) {
            if (!coded[i]) continue;
            const int32_t *t = tables + (size_t)i * (ncode + 1);
            const uint32_t total = (uint32_t)t[ncode], target = ac_decode_target(st, total);
            int s = 0;
            while (s + 1 < ncode && (uint32_t)t[s + 1] <= target) ++s;
            ac_decode_consume(st, rd, (uint32_t)t[s], (uint32_t)t[s + 1], total);
            error |= st.error;
            sym[i] = (uint8_t)s;
        }
        printf("dec %d %d %u\n", c, error, crc32(sym.data(), sym.size()));
        free(slot);
    }
    return 0;
}
