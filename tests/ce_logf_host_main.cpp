// lic360_logf of csrc/lic360_exact_math.h on the host, for tests/test_ce_rate_cases_cpu.py: reads a file of fp32 bit patterns (uint32, little endian),
// writes the bit patterns of lic360_logf of each to a second file.  Built with g++ -ffp-contract=off -fsanitize=address,undefined and run as a child
// process.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lic360_exact_math.h"

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    std::vector<uint32_t> bits;
    uint32_t word;
    while (std::fread(&word, sizeof(word), 1, in) == 1) bits.push_back(word);
    std::fclose(in);
    for (uint32_t &b : bits) {
        float x;
        std::memcpy(&x, &b, sizeof(x));
        const float y = lic360_logf(x);
        std::memcpy(&b, &y, sizeof(y));
    }
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 4;
    const size_t wrote = bits.empty() ? 0 : std::fwrite(bits.data(), sizeof(uint32_t), bits.size(), out);
    std::fclose(out);
    return wrote == bits.size() ? 0 : 5;
}
