// switches_main.cpp -- the reader of the fused latent codec's environment switches (csrc/codec_switches.h: lic360_switches_read over
// LIC360_SWITCH_TABLE) as a stand-alone program for an AddressSanitizer + UBSan build (tests/test_codec_switches_cpu.py compiles and runs it and
// holds the cases).  It includes nothing else of the project, opens no device and never looks at its own environment: the lookup it hands the reader
// searches the block of lines it has just read.
//
// Input (argv[1], text): blocks of lines NAME=value (the value may be empty), each block ended by a line "end": one environment per block.
// Output: a line "names <the table's names, in its order>", then per block one line "field=value" per field of lic360_switches and a line "end".
#include <cstdio>
#include <map>
#include <string>

#include "codec_switches.h"

static std::map<std::string, std::string> g_env;
static const char *lookup(const char *name) {
    const auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    printf("names");
    for (const lic360_switch_row &row : LIC360_SWITCH_TABLE) printf(" %s", row.name);
    printf("\n");
    char buf[512];
    while (fgets(buf, sizeof buf, f)) {
        std::string line(buf);
        while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
        if (line != "end") {
            const size_t eq = line.find('=');
            if (eq == std::string::npos) return 3;
            g_env[line.substr(0, eq)] = line.substr(eq + 1);
            continue;
        }
        const lic360_switches s = lic360_switches_read(lookup);
        printf("conv16=%d\ncoder_mode=%d\nskip=%d\nclear=%d\ndc_tall=%d\ndc_nb=%d\ndc_place=%d\ndc_order_bad=%d\ndc_order_text=%s\n", s.conv16, s.coder_mode,
               s.skip, s.clear, s.dc_tall, s.dc_nb, s.dc_place, s.dc_order_bad, s.dc_order_text.c_str());
        printf("dc_pack=%d\ndc_gstep=%d\ndc_nets=%d\nec_gbk=%d\nbalance=%d\nend\n", s.dc_pack, s.dc_gstep, s.dc_nets, s.ec_gbk, s.balance);
        g_env.clear();
    }
    fclose(f);
    return 0;
}
