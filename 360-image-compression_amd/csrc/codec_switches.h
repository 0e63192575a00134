// codec_switches.h -- the fused latent codec's environment switches (LIC360_*): one struct, one table, one reader.  Host-only plain C++17.
//
// Every switch forces a schedule or a fall-back path that the codec would not pick by itself: what A/B runs and the "fall-back path kept tested"
// tests turn.  They are read when a codec is created (lic360_codec_create fills a lic360_switches from the environment, once, and keeps it), so every
// codec has its own and two codecs of one process may differ in any of them.  lic360_switches_read is the only place under csrc/ that names such a
// variable or reads the environment; DESIGN 4.1 "Switches" is written from the table below.
#pragma once
#include <cstdlib>
#include <string>

struct lic360_switches {                   // one field per row of the table below, at its default; what each does: the table
    bool conv16 = false;
    int coder_mode = -1;                   // 0 device, 1 host, 2 auto; -1: not set
    bool skip = true, clear = true, dc_tall = true;
    // LIC360_DC_ORDER.  A value that is no order leaves nb and place alone, sets dc_order_bad and keeps its text: the create that allocates decode lists
    // fails with it, one that allocates none never looks at the order.
    int dc_nb = 8;                         // blocks per emission group
    bool dc_place = true;                  // the placement pass
    bool dc_order_bad = false;
    std::string dc_order_text;
    bool dc_pack = true, dc_nets = true;
    int dc_gstep = 0;                      // 0 by task count, 1 one group per task always, 3 never
    int ec_gbk = 16;
    bool balance = true;
};

// LIC360_DC_ORDER: "1" (nb 1, no placement), "1p" (nb 1, placed), "2" / "4" / "8" (groups of nb blocks, placed); 0 = not one of these
static inline int lic360_dc_order_parse(const char *e, int *nb, bool *place) {
    const int v = e && e[0] >= '1' && e[0] <= '8' ? e[0] - '0' : 0;
    if (!v || (v & (v - 1)) || (e[1] && !(v == 1 && e[1] == 'p' && !e[2]))) return 0;
    *nb = v; *place = v > 1 || e[1] == 'p';
    return 1;
}

// One row per switch.  The accepted values are what they were when each switch was read where it was used, quirks included: "set" means present in
// the environment with ANY value, "" and "0" too.
struct lic360_switch_row {
    const char *name, *values, *what;
    void (*set)(lic360_switches &s, const char *v);                         // v: the variable's value (never null)
};
static const lic360_switch_row LIC360_SWITCH_TABLE[] = {
    {"LIC360_FUSED_CONV", "begins with 16", "the generic 16x16x4 kernels instead of the specialised ones",
     [](lic360_switches &s, const char *v) { s.conv16 = v[0] == '1' && v[1] == '6'; }},
    {"LIC360_HOST_CODER", "first character 0: device, 1: host, anything else: auto", "where the serial coder phases run",
     [](lic360_switches &s, const char *v) { s.coder_mode = v[0] == '0' ? 0 : (v[0] == '1' ? 1 : 2); }},
    {"LIC360_NOSKIP", "set", "no dead-cone skip",
     [](lic360_switches &s, const char *) { s.skip = false; }},
    {"LIC360_NOCLEAR", "set", "a skipping encode does not clear its ping-pong buffers",
     [](lic360_switches &s, const char *) { s.clear = false; }},
    {"LIC360_DC_NOTALL", "set", "decode-order lists for latents of at most 64 rows only",
     [](lic360_switches &s, const char *) { s.dc_tall = false; }},
    {"LIC360_DC_ORDER", "1, 1p, 2, 4, 8 (anything else fails the create that allocates decode lists)", "order of the decode-order lists: blocks per group, p = placed",
     [](lic360_switches &s, const char *v) { if (!lic360_dc_order_parse(v, &s.dc_nb, &s.dc_place)) { s.dc_order_bad = true; s.dc_order_text = v; } }},
    {"LIC360_NOPACK", "set", "decode kernel without lists: one sample per wave",
     [](lic360_switches &s, const char *) { s.dc_pack = false; }},
    {"LIC360_DC_GSTEP", "first character 1: one group per task always, 3: never (else by task count)", "decode kernel without lists: task granularity",
     [](lic360_switches &s, const char *v) { s.dc_gstep = v[0] == '1' ? 1 : (v[0] == '3' ? 3 : 0); }},
    {"LIC360_DC_NONETS", "set", "the first decode layer keeps one net per task",
     [](lic360_switches &s, const char *) { s.dc_nets = false; }},
    {"LIC360_EC_GBK", "an integer in 1..4096 (anything else: 16)", "units per block of the encode kernels' task order",
     [](lic360_switches &s, const char *v) { const int x = atoi(v); s.ec_gbk = x > 0 && x <= 4096 ? x : 16; }},
    {"LIC360_NOBALANCE", "set", "decode-order lists without the XCD balancing pass",
     [](lic360_switches &s, const char *) { s.balance = false; }},
};

// the switches of the environment `get` looks names up in (null: not set)
static inline lic360_switches lic360_switches_read(const char *(*get)(const char *name)) {
    lic360_switches s;
    for (const lic360_switch_row &row : LIC360_SWITCH_TABLE)
        if (const char *v = get(row.name)) row.set(s, v);
    return s;
}
// what the create that meets s.dc_order_bad says
static inline std::string lic360_dc_order_message(const lic360_switches &s) { return "LIC360_DC_ORDER=" + s.dc_order_text + ": expected 1, 1p, 2, 4 or 8"; }
static inline lic360_switches lic360_switches_env() {
    return lic360_switches_read([](const char *name) -> const char * { return getenv(name); });
}
// For the public entry points that run one launch without a codec (lic360_cconv4_dc_plane, lic360_cconv16_ec, lic360_cconv16_ec_tables): the process's
// environment as it was at the FIRST call of any of the three, for all of them and every later call -- once per process, not per launch.  A codec never
// reads through this.
inline const lic360_switches &lic360_process_switches() {
    static const lic360_switches s = lic360_switches_env();
    return s;
}
