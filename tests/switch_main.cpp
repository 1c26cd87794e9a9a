// switch_main.cpp -- stand-alone host program for tests/test_switches.py: includes ONLY the library's switch header.
//   switch_main --table   one line per switch: name kind dflt lo hi once
//   switch_main           every switch parsed on a set of hostile values (one line each: name label set value), then the
//                         read time of one every-query and one read-once switch through the environment
#include <stdio.h>
#include <string.h>

#include <string>

#include "../pykrylov_amd/csrc/mk_switch.h"

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "--table")) {
        for (const MkSwitchRow &r : mk_switch_table)
            printf("%s %c %ld %ld %ld %d\n", r.name, r.kind, r.dflt, r.lo, r.hi, r.once ? 1 : 0);
        return 0;
    }
    const std::string digits40(40, '9'), commas(4096, ',');
    const struct {
        const char *label, *text;
    } cases[] = {{"unset", nullptr}, {"empty", ""}, {"abc", "abc"}, {"12abc", "12abc"}, {"7comma", "7,"}, {"7comma_blank", "7, "},
                 {"minus5", "-5"}, {"digits40", digits40.c_str()}, {"commas4k", commas.c_str()}};
    for (const MkSwitchRow &r : mk_switch_table)
        for (const auto &c : cases) {
            const MkSwitchVal v = mk_switch_parse(r, c.text);
            printf("%s %s %d %ld\n", r.name, c.label, v.set ? 1 : 0, v.v);
        }
    setenv("MK_CG_FUSE", "0", 1);
    setenv("MK_SPMV_FORMAT", "3", 1);
    printf("read MK_CG_FUSE %ld MK_SPMV_FORMAT %ld\n", mk_switch_int<MK_SW_CG_FUSE>(), mk_switch_int<MK_SW_SPMV_FORMAT>());
    setenv("MK_CG_FUSE", "1", 1);
    setenv("MK_SPMV_FORMAT", "5", 1);
    printf("read MK_CG_FUSE %ld MK_SPMV_FORMAT %ld\n", mk_switch_int<MK_SW_CG_FUSE>(), mk_switch_int<MK_SW_SPMV_FORMAT>());
    unsetenv("MK_DEBUG_PLAN");
    printf("flag MK_DEBUG_PLAN %d", mk_switch_flag<MK_SW_DEBUG_PLAN>() ? 1 : 0);
    setenv("MK_DEBUG_PLAN", "", 1);
    printf(" %d\n", mk_switch_flag<MK_SW_DEBUG_PLAN>() ? 1 : 0);
    return 0;
}
