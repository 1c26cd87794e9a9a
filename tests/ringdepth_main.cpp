// ringdepth_main.cpp -- stand-alone host program for tests/test_ring_depth_rule.py: includes ONLY the library's ring depth
// header.  Every argument is one case "vec_bytes:free_bytes:held:cap"; one line per case: depth fit.
#include <stdio.h>
#include <stdlib.h>

#include "../pykrylov_amd/csrc/mk_ringdepth.h"

int main(int argc, char **argv) {
    printf("max %d min_bytes %zu\n", MK_XD_MAX, MK_XD_MIN_BYTES);
    for (int k = 1; k < argc; ++k) {
        unsigned long long vec = 0, fr = 0;
        int held = 0, cap = 0;
        if (sscanf(argv[k], "%llu:%llu:%d:%d", &vec, &fr, &held, &cap) != 4) return 2;
        printf("%d %d\n", mk_ring_depth((size_t)vec, (size_t)fr, held, cap), mk_ring_fit((size_t)vec, (size_t)fr, held));
    }
    return 0;
}
