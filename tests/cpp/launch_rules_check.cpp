// launch_rules_check.cpp -- stand-alone printer of the two launch rules kept in
// csrc/host_shared.h, built by tests/test_launch_rules.py from that header alone:
//   * "G <width> <count> <g>": rbc_trees_per_block, the trees (merkle_kernel) or
//     instances (merkle_recheck_kernel) per one-wave block, for the (width, count)
//     pairs given on the command line as W:COUNT;
//   * "RC <R> <rc>": rbc_gf_pick_rc_impl(R, kGfRcMax), the body of the
//     launchers' rbc_gf_pick_rc, for R = 0..255;
//   * "RCMAX <kGfRcMax>" and "KRC <the instantiated row-chunk sizes>".
// The test compares every line with the Python mirrors (tests/launch_rules.py)
// that the packed-Merkle and row-chunk GPU tests choose their shapes by.
#include <stdio.h>
#include <stdlib.h>

#include "../../cleisthenes_amd/csrc/host_shared.h"

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        int w = 0, count = 0;
        if (sscanf(argv[i], "%d:%d", &w, &count) != 2 || w < 1 || count < 0) {
            fprintf(stderr, "FAIL bad argument %s\n", argv[i]);
            return 1;
        }
        printf("G %d %d %d\n", w, count, rbc_trees_per_block(w, count));
    }
    for (int R = 0; R <= 255; ++R) printf("RC %d %d\n", R, rbc_gf_pick_rc_impl(R, kGfRcMax));
    printf("RCMAX %d\n", kGfRcMax);
    printf("KRC");
    for (int rc : kRC) printf(" %d", rc);
    printf("\nok\n");
    return 0;
}
