// launch_rules_check.cpp -- stand-alone printer of the three launch rules kept in
// csrc/host_shared.h, built by tests/test_launch_rules.py from that header alone:
//   * "G <width> <count> <g>": rbc_trees_per_block, the trees (merkle_kernel) or
//     instances (merkle_recheck_kernel) per one-wave block, for the (width, count)
//     pairs given on the command line as W:COUNT;
//   * "RC <R> <rc>": rbc_gf_pick_rc_impl(R, kGfRcMax), the body of the
//     launchers' rbc_gf_pick_rc, for R = 0..255;
//   * "RCMAX <kGfRcMax>" and "KRC <the instantiated row-chunk sizes>";
//   * "REGEN <per-instance lens 0/1> <S> <W> <RC> <NT>": rbc_gf_regen_form, the
//     gf_regen_kernel form of rbc_launch_gf_regen, for uniform rows of S =
//     1..4200 bytes at their 64-byte pitch, and for per-instance lengths at
//     that pitch (S then stands for the pitch).
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
    printf("\n");
    for (uint32_t S = 1; S <= 4200; ++S) {
        const uint32_t pitch = (S + 63u) / 64u * 64u;
        const RbcRegenForm u = rbc_gf_regen_form(false, S, pitch);
        printf("REGEN 0 %u %d %d %d\n", S, u.W, u.RC, u.NT);
        if (S == pitch) {
            const RbcRegenForm r = rbc_gf_regen_form(true, 0, pitch);
            printf("REGEN 1 %u %d %d %d\n", pitch, r.W, r.RC, r.NT);
        }
    }
    printf("ok\n");
    return 0;
}
