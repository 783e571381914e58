// The plan of the (u, v) EHT libraries (bhnerf_amd/csrc/eht_uv.h, eht_closure.h, eht_pol.h) printed by a plain C++ build, for
// tests/test_eht_edge_cases_cpu.py to hold the Python restatement of tests/eht_edge_cases.py to.
//
//   g++ -O2 -ffp-contract=off [-fsanitize=address,undefined] -I bhnerf_amd/csrc tools/eht_plan_host.cpp -o eht_plan_host
//   eht_plan_host N nvis ncp nca H W
//
// Prints one line: kblocks RS rows_per block eht_bytes cls_bytes pol_bytes (a byte count of 0: the plan refuses the sizes).
#include <stdio.h>
#include <stdlib.h>

#include "eht_closure.h"
#include "eht_pol.h"
#include "eht_uv.h"

int main(int argc, char **argv) {
    if (argc != 7) {
        fprintf(stderr, "usage: %s N nvis ncp nca H W\n", argv[0]);
        return 2;
    }
    int32_t a[6];
    for (int i = 0; i < 6; ++i) a[i] = (int32_t)atol(argv[1 + i]);
    const int32_t N = a[0], nvis = a[1], ncp = a[2], nca = a[3], H = a[4], W = a[5];
    EhtPlan e;
    ClsPlan c;
    PolPlan p;
    if (!eht_make_plan(N, nvis, ncp, H, W, &e)) {
        fprintf(stderr, "eht_make_plan refuses N %d nvis %d ncp %d H %d W %d\n", N, nvis, ncp, H, W);
        return 1;
    }
    const size_t cls = cls_make_plan(N, nvis, ncp, nca, H, W, &c) ? c.bytes : 0;
    const size_t pol = pol_make_plan(N, nvis, H, W, &p) ? p.bytes : 0;
    printf("%d %d %d %d %zu %zu %zu\n", e.kblocks, e.RS, e.rows_per, e.block, e.bytes, cls, pol);
    return 0;
}
