// CPU build of the host-side skeleton of the side libraries (bhnerf_amd/csrc/side_lib.h), without HIP: the per-thread error
// message, for tests/test_abi_cpu.py to run under a sanitizer.
//
//   g++ -O2 -ffp-contract=off [-fsanitize=address,undefined] -I bhnerf_amd/csrc tools/side_lib_host.cpp -o side_lib_host
//   side_lib_host
//
// Exit code 0 when a message far longer than the buffer is cut at 511 characters and terminated, a failed argument check returns
// BHN_EINVAL with its message, and each of two threads that format messages at the same time reads back its own.
#include <string.h>

#include <string>
#include <thread>

#include "side_lib.h"

static int checked(int n) {
    BHN_CHECK_ARG(n >= 1, "bad count n=%d", n);
    return BHN_OK;
}

// `rounds` messages of this thread's own, each read back before the next; how many came back as written
static void writer(int id, int rounds, int *good) {
    for (int i = 0; i < rounds; ++i) {
        char want[64];
        snprintf(want, sizeof(want), "thread %d message %d", id, i);
        if (side_fail(BHN_EHIP, "thread %d message %d", id, i) == BHN_EHIP && strcmp(side_last_error(), want) == 0) ++*good;
    }
}

int main() {
    if (side_last_error()[0] != '\0') return fprintf(stderr, "the message is not empty at the start\n"), 1;
    const std::string big(4000, 'x');
    if (side_fail(BHN_EWORKSPACE, "%s and %d", big.c_str(), 7) != BHN_EWORKSPACE) return fprintf(stderr, "side_fail lost its code\n"), 1;
    const size_t len = strnlen(side_last_error(), 512);
    if (len != 511 || memcmp(side_last_error(), big.c_str(), 511) != 0) return fprintf(stderr, "long message: %zu characters kept\n", len), 1;
    if (checked(3) != BHN_OK || strnlen(side_last_error(), 512) != 511) return fprintf(stderr, "a passing check touched the message\n"), 1;
    if (checked(0) != BHN_EINVAL || strcmp(side_last_error(), "bad count n=0") != 0) return fprintf(stderr, "argument check: %s\n", side_last_error()), 1;
    const int rounds = 20000;
    int good[2] = {0, 0};
    std::thread a(writer, 1, rounds, &good[0]), b(writer, 2, rounds, &good[1]);
    a.join();
    b.join();
    if (good[0] != rounds || good[1] != rounds) return fprintf(stderr, "threads read back %d and %d of %d messages\n", good[0], good[1], rounds), 1;
    if (strcmp(side_last_error(), "bad count n=0") != 0) return fprintf(stderr, "another thread's message reached this one\n"), 1;
    return 0;
}
