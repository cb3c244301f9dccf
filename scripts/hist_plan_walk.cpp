// Walks eas_event_histogram_plan (host code of eas_snn_amd/csrc/events.hip, no GPU needed) over H 1..1200 x W 1..2048 for both counter
// widths and checks every band plan: at most 150 KB of dynamic LDS, at most 8 bands, bands that cover the frame with none empty.  Meant to
// be built with the host sanitizers, as a program of its own (from eas_snn_amd/csrc):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I. events.hip capi.hip ../../scripts/hist_plan_walk.cpp -o hist_plan_walk && ./hist_plan_walk
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../include/eas_hip.h"

int main() {
    unsetenv("EAS_HIST_FORM");
    long plans[2] = {0, 0}, bad = 0;
    for (int aligned16 = 0; aligned16 < 2; ++aligned16)
        for (int H = 1; H <= 1200; ++H)
            for (int W = 1; W <= 2048; ++W) {
                int rows = -1, nbands = -1;
                int64_t lds = -1;
                const int form = eas_event_histogram_plan((int64_t)1 << 40, 1, 1, H, W, aligned16, &rows, &nbands, &lds);
                if (form == 0) continue;
                ++plans[aligned16];
                if (form != (aligned16 ? 2 : 1) || lds > 150 * 1024 || nbands < 1 || nbands > 8 || rows * nbands < H || rows * (nbands - 1) >= H) {
                    if (++bad <= 10) printf("bad plan: H %d W %d aligned16 %d -> form %d rows %d nbands %d lds %lld\n", H, W, aligned16, form, rows, nbands, (long long)lds);
                }
            }
    // extremes of the argument range: no overflow in the plan's arithmetic
    const int ext[][2] = {{1, 2147483647}, {2147483647, 1}, {2147483647, 2147483647}, {1, 1}, {65535, 65535}};
    for (const auto& e : ext)
        for (int aligned16 = 0; aligned16 < 2; ++aligned16) eas_event_histogram_plan(INT64_MAX, (1 << 24) - 1, 1, e[0], e[1], aligned16, nullptr, nullptr, nullptr);
    printf("plans: %ld with 32-bit counters, %ld with 16-bit counters, %ld bad\n", plans[0], plans[1], bad);
    return bad != 0;
}
