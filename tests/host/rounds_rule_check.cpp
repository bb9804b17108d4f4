// Host evaluation of the sample rounds' rule (ticket_rounds, rt_kernels.h) at its edges, and of the
// launch record's field (make_params_for, launch_params.cpp).  Prints one line per case:
//   rule <mode> <pool> <chunk> <recursion> <first> <prev_rays> <result>
//   mode <RTCORE_SAMPLE_ROUNDS or -> <PathParams::sample_rounds>
//   size <sizeof(PathParams)> <offset of sample_rounds> <offset of scene_bound> <offset of cull>
// tests/test_sample_rounds_host.py works the expected values out on its own.
#include <cstdio>
#include <cstdlib>

#include "launch_params.h"
#include "rt_kernels.h"

using namespace rtc;

static void rule(int mode, int pool, int chunk, int recursion, bool first, unsigned prev)
{
    PathParams p{};
    p.sample_rounds = mode;
    p.pool = pool;
    p.chunk = chunk;
    printf("rule %d %d %d %d %d %u %d\n", mode, pool, chunk, recursion, (int)first, prev,
           (int)ticket_rounds(p, recursion, first, prev));
}

int main()
{
    const int shapes[][3] = {{64, 11, 10}, {128, 43, 3}, {64, 1, 10}, {64, 64, 0}, {4096, 64, 16383}, {64, 7, 1}};
    for (const auto& s : shapes) {
        const int pool = s[0], chunk = s[1], rec = s[2];
        const unsigned long long samples = (unsigned long long)pool * chunk;
        const unsigned long long full = samples * (unsigned long long)(rec + 1);
        const unsigned long long at_t = (full * kRoundsNum + kRoundsDen - 1) / kRoundsDen; // first count at T
        const unsigned long long edges[] = {0, 1, samples - 1, samples, samples + 1, at_t - 1, at_t, at_t + 1, full,
                                            // a short last ticket (7 of the chunk's samples) at full length
                                            (unsigned long long)pool * (chunk < 7 ? chunk : 7) * (rec + 1)};
        for (int mode = 0; mode <= 2; mode++)
            for (int first = 0; first <= 1; first++)
                for (const unsigned long long e : edges)
                    if (e <= 0xFFFFFFFFull) rule(mode, pool, chunk, rec, first != 0, (unsigned)e);
    }
    const char* settings[] = {nullptr, "0", "1", "2", "7", "-3", ""};
    for (const char* e : settings) {
        if (e) setenv("RTCORE_SAMPLE_ROUNDS", e, 1);
        else unsetenv("RTCORE_SAMPLE_ROUNDS");
        for (int kernel = 0; kernel < 4; kernel++) {
            const PathParams p = make_params_for(kernel, 0, 0, 0, 0, 256, 144, 37, 5, 0, 0.0);
            printf("mode %s %d %d\n", e ? (e[0] ? e : "empty") : "-", kernel, p.sample_rounds);
        }
    }
    printf("size %zu %zu %zu %zu\n", sizeof(PathParams), __builtin_offsetof(PathParams, sample_rounds),
           __builtin_offsetof(PathParams, scene_bound), __builtin_offsetof(PathParams, cull));
    return 0;
}
