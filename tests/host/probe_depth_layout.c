/* rt_probe_depth_params and rt_probe_depth as a C compiler sees them (tests/test_probe_depth_host.py): the
   params' size and five offsets, the accumulators' size and the offset of their second row, the flag's value. */
#include <stddef.h>
#include <stdio.h>

#include "rtcore.h"

int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %u\n", sizeof(rt_probe_depth_params), offsetof(rt_probe_depth_params, d_max),
           offsetof(rt_probe_depth_params, var_floor), offsetof(rt_probe_depth_params, sharpness),
           offsetof(rt_probe_depth_params, flags), offsetof(rt_probe_depth_params, reserved), sizeof(rt_probe_depth),
           offsetof(rt_probe_depth, s[1]), RT_PROBE_DEPTH_WRAP);
    return 0;
}
