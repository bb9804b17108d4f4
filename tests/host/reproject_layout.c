/* Prints the layout of rt_reproject_params as a C compiler sees include/rtcore.h: "sizeof <bytes>", then
 * "<field> <offset> <size>" per field, then RT_REPROJECT_SAME_PRIM and the ABI version
 * (tests/test_reproject_host.py compares it with the ctypes structure of raytracercore_amd). */
#include <stdio.h>

#include "rtcore.h"

#define FIELD(f) printf(#f " %zu %zu\n", offsetof(rt_reproject_params, f), sizeof(((rt_reproject_params*)0)->f))

int main(void)
{
    printf("sizeof %zu\n", sizeof(rt_reproject_params));
    FIELD(sigma_z);
    FIELD(normal_cos_min);
    FIELD(max_history);
    FIELD(flags);
    FIELD(reserved);
    printf("same_prim %u abi %d\n", RT_REPROJECT_SAME_PRIM, RTCORE_ABI_VERSION);
    return 0;
}
