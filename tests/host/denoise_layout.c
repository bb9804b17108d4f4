/* Prints the layout of rt_denoise_params as a C compiler sees include/rtcore.h: "sizeof <bytes>", then
 * "<field> <offset> <size>" per field, then RT_DENOISE_SAME_PRIM and the ABI version
 * (tests/test_denoise_host.py compares it with the ctypes structure of raytracercore_amd). */
#include <stdio.h>

#include "rtcore.h"

#define FIELD(f) printf(#f " %zu %zu\n", offsetof(rt_denoise_params, f), sizeof(((rt_denoise_params*)0)->f))

int main(void)
{
    printf("sizeof %zu\n", sizeof(rt_denoise_params));
    FIELD(sigma_l);
    FIELD(sigma_z);
    FIELD(lum_eps);
    FIELD(normal_pow_log2);
    FIELD(iterations);
    FIELD(flags);
    FIELD(reserved);
    printf("same_prim %u abi %d\n", RT_DENOISE_SAME_PRIM, RTCORE_ABI_VERSION);
    return 0;
}
