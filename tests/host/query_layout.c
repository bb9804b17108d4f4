/* Prints the layout of rt_ray and rt_hit as a C compiler sees include/rtcore.h: "sizeof <ray> <hit>",
 * then "<field> <offset> <size>" per field of rt_hit, then the rt_query_mode values and the ABI version
 * (tests/test_query_rays_host.py compares it with the ctypes structures and the numpy dtypes of
 * raytracercore_amd). */
#include <stdio.h>

#include "rtcore.h"

#define FIELD(f) printf(#f " %zu %zu\n", offsetof(rt_hit, f), sizeof(((rt_hit*)0)->f))

int main(void)
{
    printf("sizeof %zu %zu\n", sizeof(rt_ray), sizeof(rt_hit));
    FIELD(prim_id);
    FIELD(inside);
    FIELD(distance);
    FIELD(position);
    FIELD(normal);
    FIELD(reserved);
    printf("ray %zu %zu\n", offsetof(rt_ray, origin), offsetof(rt_ray, direction));
    printf("modes %d %d abi %d\n", RT_QUERY_FAST, RT_QUERY_EXACT, RTCORE_ABI_VERSION);
    return 0;
}
