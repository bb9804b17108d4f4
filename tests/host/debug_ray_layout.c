/* Prints the layout of rt_debug_ray as a C compiler sees include/rtcore.h: "sizeof N", then
 * "<field> <offset> <size>" per field (tests/test_trace_paths_host.py compares it with the ctypes
 * structure and the numpy dtype of raytracercore_amd). */
#include <stdio.h>

#include "rtcore.h"

#define FIELD(f) printf(#f " %zu %zu\n", offsetof(rt_debug_ray, f), sizeof(((rt_debug_ray*)0)->f))

int main(void)
{
    printf("sizeof %zu\n", sizeof(rt_debug_ray));
    FIELD(prim_id);
    FIELD(type);
    FIELD(inside);
    FIELD(distance);
    FIELD(fresnel);
    FIELD(cos_in);
    FIELD(bounce);
    FIELD(reserved0);
    FIELD(position);
    FIELD(normal);
    FIELD(origin);
    FIELD(direction);
    FIELD(tint);
    FIELD(reserved1);
    printf("abi %d max_records %d\n", RTCORE_ABI_VERSION, RT_TRACE_MAX_RECORDS);
    printf("types %d %d %d %d %d %d %d %d %d %d\n", RT_BOUNCE_SKIPPED, RT_BOUNCE_DIFFUSE, RT_BOUNCE_SPECULAR,
           RT_BOUNCE_SPECULAR_FAIL, RT_BOUNCE_TRANSMITTED, RT_BOUNCE_EMISSION, RT_BOUNCE_PURE_BLACK,
           RT_BOUNCE_RECURSION_COMPLETE, RT_BOUNCE_MISSED, RT_BOUNCE_DEBUG);
    return 0;
}
