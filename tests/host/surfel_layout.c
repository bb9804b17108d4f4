/* rt_surfel and rt_gather_mode as a C compiler sees them (tests/test_render_surfels_host.py): size, the
   two offsets and the three enum values. */
#include <stddef.h>
#include <stdio.h>

#include "rtcore.h"

int main(void)
{
    printf("%zu %zu %zu %d %d %d\n", sizeof(rt_surfel), offsetof(rt_surfel, position), offsetof(rt_surfel, normal),
           (int)RT_GATHER_DIFFUSE, (int)RT_GATHER_COSINE, (int)RT_GATHER_SPHERE);
    return 0;
}
