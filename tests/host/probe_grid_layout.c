/* rt_probe_grid as a C compiler sees it (tests/test_shade_probes_host.py): size, the six offsets and the
   flag's value. */
#include <stddef.h>
#include <stdio.h>

#include "rtcore.h"

int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %u\n", sizeof(rt_probe_grid), offsetof(rt_probe_grid, origin), offsetof(rt_probe_grid, step),
           offsetof(rt_probe_grid, dims), offsetof(rt_probe_grid, flags), offsetof(rt_probe_grid, bias),
           offsetof(rt_probe_grid, reserved), RT_PROBE_GRID_VISIBILITY);
    return 0;
}
