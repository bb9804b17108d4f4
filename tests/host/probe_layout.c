/* rt_probe_sh as a C compiler sees it (tests/test_render_probes_host.py): size, the offsets of rows 0, 1 and
   8, of element [8][3], and the size of one row. */
#include <stddef.h>
#include <stdio.h>

#include "rtcore.h"

int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(rt_probe_sh), offsetof(rt_probe_sh, c[0]), offsetof(rt_probe_sh, c[1]),
           offsetof(rt_probe_sh, c[8]), offsetof(rt_probe_sh, c[8][3]), sizeof(((rt_probe_sh*)0)->c[0]));
    return 0;
}
