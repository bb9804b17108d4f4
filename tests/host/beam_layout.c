/* rt_beam as a C compiler lays it out (tests/test_render_beams_host.py): size and the six offsets. */
#include <stddef.h>
#include <stdio.h>

#include "rtcore.h"

int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(rt_beam), offsetof(rt_beam, origin), offsetof(rt_beam, direction),
           offsetof(rt_beam, origin_du), offsetof(rt_beam, origin_dv), offsetof(rt_beam, direction_du),
           offsetof(rt_beam, direction_dv));
    return 0;
}
