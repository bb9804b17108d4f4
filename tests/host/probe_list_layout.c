/* rt_probe_moments and rt_probe_select_params as a C compiler sees them (tests/test_probe_list_host.py): the
   sizes, then the offsets of m[1], m[3][1], irr_floor, ambient, min_samples and max_samples. */
#include <stddef.h>
#include <stdio.h>

#include "rtcore.h"

int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rt_probe_moments), sizeof(rt_probe_select_params),
           offsetof(rt_probe_moments, m[1]), offsetof(rt_probe_moments, m[3][1]), offsetof(rt_probe_select_params, irr_floor),
           offsetof(rt_probe_select_params, ambient), offsetof(rt_probe_select_params, min_samples),
           offsetof(rt_probe_select_params, max_samples));
    return 0;
}
