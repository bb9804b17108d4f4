/* rt_probe_relocate_params and rt_probe_relocation as a C compiler sees them (tests/test_probe_relocate_host.py):
   the params' size and five offsets, the record's size and the offsets of state, moved, skipped, k_near, reserved,
   d_near and d_far, and the three flags' values. */
#include <stddef.h>
#include <stdio.h>

#include "rtcore.h"

int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(rt_probe_relocate_params), offsetof(rt_probe_relocate_params, back_share),
           offsetof(rt_probe_relocate_params, min_front), offsetof(rt_probe_relocate_params, max_offset),
           offsetof(rt_probe_relocate_params, flags), offsetof(rt_probe_relocate_params, reserved));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rt_probe_relocation), offsetof(rt_probe_relocation, state),
           offsetof(rt_probe_relocation, moved), offsetof(rt_probe_relocation, skipped), offsetof(rt_probe_relocation, k_near),
           offsetof(rt_probe_relocation, reserved), offsetof(rt_probe_relocation, d_near), offsetof(rt_probe_relocation, d_far));
    printf("%u %u %u\n", RT_PROBE_INSIDE, RT_PROBE_IDLE, RT_PROBE_RELOCATE_CLASSIFY_ONLY);
    return 0;
}
