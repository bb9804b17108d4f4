/* rt_obscurance_params, rt_obscurance and rt_obscurance_select_params as a C compiler sees them
   (tests/test_obscurance_host.py): each record's size and its fields' offsets. */
#include <stddef.h>
#include <stdio.h>

#include "rtcore.h"

int main(void)
{
    printf("%zu %zu %zu %zu | %zu %zu %zu %zu %zu %zu | %zu %zu %zu %zu\n", sizeof(rt_obscurance_params),
           offsetof(rt_obscurance_params, radius), offsetof(rt_obscurance_params, power), offsetof(rt_obscurance_params, reserved),
           sizeof(rt_obscurance), offsetof(rt_obscurance, o), offsetof(rt_obscurance, o2), offsetof(rt_obscurance, bent),
           offsetof(rt_obscurance, samples), offsetof(rt_obscurance, hits), sizeof(rt_obscurance_select_params),
           offsetof(rt_obscurance_select_params, tol), offsetof(rt_obscurance_select_params, min_samples),
           offsetof(rt_obscurance_select_params, max_samples));
    return 0;
}
