/* Prints the layout of rt_select_item and rt_selection as a C compiler sees include/rtcore.h:
 * "sizeof <item> <selection>", then "<struct>.<field> <offset> <size>" per field, then the
 * rt_select_kind values, the ABI version and whether RT_SELECT_MAX_TESTS is 2^32
 * (tests/test_select_host.py compares it with the ctypes structures and the numpy dtypes of
 * raytracercore_amd). */
#include <stdio.h>

#include "rtcore.h"

#define FIELD(s, f) printf(#s "." #f " %zu %zu\n", offsetof(s, f), sizeof(((s*)0)->f))

int main(void)
{
    printf("sizeof %zu %zu\n", sizeof(rt_select_item), sizeof(rt_selection));
    FIELD(rt_select_item, kind);
    FIELD(rt_select_item, index);
    FIELD(rt_selection, item);
    FIELD(rt_selection, reserved);
    FIELD(rt_selection, distance);
    printf("kinds %d %d abi %d max_tests_is_2_32 %d\n", RT_SELECT_PRIM, RT_SELECT_NODE, RTCORE_ABI_VERSION,
           RT_SELECT_MAX_TESTS == 4294967296ull);
    return 0;
}
