/*
 * lh_route_check.c -- lucille_amd/csrc/lh_route.h (what follows a device build) as a stand-alone program: every cell of its input space, one line
 * each: "who outcome build_auto ref_on_device : route".
 * tests/test_commit_route.py builds it with -fsanitize=address,undefined and compares the lines with the table written out there.
 */
#include <stdio.h>

#include "../../lucille_amd/csrc/lh_route.h"

int main(void)
{
    int who, o, au, rd;          /* the enums of lh_route.h from their first value to their last */
    for (who = 0; who <= LH_FOR_RECOMMIT; who++)
        for (o = 0; o <= LH_SIDE_SCAN_FAILED; o++)
            for (au = 0; au < 2; au++)
                for (rd = 0; rd < 2; rd++)
                    printf("%d %d %d %d : %d\n", who, o, au, rd, (int)lh_side_route((lh_side_builder_t)who, (lh_side_outcome_t)o, au, rd));
    return 0;
}
