/*
 * lh_recommit_check.c -- lucille_amd/csrc/lh_recommit.h (what a re-commit redoes) as a stand-alone program: every input of its small input space,
 * one line each: "pos attr changed had_q8 wide8 : flatten compare trees q8 gather".  tests/test_recommit_plan.py builds it with
 * -fsanitize=address,undefined and compares the lines with a table written out there.
 */
#include <stdio.h>

#include "../../lucille_amd/csrc/lh_recommit.h"

int main(void)
{
    static const int wide8[3] = {-1, 0, 1};
    int pos, attr, changed, had, w;
    for (pos = 0; pos < 2; pos++)
        for (attr = 0; attr < 2; attr++)
            for (changed = 0; changed < 2; changed++)
                for (had = 0; had < 2; had++)
                    for (w = 0; w < 3; w++) {
                        const lh_recommit_plan_t p = lh_recommit_plan(pos, attr, changed, had, wide8[w]);
                        printf("%d %d %d %d %d : %d %d %d %d %d\n", pos, attr, changed, had, wide8[w], p.flatten, p.compare, p.trees, p.q8, p.gather);
                    }
    return 0;
}
