/*
 * lh_tmax_model.c -- the PRODUCT's bounded one-ray host walk (lucille_amd/csrc/lh_hostwalk.c lh_host_walk_tmax: lh_tmax.h's rule, step for
 * step as the bounded kernels apply it) over the model's trees, ray by ray.  Test infrastructure: built by tests/tmax_cases.py into a
 * library of its own together with lh_model.c (the trees: lhm_build / lhm_ref_build) and the product's sources, so that the not-gpu
 * suite pins the rule on the oracle without a device (tests/test_tmax_model.py).
 */
#include <stddef.h>
#include <stdint.h>

#include "lh_bvh.h"
#include "lh_refbvh.h"

int lh_host_walk_tmax(const lh_bvh_t *b, const lh_refbvh_t *ref, const double o[3], const double d[3], double tmax, int anyhit,
                      uint32_t *prim, double *t, double *u, double *v);

/* n rays with a bound each.  anyhit 0: the records go to prim / t / u / v; 1: the occluded bytes to occ.  Returns the number of rays the
 * walk could not finish (0 is what the test asks for) */
int lhtm_walk(const lh_bvh_t *b, const lh_refbvh_t *ref, size_t n, const double *org, const double *dir, const double *tmax, int anyhit,
              uint32_t *prim, double *t, double *u, double *v, uint8_t *occ)
{
    size_t i; int unfinished = 0;
    for (i = 0; i < n; i++) {
        uint32_t p; double tt, uu, vv;
        const int rc = lh_host_walk_tmax(b, ref, org + 3 * i, dir + 3 * i, tmax[i], anyhit, &p, &tt, &uu, &vv);
        if (rc < 0) { unfinished++; continue; }
        if (anyhit) occ[i] = (uint8_t)(rc ? 1 : 0);
        else { prim[i] = p; t[i] = tt; u[i] = uu; v[i] = vv; }
    }
    return unfinished;
}
