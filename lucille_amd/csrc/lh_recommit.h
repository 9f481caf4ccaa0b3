/*
 * lh_recommit.h -- what a re-commit of an updatable device-mesh accelerator redoes (lh_commit.hip lh_accel_recommit), stated once.
 * Plain C without HIP: lh_commit.hip and a stand-alone checker (tests/cpu_model/lh_recommit_check.c, tests/test_recommit_plan.py)
 * read the same rule.
 *
 * The steps, in the order they run: flatten every mesh into a new array of triangle records; compare it with the resident one;
 * build both trees (and the danger list) from the new records; collapse the 8-wide nodes beside them; gather the per-vertex
 * normals and attributes again.  Whether the records changed is known only after the compare: the function is asked twice, first
 * with records_changed = 1 (its flatten and compare do not depend on it), then with what the compare found.
 */
#ifndef LH_RECOMMIT_H
#define LH_RECOMMIT_H

typedef struct lh_recommit_plan {
    int flatten;        /* lh_flatten_launch into a new tri64 array */
    int compare;        /* k_words_differ: the new records against the resident ones */
    int trees;          /* the traversal tree and tri32, lucille's own tree, the danger list */
    int q8;             /* the 8-wide nodes, from the same run of the builder */
    int gather;         /* lh_gather_launch into new per-primitive arrays */
} lh_recommit_plan_t;

/* pos_staged / attr_staged: an update of either kind since the last (re-)commit; records_changed: the compare's answer (ignored
 * unless positions are staged); had_q8: the resident scene holds 8-wide nodes; wide8: the accelerator's "wide8" (-1 / 0 / 1) */
static inline lh_recommit_plan_t lh_recommit_plan(int pos_staged, int attr_staged, int records_changed, int had_q8, int wide8)
{
    lh_recommit_plan_t p;
    p.flatten = pos_staged != 0;
    p.compare = p.flatten;
    p.trees = p.flatten && records_changed != 0;          /* the same records word for word: the trees built from them stand */
    p.q8 = p.trees && (had_q8 != 0 || wide8 == 1);        /* a scene that walked them keeps walking them; left to itself a new one gets them at its first dump */
    p.gather = pos_staged != 0 || attr_staged != 0;
    return p;
}

#endif
