/*
 * lh_route.h -- what follows a device build (lh_commit.hip side_build), stated once.  Plain C without HIP: lh_commit.hip and a
 * stand-alone checker (tests/cpu_model/lh_route_check.c, tests/test_commit_route.py) read the same rule.
 *
 * A device build makes a side -- the traversal tree and the records in its order, lucille's own tree, the danger list -- and ends
 * in one outcome.  Who asked for it and two flags of the scene decide what the caller does with anything but "built".
 */
#ifndef LH_ROUTE_H
#define LH_ROUTE_H

typedef enum lh_side_outcome {
    LH_SIDE_BUILT = 0,
    LH_SIDE_BAD_VERTEX,         /* a coordinate is NaN, infinite or beyond 1e30 (the builder's -2) */
    LH_SIDE_BUILDER_FAILED,     /* the builder of the traversal tree failed: memory, a HIP error */
    LH_SIDE_TOO_DEEP,           /* more levels than "build_depth_cap": what the walks' stacks take */
    LH_SIDE_TOO_MANY_NODES,     /* more 4-wide nodes than the 32-bit byte offset of node_step4 addresses */
    LH_SIDE_REF_FAILED,         /* the traversal tree stands, the builder of lucille's own tree failed */
    LH_SIDE_SCAN_FAILED         /* both trees stand, the danger scan over them met a HIP error */
} lh_side_outcome_t;

typedef enum lh_side_builder {
    LH_FOR_HOST_MESHES = 0,     /* lh_accel_commit of host arrays */
    LH_FOR_REPLICA,             /* lh_accel_commit_replica: a committed scene once more, on another device */
    LH_FOR_DEVICE_MESHES,       /* lh_accel_commit of device arrays: no host holds the triangles */
    LH_FOR_RECOMMIT             /* lh_accel_recommit: the resident scene stays whatever happens */
} lh_side_builder_t;

typedef enum lh_route {
    LH_ROUTE_INSTALL = 0,       /* built: the side becomes the scene */
    LH_ROUTE_ERROR,             /* the call fails */
    LH_ROUTE_HOST_BUILDERS,     /* the side is dropped, both trees are built on the host */
    LH_ROUTE_REF_HOST_THREAD    /* the side is installed without lucille's own tree: the background host thread builds that one */
} lh_route_t;

/* build_auto: the scene's size chose the device builders, nobody asked for them; ref_on_device: the scene's own tree is a device-built one, no host has a copy */
static inline lh_route_t lh_side_route(lh_side_builder_t who, lh_side_outcome_t outcome, int build_auto, int ref_on_device)
{
    if (outcome == LH_SIDE_BUILT) return LH_ROUTE_INSTALL;
    if (outcome == LH_SIDE_BAD_VERTEX || who == LH_FOR_RECOMMIT) return LH_ROUTE_ERROR;
    if (who == LH_FOR_DEVICE_MESHES) return LH_ROUTE_HOST_BUILDERS;          /* the flattened records are copied out */
    if (outcome == LH_SIDE_REF_FAILED) return ref_on_device ? LH_ROUTE_ERROR : LH_ROUTE_REF_HOST_THREAD;
    if (who == LH_FOR_REPLICA || outcome == LH_SIDE_SCAN_FAILED) return LH_ROUTE_ERROR;          /* a replica's source built the same tree: nothing to fall back to */
    if (outcome == LH_SIDE_TOO_DEEP) return LH_ROUTE_HOST_BUILDERS;          /* even where the device was asked for */
    return build_auto && !ref_on_device ? LH_ROUTE_HOST_BUILDERS : LH_ROUTE_ERROR;      /* the builder failed, or made too many nodes */
}

#endif
