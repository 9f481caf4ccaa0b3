"""ctypes binding of include/lucille_hip.h (the drop-in C ABI).

Reference interface mirrored: accel_build_func / accel_free_func /
accel_intersect_func (lucille src/render/accel.h:24-34) -- see the header for
the per-function mapping.  No compute happens in Python.
"""
import atexit
import collections
import ctypes as C
import os
import subprocess
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")

MISS = 0xFFFFFFFF
T_INF = 1.0e38
MODE_CLOSEST, MODE_ANY = 0, 1
VARIANT_DEFAULT, VARIANT_DIRECT, VARIANT_SPEC = -1, 0, 4      # the tuned walk (= SPEC), the textbook reference walk
RAYS_F64, RAYS_F32 = 0, 1           # ray formats of the _ex batch entry points (include/lucille_hip.h)
REC_F64, REC16 = 0, 1               # record formats: SoA prim / t / u / v, or 16-byte records {prim u32, t, u, v f32}
SELECT_HIT, SELECT_MISS, SELECT_OCCLUDED, SELECT_UNOCCLUDED = 0, 1, 2, 3      # what compact() keeps (LH_SELECT_*)
POS_F64, POS_F32 = 0, 1             # vertex formats of HipAccel.add_mesh_device (LH_POS_*)
AO_NO_HIT = 0xFFFFFFFF               # occluded count of a traced miss, slot of a miss (LH_AO_NO_HIT)


class LucilleHipError(RuntimeError):
    pass


def library_path():
    """LH_LIBRARY overrides the path (A/B runs of differently built kernels in tools/)"""
    return os.environ.get("LH_LIBRARY") or os.path.join(CSRC, "liblucille_hip.so")


def build_library(force=False):
    """Compile every HIP source for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC]
    if force:
        subprocess.check_call(args + ["clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(args + ["liblucille_hip.so"], stdout=subprocess.DEVNULL)
    return library_path()


class AccelInfo(C.Structure):
    _fields_ = [("ntriangles", C.c_uint32), ("nnodes", C.c_uint32), ("nleaves", C.c_uint32),
                ("max_depth", C.c_uint32), ("device_bytes", C.c_uint64), ("build_seconds", C.c_double),
                ("upload_seconds", C.c_double), ("device", C.c_int), ("ref_build_seconds", C.c_double),
                ("nnodes_traversal", C.c_uint32), ("ntriangles_in_tree", C.c_uint32)]


class RecommitInfo(C.Structure):
    """lh_recommit_info_t (include/lucille_hip.h): what lh_accel_recommit redid"""
    _fields_ = [("flattened", C.c_int), ("rebuilt_trees", C.c_int), ("regathered", C.c_int), ("seconds", C.c_double)]


class TreeImage(C.Structure):
    """lh_tree_image_t (include/lucille_hip.h): the figures of the resident traversal trees"""
    _fields_ = [("ntris", C.c_uint32), ("nlive", C.c_uint32), ("nq4", C.c_uint32), ("q4_depth", C.c_uint32), ("q4_stack", C.c_uint32),
                ("nq8", C.c_uint32), ("q8_depth", C.c_uint32), ("device_built", C.c_uint32),
                ("bmin", C.c_float * 3), ("bmax", C.c_float * 3), ("grid_lo", C.c_float * 3), ("grid_step", C.c_float * 3), ("scene_r", C.c_float)]


class RasterPlane(C.Structure):
    """lh_raster_plane_t (include/lucille_hip.h)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("frame", C.c_double * 9), ("eye", C.c_double * 3), ("fov", C.c_double)]


class Camera(C.Structure):
    """lh_camera_t: the members of ri_camera_t the ray generator reads (camera.c:248-318)"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("rh", C.c_int), ("ortho", C.c_int),
                ("flength", C.c_double), ("cam2world", C.c_double * 16)]

    @classmethod
    def make(cls, width, height, flength, cam2world, rh=1):
        c = cls(); c.width = int(width); c.height = int(height); c.rh = int(rh); c.flength = float(flength)
        m = np.asarray(cam2world, np.float64).reshape(16)
        for i in range(16):
            c.cam2world[i] = float(m[i])
        return c


class Material(C.Structure):
    """lh_material_t = ri_material_t's kd, ks, kt, ior (src/render/material.h:21-30)"""
    _fields_ = [("kd", C.c_float * 3), ("ks", C.c_float * 3), ("kt", C.c_float * 3), ("ior", C.c_float)]

    @classmethod
    def make(cls, kd=(1, 1, 1), ks=(0, 0, 0), kt=(0, 0, 0), ior=1.0):
        m = cls()
        for k in range(3):
            m.kd[k] = float(kd[k]); m.ks[k] = float(ks[k]); m.kt[k] = float(kt[k])
        m.ior = float(ior)
        return m


class Environment(C.Structure):
    _fields_ = [("rgb", C.c_float * 3), ("map_rgba", C.c_void_p), ("width", C.c_int), ("height", C.c_int)]


ALL_MESHES = 0xFFFFFFFF
PT_REFERENCE_WEIGHTS = 1
ATTR_COLOR, ATTR_TANGENT, ATTR_BINORMAL, ATTR_TEXCOORD, ATTR_TEXCOORD_UNSHARED = 0, 1, 2, 3, 4
STATE_DOUBLES = 24


class PtStats(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("rays", C.c_uint64), ("max_depth_reached", C.c_uint64)]


class TileStats(C.Structure):
    _fields_ = [("primary_rays", C.c_uint64), ("primary_hits", C.c_uint64), ("ao_rays", C.c_uint64),
                ("ao_occluded", C.c_uint64)]


class DirtParams(C.Structure):
    """lh_dirt_params_t: near clip, far clip and origin offset of the dirtmap transport (defaults: LH_DIRT_DEFAULTS)"""
    _fields_ = [("near_clip", C.c_double), ("far_clip", C.c_double), ("eps", C.c_double)]

    def __init__(self, near_clip=0.1, far_clip=0.5, eps=1.0e-5):
        super().__init__(float(near_clip), float(far_clip), float(eps))


class EnvParams(C.Structure):
    """lh_env_params_t: origin offset and scale of the environment-lit gather (defaults: LH_ENV_DEFAULTS; scale 0.3183098861837907 is
    gather_sunsky's 1 / pi, 1.0 is ri_ibl_sample_cosweight's)"""
    _fields_ = [("eps", C.c_double), ("scale", C.c_double)]

    def __init__(self, eps=1.0e-5, scale=1.0):
        super().__init__(float(eps), float(scale))


SKY_SUN = 1                       # LH_SKY_SUN: trace the sun's shadow ray


class Sky(C.Structure):
    """lh_sky_t: the sun-and-sky light of the environment-lit gather (lh_sky.h) -- the Preetham sky's angles, Perez coefficients and
    zenith values (from_site), the caller's colour pipeline's rgb and CIE y of the daylight basis spectra S0, S1, S2 (basis_rgb[j][k]:
    channel k of S_j; basis_y[j]), the sun's colour and world-space direction, and flags (SKY_SUN: trace the sun's shadow ray)"""
    _fields_ = [("sun_theta", C.c_float), ("sun_phi", C.c_float), ("perez_x", C.c_float * 5), ("perez_y", C.c_float * 5),
                ("perez_Y", C.c_float * 5), ("zenith_x", C.c_float), ("zenith_y", C.c_float), ("zenith_Y", C.c_float),
                ("basis_rgb", (C.c_float * 3) * 3), ("basis_y", C.c_float * 3), ("sun_rgb", C.c_float * 3), ("flags", C.c_uint32),
                ("sun_dir", C.c_double * 3)]

    @classmethod
    def from_site(cls, latitude, longitude, standard_meridian, julian_day, time_of_day, turbidity, basis_rgb=None, basis_y=None,
                  sun_rgb=(0.0, 0.0, 0.0), flags=0):
        """lh_sky_from_site: what ri_sunsky_init leaves for a site (degrees; standard_meridian in hours), a day of the year, a time of
        day (hours) and a turbidity; basis_rgb [3][3], basis_y [3], sun_rgb and flags are the caller's (zeros if not given)"""
        s = cls()
        if lib().lh_sky_from_site(C.byref(s), float(latitude), float(longitude), float(standard_meridian), int(julian_day),
                                  float(time_of_day), float(turbidity)) != 0:
            raise ValueError("Sky.from_site: a non-finite argument")
        if basis_rgb is not None:
            b = np.asarray(basis_rgb, np.float32).reshape(3, 3)
            for j in range(3):
                s.basis_rgb[j][:] = [float(x) for x in b[j]]
        if basis_y is not None:
            s.basis_y[:] = [float(x) for x in np.asarray(basis_y, np.float32).reshape(3)]
        s.sun_rgb[:] = [float(x) for x in sun_rgb]
        s.flags = int(flags)
        return s


LIGHT_POINT, LIGHT_COSINE, LIGHT_INVSQ = 1, 2, 4      # LH_LIGHT_*: v is a position (else the direction towards the light); weight by the cosine; divide by the squared distance
LIGHTS_MAX = 31                                        # LH_LIGHTS_MAX: a mask of 32 set bits would be AO_NO_HIT, the mark of a traced miss


class Light(C.Structure):
    """lh_light_t (56 bytes): a directional light (v: the direction TOWARDS it) or, with LIGHT_POINT, a point light (v: its position), its
    colour and flags (LIGHT_COSINE, LIGHT_INVSQ -- the latter for point lights only); reserved must stay 0"""
    _fields_ = [("v", C.c_double * 3), ("rgb", C.c_double * 3), ("flags", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, v=(0.0, 1.0, 0.0), rgb=(1.0, 1.0, 1.0), flags=0, reserved=0):
        super().__init__((C.c_double * 3)(*[float(x) for x in v]), (C.c_double * 3)(*[float(x) for x in rgb]), int(flags), int(reserved))


class LightsParams(C.Structure):
    """lh_lights_params_t: the origin offset of the shadow rays along Ns (default: LH_LIGHTS_DEFAULTS, contribution_from_sunlight's 1e-5)"""
    _fields_ = [("eps", C.c_double)]

    def __init__(self, eps=1.0e-5):
        super().__init__(float(eps))


def _light_array(what, lights):
    """a sequence of Light -> (a ctypes array of them, or None for an empty one; its length): the C call refuses what the rule does not accept"""
    lights = list(lights)
    for x in lights:
        if not isinstance(x, Light):
            raise ValueError("%s: lights must be a sequence of Light" % what)
    return ((Light * len(lights))(*lights) if lights else None), len(lights)


class PtSinkStruct(C.Structure):
    """lh_pt_sink_t (96 bytes): ten record arrays and the counts on the device, each may be NULL, and the capacity in records"""
    _fields_ = [(k, C.c_void_p) for k in ("d_path", "d_depth", "d_org", "d_dir", "d_prim", "d_t", "d_u", "d_v", "d_thr", "d_direct", "d_counts")] + \
               [("capacity", C.c_size_t)]


class PtSink:
    """the path-vertex sink of render_pt_tile_lit / render_pt_bands_lit: torch tensors for `capacity` records and the counts of `max_vertices`
    bounces on `device` -- path, depth, prim: int32 (uint32 bits); org, dir: float64 [capacity, 3]; t, u, v: float64; thr, direct: float32
    [capacity, 3]; counts: int32 [max_vertices].  fields: the record arrays to allocate (default: all); an absent one is None and is skipped.
    After a call, total() is the number of records the pass had, written or not (the caller compares it with the capacity) and records()
    the written ones as numpy arrays."""
    FIELDS = ("path", "depth", "org", "dir", "prim", "t", "u", "v", "thr", "direct")

    def __init__(self, capacity, max_vertices, device=0, fields=None):
        import torch
        dev = torch.device("cuda", device)
        self.capacity, self.max_vertices = int(capacity), int(max_vertices)
        want = self.FIELDS if fields is None else tuple(fields)
        n = self.capacity
        shapes = {"path": ((n,), torch.int32), "depth": ((n,), torch.int32), "prim": ((n,), torch.int32), "org": ((n, 3), torch.float64),
                  "dir": ((n, 3), torch.float64), "t": ((n,), torch.float64), "u": ((n,), torch.float64), "v": ((n,), torch.float64),
                  "thr": ((n, 3), torch.float32), "direct": ((n, 3), torch.float32)}
        for k in self.FIELDS:
            setattr(self, k, torch.zeros(shapes[k][0], dtype=shapes[k][1], device=dev) if k in want else None)
        self.counts = torch.zeros((self.max_vertices,), dtype=torch.int32, device=dev)

    def struct(self):
        s = PtSinkStruct()
        for k in self.FIELDS + ("counts",):
            t = getattr(self, k)
            setattr(s, "d_" + k, None if t is None else t.data_ptr())
        s.capacity = self.capacity
        return s

    def total(self):
        return int(self.counts.cpu().numpy().view(np.uint32).astype(np.int64).sum())

    def records(self):
        """-> dict of numpy arrays over the min(total, capacity) written records (path, depth, prim as uint32), plus "counts" (uint32)"""
        n = min(self.total(), self.capacity)
        out = {"counts": self.counts.cpu().numpy().view(np.uint32)}
        for k in self.FIELDS:
            t = getattr(self, k)
            if t is not None:
                a = t[:n].cpu().numpy()
                out[k] = a.view(np.uint32) if a.dtype == np.int32 else a
        return out


AREA_COSINE, AREA_FACING, AREA_INVSQ, AREA_PDF = 1, 2, 4, 8      # LH_AREA_*: the surface cosine; the emitter's cosine, one-sided; 1 / squared distance; ntris x the triangle's area
AREA_LIGHTS_MAX, AREA_SAMPLES_MAX = 31, 1024                     # LH_AREA_LIGHTS_MAX, LH_AREA_SAMPLES_MAX


class AreaLight(C.Structure):
    """lh_area_light_t (40 bytes): the run [first_tri, first_tri + ntris) of the accelerator's emitter table (set_emitters), its colour and
    flags (AREA_COSINE, AREA_FACING, AREA_INVSQ, AREA_PDF); reserved must stay 0"""
    _fields_ = [("first_tri", C.c_uint32), ("ntris", C.c_uint32), ("rgb", C.c_double * 3), ("flags", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, first_tri=0, ntris=1, rgb=(1.0, 1.0, 1.0), flags=0, reserved=0):
        super().__init__(int(first_tri), int(ntris), (C.c_double * 3)(*[float(x) for x in rgb]), int(flags), int(reserved))


class AreaParams(C.Structure):
    """lh_area_params_t (24 bytes): the origin offset along Ns, the bound of a traced ray (0 < bound <= 1; a little below 1 where the emitters
    are scene geometry too), the samples per light (defaults: LH_AREA_DEFAULTS); reserved must stay 0"""
    _fields_ = [("eps", C.c_double), ("bound", C.c_double), ("nsamples", C.c_int32), ("reserved", C.c_uint32)]

    def __init__(self, eps=1.0e-5, bound=1.0, nsamples=16, reserved=0):
        super().__init__(float(eps), float(bound), int(nsamples), int(reserved))


def _area_array(what, lights):
    """a sequence of AreaLight -> (a ctypes array of them, or None for an empty one; its length): the C call refuses what the rule does not accept"""
    lights = list(lights)
    for x in lights:
        if not isinstance(x, AreaLight):
            raise ValueError("%s: lights must be a sequence of AreaLight" % what)
    return ((AreaLight * len(lights))(*lights) if lights else None), len(lights)


class PtLights(C.Structure):
    """lh_pt_lights_t (48 bytes): the delta lights of render_pt_tile_lit (lights, nlights, params) and the area lights of area_lights_device (area,
    narea, area_params) for render_pt_tile_lights / render_pt_bands_lights; the reserved words must stay 0.  Holds pointers only: the arrays
    they point to must outlive the call (HipAccel._lights_args keeps them)"""
    _fields_ = [("lights", C.POINTER(Light)), ("nlights", C.c_int32), ("reserved0", C.c_uint32), ("params", C.POINTER(LightsParams)),
                ("area", C.POINTER(AreaLight)), ("narea", C.c_int32), ("reserved1", C.c_uint32), ("area_params", C.POINTER(AreaParams))]


class WhittedParams(C.Structure):
    """lh_whitted_params_t: origin offset, relative refractive index and depth limit of the refraction chain (defaults:
    LH_WHITTED_DEFAULTS, the constants of whitted.c); reserved must stay 0"""
    _fields_ = [("eps", C.c_double), ("eta", C.c_double), ("max_depth", C.c_int), ("reserved", C.c_int)]

    def __init__(self, eps=1.0e-7, eta=1.33, max_depth=8, reserved=0):
        super().__init__(float(eps), float(eta), int(max_depth), int(reserved))


WHITTED_CUT = 0x80000000          # LH_WHITTED_CUT: the chain was cut at the depth limit (the low bits: that depth)

# lh_beam_set_t (include/lucille_hip.h): a beam as lucille's ri_beam_set leaves it -- 232 bytes
BEAM_SET_DTYPE = np.dtype([("org", np.float64, (3,)), ("dir", np.float64, (4, 3)), ("normal", np.float64, (4, 3)),
                           ("dominant_axis", np.int32), ("dirsign", np.int32, (3,))])

# every symbol include/lucille_hip.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "lh_device_count", "lh_last_error", "lh_accel_create", "lh_accel_add_mesh", "lh_accel_add_mesh_device", "lh_accel_update_mesh_device", "lh_accel_recommit", "lh_accel_danger_list", "lh_accel_commit", "lh_accel_wait_exact", "lh_accel_ref_tree", "lh_accel_tree_image",
    "lh_accel_destroy", "lh_accel_info", "lh_accel_prim_lookup", "lh_accel_intersect1", "lh_accel_combine_statistics", "lh_accel_intersect_diag_host", "lh_accel_intersect_diag_device",
    "lh_accel_intersect_host", "lh_accel_intersect_device", "lh_accel_intersect_host_ex", "lh_accel_intersect_device_ex", "lh_accel_intersect_device_indexed", "lh_accel_intersect_device_tmax", "lh_accel_intersect_host_tmax", "lh_accel_compact_device", "lh_accel_intersect_device_counted", "lh_accel_last_retraced", "lh_accel_dump_node_bytes", "lh_accel_order_statistics",
    "lh_accel_set_grid", "lh_accel_set_param", "lh_accel_export", "lh_accel_set_normals", "lh_render_primary_rays",
    "lh_render_ao_tile", "lh_render_ao_tile_host", "lh_render_ao_bands", "lh_render_scratch", "lh_accel_beam_visibility_host", "lh_accel_beam_visibility_device", "lh_accel_beam_visibility_set_host", "lh_accel_beam_raster_host", "lh_accel_beam_raster_device", "lh_accel_beam_raster_set_host", "lh_render_pt_tile",
    "lh_accel_trace_statistics", "lh_accel_statistics", "lh_accel_slot_statistics",
    "lh_render_ao_frame_host", "lh_rib_load", "lh_rib_free", "lh_rib_last_error", "lh_rib_info", "lh_rib_messages",
    "lh_rib_mesh", "lh_accel_add_rib_scene", "lh_hdr_write",
    "lh_accel_set_material", "lh_accel_set_environment", "lh_render_pt_tile2", "lh_render_pt_bands", "lh_accel_set_attribute", "lh_accel_set_normals_device", "lh_accel_set_attribute_device",
    "lh_accel_state_build_device", "lh_accel_state_build_host", "lh_accel_ao_device", "lh_accel_ao_host", "lh_accel_ao_rays_device",
    "lh_accel_dirt_device", "lh_accel_dirt_host", "lh_render_dirt_tile",
    "lh_accel_env_device", "lh_accel_env_host", "lh_render_env_tile", "lh_accel_environment_device", "lh_accel_environment_host",
    "lh_sky_from_site", "lh_accel_set_sky", "lh_accel_sky_device", "lh_accel_sky_host",
    "lh_accel_lights_device", "lh_accel_lights_host", "lh_accel_light_rays_device", "lh_render_lights_tile",
    "lh_render_pt_tile_lit", "lh_render_pt_bands_lit", "lh_render_pt_tile_lights", "lh_render_pt_bands_lights",
    "lh_accel_set_emitters", "lh_accel_area_lights_device", "lh_accel_area_lights_host", "lh_accel_area_light_rays_device", "lh_render_area_lights_tile",
    "lh_accel_whitted_rays_device", "lh_accel_whitted_device", "lh_accel_whitted_host", "lh_render_whitted_tile",
    "lh_accel_set_texture", "lh_accel_set_texture_device", "lh_accel_texture_device", "lh_accel_texture_host", "lh_multi_set_texture",
    "lh_multi_create", "lh_multi_destroy", "lh_multi_ndevices", "lh_multi_accel", "lh_multi_add_mesh", "lh_multi_set_normals",
    "lh_multi_add_rib_scene", "lh_multi_commit", "lh_multi_set_material", "lh_multi_set_environment", "lh_multi_intersect_host",
    "lh_multi_render_ao_frame_host", "lh_multi_render_pt_frame_host",
    "lh_synth_soup_triangles", "lh_synth_soup_rays", "lh_synth_tessellate", "lh_synth_skip",
    "lh_dist_unique_id", "lh_dist_init", "lh_dist_init_file", "lh_dist_destroy", "lh_dist_rank", "lh_dist_world", "lh_dist_transport",
    "lh_dist_barrier", "lh_dist_host_barrier", "lh_dist_broadcast", "lh_dist_gather", "lh_dist_pack_records16", "lh_dist_broadcast_scene", "lh_dist_render_ao_frame_host",
]

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    try:                      # torch ships its own HIP runtime: let it initialise first when both live in one process
        import torch          # noqa: F401
    except Exception:         # noqa: BLE001 -- the library itself does not need torch
        pass
    if not os.path.exists(path):
        raise LucilleHipError(
            "%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C %s` "
            "(there is no CPU fallback)" % (path, CSRC))
    L = C.CDLL(path)
    vp, sz, i32, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    L.lh_device_count.restype = i32
    L.lh_last_error.restype = C.c_char_p
    L.lh_accel_create.argtypes = [C.POINTER(vp), i32]
    L.lh_accel_add_mesh.argtypes = [vp, u32, vp, sz, u32, vp]
    L.lh_accel_add_mesh_device.argtypes = [vp, u32, vp, i32, sz, u32, vp, vp]
    if hasattr(L, "lh_accel_recommit"):                  # an older library under LH_LIBRARY (A/B runs in tools/) has no updatable meshes
        L.lh_accel_update_mesh_device.argtypes = [vp, u32, u32, vp, i32, sz, vp]
        L.lh_accel_recommit.argtypes = [vp, C.POINTER(RecommitInfo)]
        L.lh_accel_danger_list.argtypes = [vp, C.POINTER(u32), C.POINTER(u32 * 3), C.POINTER(u32), vp]
    L.lh_accel_commit.argtypes = [vp, i32]
    L.lh_accel_wait_exact.argtypes = [vp]
    L.lh_accel_ref_tree.argtypes = [vp, C.POINTER(C.c_uint32), vp, vp]
    if hasattr(L, "lh_accel_tree_image"):                # (an older library under LH_LIBRARY has no tree image)
        L.lh_accel_tree_image.argtypes = [vp, C.POINTER(TreeImage), vp, vp, vp, vp]
    L.lh_accel_destroy.argtypes = [vp]
    L.lh_accel_destroy.restype = None
    L.lh_accel_info.argtypes = [vp, C.POINTER(AccelInfo)]
    L.lh_accel_prim_lookup.argtypes = [vp, u32, C.POINTER(u32), C.POINTER(u32)]
    L.lh_accel_intersect1.argtypes = [vp, vp, vp, C.POINTER(u32), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.lh_accel_intersect_host.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, i32]
    L.lh_accel_intersect_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]
    L.lh_accel_intersect_host_ex.argtypes = [vp, sz, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32]
    L.lh_accel_intersect_device_ex.argtypes = [vp, sz, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    L.lh_accel_intersect_device_indexed.argtypes = [vp, sz, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, sz, vp, vp]
    L.lh_accel_compact_device.argtypes = [sz, i32, vp, vp, i32, vp, sz, vp, vp, vp, vp]
    L.lh_accel_intersect_device_tmax.argtypes = [vp, sz, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, sz, vp, vp]
    L.lh_accel_intersect_host_tmax.argtypes = [vp, sz, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32]
    L.lh_accel_last_retraced.argtypes = [vp]; L.lh_accel_last_retraced.restype = C.c_uint64
    L.lh_accel_dump_node_bytes.argtypes = [vp]
    if hasattr(L, "lh_accel_order_statistics"):          # an older library under LH_LIBRARY (A/B runs in tools/) has no ordered dumps
        L.lh_accel_order_statistics.argtypes = [vp, C.POINTER(C.c_uint64), i32]
    L.lh_accel_intersect_device_counted.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, i32, i32,
                                                    C.POINTER(C.c_uint64)]
    L.lh_accel_set_grid.argtypes = [vp, i32]
    L.lh_accel_set_param.argtypes = [vp, C.c_char_p, i32]
    L.lh_accel_trace_statistics.argtypes = [vp, i32]
    L.lh_accel_statistics.argtypes = [vp, C.POINTER(C.c_uint64), i32]
    L.lh_accel_slot_statistics.argtypes = [vp, C.POINTER(C.c_uint64), i32]
    L.lh_accel_export.argtypes = [vp, vp, vp]
    L.lh_accel_set_normals.argtypes = [vp, u32, vp, sz, i32]
    L.lh_accel_set_normals_device.argtypes = [vp, u32, u32, vp, i32, sz, i32, vp]
    L.lh_accel_set_attribute_device.argtypes = [vp, u32, i32, u32, vp, i32, sz, vp]
    L.lh_render_primary_rays.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, vp, vp, vp]
    L.lh_render_ao_tile.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, C.c_uint64, vp, vp,
                                    C.POINTER(TileStats), vp]
    L.lh_render_ao_bands.argtypes = [vp, C.POINTER(Camera), i32, C.POINTER(i32), i32, i32, i32, C.c_uint64, vp, C.POINTER(TileStats), vp]
    L.lh_render_scratch.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz)]
    L.lh_render_pt_tile.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, i32, i32, C.c_float,
                                    C.POINTER(C.c_float * 3), C.c_uint64, vp, C.POINTER(PtStats), vp]
    L.lh_accel_beam_visibility_host.argtypes = [vp, sz, vp, vp, vp]
    L.lh_accel_beam_visibility_device.argtypes = [vp, sz, vp, vp, vp, vp]
    L.lh_accel_beam_raster_host.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
    L.lh_accel_beam_raster_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]
    L.lh_accel_set_material.argtypes = [vp, u32, C.POINTER(Material)]
    L.lh_accel_set_environment.argtypes = [vp, C.POINTER(Environment)]
    L.lh_render_pt_bands.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(Material), C.c_uint64, vp,
                                     C.POINTER(PtStats), vp]
    L.lh_render_pt_tile2.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, i32, i32, i32, C.c_uint64, vp,
                                     C.POINTER(PtStats), vp]
    L.lh_accel_set_attribute.argtypes = [vp, u32, i32, vp, sz, u32]
    L.lh_accel_state_build_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]
    L.lh_accel_state_build_host.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
    L.lh_accel_ao_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, i32, C.c_uint64, vp, vp, vp, sz, vp, vp, vp, vp]
    L.lh_accel_ao_host.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, i32, C.c_uint64, vp, vp, sz, vp, vp]
    L.lh_accel_ao_rays_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, i32, C.c_uint64, vp, vp, vp, vp, vp, vp, sz, vp]
    dpp = C.POINTER(DirtParams)
    L.lh_accel_dirt_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, i32, dpp, C.c_uint64, vp, vp, vp, sz, vp, vp, vp, vp]
    L.lh_accel_dirt_host.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, i32, dpp, C.c_uint64, vp, vp, sz, vp, vp]
    L.lh_render_dirt_tile.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, dpp, C.c_uint64, vp, vp,
                                      C.POINTER(TileStats), vp]
    if hasattr(L, "lh_accel_env_device"):                # an older library under LH_LIBRARY (A/B runs in tools/) has no environment gather
        epp = C.POINTER(EnvParams)
        L.lh_accel_env_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, i32, epp, C.c_uint64, vp, vp, vp, sz, vp, vp, vp, vp]
        L.lh_accel_env_host.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, i32, epp, C.c_uint64, vp, vp, sz, vp, vp]
        L.lh_render_env_tile.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, epp, C.c_uint64, vp, vp,
                                         C.POINTER(TileStats), vp]
        L.lh_accel_environment_device.argtypes = [vp, sz, vp, vp, vp]
        L.lh_accel_environment_host.argtypes = [vp, sz, vp, vp]
    if hasattr(L, "lh_accel_set_sky"):                   # an older library under LH_LIBRARY (A/B runs in tools/) has no sun-and-sky light
        L.lh_sky_from_site.argtypes = [C.POINTER(Sky), C.c_float, C.c_float, C.c_float, i32, C.c_float, C.c_float]
        L.lh_accel_set_sky.argtypes = [vp, C.POINTER(Sky)]
        L.lh_accel_sky_device.argtypes = [vp, sz, vp, vp, vp]
        L.lh_accel_sky_host.argtypes = [vp, sz, vp, vp]
    if hasattr(L, "lh_accel_lights_device"):             # an older library under LH_LIBRARY (A/B runs in tools/) has no light stage
        lp, lpp = C.POINTER(Light), C.POINTER(LightsParams)
        L.lh_accel_lights_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, lp, i32, lpp, vp, sz, vp, vp, vp, vp]
        L.lh_accel_lights_host.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, lp, i32, lpp, vp, vp]
        L.lh_accel_light_rays_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, lp, i32, lpp, vp, vp, vp, vp, vp, sz, vp]
        L.lh_render_lights_tile.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, lp, i32, lpp, vp, C.POINTER(TileStats), vp]
    if hasattr(L, "lh_render_pt_tile_lit"):              # an older library under LH_LIBRARY (A/B runs in tools/) has no lit path tracer
        lp, lpp, skp = C.POINTER(Light), C.POINTER(LightsParams), C.POINTER(PtSinkStruct)
        L.lh_render_pt_tile_lit.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, i32, i32, i32, lp, i32, lpp, skp, C.c_uint64, vp,
                                            C.POINTER(PtStats), vp]
        L.lh_render_pt_bands_lit.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(Material), lp, i32, lpp, skp,
                                             C.c_uint64, vp, C.POINTER(PtStats), vp]
    if hasattr(L, "lh_render_pt_tile_lights"):           # an older library under LH_LIBRARY (A/B runs in tools/) has no area lights at path vertices
        plp, skp = C.POINTER(PtLights), C.POINTER(PtSinkStruct)
        L.lh_render_pt_tile_lights.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, i32, i32, i32, plp, skp, C.c_uint64, vp,
                                               C.POINTER(PtStats), vp]
        L.lh_render_pt_bands_lights.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(Material), plp, skp,
                                                C.c_uint64, vp, C.POINTER(PtStats), vp]
    if hasattr(L, "lh_accel_area_lights_device"):       # an older library under LH_LIBRARY (A/B runs in tools/) has no area-light stage
        ap, app, u64 = C.POINTER(AreaLight), C.POINTER(AreaParams), C.c_uint64
        L.lh_accel_set_emitters.argtypes = [vp, vp, sz]
        L.lh_accel_area_lights_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, ap, i32, app, u64, vp, vp, vp, sz, vp, vp, vp, vp]
        L.lh_accel_area_lights_host.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, ap, i32, app, u64, vp, vp, sz, vp, vp]
        L.lh_accel_area_light_rays_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, ap, i32, app, u64, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
        L.lh_render_area_lights_tile.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, ap, i32, app, u64, vp, C.POINTER(TileStats), vp]
    if hasattr(L, "lh_accel_whitted_device"):            # an older library under LH_LIBRARY (A/B runs in tools/) has no refraction chain
        wpp = C.POINTER(WhittedParams)
        L.lh_accel_whitted_rays_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, wpp, vp, sz, vp, vp, vp, vp]
        L.lh_accel_whitted_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, wpp, vp, sz, vp, vp, vp, vp, vp, vp]
        L.lh_accel_whitted_host.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, wpp, vp, vp, vp, vp]
        L.lh_render_whitted_tile.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, wpp, vp, C.POINTER(PtStats), vp]
    if hasattr(L, "lh_accel_set_texture"):               # an older library under LH_LIBRARY (the parent's build in tools/tex_frames.py) has no textures
        L.lh_accel_set_texture.argtypes = [vp, u32, vp, i32, i32]
        L.lh_accel_set_texture_device.argtypes = [vp, u32, vp, i32, i32, vp]
        L.lh_accel_texture_device.argtypes = [vp, sz, vp, vp, vp, vp, sz, vp, vp, vp]
        L.lh_accel_texture_host.argtypes = [vp, sz, vp, vp, vp, vp]
        L.lh_multi_set_texture.argtypes = [vp, u32, vp, i32, i32]
    L.lh_multi_create.argtypes = [C.POINTER(vp), i32, C.POINTER(i32)]
    L.lh_multi_destroy.argtypes = [vp]; L.lh_multi_destroy.restype = None
    L.lh_multi_ndevices.argtypes = [vp]
    L.lh_multi_accel.argtypes = [vp, i32]; L.lh_multi_accel.restype = vp
    L.lh_multi_add_mesh.argtypes = [vp, u32, vp, sz, u32, vp]
    L.lh_multi_set_normals.argtypes = [vp, u32, vp, sz, i32]
    L.lh_multi_add_rib_scene.argtypes = [vp, vp]
    L.lh_multi_commit.argtypes = [vp, i32]
    L.lh_multi_set_material.argtypes = [vp, u32, C.POINTER(Material)]
    L.lh_multi_set_environment.argtypes = [vp, C.POINTER(Environment)]
    L.lh_multi_intersect_host.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, i32]
    L.lh_multi_render_ao_frame_host.argtypes = [vp, C.POINTER(Camera), i32, i32, C.c_uint64, i32, vp, C.POINTER(TileStats), vp]
    L.lh_multi_render_pt_frame_host.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, C.c_uint64, i32, vp, C.POINTER(PtStats), vp]
    L.lh_synth_soup_triangles.argtypes = [C.POINTER(C.c_uint64), u32, C.c_double, vp, vp]
    L.lh_synth_soup_triangles.restype = None
    L.lh_synth_soup_rays.argtypes = [C.POINTER(C.c_uint64), sz, vp, vp]
    L.lh_synth_soup_rays.restype = None
    L.lh_synth_skip.argtypes = [C.POINTER(C.c_uint64), C.c_uint64]
    L.lh_synth_skip.restype = None
    L.lh_synth_tessellate.argtypes = [vp, sz, i32, vp]
    L.lh_synth_tessellate.restype = None
    _lib = L
    return L


def device_count():
    return int(lib().lh_device_count())


def _check(rc, what):
    if rc < 0:
        raise LucilleHipError("%s: %s" % (what, lib().lh_last_error().decode()))
    return rc


def _np(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _is_f32(a):
    """a float32 numpy array or torch tensor (the dtype selects the ray format of the batch entry points)"""
    dt = getattr(a, "dtype", None)
    if dt is None:
        return False
    if isinstance(dt, np.dtype):
        return dt == np.float32
    return str(dt) == "torch.float32"


def _rec16_host(n):
    """an (n, 4) uint32 array whose data is 16-byte aligned (lh_rec16_t records)"""
    raw = np.empty(4 * n + 4, np.uint32)
    k = (-raw.ctypes.data % 16) // 4
    return raw[k:k + 4 * n].reshape(n, 4)


def _records_format(records):
    if records not in ("f64", "rec16"):
        raise ValueError("records must be 'f64' or 'rec16', not %r" % (records,))
    return REC16 if records == "rec16" else REC_F64


def _dptr(t):
    """device pointer of a torch tensor (or None)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def _list_args(index, count, what):
    """(index pointer, entries, count pointer) of a device list: `index` an int32 / uint32 tensor of ray ids (or None), `count` a
    one-element int32 / uint32 tensor (or None)"""
    import torch
    words = (torch.int32, getattr(torch, "uint32", torch.int32))
    if index is not None and not (index.is_cuda and index.dtype in words and index.dim() == 1 and index.is_contiguous()):
        raise ValueError("%s: index must be a contiguous 1-d int32 / uint32 device tensor" % what)
    if count is not None and not (count.is_cuda and count.dtype in words and count.numel() == 1):
        raise ValueError("%s: count must be a one-element int32 / uint32 device tensor" % what)
    return _dptr(index), (0 if index is None else int(index.numel())), _dptr(count)


def _tmax_device(tmax, org, what):
    """a per-ray bound tensor of a device batch: the rays' dtype and device, shape [n], contiguous"""
    if not (hasattr(tmax, "is_cuda") and tmax.is_cuda and tmax.device == org.device and tmax.dtype == org.dtype
            and tmax.dim() == 1 and tmax.shape[0] == org.shape[0] and tmax.is_contiguous()):
        raise ValueError("%s: tmax must be a contiguous device tensor of the rays' dtype and shape [n]" % what)
    return tmax


def compact(records_or_occluded, select, index=None, count=None, out=None, stream=None):
    """lh_accel_compact_device: the ids of the records that `select` (SELECT_HIT / SELECT_MISS over closest-hit records -- the prim
    tensor [n] or the rec16 tensor [n, 4], int32; SELECT_OCCLUDED / SELECT_UNOCCLUDED over the uint8 any-hit bytes [n]) keeps, in the
    order of the input list (`index` / `count` as for HipAccel.intersect_device; neither: all n records).  Returns (index, count):
    an int32 tensor with room for every candidate whose first count[0] entries are the list, and the one-element int32 count --
    both on the device, nothing is read back; pass them to intersect_device(index=..., count=...).  out: such a pair to fill; it
    must not alias or overlap `index` / `count` (the call refuses: to compact a list again, alternate between two pairs)."""
    import torch
    r = records_or_occluded
    assert r.is_cuda and r.is_contiguous()
    closest = select in (SELECT_HIT, SELECT_MISS)
    if closest:
        if r.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not (r.dim() == 1 or (r.dim() == 2 and r.shape[1] == 4)):
            raise ValueError("compact: closest-hit records are an int32 prim tensor [n] or a rec16 tensor [n, 4]")
        rf = REC16 if r.dim() == 2 else REC_F64
    else:
        if r.dtype != torch.uint8 or r.dim() != 1:
            raise ValueError("compact: any-hit records are a uint8 tensor [n]")
        rf = REC_F64
    n = int(r.shape[0])
    ip, ni, cp = _list_args(index, count, "compact")
    if index is None and count is not None:
        ni = n
    cand = ni if (index is not None or count is not None) else n
    if out is None:
        out = (torch.empty(cand, dtype=torch.int32, device=r.device), torch.empty(1, dtype=torch.int32, device=r.device))
    oi, oc = out
    assert oi.is_cuda and oc.is_cuda and oi.is_contiguous() and oi.numel() >= cand and oc.numel() == 1
    if stream is None:
        stream = torch.cuda.current_stream(r.device).cuda_stream
    with torch.cuda.device(r.device):
        _check(lib().lh_accel_compact_device(n, rf, _dptr(r) if closest else None, None if closest else _dptr(r), select,
                                             ip, ni, cp, _dptr(oi), _dptr(oc), C.c_void_p(stream)), "lh_accel_compact_device")
    return out


def _device_out(n, dev, mode, rf, out):
    """the output tensors of a device batch (allocated when `out` is None) and their places in the C call: (out, prim, t, u, v, occ)"""
    import torch
    if out is None:
        if mode == MODE_CLOSEST and rf == REC16:
            out = (torch.empty((n, 4), dtype=torch.int32, device=dev),)
        elif mode == MODE_CLOSEST:
            out = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float64, device=dev),
                   torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev))
        else:
            out = (torch.empty(n, dtype=torch.uint8, device=dev),)
    if mode == MODE_CLOSEST and rf == REC16:
        return out, out[0], None, None, None, None
    if mode == MODE_CLOSEST:
        prim, t, u, v = out
        return out, prim, t, u, v, None
    return out, None, None, None, None, out[0]


def _host_out(n, mode, rf):
    """the output arrays of a host batch, allocated here, and their places in the C call: (what the method returns, prim, t, u, v, occ)"""
    if mode == MODE_CLOSEST and rf == REC16:
        rec = _rec16_host(n)
        return rec, rec.ctypes.data, None, None, None, None
    if mode == MODE_CLOSEST:
        out = (np.empty(n, np.uint32), np.empty(n), np.empty(n), np.empty(n))
        return (out,) + tuple(x.ctypes.data for x in out) + (None,)
    occ = np.empty(n, np.uint8)
    return occ, None, None, None, None, occ.ctypes.data


_live = weakref.WeakSet()


@atexit.register
def _close_all():
    # device memory must be released while the HIP runtime is still alive
    for a in list(_live):
        a.close()


class HipAccel:
    """One committed accelerator == the `void *accel` the reference's vtable carries."""

    def __init__(self, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        _check(self.L.lh_accel_create(C.byref(self.h), int(device)), "lh_accel_create")
        self.device = int(device)
        self.committed = False
        self._npos = []            # vertex count per added mesh (set_normals validates against it)
        self._env = None           # what set_environment was last given (render.render_pt_frame_sharded restores it)
        _live.add(self)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.lh_accel_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- build ------------------------------------------------------------
    def add_mesh(self, positions, indices):
        """positions: [npos,3] (packed xyz) or [npos,4] (lucille's ri_vector_t) float64"""
        P = _np(positions, np.float64)
        if P.ndim != 2 or P.shape[1] not in (3, 4):
            raise ValueError("positions must be [n,3] or [n,4]")
        I = _np(indices, np.uint32).reshape(-1)
        _check(self.L.lh_accel_add_mesh(self.h, P.shape[0], P.ctypes.data, P.shape[1] * 8, I.shape[0],
                                        I.ctypes.data), "lh_accel_add_mesh")
        self._npos.append(P.shape[0])

    def add_mesh_device(self, positions, indices, stream=None):
        """lh_accel_add_mesh_device: a mesh whose arrays live on the accelerator's device.  positions: a CUDA tensor (n, 3), or a
        strided view (n, >= 3) whose rows are the vertices (element stride 1 along a row; the byte stride between rows is taken
        from the tensor), float64 or float32 -- a float32 vertex is the float64 vertex it widens to; indices: a contiguous CUDA
        int32 tensor (its bits are read as uint32; uint32 where torch has it), three per triangle.  The arrays are read by copies
        enqueued on `stream` (a torch.cuda.Stream, a raw stream handle, or None: torch's current stream) before this returns:
        they may be overwritten or freed in stream order afterwards.  commit() then flattens and builds on the device."""
        import torch
        P, I = positions, indices
        if not (isinstance(P, torch.Tensor) and isinstance(I, torch.Tensor) and P.is_cuda and I.is_cuda):
            raise ValueError("add_mesh_device: positions and indices must be CUDA torch tensors (host arrays: add_mesh)")
        if P.device.index != self.device or I.device.index != self.device:
            raise ValueError("add_mesh_device: the tensors must live on the accelerator's device %d" % self.device)
        if P.dtype not in (torch.float64, torch.float32):
            raise ValueError("add_mesh_device: positions must be float64 or float32, not %s" % P.dtype)
        if P.dim() != 2 or P.shape[1] < 3 or (P.shape[0] > 1 and P.stride(0) < 3) or P.stride(1) != 1:
            raise ValueError("add_mesh_device: positions must be (n, 3) or a strided view (n, >= 3) with contiguous rows")
        if I.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not I.is_contiguous():
            raise ValueError("add_mesh_device: indices must be a contiguous int32 / uint32 tensor")
        if P.shape[0] >= 1 << 32 or I.numel() >= 1 << 32:
            raise ValueError("add_mesh_device: vertex and index counts are 32-bit")
        fmt = POS_F32 if P.dtype == torch.float32 else POS_F64
        stride = (P.stride(0) if P.shape[0] > 1 else P.shape[1]) * P.element_size()
        if stream is None:
            stream = torch.cuda.current_stream(P.device)
        stream = getattr(stream, "cuda_stream", stream)
        with torch.cuda.device(P.device):
            _check(self.L.lh_accel_add_mesh_device(self.h, int(P.shape[0]), _dptr(P) if P.shape[0] else None, fmt, int(stride), int(I.numel()),
                                                   _dptr(I) if I.numel() else None, C.c_void_p(stream)), "lh_accel_add_mesh_device")

    def set_normals(self, mesh, normals, two_side=0):
        N = _np(normals, np.float64) if normals is not None else None
        if int(mesh) < 0 or int(mesh) >= len(self._npos):
            raise ValueError("set_normals: mesh %d was not added" % int(mesh))
        if N is not None and (N.ndim != 2 or N.shape[1] not in (3, 4) or N.shape[0] != self._npos[int(mesh)]):
            # the C ABI reads one normal per vertex of the mesh: a short array would be read past its end
            raise ValueError("normals must be [%d,3] or [%d,4] (one per vertex of mesh %d)"
                             % (self._npos[int(mesh)], self._npos[int(mesh)], int(mesh)))
        _check(self.L.lh_accel_set_normals(self.h, int(mesh), N.ctypes.data if N is not None else None,
                                           (N.shape[1] * 8) if N is not None else 24, int(two_side)),
               "lh_accel_set_normals")

    def _device_rows(self, what, T, ncomp):
        """the checks set_normals_device / set_attribute_device make before they call C: (count, pointer, format, byte stride)"""
        import torch
        if T is None:
            return 0, None, POS_F64, 8 * ncomp
        if not (isinstance(T, torch.Tensor) and T.is_cuda):
            raise ValueError("%s: the array must be a CUDA torch tensor, or None to remove it (host arrays: the host form)" % what)
        if T.device.index != self.device:
            raise ValueError("%s: the tensor must live on the accelerator's device %d" % (what, self.device))
        if T.dtype not in (torch.float64, torch.float32):
            raise ValueError("%s: the tensor must be float64 or float32, not %s" % (what, T.dtype))
        if T.dim() != 2 or T.shape[1] < ncomp or (T.shape[0] > 1 and T.stride(0) < ncomp) or T.stride(1) != 1:
            raise ValueError("%s: the tensor must be (n, %d) or a strided view (n, >= %d) with contiguous rows" % (what, ncomp, ncomp))
        if T.shape[0] >= 1 << 32:
            raise ValueError("%s: counts are 32-bit" % what)
        stride = (T.stride(0) if T.shape[0] > 1 else T.shape[1]) * T.element_size()
        return int(T.shape[0]), (_dptr(T) if T.shape[0] else None), (POS_F32 if T.dtype == torch.float32 else POS_F64), int(stride)

    def _stream_handle(self, stream):
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        return C.c_void_p(getattr(stream, "cuda_stream", stream))

    def set_normals_device(self, mesh, normals, two_side=0, stream=None):
        """lh_accel_set_normals_device: per-vertex normals of device mesh `mesh` (add order) from a CUDA tensor (n, 3) or a strided
        view (n, >= 3) with contiguous rows, float64 or float32, one row per vertex; None removes them and sets two_side alone.
        Read by a copy enqueued on `stream` (as add_mesh_device) before this returns."""
        import torch
        n, ptr, fmt, stride = self._device_rows("set_normals_device", normals, 3)
        with torch.cuda.device(self.device):
            _check(self.L.lh_accel_set_normals_device(self.h, int(mesh), n, ptr, fmt, stride, int(two_side), self._stream_handle(stream)),
                   "lh_accel_set_normals_device")

    def set_attribute_device(self, mesh, kind, data, stream=None):
        """lh_accel_set_attribute_device: colours, tangents, binormals (3 per vertex), texture coordinates (2 per vertex) or
        unshared texture coordinates (2 per index) of device mesh `mesh` from a CUDA tensor, as set_normals_device; None removes."""
        import torch
        ncomp = 2 if int(kind) in (ATTR_TEXCOORD, ATTR_TEXCOORD_UNSHARED) else 3
        n, ptr, fmt, stride = self._device_rows("set_attribute_device", data, ncomp)
        with torch.cuda.device(self.device):
            _check(self.L.lh_accel_set_attribute_device(self.h, int(mesh), int(kind), n, ptr, fmt, stride, self._stream_handle(stream)),
                   "lh_accel_set_attribute_device")

    def update_mesh_device(self, mesh, positions, stream=None):
        """lh_accel_update_mesh_device: new positions for device mesh `mesh` (add order) of a committed accelerator that set
        set_param("updatable", 1) before its commit.  positions: as add_mesh_device takes them, one row per vertex of the mesh; the
        dtype and the stride may differ from the add's.  Read by a copy enqueued on `stream` before this returns.  Only staged:
        queries answer from the old geometry until recommit() returns."""
        import torch
        if positions is None:
            raise ValueError("update_mesh_device: positions must be a CUDA torch tensor")
        n, ptr, fmt, stride = self._device_rows("update_mesh_device", positions, 3)
        with torch.cuda.device(self.device):
            _check(self.L.lh_accel_update_mesh_device(self.h, int(mesh), n, ptr, fmt, stride, self._stream_handle(stream)),
                   "lh_accel_update_mesh_device")

    def recommit(self):
        """lh_accel_recommit: rebuild, in place, from what update_mesh_device / set_normals_device / set_attribute_device staged since
        the last (re-)commit -> info() plus "flattened", "rebuilt_trees", "regathered" (what was redone) and "recommit_seconds".
        Synchronous; waits for the device before it swaps the new scene in.  On failure (LucilleHipError) the accelerator answers from
        the old geometry and what was staged stays staged."""
        r = RecommitInfo()
        _check(self.L.lh_accel_recommit(self.h, C.byref(r)), "lh_accel_recommit")
        out = self.info()
        out.update(flattened=int(r.flattened), rebuilt_trees=int(r.rebuilt_trees), regathered=int(r.regathered), recommit_seconds=float(r.seconds))
        return out

    def commit(self, build_threads=0, on_device=False, build=None):
        """build: "device" (= on_device: both trees on the GPU, LH_BUILD_ON_DEVICE), "host" (LH_BUILD_ON_HOST; a thread count
        in build_threads also means the host), None / "auto": the library chooses by the size of the scene"""
        if build not in (None, "auto", "host", "device"):
            raise ValueError("build must be 'auto', 'host' or 'device'")
        code = -2 if (on_device or build == "device") else (int(build_threads) if int(build_threads) > 0 else (-3 if build == "host" else 0))
        _check(self.L.lh_accel_commit(self.h, code), "lh_accel_commit")
        self.committed = True
        return self.info()

    def wait_exact(self):
        _check(self.L.lh_accel_wait_exact(self.h), "lh_accel_wait_exact")

    REF_NODE = np.dtype([("box", "<f8", (2, 6)), ("child", "<i4", (2,)), ("axis", "<i4"), ("is_leaf", "<i4"), ("first", "<u4"),
                         ("count", "<u4"), ("parent", "<i4"), ("depth", "<i4")])

    def ref_tree(self):
        """lucille's own tree as the kernels read it: (nodes [structured, 128 bytes each, root 0], leaf_prims)"""
        nn = C.c_uint32()
        _check(self.L.lh_accel_ref_tree(self.h, C.byref(nn), None, None), "lh_accel_ref_tree")
        nodes = np.zeros(nn.value, dtype=self.REF_NODE)
        prims = np.zeros(self.info()["ntriangles"], dtype=np.uint32)
        _check(self.L.lh_accel_ref_tree(self.h, C.byref(nn), nodes.ctypes.data_as(C.c_void_p), prims.ctypes.data_as(C.c_void_p)), "lh_accel_ref_tree")
        return nodes, prims

    # the record layouts of lh_q4node_t / lh_q8node_t / lh_tri32_t (lh_bvh.h); lh_tri64_t is 9 doubles
    Q4_NODE = np.dtype([("w", "<u4", (4, 3)), ("ref", "<i4", (4,))])
    Q8_NODE = np.dtype([("w", "<u4", (8, 3)), ("ref", "<i4", (8,))])
    TRI32 = np.dtype([("v0", "<f4", (3,)), ("e1", "<f4", (3,)), ("e2", "<f4", (3,)), ("prim", "<u4"), ("ne1", "<f4"), ("ne2", "<f4")])

    def tree_image(self):
        """lh_accel_tree_image: the traversal trees the device holds, read back -> dict of the figures of lh_tree_image_t (scalars; bmin, bmax,
        grid_lo, grid_step as float32 [3]) and the arrays q4nodes (Q4_NODE [nq4]), q8nodes (Q8_NODE [nq8], empty while not resident),
        tri32 (TRI32 [ntris], leaf order) and tri64 (float64 [ntris, 3, 3], primitive-id order)"""
        t = TreeImage()
        _check(self.L.lh_accel_tree_image(self.h, C.byref(t), None, None, None, None), "lh_accel_tree_image")
        q4 = np.zeros(t.nq4, self.Q4_NODE); q8 = np.zeros(t.nq8, self.Q8_NODE)
        t32 = np.zeros(t.ntris, self.TRI32); t64 = np.zeros((t.ntris, 3, 3), np.float64)
        u = TreeImage()
        _check(self.L.lh_accel_tree_image(self.h, C.byref(u), q4.ctypes.data_as(C.c_void_p), q8.ctypes.data_as(C.c_void_p),
                                          t32.ctypes.data_as(C.c_void_p), t64.ctypes.data_as(C.c_void_p)), "lh_accel_tree_image")
        if bytes(u) != bytes(t):
            raise LucilleHipError("lh_accel_tree_image: the scene changed between the two calls")
        out = {k: int(getattr(t, k)) for k in ("ntris", "nlive", "nq4", "q4_depth", "q4_stack", "nq8", "q8_depth", "device_built")}
        for k in ("bmin", "bmax", "grid_lo", "grid_step"):
            out[k] = np.array(list(getattr(t, k)), np.float32)
        out["scene_r"] = np.float32(t.scene_r)
        out.update(q4nodes=q4, q8nodes=q8, tri32=t32, tri64=t64)
        return out

    def danger_list(self):
        """lh_accel_danger_list -> (leaves behind the device's box or 0 = every ray beyond the cap, the box's three words, the host list [n, 6])"""
        nd, nh, w = C.c_uint32(), C.c_uint32(), (C.c_uint32 * 3)()
        boxes = np.zeros((16, 6))
        _check(self.L.lh_accel_danger_list(self.h, C.byref(nd), C.byref(w), C.byref(nh), boxes.ctypes.data), "lh_accel_danger_list")
        return int(nd.value), tuple(int(x) for x in w), boxes[:nh.value].copy()

    def info(self):
        s = AccelInfo()
        _check(self.L.lh_accel_info(self.h, C.byref(s)), "lh_accel_info")
        return {k: getattr(s, k) for k, _ in s._fields_}

    def prim_lookup(self, prim):
        m, i = C.c_uint32(), C.c_uint32()
        _check(self.L.lh_accel_prim_lookup(self.h, int(prim), C.byref(m), C.byref(i)), "lh_accel_prim_lookup")
        return int(m.value), int(i.value)

    def set_param(self, name, value):
        _check(self.L.lh_accel_set_param(self.h, name.encode(), int(value)), "lh_accel_set_param")

    def set_grid(self, blocks):
        _check(self.L.lh_accel_set_grid(self.h, int(blocks)), "lh_accel_set_grid")

    def export(self):
        inf = self.info()
        nodes = np.zeros((inf["nnodes"], 16), np.float32)
        tri32 = np.zeros((inf["ntriangles"], 12), np.float32)
        _check(self.L.lh_accel_export(self.h, nodes.ctypes.data, tri32.ctypes.data), "lh_accel_export")
        return nodes, tri32

    # ---- queries ----------------------------------------------------------
    def intersect_diag(self, org, dr):
        """per-ray traversal diagnostics -> ((prim, t, u, v), diag uint32 [n, 4]: 4-wide node visits, leaf visits, triangle
        records through the fp32 filter, fp64 tests) -- the sequential walk's numbers (ri_bvh_diag_t, bvh.h:103-110)"""
        o = _np(org, np.float64).reshape(-1, 3); d = _np(dr, np.float64).reshape(-1, 3); n = o.shape[0]
        prim = np.empty(n, np.uint32); t = np.empty(n); u = np.empty(n); v = np.empty(n); diag = np.zeros((n, 4), np.uint32)
        self.L.lh_accel_intersect_diag_host.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 7
        _check(self.L.lh_accel_intersect_diag_host(self.h, n, o.ctypes.data, d.ctypes.data, prim.ctypes.data, t.ctypes.data, u.ctypes.data,
                                                   v.ctypes.data, diag.ctypes.data), "lh_accel_intersect_diag_host")
        return (prim, t, u, v), diag

    def intersect_diag_device(self, org, dr, mode=MODE_CLOSEST):
        """CUDA float64 [n,3] rays -> uint32 [n,4] CUDA tensor of the sequential walk's per-ray counts (closest- or any-hit)"""
        import torch
        n = org.shape[0]
        diag = torch.zeros((n, 4), dtype=torch.int32, device=org.device)
        self.L.lh_accel_intersect_diag_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _check(self.L.lh_accel_intersect_diag_device(self.h, n, _dptr(org), _dptr(dr), int(mode), _dptr(diag),
                                                     C.c_void_p(torch.cuda.current_stream(org.device).cuda_stream)), "lh_accel_intersect_diag_device")
        return diag

    def combine_statistics(self, clear=False):
        """(launches, rays) of the coalesced single-ray path since the last clear"""
        o = (C.c_uint64 * 2)()
        self.L.lh_accel_combine_statistics.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        _check(self.L.lh_accel_combine_statistics(self.h, o, 1 if clear else 0), "lh_accel_combine_statistics")
        return int(o[0]), int(o[1])

    def intersect1(self, org, dr):
        o = _np(org, np.float64).reshape(3); d = _np(dr, np.float64).reshape(3)
        p = C.c_uint32(); t = C.c_double(); u = C.c_double(); v = C.c_double()
        hit = _check(self.L.lh_accel_intersect1(self.h, o.ctypes.data, d.ctypes.data, C.byref(p), C.byref(t),
                                                C.byref(u), C.byref(v)), "lh_accel_intersect1")
        return hit, int(p.value), t.value, u.value, v.value

    def intersect_host_tmax(self, org, dr, tmax, mode=MODE_CLOSEST, records="f64"):
        """lh_accel_intersect_host_tmax: intersect_host under a maximum distance per ray -- tmax: n bounds, taken in the rays' precision
        (float32 rays: float32 bounds).  A ray's answer is the unbounded record if that is a hit with t < tmax, else a miss.  What
        intersect_host(..., tmax=...) calls."""
        return self._intersect_host(org, dr, tmax, mode, records)

    def intersect_host(self, org, dr, mode=MODE_CLOSEST, records="f64", tmax=None):
        """org, dr: [n, 3] host rays.  float32 inputs (numpy arrays or CPU torch tensors, both float32) are sent as fp32 rays
        (traced as the widened fp64 rays: the same records); anything else as fp64.  records="rec16" (closest hit): the records
        come back as one (n, 4) uint32 array of lh_rec16_t {prim, t, u, v as float32 bits}; else (prim, t, u, v) / occluded.
        tmax (an array of n bounds, taken in the rays' precision; None: unbounded, today's paths): a ray's answer is the unbounded
        record if that is a hit with t < tmax, else a miss (lh_accel_intersect_host_tmax)."""
        return self._intersect_host(org, dr, tmax, mode, records)

    def _intersect_host(self, org, dr, tmax, mode, records):
        """intersect_host / intersect_host_tmax: plain fp64 batches go to lh_accel_intersect_host, fp32 rays or rec16 records to _ex, bounds to _tmax"""
        rf = _records_format(records)
        f32 = _is_f32(org) and _is_f32(dr)
        dt = np.float32 if f32 else np.float64
        o = _np(org, dt).reshape(-1, 3); d = _np(dr, dt).reshape(-1, 3)
        n = o.shape[0]
        fmt = (RAYS_F32 if f32 else RAYS_F64, rf)
        if tmax is not None:
            tm = _np(tmax, dt).reshape(-1)
            if tm.shape[0] != n:
                raise ValueError("intersect_host: tmax must hold one bound per ray (%d for %d rays)" % (tm.shape[0], n))
            name, head = "lh_accel_intersect_host_tmax", (tm.ctypes.data,) + fmt
        elif f32 or rf == REC16:
            name, head = "lh_accel_intersect_host_ex", fmt
        else:
            name, head = "lh_accel_intersect_host", ()
        ret, prim, t, u, v, occ = _host_out(n, mode, rf)
        _check(getattr(self.L, name)(self.h, n, o.ctypes.data, d.ctypes.data, *head, prim, t, u, v, occ, mode), name)
        return ret

    def intersect_device_indexed(self, org, dr, out=None, mode=MODE_CLOSEST, stream=None, records="f64", index=None, count=None, tmax=None):
        """lh_accel_intersect_device_indexed: trace the rays of org / dr ([n, 3] device tensors, float64 or float32) that the list
        names, and write their records to THEIR slots of `out`; every other slot of `out` stays as it is.  index: int32 / uint32
        device tensor of ray ids (None: 0 .. n-1); count: one-element int32 / uint32 device tensor, the number of list entries to
        trace (clamped to the list's length; None: all) -- read by the launch on `stream`, not by the host, so it may be what an
        earlier kernel on that stream is still to write (compact()).  Ids >= n are skipped, an id may appear twice.  out: as for
        intersect_device; when it is None the tensors are allocated here with torch.empty, and the slots of rays that are not
        listed are then UNSPECIFIED (whatever the allocator handed over).  tmax: None, or a device tensor of the rays' dtype and
        shape [n] -- a bound per ray ID (not per list position): the listed rays' answers under lh_accel_intersect_device_tmax's
        contract.  Returns out."""
        return self._intersect_device("intersect_device_indexed", org, dr, out, mode, VARIANT_DEFAULT, stream, False, records, (index, count), tmax)

    def intersect_device(self, org, dr, out=None, mode=MODE_CLOSEST, variant=VARIANT_DEFAULT, stream=None,
                         counters=False, records="f64", index=None, count=None, tmax=None):
        """org, dr: CUDA(HIP) float64 or float32 tensors [n,3] (both of one dtype: float32 = fp32 rays, traced as the widened
        fp64 rays), contiguous.  Enqueues on `stream` (default: torch's current stream) and returns the output tensors:
        (prim, t, u, v), (occluded,), or with records="rec16" (closest hit) (rec,) -- one (n, 4) int32 tensor of lh_rec16_t
        {prim, t, u, v as float32 bits}.  fp32 rays and rec16 records run the default variant, without counters.
        index / count (device tensors: a list of ray ids, the number of its entries to trace): only the listed rays are traced,
        their records go to their own slots of `out` and no other slot is written (intersect_device_indexed; the default variant,
        without counters).  With out=None the tensors are freshly allocated and the slots of rays that are not listed are
        UNSPECIFIED.
        tmax (a device tensor of the rays' dtype, shape [n]; None: unbounded, today's paths): a per-ray maximum distance -- a ray's
        answer is the unbounded record if that is a hit with t < tmax (strict; NaN, 0 and negatives: a miss; +inf: unbounded), else a
        miss (lh_accel_intersect_device_tmax; the default variant, without counters)."""
        if tmax is not None and (variant != VARIANT_DEFAULT or counters):
            raise ValueError("bounded batches (tmax) run the default variant without counters")
        if index is not None or count is not None:
            if variant != VARIANT_DEFAULT or counters:
                raise ValueError("indexed batches run the default variant without counters")
            return self.intersect_device_indexed(org, dr, out=out, mode=mode, stream=stream, records=records, index=index, count=count, tmax=tmax)
        return self._intersect_device("intersect_device", org, dr, out, mode, variant, stream, counters, records, None, tmax)

    def _intersect_device(self, what, org, dr, out, mode, variant, stream, counters, records, lst, tmax):
        """intersect_device / intersect_device_indexed behind their own refusals.  lst: None (a dense batch) or (index, count).  Bounds go to
        lh_accel_intersect_device_tmax (a dense batch with the list (NULL, 0, NULL)), a list to _indexed, fp32 rays or rec16 records to _ex,
        counters to _counted, the rest to lh_accel_intersect_device"""
        import torch
        assert org.is_cuda and dr.is_cuda and org.dtype == dr.dtype and org.dtype in (torch.float64, torch.float32)
        assert org.is_contiguous() and dr.is_contiguous()
        rf = _records_format(records)
        n, dev, f32 = org.shape[0], org.device, org.dtype == torch.float32
        ex = lst is None and tmax is None and (f32 or rf == REC16)
        if ex and (variant != VARIANT_DEFAULT or counters):
            raise ValueError("fp32 rays / rec16 records run the default variant without counters")
        out, prim, t, u, v, occ = _device_out(n, dev, mode, rf, out)
        rays = (self.h, n, _dptr(org), _dptr(dr))
        recs = (_dptr(prim), _dptr(t), _dptr(u), _dptr(v), _dptr(occ), mode)
        if counters:                  # a dense, unbounded fp64 batch: the others were refused
            torch.cuda.synchronize(dev)
            c = (C.c_uint64 * 4)()
            _check(self.L.lh_accel_intersect_device_counted(*rays, *recs, variant, c), "lh_accel_intersect_device_counted")
            return out, {"nodes": int(c[0]), "tris": int(c[1]), "exact": int(c[2]), "rays": int(c[3]),
                         "retraced": int(self.L.lh_accel_last_retraced(self.h))}
        ip, ni, cp = (None, 0, None) if lst is None else _list_args(lst[0], lst[1], "intersect_device")
        if lst is not None and lst[0] is None:
            ni = n
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        fmt = (RAYS_F32 if f32 else RAYS_F64, rf)
        if tmax is not None:
            name, args = "lh_accel_intersect_device_tmax", rays + (_dptr(_tmax_device(tmax, org, what)),) + fmt + recs + (ip, ni, cp)
        elif lst is not None:
            name, args = "lh_accel_intersect_device_indexed", rays + fmt + recs + (ip, ni, cp)
        elif ex:
            name, args = "lh_accel_intersect_device_ex", rays + fmt + recs
        else:
            name, args = "lh_accel_intersect_device", rays + recs + (variant,)
        _check(getattr(self.L, name)(*args, C.c_void_p(stream)), name)
        return out

    def trace_statistics(self, enable=True):
        """ri_bvh_clear_stat_traversal / RI_BVH_TRACE_STATISTICS: count node visits, triangle tests, fp64 re-tests, rays and hits of
        the host ray dumps and of the AO tile pipeline (the counting instantiations of the same kernels)"""
        _check(self.L.lh_accel_trace_statistics(self.h, 1 if enable else 0), "lh_accel_trace_statistics")

    def statistics(self, clear=False):
        c = (C.c_uint64 * 5)()
        _check(self.L.lh_accel_statistics(self.h, c, 1 if clear else 0), "lh_accel_statistics")
        return dict(zip(("nodes", "tris", "exact", "rays", "hits"), (int(x) for x in c)))

    def slot_statistics(self, clear=False):
        c = (C.c_uint64 * 3)()
        _check(self.L.lh_accel_slot_statistics(self.h, c, 1 if clear else 0), "lh_accel_slot_statistics")
        return dict(zip(("node_slots", "tri_slots", "regroups"), (int(x) for x in c)))

    def order_statistics(self, clear=False):
        """ray dumps traced from a copy in bin order so far ("dump_order"), and their rays"""
        c = (C.c_uint64 * 2)()
        _check(self.L.lh_accel_order_statistics(self.h, c, 1 if clear else 0), "lh_accel_order_statistics")
        return {"dumps": int(c[0]), "rays": int(c[1])}

    def dump_node_bytes(self):
        """64: ray dumps walk the 4-wide nodes; 128: the 8-wide nodes (scene larger than the Infinity Cache, or wide8 = 1)"""
        return int(self.L.lh_accel_dump_node_bytes(self.h))

    def beam_raster(self, org, corner_dirs, corners, width, height, frame, eye, fov, t_init=None):
        """ri_beam_set + ri_raster_plane_setup + ri_bvh_intersect_beam for n beams over one width x height raster window
        (frame = du dv dw, eye = plane->org, fov in degrees; corners [n,3] = plane->corner per beam).
        -> (t [n,height,width] float64, status int32 [n] (0 traced, 1 nothing done, -1 invalid beam), flags uint64 [n,4]);
        planes that are not traced keep t_init (default zeros = a freshly set-up plane)"""
        o = np.ascontiguousarray(org, np.float64).reshape(-1, 3); n = o.shape[0]
        d = np.ascontiguousarray(corner_dirs, np.float64).reshape(n, 4, 3)
        c = np.ascontiguousarray(corners, np.float64).reshape(n, 3)
        pl = RasterPlane(int(width), int(height), (C.c_double * 9)(*np.asarray(frame, np.float64).reshape(-1)),
                         (C.c_double * 3)(*np.asarray(eye, np.float64).reshape(-1)), float(fov))
        t = np.zeros((n, height, width)) if t_init is None else np.ascontiguousarray(t_init, np.float64).reshape(n, height, width).copy()
        st = np.empty(n, np.int32); fl = np.zeros((n, 4), np.uint64)
        _check(self.L.lh_accel_beam_raster_host(self.h, n, o.ctypes.data, d.ctypes.data, c.ctypes.data, C.addressof(pl),
                                                t.ctypes.data, st.ctypes.data, fl.ctypes.data), "lh_accel_beam_raster_host")
        return t, st, fl

    def beam_visibility(self, org, corner_dirs):
        """ri_beam_set + ri_bvh_intersect_beam_visibility for n beams: org [n,3], corner_dirs [n,4,3]
        -> int32 [n] in {0 miss, 1 hit completely, 2 hit partially, -1 invalid beam}"""
        o = _np(org, np.float64).reshape(-1, 3); d = _np(corner_dirs, np.float64).reshape(-1, 4, 3)
        res = np.empty(o.shape[0], np.int32)
        _check(self.L.lh_accel_beam_visibility_host(self.h, o.shape[0], o.ctypes.data, d.ctypes.data, res.ctypes.data),
               "lh_accel_beam_visibility_host")
        return res

    def _beam_tensor(self, what, name, T, dtypes, count):
        import torch
        if not (isinstance(T, torch.Tensor) and T.is_cuda and T.device.index == self.device and T.is_contiguous()):
            raise ValueError("%s: %s must be a contiguous CUDA tensor on the accelerator's device %d" % (what, name, self.device))
        if T.dtype not in dtypes or T.numel() < count:
            raise ValueError("%s: %s must hold at least %d elements of %s" % (what, name, count, " / ".join(str(d) for d in dtypes)))
        return _dptr(T)

    def beam_visibility_device(self, d_org, d_dirs, d_result, stream=None):
        """lh_accel_beam_visibility_device on the caller's tensors: d_org [n,3] and d_dirs [n,4,3] float64, d_result int32 with at
        least n elements (the first n are written).  Enqueued on `stream` (a torch.cuda.Stream, a raw handle, or None: torch's
        current stream); nothing is allocated or copied and the call does not wait for the device."""
        import torch
        what = "beam_visibility_device"
        n = int(d_org.numel()) // 3
        po = self._beam_tensor(what, "d_org", d_org, (torch.float64,), 3 * n)
        pd = self._beam_tensor(what, "d_dirs", d_dirs, (torch.float64,), 12 * n)
        pr = self._beam_tensor(what, "d_result", d_result, (torch.int32,), n)
        with torch.cuda.device(self.device):
            _check(self.L.lh_accel_beam_visibility_device(self.h, n, po, pd, pr, self._stream_handle(stream)), "lh_accel_beam_visibility_device")

    def beam_raster_device(self, d_org, d_dirs, d_corners, width, height, frame, eye, fov, d_t, d_status, d_flags, stream=None):
        """lh_accel_beam_raster_device on the caller's tensors: d_org [n,3], d_dirs [n,4,3], d_corners [n,3] float64; d_t float64
        with at least n * height * width elements (planes that are not traced keep their contents), d_status int32 (n), d_flags
        int64 / uint64 (4 n) or None.  Enqueued on `stream` as beam_visibility_device; nothing is allocated or copied."""
        import torch
        what = "beam_raster_device"
        n = int(d_org.numel()) // 3
        words = (torch.int64, getattr(torch, "uint64", torch.int64))
        po = self._beam_tensor(what, "d_org", d_org, (torch.float64,), 3 * n)
        pd = self._beam_tensor(what, "d_dirs", d_dirs, (torch.float64,), 12 * n)
        pc = self._beam_tensor(what, "d_corners", d_corners, (torch.float64,), 3 * n)
        pt = self._beam_tensor(what, "d_t", d_t, (torch.float64,), n * int(width) * int(height))
        ps = self._beam_tensor(what, "d_status", d_status, (torch.int32,), n)
        pf = None if d_flags is None else self._beam_tensor(what, "d_flags", d_flags, words, 4 * n)
        pl = RasterPlane(int(width), int(height), (C.c_double * 9)(*np.asarray(frame, np.float64).reshape(-1)),
                         (C.c_double * 3)(*np.asarray(eye, np.float64).reshape(-1)), float(fov))
        with torch.cuda.device(self.device):
            _check(self.L.lh_accel_beam_raster_device(self.h, n, po, pd, pc, C.addressof(pl), pt, ps, pf, self._stream_handle(stream)),
                   "lh_accel_beam_raster_device")

    def beam_visibility_set(self, beams):
        """ri_bvh_intersect_beam_visibility for n beams a caller's ri_beam_set has ALREADY set up: beams = a structured array of
        BEAM_SET_DTYPE (lh_beam_set_t: org, dir[4], normal[4], dominant_axis, dirsign[3]) -> int32 [n]"""
        b = np.ascontiguousarray(beams, BEAM_SET_DTYPE).reshape(-1)
        res = np.empty(b.shape[0], np.int32)
        self.L.lh_accel_beam_visibility_set_host.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        _check(self.L.lh_accel_beam_visibility_set_host(self.h, b.shape[0], b.ctypes.data, res.ctypes.data), "lh_accel_beam_visibility_set_host")
        return res

    # ---- tile rendering (device-resident pipeline) ---------------------------
    def primary_rays(self, cam, x0, y0, w, h, pixel_samples=1, stream=None):
        import torch
        n = w * h * pixel_samples * pixel_samples
        dev = torch.device("cuda", self.device)
        org = torch.empty((n, 3), dtype=torch.float64, device=dev); dr = torch.empty((n, 3), dtype=torch.float64, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(self.L.lh_render_primary_rays(self.h, C.byref(cam), x0, y0, w, h, pixel_samples, _dptr(org), _dptr(dr),
                                             C.c_void_p(stream)), "lh_render_primary_rays")
        return org, dr

    def _render_gather_tile(self, kind, params, lights, cam, x0, y0, w, h, pixel_samples, gather_nsamples, seed, uniforms, out, stream):
        """the five tiles: the row of _BATCH_STAGES, its params and light list, and the call"""
        import torch
        sg = self._BATCH_STAGES[kind]
        params, pargs, _ = self._stage_args("render_%s_tile" % kind, sg, params, lights)
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        st = TileStats()
        mid = self._stage_mid(sg, gather_nsamples, pargs, (int(seed),)) + (() if sg.pack else (_dptr(uniforms),))
        _check(getattr(self.L, sg.tile)(self.h, C.byref(cam), x0, y0, w, h, pixel_samples, *mid, _dptr(out), C.byref(st), C.c_void_p(stream)), sg.tile)
        return out, {k: int(getattr(st, k)) for k, _ in st._fields_}

    def render_ao_tile(self, cam, x0, y0, w, h, pixel_samples, gather_nsamples, seed=1, uniforms=None, out=None,
                       stream=None):
        """-> (rgb float32 [h,w,3] CUDA tensor in image orientation, stats dict)"""
        return self._render_gather_tile("ao", None, None, cam, x0, y0, w, h, pixel_samples, gather_nsamples, seed, uniforms, out, stream)

    def render_dirt_tile(self, cam, x0, y0, w, h, pixel_samples, gather_nsamples, params=None, seed=1, uniforms=None, out=None,
                         stream=None):
        """lh_render_dirt_tile: the dirtmap transport's tile (params: a DirtParams, None: the defaults) ->
        (rgb float32 [h,w,3] CUDA tensor in image orientation, stats dict: ao_rays = hits x N, ao_occluded = the bounded hits)"""
        return self._render_gather_tile("dirt", params, None, cam, x0, y0, w, h, pixel_samples, gather_nsamples, seed, uniforms, out, stream)

    def render_env_tile(self, cam, x0, y0, w, h, pixel_samples, gather_nsamples, params=None, seed=1, uniforms=None, out=None,
                        stream=None):
        """lh_render_env_tile: the environment-lit gather's tile (params: an EnvParams, None: the defaults) ->
        (rgb float32 [h,w,3] CUDA tensor in image orientation, stats dict: ao_rays = hits x N, ao_occluded = the occluded rays)"""
        return self._render_gather_tile("env", params, None, cam, x0, y0, w, h, pixel_samples, gather_nsamples, seed, uniforms, out, stream)

    def render_whitted_tile(self, cam, x0, y0, w, h, pixel_samples, params=None, out=None, stream=None):
        """lh_render_whitted_tile: the refraction chain's tile (params: a WhittedParams, None: the defaults) -- a camera miss sees the
        environment, a hit what its chain of refraction rays ends in -> (rgb float32 [h,w,3] CUDA tensor in image orientation, stats
        dict: paths = camera samples, rays = camera + chain rays, max_depth_reached = the deepest chain ray traced)"""
        import torch
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        st = PtStats()
        _check(self.L.lh_render_whitted_tile(self.h, C.byref(cam), x0, y0, w, h, pixel_samples, None if params is None else C.byref(params),
                                             _dptr(out), C.byref(st), C.c_void_p(stream)), "lh_render_whitted_tile")
        return out, {k: int(getattr(st, k)) for k, _ in st._fields_}

    def render_ao_frame_host(self, cam, pixel_samples, gather_nsamples, seed=1, tile=0):
        """lh_render_ao_frame_host: the whole frame into host memory -> (float32 [H, W, 3] numpy, top row first; stats)"""
        rgb = np.empty((cam.height, cam.width, 3), np.float32)
        st = TileStats()
        self.L.lh_render_ao_frame_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
        _check(self.L.lh_render_ao_frame_host(self.h, C.byref(cam), int(pixel_samples), int(gather_nsamples), int(seed), int(tile),
                                              rgb.ctypes.data, C.byref(st)), "lh_render_ao_frame_host")
        return rgb, {k: int(getattr(st, k)) for k, _ in st._fields_}

    def render_ao_bands(self, cam, band_y0, band_rows, pixel_samples, gather_nsamples, seed=1, out=None, stream=None):
        """full-width bands (first lines band_y0, band_rows lines each) as ONE device batch ->
        (float32 [nbands, band_rows, W, 3] CUDA tensor, every band in image orientation, stats)"""
        import torch
        dev = torch.device("cuda", self.device)
        nb = len(band_y0)
        if out is None:
            out = torch.zeros((nb, band_rows, cam.width, 3), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        st = TileStats(); arr = (C.c_int * max(nb, 1))(*[int(y) for y in band_y0])
        _check(self.L.lh_render_ao_bands(self.h, C.byref(cam), nb, arr, int(band_rows), pixel_samples, gather_nsamples, int(seed),
                                         _dptr(out), C.byref(st), C.c_void_p(stream)), "lh_render_ao_bands")
        return out, {k: int(getattr(st, k)) for k, _ in st._fields_}

    def render_pt_tile(self, cam, x0, y0, w, h, spp_begin, spp_count, spp_total, max_vertices=8, kd=0.8,
                       env=(1.0, 1.0, 1.0), seed=1, out=None, stream=None):
        """adds spp_count path-traced samples to `out` (float32 [h,w,3] CUDA, zeroed if None) -> (out, stats)"""
        import torch
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        st = PtStats(); e = (C.c_float * 3)(*[float(x) for x in env])
        _check(self.L.lh_render_pt_tile(self.h, C.byref(cam), x0, y0, w, h, spp_begin, spp_count, spp_total, max_vertices,
                                        float(kd), C.byref(e), int(seed), _dptr(out), C.byref(st), C.c_void_p(stream)),
               "lh_render_pt_tile")
        return out, {k: int(getattr(st, k)) for k, _ in st._fields_}

    def render_pt_tile2(self, cam, x0, y0, w, h, spp_begin, spp_count, spp_total, max_vertices=8, flags=0, seed=1, out=None,
                        stream=None):
        """as render_pt_tile, with the accelerator's per-mesh materials and environment (set_material / set_environment)"""
        import torch
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        st = PtStats()
        _check(self.L.lh_render_pt_tile2(self.h, C.byref(cam), x0, y0, w, h, spp_begin, spp_count, spp_total, max_vertices,
                                         int(flags), int(seed), _dptr(out), C.byref(st), C.c_void_p(stream)), "lh_render_pt_tile2")
        return out, {k: int(getattr(st, k)) for k, _ in st._fields_}

    def render_pt_bands(self, cam, y0_first, band_rows, band_stride, nbands, spp_begin, spp_count, spp_total, max_vertices=8, flags=0,
                        override=None, seed=1, out=None, stream=None):
        """lh_render_pt_bands: nbands full-width bands (band k starts at frame line y0_first + k * band_stride) as ONE pass ->
        (float32 [nbands, band_rows, W, 3] CUDA tensor, accumulated into `out`; every band in image orientation; stats).
        override: a Material for every mesh, None: the accelerator's own; environment: the accelerator's."""
        import torch
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.zeros((nbands, band_rows, cam.width, 3), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        st = PtStats()
        _check(self.L.lh_render_pt_bands(self.h, C.byref(cam), int(y0_first), int(band_rows), int(band_stride), int(nbands), int(spp_begin),
                                         int(spp_count), int(spp_total), int(max_vertices), int(flags),
                                         C.byref(override) if override is not None else None, int(seed), _dptr(out), C.byref(st),
                                         C.c_void_p(stream)), "lh_render_pt_bands")
        return out, {k: int(getattr(st, k)) for k, _ in st._fields_}

    def _lit_args(self, what, lights, params, sink):
        arr, n = _light_array(what, lights or ())
        if params is not None and not isinstance(params, LightsParams):
            raise ValueError("%s: params must be a LightsParams" % what)
        if sink is not None and not isinstance(sink, (PtSink, PtSinkStruct)):
            raise ValueError("%s: sink must be a PtSink" % what)
        sk = sink.struct() if isinstance(sink, PtSink) else sink
        return arr, n, (C.byref(params) if params is not None else None), (C.byref(sk) if sk is not None else None), sk

    def render_pt_tile_lit(self, cam, x0, y0, w, h, spp_begin, spp_count, spp_total, max_vertices=8, flags=0, lights=(), params=None, sink=None,
                           seed=1, out=None, stream=None):
        """lh_render_pt_tile_lit: render_pt_tile2 with direct light from `lights` (a sequence of 0 .. LIGHTS_MAX Light; params: a LightsParams,
        None: eps 1e-5) at every path vertex -- r = ((G kd) col) value per hit, no 1 / pi -- and a path-vertex sink (a PtSink or None) that
        receives every entry of every bounce -> (out, stats)"""
        import torch
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        arr, n, pp, skp, _keep = self._lit_args("lh_render_pt_tile_lit", lights, params, sink)
        st = PtStats()
        _check(self.L.lh_render_pt_tile_lit(self.h, C.byref(cam), x0, y0, w, h, spp_begin, spp_count, spp_total, max_vertices, int(flags),
                                            arr, n, pp, skp, int(seed), _dptr(out), C.byref(st), C.c_void_p(stream)), "lh_render_pt_tile_lit")
        return out, {k: int(getattr(st, k)) for k, _ in st._fields_}

    def render_pt_bands_lit(self, cam, y0_first, band_rows, band_stride, nbands, spp_begin, spp_count, spp_total, max_vertices=8, flags=0,
                            override=None, lights=(), params=None, sink=None, seed=1, out=None, stream=None):
        """lh_render_pt_bands_lit: render_pt_bands with the lights, params and sink of render_pt_tile_lit -> (out, stats)"""
        import torch
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.zeros((nbands, band_rows, cam.width, 3), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        arr, n, pp, skp, _keep = self._lit_args("lh_render_pt_bands_lit", lights, params, sink)
        st = PtStats()
        _check(self.L.lh_render_pt_bands_lit(self.h, C.byref(cam), int(y0_first), int(band_rows), int(band_stride), int(nbands), int(spp_begin),
                                             int(spp_count), int(spp_total), int(max_vertices), int(flags),
                                             C.byref(override) if override is not None else None, arr, n, pp, skp, int(seed), _dptr(out),
                                             C.byref(st), C.c_void_p(stream)), "lh_render_pt_bands_lit")
        return out, {k: int(getattr(st, k)) for k, _ in st._fields_}

    def _lights_args(self, what, lights, params, area, area_params, sink):
        """-> (byref of a PtLights, byref of the sink or None, what both point to: kept alive by the caller until the call has returned)"""
        arr, n, _pp, skp, sk = self._lit_args(what, lights, params, sink)
        aarr, na = _area_array(what, area or ())
        if area_params is not None and not isinstance(area_params, AreaParams):
            raise ValueError("%s: area_params must be an AreaParams" % what)
        pl = PtLights()
        pl.lights = arr if arr is not None else None
        pl.nlights = n
        pl.params = C.pointer(params) if params is not None else None
        pl.area = aarr if aarr is not None else None
        pl.narea = na
        pl.area_params = C.pointer(area_params) if area_params is not None else None
        return C.byref(pl), skp, (pl, arr, aarr, params, area_params, sk)

    def render_pt_tile_lights(self, cam, x0, y0, w, h, spp_begin, spp_count, spp_total, max_vertices=8, flags=0, lights=(), params=None, area=(),
                              area_params=None, sink=None, seed=1, out=None, stream=None):
        """lh_render_pt_tile_lights: render_pt_tile_lit with soft shadows -- `area` (a sequence of 0 .. AREA_LIGHTS_MAX AreaLight over the emitter
        table of set_emitters; area_params: an AreaParams, None: eps 1e-5, bound 1, 16 samples) lights every path vertex beside, or instead
        of, `lights`: the area value of a hit of bounce d is area_lights_device's for the key of its path's (frame pixel, sample) and the
        bounce's seed; with both kinds a hit's value is the float32 sum of the two -> (out, stats)"""
        import torch
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        plp, skp, _keep = self._lights_args("lh_render_pt_tile_lights", lights, params, area, area_params, sink)
        st = PtStats()
        _check(self.L.lh_render_pt_tile_lights(self.h, C.byref(cam), x0, y0, w, h, spp_begin, spp_count, spp_total, max_vertices, int(flags),
                                               plp, skp, int(seed), _dptr(out), C.byref(st), C.c_void_p(stream)), "lh_render_pt_tile_lights")
        return out, {k: int(getattr(st, k)) for k, _ in st._fields_}

    def render_pt_bands_lights(self, cam, y0_first, band_rows, band_stride, nbands, spp_begin, spp_count, spp_total, max_vertices=8, flags=0,
                               override=None, lights=(), params=None, area=(), area_params=None, sink=None, seed=1, out=None, stream=None):
        """lh_render_pt_bands_lights: render_pt_bands_lit with the area lights of render_pt_tile_lights -> (out, stats)"""
        import torch
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.zeros((nbands, band_rows, cam.width, 3), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        plp, skp, _keep = self._lights_args("lh_render_pt_bands_lights", lights, params, area, area_params, sink)
        st = PtStats()
        _check(self.L.lh_render_pt_bands_lights(self.h, C.byref(cam), int(y0_first), int(band_rows), int(band_stride), int(nbands), int(spp_begin),
                                                int(spp_count), int(spp_total), int(max_vertices), int(flags),
                                                C.byref(override) if override is not None else None, plp, skp, int(seed), _dptr(out),
                                                C.byref(st), C.c_void_p(stream)), "lh_render_pt_bands_lights")
        return out, {k: int(getattr(st, k)) for k, _ in st._fields_}

    def set_material(self, mesh, material):
        _check(self.L.lh_accel_set_material(self.h, int(mesh), C.byref(material)), "lh_accel_set_material")

    def set_texture(self, mesh, texels, stream=None):
        """lh_accel_set_texture / lh_accel_set_texture_device: the material texture of mesh `mesh` (or ALL_MESHES) that the AO and
        dirt tiles multiply a hit's radiance with.  texels: [h, w, 4] float32 -- a numpy array (copied), or a contiguous CUDA
        torch tensor (the device form: read by a copy enqueued on `stream`, None: the current one); None removes the texture.
        Allowed before and after commit."""
        if texels is None:
            _check(self.L.lh_accel_set_texture(self.h, int(mesh), None, 0, 0), "lh_accel_set_texture")
            return
        if hasattr(texels, "is_cuda"):
            import torch
            if not (texels.is_cuda and texels.dtype == torch.float32 and texels.dim() == 3 and texels.shape[2] == 4 and texels.is_contiguous()):
                raise ValueError("set_texture: a tensor must be a contiguous float32 device tensor [h, w, 4]")
            if stream is None:
                stream = torch.cuda.current_stream(texels.device)
            stream = getattr(stream, "cuda_stream", stream)
            _check(self.L.lh_accel_set_texture_device(self.h, int(mesh), _dptr(texels), int(texels.shape[1]), int(texels.shape[0]),
                                                      C.c_void_p(stream)), "lh_accel_set_texture_device")
            return
        T = _np(texels, np.float32)
        if T.ndim != 3 or T.shape[2] != 4:
            raise ValueError("set_texture: texels must be [h, w, 4]")
        _check(self.L.lh_accel_set_texture(self.h, int(mesh), T.ctypes.data, int(T.shape[1]), int(T.shape[0])), "lh_accel_set_texture")

    def texture_device(self, records, index=None, count=None, out=None, stream=None):
        """lh_accel_texture_device: the texture fetch alone for a batch of closest-hit records -- `records` = the (prim, t, u, v)
        device tensors of intersect_device (t is not read).  index / count: a device list as for ao_device.  Returns the float64
        tensor [n, 4]: the filtered RGBA at the hit, 1 1 1 1 where its mesh has no texture, zeros for a traced miss.  out: such a
        tensor to fill; with out=None it is allocated with torch.empty and the rows of rays that are not listed are UNSPECIFIED.
        Asynchronous on `stream`."""
        import torch
        what = "texture_device"
        if not isinstance(records, (tuple, list)) or len(records) != 4:
            raise ValueError("%s: records must be the (prim, t, u, v) tensors of a closest-hit batch" % what)
        prim, _, u, v = records
        words = (torch.int32, getattr(torch, "uint32", torch.int32))
        if not (isinstance(prim, torch.Tensor) and prim.is_cuda and prim.dtype in words and prim.dim() == 1 and prim.is_contiguous()):
            raise ValueError("%s: prim must be a contiguous int32 / uint32 device tensor [n]" % what)
        n = int(prim.shape[0])
        for name, x in (("u", u), ("v", v)):
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float64 and x.dim() == 1 and x.shape[0] == n and x.is_contiguous()):
                raise ValueError("%s: %s must be a contiguous float64 device tensor [n]" % (what, name))
        ip, ni, cp = _list_args(index, count, what)
        if index is None and count is not None:
            ni = n
        if out is None:
            out = torch.empty((n, 4), dtype=torch.float64, device=prim.device)
        if not (out.is_cuda and out.dtype == torch.float64 and out.dim() == 2 and tuple(out.shape) == (n, 4) and out.is_contiguous()):
            raise ValueError("%s: out must be a contiguous float64 device tensor [n, 4]" % what)
        if stream is None:
            stream = torch.cuda.current_stream(prim.device)
        stream = getattr(stream, "cuda_stream", stream)
        _check(self.L.lh_accel_texture_device(self.h, n, _dptr(prim), _dptr(u), _dptr(v), ip, ni, cp, _dptr(out), C.c_void_p(stream)),
               "lh_accel_texture_device")
        return out

    def texture_host(self, prim, u, v):
        """lh_accel_texture_host: host arrays of closest-hit records -> float64 [n, 4] as texture_device (every ray is traced)"""
        p = _np(prim, np.uint32).reshape(-1); uu = _np(u, np.float64).reshape(-1); vv = _np(v, np.float64).reshape(-1)
        if not (p.shape[0] == uu.shape[0] == vv.shape[0]):
            raise ValueError("texture_host: prim, u and v must describe the same rays")
        out = np.zeros((p.shape[0], 4))
        _check(self.L.lh_accel_texture_host(self.h, p.shape[0], p.ctypes.data, uu.ctypes.data, vv.ctypes.data, out.ctypes.data), "lh_accel_texture_host")
        return out

    def reset_environment(self):
        """back to the default environment of the path tracer (constant white)"""
        _check(self.L.lh_accel_set_environment(self.h, None), "lh_accel_set_environment")
        self._env = None

    def set_environment(self, rgb=(1.0, 1.0, 1.0), envmap=None):
        """envmap: [H,W,4] float32 angular-map light probe or None (constant radiance rgb).  An explicit (0, 0, 0) is black."""
        self._env = (tuple(float(x) for x in rgb), envmap)
        e = Environment()
        for k in range(3):
            e.rgb[k] = float(rgb[k])
        m = None
        if envmap is not None:
            m = np.ascontiguousarray(envmap, np.float32)
            assert m.ndim == 3 and m.shape[2] == 4
            e.map_rgba = m.ctypes.data; e.height, e.width = m.shape[0], m.shape[1]
        _check(self.L.lh_accel_set_environment(self.h, C.byref(e)), "lh_accel_set_environment")

    def set_attribute(self, mesh, kind, data):
        D = _np(data, np.float64)
        if D.ndim != 2:
            raise ValueError("attribute data must be [n, components]")
        _check(self.L.lh_accel_set_attribute(self.h, int(mesh), int(kind), D.ctypes.data, D.shape[1] * 8, D.shape[0]),
               "lh_accel_set_attribute")

    def state_build(self, org, dr, prim, t, u, v):
        """host arrays -> [n, 24] ri_intersection_state_build records (zeros for misses)"""
        o = _np(org, np.float64).reshape(-1, 3); d = _np(dr, np.float64).reshape(-1, 3)
        p = _np(prim, np.uint32); tt = _np(t, np.float64); uu = _np(u, np.float64); vv = _np(v, np.float64)
        st = np.zeros((o.shape[0], STATE_DOUBLES))
        _check(self.L.lh_accel_state_build_host(self.h, o.shape[0], o.ctypes.data, d.ctypes.data, p.ctypes.data, tt.ctypes.data,
                                                uu.ctypes.data, vv.ctypes.data, st.ctypes.data), "lh_accel_state_build_host")
        return st

    def state_build_device(self, org, dr, prim, t, u, v, out=None, stream=None):
        """lh_accel_state_build_device: float64 device tensors org, dr [n, 3], t, u, v [n] and the int32 / uint32 prim [n] of a batch's hit
        records -> the float64 device tensor [n, 24] of their ri_intersection_state_build records, in stream order (nothing is read back).
        The record of a miss (prim AO_NO_HIT's bits, LH_MISS_PRIM) is NOT written, and no record at all on an empty scene: out -- such a tensor
        to fill -- keeps what it held there; with out=None it is allocated with torch.empty and those records are UNSPECIFIED."""
        import torch
        what = "state_build_device"
        n, prim, t, u, v = self._ao_batch_in(what, org, dr, (prim, t, u, v), None, None)
        if out is None:
            out = torch.empty((n, STATE_DOUBLES), dtype=torch.float64, device=org.device)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and out.dim() == 2 and tuple(out.shape) == (n, STATE_DOUBLES)
                and out.is_contiguous()):
            raise ValueError("%s: out must be a contiguous float64 device tensor [n, %d]" % (what, STATE_DOUBLES))
        if stream is None:
            stream = torch.cuda.current_stream(org.device)
        stream = getattr(stream, "cuda_stream", stream)
        _check(self.L.lh_accel_state_build_device(self.h, n, _dptr(org), _dptr(dr), _dptr(prim), _dptr(t), _dptr(u), _dptr(v), _dptr(out), C.c_void_p(stream)),
               "lh_accel_state_build_device")
        return out

    # ---- the AO stage for a caller's batch of hit records -------------------------------
    @staticmethod
    def _ao_batch_in(what, org, dr, records, key, uniforms):
        """the checks ao_device / ao_rays_device make before they call C: (n, prim, t, u, v)"""
        import torch
        words = (torch.int32, getattr(torch, "uint32", torch.int32))
        keys = (torch.int64, getattr(torch, "uint64", torch.int64))
        for name, x in (("org", org), ("dr", dr)):
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float64 and x.dim() == 2 and x.shape[1] == 3 and x.is_contiguous()):
                raise ValueError("%s: %s must be a contiguous float64 device tensor [n, 3]" % (what, name))
        n = int(org.shape[0])
        if int(dr.shape[0]) != n:
            raise ValueError("%s: org and dr differ in length" % what)
        if not isinstance(records, (tuple, list)) or len(records) != 4:
            raise ValueError("%s: records must be the (prim, t, u, v) tensors of a closest-hit batch" % what)
        prim, t, u, v = records
        if not (isinstance(prim, torch.Tensor) and prim.is_cuda and prim.dtype in words and prim.dim() == 1 and prim.shape[0] == n and prim.is_contiguous()):
            raise ValueError("%s: prim must be a contiguous int32 / uint32 device tensor [n]" % what)
        for name, x in (("t", t), ("u", u), ("v", v)):
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float64 and x.dim() == 1 and x.shape[0] == n and x.is_contiguous()):
                raise ValueError("%s: %s must be a contiguous float64 device tensor [n]" % (what, name))
        if key is not None and not (isinstance(key, torch.Tensor) and key.is_cuda and key.dtype in keys and key.dim() == 1 and key.shape[0] == n and key.is_contiguous()):
            raise ValueError("%s: key must be a contiguous int64 / uint64 device tensor [n]" % what)
        if uniforms is not None and not (isinstance(uniforms, torch.Tensor) and uniforms.is_cuda and uniforms.dtype == torch.float64 and uniforms.is_contiguous()):
            raise ValueError("%s: uniforms must be a contiguous float64 device tensor" % what)
        return n, prim, t, u, v

    def ao_device(self, org, dr, records, gather_nsamples, seed=1, key=None, uniforms=None, index=None, count=None, out=None,
                  stream=None):
        """lh_accel_ao_device: the AO stage of render_ao_tile for a batch of rays and their closest-hit records (`records` = the
        (prim, t, u, v) tensors intersect_device returned for org / dr, float64 rays).  N = floor(sqrt(gather_nsamples))^2 AO rays
        per hit.  key: int64 / uint64 device tensor [n] whose low 34 bits key the built-in generator (None: ray i has key i);
        uniforms: float64 device tensor, 2 per AO ray in (hit slot, j, i) order -- the replay path (None: the built-in generator);
        index / count: a device list as for intersect_device (only the listed rays are traced, no other slot of `out` is written).
        Returns (count, radiance): an int32 tensor [n] whose bits are uint32 -- the occluded rays of the hit, AO_NO_HIT for a miss --
        and the float32 tensor [n] of (N - count) / N (0 for a miss).  out: such a pair to fill (either member may be None, not
        both); with out=None both are allocated with torch.empty and the slots of rays that are not listed are UNSPECIFIED.
        Synchronous: the outputs are complete on return."""
        return self._batch_stage_device("ao", None, None, org, dr, records, gather_nsamples, seed, key, uniforms, index, count, out, stream)

    def dirt_device(self, org, dr, records, gather_nsamples, params=None, seed=1, key=None, uniforms=None, index=None, count=None,
                    out=None, stream=None):
        """lh_accel_dirt_device: the dirtmap transport's stage -- range-limited, distance-weighted occlusion -- for a batch of rays
        and their closest-hit records; arguments as ao_device, and params: a DirtParams (None: near 0.1, far 0.5, eps 1e-5).
        Returns (near_hits, value): an int32 tensor [n] whose bits are uint32 -- the hit's gather rays with a closest hit below
        the far clip, AO_NO_HIT for a miss -- and the float32 tensor [n] of the mean weight (0 for a miss).  out: such a pair to
        fill (either member may be None, not both); with out=None the slots of rays that are not listed are UNSPECIFIED.
        Synchronous: the outputs are complete on return."""
        return self._batch_stage_device("dirt", params, None, org, dr, records, gather_nsamples, seed, key, uniforms, index, count, out, stream)

    def env_device(self, org, dr, records, gather_nsamples, params=None, seed=1, key=None, uniforms=None, index=None, count=None,
                   out=None, stream=None):
        """lh_accel_env_device: the environment-lit gather -- sky light with visibility -- for a batch of rays and their closest-hit
        records; arguments as ao_device, and params: an EnvParams (None: eps 1e-5, scale 1).  Returns (count, rgb): an int32 tensor
        [n] whose bits are uint32 -- the hit's occluded gather rays, AO_NO_HIT for a miss -- and the float32 tensor [n, 3] of the
        gathered colour (zeros for a miss), the accelerator's environment (set_environment) seen by the rays that are not occluded.
        out: such a pair to fill (either member may be None, not both); with out=None the slots of rays that are not listed are
        UNSPECIFIED.  Synchronous: the outputs are complete on return."""
        return self._batch_stage_device("env", params, None, org, dr, records, gather_nsamples, seed, key, uniforms, index, count, out, stream)

    # kind -> what differs between the kinds' forms.  device, host, tile, rays: the C functions (rays None: the kind has no rays-alone form); ptype, pname:
    # the type of params and how a refusal names it; pack: how the light list is packed (None: a sampled kind, gather_nsamples goes to C instead);
    # seeded: seed, key and uniforms go to C; rgb: the value is [n, 3]; word, pair: how the messages name the 32-bit output and the out pair; host_key:
    # the host form's refusal of a key array of another length; rays_out: the names of the rays-alone form's double outputs, [m, 3] twice, then [m]
    _Stage = collections.namedtuple("_Stage", "device host tile rays ptype pname pack seeded rgb word pair host_key rays_out")
    _BATCH_STAGES = {
        "ao": _Stage("lh_accel_ao_device", "lh_accel_ao_host", "lh_render_ao_tile", "lh_accel_ao_rays_device", None, None, None, True, False,
                     "count", "(count, radiance)", "one key per ray", ("ao_org", "ao_dir")),
        "dirt": _Stage("lh_accel_dirt_device", "lh_accel_dirt_host", "lh_render_dirt_tile", None, DirtParams, "a DirtParams", None, True, False,
                       "count", "(count, radiance)", "one key per ray", None),
        "env": _Stage("lh_accel_env_device", "lh_accel_env_host", "lh_render_env_tile", None, EnvParams, "an EnvParams", None, True, True,
                      "count", "(count, radiance)", "one key per ray", None),
        "lights": _Stage("lh_accel_lights_device", "lh_accel_lights_host", "lh_render_lights_tile", "lh_accel_light_rays_device", LightsParams,
                         "a LightsParams", _light_array, False, True, "mask", "(visible, rgb)", None, ("org", "dir", "tmax")),
        "area_lights": _Stage("lh_accel_area_lights_device", "lh_accel_area_lights_host", "lh_render_area_lights_tile", "lh_accel_area_light_rays_device",
                              AreaParams, "an AreaParams", _area_array, True, True, "mask", "(visible, rgb)", "key must hold one word per ray",
                              ("org", "dir", "tmax", "weight"))}

    @staticmethod
    def _stage_args(what, sg, params, lights):
        """-> (the row's params: the caller's, or for None the type's defaults; params and the packed light list as the C call takes them; the lights)"""
        if sg.ptype is not None:
            if params is None:
                params = sg.ptype()
            if not isinstance(params, sg.ptype):
                raise ValueError("%s: params must be %s" % (what, sg.pname))
        pargs = () if sg.ptype is None else (C.byref(params),)
        if sg.pack is None:
            return params, pargs, 0
        arr, nl = sg.pack(what, lights)
        return params, (arr, nl) + pargs, nl

    @staticmethod
    def _stage_mid(sg, gather_nsamples, pargs, seeded):
        """what a C call takes between the records and its outputs: gather_nsamples (a sampled kind), params, `seeded` (a seeded kind)"""
        return (() if sg.pack else (int(gather_nsamples),)) + pargs + (seeded if sg.seeded else ())

    def _batch_stage_device(self, kind, params, lights, org, dr, records, gather_nsamples, seed, key, uniforms, index, count, out, stream):
        """the five device forms: the row of _BATCH_STAGES, the checks and the call (params None: the type's defaults)"""
        import torch
        sg = self._BATCH_STAGES[kind]
        what = kind + "_device"
        params, pargs, _ = self._stage_args(what, sg, params, lights)
        n, prim, t, u, v = self._ao_batch_in(what, org, dr, records, key, uniforms)
        dev = org.device
        ip, ni, cp = _list_args(index, count, what)
        if index is None and count is not None:
            ni = n
        if out is None:
            out = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 3) if sg.rgb else n, dtype=torch.float32, device=dev))
        if not isinstance(out, (tuple, list)) or len(out) != 2 or (out[0] is None and out[1] is None):
            raise ValueError("%s: out must be a %s pair, at least one of them a tensor" % (what, sg.pair))
        oc, orad = out
        words = (torch.int32, getattr(torch, "uint32", torch.int32))
        if oc is not None and not (oc.is_cuda and oc.dtype in words and oc.dim() == 1 and oc.shape[0] == n and oc.is_contiguous()):
            raise ValueError("%s: the %s output must be a contiguous int32 / uint32 device tensor [n]" % (what, sg.word))
        if sg.rgb and orad is not None and not (orad.is_cuda and orad.dtype == torch.float32 and orad.dim() == 2 and tuple(orad.shape) == (n, 3) and orad.is_contiguous()):
            raise ValueError("%s: the colour output must be a contiguous float32 device tensor [n, 3]" % what)
        if not sg.rgb and orad is not None and not (orad.is_cuda and orad.dtype == torch.float32 and orad.dim() == 1 and orad.shape[0] == n and orad.is_contiguous()):
            raise ValueError("%s: the radiance output must be a contiguous float32 device tensor [n]" % what)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        stream = getattr(stream, "cuda_stream", stream)
        mid = self._stage_mid(sg, gather_nsamples, pargs, (int(seed), _dptr(key), _dptr(uniforms)))
        _check(getattr(self.L, sg.device)(self.h, n, _dptr(org), _dptr(dr), _dptr(prim), _dptr(t), _dptr(u), _dptr(v), *mid, ip, ni, cp, _dptr(oc), _dptr(orad),
                                          C.c_void_p(stream)), sg.device)
        return out

    def _rays_device(self, kind, params, lights, org, dr, records, gather_nsamples, seed, key, uniforms, out, stream):
        """the three rays-alone forms: the row of _BATCH_STAGES, the checks and the call.  out: (slot_of_ray, nslots) and the row's rays_out; a last member
        "weight" may be None; the capacity handed to C is the shortest of the double outputs that are given"""
        import torch
        sg = self._BATCH_STAGES[kind]
        what = sg.rays[len("lh_accel_"):]
        params, pargs, nl = self._stage_args(what, sg, params, lights)
        n, prim, t, u, v = self._ao_batch_in(what, org, dr, records, key, uniforms)
        dev = org.device
        if sg.pack is None:
            if int(gather_nsamples) < 1:
                raise ValueError("%s: gather_nsamples must be at least 1" % what)
            m = n * int(int(gather_nsamples) ** 0.5) ** 2
        else:
            m = n * max(nl, 1) * max(int(getattr(params, "nsamples", 1)), 1)
        names = ("slot_of_ray", "nslots") + sg.rays_out
        if out is None:
            out = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)) + tuple(
                torch.empty((m, 3) if k < 2 else m, dtype=torch.float64, device=dev) for k in range(len(sg.rays_out)))
        if not isinstance(out, (tuple, list)) or len(out) != len(names):
            raise ValueError("%s: out must be (%s)" % (what, ", ".join(names)))
        so, ns = out[:2]
        words = (torch.int32, getattr(torch, "uint32", torch.int32))
        if not (so.is_cuda and so.dtype in words and so.dim() == 1 and so.shape[0] == n and so.is_contiguous()):
            raise ValueError("%s: slot_of_ray must be a contiguous int32 / uint32 device tensor [n]" % what)
        if not (ns.is_cuda and ns.dtype in words and ns.numel() == 1):
            raise ValueError("%s: nslots must be a one-element int32 / uint32 device tensor" % what)
        for k, (name, x) in enumerate(zip(sg.rays_out, out[2:])):
            if x is None and name == "weight":
                continue
            if k < 2 and not (x.is_cuda and x.dtype == torch.float64 and x.dim() == 2 and x.shape[1] == 3 and x.is_contiguous()):
                raise ValueError("%s: %s must be a contiguous float64 device tensor [m, 3]" % (what, name))
            if k >= 2 and not (x.is_cuda and x.dtype == torch.float64 and x.dim() == 1 and x.is_contiguous()):
                raise ValueError("%s: %s must be a contiguous float64 device tensor [m]" % (what, name))
        cap = min(int(x.shape[0]) for x in out[2:] if x is not None)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        stream = getattr(stream, "cuda_stream", stream)
        mid = self._stage_mid(sg, gather_nsamples, pargs, (int(seed), _dptr(key), _dptr(uniforms)))
        _check(getattr(self.L, sg.rays)(self.h, n, _dptr(org), _dptr(dr), _dptr(prim), _dptr(t), _dptr(u), _dptr(v), *mid, _dptr(so), _dptr(ns),
                                        *[_dptr(x) for x in out[2:]], cap, C.c_void_p(stream)), sg.rays)
        return out

    def ao_rays_device(self, org, dr, records, gather_nsamples, seed=1, key=None, uniforms=None, out=None, stream=None):
        """lh_accel_ao_rays_device: only the AO rays of the batch's hits, for a caller who traces them itself.  Returns
        (slot_of_ray int32 [n] -- the hit slot of every ray, AO_NO_HIT (as uint32 bits) for a miss; nslots -- one-element int32
        tensor, the number of hits; ao_org, ao_dir -- float64 [n * N, 3], ray (slot, r) at row slot * N + r, the first
        nslots * N rows written).  Everything stays on the device and nothing is read back; out: such a 4-tuple to fill."""
        return self._rays_device("ao", None, None, org, dr, records, gather_nsamples, seed, key, uniforms, out, stream)

    def ao_host(self, org, dr, records, gather_nsamples, seed=1, key=None, uniforms=None):
        """lh_accel_ao_host: host arrays (org, dr [n, 3]; records = (prim, t, u, v)) -> (count uint32 [n], radiance float32 [n])"""
        return self._batch_stage_host("ao", None, None, org, dr, records, gather_nsamples, seed, key, uniforms)

    def dirt_host(self, org, dr, records, gather_nsamples, params=None, seed=1, key=None, uniforms=None):
        """lh_accel_dirt_host: host arrays as ao_host, params as dirt_device -> (near_hits uint32 [n], value float32 [n])"""
        return self._batch_stage_host("dirt", params, None, org, dr, records, gather_nsamples, seed, key, uniforms)

    def env_host(self, org, dr, records, gather_nsamples, params=None, seed=1, key=None, uniforms=None):
        """lh_accel_env_host: host arrays as ao_host, params as env_device -> (count uint32 [n], rgb float32 [n, 3])"""
        return self._batch_stage_host("env", params, None, org, dr, records, gather_nsamples, seed, key, uniforms)

    # ---- direct light: shadow rays from a batch of hits to a list of lights (lh_lights.h) ----
    def lights_device(self, org, dr, records, lights, params=None, index=None, count=None, out=None, stream=None):
        """lh_accel_lights_device: which of `lights` (a sequence of 1 .. LIGHTS_MAX Light) every hit of a batch of rays and their closest-hit
        records sees, and what they add; org / dr / records / index / count as env_device, params: a LightsParams (None: eps 1e-5).  Returns
        (visible, rgb): an int32 tensor [n] whose bits are uint32 -- bit l: the hit sees light l; AO_NO_HIT for a miss -- and the float32
        tensor [n, 3] of the sum of the visible lights' weighted colours in list order (zeros for a miss).  out: such a pair to fill (either
        member may be None, not both); with out=None the slots of rays that are not listed are UNSPECIFIED.  Synchronous."""
        return self._batch_stage_device("lights", params, lights, org, dr, records, None, 0, None, None, index, count, out, stream)

    def lights_host(self, org, dr, records, lights, params=None):
        """lh_accel_lights_host: host arrays (org, dr [n, 3]; records = (prim, t, u, v)) -> (visible uint32 [n], rgb float32 [n, 3])"""
        return self._batch_stage_host("lights", params, lights, org, dr, records, None, 0, None, None)

    def light_rays_device(self, org, dr, records, lights, params=None, out=None, stream=None):
        """lh_accel_light_rays_device: only the shadow rays of the batch's hits, for a caller who traces them itself.  Returns (slot_of_ray
        int32 [n] -- the hit slot of every ray, AO_NO_HIT (as uint32 bits) for a miss; nslots -- one-element int32 tensor, the number of hits;
        org, dir -- float64 [n * L, 3]; tmax -- float64 [n * L]: ray (slot, l) at row slot * L + l, the first nslots * L rows written; tmax is
        +inf for a directional light, 1 for a point light, 0 for a ray that is not traced: its bit is clear whatever a launch answers).
        intersect_device(..., mode=MODE_ANY, tmax=tmax) on them gives the stage's bytes.  Everything stays on the device and nothing is read
        back; out: such a 5-tuple to fill."""
        return self._rays_device("lights", params, lights, org, dr, records, None, 0, None, None, out, stream)

    def render_lights_tile(self, cam, x0, y0, w, h, pixel_samples, lights, params=None, out=None, stream=None):
        """lh_render_lights_tile: direct light per camera sample -- a miss gives 0, a hit the sum of the lights it sees -> (rgb float32
        [h,w,3] CUDA tensor in image orientation, stats dict: ao_rays = hits x lights, ao_occluded = the items whose bit is clear)"""
        return self._render_gather_tile("lights", params, lights, cam, x0, y0, w, h, pixel_samples, None, 0, None, out, stream)

    # ---- area lights: soft shadows from triangle emitters (lh_area.h) ----
    def set_emitters(self, tris):
        """lh_accel_set_emitters: the table of emitter triangles the area lights' runs index -- host array [ntris, 3, 3] (or [ntris, 9]) of
        float64 vertices; None (or an empty array) removes it.  After commit, at any time; kept across recommit."""
        if tris is None:
            _check(self.L.lh_accel_set_emitters(self.h, None, 0), "lh_accel_set_emitters")
            return
        t = _np(tris, np.float64).reshape(-1, 9)
        if t.shape[0] == 0:
            _check(self.L.lh_accel_set_emitters(self.h, None, 0), "lh_accel_set_emitters")
            return
        _check(self.L.lh_accel_set_emitters(self.h, t.ctypes.data, t.shape[0]), "lh_accel_set_emitters")

    def area_lights_device(self, org, dr, records, lights, params=None, seed=1, key=None, uniforms=None, index=None, count=None, out=None, stream=None):
        """lh_accel_area_lights_device: which of `lights` (a sequence of 1 .. AREA_LIGHTS_MAX AreaLight) every hit of a batch of rays and their
        closest-hit records sees through params.nsamples samples each, and the mean of what the samples add; org / dr / records / index / count
        as lights_device, seed / key / uniforms as ao_device (uniforms: 3 per item in (hit slot, l, s) order).  Returns (visible, rgb) as
        lights_device does.  Synchronous."""
        return self._batch_stage_device("area_lights", params, lights, org, dr, records, None, seed, key, uniforms, index, count, out, stream)

    def area_lights_host(self, org, dr, records, lights, params=None, seed=1, key=None, uniforms=None):
        """lh_accel_area_lights_host: host arrays (org, dr [n, 3]; records = (prim, t, u, v); key uint64 [n] or None; uniforms float64, 3 per
        item, or None) -> (visible uint32 [n], rgb float32 [n, 3])"""
        return self._batch_stage_host("area_lights", params, lights, org, dr, records, None, seed, key, uniforms)

    def area_light_rays_device(self, org, dr, records, lights, params=None, seed=1, key=None, uniforms=None, out=None, stream=None):
        """lh_accel_area_light_rays_device: only the rays of the batch's hits to the lights' samples.  Returns (slot_of_ray int32 [n], nslots --
        one-element int32 tensor, org, dir -- float64 [n * L * S, 3], tmax, weight -- float64 [n * L * S]: item (slot, l, s) at row
        (slot * L + l) * S + s, the first nslots * L * S rows written; tmax is params.bound, or 0 for an item that is not traced).
        intersect_device(..., mode=MODE_ANY, tmax=tmax) on them gives the stage's bytes.  Nothing is read back; out: such a 6-tuple to fill."""
        return self._rays_device("area_lights", params, lights, org, dr, records, None, seed, key, uniforms, out, stream)

    def render_area_lights_tile(self, cam, x0, y0, w, h, pixel_samples, lights, params=None, seed=1, out=None, stream=None):
        """lh_render_area_lights_tile: area lights per camera sample -- a miss gives 0, a hit the mean over the samples of what its lights add ->
        (rgb float32 [h,w,3] CUDA tensor in image orientation, stats dict: ao_rays = hits x lights x samples, ao_occluded = the items that are
        not open).  The built-in generator, keyed by the absolute sample position: a frame does not depend on its tiling."""
        return self._render_gather_tile("area_lights", params, lights, cam, x0, y0, w, h, pixel_samples, None, seed, None, out, stream)

    def environment_device(self, dirs, out=None, stream=None):
        """lh_accel_environment_device: the accelerator's environment (set_environment; constant white if none was set) seen in each of
        the directions `dirs` (contiguous float64 device tensor [n, 3], need not be unit vectors) -> float32 device tensor [n, 3].
        Asynchronous on the stream; a zero or non-finite direction gives an unspecified colour."""
        import torch
        if not (isinstance(dirs, torch.Tensor) and dirs.is_cuda and dirs.dtype == torch.float64 and dirs.dim() == 2 and dirs.shape[1] == 3 and dirs.is_contiguous()):
            raise ValueError("environment_device: dirs must be a contiguous float64 device tensor [n, 3]")
        n = int(dirs.shape[0])
        if out is None:
            out = torch.empty((n, 3), dtype=torch.float32, device=dirs.device)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n, 3) and out.is_contiguous()):
            raise ValueError("environment_device: out must be a contiguous float32 device tensor [n, 3]")
        if stream is None:
            stream = torch.cuda.current_stream(dirs.device)
        stream = getattr(stream, "cuda_stream", stream)
        _check(self.L.lh_accel_environment_device(self.h, n, _dptr(dirs), _dptr(out), C.c_void_p(stream)), "lh_accel_environment_device")
        return out

    def environment_host(self, dirs):
        """lh_accel_environment_host: host directions [n, 3] -> float32 [n, 3]"""
        d = _np(dirs, np.float64).reshape(-1, 3)
        rgb = np.empty((d.shape[0], 3), np.float32)
        _check(self.L.lh_accel_environment_host(self.h, d.shape[0], d.ctypes.data, rgb.ctypes.data), "lh_accel_environment_host")
        return rgb

    # ---- the sun-and-sky light of the environment-lit gather (lh_sky.h) --------
    def set_sky(self, sky):
        """lh_accel_set_sky: from now on env_device / env_host / render_env_tile read this Sky in place of the environment -- the
        Preetham sky as the radiance of an open gather ray and, with SKY_SUN in its flags, the sun's shadow ray per hit.  After commit;
        the struct is copied.  A non-finite field or an undefined flag is refused."""
        if not isinstance(sky, Sky):
            raise ValueError("set_sky: sky must be a Sky")
        _check(self.L.lh_accel_set_sky(self.h, C.byref(sky)), "lh_accel_set_sky")

    def reset_sky(self):
        """no sky: the gather reads the environment again"""
        _check(self.L.lh_accel_set_sky(self.h, None), "lh_accel_set_sky")

    def sky_device(self, dirs, out=None, stream=None):
        """lh_accel_sky_device: the accelerator's sky (set_sky) seen in each of the directions `dirs` (contiguous float64 device tensor
        [n, 3]; unit vectors: any other length gives an unspecified colour) -> float32 device tensor [n, 3].  Asynchronous on the stream."""
        import torch
        if not (isinstance(dirs, torch.Tensor) and dirs.is_cuda and dirs.dtype == torch.float64 and dirs.dim() == 2 and dirs.shape[1] == 3 and dirs.is_contiguous()):
            raise ValueError("sky_device: dirs must be a contiguous float64 device tensor [n, 3]")
        n = int(dirs.shape[0])
        if out is None:
            out = torch.empty((n, 3), dtype=torch.float32, device=dirs.device)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n, 3) and out.is_contiguous()):
            raise ValueError("sky_device: out must be a contiguous float32 device tensor [n, 3]")
        if stream is None:
            stream = torch.cuda.current_stream(dirs.device)
        stream = getattr(stream, "cuda_stream", stream)
        _check(self.L.lh_accel_sky_device(self.h, n, _dptr(dirs), _dptr(out), C.c_void_p(stream)), "lh_accel_sky_device")
        return out

    def sky_host(self, dirs):
        """lh_accel_sky_host: host directions [n, 3] -> float32 [n, 3]"""
        d = _np(dirs, np.float64).reshape(-1, 3)
        rgb = np.empty((d.shape[0], 3), np.float32)
        _check(self.L.lh_accel_sky_host(self.h, d.shape[0], d.ctypes.data, rgb.ctypes.data), "lh_accel_sky_host")
        return rgb

    # ---- the refraction chain for a caller's batch of hit records (lh_whitted.h) --------
    def whitted_rays_device(self, org, dr, records, params=None, index=None, count=None, out=None, stream=None):
        """lh_accel_whitted_rays_device: the bounce alone -- the refraction ray (or its mirror image, at a total internal reflection)
        every traced hit of the batch sends on; arguments as whitted_device.  Returns (org_out, dir_out), float64 [n, 3]: row id is
        written for a traced hit and stays as it is for a miss or a ray that is not listed (out=None: torch.empty, UNSPECIFIED there).
        Asynchronous on the stream, nothing is read back."""
        import torch
        what = "whitted_rays_device"
        n, prim, t, u, v = self._ao_batch_in(what, org, dr, records, None, None)
        params = self._whitted_params(what, params)
        ip, ni, cp = _list_args(index, count, what)
        if index is None and count is not None:
            ni = n
        if out is None:
            out = (torch.empty((n, 3), dtype=torch.float64, device=org.device), torch.empty((n, 3), dtype=torch.float64, device=org.device))
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise ValueError("%s: out must be an (org_out, dir_out) pair" % what)
        for name, x in (("org_out", out[0]), ("dir_out", out[1])):
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float64 and tuple(x.shape) == (n, 3) and x.is_contiguous()):
                raise ValueError("%s: %s must be a contiguous float64 device tensor [n, 3]" % (what, name))
        if stream is None:
            stream = torch.cuda.current_stream(org.device)
        stream = getattr(stream, "cuda_stream", stream)
        _check(self.L.lh_accel_whitted_rays_device(self.h, n, _dptr(org), _dptr(dr), _dptr(prim), _dptr(t), _dptr(u), _dptr(v), C.byref(params),
                                                   ip, ni, cp, _dptr(out[0]), _dptr(out[1]), C.c_void_p(stream)), "lh_accel_whitted_rays_device")
        return out

    def whitted_device(self, org, dr, records, params=None, index=None, count=None, out=None, stream=None):
        """lh_accel_whitted_device: the reference's Whitted transport for a batch of rays and their closest-hit records (`records` = the
        (prim, t, u, v) tensors intersect_device returned for org / dr, float64 rays): every hit sends a chain of up to
        params.max_depth refraction rays on, which ends in the accelerator's environment (set_environment) or at the depth limit.
        params: a WhittedParams (None: eps 1e-7, eta 1.33, max_depth 8); index / count: a device list as for ao_device.  Returns
        (bounces, end_org, end_dir, rgb): an int32 tensor [n] whose bits are uint32 -- AO_NO_HIT for a miss record, d for a chain whose
        ray d left the scene, d | WHITTED_CUT for a chain cut at the limit --, the last ray traced for the id (float64 [n, 3] each;
        untouched for a miss record and with max_depth 0) and the float32 [n, 3] colour (the environment seen by the escaping ray, zeros
        for a cut chain and for a miss record).  out: such a 4-tuple to fill, any member None; with out=None all four are allocated
        with torch.empty and what the call does not write is UNSPECIFIED.  Synchronous: the outputs are complete on return."""
        import torch
        what = "whitted_device"
        n, prim, t, u, v = self._ao_batch_in(what, org, dr, records, None, None)
        params = self._whitted_params(what, params)
        dev = org.device
        ip, ni, cp = _list_args(index, count, what)
        if index is None and count is not None:
            ni = n
        if out is None:
            out = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 3), dtype=torch.float64, device=dev),
                   torch.empty((n, 3), dtype=torch.float64, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev))
        if not isinstance(out, (tuple, list)) or len(out) != 4:
            raise ValueError("%s: out must be a (bounces, end_org, end_dir, rgb) 4-tuple (any member may be None)" % what)
        ob, oeo, oed, orgb = out
        words = (torch.int32, getattr(torch, "uint32", torch.int32))
        if ob is not None and not (isinstance(ob, torch.Tensor) and ob.is_cuda and ob.dtype in words and ob.dim() == 1 and ob.shape[0] == n and ob.is_contiguous()):
            raise ValueError("%s: bounces must be a contiguous int32 / uint32 device tensor [n]" % what)
        for name, x, dt in (("end_org", oeo, torch.float64), ("end_dir", oed, torch.float64), ("rgb", orgb, torch.float32)):
            if x is not None and not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == dt and tuple(x.shape) == (n, 3) and x.is_contiguous()):
                raise ValueError("%s: %s must be a contiguous %s device tensor [n, 3]" % (what, name, "float64" if dt == torch.float64 else "float32"))
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        stream = getattr(stream, "cuda_stream", stream)
        _check(self.L.lh_accel_whitted_device(self.h, n, _dptr(org), _dptr(dr), _dptr(prim), _dptr(t), _dptr(u), _dptr(v), C.byref(params),
                                              ip, ni, cp, _dptr(ob), _dptr(oeo), _dptr(oed), _dptr(orgb), C.c_void_p(stream)), "lh_accel_whitted_device")
        return out

    def whitted_host(self, org, dr, records, params=None):
        """lh_accel_whitted_host: host arrays (org, dr [n, 3]; records = (prim, t, u, v)), params as whitted_device ->
        (bounces uint32 [n], end_org float64 [n, 3], end_dir float64 [n, 3], rgb float32 [n, 3]); the end rays of a miss record (and
        of every record with max_depth 0) are zeros"""
        what = "whitted_host"
        params = self._whitted_params(what, params)
        o = _np(org, np.float64).reshape(-1, 3); d = _np(dr, np.float64).reshape(-1, 3); n = o.shape[0]
        if d.shape[0] != n or len(records) != 4:
            raise ValueError("%s: org, dr and the (prim, t, u, v) records must describe the same rays" % what)
        p = _np(records[0], np.uint32).reshape(-1); t = _np(records[1], np.float64).reshape(-1)
        u = _np(records[2], np.float64).reshape(-1); v = _np(records[3], np.float64).reshape(-1)
        if not (p.shape[0] == t.shape[0] == u.shape[0] == v.shape[0] == n):
            raise ValueError("%s: org, dr and the (prim, t, u, v) records must describe the same rays" % what)
        b = np.empty(n, np.uint32); eo = np.zeros((n, 3)); ed = np.zeros((n, 3)); rgb = np.empty((n, 3), np.float32)
        _check(self.L.lh_accel_whitted_host(self.h, n, o.ctypes.data, d.ctypes.data, p.ctypes.data, t.ctypes.data, u.ctypes.data, v.ctypes.data,
                                            C.byref(params), b.ctypes.data, eo.ctypes.data, ed.ctypes.data, rgb.ctypes.data), "lh_accel_whitted_host")
        return b, eo, ed, rgb

    @staticmethod
    def _whitted_params(what, params):
        if params is None:
            params = WhittedParams()
        if not isinstance(params, WhittedParams):
            raise ValueError("%s: params must be a WhittedParams" % what)
        return params

    def _batch_stage_host(self, kind, params, lights, org, dr, records, gather_nsamples, seed, key, uniforms):
        """the five host forms: the row of _BATCH_STAGES, the checks and the call (params None: the type's defaults)"""
        sg = self._BATCH_STAGES[kind]
        what = kind + "_host"
        params, pargs, _ = self._stage_args(what, sg, params, lights)
        o = _np(org, np.float64).reshape(-1, 3); d = _np(dr, np.float64).reshape(-1, 3); n = o.shape[0]
        if d.shape[0] != n or len(records) != 4:
            raise ValueError("%s: org, dr and the (prim, t, u, v) records must describe the same rays" % what)
        p = _np(records[0], np.uint32).reshape(-1); t = _np(records[1], np.float64).reshape(-1)
        u = _np(records[2], np.float64).reshape(-1); v = _np(records[3], np.float64).reshape(-1)
        if not (p.shape[0] == t.shape[0] == u.shape[0] == v.shape[0] == n):
            raise ValueError("%s: org, dr and the (prim, t, u, v) records must describe the same rays" % what)
        k = None if key is None else _np(key, np.uint64).reshape(-1)
        if k is not None and k.shape[0] != n:
            raise ValueError("%s: %s" % (what, sg.host_key))
        un = None if uniforms is None else _np(uniforms, np.float64).reshape(-1)
        cnt = np.empty(n, np.uint32); rad = np.empty((n, 3) if sg.rgb else n, np.float32)
        mid = self._stage_mid(sg, gather_nsamples, pargs, (int(seed), None if k is None else k.ctypes.data, None if un is None else un.ctypes.data,
                                                           0 if un is None else un.shape[0]))
        _check(getattr(self.L, sg.host)(self.h, n, o.ctypes.data, d.ctypes.data, p.ctypes.data, t.ctypes.data, u.ctypes.data, v.ctypes.data, *mid,
                                        cnt.ctypes.data, rad.ctypes.data), sg.host)
        return cnt, rad

    def scratch(self, which, dtype, width):
        """view (copy to host) of a scratch buffer of the last render_ao_tile call"""
        p = C.c_void_p(); n = C.c_size_t()
        _check(self.L.lh_render_scratch(self.h, which, C.byref(p), C.byref(n)), "lh_render_scratch")
        count = n.value * width
        host = np.empty(count, dtype)
        if count:
            hip = C.CDLL("libamdhip64.so")
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            assert hip.hipMemcpy(host.ctypes.data, p, host.nbytes, 2) == 0
        return host.reshape(n.value, width) if width > 1 else host


class _AccelView(HipAccel):
    """a replica of a HipMulti as a HipAccel (borrowed handle: closing it does nothing)"""

    def __init__(self, handle, device):        # noqa: D401 -- no lh_accel_create here
        self.L = lib(); self.h = C.c_void_p(handle); self.device = int(device); self.committed = True; self._npos = []

    def close(self):
        self.h = None


class HipMulti:
    """lh_multi_t: the G GPUs of one node from one process -- one host build, replicated; frames through a tile
    queue with the slabs gathered on device 0; ray dumps in contiguous slices."""

    def __init__(self, devices=None):
        self.L = lib()
        self.h = C.c_void_p()
        if devices is None:
            _check(self.L.lh_multi_create(C.byref(self.h), 0, None), "lh_multi_create")
        else:
            arr = (C.c_int * len(devices))(*[int(d) for d in devices])
            _check(self.L.lh_multi_create(C.byref(self.h), len(devices), arr), "lh_multi_create")
        self.n = int(self.L.lh_multi_ndevices(self.h))
        self.devices = list(devices) if devices is not None else list(range(self.n))
        _live.add(self)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.lh_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_mesh(self, positions, indices):
        P = _np(positions, np.float64); I = _np(indices, np.uint32).reshape(-1)
        _check(self.L.lh_multi_add_mesh(self.h, P.shape[0], P.ctypes.data, P.shape[1] * 8, I.shape[0], I.ctypes.data), "lh_multi_add_mesh")

    def set_normals(self, mesh, normals, two_side=0):
        N = _np(normals, np.float64) if normals is not None else None
        _check(self.L.lh_multi_set_normals(self.h, int(mesh), N.ctypes.data if N is not None else None,
                                           (N.shape[1] * 8) if N is not None else 24, int(two_side)), "lh_multi_set_normals")

    def commit(self, build_threads=0):
        _check(self.L.lh_multi_commit(self.h, int(build_threads)), "lh_multi_commit")

    def accel(self, k):
        return _AccelView(self.L.lh_multi_accel(self.h, int(k)), self.devices[k])

    def set_material(self, mesh, material):
        _check(self.L.lh_multi_set_material(self.h, int(mesh), C.byref(material)), "lh_multi_set_material")

    def set_texture(self, mesh, texels):
        """lh_multi_set_texture: every replica gets the texture ([h, w, 4] float32 numpy; None removes it), after commit"""
        if texels is None:
            _check(self.L.lh_multi_set_texture(self.h, int(mesh), None, 0, 0), "lh_multi_set_texture")
            return
        T = _np(texels, np.float32)
        if T.ndim != 3 or T.shape[2] != 4:
            raise ValueError("set_texture: texels must be [h, w, 4]")
        _check(self.L.lh_multi_set_texture(self.h, int(mesh), T.ctypes.data, int(T.shape[1]), int(T.shape[0])), "lh_multi_set_texture")

    def set_environment(self, rgb=(1.0, 1.0, 1.0), envmap=None):
        e = Environment()
        for k in range(3):
            e.rgb[k] = float(rgb[k])
        m = None
        if envmap is not None:
            m = np.ascontiguousarray(envmap, np.float32)
            e.map_rgba = m.ctypes.data; e.height, e.width = m.shape[0], m.shape[1]
        _check(self.L.lh_multi_set_environment(self.h, C.byref(e)), "lh_multi_set_environment")

    def intersect_host(self, org, dr, mode=MODE_CLOSEST):
        o = _np(org, np.float64).reshape(-1, 3); d = _np(dr, np.float64).reshape(-1, 3)
        n = o.shape[0]
        if mode == MODE_CLOSEST:
            prim = np.empty(n, np.uint32); t = np.empty(n); u = np.empty(n); v = np.empty(n)
            _check(self.L.lh_multi_intersect_host(self.h, n, o.ctypes.data, d.ctypes.data, prim.ctypes.data, t.ctypes.data,
                                                  u.ctypes.data, v.ctypes.data, None, mode), "lh_multi_intersect_host")
            return prim, t, u, v
        occ = np.empty(n, np.uint8)
        _check(self.L.lh_multi_intersect_host(self.h, n, o.ctypes.data, d.ctypes.data, None, None, None, None, occ.ctypes.data, mode),
               "lh_multi_intersect_host")
        return occ

    def render_ao_frame(self, cam, pixel_samples, gather_nsamples, seed=1, tile=512):
        """-> (rgb [H,W,3] float32 host array, stats, per-replica busy seconds)"""
        rgb = np.empty((cam.height, cam.width, 3), np.float32); st = TileStats(); secs = (C.c_double * self.n)()
        _check(self.L.lh_multi_render_ao_frame_host(self.h, C.byref(cam), pixel_samples, gather_nsamples, int(seed), int(tile),
                                                    rgb.ctypes.data, C.byref(st), secs), "lh_multi_render_ao_frame_host")
        return rgb, {k: int(getattr(st, k)) for k, _ in st._fields_}, list(secs)

    def render_pt_frame(self, cam, spp, spp_chunk=0, max_vertices=8, flags=0, seed=1, tile=512):
        rgb = np.empty((cam.height, cam.width, 3), np.float32); st = PtStats(); secs = (C.c_double * self.n)()
        _check(self.L.lh_multi_render_pt_frame_host(self.h, C.byref(cam), int(spp), int(spp_chunk), int(max_vertices), int(flags),
                                                    int(seed), int(tile), rgb.ctypes.data, C.byref(st), secs),
               "lh_multi_render_pt_frame_host")
        return rgb, {k: int(getattr(st, k)) for k, _ in st._fields_}, list(secs)


DIST_RCCL, DIST_SHM = 0, 1


def pack_records16(prim, t, u, v, out, n=None, stream=None):
    """lh_dist_pack_records16: the first n hit records (prim i32/u32, t, u, v f64 CUDA tensors) -> n 16-byte wire records
    {prim u32, t, u, v f32} in `out` (a CUDA uint8 tensor of >= 16 n bytes)"""
    import torch
    n = int(prim.shape[0]) if n is None else int(n)
    L = lib()
    L.lh_dist_pack_records16.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    s = stream if stream is not None else torch.cuda.current_stream(prim.device)
    _check(L.lh_dist_pack_records16(n, prim.data_ptr(), t.data_ptr(), u.data_ptr(), v.data_ptr(), out.data_ptr(), C.c_void_p(s.cuda_stream)),
           "lh_dist_pack_records16")
    return out


class HipDist:
    """lh_dist_t: this process as one rank of a one-process-per-GPU job (RCCL over xGMI through the C ABI; DIST_SHM when the
    ranks share a device).  Rendezvous: `unique_id()` on rank 0 + any out-of-band channel (torch.distributed's store), or a
    fresh file path."""

    @staticmethod
    def unique_id():
        buf = (C.c_ubyte * 128)()
        _check(lib().lh_dist_unique_id(buf), "lh_dist_unique_id")
        return bytes(buf)

    def __init__(self, rank, world, device, unique_id=None, rendezvous=None, transport=DIST_RCCL):
        self.L = lib(); self.h = C.c_void_p()
        self.L.lh_dist_init.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]
        self.L.lh_dist_init_file.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
        if rendezvous is not None:
            _check(self.L.lh_dist_init_file(C.byref(self.h), str(rendezvous).encode(), int(rank), int(world), int(device)), "lh_dist_init_file")
        else:
            assert unique_id is not None and len(unique_id) == 128
            _check(self.L.lh_dist_init(C.byref(self.h), bytes(unique_id), int(rank), int(world), int(device), int(transport)), "lh_dist_init")
        self.rank, self.world, self.device = int(rank), int(world), int(device)
        self.transport = int(self.L.lh_dist_transport(self.h))
        _live.add(self)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.lh_dist_destroy.argtypes = [C.c_void_p]
            self.L.lh_dist_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def barrier(self):
        self.L.lh_dist_barrier.argtypes = [C.c_void_p]
        _check(self.L.lh_dist_barrier(self.h), "lh_dist_barrier")

    def host_barrier(self):
        """the ranks of one node meet in shared memory (microseconds): the barrier around a timed frame"""
        self.L.lh_dist_host_barrier.argtypes = [C.c_void_p]
        _check(self.L.lh_dist_host_barrier(self.h), "lh_dist_host_barrier")

    @staticmethod
    def _stream_of(tensor, stream):
        """the stream a collective on `tensor` is enqueued on: the caller's, else torch's CURRENT stream of the tensor's device --
        behind whatever torch op produced the tensor (the communicator's private stream has no such dependency)"""
        import torch
        if stream is None:
            cur = torch.cuda.current_stream(tensor.device)
            if cur.cuda_stream == 0:
                # torch's default stream has handle 0, which lh_dist_* reads as "the communicator's own stream" -- a non-blocking
                # stream with no dependency on the legacy default stream: finish the producer first
                cur.synchronize()
            return C.c_void_p(cur.cuda_stream)
        return C.c_void_p(stream.cuda_stream) if hasattr(stream, "cuda_stream") else C.c_void_p(stream)

    def broadcast(self, tensor, stream=None):
        """in-place broadcast of a CUDA tensor from rank 0 (stream: a torch.cuda.Stream or a raw handle; default: torch's current stream)"""
        self.L.lh_dist_broadcast.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        _check(self.L.lh_dist_broadcast(self.h, tensor.data_ptr(), tensor.numel() * tensor.element_size(), self._stream_of(tensor, stream)), "lh_dist_broadcast")
        return tensor

    def gather(self, tensor, stream=None):
        """equal-sized contiguous CUDA tensors to rank 0 -> [world, ...] there, None elsewhere"""
        import torch
        t = tensor.contiguous()
        out = torch.empty((self.world,) + tuple(t.shape), dtype=t.dtype, device=t.device) if self.rank == 0 else None
        self.L.lh_dist_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        _check(self.L.lh_dist_gather(self.h, t.data_ptr(), t.numel() * t.element_size(), out.data_ptr() if out is not None else None, self._stream_of(t, stream)), "lh_dist_gather")
        torch.cuda.synchronize(t.device)
        return out

    def broadcast_scene(self, acc):
        """rank 0: a committed HipAccel; other ranks: a fresh one (committed on return: no build on those ranks)"""
        self.L.lh_dist_broadcast_scene.argtypes = [C.c_void_p, C.c_void_p]
        _check(self.L.lh_dist_broadcast_scene(self.h, acc.h), "lh_dist_broadcast_scene")
        return acc

    def render_ao_frame(self, acc, cam, pixel_samples, gather_nsamples, seed=1, band_rows=0):
        """-> (frame [H, W, 3] float32 numpy on rank 0 | None, stats)"""
        rgb = np.empty((cam.height, cam.width, 3), np.float32) if self.rank == 0 else None
        st = TileStats()
        self.L.lh_dist_render_ao_frame_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
        _check(self.L.lh_dist_render_ao_frame_host(self.h, acc.h, C.byref(cam), int(pixel_samples), int(gather_nsamples), int(seed), int(band_rows),
                                                   rgb.ctypes.data if rgb is not None else None, C.byref(st)), "lh_dist_render_ao_frame_host")
        return rgb, {"primary_rays": st.primary_rays, "primary_hits": st.primary_hits, "ao_rays": st.ao_rays, "ao_occluded": st.ao_occluded}
