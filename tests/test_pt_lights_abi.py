"""The path tracer's entry points with area lights (lh_render_pt_tile_lights, lh_render_pt_bands_lights) and lh_pt_lights_t: the C ABI, the binding
and the refusals that need no device.  The rule is tests/test_pta_rule.py, the GPU side tests/test_gpu_pt_area.py."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np

import lucille_amd as la
from lucille_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lh_render_pt_tile_lights", "lh_render_pt_bands_lights")
FIELDS = ("lights", "nlights", "reserved0", "params", "area", "narea", "reserved1", "area_params")


def test_library_exports_the_entry_points():
    L = C.CDLL(la.build_library())
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert all(n in binding.ABI_SYMBOLS for n in NEW)
    assert la.PtLights is binding.PtLights


def test_header_declares_them_and_the_layout_is_the_bindings(tmp_path):
    """a C program compiled against include/lucille_hip.h assigns the two functions to pointers of the stated types and prints the structure's size
    and offsets"""
    src = tmp_path / "ptlights.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "lucille_hip.h"
int main(void)
{
    int (*a)(lh_accel_t *, const lh_camera_t *, int, int, int, int, int, int, int, int, int, const lh_pt_lights_t *, const lh_pt_sink_t *, uint64_t, void *,
             lh_pt_stats_t *, void *) = lh_render_pt_tile_lights;
    int (*b)(lh_accel_t *, const lh_camera_t *, int, int, int, int, int, int, int, int, int, const lh_material_t *, const lh_pt_lights_t *,
             const lh_pt_sink_t *, uint64_t, void *, lh_pt_stats_t *, void *) = lh_render_pt_bands_lights;
    printf("%zu %zu %d %zu", sizeof(lh_pt_lights_t), _Alignof(lh_pt_lights_t), a != NULL && b != NULL, sizeof(lh_pt_sink_t));
    printf(" %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(lh_pt_lights_t, lights), offsetof(lh_pt_lights_t, nlights), offsetof(lh_pt_lights_t, reserved0),
           offsetof(lh_pt_lights_t, params), offsetof(lh_pt_lights_t, area), offsetof(lh_pt_lights_t, narea), offsetof(lh_pt_lights_t, reserved1),
           offsetof(lh_pt_lights_t, area_params));
    return 0;
}
''')
    exe = tmp_path / "ptlights"
    lib_dir = os.path.join(ROOT, "lucille_amd", "csrc")
    la.build_library()
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-llucille_hip", "-Wl,-rpath," + lib_dir])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got[:4] == [C.sizeof(binding.PtLights), C.alignment(binding.PtLights), 1, 96] and got[0] == 48          # the sink's layout did not change
    assert [n for n, _ in binding.PtLights._fields_] == list(FIELDS)
    assert got[4:] == [getattr(binding.PtLights, n).offset for n in FIELDS] == [0, 8, 12, 16, 24, 32, 36, 40]


def test_binding_prototypes_and_signatures():
    L = binding.lib()
    assert [len(getattr(L, n).argtypes) for n in NEW] == [17, 18]
    # as the _lit forms, with the list's three arguments replaced by the one structure
    tl, bl = list(L.lh_render_pt_tile_lit.argtypes), list(L.lh_render_pt_bands_lit.argtypes)
    plp = C.POINTER(binding.PtLights)
    assert list(L.lh_render_pt_tile_lights.argtypes) == tl[:11] + [plp] + tl[14:]
    assert list(L.lh_render_pt_bands_lights.argtypes) == bl[:12] + [plp] + bl[15:]
    assert list(inspect.signature(la.HipAccel.render_pt_tile_lights).parameters) == ["self", "cam", "x0", "y0", "w", "h", "spp_begin", "spp_count", "spp_total",
                                                                                     "max_vertices", "flags", "lights", "params", "area", "area_params",
                                                                                     "sink", "seed", "out", "stream"]
    assert list(inspect.signature(la.HipAccel.render_pt_bands_lights).parameters) == ["self", "cam", "y0_first", "band_rows", "band_stride", "nbands",
                                                                                      "spp_begin", "spp_count", "spp_total", "max_vertices", "flags",
                                                                                      "override", "lights", "params", "area", "area_params", "sink", "seed",
                                                                                      "out", "stream"]


def test_refusals_need_no_device():
    """both lists are refused as their stages refuse them, the reserved words and a misaligned sink pointer by the call itself, all before the
    accelerator is looked at; an area list on no accelerator has no emitter table to lie in; a good call on no accelerator is refused by the
    accelerator; NULL is no lights at all"""
    L = binding.lib()
    cam = la.Camera.make(8, 8, 1.0, np.eye(4))
    rgb = np.full((8, 8, 3), 7.0, np.float32)
    buf = np.zeros(64, np.float64)

    def calls(pl, sink):
        lp = None if pl is None else C.byref(pl)
        sp = None if sink is None else C.byref(sink)
        return [("lh_render_pt_tile_lights", lambda: L.lh_render_pt_tile_lights(None, C.byref(cam), 0, 0, 8, 8, 0, 1, 1, 4, 0, lp, sp, 1, rgb.ctypes.data, None, None)),
                ("lh_render_pt_bands_lights", lambda: L.lh_render_pt_bands_lights(None, C.byref(cam), 0, 4, 4, 2, 0, 1, 1, 4, 0, None, lp, sp, 1, rgb.ctypes.data,
                                                                                  None, None))]

    def refused(pl, sink, *msgs):
        for name, call in calls(pl, sink):
            rc = call()
            err = L.lh_last_error().decode()
            assert rc == -1 and name in err and all(m in err for m in msgs), (name, err)
        assert (rgb == 7.0).all()

    def both(lights=None, nl=None, params=None, area=None, na=None, aparams=None, r0=0, r1=0):
        pl = la.PtLights()
        keep = []
        if lights is not None:
            arr = (la.Light * len(lights))(*lights); keep.append(arr)
            pl.lights = arr
        pl.nlights = (len(lights) if lights is not None else 0) if nl is None else nl
        if area is not None:
            aarr = (la.AreaLight * len(area))(*area); keep.append(aarr)
            pl.area = aarr
        pl.narea = (len(area) if area is not None else 0) if na is None else na
        if params is not None:
            pl.params = C.pointer(params)
        if aparams is not None:
            pl.area_params = C.pointer(aparams)
        pl.reserved0 = r0; pl.reserved1 = r1
        pl._keep = keep
        return pl

    good = [la.Light((0.3, 0.9, 0.2), (1, 1, 1)), la.Light((1, 2, 3), (2, 0, 1), la.LIGHT_POINT | la.LIGHT_COSINE | la.LIGHT_INVSQ)]
    refused(None, None, "not committed")                                 # no lights at all
    refused(both(), None, "not committed")
    refused(both(good), None, "not committed")
    refused(both(good, nl=0), None, "not committed")
    refused(both([la.Light((0, 1, 0), (1, 1, 1))] * 32), None, "bad lights")
    refused(both([la.Light((0, 1, 0), (1, float("nan"), 1))]), None, "bad lights")
    refused(both(nl=2), None, "bad lights")
    refused(both(good, nl=-1), None, "bad lights")
    refused(both(good, params=la.LightsParams(-1.0)), None, "bad lights")
    # the reserved words, before either list is looked at
    refused(both(good, r0=1), None, "reserved")
    refused(both(good, r1=1 << 31), None, "reserved")
    refused(both(r0=7, nl=2), None, "reserved")
    # an area list: no accelerator, so no emitter table its runs could lie in; and every refusal of the rule
    one = [la.AreaLight(0, 1, (1, 1, 1))]
    refused(both(area=one), None, "bad area lights")
    refused(both(good, area=one), None, "bad area lights")
    refused(both(na=1), None, "bad area lights")
    refused(both(area=one, na=-1), None, "bad area lights")
    refused(both(area=one * 32), None, "bad area lights")
    refused(both(area=one, aparams=la.AreaParams(1e-5, 1.0, 0)), None, "bad area lights")
    refused(both(area=one, aparams=la.AreaParams(1e-5, 1.5, 4)), None, "bad area lights")
    refused(both(area=one, na=0), None, "not committed")                # narea == 0: no list needed
    # the delta list is looked at first
    refused(both([la.Light((0, 1, 0), (1, 1, 1), la.LIGHT_INVSQ)], area=one), None, "bad lights")
    # the sink: as the _lit forms
    s = la.PtSinkStruct(); s.capacity = 4
    refused(both(good), s, "not committed")
    for field in ("d_org", "d_v"):
        s = la.PtSinkStruct(); s.capacity = 4; setattr(s, field, buf.ctypes.data + 4)
        refused(None, s, "sink", "not 8-byte aligned")
    for field in ("d_path", "d_direct", "d_counts"):
        s = la.PtSinkStruct(); s.capacity = 4; setattr(s, field, buf.ctypes.data + 2)
        refused(both(good), s, "sink", "not 4-byte aligned")
