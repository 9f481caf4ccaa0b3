"""The lit path tracer's entry points (lh_render_pt_tile_lit, lh_render_pt_bands_lit) and lh_pt_sink_t: the C ABI, the binding and the refusals
that need no device.  The rule is tests/test_ptl_rule.py, the GPU side tests/test_gpu_pt_lit.py."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np

import lucille_amd as la
from lucille_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lh_render_pt_tile_lit", "lh_render_pt_bands_lit")
SINK_FIELDS = ("d_path", "d_depth", "d_org", "d_dir", "d_prim", "d_t", "d_u", "d_v", "d_thr", "d_direct", "d_counts", "capacity")


def test_library_exports_the_entry_points():
    L = C.CDLL(la.build_library())
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert all(n in binding.ABI_SYMBOLS for n in NEW)
    assert la.PtSink is binding.PtSink and la.PtSinkStruct is binding.PtSinkStruct


def test_header_declares_them_and_the_layout_is_the_bindings(tmp_path):
    """a C program compiled against include/lucille_hip.h assigns the two functions to pointers of the stated types and prints the sink's size and offsets"""
    src = tmp_path / "ptlit.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "lucille_hip.h"
int main(void)
{
    int (*a)(lh_accel_t *, const lh_camera_t *, int, int, int, int, int, int, int, int, int, const lh_light_t *, int, const lh_lights_params_t *,
             const lh_pt_sink_t *, uint64_t, void *, lh_pt_stats_t *, void *) = lh_render_pt_tile_lit;
    int (*b)(lh_accel_t *, const lh_camera_t *, int, int, int, int, int, int, int, int, int, const lh_material_t *, const lh_light_t *, int,
             const lh_lights_params_t *, const lh_pt_sink_t *, uint64_t, void *, lh_pt_stats_t *, void *) = lh_render_pt_bands_lit;
    printf("%zu %zu %d", sizeof(lh_pt_sink_t), _Alignof(lh_pt_sink_t), a != NULL && b != NULL);
    printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(lh_pt_sink_t, d_path), offsetof(lh_pt_sink_t, d_depth), offsetof(lh_pt_sink_t, d_org),
           offsetof(lh_pt_sink_t, d_dir), offsetof(lh_pt_sink_t, d_prim), offsetof(lh_pt_sink_t, d_t), offsetof(lh_pt_sink_t, d_u), offsetof(lh_pt_sink_t, d_v),
           offsetof(lh_pt_sink_t, d_thr), offsetof(lh_pt_sink_t, d_direct), offsetof(lh_pt_sink_t, d_counts), offsetof(lh_pt_sink_t, capacity));
    return 0;
}
''')
    exe = tmp_path / "ptlit"
    lib_dir = os.path.join(ROOT, "lucille_amd", "csrc")
    la.build_library()
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-llucille_hip", "-Wl,-rpath," + lib_dir])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got[:3] == [C.sizeof(binding.PtSinkStruct), C.alignment(binding.PtSinkStruct), 1] and got[0] == 96
    assert [n for n, _ in binding.PtSinkStruct._fields_] == list(SINK_FIELDS)
    assert got[3:] == [getattr(binding.PtSinkStruct, n).offset for n in SINK_FIELDS]


def test_binding_prototypes_and_signatures():
    L = binding.lib()
    assert [len(getattr(L, n).argtypes) for n in NEW] == [19, 20]
    # as the unlit forms, with the four new arguments in their places
    t2, bd = list(L.lh_render_pt_tile2.argtypes), list(L.lh_render_pt_bands.argtypes)
    four = list(L.lh_render_pt_tile_lit.argtypes[11:15])
    assert list(L.lh_render_pt_tile_lit.argtypes) == t2[:11] + four + t2[11:]
    assert list(L.lh_render_pt_bands_lit.argtypes) == bd[:12] + four + bd[12:]
    assert list(inspect.signature(la.HipAccel.render_pt_tile_lit).parameters) == ["self", "cam", "x0", "y0", "w", "h", "spp_begin", "spp_count", "spp_total",
                                                                                  "max_vertices", "flags", "lights", "params", "sink", "seed", "out", "stream"]
    assert list(inspect.signature(la.HipAccel.render_pt_bands_lit).parameters) == ["self", "cam", "y0_first", "band_rows", "band_stride", "nbands", "spp_begin",
                                                                                   "spp_count", "spp_total", "max_vertices", "flags", "override", "lights",
                                                                                   "params", "sink", "seed", "out", "stream"]


def test_refusals_need_no_device():
    """the list is refused as the light stage refuses it and a misaligned sink pointer by the call itself, before the accelerator is looked at; a
    good call on no accelerator by the accelerator; nlights == 0 needs no list"""
    L = binding.lib()
    cam = la.Camera.make(8, 8, 1.0, np.eye(4))
    rgb = np.full((8, 8, 3), 7.0, np.float32)
    buf = np.zeros(64, np.float64)

    def calls(lights, nl, params, sink):
        pp = None if params is None else C.byref(params)
        sp = None if sink is None else C.byref(sink)
        return [("lh_render_pt_tile_lit", lambda: L.lh_render_pt_tile_lit(None, C.byref(cam), 0, 0, 8, 8, 0, 1, 1, 4, 0, lights, nl, pp, sp, 1, rgb.ctypes.data, None, None)),
                ("lh_render_pt_bands_lit", lambda: L.lh_render_pt_bands_lit(None, C.byref(cam), 0, 4, 4, 2, 0, 1, 1, 4, 0, None, lights, nl, pp, sp, 1, rgb.ctypes.data,
                                                                            None, None))]

    def refused(lights, nl, params, sink, *msgs):
        for name, call in calls(lights, nl, params, sink):
            rc = call()
            err = L.lh_last_error().decode()
            assert rc == -1 and name in err and all(m in err for m in msgs), (name, err)
        assert (rgb == 7.0).all()

    def arr(ls):
        return (la.Light * len(ls))(*ls)

    good = arr([la.Light((0.3, 0.9, 0.2), (1, 1, 1)), la.Light((1, 2, 3), (2, 0, 1), la.LIGHT_POINT | la.LIGHT_COSINE | la.LIGHT_INVSQ)])
    refused(good, 2, None, None, "not committed")
    refused(None, 0, None, None, "not committed")                       # no lights: no list needed
    refused(good, 0, None, None, "not committed")
    refused(arr([la.Light((0, 1, 0), (1, 1, 1))] * 31), 31, None, None, "not committed")
    refused(arr([la.Light((0, 1, 0), (1, 1, 1))] * 32), 32, None, None, "bad lights")
    refused(arr([la.Light((0, 1, 0), (1, float("nan"), 1))]), 1, None, None, "bad lights")
    refused(arr([la.Light((0, 1, 0), (1, 1, 1), la.LIGHT_INVSQ)]), 1, None, None, "bad lights")
    refused(None, 2, None, None, "bad lights")
    refused(good, -1, None, None, "bad lights")
    refused(good, 2, la.LightsParams(-1.0), None, "bad lights")
    # the sink: every array may be NULL; doubles on 8 bytes, words on 4
    s = la.PtSinkStruct(); s.capacity = 4
    refused(good, 2, None, s, "not committed")
    for field in ("d_org", "d_dir", "d_t", "d_u", "d_v"):
        s = la.PtSinkStruct(); s.capacity = 4; setattr(s, field, buf.ctypes.data + 4)
        refused(None, 0, None, s, "sink", "not 8-byte aligned")
    for field in ("d_path", "d_depth", "d_prim", "d_thr", "d_direct", "d_counts"):
        s = la.PtSinkStruct(); s.capacity = 4; setattr(s, field, buf.ctypes.data + 2)
        refused(None, 0, None, s, "sink", "not 4-byte aligned")
        s = la.PtSinkStruct(); s.capacity = 4; setattr(s, field, buf.ctypes.data + 4)
        refused(None, 0, None, s, "not committed")
