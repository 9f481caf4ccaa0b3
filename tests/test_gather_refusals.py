"""Which refusal of the gather stage's entry points wins, and its full text, without a GPU: the five *_device batch entry points, the five *_host
ones, the five tiles and the three *_rays_device ones, each called through binding.lib() with one fault at a time and then with pairs of faults
that show the order.  No accelerator can be created without a device, so every call is made on a NULL one: `!a || !a->committed` is one branch,
and a created accelerator that was never committed gives the same answers.  The strings are those of the commit before the entry points came to
share their bodies; the refusals behind "not committed" (NULL outputs, capacity_rays, "uniforms given") stay with the GPU tests that match them."""
import ctypes as C

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding

KINDS = ("ao", "dirt", "env", "lights", "area_lights")
FN = {"device": {k: "lh_accel_%s_device" % k for k in KINDS}, "host": {k: "lh_accel_%s_host" % k for k in KINDS},
      "tile": {k: "lh_render_%s_tile" % k for k in KINDS},
      "rays": {"ao": "lh_accel_ao_rays_device", "lights": "lh_accel_light_rays_device", "area_lights": "lh_accel_area_light_rays_device"}}

# the full text of every refusal met below; {f}: the entry point's name
MSG = {
    "dirt": "{f}: bad dirt parameters (near_clip nan, far_clip 0.5, eps 1e-05: all finite, 0 <= near_clip < far_clip <= 1e38, eps >= 0)",
    "env": "{f}: bad environment-gather parameters (eps -1, scale 1: both finite, eps >= 0, scale >= 0)",
    "lights": "{f}: bad lights (1 .. 31 lights in host memory, every v and rgb finite, a directional v not zero, flags within POINT | COSINE | INVSQ, "
              "INVSQ only with POINT, reserved 0; eps 1e-05 finite and >= 0)",
    "area_lights": "{f}: bad area lights (1 .. 31 lights in host memory, every rgb finite, flags within COSINE | FACING | INVSQ | PDF, reserved 0, ntris >= 1 "
                   "and first_tri + ntris within the 0 triangles of lh_accel_set_emitters; eps 1e-05 finite and >= 0, 0 < bound 1 <= 1, nsamples 16 in "
                   "1 .. 1024, reserved 0)",
    "ns0": "{f}: gather_nsamples must be at least 1 (0 given)",
    "list": "{f}: the list and its count are 32-bit words: a pointer is not 4-byte aligned",
    "key": "{f}: keys and uniforms are 64-bit words: a pointer is not 8-byte aligned",
    "out32": "{f}: the outputs are 32-bit words: a pointer is not 4-byte aligned",
    "out64_ao": "{f}: the ray arrays are doubles: a pointer is not 8-byte aligned",
    "out64_lights": "{f}: the ray and bound arrays are doubles: a pointer is not 8-byte aligned",
    "out64_area_lights": "{f}: the ray, bound and weight arrays are doubles: a pointer is not 8-byte aligned",
    "none": "{f}: accel not committed",
}

# (form, kind, the faults of the call, the key of the refusal that wins).  Faults: "params" -- bad parameters (dirt, env) or an empty list (lights;
# the area kind needs none: without an emitter table every list is refused); "ns0" -- gather_nsamples 0; "out64" -- a misaligned double output;
# "out32" -- a misaligned 32-bit output; "key" -- a misaligned key; "list" / "count" -- a misaligned list or count
CASES = []
for _k in ("ao", "dirt", "env"):
    _p = [] if _k == "ao" else [(("params",), _k), (("params", "ns0"), _k), (("params", "out32"), _k), (("params", "list", "key"), _k)]
    CASES += [("device", _k, f, m) for f, m in _p + [
        (("ns0",), "ns0"), (("list",), "list"), (("count",), "list"), (("key",), "key"), (("out32",), "out32"), ((), "none"),
        (("ns0", "list"), "ns0"), (("list", "key"), "list"), (("key", "out32"), "key"), (("ns0", "key", "out32"), "ns0")]]
    # the host forms hand no key, list or output to the shared check: their pointers are the host's own
    CASES += [("host", _k, f, m) for f, m in _p[:2] + [(("ns0",), "ns0"), (("key",), "none"), (("out32",), "none"), ((), "none")]]
    # a tile looks at its counts behind the accelerator
    CASES += [("tile", _k, f, m) for f, m in _p[:2] + [(("ns0",), "none"), ((), "none")]]
CASES += [("device", "lights", f, m) for f, m in [
    (("params",), "lights"), (("params", "list"), "lights"), (("params", "out32"), "lights"),
    (("list",), "list"), (("count",), "list"), (("out32",), "out32"), ((), "none"), (("list", "out32"), "list")]]
CASES += [("host", "lights", f, m) for f, m in [(("params",), "lights"), (("out32",), "none"), ((), "none")]]
CASES += [("tile", "lights", f, m) for f, m in [(("params",), "lights"), ((), "none")]]
# AO: the double outputs' alignment first; light: the parameters, then the double outputs, then the shared check
CASES += [("rays", "ao", f, m) for f, m in [
    (("out64",), "out64_ao"), (("ns0",), "ns0"), (("key",), "key"), (("out32",), "out32"), ((), "none"),
    (("out64", "ns0"), "out64_ao"), (("out64", "key", "out32"), "out64_ao"), (("ns0", "key"), "ns0"), (("key", "out32"), "key")]]
CASES += [("rays", "lights", f, m) for f, m in [
    (("params",), "lights"), (("out64",), "out64_lights"), (("out32",), "out32"), ((), "none"),
    (("params", "out64"), "lights"), (("params", "out32"), "lights"), (("out64", "out32"), "out64_lights")]]
# the area kind without an emitter table: whatever else is wrong, "bad area lights" -- the parameters' refusal comes first
for _form in ("device", "host", "tile", "rays"):
    CASES += [(_form, "area_lights", f, "area_lights") for f in [(), ("params",), ("key",), ("out32",), ("list",), ("out64",), ("key", "out32", "list", "out64")]]


class _Arrays:
    def __init__(self, n=8):
        self.n = n
        self.o = np.zeros((n, 3)); self.t = np.zeros(n); self.p = np.zeros(n, np.uint32); self.key = np.zeros(n + 1, np.uint64)
        self.idx = np.zeros(n + 1, np.uint32); self.cnt = np.full(n + 1, 0x77777777, np.uint32); self.val = np.full(3 * n + 1, 7.0, np.float32)
        self.big = np.full((64 * n + 1, 3), 7.0); self.tm = np.full(64 * n + 1, 7.0); self.rgb = np.full((4, 4, 3), 7.0, np.float32)
        self.cam = la.Camera.make(8, 8, 1.0, np.eye(4)); self.st = binding.TileStats()
        self.lights = (la.Light * 2)(la.Light(), la.Light((1, 0, 0), (1, 2, 3), la.LIGHT_POINT))
        self.area = (la.AreaLight * 2)(la.AreaLight(0, 1), la.AreaLight(1, 2, (2, 0, 1)))
        self.bad = {"dirt": la.DirtParams(float("nan"), 0.5, 1e-5), "env": la.EnvParams(eps=-1.0)}

    def untouched(self):
        return ((self.cnt == 0x77777777).all() and (self.val == 7.0).all() and (self.big == 7.0).all() and (self.tm == 7.0).all() and (self.rgb == 7.0).all())


def _args(A, form, kind, faults):
    """the arguments of the entry point behind the accelerator, well-formed but for `faults`"""
    n = A.n
    O, T, P = A.o.ctypes.data, A.t.ctypes.data, A.p.ctypes.data
    sampled = kind in ("ao", "dirt", "env")
    keyed = kind != "lights"
    ns = [0 if "ns0" in faults else 16] if sampled else []
    if kind in ("dirt", "env"):
        params = [C.byref(A.bad[kind]) if "params" in faults else None]
    elif kind == "lights":
        params = [A.lights, 0 if "params" in faults else 2, None]
    elif kind == "area_lights":
        params = [A.area, 0 if "params" in faults else 2, None]
    else:
        params = []
    key = A.key.ctypes.data + 4 if "key" in faults else None
    o32a = A.cnt.ctypes.data + (2 if "out32" in faults else 0)
    if form == "tile":
        return ([C.byref(A.cam), 0, 0, 4, 4, 1] + ns + params + ([1] if keyed else []) + ([None] if sampled else []) + [A.rgb.ctypes.data, C.byref(A.st), None])
    head = [n, O, O, P, T, T, T] + ns + params
    if form == "host":
        return head + ([1, key, None, 0] if keyed else []) + [o32a, A.val.ctypes.data]
    head += [1, key, None] if keyed else []
    if form == "device":
        return head + [A.idx.ctypes.data + 2 if "list" in faults else None, 4 if "list" in faults else (n if "count" in faults else 0),
                       A.idx.ctypes.data + 1 if "count" in faults else None, o32a, A.val.ctypes.data, None]
    o64 = A.big.ctypes.data + (4 if "out64" in faults else 0)
    outs = {"ao": [o64, A.big.ctypes.data], "lights": [A.big.ctypes.data, A.big.ctypes.data, o64],
            "area_lights": [A.big.ctypes.data, A.big.ctypes.data, A.tm.ctypes.data, o64]}[kind]
    return head + [o32a, A.idx.ctypes.data] + outs + [64 * n, None]


@pytest.mark.parametrize("form", ("device", "host", "tile", "rays"))
def test_the_refusal_that_wins_and_its_text(form):
    L = binding.lib()
    A = _Arrays()
    cases = [c for c in CASES if c[0] == form]
    assert {c[1] for c in cases} == set(FN[form])
    for _, kind, faults, msg in cases:
        name = FN[form][kind]
        rc = getattr(L, name)(None, *_args(A, form, kind, faults))
        err = L.lh_last_error().decode()
        assert rc == -1 and err == MSG[msg].format(f=name), (name, faults, err)
    assert A.untouched()
