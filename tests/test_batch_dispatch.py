"""Which C entry point HipAccel.intersect_device / intersect_device_indexed / intersect_host / intersect_host_tmax call for every
combination of ray format, record format, mode, list, bound, counters and variant, and with which arguments -- without a GPU: the
library is a recording stand-in, the device tensors are fakes (tests/test_tmax_abi.py's, with data_ptr / numel).  The expectation is
the table of the binding's contract (include/lucille_hip.h, the methods' docstrings), written out below independently of the binding.

tests/conftest.py narrows intersect_host / intersect_device while a GPU is visible: this file is for the machines without one."""
import ctypes as C
import itertools

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="tests/conftest.py replaces the methods under test while a GPU is visible")

H = 0xABC0
N = 8
HOST_ARGS = {          # positions of (tmax, formats, the five outputs, mode) in the host entry points' argument lists
    "lh_accel_intersect_host": (None, None, 4, 9),
    "lh_accel_intersect_host_ex": (None, 4, 6, 11),
    "lh_accel_intersect_host_tmax": (4, 5, 7, 12),
}


def val(x):
    """an argument as the C function sees it: NULL and 0 alike"""
    if x is None:
        return 0
    if isinstance(x, C.c_void_p):
        return x.value or 0
    return x


def mem(ptr, count, dtype):
    """count elements at ptr, as a writable array"""
    return np.frombuffer((C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr), dtype=dtype)


class Recorder:
    """stands in for the loaded library: every call is logged and succeeds; a host batch call has its rays read and its outputs written"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            if name in HOST_ARGS:
                self.host(name, [val(a) for a in args])
            return 0
        return f

    def host(self, name, a):
        k_tmax, k_fmt, k_out, k_mode = HOST_ARGS[name]
        n = a[1]
        fmt, rf = (binding.RAYS_F64, binding.REC_F64) if k_fmt is None else (a[k_fmt], a[k_fmt + 1])
        dt = np.float32 if fmt == binding.RAYS_F32 else np.float64
        self.rays = (mem(a[2], 3 * n, dt).copy(), mem(a[3], 3 * n, dt).copy(), None if k_tmax is None else mem(a[k_tmax], n, dt).copy())
        prim, t, u, v, occ = a[k_out:k_out + 5]
        if rf == binding.REC16 and a[k_mode] == la.MODE_CLOSEST:
            assert prim % 16 == 0
            mem(prim, 4 * n, np.uint32)[:] = np.arange(4 * n) + 7
        elif prim:
            mem(prim, n, np.uint32)[:] = np.arange(n) + 7
        for p, add in ((t, 0.5), (u, 0.25), (v, 0.125)):
            if p:
                mem(p, n, np.float64)[:] = np.arange(n) + add
        if occ:
            mem(occ, n, np.uint8)[:] = np.arange(n) % 2


class FakeTensor:
    """enough of a device tensor for the binding, which touches no device before the C call"""
    is_cuda = True
    _next = [0x10000]

    def __init__(self, dtype, shape, device="cuda:0"):
        self.dtype, self.shape, self.device = dtype, shape, device
        self._ptr = self._next[0]; self._next[0] += 0x1000

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return int(np.prod(self.shape))


def accel():
    acc = la.HipAccel.__new__(la.HipAccel)
    acc.L = Recorder()
    acc.h = C.c_void_p(H)
    return acc


LISTS = ("none", "index", "count", "tmax", "index+tmax")
EXTRAS = ("plain", "counters", "variant")
DEVICE_CASES = list(itertools.product((False, True), (False, True), (False, True), LISTS, EXTRAS))


def case_id(c):
    f32, rec16, anyhit, lst, extra = c
    return "-".join(("f32" if f32 else "f64", "rec16" if rec16 else "soa", "any" if anyhit else "closest", lst, extra))


def device_expectation(f32, rec16, anyhit, lst, extra, p):
    """-> ("error", text) or (symbol, arguments); p: the pointers of org, dir, tmax, index, count and the five outputs"""
    mode = la.MODE_ANY if anyhit else la.MODE_CLOSEST
    variant = la.VARIANT_DIRECT if extra == "variant" else la.VARIANT_DEFAULT
    fmt = binding.RAYS_F32 if f32 else binding.RAYS_F64
    rf = binding.REC16 if rec16 else binding.REC_F64
    bounded, listed = "tmax" in lst, lst in ("index", "count", "index+tmax")
    head = (H, N, p["org"], p["dir"])
    outs = tuple(p["outs"])
    if bounded and extra != "plain":
        return "error", "bounded batches (tmax) run the default variant without counters"
    if listed and extra != "plain":
        return "error", "indexed batches run the default variant without counters"
    if listed or bounded:
        lst_args = (p["index"] if "index" in lst else 0, N if listed else 0, p["count"] if lst == "count" else 0)       # no index: all n rays; dense: (NULL, 0, NULL)
        if bounded:
            return "lh_accel_intersect_device_tmax", head + (p["tmax"], fmt, rf) + outs + (mode,) + lst_args + (0,)
        return "lh_accel_intersect_device_indexed", head + (fmt, rf) + outs + (mode,) + lst_args + (0,)
    if f32 or rec16:
        if extra != "plain":
            return "error", "fp32 rays / rec16 records run the default variant without counters"
        return "lh_accel_intersect_device_ex", head + (fmt, rf) + outs + (mode, 0)
    if extra == "counters":
        return "lh_accel_intersect_device_counted", head + outs + (mode, variant)
    return "lh_accel_intersect_device", head + outs + (mode, variant, 0)


@pytest.mark.parametrize("case", DEVICE_CASES, ids=case_id)
def test_intersect_device_dispatch(case, monkeypatch):
    f32, rec16, anyhit, lst, extra = case
    synced = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda dev=None: synced.append(dev))
    dt = torch.float32 if f32 else torch.float64
    org, dr, tmax = FakeTensor(dt, (N, 3)), FakeTensor(dt, (N, 3)), FakeTensor(dt, (N,))
    index, count = FakeTensor(torch.int32, (N,)), FakeTensor(torch.int32, (1,))
    if anyhit:
        out = (FakeTensor(torch.uint8, (N,)),)
        outs = [0, 0, 0, 0, out[0].data_ptr()]
    elif rec16:
        out = (FakeTensor(torch.int32, (N, 4)),)
        outs = [out[0].data_ptr(), 0, 0, 0, 0]
    else:
        out = (FakeTensor(torch.int32, (N,)),) + tuple(FakeTensor(torch.float64, (N,)) for _ in range(3))
        outs = [x.data_ptr() for x in out] + [0]
    p = dict(org=org.data_ptr(), dir=dr.data_ptr(), tmax=tmax.data_ptr(), index=index.data_ptr(), count=count.data_ptr(), outs=outs)
    kw = dict(out=out, mode=la.MODE_ANY if anyhit else la.MODE_CLOSEST, stream=0, records="rec16" if rec16 else "f64")
    if "index" in lst:
        kw["index"] = index
    if lst == "count":
        kw["count"] = count
    if "tmax" in lst:
        kw["tmax"] = tmax
    if extra == "counters":
        kw["counters"] = True
    if extra == "variant":
        kw["variant"] = la.VARIANT_DIRECT
    exp = device_expectation(f32, rec16, anyhit, lst, extra, p)
    acc = accel()
    if exp[0] == "error":
        with pytest.raises(ValueError) as e:
            la.HipAccel.intersect_device(acc, org, dr, **kw)
        assert str(e.value) == exp[1]
        assert acc.L.calls == [] and synced == []
        return
    got = la.HipAccel.intersect_device(acc, org, dr, **kw)
    name, args = acc.L.calls[0]
    assert name == exp[0]
    if name == "lh_accel_intersect_device_counted":
        assert synced == ["cuda:0"]                                        # the counted launch reads its counters behind a device-wide wait
        assert len(args[-1]) == 4 and isinstance(args[-1], C.Array)
        assert tuple(val(a) for a in args[:-1]) == exp[1]
        assert [c[0] for c in acc.L.calls] == [name, "lh_accel_last_retraced"]
        assert got[0] is out and sorted(got[1]) == ["exact", "nodes", "rays", "retraced", "tris"]
    else:
        assert synced == [] and len(acc.L.calls) == 1
        assert tuple(val(a) for a in args) == exp[1]
        assert got is out
    if lst != "none" and extra == "plain":                                 # the method intersect_device forwards a listed batch to
        acc2 = accel()
        kw2 = {k: v for k, v in kw.items() if k not in ("counters", "variant")}
        assert la.HipAccel.intersect_device_indexed(acc2, org, dr, **kw2) is out
        name2, args2 = acc2.L.calls[0]
        if lst == "tmax":                                                  # called directly a dense bounded batch is the list of all n rays
            exp = (exp[0], exp[1][:-4] + (0, N, 0, 0))
        assert (name2, tuple(val(a) for a in args2)) == exp and len(acc2.L.calls) == 1


def test_intersect_device_refuses_before_it_calls():
    acc = accel()
    org = FakeTensor(torch.float64, (N, 3))
    with pytest.raises(ValueError, match="records must be 'f64' or 'rec16'"):
        la.HipAccel.intersect_device(acc, org, org, out=(), stream=0, records="f32")
    with pytest.raises(ValueError, match="records must be 'f64' or 'rec16'"):
        la.HipAccel.intersect_device(acc, org, org, out=(), stream=0, records="f32", index=FakeTensor(torch.int32, (N,)))
    with pytest.raises(ValueError, match="intersect_device: index must be"):
        la.HipAccel.intersect_device(acc, org, org, out=(None,) * 4, stream=0, index=FakeTensor(torch.int64, (N,)))
    with pytest.raises(ValueError, match="intersect_device: count must be"):
        la.HipAccel.intersect_device(acc, org, org, out=(None,) * 4, stream=0, count=FakeTensor(torch.int32, (2,)))
    with pytest.raises(ValueError, match="intersect_device: tmax must be"):
        la.HipAccel.intersect_device(acc, org, org, out=(None,) * 4, stream=0, tmax=FakeTensor(torch.float32, (N,)))
    with pytest.raises(ValueError, match="intersect_device_indexed: tmax must be"):
        la.HipAccel.intersect_device(acc, org, org, out=(None,) * 4, stream=0, tmax=FakeTensor(torch.float32, (N,)), index=FakeTensor(torch.int32, (N,)))
    with pytest.raises(AssertionError):
        la.HipAccel.intersect_device(acc, org, FakeTensor(torch.float32, (N, 3)), out=(None,) * 4, stream=0)
    assert acc.L.calls == []


HOST_CASES = list(itertools.product(("f64", "f32", "mixed"), (False, True), (False, True), (False, True)))


def host_id(c):
    rays, rec16, anyhit, bounded = c
    return "-".join((rays, "rec16" if rec16 else "soa", "any" if anyhit else "closest", "tmax" if bounded else "unbounded"))


@pytest.mark.parametrize("case", HOST_CASES, ids=host_id)
def test_intersect_host_dispatch(case):
    rays, rec16, anyhit, bounded = case
    rng = np.random.default_rng(5)
    org = rng.uniform(-1, 1, (N, 3)).astype(np.float32 if rays != "f64" else np.float64)
    dr = rng.uniform(-1, 1, (N, 3)).astype(np.float32 if rays == "f32" else np.float64)          # mixed: one array of each -> fp64 rays
    tmax = rng.uniform(0, 2, N)                                                                 # taken in the rays' precision
    f32 = rays == "f32"
    dt = np.float32 if f32 else np.float64
    mode = la.MODE_ANY if anyhit else la.MODE_CLOSEST
    fmt, rf = (binding.RAYS_F32 if f32 else binding.RAYS_F64), (binding.REC16 if rec16 else binding.REC_F64)
    kw = dict(mode=mode, records="rec16" if rec16 else "f64")
    runs = [lambda acc: la.HipAccel.intersect_host(acc, org, dr, tmax=tmax if bounded else None, **kw)]
    if bounded:
        runs.append(lambda acc: la.HipAccel.intersect_host_tmax(acc, org, dr, tmax, **kw))
    for run in runs:
        acc = accel()
        got = run(acc)
        assert len(acc.L.calls) == 1
        name, args = acc.L.calls[0]
        a = [val(x) for x in args]
        if bounded:
            assert name == "lh_accel_intersect_host_tmax" and len(a) == 13 and a[5:7] == [fmt, rf]
        elif f32 or rec16:
            assert name == "lh_accel_intersect_host_ex" and len(a) == 12 and a[4:6] == [fmt, rf]
        else:
            assert name == "lh_accel_intersect_host" and len(a) == 10
        assert a[0] == H and a[1] == N and a[-1] == mode
        o, d, tm = acc.L.rays
        assert o.dtype == dt and np.array_equal(o, org.astype(dt).reshape(-1)) and np.array_equal(d, dr.astype(dt).reshape(-1))
        assert (tm is None) == (not bounded) and (tm is None or (tm.dtype == dt and np.array_equal(tm, tmax.astype(dt))))
        outs = a[HOST_ARGS[name][2]:HOST_ARGS[name][2] + 5]
        if anyhit:
            assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (N,)
            assert outs == [0, 0, 0, 0, got.ctypes.data] and np.array_equal(got, np.arange(N) % 2)
        elif rec16:
            assert isinstance(got, np.ndarray) and got.dtype == np.uint32 and got.shape == (N, 4) and got.ctypes.data % 16 == 0
            assert outs == [got.ctypes.data, 0, 0, 0, 0] and np.array_equal(got.reshape(-1), np.arange(4 * N) + 7)
        else:
            assert isinstance(got, tuple) and len(got) == 4
            assert [x.dtype for x in got] == [np.uint32, np.float64, np.float64, np.float64] and all(x.shape == (N,) for x in got)
            assert outs == [x.ctypes.data for x in got] + [0]
            for x, add in zip(got, (7, 0.5, 0.25, 0.125)):
                assert np.array_equal(x, np.arange(N) + add)


def test_intersect_host_refuses_before_it_calls():
    acc = accel()
    o = np.zeros((N, 3))
    for f in (lambda **kw: la.HipAccel.intersect_host(acc, o, o, **kw), lambda **kw: la.HipAccel.intersect_host_tmax(acc, o, o, np.zeros(N), **kw)):
        with pytest.raises(ValueError, match="records must be 'f64' or 'rec16'"):
            f(records="f32")
    with pytest.raises(ValueError) as e:
        la.HipAccel.intersect_host(acc, o, o, tmax=np.zeros(N - 1))
    assert str(e.value) == "intersect_host: tmax must hold one bound per ray (%d for %d rays)" % (N - 1, N)
    with pytest.raises(ValueError) as e:
        la.HipAccel.intersect_host_tmax(acc, o, o, np.zeros(N + 1))
    assert str(e.value) == "intersect_host: tmax must hold one bound per ray (%d for %d rays)" % (N + 1, N)
    assert acc.L.calls == []


def test_an_empty_host_batch_still_calls():
    """n == 0: the C function is asked (it is what says "not committed"), the outputs are empty arrays of the right kinds"""
    acc = accel()
    o = np.zeros((0, 3), np.float32)
    rec = la.HipAccel.intersect_host(acc, o, o, records="rec16")
    assert rec.shape == (0, 4) and rec.dtype == np.uint32
    occ = la.HipAccel.intersect_host(acc, o, o, mode=la.MODE_ANY, tmax=np.zeros(0))
    assert occ.shape == (0,) and occ.dtype == np.uint8
    assert [c[0] for c in acc.L.calls] == ["lh_accel_intersect_host_ex", "lh_accel_intersect_host_tmax"]
