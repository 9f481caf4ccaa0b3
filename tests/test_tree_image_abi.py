"""The read-only image of the resident traversal trees (lh_accel_tree_image): header, library and binding agree, without a GPU.  The GPU side is
tests/test_gpu_tree_image.py (an accelerator that is created but not committed needs a device: its refusal is checked there)."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np

import lucille_amd as la
from lucille_amd import binding
from tests import tree_check as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["ntris", "nlive", "nq4", "q4_depth", "q4_stack", "nq8", "q8_depth", "device_built", "bmin", "bmax", "grid_lo", "grid_step", "scene_r"]


def test_library_exports_the_entry_point():
    L = C.CDLL(la.build_library())
    assert hasattr(L, "lh_accel_tree_image")
    assert "lh_accel_tree_image" in binding.ABI_SYMBOLS


def test_header_declares_it_and_the_info_struct(tmp_path):
    """a C program compiled against include/lucille_hip.h takes the function's address with its declared type and prints the size and the
    offsets of lh_tree_image_t: they are the binding's structure's"""
    src = tmp_path / "tree_image.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "lucille_hip.h"
int main(void)
{
    int (*f)(lh_accel_t *, lh_tree_image_t *, void *, void *, void *, void *) = lh_accel_tree_image;
    printf("%zu %d", sizeof(lh_tree_image_t), f != NULL);
#define O(F) printf(" %zu", offsetof(lh_tree_image_t, F))
    O(ntris); O(nlive); O(nq4); O(q4_depth); O(q4_stack); O(nq8); O(q8_depth); O(device_built); O(bmin); O(bmax); O(grid_lo); O(grid_step); O(scene_r);
    printf("\n");
    return 0;
}
''')
    exe = tmp_path / "tree_image"
    lib_dir = os.path.join(ROOT, "lucille_amd", "csrc")
    la.build_library()
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-llucille_hip", "-Wl,-rpath," + lib_dir])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    T = binding.TreeImage
    assert [n for n, _ in T._fields_] == FIELDS
    assert got == [C.sizeof(T), 1] + [getattr(T, n).offset for n in FIELDS]
    assert C.sizeof(T) == 8 * 4 + 13 * 4 and T.scene_r.offset == 80


def test_binding_prototype_method_and_record_layouts():
    L = binding.lib()
    vp = C.c_void_p
    assert L.lh_accel_tree_image.argtypes == [vp, C.POINTER(binding.TreeImage), vp, vp, vp, vp]
    assert la.TreeImage is binding.TreeImage
    assert list(inspect.signature(la.HipAccel.tree_image).parameters) == ["self"]
    # lh_q4node_t, lh_q8node_t, lh_tri32_t (lh_bvh.h): 64, 128 and 48 bytes, the words before the references, prim at byte 36
    A = la.HipAccel
    assert (A.Q4_NODE.itemsize, A.Q8_NODE.itemsize, A.TRI32.itemsize) == (64, 128, 48)
    assert A.Q4_NODE.fields["ref"][1] == 48 and A.Q8_NODE.fields["ref"][1] == 96
    assert [A.TRI32.fields[n][1] for n in ("v0", "e1", "e2", "prim", "ne1", "ne2")] == [0, 12, 24, 36, 40, 44]
    assert A.TRI32 == tc.TRI32                    # the checker reads the same records
    w, r = tc.split_nodes(np.zeros(3, A.Q8_NODE), 8)
    assert w.shape == (3, 8, 3) and r.shape == (3, 8)


def test_the_record_sizes_are_the_librarys(tmp_path):
    """... and lh_bvh.h's own: the sizes the image is copied with"""
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lh_bvh.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(lh_q4node_t), '
                   'sizeof(lh_q8node_t), sizeof(lh_tri32_t), sizeof(lh_tri64_t), offsetof(lh_q4node_t, ref), offsetof(lh_tri32_t, prim)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lucille_amd", "csrc"), str(src), "-o", str(exe), "-lm"])
    assert [int(x) for x in subprocess.check_output([str(exe)]).decode().split()] == [64, 128, 48, 72, 48, 36]


def test_a_null_accelerator_is_refused_before_anything_is_looked_at():
    L = binding.lib()
    info = binding.TreeImage()
    assert L.lh_accel_tree_image(None, C.byref(info), None, None, None, None) == -1
    assert "lh_accel_tree_image: accel not committed" in L.lh_last_error().decode()
    assert L.lh_accel_tree_image(None, None, None, None, None, None) == -1
    assert bytes(info) == bytes(C.sizeof(info))            # nothing was written
