"""What a re-commit of an updatable device-mesh accelerator redoes (lucille_amd/csrc/lh_recommit.h, read by lh_commit.hip lh_accel_recommit) on the
CPU: the header, compiled into the stand-alone program tests/cpu_model/lh_recommit_check.c with -fsanitize=address,undefined, over its whole input
space -- positions staged, attributes staged, the compare's answer, the resident scene's 8-wide nodes, "wide8" -- against the table below, written
from the contract in include/lucille_hip.h and not from the header:

  - positions staged: flatten and compare, whatever else; the trees only where the records changed; the 8-wide nodes beside the trees where the old
    scene had them or "wide8" is 1, never without the trees;
  - positions or attributes staged: gather again;
  - nothing staged: nothing, whatever the other inputs say."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_model", "lh_recommit_check.c")

# (pos_staged, attr_staged) -> for (records_changed, had_q8) -> for wide8 in (-1, 0, 1): "flatten compare trees q8 gather"
TABLE = {
    (0, 0): {(0, 0): ["00000", "00000", "00000"], (0, 1): ["00000", "00000", "00000"], (1, 0): ["00000", "00000", "00000"], (1, 1): ["00000", "00000", "00000"]},
    (0, 1): {(0, 0): ["00001", "00001", "00001"], (0, 1): ["00001", "00001", "00001"], (1, 0): ["00001", "00001", "00001"], (1, 1): ["00001", "00001", "00001"]},
    (1, 0): {(0, 0): ["11001", "11001", "11001"], (0, 1): ["11001", "11001", "11001"], (1, 0): ["11101", "11101", "11111"], (1, 1): ["11111", "11111", "11111"]},
    (1, 1): {(0, 0): ["11001", "11001", "11001"], (0, 1): ["11001", "11001", "11001"], (1, 0): ["11101", "11101", "11111"], (1, 1): ["11111", "11111", "11111"]},
}


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("recommit") / "lh_recommit_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr          # a sanitizer report ends the program with a message
    out = {}
    for line in r.stdout.splitlines():
        k, v = line.split(" : ")
        out[tuple(int(x) for x in k.split())] = v.replace(" ", "")
    return out


def test_the_whole_input_space_against_the_table(rows):
    assert len(rows) == 2 * 2 * 2 * 2 * 3
    for (pos, attr), by in TABLE.items():
        for (changed, had), per_wide8 in by.items():
            for w, want in zip((-1, 0, 1), per_wide8):
                assert rows[(pos, attr, changed, had, w)] == want, (pos, attr, changed, had, w)


def test_invariants(rows):
    for (pos, attr, changed, had, w), v in rows.items():
        flatten, compare, trees, q8, gather = (int(c) for c in v)
        assert flatten == compare == pos
        assert not trees or (flatten and changed)          # no tree without new records that differ
        assert not q8 or trees                              # the 8-wide nodes come from the same run of the builder
        assert gather == int(bool(pos or attr))
        if not pos and not attr:
            assert v == "00000"
