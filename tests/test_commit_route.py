"""What follows a device build (lucille_amd/csrc/lh_route.h, read by lh_commit.hip device_upload and lh_accel_recommit) on the CPU: the header,
compiled into the stand-alone program tests/cpu_model/lh_route_check.c with -fsanitize=address,undefined, over every (builder, outcome, flags) cell,
against the table below -- written from what each caller did with the builders' return codes before the header existed, not from the header:

  - a bad vertex is an error for everybody; a re-commit turns every failure into an error (the resident scene stays);
  - device meshes fall back to the host builders on every other failure (the flattened records are copied out);
  - host meshes: a tree too deep goes to the host builders even where the device was asked for; a builder that failed (or made more nodes than a
    32-bit byte offset addresses) only where nobody asked for the device; lucille's own tree failing leaves that tree to the host thread;
  - a danger scan that met a HIP error is an error wherever a failed builder of lucille's own tree would have gone to the host thread;
  - a replica has nothing to fall back to: errors, but for its own tree where the source's came from a host (the host thread's copy is attached);
  - wherever the scene's own tree is a device-built one no host thread can stand in: an error."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_model", "lh_route_check.c")

BUILDERS = ("host meshes", "replica", "device meshes", "re-commit")
OUTCOMES = ("built", "bad vertex", "builder failed", "too deep", "too many nodes", "own tree failed", "danger scan failed")
ROUTES = "IEHT"          # install, error, host builders, lucille's own tree by the host thread
# builder -> outcome -> the route for (build_auto, ref_on_device) = (0, 0), (0, 1), (1, 0), (1, 1)
TABLE = {
    "host meshes":   {"built": "IIII", "bad vertex": "EEEE", "builder failed": "EEHE", "too deep": "HHHH", "too many nodes": "EEHE", "own tree failed": "TETE", "danger scan failed": "EEEE"},
    "replica":       {"built": "IIII", "bad vertex": "EEEE", "builder failed": "EEEE", "too deep": "EEEE", "too many nodes": "EEEE", "own tree failed": "TETE", "danger scan failed": "EEEE"},
    "device meshes": {"built": "IIII", "bad vertex": "EEEE", "builder failed": "HHHH", "too deep": "HHHH", "too many nodes": "HHHH", "own tree failed": "HHHH", "danger scan failed": "HHHH"},
    "re-commit":     {"built": "IIII", "bad vertex": "EEEE", "builder failed": "EEEE", "too deep": "EEEE", "too many nodes": "EEEE", "own tree failed": "EEEE", "danger scan failed": "EEEE"},
}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("route") / "lh_route_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr          # a sanitizer report ends the program with a message
    routes = {}
    for line in r.stdout.splitlines():
        k, v = line.split(" : ")
        routes[tuple(int(x) for x in k.split())] = ROUTES[int(v)]
    return routes


def test_every_cell_against_the_table(lines):
    routes = lines
    assert len(routes) == len(BUILDERS) * len(OUTCOMES) * 4
    for w, who in enumerate(BUILDERS):
        for o, outcome in enumerate(OUTCOMES):
            for f, (auto, rdev) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                assert routes[(w, o, auto, rdev)] == TABLE[who][outcome][f], (who, outcome, auto, rdev)


def test_invariants(lines):
    routes = lines
    for (w, o, auto, rdev), r in routes.items():
        assert (r == "I") == (OUTCOMES[o] == "built")
        if OUTCOMES[o] == "bad vertex" or BUILDERS[w] == "re-commit":
            assert r in "IE"
        if r == "T":          # only lucille's own tree is ever left to the host thread, and only where a host can have one
            assert OUTCOMES[o] == "own tree failed" and not rdev and BUILDERS[w] in ("host meshes", "replica")
        if r == "H":
            assert BUILDERS[w] in ("host meshes", "device meshes")
