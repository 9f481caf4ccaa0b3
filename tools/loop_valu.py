"""VALU instructions of the persistent walk's loop, per instantiation, from a device listing of lh_kernels.hip -- no GPU needed.
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -S --cuda-device-only lucille_amd/csrc/lh_kernels.hip -o k.s
  python tools/loop_valu.py k.s [other.s]
Per kernel that inlines node_step4 (walks 3 and 8 of k_trace_persist_lane / _indexed / _tmax, k_coop_walk): `step` = the v_* lines of the
node step's blocks (from the block behind the `cur >= 0` branch to the exec restore behind the four stack writes), `loop` = the v_* lines
of every block the listing tags with the loop that holds the step (blocks of loops nested in it -- the fp64 resolve -- excluded), and
the step's memory instructions by kind.  Two listings: side by side, with the differences."""
import re, sys


def kernels(path):
    lines = open(path).read().split("\n")
    out = {}; i = 0
    while i < len(lines):
        m = re.match(r"^(_ZN\S*?(k_trace_persist\w*?|k_coop_walk\w*?)I\S*):", lines[i])
        if m:
            j = i + 1
            while not lines[j].strip().startswith("s_endpgm"): j += 1
            n = re.sub(r"_ZN12_GLOBAL__N_1\d+", "", m.group(1)); n = re.sub(r"E+v12lh_dev.*", "", n)
            n = n.replace("ILb", "<").replace("ELb", ",").replace("ELi", ",").replace("ILi", "<")
            out[n] = lines[i:j + 1]; i = j
        i += 1
    return out


def stats(body):
    try: return stats_(body)
    except (IndexError, StopIteration, AttributeError): return None          # no 4-wide step of that shape in this kernel (walk 7: the 8-wide step)


def stats_(body):
    ab = [n for n, l in enumerate(body) if "v_alignbit_b32" in l]
    first = next((n for n in ab if sum(1 for m in ab if n <= m < n + 100) >= 12), None)
    if first is None: return None
    start = first
    blk = r"^(\.LBB\d+_\d+:|; %bb\.\d+:)"          # the block entered under `cur >= 0`: compare, saveexec, branch, block
    while not (re.match(blk, body[start]) and "s_cbranch_exec" in body[start - 1] and "saveexec" in body[start - 2]
               and any("v_cmp_lt_i32" in l for l in body[start - 6:start - 2])): start -= 1
    w = [n for n in range(first, first + 200) if "ds_write_b32" in body[n]][3]
    end = next(n for n in range(w, w + 40) if body[n].strip().startswith("s_or_b64 exec, exec"))
    hdr = re.search(r"Header=(BB\d+_\d+) Depth=(\d+)", body[start]).groups()
    tag = "Header=%s Depth=%s" % hdr
    step = body[start:end + 1]
    cnt = lambda ls, p: sum(1 for l in ls if l.strip().startswith(p))
    loop = 0; inside = False
    for l in body:
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", l):
            inside = (tag in l) or l.startswith("." + "L" + hdr[0] + ":")
        elif inside and l.strip().startswith("v_"): loop += 1
    return {"step": cnt(step, "v_"), "loop": loop, "flat": cnt(step, "flat_"), "global": cnt(step, "global_"),
            "ds_read_b128": cnt(step, "ds_read_b128"), "ds": cnt(step, "ds_"), "waitcnt": cnt(step, "s_waitcnt")}


if __name__ == "__main__":
    tabs = [{k: stats(b) for k, b in kernels(p).items()} for p in sys.argv[1:3]]
    keys = ["step", "loop", "flat", "global", "ds_read_b128", "ds", "waitcnt"]
    for name in sorted(tabs[0]):
        rows = [t.get(name) for t in tabs]
        if not all(rows): continue
        if len(rows) == 1: print("%-34s" % name, " ".join("%s %d" % (k, rows[0][k]) for k in keys))
        else: print("%-34s" % name, " ".join("%s %d->%d" % (k, rows[0][k], rows[1][k]) for k in keys), " (step %+d, loop %+d)" % (rows[1]["step"] - rows[0]["step"], rows[1]["loop"] - rows[0]["loop"]))
