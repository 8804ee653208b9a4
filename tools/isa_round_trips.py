#!/usr/bin/env python3
"""What the compiler made of a kernel's "first round trip": the vector-memory loads it issues and the s_waitcnt vmcnt(n) it
places, in program order from the kernel's entry to its first s_barrier, plus the VGPR / scratch / occupancy lines of its
resource report.  Reads text only; runs on a CPU.

    tools/isa_round_trips.py                      # compiles csrc/o3s_icp.hip (the Makefile's flags) into a temporary directory
    tools/isa_round_trips.py o3s_icp.s            # reads device assembly made with `hipcc ... --cuda-device-only -S`
    tools/isa_round_trips.py -k k_solve -k 'k_match2<false,2,2,4,true,true>'
    tools/isa_round_trips.py --kernarg-front      # the front of every launch: what stands between a wave's start and its first loads

The chain kernels are one generation of waves and latency-bound: what a launch costs is its number of DEPENDENT memory round
trips.  A wait is *serial* when it retires at least one outstanding load and another load is issued after it (ahead of the
first barrier): the later load starts a new trip.  Waits that follow one another with no load in between (vmcnt(6), vmcnt(5), ...:
one batch consumed in order) are one serial wait.  trips = serial waits + 1 (the final drain).

When the tool compiles it compiles twice, side by side: once as the library is built and once with -gline-tables-only, from which
every load takes the source line it came from.  A region can then be named by a piece of its source text: `--ignore TEXT` leaves
out the loads whose source line contains TEXT (regions the measured chain never enters), `region_waits()` looks at the loads of
one source line.  Assembly given on the command line is read as it is (source lines if it carries .loc directives).

`--kernarg-front` reads the very first thing a launch does.  Every address comes out of a kernel argument; an
argument is either delivered in SGPRs at wave launch (the leading ones, up to `.amdhsa_user_sgpr_kernarg_preload_length` dwords:
-amdgpu-kernarg-preload-count in HIPFLAGS) or fetched with a scalar load from the kernarg segment, which the first vector load that
needs it has to wait for (`s_waitcnt lgkmcnt`).  Per kernel the report gives the preload length, the kernarg scalar loads that
stand between the end of the compatibility prologue (the copy of the preloaded arguments' loads that firmware without the feature
enters through) and the first vector load, the lgkmcnt wait that load sits behind, if any, and whether a kernarg load is waited for
between loads of the first batch of vector loads (tests/test_isa_kernarg_front.py pins the preload length and the first wait).
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open3d_slam_advanced_rss_2024_public_amd", "csrc")
DEFAULT_KERNELS = ["k_match2<false,2,2,4,true,true>", "k_classify", "k_sel_ne", "k_solve", "k_sel_finish", "k_sel_partial", "k_normal_eq"]
# --kernarg-front: every kernel the chain and the reading's preparation launch (the settle front is the seven-argument overload)
FRONT_KERNELS = ["k_match2<false,4,2,4,true,true,true>", "k_match2<false,2,2,4,true,true>", "k_match2<false,4,2,4,true,false>", "k_classify", "k_sel_ne",
                 "k_solve", "k_sel_partial", "k_sel_finish", "k_normal_eq", "k_read_prep", "k_read_starts", "k_read_scatter", "k_read_place"]
# Regions the converged C2 chain never enters, by a piece of their source line: not counted, each with the branch region around it.
# The one list: tests/test_isa_round_trips.py pins its bounds on the same regions this tool leaves out of its table.
DEFAULT_IGNORE = {
    "k_classify": [
        "? mn[i] :",                    # kModeNormalReady: the matcher wrote the normals (readings from 200 k points)
        "rnx[i]", "rny[i]", "rnz[i]",   # the SurfaceNormalOutlierFilter's reading normals (no gate in the benchmark's chain)
        "hist_rep + (size_t)",          # the level-1 replicas: first iterations and chains without counters (pinned as a batch by the test)
    ],
}

_LOAD = re.compile(r"^(global|buffer|flat|scratch)_load_\w+")
_VMEM_OTHER = re.compile(r"^(global|buffer|flat|scratch)_(store|atomic)_\w+")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")
_LGKMCNT = re.compile(r"lgkmcnt\((\d+)\)")
_SPAIR = re.compile(r"s\[(\d+):(\d+)\]")


def makefile_flags() -> list[str]:
    """HIPFLAGS of csrc/Makefile (ARCH expanded), so the tool reads what the library is built from."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    flags = re.search(r"^HIPFLAGS \?= (.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def hipcc() -> str | None:
    import shutil

    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def compile_asm(out_dir: str, src: str = "o3s_icp.hip", extra: tuple[str, ...] = ()) -> str:
    out = os.path.join(out_dir, os.path.splitext(src)[0] + ".s")
    cmd = [hipcc(), *makefile_flags(), *extra, "--cuda-device-only", "-S", "-o", out, src]
    subprocess.run(cmd, cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out


def mangled_fragment(spec: str) -> str:
    """`k_solve` -> `7k_solveE`, `k_match2<false,2,2,4,true,true>` -> `8k_match2ILb0ELi2E...E` (Itanium: bool and int arguments)."""
    m = re.fullmatch(r"\s*(\w+)\s*(?:<(.*)>)?\s*", spec)
    if not m:
        raise ValueError(f"not a kernel name: {spec!r}")
    name, args = m.group(1), m.group(2)
    frag = f"{len(name)}{name}"
    if args is None:
        return frag + "E"
    frag += "I"
    for a in (x.strip() for x in args.split(",")):
        if a in ("true", "false"):
            frag += f"Lb{1 if a == 'true' else 0}E"
        else:
            v = int(a)
            frag += f"Li{'n' if v < 0 else ''}{abs(v)}E"
    return frag + "E"


class Kernel:
    def __init__(self, symbol: str):
        self.symbol = symbol
        self.ops: list[tuple[str, str, str]] = []  # (kind, text, source line text); kind: load / vmem / wait / barrier / label / branch
        self.resources: list[str] = []
        # the kernarg front: scalar loads, every s_waitcnt, vector loads, barriers and unconditional branches in program order
        # (kind, text); kind: sload / swait / load / barrier / jump / smov64
        self.front_ops: list[tuple[str, str]] = []
        self.hsa: dict[str, int] = {}  # the .amdhsa_user_sgpr_* lines of the kernel descriptor


def parse(asm_path: str, src_dir: str = CSRC) -> dict[str, Kernel]:
    """Every function of the assembly: its vector-memory instructions, vmcnt waits and barriers in program order.  `src_dir`: where
    the relative paths of the .file directives start (the directory the assembly was compiled in)."""
    files: dict[int, str] = {}
    src_cache: dict[str, list[str]] = {}

    def src_text(fileno: int, line: int) -> str:
        path = files.get(fileno)
        if not path:
            return ""
        if path not in src_cache:
            cand = path if os.path.isabs(path) else os.path.join(src_dir, path)
            try:
                src_cache[path] = open(cand, errors="replace").read().splitlines()
            except OSError:
                src_cache[path] = []
        ls = src_cache[path]
        return f"{os.path.basename(path)}:{line}: {ls[line - 1].strip()}" if 0 < line <= len(ls) else f"{os.path.basename(path)}:{line}"

    kernels: dict[str, Kernel] = {}
    cur: Kernel | None = None
    last: Kernel | None = None
    loc = ""
    pending_type: set[str] = set()
    hsa_of: Kernel | None = None
    for raw in open(asm_path, errors="replace"):
        s = raw.strip()
        if not s:
            continue
        if s.startswith(".file"):
            m = re.match(r'\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', s)
            if m:
                files[int(m.group(1))] = os.path.join(m.group(2), m.group(3)) if m.group(3) else m.group(2)
            continue
        if s.startswith(".amdhsa_kernel "):
            hsa_of = kernels.get(s.split()[1])
            continue
        if s.startswith(".amdhsa_user_sgpr_") and hsa_of is not None:
            key, val = s.split()[:2]
            if val.isdigit():
                hsa_of.hsa[key[len(".amdhsa_user_sgpr_"):]] = int(val)
            continue
        if s.startswith(".type") and s.endswith(",@function"):
            pending_type.add(s.split()[1].split(",")[0])
            continue
        if s.startswith(".loc"):
            p = s.split()
            loc = src_text(int(p[1]), int(p[2]))
            continue
        if cur is None:
            m = re.match(r"^([\w.$]+):", s)
            if m and m.group(1) in pending_type:
                cur = Kernel(m.group(1))
                kernels[cur.symbol] = cur
                loc = ""
            elif last is not None and s.startswith(";"):
                m = re.match(r";\s*(NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|LDSByteSize|NumSgprs):\s*(\S+)", s)
                if m:
                    last.resources.append(f"{m.group(1)}: {m.group(2)}")
            continue
        if s.startswith(".Lfunc_end"):
            last, cur = cur, None
            continue
        if s.startswith(".LBB") and s.split(";")[0].strip().endswith(":"):  # basic-block labels (not the line tables' .Ltmp)
            cur.ops.append(("label", s.split(":")[0], ""))
            continue
        if s[0] in ".;" or s.endswith(":"):
            continue
        ins = s.split(";")[0].strip()
        mnem = ins.split()[0] if ins else ""
        if mnem.startswith("s_load_"):
            cur.front_ops.append(("sload", ins))
        elif mnem == "s_waitcnt":
            cur.front_ops.append(("swait", ins))
        elif mnem == "s_branch":
            cur.front_ops.append(("jump", ins))
        elif mnem == "s_mov_b64":
            cur.front_ops.append(("smov64", ins))
        elif _LOAD.match(mnem):
            cur.front_ops.append(("load", ins))
        elif mnem == "s_barrier":
            cur.front_ops.append(("barrier", ins))
        if mnem.startswith("s_cbranch_"):
            cur.ops.append(("branch", ins, ""))
        elif _LOAD.match(mnem):
            cur.ops.append(("load", ins, loc))
        elif _VMEM_OTHER.match(mnem):
            cur.ops.append(("vmem", ins, loc))
        elif mnem == "s_waitcnt" and _VMCNT.search(ins):
            cur.ops.append(("wait", ins, loc))
        elif mnem == "s_barrier":
            cur.ops.append(("barrier", ins, loc))
    return kernels


def find(kernels: dict[str, Kernel], spec: str) -> Kernel:
    frag = mangled_fragment(spec)
    hits = [k for s, k in kernels.items() if frag in s]
    if len(hits) != 1:
        raise KeyError(f"{spec}: {len(hits)} kernels carry {frag}")
    return hits[0]


def first_trip(k: Kernel, ignore: list[str] | tuple[str, ...] = (), barriers: int = 0):
    """Entry to the first s_barrier (`barriers` > 0: on through that many of them).  Returns (events, serial_waits, loads): events
    are printable lines; a serial wait retires at least one outstanding load and has another load behind it."""
    # an ignored load takes the forward-branch region around it along (its waits belong to a path that is not taken)
    label_at = {ins: j for j, (kind, ins, _) in enumerate(k.ops) if kind == "label"}
    dropped = [False] * len(k.ops)
    named = [kind == "load" and any(t in loc for t in ignore) for kind, _, loc in k.ops]
    for j in (j for j, hit in enumerate(named) if hit and not dropped[j]):
        dropped[j] = True
        for b in range(j - 1, -1, -1):
            if k.ops[b][0] == "branch" and label_at.get(k.ops[b][1].split()[-1], -1) > j:
                for x in range(b + 1, label_at[k.ops[b][1].split()[-1]]):
                    dropped[x] = True
                break
    ops, skipped = [], []
    for j, (kind, ins, loc) in enumerate(k.ops):
        if kind in ("label", "branch") or (dropped[j] and not named[j]):
            continue
        if kind == "barrier":
            if barriers <= 0:
                break
            barriers -= 1
        ops.append((kind, ins, loc))
        skipped.append(named[j])
    last_load = max((j for j, (kind, _, _) in enumerate(ops) if kind == "load" and not skipped[j]), default=-1)
    inflight: list[str] = []  # oldest first; "load" or "vmem" (stores and atomics share the counter)
    events, serial, loads = [], 0, 0
    waited = False  # a wait has retired a load since the last load was issued: the next load opens a new trip
    for j, (kind, ins, loc) in enumerate(ops):
        if kind == "load":
            if skipped[j]:
                events.append(f"      (ignored)  {ins}   ; {loc}")
                continue
            serial += waited
            waited = False
            inflight.append("load")
            loads += 1
            events.append(f"      {ins}   ; {loc}")
        elif kind == "vmem":
            inflight.append("vmem")
        elif kind == "barrier":
            events.append(f"  ------ {ins}   ; {len([x for x in inflight if x == 'load'])} load(s) in flight")
        else:
            n = int(_VMCNT.search(ins).group(1))
            retired = 0
            while len(inflight) > n:
                retired += inflight.pop(0) == "load"
            if retired:
                is_serial = j < last_load
                waited = True
                events.append(f"  {'SERIAL' if is_serial else 'drain '} {ins}   ; retires {retired} load(s)")
    return events, serial, loads


def region_waits(k: Kernel, text: str, batch: int):
    """The loads whose source line contains `text`, in program order over the WHOLE kernel, in groups of `batch` (one group per
    inlined copy of an unrolled loop).  Returns [(loads in the group, waits that retire one of the group's loads before its last load
    is issued)]: (batch, 0) is a group that travels as one batch."""
    groups: list[list[int]] = []  # [loads, splitting waits]
    inflight: list[int | None] = []  # oldest first: the group of a region load, None for any other vector-memory operation
    for kind, ins, loc in k.ops:
        if kind in ("label", "branch"):
            continue
        if kind == "load" and text in loc:
            if not groups or groups[-1][0] == batch:
                groups.append([0, 0])
            groups[-1][0] += 1
            inflight.append(len(groups) - 1)
        elif kind in ("load", "vmem"):
            inflight.append(None)
        elif kind == "wait":
            n = int(_VMCNT.search(ins).group(1))
            split = set()
            while len(inflight) > n:
                g = inflight.pop(0)
                if g is not None and groups[g][0] < batch:
                    split.add(g)
            for g in split:
                groups[g][1] += 1
    return [tuple(g) for g in groups]


def kernarg_front(k: Kernel) -> dict:
    """The front of a launch: what stands between a wave's start and its first batch of vector loads.
      preload        dwords of arguments delivered in SGPRs at wave launch
      sloads         the kernarg scalar loads between the end of the compatibility prologue and the first vector load
      first_wait     the lgkmcnt wait, with a kernarg load outstanding, that the first vector load sits behind (None: it goes out at once)
      batch_wait     the first such wait with another vector load of the first batch behind it, in program order, branches not followed
                     (None: the whole batch goes out without waiting for an argument; a wait behind the batch's last load overlaps
                     with the loads in flight); the batch ends at the first vmcnt wait that retires one of its loads, or a barrier
      batch_loads    vector loads of that first batch"""
    preload = k.hsa.get("kernarg_preload_length", 0)
    # the kernarg pointer's SGPR pair: the user SGPRs in front of it are the private segment buffer (4), the dispatch and queue pointers (2 each)
    base = 4 * k.hsa.get("private_segment_buffer", 0) + 2 * k.hsa.get("dispatch_ptr", 0) + 2 * k.hsa.get("queue_ptr", 0)
    karg = {(base, base + 1)}
    ops = k.front_ops
    if preload:  # the prologue ends with the jump over the padding to the entry that hardware with the feature starts at
        j = next((j for j, (kind, _) in enumerate(ops) if kind == "jump"), -1)
        ops = ops[j + 1:]
    out = {"preload": preload, "sloads": [], "first_wait": None, "batch_wait": None, "batch_loads": 0}
    pending = 0    # kernarg scalar loads not waited for yet
    inflight = 0   # vector loads in flight
    held = None    # a kernarg wait seen inside the batch: it counts once another load of the batch follows it
    for kind, ins in ops:
        if kind == "smov64":
            pairs = _SPAIR.findall(ins)
            if len(pairs) == 2 and (int(pairs[1][0]), int(pairs[1][1])) in karg:
                karg.add((int(pairs[0][0]), int(pairs[0][1])))
        elif kind == "sload":
            pairs = _SPAIR.findall(ins.split(",", 1)[1]) if "," in ins else []
            if pairs and (int(pairs[0][0]), int(pairs[0][1])) in karg:
                pending += 1
                if out["batch_loads"] == 0:
                    out["sloads"].append(ins)
        elif kind == "swait":
            m = _LGKMCNT.search(ins)
            if m and pending:  # scalar loads return out of order: any lgkmcnt wait with one outstanding waits for it
                if out["batch_loads"] == 0 and out["first_wait"] is None:
                    out["first_wait"] = ins
                if out["batch_wait"] is None and held is None:
                    held = ins
                pending = 0
            v = _VMCNT.search(ins)
            if v and int(v.group(1)) < inflight:
                break
        elif kind == "load":
            inflight += 1
            out["batch_loads"] += 1
            if held is not None and out["batch_wait"] is None:
                out["batch_wait"] = held
        elif kind == "barrier":
            break
    return out


def report_kernarg_front(kernels: dict[str, Kernel], specs: list[str], out=sys.stdout) -> dict[str, dict]:
    res = {}
    for spec in specs:
        k = find(kernels, spec)
        f = res[spec] = kernarg_front(k)
        print(f"== {spec}: preload length {f['preload']} dwords, first batch of {f['batch_loads']} vector load(s)", file=out)
        print(f"   kernarg scalar loads ahead of the first vector load: {len(f['sloads'])}", file=out)
        for ins in f["sloads"]:
            print(f"      {ins}", file=out)
        print(f"   the first vector load sits behind: {f['first_wait'] or 'no kernarg wait'}", file=out)
        print(f"   a kernarg load is waited for between loads of the first batch: {f['batch_wait'] or 'no'}", file=out)
    return res


def compile_both(out_dir: str, src: str = "o3s_icp.hip") -> dict[str, Kernel]:
    """Two compiles side by side: the Makefile's flags (the instructions and the resource report of the library) and the same with
    -gline-tables-only (the source line of every instruction; it makes a non-inlined callee save one more register, which shows in the
    resource report of its callers).  A kernel whose loads, waits and barriers are the same in both takes the source lines."""
    import concurrent.futures as cf

    os.makedirs(os.path.join(out_dir, "lines"), exist_ok=True)
    with cf.ThreadPoolExecutor(2) as ex:
        plain = ex.submit(compile_asm, out_dir, src, ())
        lines = ex.submit(compile_asm, os.path.join(out_dir, "lines"), src, ("-gline-tables-only",))
        kp, kl = parse(plain.result()), parse(lines.result())
    for sym, k in kp.items():
        other = kl.get(sym)
        if other is not None and [(a, b) for a, b, _ in k.ops] == [(a, b) for a, b, _ in other.ops]:
            k.ops = other.ops
        else:
            k.resources.append("(no source lines: the line-table build differs)")
    return kp


def report(kernels: dict[str, Kernel], specs: list[str], ignore: dict[str, list[str]], out=sys.stdout, barriers: int = 0) -> dict[str, int]:
    trips = {}
    for spec in specs:
        k = find(kernels, spec)
        base = spec.split("<")[0]
        events, serial, loads = first_trip(k, ignore.get(base, ()), barriers)
        trips[spec] = serial + (1 if loads else 0)
        print(f"== {spec}: {loads} loads, {serial} serial wait(s), {trips[spec]} round trip(s) ahead of {'the first barrier' if barriers == 0 else f'barrier {barriers + 1}'}", file=out)
        print("   " + "  ".join(k.resources), file=out)
        for e in events:
            print(e, file=out)
    return trips


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("asm", nargs="?", help="device assembly (default: compile csrc/o3s_icp.hip)")
    ap.add_argument("-k", "--kernel", action="append", help="kernel name, template arguments as in C++ (repeatable)")
    ap.add_argument("--ignore", action="append", default=[], help="leave out loads whose source line contains this text")
    ap.add_argument("--src-dir", default=CSRC, help="the directory the given assembly was compiled in (for its source lines)")
    ap.add_argument("--barriers", type=int, default=0, help="read on through this many s_barrier (default: stop at the first)")
    ap.add_argument("--kernarg-front", action="store_true", help="report the kernarg front of every chain and reading kernel instead")
    a = ap.parse_args()
    if a.kernarg_front:
        specs = a.kernel or FRONT_KERNELS
        if a.asm:
            report_kernarg_front(parse(a.asm, a.src_dir), specs)
        elif not hipcc():
            print("hipcc not found", file=sys.stderr)
            return 2
        else:
            with tempfile.TemporaryDirectory() as d:
                report_kernarg_front(parse(compile_asm(d)), specs)
        return 0
    specs = a.kernel or DEFAULT_KERNELS
    ignore = {s.split("<")[0]: list(DEFAULT_IGNORE.get(s.split("<")[0], [])) + a.ignore for s in specs}
    if a.asm:
        report(parse(a.asm, a.src_dir), specs, ignore, barriers=a.barriers)
    else:
        if not hipcc():
            print("hipcc not found", file=sys.stderr)
            return 2
        with tempfile.TemporaryDirectory() as d:
            report(compile_both(d), specs, ignore, barriers=a.barriers)
    return 0


if __name__ == "__main__":
    sys.exit(main())
