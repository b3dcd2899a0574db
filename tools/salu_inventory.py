#!/usr/bin/env python3
"""Scalar-unit inventory of one trace kernel: its scalar instructions per phase of a round and per loop,
from the kernel's ISA compiled with line tables, weighted by trip counts.

    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> --cuda-device-only -S -gline-tables-only \
        viennaray_amd/csrc/vr_trace.hip -o k.s
    tools/salu_inventory.py k.s [mangled kernel name]

(vr_trace.hip holds the generators of vr_generate.hpp and the trace kernels of vr_trace_kernel.hpp; the other .hip files
— its header has the map — hold none of them.  The trace kernels are in vr_trace.hip's assembly.)

(The tool prints the kernel's instruction count: compare it with tools/spill_by_depth.py on the plain build — line
tables can move a kernel's register allocation, and an inventory of other code than the library's is worthless.)

What is counted as SALU: every s_* instruction but scalar memory loads (SQ_INSTS_SMEM), branches
(SQ_INSTS_BRANCH) and s_waitcnt / s_nop / s_barrier / s_endpgm / s_sleep / s_setprio, which never reach the scalar ALU.
A phase is a range of source lines (the innermost inlined location of each instruction), found at run time: in
vr_trace_kernel.hpp it runs from one marker comment of the kernel body (MARKERS) to the next; a loop is named by
its header's label.  Weights (WEIGHTS below): executions per packet round of each loop's body, from the committed
profile of the headline launch (profiles/r04_C2_s1.0_summary.txt)."""
import re
import sys

DEFAULT = "_ZN2vr12trace_kernelILi3ELi0ELi0ELi1EEEvNS_11TraceParamsE"

# phases of the kernel body in vr_trace_kernel.hpp: each begins at the line of its marker comment and ends before the next
# marker's; what lies before the first marker belongs to the prologue.  Every marker must be there exactly once, in this order.
MARKERS = [
    ("// ---- wave-wide compaction / restart", "refill bin walk"),
    ("// ---- queue pull", "queue pull"),
    ("// ---- (end of the queue pull", "refill bin walk"),
    ("// ---- round set-up", "round set-up / votes"),
    ("// ---- walls first", "walls"),
    ("// ---- packet query", "packet query (call, back-off)"),
    ("// ---- fall-back", "fall-back packet / walk"),
    ("// ---- walls of the finished segments", "walls"),
    ("// ---- the aggregation vote", "state machine"),
    ("// ---- crediting", "crediting"),
    ("// ---- end of crediting", "prologue / epilogue"),
]


def kernel_phases(path):
    """[(phase, first line, last line)] of vr_trace_kernel.hpp, from MARKERS"""
    src = open(path).read().split("\n")
    at = []
    for text, _ in MARKERS:
        hits = [i for i, l in enumerate(src, 1) if l.strip().startswith(text)]
        if len(hits) != 1 or (at and hits[0] <= at[-1]):
            sys.exit(f"{path}: the marker comment '{text}' must be there exactly once, behind the marker before it "
                     f"(found at lines {hits}): the kernel body has changed, bring MARKERS and its comments back in line")
        at.append(hits[0])
    out = [("prologue / epilogue", 0, at[0] - 1)]
    for k, (_, phase) in enumerate(MARKERS):
        out.append((phase, at[k], at[k + 1] - 1 if k + 1 < len(at) else 10 ** 9))
    return out


# the role headers behind vr_device.hpp (its map says which holds what) whose functions can be a phase
DEVICE_HEADERS = ("vr_math.hpp", "vr_rng.hpp", "vr_intersect.hpp", "vr_walk.hpp", "vr_packet_query.hpp")
# functions of those headers that ARE a phase; every other function there (edot, hit_disc, ballot64, ...) and every
# system header is a helper inlined into its caller: its instructions stay with the phase seen last
DEVICE_FUNCS = {
    "pq_hit_packet": None,  # split: box + descent / candidate loop
    "hit_walls_from": "walls", "hit_walls_lds": "walls", "hit_walls": "walls", "wall_reachable": "walls", "hit_tri": "walls: exact test",
    "relief_clip": "packet query: box + descent", "wave_minmax6": "packet query: box + descent",
    "bvh_hit_packet": "fall-back packet / walk", "bvh_walk_lanes": "fall-back packet / walk",
    "pair_walk_lanes": "fall-back packet / walk", "process_boundary_hit": "state machine",
}
# executions of a loop body per packet round, by phase and loop depth (depth 1 is the round itself).  From the
# committed profile of the headline launch: 8.7 candidates per packet, 2 - 3 bins per refill (each bin is one pass that
# changes the bin and one that takes its rays: half of the loop body each), a span of 32 bins per queue pull, one or
# two leaf nodes per query; the descent proper runs only where the frontier cache misses and the fall-back packet /
# walk only where the query gives up (both a few per cent of the rounds: weighted 0.05).
WEIGHTS = {
    "refill bin walk": {1: 1.0, 2: 2.5},
    "queue pull": {1: 2.5 / 32, 2: 2.5 / 32, 3: 2.5 / 32},
    "round set-up / votes": {1: 1.0},
    "walls": {1: 1.0},
    # (behind the conservative pre-tests: only the rounds with a ray next to a side wall — 0.3 % of the headline's
    #  segments meet a wall, all of them in the bins along the edge: about 3 % of the rounds)
    "walls: exact test": {1: 0.03},
    "packet query (call, back-off)": {1: 1.0},
    "packet query: box + descent": {1: 1.0, 2: 0.05, 3: 0.05 * 3},
    "candidate loop": {1: 1.0, 2: 1.5, 3: 8.7},
    "state machine": {1: 1.0, 2: 0.05, 3: 0.05},
    "crediting": {1: 1.0, 2: 8.7},
    "fall-back packet / walk": {1: 0.05, 2: 0.05 * 4, 3: 0.05 * 16},
    "prologue / epilogue": {0: 0.0, 1: 0.0, 2: 0.0, 3: 0.0},
}

NOT_SALU = ("s_load", "s_buffer_load", "s_waitcnt", "s_nop", "s_barrier", "s_endpgm", "s_sleep", "s_setprio",
            "s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_getpc", "s_code_end", "s_inst_prefetch", "s_clause")


def device_ranges(path):
    """[(first line, last line, function name)] of the __device__ functions of one header"""
    out, name, start = [], None, 0
    for i, l in enumerate(open(path), 1):
        m = re.match(r'(?:template[^\n]*>\s*)?__device__\s+(?:__forceinline__\s+)?[\w:<> \*&]+?\b(\w+)\(', l)
        if m:
            if name:
                out.append((start, i - 1, name))
            name, start = m.group(1), i
    if name:
        out.append((start, 10 ** 9, name))
    return out


def main():
    args = sys.argv[1:]
    txt = open(args[0]).read().split("\n")
    kern = args[1] if len(args) > 1 else DEFAULT
    import os
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(here, "viennaray_amd", "csrc")
    dev = {h: device_ranges(os.path.join(csrc, h)) for h in DEVICE_HEADERS}
    phases = kernel_phases(os.path.join(here, "viennaray_amd", "csrc", "vr_trace_kernel.hpp"))
    src = open(os.path.join(csrc, "vr_packet_query.hpp")).read().split("\n")
    # the candidate loop of pq_hit_packet starts at its "unsigned tests = 0;"
    pq = [r for r in dev["vr_packet_query.hpp"] if r[2] == "pq_hit_packet"][0]
    pq_split = next(i for i in range(pq[0], pq[1]) if "unsigned tests = 0;" in src[i - 1])

    files = {}
    for l in txt:
        m = re.match(r'\s*\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]*)"', l)
        if m:
            files[int(m.group(1))] = m.group(2)

    def phase_of(fno, line, last):
        f = files.get(fno, "")
        if f.endswith("vr_trace_kernel.hpp"):
            for name, lo, hi in phases:
                if lo <= line <= hi:
                    return name
        if os.path.basename(f) in dev:
            for lo, hi, fn in dev[os.path.basename(f)]:
                if lo <= line <= hi and fn in DEVICE_FUNCS:
                    if fn == "pq_hit_packet":
                        return "candidate loop" if line >= pq_split else "packet query: box + descent"
                    return DEVICE_FUNCS[fn]
        return last

    on = False
    loop = ("-", 0)      # (header label, depth) of the innermost loop
    loops = {}           # label -> depth
    phase = 'prologue / epilogue'
    rows = {}            # (phase, loop label, depth) -> counters
    total = 0
    cur_label = '-'
    for l in txt:
        if l.startswith(kern + ":"):
            on = True
            continue
        if not on:
            continue
        if l.startswith(".Lfunc_end"):
            break
        m = re.match(r'\s*\.loc\s+(\d+)\s+(\d+)', l)
        if m:
            if int(m.group(2)):  # (line 0: compiler-made glue, stays with the code around it)
                phase = phase_of(int(m.group(1)), int(m.group(2)), phase)
            continue
        if l.startswith(".LBB") or l.startswith("; %bb"):
            cur_label = l.split(":")[0].lstrip(".L; %").replace("bb.", "BB_")
            m = re.search(r'Header=(\w+) Depth=(\d+)', l)
            if m:
                loop = (m.group(1), int(m.group(2)))
            elif "Depth" not in l:
                loop = ("-", 0)
        m = re.search(r'=>\s*This (?:Inner )?Loop Header: Depth=(\d+)', l)
        if m:  # (on the label's own line, or on a comment line under it)
            loop = (cur_label, int(m.group(1)))
            continue
        if l.startswith(".LBB") or l.startswith("; %bb"):
            continue
        s = l.strip()
        if not s or s.startswith((";", ".")) or s.split(" ")[0].endswith(":"):
            continue
        ins = s.split()[0]
        total += 1
        key = (phase, loop[0], loop[1])
        c = rows.setdefault(key, dict(all=0, salu=0, branch=0, smem=0, valu=0, rl=0, wl=0, other=0))
        c["all"] += 1
        if ins.startswith(("s_load", "s_buffer_load")):
            c["smem"] += 1
        elif ins.startswith(("s_branch", "s_cbranch")):
            c["branch"] += 1
        elif ins.startswith("s_") and not ins.startswith(NOT_SALU):
            c["salu"] += 1
        elif ins.startswith("v_readlane") or ins.startswith("v_readfirstlane"):
            c["rl"] += 1
            c["valu"] += 1
        elif ins.startswith("v_writelane"):
            c["wl"] += 1
            c["valu"] += 1
        elif ins.startswith("v_"):
            c["valu"] += 1
        else:
            c["other"] += 1
    print(f"kernel {kern}: {total} instructions")
    print("%-30s %-10s %2s %5s %5s %5s %4s %5s %5s | %6s %8s %8s" % ("phase", "loop", "d", "all", "SALU", "VALU", "br", "rdln",
                                                                 "wrln", "weight", "SALU/rnd", "VALU/rnd"))
    per_phase = {}
    for key in sorted(rows, key=lambda k: (k[0], k[2], k[1])):
        c = rows[key]
        w = WEIGHTS.get(key[0], {}).get(key[2], 0.0)
        pp = per_phase.setdefault(key[0], [0.0, 0.0, 0.0, 0.0])
        pp[0] += w * c["salu"]
        pp[1] += w * c["valu"]
        pp[2] += w * (c["rl"] + c["wl"])
        pp[3] += w * c["branch"]
        print("%-30s %-10s %2d %5d %5d %5d %4d %5d %5d | %6.2f %8.1f %8.1f" % (key[0][:30], key[1], key[2], c["all"], c["salu"],
              c["valu"], c["branch"], c["rl"], c["wl"], w, w * c["salu"], w * c["valu"]))
    print()
    print("per packet round, every instruction of a weighted block counted as executed (an upper bound: blocks behind a")
    print("branch that is not taken are in it):")
    print("%-34s %9s %9s %12s %8s" % ("phase", "SALU", "VALU", "rdln+wrln", "branch"))
    for k, v in sorted(per_phase.items(), key=lambda kv: -kv[1][0]):
        print("%-34s %9.0f %9.0f %12.0f %8.0f" % (k, v[0], v[1], v[2], v[3]))
    tot = [sum(v[i] for v in per_phase.values()) for i in range(4)]
    print("%-34s %9.0f %9.0f %12.0f %8.0f" % ("total", tot[0], tot[1], tot[2], tot[3]))


if __name__ == "__main__":
    main()
