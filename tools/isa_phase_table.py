"""Per-phase DYNAMIC instruction table of one A wave and one B wave of k_sample8 for one sampling step, from the gfx950 ISA hipcc emits (`make isa`, so the unit's
own flags; cross-compiles without a GPU).  A reporting tool: nothing asserts on it.

How: the product instantiation's text (k_sample8<false, false>, the first in the listing) is cut into a control-flow graph whose nodes end at labels, branches and
WAYPOINTS - every s_barrier and every `; combine_red case W` marker.  A wave's step is the walk from its role loop's header back to that header that passes the
waypoints in the order the source fixes (both roles execute the same barriers: per block three for the out_proj combine and three for the linear2 combine, one more in
front of the four blocks with a skip linear, two in the step's tail; the reducer W = 0 also passes its own case marker at the end of each combine).  Among the walks
that do, the one with the fewest instructions is taken (Dijkstra over (node, next waypoint)); lane-mask branches follow the lanes (s_cbranch_execz falls through,
s_cbranch_execnz is taken), and the walk must run the ancestral-noise draw and the scheduler update once each (MUST_RUN below).  What the shortest walk leaves out: every debugging tap and optional output, and
the extra work in front of a skip block (a B wave's 8 early units, an A wave's u = W[:, 128:] . skip: 8 MFMAs and 4 LDS reads) - listed under the table.
The STEP HEAD (token assembly, wave 4's time-token copy: role loop header -> the `step start` stamp) gets a table of its own, read off the phase-stamped
instantiation, which is the one that marks where the head ends (head_rows).

Usage: python tools/isa_phase_table.py [k_sampler8.s] > profiles/rNN_k_sample8_phase_instructions.txt      (without an argument it runs `make isa` itself)"""
import heapq
import json
import re
import shutil
import subprocess
import sys
import tempfile
from collections import Counter
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "amuse_amd" / "csrc"
CLASSES = ("VALU", "MFMA", "LDS", "VMEM", "s_nop", "s_waitcnt", "SALU")
BLOCKS, SKIP_BLOCKS = 9, 4
# blocks of the step that sit behind wave-uniform branches the shortest walk would take the short side of: the ancestral-noise draw (Box-Muller's v_log_f32)
# and the scheduler update (the clamp's v_min_f32) - each is run once per step
MUST_RUN = ("v_log_f32", "v_min_f32")


def classify(ins: str) -> str:
    op = ins.split()[0]
    if op.startswith("v_mfma"):
        return "MFMA"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "VMEM"
    if op in ("s_nop", "s_waitcnt"):
        return op
    return "SALU"     # scalar ALU, scalar loads, branches, s_barrier


def kernel_text(asm: str):
    """Lines of the first k_sample8 instantiation (label line .. s_endpgm)."""
    lines = asm.splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*k_sample8\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip() == "s_endpgm")
    return lines[start:end + 1], lines[start].split(":")[0]


def build_cfg(lines):
    """nodes: [{"label", "ins": [...], "way": None | "B" | "c<W>", "succ": [...]}]; label -> node index."""
    nodes, labels = [], {}
    cur = {"label": None, "ins": [], "way": None, "term": None}

    def close():
        nonlocal cur
        nodes.append(cur)
        cur = {"label": None, "ins": [], "way": None, "term": None}

    for raw in lines:
        l = raw.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            if cur["ins"] or cur["label"]:
                close()
            cur["label"] = m.group(1)
            labels[m.group(1)] = len(nodes)
            continue
        m = re.match(r"^; combine_red case (\d)", l)
        if m:
            if cur["ins"] or cur["label"]:
                close()
            cur["way"] = "c" + m.group(1)
            close()
            continue
        if not l or l[0] in ".;" or l.endswith(":"):
            continue
        ins = l.split(";")[0].strip()
        if not ins:
            continue
        op = ins.split()[0]
        if op == "s_barrier":
            if cur["ins"] or cur["label"]:
                close()
            cur["ins"], cur["way"] = [ins], "B"
            close()
            continue
        cur["ins"].append(ins)
        if op.startswith(("s_cbranch", "s_branch")) or op == "s_endpgm":
            cur["term"] = ins
            close()
    if cur["ins"] or cur["label"]:
        close()
    # a label that opened a node which was closed at once by a waypoint: labels[] points at the first node of the run, which is what a branch wants
    for i, n in enumerate(nodes):
        t = n["term"]
        nxt = [i + 1] if i + 1 < len(nodes) else []
        if t is None:
            n["succ"] = nxt
        else:
            op, *arg = t.split()
            tgt = [labels[arg[0]]] if arg and arg[0] in labels else []
            if op == "s_endpgm":
                n["succ"] = []
            elif op == "s_branch" or op == "s_cbranch_execnz":
                n["succ"] = tgt
            elif op == "s_cbranch_execz":
                n["succ"] = nxt
            else:
                n["succ"] = tgt + nxt
        n["cost"] = Counter(classify(x) for x in n["ins"])
        n["n"] = len(n["ins"])
    return nodes, labels


def role_headers(lines, labels):
    """Depth-1 loop headers whose loop (the text up to the next such header) holds MFMAs: the role loops.  B = the one with the combine_red markers."""
    heads = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):.*Loop Header: Depth=1", l)] if m]
    out = {}
    for n, (i, lab) in enumerate(heads):
        text = "\n".join(lines[i:heads[n + 1][0] if n + 1 < len(heads) else len(lines)])
        if "v_mfma" in text:
            out["B" if "combine_red case" in text else "A"] = lab
    return out


def step_waypoints(role):
    per_block = ["B", "B", "B"] + (["c0"] if role == "B" else [])
    seq = []
    for blk in range(BLOCKS):
        if blk >= BLOCKS - SKIP_BLOCKS:
            seq.append("B")
        seq += per_block + per_block
    return seq + ["B", "B"]


def walk(nodes, start, seq):
    """Fewest-instruction walk start -> start through the waypoints in order that also runs every MUST_RUN block it can reach, once.
    Returns the per-interval cost vectors (len(seq) + 1 of them)."""
    seen, todo = {start}, [start]
    while todo:
        for v in nodes[todo.pop()]["succ"]:
            if v not in seen:
                seen.add(v)
                todo.append(v)
    noise = {u: 1 << b for b, u in enumerate(sorted(u for u in seen if any(x.startswith(MUST_RUN) for x in nodes[u]["ins"])))}
    full = (1 << len(noise)) - 1
    goal = (start, len(seq), full)
    dist, prev = {(start, 0, 0): 0}, {}
    pq = [(0, start, 0, 0)]
    while pq:
        d, u, k, msk = heapq.heappop(pq)
        if (u, k, msk) == goal:
            break
        if d > dist.get((u, k, msk), 1 << 60):
            continue
        n = nodes[u]
        k2, m2 = k, msk
        if n["way"]:
            if k < len(seq) and n["way"] == seq[k]:
                k2 = k + 1
            else:
                continue    # a waypoint out of order: not this wave's walk
        if u in noise:
            if msk & noise[u]:
                continue
            m2 = msk | noise[u]
        for v in n["succ"]:
            if v == start and (k2, m2) != (len(seq), full):
                continue
            nd = d + n["n"]
            if nd < dist.get((v, k2, m2), 1 << 60):
                dist[(v, k2, m2)] = nd
                prev[(v, k2, m2)] = (u, k, msk)
                heapq.heappush(pq, (nd, v, k2, m2))
    if goal not in prev:
        raise SystemExit("no walk through the waypoints - has the barrier sequence of the step changed?")
    path, s = [], goal
    while s in prev:
        s = prev[s]
        path.append(s)
    path.reverse()
    iv = [Counter() for _ in range(len(seq) + 1)]
    for u, k, _ in path:
        iv[k] += nodes[u]["cost"]     # a waypoint node (the barrier itself) is booked to the interval it ends
    return iv


B_PHASES = ["wait for attention: early units, combine parameters -> barrier", "out_proj combine: sum, residual, row statistics -> barrier",
            "out_proj combine: merge, normalise, publish -> barrier", "out_proj combine: gather", "FFN half + linear2 partials, parameters -> barrier",
            "linear2 combine: sum, residual, row statistics -> barrier", "linear2 combine: merge, normalise, publish -> barrier", "linear2 combine: gather"]
A_PHASES = ["in_proj, attention, out_proj partial, publish -> barrier", "out_proj combine: fetch N1 -> barrier", "out_proj combine: fetch N2 -> barrier",
            "gather, fetch, FFN half, publish, fetch N0 -> barrier", "linear2 combine: fetch N1 -> barrier", "linear2 combine: fetch N2 -> barrier"]


def fold(role, iv):
    """Intervals of the step -> rows name: (count vector of a typical occurrence - the median one by size -, sum over the step, occurrences)."""
    per = 8 if role == "B" else 6
    names = B_PHASES if role == "B" else A_PHASES
    occ = {n: [] for n in ["skip linear -> barrier"] + names + ["final LayerNorm statistics -> barrier", "scheduler update (tail) -> step barrier"]}
    i = 0
    for blk in range(BLOCKS):
        if blk >= BLOCKS - SKIP_BLOCKS:
            occ["skip linear -> barrier"].append(iv[i])
            i += 1
        for p in range(per):     # (what follows a block's last waypoint runs into the next block's first interval; block 0's first holds the step head)
            occ[names[p]].append(iv[i])
            i += 1
    occ["final LayerNorm statistics -> barrier"].append(iv[i])
    occ["scheduler update (tail) -> step barrier"].append(iv[i + 1] + iv[i + 2])     # (+ the loop's latch behind the step barrier)
    assert i + 2 == len(iv) - 1
    return {n: (sorted(v, key=lambda c: sum(c.values()))[len(v) // 2], sum(v, Counter()), len(v)) for n, v in occ.items()}


def head_rows(asm: str):
    """The step head - token assembly and wave 4's time-token copy - of both roles: role -> count vector of the text between the role loop's header and
    the `step start` stamp.  The product instantiation carries no stamp, so this reads the phase-stamped one (k_sample8<true, false>): the head is
    its text up to the third s_memtime behind the header (two stamps at the step's top, the third behind the head).  A count of the TEXT, lane-mask
    regions included (some lane runs each of them), which is what a wave issues as long as the head is laid out in one piece - it is straight-line code."""
    lines = asm.splitlines()
    start = next((i for i, l in enumerate(lines) if re.match(r"^_Z\w*k_sample8\w?ILb1ELb0E\w*:", l)), None)
    if start is None:
        return {}
    end = next(i for i in range(start, len(lines)) if lines[i].strip() == "s_endpgm")
    lines = lines[start:end + 1]
    out = {}
    for role, lab in role_headers(lines, None).items():
        i = next(k for k, l in enumerate(lines) if l.startswith(lab + ":"))
        c, stamps = Counter(), 0
        for l in lines[i + 1:]:
            l = l.strip()
            if not l or l[0] in ".;" or l.endswith(":"):
                continue
            ins = l.split(";")[0].strip()
            if not ins:
                continue
            if ins.startswith("s_memtime"):
                stamps += 1
                if stamps == 3:
                    break
            c[classify(ins)] += 1
            c["flat"] += ins.startswith("flat_load")
            c["vmcnt"] += ins.startswith("s_waitcnt") and "vmcnt" in ins
        out[role] = c
    return out


def report(asm_path: Path, out=sys.stdout):
    lines, sym = kernel_text(asm_path.read_text())
    nodes, labels = build_cfg(lines)
    heads = role_headers(lines, labels)
    kid = json.loads(subprocess.run([sys.executable, str(REPO / "tools" / "kernel_id.py"), "k_sample8"], capture_output=True, text=True).stdout or "{}").get("k_sample8", {})
    print(f"# k_sample8 per-phase dynamic instruction counts, one wave, one step ({BLOCKS} blocks, {SKIP_BLOCKS} with a skip linear) - tools/isa_phase_table.py", file=out)
    print(f"# kernel {sym}\n# source_sha256 {kid.get('source_sha256')}\n# object_sha256 {kid.get('object_sha256')}", file=out)
    totals = {}
    for role in ("B", "A"):
        iv = walk(nodes, labels[heads[role]], step_waypoints(role))
        rows = fold(role, iv)
        print(f"\n## {role} wave ({'reducer W = 0, wave 4' if role == 'B' else 'wave 0'}); role loop {heads[role]}", file=out)
        print(f"{'phase':68s} {'x':>3s} " + " ".join(f"{c:>9s}" for c in CLASSES) + "   | per step: " + " ".join(f"{c:>6s}" for c in CLASSES[:4]), file=out)
        tot = Counter()
        for name, (one, allc, n) in rows.items():
            tot += allc
            print(f"{name:68s} {n:3d} " + " ".join(f"{one[c]:9d}" for c in CLASSES) + "   |           " + " ".join(f"{allc[c]:6d}" for c in CLASSES[:4]), file=out)
        print(f"{'TOTAL per step':68s}     " + " ".join(f"{tot[c]:9d}" for c in CLASSES), file=out)
        totals[role] = tot
    hd = head_rows(asm_path.read_text())
    if hd:
        print("\n## step head: role loop header -> `step start` stamp, text of the phase-stamped instantiation k_sample8<true, false> (its three stamps included)", file=out)
        print(f"{'role':68s}     " + " ".join(f"{c:>9s}" for c in CLASSES) + "   | flat_load  waits on vmcnt", file=out)
        for role in ("B", "A"):
            c = hd[role]
            print(f"{role + ' wave':68s}     " + " ".join(f"{c[k]:9d}" for k in CLASSES) + f"   | {c['flat']:9d}  {c['vmcnt']:14d}", file=out)
    avg = (totals["A"]["VALU"] + totals["B"]["VALU"]) / 2
    print(f"\nVALU per wave and step, mean of the two roles: {avg:.0f}   (B {totals['B']['VALU']}, A {totals['A']['VALU']})", file=out)
    print(f"MFMA per step: A {totals['A']['MFMA']}, B {totals['B']['MFMA']}", file=out)
    print("(x: occurrences per step; left columns: a typical occurrence, the median one by size; right columns: the sum over the step.  The first phase of block 0 holds the\n"
          " step head - the gather of the step's operands -, the first phase of every later block the few instructions behind the previous block's last waypoint, and one of the nine\n"
          " the reducers' noise draw where the kernel makes it ahead of the tail.  Left out by the shortest walk: taps and optional outputs, and in front of each of the\n"
          " four skip blocks a B wave's 8 early units and an A wave's u = W[:, 128:] . skip - 8 MFMAs, 4 LDS reads, 2 LDS writes -, and in the tail a B wave's assembly of the\n next step's two tiles (behind `step + 1 < T`: 2 LDS reads, the adds and selects of two tiles, the pack, 1 LDS write).  SQ_INSTS_VALU counts MFMAs as VALU.)", file=out)
    return totals


if __name__ == "__main__":
    if len(sys.argv) > 1:
        report(Path(sys.argv[1]))
    else:
        d = Path(tempfile.mkdtemp(prefix="amuse_isa_"))
        made = subprocess.run(["make", "-s", "-C", str(CSRC), "isa", f"OUT={d}", f"ISA={d}/k_sampler8.s"], capture_output=True, text=True)
        if made.returncode:
            sys.exit(made.stderr[-2000:])
        report(d / "k_sampler8.s")
        shutil.rmtree(d, ignore_errors=True)
