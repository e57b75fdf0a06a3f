#!/usr/bin/env python3
"""Where do a kernel's software-pipelined loops wait for their own prefetch?  

    python scripts/prefetch_waits.py kernels.s 'k_cl_loop<2,0>' [--name .LBB130_520=forward ... --only-named] [--summary] [--early 0.4]

Reads gfx9 / CDNA assembly as the compiler writes it (hipcc -S --cuda-device-only), finds the loops of one kernel by their back edges (the loop
nest of the control flow graph: strongly connected components, the edges into a component's header taken out to find the loops nested in it)
and, in every loop that issues a group of global loads, follows each group from its issue along the control flow graph until it is issued
again: one trip round the loop.

Vector memory operations (loads and stores alike on this target) return in the order of their issue, and s_waitcnt vmcnt(n) lets at most the n
youngest stay in flight.  So a wait lands a load as soon as n is no larger than the number of vector memory operations issued behind that load,
whatever value the wait was placed for.  Per group the script prints every wait that is the first to land some of its loads: the line, the
count n, how many instructions lie between the group's issue and the wait (shortest path), which part of the trip that is, how many loads
the wait is the first to land, how many operations were issued behind the group by then and how many the wait leaves in flight.  A prefetch
that works shows its first such wait near the end of the trip, in the hand-over of the loaded registers to their user; one that does not
shows it a few instructions behind the issue.  Per loop the headline is the number of prefetch loads landed in the first part of the trip
that issued them (--early, default 0.4): "landed in the stage that issued them".  Where no way from a group back to its next issue is found (the
trip is looked for in the enclosing loops too), the place is printed as `?`: a wait within --gap instructions of the issue still counts as
early, any other is reported as not placed, never as late.  In a loop that works on two stages per trip with two
register sets (ne_backward) half a trip is one stage, and what to read is the n of a set's first wait: the other set's loads that stay in flight.

Paths: the counts are taken over all paths the walk follows, `some path` with the most operations behind the group, `every path` with the
fewest.  Blocks under `if (lane < ...)` are taken as entered by some lane (s_cbranch_execz falls through, a forward s_cbranch_execnz
jumps), so what they issue counts as issued; every other conditional branch is followed both ways.  Calls and indirect branches are not
followed (the kernels have none inside their loops).  Loops are named by the label of their header block; which one is which sweep is read
off the loop line (instructions, MFMAs, loads, stores) and the source.
"""
import argparse
import re
import sys
from collections import namedtuple

CAP = 64            # vmcnt has 6 bits on gfx9: counts saturate here
VM_OP = re.compile(r"^(global|flat|scratch|buffer)_(load|store|atomic)")
VM_LOAD = re.compile(r"^(global|flat|scratch|buffer)_load")
GLOBAL_LOAD = re.compile(r"^global_load")
LABEL = re.compile(r"^([.\w$@]+):")
BRANCH = re.compile(r"^s_(branch|cbranch_\w+)$")

Ins = namedtuple("Ins", "line op args")
Loop = namedtuple("Loop", "head body")                 # index of the header's first instruction; the set of the loop's basic blocks
Group = namedtuple("Group", "first last members")      # instruction indices; members in issue order
Hit = namedtuple("Hit", "idx n dist pmin pmax")      # a wait with a vmcnt field met on the walk


def mangled_fragment(name):
    """'k_qp_solve<17,4,false>' -> '10k_qp_solveILi17ELi4ELb0EE' (integers and bools are all the kernels here take); a name without '<' -> itself."""
    m = re.match(r"^\s*([\w:]+)\s*<(.*)>\s*$", name)
    if not m:
        return name.strip()
    base = m.group(1).split("::")[-1]
    parts = []
    for a in m.group(2).split(","):
        a = a.strip()
        if a in ("true", "false"):
            parts.append("Lb%dE" % (a == "true"))
        elif a.startswith("-"):
            parts.append("Lin%sE" % a[1:])
        else:
            parts.append("Li%sE" % a)
    return "%d%sI%sE" % (len(base), base, "".join(parts))


def vmcnt_of(args):
    """The vmcnt field of an s_waitcnt operand string, None when the wait leaves vmcnt alone."""
    m = re.search(r"vmcnt\((\d+)\)", args)
    if m:
        return int(m.group(1))
    a = args.strip()
    if re.fullmatch(r"(0x[0-9a-fA-F]+|\d+)", a):       # the raw gfx9 immediate: vmcnt = [3:0] | [15:14] << 4
        v = int(a, 0)
        n = (v & 0xF) | (((v >> 14) & 0x3) << 4)
        return None if n == 63 else n
    return None


def parse_kernel(lines, name):
    """Instructions and labels of the kernel whose symbol contains the mangled form of `name`.  Returns (symbol, [Ins], {label: index of the next instruction})."""
    frag = mangled_fragment(name)
    start, sym = None, None
    for i, ln in enumerate(lines):
        m = LABEL.match(ln)
        if m and not m.group(1).startswith(".") and frag in m.group(1):
            if m.group(1) == frag or start is None:
                start, sym = i, m.group(1)
                if m.group(1) == frag:
                    break
    if start is None:
        raise SystemExit("prefetch_waits: no kernel symbol contains %r" % frag)
    ins, labels = [], {}
    for i in range(start + 1, len(lines)):
        ln = lines[i]
        m = LABEL.match(ln)
        if m:
            if m.group(1).startswith(".Lfunc_end"):
                break
            labels[m.group(1)] = len(ins)
            continue
        s = ln.split(";", 1)[0].strip()
        if not s or s.startswith("."):
            continue
        op, _, args = s.partition(" ")
        ins.append(Ins(i + 1, op.strip(), args.strip()))
    return sym, ins, labels


def branch_target(ins, labels):
    if BRANCH.match(ins.op):
        return labels.get(ins.args.split(",")[0].strip())
    return None


class Cfg:
    """Basic blocks of a kernel (leaders: the entry, every label that a branch names, what follows a branch), their successors and predecessors."""

    def __init__(self, ins, labels):
        self.ins = ins
        n = len(ins)
        leaders = {0}
        for i, x in enumerate(ins):
            t = branch_target(x, labels)
            if t is not None and t < n:
                leaders.add(t)
            if (BRANCH.match(x.op) or x.op in ("s_endpgm", "s_setpc_b64", "s_swappc_b64")) and i + 1 < n:
                leaders.add(i + 1)
        self.start = sorted(leaders)
        self.block_of = [0] * n
        for b, s0 in enumerate(self.start):
            for i in range(s0, self.start[b + 1] if b + 1 < len(self.start) else n):
                self.block_of[i] = b
        self.end = [(self.start[b + 1] if b + 1 < len(self.start) else n) - 1 for b in range(len(self.start))]
        self.succ = [[self.block_of[s] for s in successors(ins, labels, e)] for e in self.end]
        # the successors a wave takes that has a lane inside every `if (lane < ...)`: s_cbranch_execz falls through, s_cbranch_execnz jumps.  The
        # walk follows these, so that what such a block issues counts as issued and the distances are those of a wave that does the work.
        self.live_succ = []
        back = [i for i, x in enumerate(ins) if (branch_target(x, labels) if branch_target(x, labels) is not None else n) <= i]
        for b, e in enumerate(self.end):
            ss = self.succ[b]
            t = branch_target(ins[e], labels)
            if ins[e].op == "s_cbranch_execz" and t is not None and t > e + 1 and not any(e < i < t and (branch_target(ins[i], labels) or 0) <= e for i in back):
                ss = [self.block_of[e + 1]]             # (not the exit of a divergent loop: nothing in the skipped part branches back over it)
            elif ins[e].op == "s_cbranch_execnz" and t is not None and t > e:      # (a backward one closes a divergent loop: both ways)
                ss = [self.block_of[t]]
            self.live_succ.append(ss)
        self.pred = [[] for _ in self.start]
        for b, ss in enumerate(self.succ):
            for s in ss:
                self.pred[s].append(b)


def sccs(nodes, succ):
    """Strongly connected components of the subgraph on `nodes` (Tarjan, without recursion); succ(b) yields the successors to follow."""
    index, low, on, st, out = {}, {}, set(), [], []
    for root in sorted(nodes):
        if root in index:
            continue
        index[root] = low[root] = len(index)
        st.append(root)
        on.add(root)
        stack = [(root, iter(succ(root)))]
        while stack:
            b, it = stack[-1]
            nxt = next(it, None)
            if nxt is None:
                stack.pop()
                if stack:
                    low[stack[-1][0]] = min(low[stack[-1][0]], low[b])
                if low[b] == index[b]:
                    comp = set()
                    while True:
                        w = st.pop()
                        on.discard(w)
                        comp.add(w)
                        if w == b:
                            break
                    out.append(comp)
            elif nxt not in nodes:
                continue
            elif nxt not in index:
                index[nxt] = low[nxt] = len(index)
                st.append(nxt)
                on.add(nxt)
                stack.append((nxt, iter(succ(nxt))))
            elif nxt in on:
                low[b] = min(low[b], index[nxt])
    return out


def find_loops(cfg):
    """The loop nest: every cycle of the control flow graph belongs to a strongly connected component; its header is the first block in the layout
    that is entered from outside, its back edges are the edges to the header from inside.  With the back edges taken out, the components that
    remain are the loops nested in it.  A loop with a second entry, which the compiler itself does not list as a loop (a rotated stage loop
    whose hand-over blocks are shared with its prologue), is found like any other: what is left of it when only its header is taken out is still
    one cycle, entered elsewhere, and counts as the same loop and not as one nested in it."""
    loops = []
    todo = [(set(range(len(cfg.start))), frozenset(), None)]
    while todo:
        nodes, cut, parent = todo.pop()
        for comp in sccs(nodes, lambda b: [s for s in cfg.succ[b] if s not in cut]):
            if comp <= cut or (len(comp) == 1 and next(iter(comp)) not in cfg.succ[next(iter(comp))]):
                continue
            entries = [b for b in comp if b == 0 or any(q not in comp for q in cfg.pred[b])]
            h = min(entries or comp)
            if parent is None or len(comp) < parent - 1:
                loops.append(Loop(cfg.start[h], frozenset(comp)))
            if len(comp) > 1:
                todo.append((comp, frozenset([h]), len(comp)))
    loops.sort(key=lambda lp: (lp.head, -len(lp.body)))
    return loops


def innermost(cfg, loops, i):
    best = None
    for lp in loops:
        if cfg.block_of[i] in lp.body and (best is None or len(lp.body) < len(best.body)):
            best = lp
    return best


def loop_instructions(cfg, loop):
    """Instruction indices of the loop's blocks in layout order."""
    return [i for b in sorted(loop.body) for i in range(cfg.start[b], cfg.end[b] + 1)]


def load_groups(cfg, loops, loop, gap):
    """Runs of global loads whose innermost loop is `loop`, consecutive members at most `gap` instructions apart in the layout."""
    groups, cur = [], []
    for i in loop_instructions(cfg, loop):
        if GLOBAL_LOAD.match(cfg.ins[i].op) and innermost(cfg, loops, i) == loop:
            if cur and i - cur[-1] > gap:
                groups.append(Group(cur[0], cur[-1], tuple(cur)))
                cur = []
            cur.append(i)
    if cur:
        groups.append(Group(cur[0], cur[-1], tuple(cur)))
    return groups


def successors(ins, labels, i):
    x = ins[i]
    if x.op in ("s_endpgm", "s_setpc_b64", "s_swappc_b64"):
        return []
    t = branch_target(x, labels)
    if x.op == "s_branch":
        return [] if t is None or t >= len(ins) else [t]
    out = [i + 1] if i + 1 < len(ins) else []
    if t is not None and t < len(ins) and BRANCH.match(x.op):
        out.append(t)
    return out


def walk(cfg, loop, group):
    """Every wait with a vmcnt field that can follow the group's last load inside the loop, up to the point where the group is issued again.
    State per instruction: fewest and most vector memory operations issued behind the group, shortest distance in instructions.  Returns the
    waits and whether the walk was forced out of the loop's body."""
    ins = cfg.ins
    state = {}
    work = []
    forced_out = []

    def push(i, pmin, pmax, dist):
        if i == group.first or cfg.block_of[i] not in loop.body:
            return                                      # the group is issued again, or the path leaves the loop
        old = state.get(i)
        new = (pmin, pmax, dist) if old is None else (min(old[0], pmin), max(old[1], pmax), min(old[2], dist))
        if new != old:
            state[i] = new
            work.append(i)

    def leave(i, pmin, pmax, dist):
        b = cfg.block_of[i]
        if i < cfg.end[b]:
            push(i + 1, pmin, pmax, dist + 1)
            return
        if cfg.live_succ[b] and not any(sb in loop.body for sb in cfg.live_succ[b]):
            forced_out.append(b)                        # no way on inside the body: the cycle is larger than this loop (see analyse_loop)
        for sb in cfg.live_succ[b]:
            push(cfg.start[sb], pmin, pmax, dist + 1)

    leave(group.last, 0, 0, 0)
    while work:
        i = work.pop()
        pmin, pmax, dist = state[i]
        x = ins[i]
        if x.op == "s_waitcnt":
            n = vmcnt_of(x.args)
            if n is not None and n <= pmin:
                continue                                # the whole group has landed on every path: nothing left to follow
        if VM_OP.match(x.op):
            pmin, pmax = min(pmin + 1, CAP), min(pmax + 1, CAP)
        leave(i, pmin, pmax, dist)
    hits = []
    for i, (pmin, pmax, dist) in state.items():
        if ins[i].op == "s_waitcnt":
            n = vmcnt_of(ins[i].args)
            if n is not None:
                hits.append(Hit(i, n, dist, pmin, pmax))
    hits.sort(key=lambda h: (h.dist, h.idx))
    return hits, bool(forced_out)


def trip_length(cfg, loop, group):
    """Fewest instructions from one issue of the group to the next inside the loop, on the paths the walk follows (None: it is not issued again)."""
    dist = {}
    frontier = [(group.last, 0)]
    while frontier:
        nxt = []
        for i, d in frontier:
            b = cfg.block_of[i]
            if i < cfg.end[b]:
                succ = [i + 1]
            else:
                succ = [cfg.start[sb] for sb in cfg.live_succ[b] if sb in loop.body]
            for s in succ:
                # (the rest of a block is walked in one go: only block starts and the group's first load are recorded)
                e = cfg.end[cfg.block_of[s]]
                stop = group.first if s <= group.first <= e else None
                if stop is not None:
                    cand = d + 1 + (stop - s) + (group.last - group.first)
                    dist["trip"] = min(dist.get("trip", cand), cand)
                    continue
                if s not in dist or d + 1 < dist[s]:
                    dist[s] = d + 1
                    nxt.append((e, d + 1 + (e - s)))
        frontier = nxt
    return dist.get("trip")


def landed(m, n, p):
    """How many of a group's m loads a vmcnt(n) lands when p operations were issued behind the group's last one."""
    return max(0, min(m, m + p - n))


def analyse_loop(cfg, loops, loop, gap=16, min_loads=4):
    """For the loop's groups of at least min_loads loads: [(group, trip, [(Hit, loads it is the first to land on some path, on every path)])]."""
    out = []
    for g in load_groups(cfg, loops, loop, gap):
        m = len(g.members)
        if m < min_loads:
            continue
        # a stage loop with a second entry comes out of find_loops without the blocks it shares with its prologue: where the walk is forced out
        # of the body, it is repeated in the next loop around it
        around = sorted((lp for lp in loops if loop.body <= lp.body), key=lambda lp: len(lp.body))
        for lp in around:
            hits, forced_out = walk(cfg, lp, g)
            if not forced_out:
                break
        # the trip is looked for the same way: an early wait ends the walk before it is forced out, so the loop it ended in may be the one
        # without a way back to the group
        trip = next((t for t in (trip_length(cfg, o, g) for o in around[around.index(lp):]) if t is not None), None)
        rows, done, done_every = [], 0, 0
        for h in hits:
            some, every = landed(m, h.n, h.pmax), landed(m, h.n, h.pmin)
            if some > done or every > done_every:
                rows.append((h, max(0, some - done), max(0, every - done_every)))
                done, done_every = max(done, some), max(done_every, every)
        out.append((g, trip, rows))
    return out


def report(cfg, labels, loops, names, gap, min_loads, early=0.4, only_named=False, summary=False, out=sys.stdout):
    """Prints the loops that issue a prefetch group; returns {header label: (loads landed early in the trip that issued them, loads)}."""
    ins = cfg.ins
    total = {}
    for lp in loops:
        label = next((l for l, i in labels.items() if i == lp.head and l.startswith(".LBB")), "?")
        name = names.get(label, "")
        if only_named and not name:
            continue
        res = analyse_loop(cfg, loops, lp, gap, min_loads)
        if not res:
            continue
        body = [ins[i] for i in loop_instructions(cfg, lp)]
        print("loop %s%s: header at line %d, %d instructions, %d mfma, %d vector loads (%d scratch), %d vector stores" % (
            label, " [%s]" % name if name else "", ins[lp.head].line, len(body), sum(x.op.startswith("v_mfma") for x in body),
            sum(bool(VM_LOAD.match(x.op)) for x in body), sum(x.op.startswith("scratch_load") for x in body),
            sum(bool(VM_OP.match(x.op)) and not VM_LOAD.match(x.op) for x in body)), file=out)
        early_sum = loads_sum = unknown = 0
        for g, trip, rows in res:
            m = len(g.members)
            loads_sum += m
            if not summary:
                print("  group of %d global loads, lines %d-%d, shortest trip to their next issue %s instructions" % (
                    m, ins[g.first].line, ins[g.last].line, trip if trip is not None else "?"), file=out)
            for h, some, every in rows:
                # no way back to the group was found: the wait's place in the trip is not known and is not made up.  A wait no further behind
                # the issue than two loads of a group may lie apart is early whatever the trip; any other is counted as not placed.
                part = min(1.0, h.dist / trip) if trip else None
                if (part is not None and part < early) or (part is None and h.dist <= gap):
                    early_sum += some
                elif part is None:
                    unknown += some
                if not summary:
                    print("    line %d  s_waitcnt vmcnt(%d)  %4d instructions behind the issue (%s %% of the trip)  first to land %d (on every path %d), "
                          "%d-%d operations issued behind the group, up to %d stay in flight" % (
                              ins[h.idx].line, h.n, h.dist, "%3.0f" % (100.0 * part) if part is not None else "  ?", some, every, h.pmin, h.pmax,
                              min(h.n, h.pmax)), file=out)
            if not rows and not summary:
                print("    no wait lands any of them before they are issued again", file=out)
        print("  prefetch loads landed in the first %.0f %% of the trip that issued them: %d of %d%s" % (
            100 * early, early_sum, loads_sum, " (%d more landed at a place in the trip that could not be found)" % unknown if unknown else ""), file=out)
        total[label] = (early_sum, loads_sum)
    return total


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("asm")
    ap.add_argument("kernel", help="a mangled symbol, or a template name such as 'k_qp_solve<17,4,false>'")
    ap.add_argument("--name", action="append", default=[], metavar="LABEL=NAME", help="call the loop with this header label NAME in the report")
    ap.add_argument("--only-named", action="store_true", help="report the loops given with --name only")
    ap.add_argument("--summary", action="store_true", help="one headline per loop, no groups")
    ap.add_argument("--min-loads", type=int, default=4, help="smallest run of global loads that counts as a prefetch group (default 4)")
    ap.add_argument("--gap", type=int, default=16, help="most instructions between two loads of one group (default 16)")
    ap.add_argument("--early", type=float, default=0.4, help="a load landed before this part of the trip to its group's next issue counts as landed in the stage that issued it (default 0.4)")
    a = ap.parse_args(argv)
    with open(a.asm, errors="replace") as f:
        lines = f.read().split("\n")
    sym, ins, labels = parse_kernel(lines, a.kernel)
    cfg = Cfg(ins, labels)
    loops = find_loops(cfg)
    print("kernel %s: %d instructions, %d loops" % (sym, len(ins), len(loops)))
    report(cfg, labels, loops, dict(n.split("=", 1) for n in a.name), a.gap, a.min_loads, a.early, a.only_named, a.summary)
    return 0


if __name__ == "__main__":
    sys.exit(main())
