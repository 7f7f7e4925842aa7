"""Instruction, v_readlane / v_writelane and scratch counts per region of the 64-texel IrT kernels, from the device assembly of kernels.hip:

    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> --cuda-device-only -S -o kernels.s texir_code_amd/csrc/kernels.hip
    python tools/isa_regions.py kernels.s [substring of the mangled kernel names, default irt_group_kernelILb0]

The regions come from the kernel's control-flow graph, not from line numbers (the compiler lays the blocks out in no source order): the chunk loop is the
outermost cycle, the pass loop the cycle inside it that holds the traversal's scheduler (the two s_bcnt1_i32_b64 of trace_core), the traversal loop the
cycle inside that.  `pass head` = the blocks of the pass loop outside the traversal loop from which the traversal loop can still be reached in that pass
(sampling, ray set-up), `pass tail` = the others (the hit shader and the accumulation), `chunk` = the chunk loop outside the pass loop (ticket, texel
load, frame, reduction, store), `outside` = prologue and epilogue.  Static counts: what the kernel holds, not what a wave executes."""
import re
import sys


def kernels(path, pat):
    name, body = None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None and pat in m.group(1):
            name, body = m.group(1), []
            continue
        if name is not None:
            body.append(line.rstrip("\n"))
            if "s_endpgm" in line:
                yield name, body
                name = None


def blocks(body):
    """[(label, [instructions])], edges as indices"""
    bl, cur = [("entry", [])], {}
    for line in body:
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            bl.append((m.group(1), []))
            continue
        m = re.match(r"^\s+([a-z][a-z0-9_]+)\b(.*)", line)
        if m and not line.lstrip().startswith((";", ".")):
            bl[-1][1].append((m.group(1), m.group(2)))
    idx = {b[0]: i for i, b in enumerate(bl)}
    succ = [set() for _ in bl]
    for i, (_, ins) in enumerate(bl):
        fall = True
        for op, rest in ins:
            if op.startswith("s_cbranch") or op == "s_branch":
                t = re.search(r"(\.LBB\w+)", rest)
                if t and t.group(1) in idx:
                    succ[i].add(idx[t.group(1)])
            if op in ("s_branch", "s_endpgm"):
                fall = False
        if fall and i + 1 < len(bl):
            succ[i].add(i + 1)
    return bl, succ


def sccs(nodes, succ):
    """strongly connected components with a cycle (Tarjan, iterative)"""
    nodes = set(nodes)
    index, low, on, stack, out, n = {}, {}, set(), [], [], [0]
    for root in sorted(nodes):
        if root in index:
            continue
        work = [(root, iter(sorted(succ[root] & nodes)))]
        index[root] = low[root] = n[0]; n[0] += 1; stack.append(root); on.add(root)
        while work:
            v, it = work[-1]
            for w in it:
                if w not in index:
                    index[w] = low[w] = n[0]; n[0] += 1; stack.append(w); on.add(w)
                    work.append((w, iter(sorted(succ[w] & nodes))))
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            else:
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == index[v]:
                    comp = set()
                    while True:
                        w = stack.pop(); on.discard(w); comp.add(w)
                        if w == v:
                            break
                    if len(comp) > 1 or v in succ[v]:
                        out.append(comp)
    return out


def inner_loop(loop, succ, marked):
    """the cycle inside `loop` that holds the marked blocks, after the loop's headers (blocks entered from outside it) are taken out"""
    heads = {v for v in loop if any(v in succ[u] for u in range(len(succ)) if u not in loop)} or {min(loop)}
    for comp in sccs(loop - heads, succ):
        if comp & marked:
            return comp
    return set()


def main():
    path, pat = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "irt_group_kernelILb0")
    for name, body in kernels(path, pat):
        bl, succ = blocks(body)
        marked = {i for i, (_, ins) in enumerate(bl) if any(op == "s_bcnt1_i32_b64" for op, _ in ins)}
        chunk = next((c for c in sccs(range(len(bl)), succ) if c & marked), set())
        passes = inner_loop(chunk, succ, marked)
        trav = inner_loop(passes, succ, marked)
        rest = passes - trav
        # blocks of the pass loop from which the traversal is reached in the SAME pass: not through the pass loop's header (the header itself is head)
        heads = {v for v in passes if any(v in succ[u] for u in range(len(succ)) if u not in passes)}
        head, grew = set(), True
        while grew:
            grew = False
            for v in rest - head:
                if succ[v] & (trav | (head - heads)):
                    head.add(v); grew = True
        head |= heads & rest
        region = {}
        for i in range(len(bl)):
            region[i] = "traversal" if i in trav else "pass head" if i in head else "pass tail" if i in rest else "chunk" if i in chunk else "outside"
        rows = {r: [0, 0, 0, 0] for r in ("outside", "chunk", "pass head", "traversal", "pass tail")}
        for i, (_, ins) in enumerate(bl):
            for op, _ in ins:
                r = rows[region[i]]
                r[0] += 1
                r[1] += op.startswith("v_readlane")
                r[2] += op.startswith("v_writelane")
                r[3] += op.startswith("scratch_")
        print(name)
        print("  %-10s %12s %10s %11s %8s" % ("region", "instructions", "v_readlane", "v_writelane", "scratch"))
        for r, v in rows.items():
            print("  %-10s %12d %10d %11d %8d" % (r, *v))
        print("  %-10s %12d %10d %11d %8d" % ("total", *[sum(v[k] for v in rows.values()) for k in range(4)]))


if __name__ == "__main__":
    main()
