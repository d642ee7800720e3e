"""Instruction classes of one even + odd chunk pair of the fused field-MLP kernels' steady-state loop
over a 256 -> 256 layer, from a hipcc -S listing of csrc/mlp_fused.hip:

    python tools/isa_pair.py <file.s> [<symbol substring> ...]      (default: the forward and the chain)

The chunk loop is unrolled by two, so one trip of it is one chunk pair.  The loop is found on the
control-flow graph, not in text order: every edge to a dominating block closes a natural loop (the
blocks that reach the edge without passing its target); the pair loop of a register-fed 256-wide layer is a
loop with exactly two barriers and 2 x 24 matrix instructions (8 k-blocks x 3 bf16 products; 2 x 8
in a single-pass kernel).  Where several loops qualify (the plain and the generic loop of the same
layer shape) the one with the fewest vector-memory instructions is reported (ties: the fewest
instructions): the plain loop issues two stores per pair where the generic one issues four.  The
totals are over all blocks of the loop, the rarely taken ones (the DMA cursor's layer change)
included.  Instructions are classed by the broad prefixes of tools/isa_loop.py."""
import collections
import json
import re
import sys

CLASSES = ("mfma", "valu", "salu", "lds", "vmem", "other")


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return "other"


def function_body(text, sym):
    m = re.search(r"^(_Z\S*" + re.escape(sym) + r"\S*):", text, re.M)
    if m is None:
        raise KeyError(sym)
    return text[m.end():text.index(".Lfunc_end", m.start())].split("\n")


def blocks_of(lines):
    """[(label or None, [opcode operands...])] in text order, plus successor lists by block index."""
    blocks = [[None, []]]
    for ln in lines:
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            blocks.append([m.group(1), []])
            continue
        if re.match(r"^; %bb\.\d+:", ln):
            blocks.append([None, []])
            continue
        t = ln.split(";")[0].strip()
        if not t or t.startswith("."):
            continue
        blocks[-1][1].append(t)
    index = {b[0]: i for i, b in enumerate(blocks) if b[0] is not None}
    succ = []
    for i, (_, ins) in enumerate(blocks):
        out, fall = [], True
        for t in ins:
            f = t.split()
            if f[0].startswith("s_cbranch") and f[-1] in index:
                out.append(index[f[-1]])
            elif f[0] == "s_branch" and f[-1] in index:
                out.append(index[f[-1]])
                fall = False
            elif f[0] in ("s_endpgm", "s_setpc_b64"):
                fall = False
        if fall and i + 1 < len(blocks):
            out.append(i + 1)
        succ.append(out)
    return blocks, succ


def natural_loops(blocks, succ):
    """{header: blocks} of every natural loop: a back edge is an edge n -> h whose target dominates
    its source (block placement in the text plays no part: hipcc rotates these loops)."""
    n = len(blocks)
    pred = collections.defaultdict(list)
    for i, out in enumerate(succ):
        for j in out:
            pred[j].append(i)
    order, seen, stack = [], {0}, [(0, iter(succ[0]))]
    while stack:                                  # reverse postorder from the entry block
        node, it = stack[-1]
        for j in it:
            if j not in seen:
                seen.add(j)
                stack.append((j, iter(succ[j])))
                break
        else:
            order.append(node)
            stack.pop()
    order.reverse()
    rpo = {b: k for k, b in enumerate(order)}
    idom = {0: 0}

    def meet(a, b):
        while a != b:
            while rpo[a] > rpo[b]:
                a = idom[a]
            while rpo[b] > rpo[a]:
                b = idom[b]
        return a

    changed = True
    while changed:                                # Cooper, Harvey, Kennedy: iterative dominators
        changed = False
        for b in order[1:]:
            ps = [p for p in pred[b] if p in idom]
            new = ps[0]
            for p in ps[1:]:
                new = meet(p, new)
            if idom.get(b) != new:
                idom[b] = new
                changed = True

    def dominates(h, x):
        while True:
            if x == h:
                return True
            if x == 0:
                return False
            x = idom[x]

    loops = {}
    for i in order:
        for h in succ[i]:
            if h not in idom or not dominates(h, i):
                continue
            body, work = {h, i}, [i] if i != h else []
            while work:
                x = work.pop()
                for p in pred[x]:
                    if p not in body and p in idom:
                        body.add(p)
                        work.append(p)
            loops.setdefault(h, set()).update(body)
    return loops


def count(blocks, body):
    c = collections.Counter({k: 0 for k in CLASSES})
    c["barrier"] = 0
    for i in body:
        for t in blocks[i][1]:
            op = t.split()[0]
            c[classify(op)] += 1
            if op == "s_barrier":
                c["barrier"] += 1
    return c


def pair_counts(text, sym, mfma_per_pair=(48, 16)):
    """Totals of the pair loop of kernel `sym`: {class: count, "non_mfma": ..., "blocks": ...}."""
    blocks, succ = blocks_of(function_body(text, sym))
    best = None
    for h, body in natural_loops(blocks, succ).items():
        c = count(blocks, body)
        if c["barrier"] != 2 or c["mfma"] not in mfma_per_pair:
            continue
        non = sum(c[k] for k in CLASSES if k != "mfma")
        key = (c["vmem"], non)
        if best is None or key < best[0]:
            best = (key, c, non, len(body))
    if best is None:
        raise LookupError(f"no chunk-pair loop in {sym}")
    _, c, non, nb = best
    out = {k: c[k] for k in CLASSES}
    out.update(non_mfma=non, blocks=nb)
    return out


def resources(text, sym):
    """(VGPRs, scratch bytes) of kernel `sym`, from the listing's `.set <kernel>.num_vgpr` /
    `.private_seg_size` lines."""
    def field(name):
        return int(re.search(r"^\s*\.set\s+_Z\S*" + re.escape(sym) + r"\S*\." + name + r",\s*(\d+)", text, re.M).group(1))
    return field("num_vgpr"), field("private_seg_size")


if __name__ == "__main__":
    text = open(sys.argv[1]).read()
    syms = sys.argv[2:] or ["mlp_fused_kernelILi0E", "mlp_fused_kernelILi1E"]
    for sym in syms:
        r = pair_counts(text, sym)
        vg, priv = resources(text, sym)
        r.update(vgpr=vg, scratch_bytes=priv)
        print(json.dumps({sym: r}))
