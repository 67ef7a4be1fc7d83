"""Instruction mix and spill sites of one kernel in a hipcc -S listing:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only heat_amd/csrc/kernels.hip -o /tmp/k.s
    python tools/isa_stats.py /tmp/k.s k_surfaces_stream
(the k_series_* kernels and k_fill_f64 are in heat_amd/csrc/series_kernels.hip: take its listing the same way)

    python tools/isa_stats.py /tmp/k.s k_surfaces_fastILi16ELi0ELi1ELi0ELi4ELi0ELi0E --blocks [--loop BB112_62] [--json OUT]
The second form prints the instruction classes of every basic block between the header of the sub-timestep loop and
the loop's closing barrier: f64 VALU / other VALU by opcode / SALU (with SMEM) / LDS / VMEM, and how many DPP moves have
a plain v_mov_b32 into their destination right in front of them (a named `old` value). The loop is, unless --loop
names its header, the one that holds a barrier and the most f64 instructions (the compiler's own loop comments say which
block belongs to which loop). Blocks are the listing's labels and `%bb.N` comments: counts are static."""
import collections, json, re, sys


def kernel_lines(path, name):
    txt = open(path).read().split("\n")
    start = next(i for i, l in enumerate(txt) if l.startswith("_Z") and name in l and l.rstrip().split(":")[0].endswith(l.split(":")[0]) and ":" in l)
    end = next(i for i in range(start, len(txt)) if txt[i].startswith(".Lfunc_end"))
    return txt[start + 1:end]


def is_instruction(l):
    return l.startswith("\t") and not l.strip().startswith((".", ";"))


def group_of(op):
    return ("scratch" if op.startswith("scratch") else "vmem" if op.startswith(("global_", "buffer_", "flat_")) else
            "lds" if op.startswith("ds_") else "salu/smem" if op.startswith("s_") else
            "valu f64" if op.startswith("v_") and "f64" in op else "valu other" if op.startswith("v_") else "other")


def whole_kernel(lines):
    ins = [l.strip() for l in lines if is_instruction(l)]
    print("instructions:", len(ins))
    c = collections.Counter(i.split()[0] for i in ins)
    groups = collections.Counter()
    for op, n in c.items():
        groups[group_of(op)] += n
    print(dict(groups))
    print(c.most_common(30))
    sites = [n for n, i in enumerate(ins) if i.startswith("scratch_")]
    print("scratch instructions:", len(sites), "at", sites[:80])


BLOCK = re.compile(r"^(?:\.L(BB\d+_\d+):|; %bb\.(\d+):)")
LOOP_OF = re.compile(r"in Loop: Header=(BB\d+_\d+)")
PARENT = re.compile(r"Parent Loop (BB\d+_\d+)")


def split_blocks(lines):
    """[(name, set of the loops the block is in, [instructions])] in listing order."""
    blocks, cur, prefix = [], None, None
    for i, l in enumerate(lines):
        m = BLOCK.match(l)
        if m:
            name = m.group(1) or "bb.%s" % m.group(2)
            if prefix is None and m.group(1):
                prefix = m.group(1).split("_")[0]
            loops = set()
            lo = LOOP_OF.search(l)
            if lo:
                loops.add(lo.group(1))
            j = i  # a loop header's comment runs over the lines that follow: its parents, then "This ... Loop Header"
            header = False
            while True:
                loops.update(PARENT.findall(lines[j]))
                header = header or "Loop Header" in lines[j]
                j += 1
                if j >= len(lines) or not lines[j].startswith(" "):
                    break
            if header and m.group(1):
                loops.add(m.group(1))
            cur = [name, loops, []]
            blocks.append(cur)
        elif cur is not None and is_instruction(l):
            cur[2].append(l.strip())
    # a block "in Loop: Header=H" of an inner loop is in H's parents too
    parents = {}
    for name, loops, _ in blocks:
        if name in loops:
            parents[name] = loops - {name}
    for b in blocks:
        for h in list(b[1]):
            b[1].update(parents.get(h, ()))
    return blocks


def classify(ins):
    row = collections.OrderedDict((k, 0) for k in ("valu f64", "valu other", "salu/smem", "lds", "vmem", "scratch", "other"))
    other = collections.Counter()
    named_old = 0
    for n, i in enumerate(ins):
        op = i.split()[0]
        row[group_of(op)] += 1
        if group_of(op) == "valu other":
            other[op] += 1
        if op.endswith("_dpp"):
            dst = i.split()[1].rstrip(",")
            for back in ins[max(0, n - 4):n]:
                f = back.replace(",", " ").split()
                if f[0] in ("v_mov_b32_e32", "v_mov_b32") and f[1] == dst:
                    named_old += 1
    return row, other, named_old


def loop_blocks(lines, header=None):
    blocks = split_blocks(lines)
    if header is None:
        score = collections.Counter()
        barrier = set()
        for name, loops, ins in blocks:
            for h in loops:
                score[h] += sum(1 for i in ins if group_of(i.split()[0]) == "valu f64")
                if any(i.startswith("s_barrier") for i in ins):
                    barrier.add(h)
        depth = {h: len(next(b[1] for b in blocks if b[0] == h)) for h in barrier}
        # the innermost loop that holds a barrier (the persistent loop around it holds all of its instructions too)
        header = max(barrier, key=lambda h: (depth[h], score[h]))
    inside = [b for b in blocks if header in b[1]]
    first = next(n for n, b in enumerate(inside) if b[0] == header)
    inside = inside[first:]
    last = max(n for n, b in enumerate(inside) if any(i.startswith("s_barrier") for i in b[2]))
    out = inside[:last + 1]
    # the closing barrier ends the last block
    name, loops, ins = out[-1]
    cut = max(n for n, i in enumerate(ins) if i.startswith("s_barrier"))
    out[-1] = [name, loops, ins[:cut + 1]]
    return header, out


def per_block(lines, header=None, json_out=None):
    header, blocks = loop_blocks(lines, header)
    print("loop header %s: %d blocks up to the closing barrier" % (header, len(blocks)))
    print("%-12s %5s %5s %5s %5s %4s %5s %4s  %s" % ("block", "insts", "f64", "other", "salu", "lds", "vmem", "old", "other VALU by opcode"))
    total = collections.Counter()
    total_other = collections.Counter()
    rows = []
    for name, loops, ins in blocks:
        row, other, named_old = classify(ins)
        inner = sorted(loops - {header} - set(next(b[1] for b in blocks if b[0] == header)))
        label = name + ("*" if inner else "")  # * the block belongs to a loop inside the sub-timestep loop
        ops = " ".join("%s:%d" % (k.replace("v_", "", 1), v) for k, v in other.most_common())
        print("%-12s %5d %5d %5d %5d %4d %5d %4d  %s" % (label, len(ins), row["valu f64"], row["valu other"], row["salu/smem"],
                                                       row["lds"], row["vmem"] + row["scratch"], named_old, ops))
        total.update(row)
        total["insts"] += len(ins)
        total["named old"] += named_old
        total_other.update(other)
        rows.append({"block": label, "insts": len(ins), **row, "dpp_with_named_old": named_old, "valu_other_by_opcode": dict(other)})
    print("%-12s %5d %5d %5d %5d %4d %5d %4d  %s" % ("sum", total["insts"], total["valu f64"], total["valu other"], total["salu/smem"],
                                                   total["lds"], total["vmem"] + total["scratch"], total["named old"],
                                                   " ".join("%s:%d" % (k.replace("v_", "", 1), v) for k, v in total_other.most_common())))
    if json_out:
        with open(json_out, "w") as f:
            json.dump({"loop_header": header, "blocks": rows, "sum": dict(total), "sum_valu_other_by_opcode": dict(total_other)}, f, indent=1)


if __name__ == "__main__":
    args = sys.argv[1:]
    lines = kernel_lines(args[0], args[1])
    if "--blocks" in args:
        header = args[args.index("--loop") + 1] if "--loop" in args else None
        per_block(lines, header, args[args.index("--json") + 1] if "--json" in args else None)
    else:
        whole_kernel(lines)
