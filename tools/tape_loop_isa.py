"""What do the events of the 32-lane stage-1 kernel cost in instructions, the rule-3 step and the others?  Disassembles
k_stage1_row<1, 16, false> (or the instantiation named with --kernel) of a gecm_rowk.o, takes the tape loop (the widest
backward branch that spans the multiply-adds of a point addition) and cuts it into stretches at every far jump (a branch
over more than FAR bytes, or backwards) and at every target of one: a stretch is then a piece of straight-line code, short
forward skips included (both sides counted).  Prints, per stretch that holds a multiply, its instruction counts by class
and its bytes, with a label from what it holds:

  rule-3 step            three multiplies, no subtraction (a double has w = t - q), three renaming v_cndmask or more
  addition               three multiplies, no subtraction, fewer v_cndmask
  double                 three multiplies, a subtraction
  addition and double    six multiplies

and then the sums: the rule-3 step, and the generic code = everything else in the tape loop, multiplies or not.  (Where
rule-3 steps are a loop of their own inside the tape loop, as before DESIGN.md §5g, the rule-3 stretch is that loop, and
tools/rule3_loop_isa.py counts the same instructions.)  With two objects: one after the other.
usage: python tools/tape_loop_isa.py <gecm_rowk.o> [<other gecm_rowk.o>] [--kernel 'k_stage1_row<1, 16, false>']"""
import sys, tempfile

from rule3_loop_isa import CLASSES, classify, code_object, kernel_body, resources

FAR = 256
MAD = CLASSES[0]


def is_branch(mn):
    return mn == "s_branch" or mn.startswith("s_cbranch")


def analyse(obj, kernel):
    with tempfile.TemporaryDirectory() as td:
        co = code_object(obj, td)
        body = kernel_body(co, kernel)
        res = resources(co, kernel)
    rows = int(kernel.split(",")[1])
    first = body[0][0]
    index = {a: i for i, (a, _, _, _) in enumerate(body)}
    size = lambda i: (body[i + 1][0] if i + 1 < len(body) else body[i][0] + 4) - body[i][0]
    loop = None
    for i, (addr, mn, ops, tgt) in enumerate(body):
        if is_branch(mn) and tgt is not None and first + tgt <= addr and first + tgt in index:
            j = index[first + tgt]
            mads = sum(1 for k in range(j, i + 1) if classify(body[k][1], body[k][2]) == MAD)
            if mads >= 9 * rows and (loop is None or i - j > loop[1] - loop[0]):
                loop = (j, i)
    if loop is None:
        sys.exit("no loop with %d multiply-adds in %s" % (9 * rows, kernel))
    lo, hi = loop
    for k in range(hi + 1, len(body)):                  # further ways back into the loop behind its last back edge
        if is_branch(body[k][1]) and body[k][3] is not None and body[lo][0] <= first + body[k][3] <= body[hi][0]:
            hi = k
    cuts = {lo, hi + 1}
    for k in range(lo, hi + 1):
        addr, mn, ops, tgt = body[k]
        if is_branch(mn) and tgt is not None and first + tgt in index:
            t = first + tgt
            if t <= addr or t - addr > FAR:
                cuts.add(k + 1)
                if lo <= index[t] <= hi:
                    cuts.add(index[t])
    cuts = sorted(cuts)
    stretches = []
    for a, b in zip(cuts, cuts[1:]):
        c = dict.fromkeys(CLASSES, 0)
        subs = picks = 0
        for k in range(a, b):
            c[classify(body[k][1], body[k][2])] += 1
            subs += body[k][1].startswith("v_sub")
            picks += body[k][1].startswith("v_cndmask")
        c["bytes"] = sum(size(k) for k in range(a, b))
        mults = c[MAD] / (3.0 * rows)
        label = ""
        if mults >= 6:
            label = "addition and double"
        elif mults >= 3:
            label = "double" if subs else "rule-3 step" if picks >= 3 else "addition"
        elif c[MAD]:
            label = "(part of a point operation)"
        stretches.append((body[a][0] - first, label, c))
    return stretches, res


def total(stretches, want):
    out = dict.fromkeys(list(CLASSES) + ["bytes"], 0)
    for _, label, c in stretches:
        if (label == "rule-3 step") == want:
            for k in out:
                out[k] += c[k]
    return out


def main(argv):
    kernel, objs = "k_stage1_row<1, 16, false>", []
    it = iter(argv)
    for a in it:
        if a == "--kernel":
            kernel = next(it)
        else:
            objs.append(a)
    if not 1 <= len(objs) <= 2:
        sys.exit(__doc__)
    for o in objs:
        stretches, res = analyse(o, kernel)
        print("%s of %s: VGPRs %d, SGPRs %d, scratch %d bytes" % ((kernel, o) + (res or (-1, -1, -1))))
        keys = list(CLASSES) + ["bytes"]
        print("%-8s %-28s %s" % ("offset", "stretch of the tape loop", " ".join("%10s" % k[:10] for k in keys)))
        for off, label, c in stretches:
            if c[MAD]:
                print("%#-8x %-28s %s" % (off, label, " ".join("%10d" % c[k] for k in keys)))
        for name, want in (("rule-3 step", True), ("generic code (all the rest)", False)):
            t = total(stretches, want)
            valu = sum(t[k] for k in CLASSES[:6])
            print("%-8s %-28s %s   VALU %d" % ("sum", name, " ".join("%10d" % t[k] for k in keys), valu))
        print()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
