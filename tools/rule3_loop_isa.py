"""What does one rule-3 step of the 32-lane stage-1 kernel cost in instructions?  Disassembles k_stage1_row<1, 16, false>
(or the instantiation named with --kernel) of a gecm_rowk.o, takes the innermost loop that holds the three multiplies of
a point addition (the smallest backward branch spanning 3 x 3 x ROWS multiply-adds) and prints its instruction counts by
class, its size in bytes and the kernel's registers and scratch.  With two objects: the two columns side by side.
usage: python tools/rule3_loop_isa.py <gecm_rowk.o> [<other gecm_rowk.o>] [--kernel 'k_stage1_row<1, 16, false>'] [--dump]"""
import os, re, subprocess, sys, tempfile
LLVM = "/opt/rocm/lib/llvm/bin"
CLASSES = ("v_mad_[iu]64_[iu]32", "v_mov_b32_dpp", "v_mov_b64_dpp", "v_mov_b32", "v_mov_b64", "other VALU", "s_nop", "ds_swizzle",
           "other (scalar, waits, branches)")


def code_object(obj, td):
    fat, co = os.path.join(td, "fat.bin"), os.path.join(td, "dev.co")
    subprocess.run([LLVM + "/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + fat, "--output=" + co], check=True, stderr=subprocess.DEVNULL)
    return co


def kernel_body(co, kernel):
    """[(address, mnemonic, operands, branch target or None)] of the kernel whose demangled name is `kernel`"""
    text = subprocess.run([LLVM + "/llvm-objdump", "-d", "-C", "--no-show-raw-insn", co], check=True, capture_output=True,
                          text=True).stdout
    body, inside = [], False
    for line in text.splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            inside = m.group(1).startswith("void " + kernel + "(") or m.group(1).startswith(kernel + "(")
            continue
        if not inside or not line.startswith("\t"):
            continue
        ins, _, comment = line.partition("//")
        ins = ins.split()
        if not ins or ":" not in comment:
            continue
        addr = int(comment.split(":")[0].strip(), 16)
        tgt = re.search(r"\+0x([0-9a-f]+)>\s*$", comment)
        body.append((addr, ins[0], " ".join(ins[1:]), tgt and int(tgt.group(1), 16)))
    if not body:
        sys.exit("kernel %r not found in %s" % (kernel, co))
    return body


def classify(mn, ops):
    if re.fullmatch(r"v_mad_[iu]64_[iu]32", mn):
        return CLASSES[0]
    if mn in ("v_mov_b32_dpp", "v_mov_b64_dpp"):
        return mn
    if mn in ("v_mov_b32", "v_mov_b64", "v_mov_b32_e32", "v_mov_b64_e32"):
        return mn[:9]
    if mn.startswith("v_") and mn.endswith("_dpp"):
        return "other VALU"
    if mn.startswith("v_"):
        return "other VALU"
    if mn in ("s_nop", "ds_swizzle_b32"):
        return mn[:10]
    return CLASSES[-1]


def resources(co, kernel):
    """(vgprs, sgprs, scratch bytes) from the code object's metadata notes"""
    notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out = None
    nq, rows, alds = [t.strip() for t in kernel[kernel.index("<") + 1:kernel.index(">")].split(",")]
    mangled = "_Z12k_stage1_rowILi%sELi%sELb%dEE" % (nq, rows, alds == "true")
    for block in notes.split("- .agpr_count")[1:]:
        if re.search(r"\.name:\s+" + mangled + "v", block):
            g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
            out = (g("vgpr_count"), g("sgpr_count"), g("private_segment_fixed_size"))
    return out


def analyse(obj, kernel, dump):
    with tempfile.TemporaryDirectory() as td:
        co = code_object(obj, td)
        body = kernel_body(co, kernel)
        res = resources(co, kernel)
    rows = int(kernel.split(",")[1])
    first = body[0][0]
    index = {a: i for i, (a, _, _, _) in enumerate(body)}
    best = None
    for i, (addr, mn, ops, tgt) in enumerate(body):
        if not mn.startswith("s_cbranch") and mn != "s_branch":
            continue
        if tgt is None or first + tgt > addr or first + tgt not in index:
            continue
        j = index[first + tgt]
        mads = sum(1 for k in range(j, i + 1) if classify(body[k][1], body[k][2]) == CLASSES[0])
        if mads >= 9 * rows and (best is None or i - j < best[1] - best[0]):
            best = (j, i)
    if best is None:
        sys.exit("no loop with %d multiply-adds in %s" % (9 * rows, kernel))
    j, i = best
    for k in range(i + 1, len(body)):               # a second way back to the same loop head (the fetch of the next tape byte)
        if body[k][1] in ("s_branch",) or body[k][1].startswith("s_cbranch"):
            if body[k][3] is not None and first + body[k][3] == body[j][0]:
                i = k
    counts = dict.fromkeys(CLASSES, 0)
    for k in range(j, i + 1):
        counts[classify(body[k][1], body[k][2])] += 1
        if dump:
            print("%6x  %s %s" % (body[k][0], body[k][1], body[k][2]))
    end = body[i + 1][0] if i + 1 < len(body) else body[i][0] + 4
    counts["loop bytes"] = end - body[j][0]
    counts["kernel bytes"] = body[-1][0] + 4 - first
    counts["VGPRs"], counts["SGPRs"], counts["scratch bytes"] = res if res else (-1, -1, -1)
    return counts


def main(argv):
    kernel, dump, objs = "k_stage1_row<1, 16, false>", False, []
    it = iter(argv)
    for a in it:
        if a == "--kernel":
            kernel = next(it)
        elif a == "--dump":
            dump = True
        else:
            objs.append(a)
    if not 1 <= len(objs) <= 2:
        sys.exit(__doc__)
    cols = [analyse(o, kernel, dump) for o in objs]
    print("%s, the loop of rule-3 steps (all paths of one iteration)" % kernel)
    for key in cols[0]:
        print("%-34s %s" % (key, " ".join("%8d" % c[key] for c in cols)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
