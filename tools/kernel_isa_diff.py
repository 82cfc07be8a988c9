"""Are the kernels of two builds the same instructions?  For every gecm_kernels_*_p?.o, gecm_rowk.o and gecm_rowk_wide.o present in both
build directories: the gfx950 code object (taken as tools/kernel_resources.py takes it) is disassembled and every
symbol's instruction stream compared.  Masked: the padding after a function, and the pc-relative literal of a call
(s_getpc_b64 and the s_add_u32 / s_addc_u32 pair behind it), which moves with the layout of the object.
One line per object (symbols compared, symbols differing), then the names that differ or exist on one side only.
Exit status 0 only if every symbol of every object is on both sides with the same instructions.
usage: python tools/kernel_isa_diff.py <dirA> <dirB>"""
import glob, os, re, subprocess, sys, tempfile
LLVM = "/opt/rocm/lib/llvm/bin"
PADDING = ("s_nop", "s_code_end")


def symbols(obj):
    """{mangled name: [instruction, ...]} of the gfx950 code object in one host object."""
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "fat.bin"), os.path.join(td, "dev.co")
        subprocess.run([LLVM + "/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
        subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        "--input=" + fat, "--output=" + co], check=True, stderr=subprocess.DEVNULL)
        text = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True,
                              text=True).stdout
    out, cur, pcrel = {}, None, 0
    for line in text.splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith("\t") or line.strip() == "...":
            continue
        ins = " ".join(line.split("//")[0].split())       # no address, no encoding, no branch-target comment
        if ins.startswith("s_getpc_b64"):
            pcrel = 2
        elif pcrel and re.match(r"s_addc?_u32 ", ins):
            ins = ins.rsplit(",", 1)[0] + ", <pc-relative>"
            pcrel -= 1
        else:
            pcrel = 0
        cur.append(ins)
    for body in out.values():
        while body and body[-1].split()[0] in PADDING:
            body.pop()
    return out


def main(dir_a, dir_b):
    names = lambda d: {os.path.basename(p) for pat in ("gecm_kernels_*_p?.o", "gecm_rowk.o", "gecm_rowk_wide.o") for p in glob.glob(os.path.join(d, pat))}
    both = sorted(names(dir_a) & names(dir_b), key=lambda n: [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", n)])
    if not both:
        print("no kernel object is in both directories")
        return 1
    bad = 0
    for name in both:
        a, b = symbols(os.path.join(dir_a, name)), symbols(os.path.join(dir_b, name))
        differ = sorted(s for s in a.keys() & b.keys() if a[s] != b[s])
        only_a, only_b = sorted(a.keys() - b.keys()), sorted(b.keys() - a.keys())
        print("%-26s %3d symbols compared, %d differ, %d only in A, %d only in B" %
              (name, len(a.keys() & b.keys()), len(differ), len(only_a), len(only_b)))
        for s in differ:
            print("    differs    %s  (%d -> %d instructions)" % (s, len(a[s]), len(b[s])))
        for s in only_a:
            print("    only in A  %s" % s)
        for s in only_b:
            print("    only in B  %s" % s)
        bad += len(differ) + len(only_a) + len(only_b)
    print("%d objects, %d symbols differing or on one side only" % (len(both), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
