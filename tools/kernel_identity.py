"""Are the kernels of two source trees the same machine code?  Compiles every device unit of each tree's miniprot_amd/csrc for gfx950
(`hipcc -S --cuda-device-only`, the flags of the Makefile that matter to device code) and compares, kernel by kernel, the text between
the kernel's label and its `.end_amdhsa_kernel` (instructions, kernel descriptor) after stripping `;` comments and renumbering the
local labels (.LBB<n>_, .Lfunc_begin<n>, .Ltmp<n>: they count functions of the unit).  rocPRIM's kernels are counted, not listed.
    python tools/kernel_identity.py PARENT_TREE [THIS_TREE] > profiles/NAME.txt        (a few minutes: every unit is compiled)
Exit status 1 if a kernel differs or the two sets of kernels differ."""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
UNITS = ("dev_ctx.hip", "seed_run.hip", "refine_run.hip", "index_run.hip", "dp_exec.hip", "stats_run.hip")

def kernels_of(tree):
    csrc = os.path.join(tree, "miniprot_amd", "csrc")
    units = [u for u in UNITS if os.path.exists(os.path.join(csrc, u))]
    out = {}
    with tempfile.TemporaryDirectory() as d:
        def asm(u):
            s = os.path.join(d, u + ".s")
            subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-o", s, os.path.join(csrc, u)],
                           check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            return u, open(s).read()
        with ThreadPoolExecutor(4) as ex:
            texts = list(ex.map(asm, units))
    for u, text in texts:
        for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\s*$", text, re.M):
            name = m.group(1)
            a = re.search(r"^%s:" % re.escape(name), text, re.M).start()
            b = text.index(".end_amdhsa_kernel", m.start())
            body, tmp = [], {}
            for line in text[a:b].split("\n"):
                line = line.split(";")[0].rstrip()
                if not line.strip():
                    continue
                line = re.sub(r"\.LBB\d+_", ".LBB_", line)
                line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
                line = re.sub(r"\.Ltmp\d+", lambda t: tmp.setdefault(t.group(0), ".Ltmp#%d" % len(tmp)), line)
                body.append(line)
            assert name not in out or "rocprim" in name, "kernel %s in two units" % name
            if name in out and out[name][1] != "\n".join(body):
                name += " [%s]" % u          # (a rocPRIM kernel that two units compiled differently: listed apart)
            out[name] = (u, "\n".join(body))
    return units, out

def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"^void ", "", re.sub(r"\(.*$", "", d)).replace("mpa::", "") for n, d in zip(names, r)}

parent, this = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
(pu, pk), (tu, tk) = kernels_of(parent), kernels_of(this)
own = lambda k: sorted(n for n in k if "rocprim" not in n)
names = demangle(sorted(set(pk) | set(tk)))
print("# parent units: %s\n# this tree's units: %s" % (" ".join(pu), " ".join(tu)))
print("# kernels: parent %d (+ %d of rocPRIM), this tree %d (+ %d of rocPRIM; a rocPRIM kernel is instantiated by every unit that uses it)"
      % (len(own(pk)), len(pk) - len(own(pk)), len(own(tk)), len(tk) - len(own(tk))))
bad = 0
print("%-10s %-16s %6s  %s" % ("result", "unit", "lines", "kernel"))
for n in sorted(set(own(pk)) | set(own(tk)), key=lambda n: (tk.get(n, ("~",))[0], names[n])):
    if n not in pk or n not in tk:
        res = "only-parent" if n in pk else "only-this"
    else:
        res = "identical" if pk[n][1] == tk[n][1] else "DIFFERENT"
    bad += res != "identical"
    print("%-10s %-16s %6d  %s" % (res, tk.get(n, pk.get(n))[0], tk.get(n, pk.get(n))[1].count("\n") + 1, names[n]))
same_prim = sum(1 for n in tk if "rocprim" in n and n in pk and pk[n][1] == tk[n][1])
print("# rocPRIM kernels of this tree identical to the parent's of the same name: %d of %d" % (same_prim, len(tk) - len(own(tk))))
print("# %d of %d kernels identical" % (len(set(own(pk)) | set(own(tk))) - bad, len(set(own(pk)) | set(own(tk)))))
sys.exit(1 if bad else 0)
