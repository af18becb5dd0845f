"""Compare the gfx950 device code of two source trees kernel by kernel (no GPU needed).

    python scripts/isa_diff.py OLD_TREE NEW_TREE [-j JOBS] [--only gemm.hip ...]

Every csrc/*.hip of both trees is compiled to device assembly with the Makefile's flags, the
assembly is split per kernel, and labels, comments, directives and the per-file `__hip_cuid_`
symbol are dropped.  A kernel matches when the other tree has a kernel of the same name (template
arguments stripped, so a removed template parameter does not count) with equal instruction text.
Kernels without a match are listed with their instruction, VGPR, SGPR and static-LDS counts.
Exit status 1 if any kernel is unmatched.
"""
import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join("transmil_deepgraft_amd", "csrc")


def file_flags(tree):
    """FILEFLAGS_<stem> of the tree's Makefile, with $(VAR) expanded."""
    vars_ = dict(re.findall(r"^(\w+)\s*=\s*(.*)$", open(os.path.join(tree, CSRC, "Makefile")).read(), re.M))
    expand = lambda s: re.sub(r"\$\((\w+)\)", lambda m: vars_.get(m.group(1), ""), s)
    return {k[len("FILEFLAGS_"):]: expand(v).split() for k, v in vars_.items() if k.startswith("FILEFLAGS_")}


def compile_s(tree, name, flags, out):
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *flags, "--cuda-device-only",
                    "-S", "-o", out, os.path.join(tree, CSRC, name)], check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def base_name(mangled):
    """The kernel's own identifier: the last length-prefixed name of the mangled symbol's qualified
    name, i.e. without namespaces, template arguments and parameter types."""
    pos, name = (3 if mangled.startswith("_ZN") else 2), mangled
    while m := re.match(r"\d+", mangled[pos:]):
        pos += len(m.group())
        name, pos = mangled[pos:pos + int(m.group())], pos + int(m.group())
    return name


def kernels(asm):
    """{mangled name: (instruction text, {resource: count})} of one assembly file."""
    asm = re.sub(r"__hip_cuid_\w+", "__hip_cuid", asm)
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.M | re.S):
        name, grab = m.group(1), lambda key: int(re.search(rf"\.amdhsa_{key} (\d+)", m.group(2)).group(1))
        body = re.search(rf"^{re.escape(name)}:.*?\n(.*?)^\.Lfunc_end\d+:", asm, re.M | re.S).group(1)
        insns = [re.sub(r"\.LBB\d+_", ".LBB_", line) for line in (l.split(";")[0].strip() for l in body.splitlines())
                 if line and not line.endswith(":") and not line.startswith(".")]
        out[name] = ("\n".join(insns), {"insns": len(insns), "vgpr": grab("next_free_vgpr"),
                                        "sgpr": grab("next_free_sgpr"), "lds": grab("group_segment_fixed_size")})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 4))
    ap.add_argument("--only", nargs="*", default=None, help="file names to compare (default: every csrc/*.hip)")
    args = ap.parse_args()
    trees = (args.old, args.new)
    names = sorted({f for t in trees for f in os.listdir(os.path.join(t, CSRC)) if f.endswith(".hip")})
    if args.only:
        names = [f for f in names if f in args.only]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(args.j) as pool:
        jobs = {}
        for side, tree in enumerate(trees):
            flags = file_flags(tree)
            for f in names:
                if os.path.exists(os.path.join(tree, CSRC, f)):
                    jobs[side, f] = pool.submit(compile_s, tree, f, flags.get(f[:-4], []),
                                                os.path.join(tmp, f"{side}_{f}.s"))
        for f in names:
            ks = [kernels(jobs[s, f].result()) if (s, f) in jobs else {} for s in (0, 1)]
            keyed = [{(base_name(n), text) for n, (text, _) in k.items()} for k in ks]
            lines = []
            for side, tag in ((0, "old"), (1, "new")):
                for n, (text, r) in sorted(ks[side].items()):
                    if (base_name(n), text) not in keyed[1 - side]:
                        pretty = subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip() or n
                        lines.append(f"  {tag} only: {pretty}\n            insns {r['insns']} vgpr {r['vgpr']} "
                                     f"sgpr {r['sgpr']} lds {r['lds']}")
            print(f"{f}: {len(ks[0])} kernels old, {len(ks[1])} new, {len(lines)} unmatched", flush=True)
            print("\n".join(lines), end="\n" if lines else "")
            bad += len(lines)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
