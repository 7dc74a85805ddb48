"""Developer tool: do the kernels of some sources compile to the same gfx950 code as at another commit?
    python tools/kernel_asm_diff.py REV pct_fit.hip pct_fit_ball.hip [--strip REGEX]
Compiles csrc/<source> of REV (git archive into a temporary directory) and of the working tree with the library's flags
plus --cuda-device-only -S -Rpass-analysis=kernel-resource-usage, and compares kernel by kernel: the instructions, with
the kernel's own symbol and the function number in block labels (BB<n>_) replaced and white space squeezed, and the
resource usage the compiler reports (registers, scratch, occupancy, LDS).  Kernels are matched by mangled name;
--strip removes a pattern from REV's names first (a template parameter that no longer exists: --strip 'Li0E(?=EEv)').
Exit status 1 if a kernel both trees have differs, or the working tree has a kernel REV has not."""
import os, re, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge


def compile_s(csrc, src, out):
    cmd = [ge.HIPCC] + ge.COMPILE_FLAGS + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", out]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    return r.stderr


def kernels(path):
    """{symbol: normalised instruction lines} of every function of a -S output."""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
        elif name is not None and line.startswith(".Lfunc_end"):
            out[name] = [l for l in (re.sub(r"\s+", " ", re.sub(r"BB\d+_", "BB_", l.replace(name, "SYM"))).strip() for l in body) if l]
            name = None
        elif name is not None:
            body.append(line)
    return out


def resources(remarks):
    out, cur = {}, None
    for l in remarks.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", l)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(\w[\w \[\]/]*): (\S+) \[-R", l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def main():
    args = sys.argv[1:]
    strip = None
    if "--strip" in args:
        i = args.index("--strip")
        strip = re.compile(args[i + 1])
        del args[i:i + 2]
    rev, sources = args[0], args[1:]
    rel = os.path.relpath(ge.CSRC, ge.ROOT)
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "archive", rev, rel, "include"], cwd=ge.ROOT, capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        for src in sources:
            sides = []
            for csrc, tag in ((os.path.join(tmp, rel), "old"), (ge.CSRC, "new")):
                s = os.path.join(tmp, f"{tag}_{src}.s")
                res = resources(compile_s(csrc, src, s))
                sides.append((kernels(s), res, sum(1 for _ in open(s))))
            (old, old_res, old_lines), (new, new_res, new_lines) = sides
            if strip:
                old = {strip.sub("", n): (n, b) for n, b in old.items()}
            else:
                old = {n: (n, b) for n, b in old.items()}
            same = 0
            for n in sorted(set(old) | set(new)):
                if n not in new:
                    print(f"{src}: only in {rev}: {old[n][0]}")
                elif n not in old:
                    print(f"{src}: NEW: {n}")
                    bad += 1
                elif old[n][1] != new[n] or old_res.get(old[n][0]) != new_res.get(n):
                    print(f"{src}: DIFFERENT: {n}  {old_res.get(old[n][0])} -> {new_res.get(n)}")
                    bad += 1
                else:
                    same += 1
            print(f"{src}: {same} kernels identical in instructions and resource usage, {len(old)} in {rev}, {len(new)} now; "
                  f"{old_lines} -> {new_lines} lines of assembly")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
