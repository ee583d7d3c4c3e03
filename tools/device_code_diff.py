#!/usr/bin/env python3
"""CPU only: is the device code of two checkouts the same?  For a change of the host layer alone, where the fat binary still
differs byte for byte (kernels reached through a generic lambda are instantiated later, so they are emitted in another order and
every PC-relative offset to a global moves).  Compiles csrc/ddz_engine.hip of both trees for gfx950, device side only, to
assembly with the resource-usage remarks, in the default build and with -DDDZ_NATIVE_JOKER_KICKERS=1, and compares
  1. the set of kernel names, and the resource lines of every kernel (SGPRs, VGPRs, AGPRs, scratch, dynamic stack, occupancy,
     both spill counts, LDS), by name;
  2. the assembly of every symbol (kernels, device functions, globals), by name: the file split at its global labels, comments
     dropped, the local labels of a body (.LBB<f>_<b>, .Ltmp<n>, .Lfunc_end<f>) renumbered in their order of appearance, the
     hash in __hip_cuid_<hash> masked;
  3. the entries of the amdhsa.kernels metadata list, by name.
Exit status 0 where all of it is equal.  The outputs stay in --work (a.s, a.rem, a_jk.s, ... b_jk.rem) and are reused when there
WITHOUT a look at the trees: a work directory kept across a change of a tree compares the stale files, so give a fresh one (the
default: a new temporary directory) unless the files are known to belong to the trees.
  python tools/device_code_diff.py PARENT_TREE [THIS_TREE] [--work DIR]"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = (("", []), ("_jk", ["-DDDZ_NATIVE_JOKER_KICKERS=1"]))
LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
LOCAL = re.compile(r"\.L(?:BB\d+_\d+|tmp\d+|func_(?:begin|end)\d+)\b")
LEAD_IN = re.compile(r"^\s*\.(globl|weak|protected|hidden|p2align|type|section|text|data|bss)\b")
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
NAME = re.compile(r"Function Name: (\S+)")


def compile_tree(tree, stem, extra):
    """starts the compilation of `tree` into stem.s (assembly) and stem.rem (the remarks) -> (command, process, remarks file)"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(tree, "doudizhu-rl_amd", "csrc", "ddz_engine.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
           "-o", stem + ".s"] + extra + [src]
    rem = open(stem + ".rem", "w")
    return cmd, subprocess.Popen(cmd, stderr=rem), rem


def resources(path):
    """kernel name -> its resource lines, from the remarks"""
    out, cur = {}, None
    for line in open(path, errors="replace"):
        if "remark:" not in line or "kernel-resource-usage" not in line:
            continue
        text = line.split("remark:", 1)[1].rsplit("[-Rpass", 1)[0].strip()
        m = NAME.match(text)
        if m:
            cur = out.setdefault(m.group(1), [])
            cur.clear()     # (the remarks come once per diagnostic form: keep the last block)
        elif cur is not None:
            cur.append(text)
    return out


def renumber(lines):
    seen = {}
    return [LOCAL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), ln) for ln in lines]


def symbols(path):
    """-> (symbol -> canonical body, kernel name -> metadata entry, the lines that belong to neither: what stands in front of
    the first label and behind the kernels' metadata; the directives behind the last symbol count as its body)"""
    text = open(path, errors="replace").read()
    head, _, meta = text.partition("\n\t.amdgpu_metadata\n")
    body, chunks, name = {}, [("", [])], ""
    for raw in head.split("\n"):
        ln = CUID.sub("__hip_cuid_#", raw.split(";", 1)[0].rstrip())
        if not ln.strip():
            continue
        m = LABEL.match(ln)
        if m and not ln.startswith(".L"):
            name = m.group(1)
            chunks.append((name, []))
            continue
        chunks[-1][1].append(ln)
    rest = []
    for i, (name, lines) in enumerate(chunks):
        while i + 1 < len(chunks) and lines and LEAD_IN.match(lines[-1]):   # the lead-in of the next symbol
            lines.pop()
        if name:
            assert name not in body, name
            body[name] = renumber(lines)
        else:
            rest = [ln for ln in lines if not LEAD_IN.match(ln)]
    entries = {}
    kernels, _, tail = meta.partition("\namdhsa.target:")
    for e in re.split(r"\n(?=  - \.)", kernels.partition("amdhsa.kernels:\n")[2]):
        m = re.search(r"^\s+\.name:\s+(\S+)", e, re.M)
        if m:
            entries[m.group(1)] = e.split("\n")
    return body, entries, sorted(rest) + tail.split("\n")


def compare(what, a, b, report):
    """two dicts name -> list of lines"""
    bad = 0
    for n in sorted(set(a) | set(b)):
        if n not in a or n not in b:
            report.append(f"{what}: {n} only in {'B' if n not in a else 'A'}")
            bad += 1
        elif a[n] != b[n]:
            k = next((i for i, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
            report.append(f"{what}: {n} differs at line {k} of {len(a[n])} / {len(b[n])}:\n    A: {a[n][k:k + 1]}\n    B: {b[n][k:k + 1]}")
            bad += 1
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("tree", nargs="?", default=REPO)
    ap.add_argument("--work", default=None)
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="device_code_diff_")
    os.makedirs(work, exist_ok=True)
    jobs = []
    for side, tree in (("a", a.parent), ("b", a.tree)):
        for suffix, extra in BUILDS:
            stem = os.path.join(work, side + suffix)
            if not (os.path.exists(stem + ".s") and os.path.exists(stem + ".rem")):
                jobs.append(compile_tree(tree, stem, extra))
    for cmd, p, rem in jobs:
        rc = p.wait()
        rem.close()
        if rc != 0:
            sys.exit("failed: " + " ".join(cmd))
    total = 0
    for suffix, extra in BUILDS:
        A, B = os.path.join(work, "a" + suffix), os.path.join(work, "b" + suffix)
        ra, rb = resources(A + ".rem"), resources(B + ".rem")
        (sa, ma, xa), (sb, mb, xb) = symbols(A + ".s"), symbols(B + ".s")
        report = []
        bad = compare("resources", ra, rb, report) + compare("assembly", sa, sb, report) + compare("metadata", ma, mb, report)
        bad += compare("outside every symbol", {"-": xa}, {"-": xb}, report)
        if set(ra) != set(ma) or any(len(v) != 9 for v in ra.values()):
            report.append("resources: the remarks do not name the metadata's kernels with nine lines each")
            bad += 1
        print(f"build {' '.join(extra) or '(default)'}: {len(ra)} / {len(rb)} kernels, {len(sa)} / {len(sb)} symbols, "
              f"{sum(map(len, sa.values()))} / {sum(map(len, sb.values()))} assembly lines compared: "
              f"{'EQUAL' if not bad else '%d DIFFERENCES' % bad}")
        print("\n".join(report[:40]))
        total += bad
    print("outputs in", work)
    sys.exit(1 if total else 0)


if __name__ == "__main__":
    main()
