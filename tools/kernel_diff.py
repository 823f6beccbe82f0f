#!/usr/bin/env python3
"""kernel_diff.py OLD_TREE NEW_TREE [NAME.hip ...]: is the device code the same, kernel by kernel?

Compiles every lesion_gnn_amd/csrc/*.hip of both trees for the device only, with the Makefile's
HIPFLAGS, and compares per symbol the disassembled instruction text (addresses and encodings
dropped) and the kernel metadata (registers, LDS, scratch, workgroup size). Prints one summary
line per file and a total; exits 1 on any difference. Two compilations of one file differ in their
ELF bytes but not in this text. The trees are only read; objects go to a temporary directory.
A symbol's text runs to the next symbol, alignment padding included, and a code object lists its
kernels in the order the host code first uses them: a change of that order shows up as a text
difference of the kernels whose successor changed (compare the bodies before reading more into it).
Optional file names after the two trees restrict the comparison to those files.
"""
import concurrent.futures as cf
import pathlib
import re
import subprocess
import sys
import tempfile

LLVM = pathlib.Path("/opt/rocm/llvm/bin")
CSRC = "lesion_gnn_amd/csrc"


def hipflags(tree):
    mk = (pathlib.Path(tree) / "Makefile").read_text()
    flags = re.search(r"^HIPFLAGS \?= (.*)$", mk, re.M).group(1)
    arch = re.search(r"^ARCH \?= (.*)$", mk, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def kernels(tree, name, tmp):
    """{symbol: instruction text}, {symbol: metadata text} of one file's device code"""
    obj = pathlib.Path(tmp) / f"{abs(hash(str(tree)))}_{name}.o"
    subprocess.run(["/opt/rocm/bin/hipcc", *hipflags(tree), "--offload-device-only",
                    "--no-gpu-bundle-output", "-c", str(pathlib.Path(tree) / CSRC / name),
                    "-o", str(obj)], check=True, capture_output=True)
    run = lambda *c: subprocess.run(c, check=True, capture_output=True, text=True).stdout
    code, sym = {}, None
    for line in run(str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", str(obj)).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            sym = m.group(1)
            code[sym] = []
        elif sym and line.strip() and not line.startswith("Disassembly"):
            # drop the address column and the "// 0000AB: ENCODING" comment
            code[sym].append(re.sub(r"\s*//.*$", "", re.sub(r"^\s*[0-9a-f]+:\s*", "", line)).strip())
    meta = {}
    notes = run(str(LLVM / "llvm-readelf"), "--notes", str(obj))
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        block = ".agpr_count:" + block
        name_ = re.search(r"\.name:\s+(\S+)", block).group(1)
        keep = re.findall(r"\.(agpr_count|vgpr_count|sgpr_count|group_segment_fixed_size|"
                          r"private_segment_fixed_size|max_flat_workgroup_size|"
                          r"reqd_workgroup_size|sgpr_spill_count|vgpr_spill_count|"
                          r"kernarg_segment_size|wavefront_size):\s+(\S+)", block)
        meta[name_] = sorted(keep)
    return {s: "\n".join(t) for s, t in code.items()}, meta


def main(old, new, *only):
    names = sorted({p.name for t in (old, new) for p in (pathlib.Path(t) / CSRC).glob("*.hip")})
    names = [n for n in names if not only or n in only]
    bad = files = syms = 0
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(16) as ex:
        exists = lambda t, n: (pathlib.Path(t) / CSRC / n).exists()
        jobs = {(t, n): ex.submit(kernels, t, n, tmp) for t in (old, new) for n in names
                if exists(t, n)}
        for n in names:
            if not (exists(old, n) and exists(new, n)):
                print(f"{n}: only in {'OLD' if exists(old, n) else 'NEW'}")
                bad += 1
                continue
            (co, mo), (cn, mn) = jobs[old, n].result(), jobs[new, n].result()
            only_one = sorted(set(co) ^ set(cn))
            text = sorted(s for s in set(co) & set(cn) if co[s] != cn[s])
            metad = sorted(s for s in set(mo) | set(mn) if mo.get(s) != mn.get(s))
            print(f"{n}: {len(set(co) & set(cn))} symbols, {len(mn)} kernels; one side only "
                  f"{len(only_one)}, text differs {len(text)}, metadata differs {len(metad)}")
            for kind, lst in (("one side only", only_one), ("text", text), ("metadata", metad)):
                for s in lst:
                    print(f"    {kind}: {s}")
            bad += len(only_one) + len(text) + len(metad)
            files += 1
            syms += len(set(co) & set(cn))
    print(f"TOTAL: {files} files, {syms} symbols compared, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    sys.exit(main(*sys.argv[1:]))
