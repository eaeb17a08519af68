#!/usr/bin/env python3
"""Offline (no GPU): is the device code of two trees the same, kernel by kernel?  Every source of builder.SOURCES is
compiled with its own unit's flags plus `--cuda-device-only -S` (each tree's own builder.py says which sources and which
flags), and per unit the kernels (`.amdhsa_kernel` names) are compared: the set of them, each one's instruction text and
its `.amdhsa_*` block, after dropping comments, `.file` / `.ident` lines and the unit id the compiler derives from the
source's path.  A tree is a git revision or a directory.

Usage: compare_device_code.py <tree A> <tree B>     (e.g. HEAD~1 .)        exit status 1 when anything differs"""
import concurrent.futures
import importlib.util
import os
import re
import subprocess
import sys
import tempfile


def checkout(tree, into):
    if os.path.isdir(tree):
        return os.path.abspath(tree)
    os.makedirs(into)
    archive = subprocess.run(["git", "archive", tree, "codecad_amd/csrc", "codecad_amd/hip_util/builder.py", "include"],
                             check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", into], input=archive, check=True)
    return into


def load_builder(root):
    spec = importlib.util.spec_from_file_location("builder_of_" + re.sub(r"\W", "_", root), os.path.join(root, "codecad_amd", "hip_util", "builder.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def normalised(text):
    lines = []
    for line in text.split("\n"):
        line = line.split(";")[0].rstrip()
        if not line or re.match(r"\s*\.(file|ident)\b", line):
            continue
        lines.append(re.sub(r"(__hip_cuid_|\.(?:intern|static|anon)\.)[0-9a-f]+", r"\1", line))
    return lines


def kernels_of(text):
    """{kernel: its instructions and its descriptor}, and the unit's other lines (device functions, tables, metadata)"""
    lines = normalised(text)
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel (\S+)", line) for line in lines) if m]
    found, rest, current, end = {n: [] for n in names}, [], None, None
    for line in lines:
        label = re.match(r"(\S+):$", line)
        descriptor = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
        if current is None and label and label.group(1) in found:
            current, end = label.group(1), r"\.Lfunc_end\d+:$"
        elif current is None and descriptor:
            current, end = descriptor.group(1), r"\s*\.end_amdhsa_kernel$"
        (found[current] if current else rest).append(line)
        if current and re.match(end, line):
            current = None
    return found, rest


def assembly(root, builder, source, out_dir):
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"] + (builder.INTERPRETER_FLAGS if source in builder.FLAGGED_SOURCES else [])
    out = os.path.join(out_dir, source + ".s")
    subprocess.run([builder.find_hipcc()] + flags + ["-I", os.path.join(root, "include"), "--cuda-device-only", "-S", "-o", out,
                                                     os.path.join(root, "codecad_amd", "csrc", source)], check=True, capture_output=True)
    return kernels_of(open(out).read())


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        roots = [checkout(tree, os.path.join(tmp, "tree%d" % i)) for i, tree in enumerate(sys.argv[1:])]
        builders = [load_builder(root) for root in roots]
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            jobs = []
            for i, (root, builder) in enumerate(zip(roots, builders)):
                out_dir = os.path.join(tmp, "asm%d" % i)
                os.makedirs(out_dir)
                jobs.append({s: pool.submit(assembly, root, builder, s, out_dir) for s in builder.SOURCES})
            units = [{s: job.result() for s, job in side.items()} for side in jobs]
    different = False
    for source in sorted(set(units[0]) | set(units[1])):
        if source not in units[0] or source not in units[1]:
            only = units[0].get(source) or units[1].get(source)
            where = "A" if source in units[0] else "B"
            print("%-22s only in %s, %d kernels%s" % (source, where, len(only[0]), "" if not only[0] else ": " + " ".join(sorted(only[0]))))
            different = different or bool(only[0])
            continue
        (ka, rest_a), (kb, rest_b) = units[0][source], units[1][source]
        notes = ["kernel only in A: " + k for k in sorted(set(ka) - set(kb))] + ["kernel only in B: " + k for k in sorted(set(kb) - set(ka))]
        notes += ["kernel differs: " + k for k in sorted(set(ka) & set(kb)) if ka[k] != kb[k]]
        if rest_a != rest_b:
            notes.append("lines outside the kernels differ (device functions, tables, metadata)")
        print("%-22s %d kernels, %s" % (source, len(ka), "identical" if not notes else "DIFFERENT"))
        for note in notes:
            print("    " + note)
        different = different or bool(notes)
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())
