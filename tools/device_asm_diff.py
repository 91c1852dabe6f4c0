#!/usr/bin/env python3
"""Compare the gfx950 device assembly of every csrc/*.hip between two source trees.

    tools/device_asm_diff.py BASE NEW [--files mlp_x3.hip ...] [--json OUT] [--jobs N]

BASE and NEW are each a checkout's root directory or a git revision of this repository (exported to
a temporary directory).  Every `code-nerf_amd/csrc/*.hip` of both is compiled with the Makefile's
flags plus `--cuda-device-only -S`, the text is normalised (comments dropped, the `__hip_cuid_*`
symbol masked, local labels renumbered in order of appearance per function) and compared: per file
the number of kernels, a hash of the normalised text on each side and, on a mismatch, the kernels
whose text, descriptor (`.amdhsa_*`, resource `.set`s) or metadata entry differs.

It compares two builds and looks for nothing in particular in either.  CPU only; exit status 1 on
any difference.
"""
from __future__ import annotations

import argparse
import concurrent.futures
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("code-nerf_amd", "csrc")
MAX_JOBS = 16


def makefile_flags(csrc: str) -> tuple[str, list[str]]:
    """(hipcc, flags) as csrc/Makefile's object rule uses them (no CXXFLAGS_EXTRA)."""
    text = open(os.path.join(csrc, "Makefile")).read()
    var = {k: v.strip() for k, v in re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}
    flags = re.sub(r"\$\((\w+)\)", lambda m: "" if m.group(1) == "CXXFLAGS_EXTRA" else var.get(m.group(1), ""),
                   var["CXXFLAGS"])
    return os.environ.get("HIPCC", var.get("HIPCC", "hipcc")), flags.split()


def export(rev: str, into: str) -> str:
    """`git archive` of rev's csrc/ and include/ under `into`; returns the exported root."""
    root = os.path.join(into, re.sub(r"\W", "_", rev))
    os.makedirs(root)
    ar = subprocess.run(["git", "-C", REPO, "archive", rev, "code-nerf_amd/csrc", "include"], check=True,
                        capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", root], input=ar, check=True)
    return root


def compile_one(hipcc: str, flags: list[str], csrc: str, name: str, out_dir: str, stub: str, reuse: bool = False) -> str:
    out = os.path.join(out_dir, name + ".s")
    if reuse and os.path.exists(out):
        return out
    # relative source name from csrc/ so that .file is the same text on both sides; `stub` holds a
    # constant cn_build_info.h (abi.hip's generated header: host strings only)
    cmd = [hipcc, *flags, "-I" + stub, "--cuda-device-only", "-S", name, "-o", out]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} (in {csrc}) failed:\n{r.stderr}")
    return out


_LABEL = re.compile(r"\.L[A-Za-z_$][\w$.]*|\.LBB\d+_\d+|\bBB\d+_\d+")
_CUID = re.compile(r"__hip_cuid_[0-9a-f]+")


def normalise(text: str) -> dict:
    """Normalised text plus, per function, its body, and per kernel its descriptor and metadata."""
    lines, funcs, desc, meta = [], {}, {}, {}
    cur, labels, in_desc, in_meta = None, {}, None, False
    meta_item: list[str] = []

    def flush_meta():
        if meta_item:
            m = re.search(r"^\s+\.name:\s+(\S+)", "\n".join(meta_item), re.M)
            if m:
                meta[m.group(1)] = "\n".join(meta_item)

    for raw in text.splitlines():
        line = raw if '"' in raw else raw.split(";", 1)[0]
        line = _CUID.sub("__hip_cuid_X", line.rstrip())
        if not line.strip():
            continue
        if line.strip() == ".amdgpu_metadata":
            in_meta = True
        elif line.strip() == ".end_amdgpu_metadata":
            flush_meta()
            in_meta = False
        if in_meta:
            if line.startswith("  - "):
                flush_meta()
                meta_item = []
            meta_item.append(line)
            lines.append(line)
            continue
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur, labels = m.group(1), {}
            funcs[cur] = []
        if cur is not None:
            line = _LABEL.sub(lambda k: labels.setdefault(k.group(0).replace(".L", ""), f".L{len(labels)}"), line)
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            in_desc = m.group(1)
            desc[in_desc] = []
        if in_desc is not None:
            desc[in_desc].append(line)
            if line.strip() == ".end_amdhsa_kernel":
                in_desc = None
        elif cur is not None:
            m = re.match(r"\s*\.set\s+(\S+)\.\w+,", line)
            if m and m.group(1) == cur:
                desc.setdefault(cur, []).append(line)
            elif not line.lstrip().startswith(".section"):
                funcs[cur].append(line)
        lines.append(line)
        if cur is not None and re.match(r"\s*\.set\s+" + re.escape(cur) + r"\.has_indirect_call,", line):
            cur = None
    return {"text": "\n".join(lines), "funcs": {k: "\n".join(v) for k, v in funcs.items()},
            "desc": {k: "\n".join(v) for k, v in desc.items()}, "meta": meta}


def sha(s: str) -> str:
    return hashlib.sha256(s.encode()).hexdigest()[:16]


def compare(name: str, a: dict, b: dict) -> dict:
    kernels_a = sorted(k for k in a["desc"] if ".amdhsa_kernel" in a["desc"][k])
    kernels_b = sorted(k for k in b["desc"] if ".amdhsa_kernel" in b["desc"][k])
    rec = {"file": name, "kernels": [len(kernels_a), len(kernels_b)], "hash": [sha(a["text"]), sha(b["text"])]}
    rec["identical"] = rec["hash"][0] == rec["hash"][1]
    if not rec["identical"]:
        diff = {}
        for k in sorted(set(a["funcs"]) | set(b["funcs"])):
            what = []
            if k not in a["funcs"] or k not in b["funcs"]:
                what.append("only in " + ("base" if k in a["funcs"] else "new"))
            else:
                if a["funcs"][k] != b["funcs"][k]:
                    what.append("text")
                if a["desc"].get(k) != b["desc"].get(k):
                    what.append("descriptor")
                if a["meta"].get(k) != b["meta"].get(k):
                    what.append("metadata")
            if what:
                diff[k] = what
        rec["differs"] = diff
    return rec


def hipcc_version(hipcc: str) -> str:
    out = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout
    return " | ".join(l.strip() for l in out.splitlines()[:2])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("base", help="source tree root or git revision")
    ap.add_argument("new", help="source tree root or git revision")
    ap.add_argument("--files", nargs="*", help="only these csrc/*.hip (default: all of both trees)")
    ap.add_argument("--jobs", type=int, default=min(MAX_JOBS, os.cpu_count() or 1))
    ap.add_argument("--json", help="write the report here")
    ap.add_argument("--keep", help="keep the .s files under this directory")
    ap.add_argument("--reuse-base", action="store_true", help="with --keep: do not recompile a base .s already there")
    args = ap.parse_args()
    jobs = max(1, min(MAX_JOBS, args.jobs))

    with tempfile.TemporaryDirectory(prefix="device_asm_") as tmp:
        work = args.keep or tmp
        stub = os.path.join(tmp, "stub")
        os.makedirs(stub)
        with open(os.path.join(stub, "cn_build_info.h"), "w") as f:
            f.write('#define CN_SRC_HASH "0"\n#define CN_GIT_HEAD "0"\n')
        sides = []
        for tag, spec in (("base", args.base), ("new", args.new)):
            root = os.path.abspath(spec) if os.path.isdir(spec) else export(spec, tmp)
            csrc = os.path.join(root, CSRC)
            names = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
            out_dir = os.path.join(work, tag)
            os.makedirs(out_dir, exist_ok=True)
            sides.append((csrc, names, out_dir, makefile_flags(csrc)))
        names = sorted(set(sides[0][1]) | set(sides[1][1]))
        if args.files:
            names = [n for n in names if n in args.files]
        asm = [{}, {}]
        with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
            futs = {}
            for i, (csrc, have, out_dir, (hipcc, flags)) in enumerate(sides):
                for n in names:
                    if n in have:
                        futs[pool.submit(compile_one, hipcc, flags, csrc, n, out_dir, stub,
                                         args.reuse_base and i == 0)] = (i, n)
            for fut in concurrent.futures.as_completed(futs):
                i, n = futs[fut]
                asm[i][n] = normalise(open(fut.result()).read())
        report = {"base": args.base, "new": args.new, "hipcc": hipcc_version(sides[1][3][0]),
                  "flags": " ".join(sides[1][3][1]) + " --cuda-device-only -S", "files": []}
        for n in names:
            if n not in asm[0] or n not in asm[1]:
                report["files"].append({"file": n, "identical": False,
                                        "differs": "only in " + ("base" if n in asm[0] else "new")})
            else:
                report["files"].append(compare(n, asm[0][n], asm[1][n]))
    report["identical"] = all(f["identical"] for f in report["files"])
    for f in report["files"]:
        print(f"{f['file']:18s} kernels {f.get('kernels')}  {' '.join(f.get('hash', []))}  "
              + ("identical" if f["identical"] else "DIFFERENT"))
        if not f["identical"]:
            diff = f["differs"]
            for k, what in (diff.items() if isinstance(diff, dict) else [(diff, [])]):
                print(f"    {k}: {', '.join(what)}")
    print("all identical" if report["identical"] else "DIFFERENCES FOUND")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 0 if report["identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
