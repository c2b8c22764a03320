#!/usr/bin/env python3
"""Do two checkouts compile the same gfx950 machine code?  CPU only.

    tools/isa_diff.py PARENT_TREE THIS_TREE [--files a.hip b.hip ...] [--rename REGEX=REPL ...] [--report FILE]

For each checkout the given csrc/*.hip files (default: the decoder's three) are compiled to device assembly with the flags of THAT
checkout's thewhisper_amd/build.py for the file - the command build_library would run, plus `-S --cuda-device-only`.  The listing is
split per kernel symbol (every symbol with a kernel descriptor), names are demangled, a --rename (a regular expression applied to
the FIRST tree's demangled names: kernels whose name or template arguments changed) is applied, and the instruction text and the
kernel descriptor block (.amdhsa_* lines: registers, LDS, scratch, kernarg size and preload) are compared as text, with comments
removed and local labels (.LBB12_3, .Ltmp5, .Lfunc_end12) renumbered per kernel by first appearance.  One report line per kernel; exit status 1 on any
difference and on a kernel that only one side has.  The tool compares text: it knows nothing about individual instructions.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Tuple

DEFAULT_FILES = ["k_decode.hip", "k_decode_kv8_rows.hip", "k_decode_kv8_beams.hip", "k_decode_beam_cross.hip"]
_LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?\b")


def _load_build(tree: str):
    path = os.path.join(tree, "thewhisper_amd", "build.py")
    spec = importlib.util.spec_from_file_location("tw_build_" + str(abs(hash(path))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_asm(tree: str, name: str, outdir: str) -> str:
    b = _load_build(tree)
    src = os.path.join(b.CSRC, name)
    out = os.path.join(outdir, name.replace(".hip", ".s"))
    cmd = [b._hipcc(), *b.FLAGS, *b.FILE_FLAGS.get(name, []), "-c", src, "-o", out, "-S", "--cuda-device-only"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
    with open(out) as f:
        return f.read()


def demangle(names: List[str], need: bool = False) -> Dict[str, str]:
    if not names:
        return {}
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        if need:
            raise RuntimeError("--rename is written against demangled names, and neither llvm-cxxfilt nor c++filt was found")
        return {n: n for n in names}
    # binutils' c++filt predates the manglings of __bf16 and _Float16: they go through as two other builtin types
    # (builtin types are no substitution candidates, so the rest of the name is unaffected) and get their names back afterwards
    text = "\n".join(names).replace("DF16b", "Dd").replace("DF16_", "De") + "\n"
    r = subprocess.run([tool], input=text, capture_output=True, text=True, check=True)
    shown = r.stdout.replace("decimal64", "__bf16").replace("decimal128", "_Float16").splitlines()
    if len(shown) != len(names):
        raise RuntimeError(f"{tool} gave {len(shown)} lines for {len(names)} names")
    return dict(zip(names, shown))


def _clean(lines: List[str], sym: str) -> List[str]:
    """comments and blank lines out, the symbol's own name -> <self>, local labels renumbered by first appearance"""
    seen: Dict[str, str] = {}
    out = []
    for line in lines:
        line = line.split(";", 1)[0].split("//", 1)[0].strip().replace(sym, "<self>")
        if line:
            out.append(_LABEL.sub(lambda m: seen.setdefault(m.group(0), f".L{len(seen)}"), line))
    return out


def split_kernels(asm: str) -> Dict[str, Tuple[List[str], List[str]]]:
    """mangled symbol -> (instruction text, descriptor block), both normalised"""
    lines = asm.splitlines()
    out: Dict[str, Tuple[List[str], List[str]]] = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        sym = m.group(1)
        j = next((k for k in range(i + 1, len(lines)) if lines[k].strip().startswith(".end_amdhsa_kernel")), None)
        if j is None:
            raise RuntimeError(f"listing ends inside the descriptor of {sym}")
        start = next((k for k, l in enumerate(lines) if l.startswith(sym + ":")), None)
        if start is None:
            raise RuntimeError(f"{sym} has a descriptor and no body")
        end = next((k for k in range(start, len(lines)) if re.match(r"\s*\.size\s+" + re.escape(sym) + r"\s*,", lines[k])), None)
        if end is None:
            raise RuntimeError(f"the body of {sym} has no .size line")
        out[sym] = (_clean(lines[start + 1:end], sym), _clean(lines[i + 1:j], sym))
    return out


def kernels_of(tree: str, files: List[str], outdir: str, renames: List[Tuple[re.Pattern, str]]):
    res: Dict[str, Tuple[str, List[str], List[str]]] = {}
    with ThreadPoolExecutor(max_workers=len(files)) as ex:
        listings = list(ex.map(lambda n: compile_asm(tree, n, outdir), files))
    for name, asm in zip(files, listings):
        ks = split_kernels(asm)
        dm = demangle(list(ks), need=bool(renames))
        for sym, (text, dsc) in ks.items():
            shown = dm[sym]
            for pat, repl in renames:
                shown = pat.sub(repl, shown)
            key = f"{name}: {shown}"
            if key in res:
                raise RuntimeError(f"two kernels of {tree} read {key!r} (rename map?)")
            res[key] = (sym, text, dsc)
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--files", nargs="+", default=DEFAULT_FILES)
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL",
                    help="applied to the demangled kernel names of the first tree")
    ap.add_argument("--report", help="write the per-kernel lines here as well")
    a = ap.parse_args()
    renames = []
    for r in a.rename:
        pat, _, repl = r.partition("=")
        renames.append((re.compile(pat), repl))
    with tempfile.TemporaryDirectory() as t0, tempfile.TemporaryDirectory() as t1:
        with ThreadPoolExecutor(max_workers=2) as ex:
            fo = ex.submit(kernels_of, os.path.abspath(a.parent), a.files, t0, renames)
            fn = ex.submit(kernels_of, os.path.abspath(a.this), a.files, t1, [])
            old, new = fo.result(), fn.result()
    rows, bad = [], 0
    for key in sorted(set(old) | set(new)):
        if key not in new:
            rows.append(f"ONLY-FIRST   {key}")
        elif key not in old:
            rows.append(f"ONLY-SECOND  {key}")
        else:
            same_t, same_d = old[key][1] == new[key][1], old[key][2] == new[key][2]
            if same_t and same_d:
                rows.append(f"identical    {key}  ({len(new[key][1])} lines)")
                continue
            rows.append(f"DIFFERENT    {key}  (text {'same' if same_t else 'differs'}, descriptor {'same' if same_d else 'differs'})")
        bad += 1
    rows.append(f"# {len(rows) - bad} identical, {bad} different or one-sided; files: {' '.join(a.files)}")
    report = "\n".join(rows) + "\n"
    sys.stdout.write(report)
    if a.report:
        with open(a.report, "w") as f:
            f.write(report)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
