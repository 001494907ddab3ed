#!/usr/bin/env python3
"""Development tool: do two trees compile to the same device instructions?

    python tools/isa_same.py OTHER_TREE [--jobs J] [--keep DIR]

Takes the compile jobs of ``__graft_entry__._compile_jobs`` of this tree and of OTHER_TREE (a checkout
of another commit), runs each as ``--cuda-device-only -S`` into a scratch directory, splits the
assembly into functions, drops comments, numbers the local labels of a function by their first
appearance in it, and compares what is left (instructions, labels, the kernel descriptor) per kernel
and object.  One line per kernel: ``same``, ``DIFF`` (with both line counts and the number of differing
lines) or the tree it is missing from; exit status 1 on any difference.  Runs on the CPU
(cross-compilation only); the order of the kernels in a file and the compiler's numbering of functions
and block labels are not compared.
"""
from __future__ import annotations

import argparse
import difflib
import importlib.util
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
BEGIN = re.compile(r"; -- Begin function (\S+)")
END = re.compile(r"; -- End function")
# Lpost_getpc: the label of a relaxed (long) branch, numbered through the whole file
LABEL = re.compile(r"\.(LBB|Ltmp|Lfunc_end|Lfunc_begin|LJTI|Lpost_getpc)\d+(?:_\d+)*")


def _jobs(tree: Path, out: Path) -> dict[str, list[str]]:
    """object name -> the tree's compile command, turned into a device-only assembly job"""
    spec = importlib.util.spec_from_file_location(f"entry_{out.name}", tree / "__graft_entry__.py")
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    jobs = {}
    for cmd in entry._compile_jobs("/opt/rocm/bin/hipcc"):
        i = cmd.index("-o")
        name = Path(cmd[i + 1]).stem
        keep = [a for a in cmd[:i] + cmd[i + 2:] if a != "-c" and not a.startswith("-Rpass")]
        jobs[name] = [*keep[:-1], "--cuda-device-only", "-S", "-o", str(out / f"{name}.s"), keep[-1]]
    return jobs


def functions(text: str) -> dict[str, list[str]]:
    """function name -> its instruction and label lines, comments removed and the local labels
    numbered by first appearance within the function"""
    out, cur, seen = {}, None, {}

    def number(m):  # `seen` is looked up at each call: the dict of the function being read
        return seen.setdefault(m.group(0), f".{m.group(1)}#{len(seen)}")

    for line in text.splitlines():
        m = BEGIN.search(line)
        if m:
            cur, seen = out.setdefault(m.group(1), []), {}
        elif END.search(line):
            cur = None
        elif cur is not None:
            code = LABEL.sub(number, line.split(";", 1)[0]).strip()
            if code:
                cur.append(code)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("other", type=Path)
    ap.add_argument("--jobs", type=int, default=8, help="compilations at a time (at most 16)")
    ap.add_argument("--keep", type=Path, help="keep the assembly files in this directory")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        root = args.keep or Path(tmp)
        sides = {}
        for side, tree in (("this", HERE), ("other", args.other.resolve())):
            (root / side).mkdir(parents=True, exist_ok=True)
            sides[side] = _jobs(tree, root / side)
        cmds = [c for jobs in sides.values() for c in jobs.values()]
        with ThreadPoolExecutor(max(1, min(16, args.jobs))) as ex:
            for res in ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), cmds):
                if res.returncode != 0:
                    print(f"hipcc failed: {' '.join(res.args)}\n{res.stderr}", file=sys.stderr)
                    return 2
        bad = seen = 0
        for obj in sorted(set(sides["this"]) | set(sides["other"])):
            fa, fb = (functions((root / side / f"{obj}.s").read_text()) if obj in sides[side] else {}
                      for side in ("this", "other"))
            for name in sorted(set(fa) | set(fb)):
                verdict = ("only in the other tree" if name not in fa else "only in this tree" if name not in fb
                           else "same" if fa[name] == fb[name] else "DIFF")
                bad += verdict != "same"
                seen += 1
                if verdict == "DIFF":
                    ops = difflib.SequenceMatcher(None, fa[name], fb[name], autojunk=False).get_opcodes()
                    nd = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in ops if tag != "equal")
                    print(f"{obj}: {name}: DIFF (this {len(fa[name])} lines, other {len(fb[name])} lines, "
                          f"{nd} differ)")
                else:
                    print(f"{obj}: {name}: {verdict} ({len(fa.get(name, fb.get(name)))} lines)")
        print(f"{'DIFFERENT' if bad else 'all the same'}: {bad} of {seen} kernels differ or are missing")
        return 1 if bad or not seen else 0


if __name__ == "__main__":
    sys.exit(main())
