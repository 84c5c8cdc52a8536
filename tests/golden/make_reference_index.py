"""Regenerate tests/golden/reference_index.json, the index tests/test_citations.py resolves the
repository's `src/<file>:<lines>` citations against:

    python tests/golden/make_reference_index.py <reference checkout>/src

It holds no reference text: per reference file its line count and, for every function name the
reference defines, the numbers of the lines that name appears on; plus the lists of function and
class names."""
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_index.json")
VENDORED = ("tinyexr", "tinyxml2", "happly")


def read_lines(path):
    with open(path, errors="replace") as f:
        lines = f.read().split("\n")
    return lines[:-1] if lines and lines[-1] == "" else lines


def main(ref):
    names = sorted(f for f in os.listdir(ref) if f.endswith((".cpp", ".h")))
    text = {f: read_lines(os.path.join(ref, f)) for f in names}
    # a definition line: a name, a parameter list and no `;`
    defs, classes = set(), set()
    for f in names:
        if f.startswith(VENDORED):
            continue
        for line in text[f]:
            m = re.match(r"^\s*(?:[\w:<>\*&]+\s+)*?(?:\w+::)?([A-Za-z_]\w*)\s*\([^;]*$", line)
            if m and not re.match(r"^\s*(if|for|while|switch|return|else)\b", line):
                defs.add(m.group(1))
            classes |= set(re.findall(r"(?:class|struct)\s+([A-Za-z_]\w*)", line))
    files = {}
    for f in names:
        seen = {}
        for ln, line in enumerate(text[f], 1):
            for w in set(re.findall(r"\b[A-Za-z_]\w*\b", line)):
                if w in defs:
                    seen.setdefault(w, []).append(ln)
        files[f] = {"lines": len(text[f]), "symbols": {w: seen[w] for w in sorted(seen)}}
    with open(OUT, "w") as fh:
        json.dump({"defs": sorted(defs), "classes": sorted(classes), "files": files}, fh, separators=(",", ":"))
        fh.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes,", len(names), "files,", len(defs), "function names")


if __name__ == "__main__":
    main(sys.argv[1])
