#!/usr/bin/env python3
"""Copy the function bodies the bridge needs out of the reference tree.

Renderer.cpp and Scene.cpp cannot be compiled whole on a host (kernel launch
syntax, Assimp), so the definitions listed below are copied, unchanged, into
``<out>/renderer_device.inc`` and ``<out>/scene_grid.inc``.  Each one is found
by its signature and cut at its matching closing brace; a signature that is
missing, or found twice, stops the build.  The output directory is a build
directory (oracle/_ref/): the copies are never committed.

usage: extract.py <reference PathTracerAP directory> <output directory>
"""
import os
import re
import sys

QUALIFIERS = re.compile(r"^\s*(?:(?:__inline__|__forceinline__|__host__|__device__|__global__|inline|static)\s*)+$")

# (kind, name): "fn" is a free or member function definition, "struct" a struct.
RENDERER = [
    ("fn", "computeRayBoundingBoxIntersection"),
    ("fn", "computeRayTriangleIntersection"),
    ("fn", "computeRayVoxelIntersection"),
    ("fn", "computeRayGridIntersection"),
    ("fn", "computeRaySceneIntersectionKernel"),
    ("fn", "shadeRayKernel"),
    ("fn", "gatherImageDataKernel"),
    ("struct", "hasTerminated"),
    ("fn", "compactStencilKernel"),
    ("fn", "generateRaysKernel"),
    ("fn", "initImageKernel"),
]
SCENE = [
    ("fn", "computeVoxelIndex"),
    ("fn", "Scene::addMeshesToGrid"),
]


def strip_comments(line, in_block):
    """The line with // and /* */ comments and string literals blanked, for brace counting."""
    out = []
    i = 0
    while i < len(line):
        if in_block:
            j = line.find("*/", i)
            if j < 0:
                return "".join(out), True
            i = j + 2
            in_block = False
        elif line.startswith("//", i):
            break
        elif line.startswith("/*", i):
            in_block = True
            i += 2
        elif line[i] in "\"'":
            q = line[i]
            i += 1
            while i < len(line) and line[i] != q:
                i += 2 if line[i] == "\\" else 1
            i += 1
        else:
            out.append(line[i])
            i += 1
    return "".join(out), in_block


def find_definition(lines, kind, name, path):
    if kind == "struct":
        pat = re.compile(r"^\s*struct\s+" + re.escape(name) + r"\b(?!\s*;)")
    else:
        # a return type, the name, an opening parenthesis, and no ';' on the line:
        # a definition's first line, not a call and not a declaration
        pat = re.compile(r"^\s*(?:[\w:<>\*&]+\s+)*(?:void|bool|int|float)\s+" + re.escape(name) + r"\s*\([^;]*$")
    hits = [i for i, l in enumerate(lines) if pat.match(l)]
    if len(hits) != 1:
        sys.exit(f"extract.py: expected exactly one definition of '{name}' in {path}, found {len(hits)}")
    start = hits[0]
    while start > 0 and QUALIFIERS.match(lines[start - 1]):
        start -= 1
    depth = 0
    seen = False
    in_block = False
    for end in range(hits[0], len(lines)):
        code, in_block = strip_comments(lines[end], in_block)
        for ch in code:
            if ch == "{":
                depth += 1
                seen = True
            elif ch == "}":
                depth -= 1
        if seen and depth == 0:
            return lines[start:end + 1]
    sys.exit(f"extract.py: no closing brace for '{name}' in {path}")


def extract(src, wanted, dst):
    if not os.path.isfile(src):
        sys.exit(f"extract.py: {src} not found")
    with open(src, "r", encoding="utf-8", errors="replace") as f:
        lines = f.read().splitlines()
    out = [f"// Generated at build time from {os.path.basename(src)}; do not commit.", ""]
    for kind, name in wanted:
        out += find_definition(lines, kind, name, src)
        out.append("")
    with open(dst, "w", encoding="utf-8") as f:
        f.write("\n".join(out))


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    ref, out = sys.argv[1], sys.argv[2]
    os.makedirs(out, exist_ok=True)
    extract(os.path.join(ref, "Renderer.cpp"), RENDERER, os.path.join(out, "renderer_device.inc"))
    extract(os.path.join(ref, "Scene.cpp"), SCENE, os.path.join(out, "scene_grid.inc"))


if __name__ == "__main__":
    main()
