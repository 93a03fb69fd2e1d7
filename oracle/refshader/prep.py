"""ORACLE — TEST INFRASTRUCTURE ONLY.

prep.py — syntactic pre-pass from one of the reference's compute shaders (`*.comp.glsl`) to a C++ header that
glsl_compat.hpp can compile.  The output is written under oracle/_ref/ (git-ignored) and never committed: it is the
reference's text.  Nothing here knows what the shaders compute; the pass rewrites *syntax* only:

  * `#version` / `#extension` dropped, `#include "../common.h"` resolved (its `#ifdef __cplusplus` block dropped);
  * `layout(...) uniform T x;` -> member `T x;`, `layout(...) buffer B { T a[]; };` -> member `const T* a;`,
    push-constant / UBO blocks -> plain members, `layout(local_size...) in;` dropped;
  * `inout T x` / `out T x` parameters -> `T& x`;
  * GLSL array constructors `float[5][5](float[5](..), ..)` -> brace initialisers;
  * `float` -> `Real`, every floating literal `2.0` -> `RL(2.0)` (a literal of type Real with the literal's binary32
    value: C++ would otherwise evaluate `2.0 * x - 1.0` in double and round once, which is not the text's arithmetic);
  * `void main()` -> `void main_invocation()`; the whole text becomes the body of `struct Shader` in namespace
    glsl::<name>, so the shader's globals are members of a per-shader context.

No arithmetic expression is touched otherwise.  The only edits that are not syntax are the HOOKS below.
"""
from __future__ import annotations

import argparse
import os
import re
import sys

# (file, line, old text on that line, new text) — each defaults to the reference's behaviour.
HOOKS = [
    # segment bound: a member the host sets (default 32), so max_segments configurations can run
    ("raytrace.comp.glsl", 204, "< 32;", "< ref_max_segments;"),
    # NUM_SAMPLES: a member the host sets (default 1), so samples_per_pixel configurations can run
    ("raytrace.comp.glsl", 306, "= 1;", "= ref_num_samples;"),
    # trig argument: the numerics contract defines sincos(2 pi u) from u, not from theta = 2*k_pi*u.  The hook hands
    # u along with theta; R32 evaluates dm_sincos2pi(u), R64 evaluates cos(theta) / sin(theta) as written.
    ("raytrace.comp.glsl", 91, "cos(theta)", "rs_cos_hook(theta, u2)"),
    ("raytrace.comp.glsl", 91, "sin(theta)", "rs_sin_hook(theta, u2)"),
    ("raytrace.comp.glsl", 256, "stepAndOutputRNGFloat(rngState)", "(ref_theta_u = stepAndOutputRNGFloat(rngState))"),
    ("raytrace.comp.glsl", 259, "cos(theta)", "rs_cos_hook(theta, ref_theta_u)"),
    ("raytrace.comp.glsl", 259, "sin(theta)", "rs_sin_hook(theta, ref_theta_u)"),
]
HOOK_MEMBERS = ("  int ref_max_segments = 32;  /* hook :204 */\n  int ref_num_samples = 1;    /* hook :306 */\n"
                "  Real ref_theta_u = 0;       /* hook :256: the draw that theta is 2*k_pi times */\n")

_LIT = re.compile(r"(?<![\w.])((?:\d+\.\d*|\.\d+)(?:[eE][-+]?\d+)?|\d+[eE][-+]?\d+)([fF]?)(?![\w.])")


def _lit(m):
    return ("RLF(%s%s)" if m.group(2) else "RL(%s%s)") % (m.group(1), m.group(2))


def _outside_comments(text, fn):
    """apply fn to the code parts of text, leaving // and /* */ comments alone"""
    out, i, n = [], 0, len(text)
    while i < n:
        a, b = text.find("//", i), text.find("/*", i)
        nxt = min(x for x in (a, b, n) if x >= 0)
        out.append(fn(text[i:nxt]))
        if nxt == n:
            break
        if nxt == a and (b < 0 or a < b):
            end = text.find("\n", nxt)
            end = n if end < 0 else end
        else:
            end = text.find("*/", nxt)
            end = n if end < 0 else end + 2
        out.append(text[nxt:end])
        i = end
    return "".join(out)


def _array_ctors(code):
    """float[5][5]( ... ) / float[5]( ... ) -> { ... } with the matching parenthesis"""
    pat = re.compile(r"\bfloat(?:\[\d+\])+\(")
    while True:
        m = pat.search(code)
        if not m:
            return code
        depth, j = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(code[j], 0)
            j += 1
        code = code[:m.start()] + "{" + code[m.end():j - 1] + "}" + code[j:]


def _code(code):
    code = re.sub(r"layout\s*\([^)]*\)\s*in\s*;", "", code)
    # storage buffers: layout(...) buffer Name { T a[]; };  ->  const T* a = nullptr;
    code = re.sub(r"layout\s*\([^)]*\)\s*buffer\s+\w+\s*\{\s*(\w+)\s+(\w+)\s*\[\s*\]\s*;\s*\}\s*;",
                  r"const \1* \2 = nullptr;", code)
    # push constants: layout(push_constant) uniform Name { T x; };  ->  T x;
    code = re.sub(r"layout\s*\(\s*push_constant\s*\)\s*uniform\s+\w+\s*\{\s*(\w+\s+\w+\s*;)\s*\}\s*;", r"\1", code)
    # UBO with an instance name: layout(...) uniform Name { ... } inst;  ->  struct Name { ... } inst;
    code = re.sub(r"layout\s*\([^)]*\)\s*uniform\s+(\w+)\s*\{", r"struct \1 {", code)
    # opaque bindings: layout(...) uniform T x;  ->  T x;
    code = re.sub(r"layout\s*\([^)]*\)\s*uniform\s+(\w+\s+\w+\s*;)", r"\1", code)
    code = re.sub(r"\b(?:inout|out)\s+(\w+)\s+(\w+)", r"\1& \2", code)
    code = _array_ctors(code)
    code = re.sub(r"\bfloat\b", "Real", code)
    code = re.sub(r"\bvoid\s+main\s*\(\s*\)", "void main_invocation()", code)
    return _LIT.sub(_lit, code)


def translate(shader_path: str, name: str, mutations=()) -> str:
    base = os.path.basename(shader_path)
    lines = open(shader_path, encoding="utf-8", errors="replace").read().split("\n")
    edits = [h for h in HOOKS if h[0] == base] + [(base, int(ln), o, n) for (ln, o, n) in mutations]
    for _, ln, old, new in edits:
        if old not in lines[ln - 1]:
            raise SystemExit(f"prep.py: {base}:{ln} does not contain {old!r}: the hook table no longer matches the reference")
        lines[ln - 1] = lines[ln - 1].replace(old, new)
    macros, body = [], []
    for line in lines:
        s = line.strip()
        if s.startswith("#version") or s.startswith("#extension"):
            continue
        m = re.match(r'#include\s+"([^"]+)"', s)
        if m:
            inc = os.path.normpath(os.path.join(os.path.dirname(shader_path), m.group(1)))
            skip = 0
            for il in open(inc, encoding="utf-8", errors="replace").read().split("\n"):
                t = il.strip()
                if t.startswith("#ifdef __cplusplus"):
                    skip = 1
                elif skip and t.startswith("#endif"):
                    skip = 0
                elif not skip and t.startswith("#define") and len(t.split("//")[0].split()) >= 3:
                    macros.append(_outside_comments(il, _code))  # object-like macros with a value only
            continue
        body.append(line)
    text = _outside_comments("\n".join(body), _code)
    undef = "".join("#undef %s\n" % mm.split()[1] for mm in macros)
    return (f"// GENERATED by oracle/refshader/prep.py from the reference's {base} — never commit this file.\n"
            + "\n".join(macros) + f"\nnamespace glsl {{ namespace {name} {{\n"
            "enum { WG_W = WORKGROUP_WIDTH, WG_H = WORKGROUP_HEIGHT };\n"
            "struct Shader {\n  uvec3 gl_GlobalInvocationID;\n" + HOOK_MEMBERS + text + "\n};\n}}\n" + undef)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("shader")
    ap.add_argument("name", help="namespace of the generated Shader struct")
    ap.add_argument("-o", "--output", required=True)
    ap.add_argument("--mutate", action="append", default=[], metavar="LINE:OLD:NEW",
                    help="tests only: alter one piece of text on the way through (the host must then be seen to disagree)")
    a = ap.parse_args(argv)
    muts = [tuple(m.split(":", 2)) for m in a.mutate]
    out = translate(a.shader, a.name, muts)
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    with open(a.output, "w", encoding="utf-8") as f:
        f.write(out)


if __name__ == "__main__":
    sys.exit(main())
