#!/usr/bin/env python3
"""ChomboFortran (.ChF) to fixed-form Fortran 77/90, for CH_SPACEDIM == 3.

TEST INFRASTRUCTURE ONLY.  The reference's kernels are ChomboFortran, which
Chombo's own preprocessor turns into Fortran.  This is a small stand-in for
that preprocessor, written from the macro semantics Chombo documents (the
"ChomboFortran" chapter of the Chombo design document), covering what the
reference's two .ChF files use:

  argument lists   CHF_FRA CHF_CONST_FRA CHF_FRA1 CHF_CONST_FRA1 CHF_BOX
                   CHF_CONST_REAL CHF_REAL CHF_CONST_INT CHF_INT
  bodies           CHF_DDECL CHF_NCOMP CHF_LBOUND CHF_UBOUND CHF_DTERM CHF_IX
                   CHF_MULTIDO CHF_ENDDO CHF_ID CHF_AUTODECL CHF_AUTOMULTIDO
                   CHF_AUTOIX CHF_OFFSETIX
  C preprocessor   #if / #elif / #else / #endif on CH_SPACEDIM, #include
                   (dropped), D_TERM, REAL_T, CH_SPACEDIM and the CONSTANTS.H
                   names (zero, one, two, half, ...)

The generated C ABI is Chombo's: every dummy argument by reference, and
  CHF_FRA[x]   -> x, ixlo0, ixlo1, ixlo2, ixhi0, ixhi1, ixhi2, nxcomp
  CHF_FRA1[x]  -> the same without nxcomp
  CHF_BOX[b]   -> iblo0, iblo1, iblo2, ibhi0, ibhi1, ibhi2
so include/mgic_chf.h describes the compiled objects too.  MAYDAYERROR stays
an external call (the C side supplies maydayerror_).

A macro may span fixed-form continuation lines, so every logical statement
is joined first, expanded, and wrapped again at column 72; no compiler flag
for long lines is needed.

usage: chf2f.py input.ChF output.f
"""
from __future__ import annotations

import re
import sys

SPACEDIM = 3

# CONSTANTS.H: named double-precision literals
CONSTANTS = {
    "zero": "0.0d0", "one": "1.0d0", "two": "2.0d0", "three": "3.0d0", "four": "4.0d0",
    "five": "5.0d0", "six": "6.0d0", "seven": "7.0d0", "eight": "8.0d0", "nine": "9.0d0",
    "ten": "10.0d0", "twelve": "12.0d0", "fifteen": "15.0d0", "sixteen": "16.0d0",
    "twenty": "20.0d0", "tenth": "0.100d0", "eighth": "0.125d0", "sixth": "(1.0d0/6.0d0)",
    "fifth": "0.200d0", "fourth": "0.250d0", "third": "(1.0d0/3.0d0)", "half": "0.500d0",
    "two3rd": "(2.0d0/3.0d0)", "three4th": "0.750d0", "hundred": "100.0d0",
    "Pi": "3.14159265358979323846264338327950288d0",
}


class ChFError(Exception):
    pass


# ------------------------------------------------------------------ C preprocessor
def _cond(expr: str) -> bool:
    e = re.sub(r"\bCH_SPACEDIM\b", str(SPACEDIM), expr)
    e = re.sub(r"\bdefined\s*\(?\s*\w+\s*\)?", "0", e)
    e = e.replace("&&", " and ").replace("||", " or ")
    e = re.sub(r"!(?!=)", " not ", e)
    if not re.fullmatch(r"[\d\s<>=!()a-z]*", e):
        raise ChFError(f"cannot evaluate '#if {expr}'")
    return bool(eval(e, {"__builtins__": {}}, {}))  # digits, comparisons, and/or/not only


def preprocess(lines):
    """Resolve #if/#elif/#else/#endif, drop #include; yields kept lines."""
    stack = []  # [taking now, any branch taken yet, enclosing taking]
    for ln in lines:
        s = ln.strip()
        if s.startswith("#"):
            d = s[1:].strip()
            outer = all(f[0] for f in stack)
            if d.startswith("if"):
                if d.startswith("ifdef") or d.startswith("ifndef"):
                    take = d.startswith("ifndef")  # nothing is defined here
                else:
                    take = _cond(d[2:])
                stack.append([take, take, outer])
            elif d.startswith("elif"):
                f = stack[-1]
                take = (not f[1]) and _cond(d[4:])
                f[0], f[1] = take, f[1] or take
            elif d.startswith("else"):
                f = stack[-1]
                f[0], f[1] = not f[1], True
            elif d.startswith("endif"):
                stack.pop()
            elif d.startswith("include"):
                pass
            else:
                raise ChFError(f"unsupported directive: {s}")
            continue
        if all(f[0] for f in stack):
            yield ln
    if stack:
        raise ChFError("unterminated #if")


# ------------------------------------------------------------------ fixed form
def statements(lines):
    """Join fixed-form continuation lines: yields (label, text) per statement."""
    label, text = None, None
    for ln in lines:
        ln = ln.rstrip("\n").expandtabs(8)
        if not ln.strip() or ln[0] in "Cc*!":
            continue
        body = ln[6:]  # ChomboFortran lines may pass column 72: macros shrink or get re-wrapped
        open_macro = text is not None and text.count("[") > text.count("]")
        if open_macro:  # CHF_DTERM[ may hold whole statements, one per line
            text += " " + ln[:5].strip() + body.strip()
        elif len(ln) > 5 and ln[5] not in " 0":
            if text is None:
                raise ChFError("continuation line without a statement: " + ln)
            text += " " + body.strip()
        else:
            if text is not None:
                yield label, text
            label, text = ln[:5].strip(), body.strip()
    if text is not None:
        yield label, text


def emit(out, label, text, indent=0):
    """One statement as fixed form, wrapped at column 72."""
    text = " " * indent + text
    first = True
    while first or text:
        chunk, text = text[:66], text[66:]
        out.append(("%-5s " % label if first else "     &") + chunk)
        first = False


# ------------------------------------------------------------------ macros
def _split(args: str):
    return [a.strip() for a in args.split(";")]


def _dims(name):
    return [f"{name}{d}" for d in range(SPACEDIM)]


def _bounds(name):
    return [f"i{name}lo{d}" for d in range(SPACEDIM)] + [f"i{name}hi{d}" for d in range(SPACEDIM)]


def _offset(idx: str, off: str):
    m = re.fullmatch(r"([+-])\s*((?:\d+\s*\*\s*)?)(\w+)", off)
    if not m:
        raise ChFError(f"CHF_OFFSETIX offset '{off}'")
    sign, coef, name = m.groups()
    return ",".join(f"{idx}{d}{sign}{coef.replace(' ', '')}{name}{d}" for d in range(SPACEDIM))


def _do_loops(box, idx):
    """Loop nest over a box, last direction outermost (first index fastest)."""
    return [f"do {idx[d]} = i{box}lo{d},i{box}hi{d}" for d in reversed(range(SPACEDIM))]


_BRACKET = re.compile(r"\b(CHF_[A-Z0-9_]+)\s*\[([^\[\]]*)\]")
_ID = re.compile(r"\bCHF_ID\s*\(\s*([^,()]+?)\s*,\s*([^,()]+?)\s*\)")
_DTERM_C = re.compile(r"\bD_TERM\s*\(([^()]*)\)")


def expand_body(text: str):
    """Expand the body macros of one statement; returns a list of statements
    (the loop macros expand to several)."""
    pre, post = [], []

    def one(m):
        name, args = m.group(1), _split(m.group(2))
        if name == "CHF_DDECL" or name == "CHF_IX":
            return ",".join(args[:SPACEDIM])
        if name == "CHF_DTERM":
            return " ".join(args[:SPACEDIM])
        if name == "CHF_NCOMP":
            return f"n{args[0]}comp"
        if name == "CHF_LBOUND":
            return f"i{args[0]}lo{int(args[1])}"
        if name == "CHF_UBOUND":
            return f"i{args[0]}hi{int(args[1])}"
        if name in ("CHF_AUTODECL", "CHF_AUTOIX"):
            return ",".join(_dims(args[0]))
        if name == "CHF_OFFSETIX":
            return _offset(args[0], args[1])
        if name == "CHF_MULTIDO":
            pre.extend(_do_loops(args[0], args[1:1 + SPACEDIM]))
            return ""
        if name == "CHF_AUTOMULTIDO":
            pre.extend(_do_loops(args[0], _dims(args[1])))
            return ""
        raise ChFError(f"unsupported macro {name}")

    while True:
        text, n = _BRACKET.subn(one, text)
        if not n:
            break
    if "CHF_ENDDO" in text:
        text = re.sub(r"\bCHF_ENDDO\b", "", text)
        post.extend(["enddo"] * SPACEDIM)
    # Kronecker delta of two integers
    text = _ID.sub(lambda m: f"(1-min(1,abs(({m.group(1)})-({m.group(2)}))))", text)
    text = _DTERM_C.sub(lambda m: " ".join(a.strip() for a in m.group(1).split(",")[:SPACEDIM]), text)
    text = re.sub(r"\bREAL_T\b", "REAL*8", text, flags=re.I)
    text = re.sub(r"\bCH_SPACEDIM\b", str(SPACEDIM), text)
    text = re.sub(r"\b(" + "|".join(CONSTANTS) + r")\b", lambda m: CONSTANTS[m.group(1)], text)
    if "CHF_" in text:
        raise ChFError("unexpanded macro in: " + text)
    out = list(pre)
    if text.strip():
        # CHF_DTERM[ a = ..; b = ..; c = .. ] holds several assignments
        parts = _assignments(text)
        out.extend(parts)
    out.extend(post)
    return out


def _assignments(text: str):
    """`ii = i/2 jj = j/2 kk = k/2` (a CHF_DTERM of statements) -> three."""
    t = text.strip()
    cuts = [m.start() for m in re.finditer(r"(?<![<>=/.])\b[A-Za-z_]\w*\s*=(?!=)", t)]
    if len(cuts) <= 1 or cuts[0] != 0 or re.match(r"do\b", t, flags=re.I):
        return [t]
    depth, ok = 0, []
    for c in cuts:  # only assignments outside parentheses start a statement
        depth = t[:c].count("(") - t[:c].count(")")
        if depth == 0:
            ok.append(c)
    ok.append(len(t))
    return [t[a:b].strip() for a, b in zip(ok, ok[1:])]


_ARG = re.compile(r"\b(CHF_[A-Z0-9_]+)\s*\[\s*(\w+)\s*\]")


def expand_header(text: str):
    """subroutine NAME(args): returns (statement, declarations)."""
    ints, reals = [], []

    def one(m):
        kind, x = m.group(1), m.group(2)
        if kind in ("CHF_FRA", "CHF_CONST_FRA"):
            ints.append(f"integer n{x}comp")
            ints.append("integer " + ",".join(_bounds(x)))
            dims = ",".join(f"i{x}lo{d}:i{x}hi{d}" for d in range(SPACEDIM))
            reals.append(f"REAL*8 {x}({dims},0:n{x}comp-1)")
            return ",".join([x] + _bounds(x) + [f"n{x}comp"])
        if kind in ("CHF_FRA1", "CHF_CONST_FRA1"):
            ints.append("integer " + ",".join(_bounds(x)))
            dims = ",".join(f"i{x}lo{d}:i{x}hi{d}" for d in range(SPACEDIM))
            reals.append(f"REAL*8 {x}({dims})")
            return ",".join([x] + _bounds(x))
        if kind == "CHF_BOX":
            ints.append("integer " + ",".join(_bounds(x)))
            return ",".join(_bounds(x))
        if kind in ("CHF_CONST_REAL", "CHF_REAL"):
            reals.append(f"REAL*8 {x}")
            return x
        if kind in ("CHF_CONST_INT", "CHF_INT"):
            ints.append(f"integer {x}")
            return x
        raise ChFError(f"unsupported argument macro {kind}")

    return _ARG.sub(one, text), ["implicit none"] + ints + reals


def translate(src: str) -> str:
    out = ["C     Generated by chf2f.py from ChomboFortran; not a source file."]
    depth = 0
    for label, text in statements(preprocess(src.splitlines())):
        if re.match(r"subroutine\b", text, flags=re.I):
            head, decls = expand_header(text)
            emit(out, label, head, 0)
            for d in decls:
                emit(out, "", d, 2)
            depth = 1
            continue
        for st in expand_body(text):
            low = st.lower()
            if re.match(r"(end\s*do|end\s*if|else|end$)", low):
                depth = max(0, depth - 1)
            emit(out, label, st, 2 * depth)
            label = ""
            if re.match(r"do\b", low) or re.match(r"if\b.*\bthen$", low) or low.startswith("else"):
                depth += 1
    return "\n".join(out) + "\n"


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    with open(argv[1]) as f:
        src = f.read()
    with open(argv[2], "w") as f:
        f.write(translate(src))


if __name__ == "__main__":
    main(sys.argv)
