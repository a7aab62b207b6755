"""Reads a C ABI header (include/kdiff_hip.h) into ctypes: prototypes, descriptor structs, enum constants and integer #defines.

The header is the one declaration of the ABI; ``_native`` binds from what ``parse`` returns.  The parser knows the small subset of C the
header is written in and fails closed: whatever it cannot read as that subset raises ``HeaderError`` with the offending text.  It never guesses.

Type rule (no exceptions by name): int, unsigned, float, double, long long and unsigned long long are the matching ctypes type; char* and
const char* are c_char_p; every other pointer is c_void_p (pointers to pointers and to the Kd* structs included: callers pass byref(...), a
ctypes array, a device address or None).
"""
import ctypes as C
import re
from collections import namedtuple

Abi = namedtuple("Abi", "signatures restypes structs constants")     # name -> argtypes / restype / Structure class / int


class HeaderError(ValueError):
    pass


_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong,
            "unsigned long long": C.c_ulonglong}
_POINTEES = set(_SCALARS) | {"void", "char", "unsigned char"}         # and the structs declared so far
_INT = r"\(?\s*(-?\d+)\s*\)?"


def _ctype(text, structs, where):
    """The ctypes type of the C type ``text`` by the rule above."""
    words = [w for w in text.replace("*", " * ").split() if w != "const"]
    base, stars = " ".join(w for w in words if w != "*"), words.count("*")
    if not stars:
        if base not in _SCALARS:
            raise HeaderError(f"type {text.strip()!r} is outside the type rule, in: {where}")
        return _SCALARS[base]
    if base not in _POINTEES and base not in structs:
        raise HeaderError(f"pointer to {base!r} is outside the type rule, in: {where}")
    return C.c_char_p if (base, stars) == ("char", 1) else C.c_void_p


def _preprocess(text, constants):
    """The text a C compiler sees: comments out, #ifdef / #ifndef blocks of undefined names out, integer ``#define KD_X n`` into ``constants``."""
    if text.count("/*") != len(re.findall(r"/\*.*?\*/", text, flags=re.S)):
        raise HeaderError("unterminated comment")
    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    defined, active, out = set(), [], []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            if all(active):
                out.append(line)
            continue
        m = re.fullmatch(r"\s*#\s*(ifdef|ifndef|endif|define)\b\s*(\w*)\s*(.*?)\s*", line)
        word, name, value = m.groups() if m else ("", "", "")
        if not m or (word == "endif") != (name == "") or (value and word != "define"):
            raise HeaderError(f"preprocessor line not understood: {line.strip()}")
        if word == "endif":
            if not active:
                raise HeaderError("#endif without #if")
            active.pop()
        elif word != "define":
            active.append((name in defined) == (word == "ifdef"))
        elif all(active):
            defined.add(name)
            if value:
                v = re.fullmatch(_INT, value)
                if not v or not name.startswith("KD_"):
                    raise HeaderError(f"#define is not an integer constant KD_*: {line.strip()}")
                constants[name] = int(v.group(1))
    if active:
        raise HeaderError("#if without #endif")
    return "\n".join(out)


def _declarations(text):
    """The top-level declarations: split at every ';' outside braces."""
    depth, cur = 0, []
    for piece in text.split(";"):
        cur.append(piece)
        for brace in re.findall(r"[{}]", piece):
            depth += 1 if brace == "{" else -1
            if depth < 0:
                raise HeaderError("unbalanced '}' after: " + " ".join(";".join(cur).split())[-80:])
        if depth == 0:
            yield " ".join(";".join(cur).split())
            cur = []
    if depth:
        raise HeaderError("unbalanced '{' in: " + " ".join(";".join(cur).split())[:120])


def _enum(body, constants, where):
    for item in body.split(","):
        m = re.fullmatch(r"\s*(KD_[A-Za-z0-9_]+)\s*=\s*" + _INT + r"\s*", item)
        if not m:
            raise HeaderError(f"enumerator {item.strip()!r} is not 'KD_NAME = integer', in: {where}")
        if m.group(1) in constants:
            raise HeaderError(f"{m.group(1)} is defined twice")
        constants[m.group(1)] = int(m.group(2))


def _struct(body, structs, where):
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.fullmatch(r"([A-Za-z_][\w\s\*]*?[\s\*])((?:\w+(?:\s*\[\s*\d+\s*\])?\s*,\s*)*\w+(?:\s*\[\s*\d+\s*\])?)", decl)
        if not m or re.search(r"\b(struct|union|enum)\b", decl) or (m.group(2).count(",") and "*" in decl):
            raise HeaderError(f"struct field {decl!r} cannot be classified, in: {where}")
        ctype = _ctype(m.group(1), structs, decl)
        for item in m.group(2).split(","):
            name, count = re.fullmatch(r"\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", item).groups()
            fields.append((name, ctype * int(count) if count else ctype))
    if not fields:
        raise HeaderError(f"struct without fields: {where}")
    return fields


def _prototype(ret, args, structs, where):
    argtypes = []
    if args.strip() != "void":
        for arg in args.split(","):
            m = re.fullmatch(r"\s*([A-Za-z_][\w\s\*]*?[\s\*])(\w+)\s*", arg)
            if not m:
                raise HeaderError(f"parameter {arg.strip()!r} is not 'type name', in: {where}")
            argtypes.append(_ctype(m.group(1), structs, where))
    return argtypes, _ctype(ret, structs, where)


def parse(text):
    """``Abi`` of a header's text."""
    signatures, restypes, structs, constants = {}, {}, {}, {}
    text = _preprocess(text, constants)
    for decl in _declarations(text):
        if not decl:
            continue
        m = re.fullmatch(r"enum\s*\{(.*)\}", decl)
        if m:
            _enum(m.group(1), constants, decl)
            continue
        m = re.fullmatch(r"typedef struct\s*(\w*)\s*\{(.*)\}\s*(\w+)", decl)
        if m:
            if m.group(3) in structs or m.group(1) not in ("", m.group(3)):
                raise HeaderError(f"struct {m.group(3)} is declared twice or under two names")
            fields = _struct(m.group(2), structs, decl)
            structs[m.group(3)] = type(m.group(3), (C.Structure,), {"_fields_": fields, "__doc__": f"{m.group(3)} of the C ABI header"})
            continue
        m = re.fullmatch(r"([A-Za-z_][\w\s\*]*?[\s\*])(kd_\w+)\s*\(([^(){}]*)\)", decl)
        if not m or m.group(2) in signatures:
            raise HeaderError(f"not an enum, a typedef struct or a prototype of a kd_* entry point: {decl[:200]}")
        signatures[m.group(2)], restypes[m.group(2)] = _prototype(m.group(1), m.group(3), structs, decl)
    named = re.findall(r"\b(kd_\w+)\s*\(", text)
    if sorted(named) != sorted(signatures):
        raise HeaderError(f"kd_* followed by '(' that is no prototype: {sorted(set(named) - set(signatures)) or named}")
    return Abi(signatures, restypes, structs, constants)
