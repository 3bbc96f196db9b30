"""Reader of include/omega_amd.h, the one statement of what the C ABI takes: the ctypes binding sets its prototypes and
builds its struct mirrors from what read() returns.

Kinds are the header's own spellings without the parameter name: the scalars "int", "double", "size_t", "int64_t"
(struct members: "int32_t", "double"), pointers ("const char *", "double **", "const omg_mesh *", "void *const *", ...)
and the names of the callback typedefs.  A statement or a type outside these raises HeaderError naming it: nothing is
guessed and nothing is skipped.
"""
import re

SCALARS = ("int", "double", "size_t", "int64_t")
_STRUCT = r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;"


class HeaderError(ValueError):
    pass


def strip_comments(text: str) -> str:
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)


def _members(name: str, body: str) -> list:
    out = []
    for stmt in filter(None, (" ".join(s.split()) for s in body.split(";"))):
        m = re.fullmatch(r"(int32_t|double|const int32_t|const double) (.+)", stmt)
        if not m:
            raise HeaderError(f"cannot classify member `{stmt}` of {name}")
        for item in m.group(2).split(","):
            star, member = re.fullmatch(r" ?(\*?)(\w+)", item).groups()
            if bool(star) != m.group(1).startswith("const"):
                raise HeaderError(f"cannot classify member `{item.strip()}` of {name}")
            out.append((member, m.group(1) + (" *" if star else "")))
    return out


def _param(decl: str, callbacks: set, where: str) -> str:
    kind = re.sub(r"(?<=[*\s])\w+$", "", " ".join(decl.split())).strip()   # without the parameter's name
    if not (kind in SCALARS or kind in callbacks or re.fullmatch(r"(const )?\w+ \*(\*|const \*)?", kind)):
        raise HeaderError(f"cannot classify parameter `{decl.strip()}` of `{where}`")
    return kind


def read(path: str):
    """(functions, structs) of the header at `path`: {name: (return kind, [parameter kinds])} for every declared
    function and {name: [(member, kind), ...]} for every struct that has a body."""
    text = re.sub(r"^\s*#[^\n]*", "", strip_comments(open(path).read()), flags=re.M).replace('extern "C" {', "")
    structs = {name: _members(name, body) for body, name in re.findall(_STRUCT, text, flags=re.S)}
    text = re.sub(_STRUCT, "", text, flags=re.S)
    callbacks = set(re.findall(r"typedef int \(\*(\w+)\)", text))
    functions = {}
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        if stmt.startswith(("typedef ", "enum ")) or stmt == "}":
            continue
        m = re.fullmatch(r"(int|void|const char \*) ?(omg_\w+)\((.*)\)", stmt)
        if not m:
            raise HeaderError(f"cannot classify `{stmt}`")
        ret, name, params = m.groups()
        functions[name] = (ret, [] if params == "void" else [_param(p, callbacks, stmt) for p in params.split(",")])
    return functions, structs
