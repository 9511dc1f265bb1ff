"""CPU: the ctypes binding (_lib.py) against include/sdfr.h -- struct layouts through a
compiled C program, prototypes through the header's text.  Needs neither a GPU nor
libsdfr.so.

The file also runs against a binding from before ``c_name`` and ``PROTOTYPES`` existed
(the C name is then the first word of the class docstring, the prototypes are what
``lib()`` sets on the functions of a recording stand-in for the library): that is how
the table was shown to state what the statements it replaced stated.
"""
import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path


REPO = Path(__file__).resolve().parents[1]
HEADER = REPO / "include" / "sdfr.h"

SCALARS = {"uint32_t": ctypes.c_uint32, "int": ctypes.c_int, "float": ctypes.c_float,
           "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64}
RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p}


def c_name(cls):
    name = getattr(cls, "c_name", None)
    if name is None and cls.__doc__:
        name = cls.__doc__.split()[0]
    return name if name and name.startswith("sdfr_") else None


def mirrors(_lib):
    """C struct name -> the ctypes.Structure of _lib.py that mirrors it (each class once,
    whatever aliases it has)."""
    classes = {id(v): v for v in vars(_lib).values()
               if isinstance(v, type) and issubclass(v, ctypes.Structure)
               and v is not ctypes.Structure}
    named = {c_name(c): c for c in classes.values() if c_name(c)}
    unnamed = [c.__name__ for c in classes.values() if not c_name(c)]
    assert unnamed == ["ConvPlanStep"], unnamed      # (an unnamed member of the header)
    return named


def host_compiler():
    cc = shutil.which("cc")
    if cc:
        return cc
    clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    assert os.path.exists(clang), "no host C compiler: neither cc nor ROCm's clang"
    return clang


def members(cls, prefix=""):
    """(C member designator, ctypes offset, ctypes size) of every field; an array of
    structs (sdfr_conv_plan_info.steps, whose element type the header does not name) also
    gives the members of its first element."""
    for name, typ in cls._fields_:
        off = getattr(cls, name).offset
        yield prefix + name, off, ctypes.sizeof(typ)
        elem = getattr(typ, "_type_", None)
        if isinstance(elem, type) and issubclass(elem, ctypes.Structure):
            for sub, sub_off, size in members(elem, f"{prefix}{name}[0]."):
                yield sub, off + sub_off, size


def test_struct_layouts_match_header(sdfr, tmp_path):
    """sizeof of every mirrored struct and offsetof / sizeof of every ``_fields_`` entry,
    as the host C compiler lays include/sdfr.h out.  A field the header lacks does not
    compile.  Known limit: a trailing C member that ctypes lacks goes unnoticed when it
    fits into the struct's tail padding (the size does not change)."""
    named = mirrors(sdfr._lib)
    assert len(named) >= 14
    want, lines = {}, []
    for cname, cls in sorted(named.items()):
        want[cname] = (ctypes.sizeof(cls),)
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for member, off, size in members(cls):
            want[f"{cname}.{member}"] = (off, size)
            lines.append(f'printf("{cname}.{member} %zu %zu\\n", offsetof({cname}, {member}), '
                         f'sizeof((({cname} *)0)->{member}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdfr.h"\n'
                   "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([host_compiler(), "-std=c99", "-I", str(HEADER.parent), str(src), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {ln.split()[0]: tuple(map(int, ln.split()[1:])) for ln in out.splitlines()}
    assert set(got) == set(want)
    wrong = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not wrong, f"(ctypes, C) differ: {wrong}"
    # the element type of sdfr_conv_plan_info.steps, through the member's size
    info = named["sdfr_conv_plan_info"]
    assert got["sdfr_conv_plan_info.steps"][1] == 6 * ctypes.sizeof(sdfr._lib.ConvPlanStep)
    assert dict(info._fields_)["steps"]._type_ is sdfr._lib.ConvPlanStep


def binding_prototypes(_lib, monkeypatch):
    """name -> (restype, argtypes) of the binding."""
    table = getattr(_lib, "PROTOTYPES", None)
    if table is not None:
        return {k: (r, list(a)) for k, (r, a) in table.items()}

    class Fn:                       # what ctypes gives a function nobody described
        restype, argtypes = ctypes.c_int, None

        def __call__(self):
            return _lib.ABI_VERSION

    class Recorder:
        def __getattr__(self, name):
            return self.__dict__.setdefault(name, Fn())

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", HEADER)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: Recorder())
    rec = _lib.lib()
    return {k: (getattr(rec, k).restype, list(getattr(rec, k).argtypes or []))
            for k in _lib.EXPORTS}


def test_prototypes_match_header(sdfr, monkeypatch):
    """Return type and the class of every parameter of every function the header declares:
    pointer, or the exact ctypes type of a scalar.  A pointer to an sdfr_* struct is
    POINTER(its mirror) or c_void_p."""
    named = mirrors(sdfr._lib)
    bound = binding_prototypes(sdfr._lib, monkeypatch)
    txt = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    alias = dict((new, old) for old, new in re.findall(r"typedef\s+(sdfr_\w+)\s+(sdfr_\w+)\s*;", txt))
    protos = re.findall(r"\b(int|size_t|const char \*)\s*(sdfr_\w+)\s*\(([^()]*)\)\s*;", txt)
    assert len(protos) >= 86 and {p[1] for p in protos} == set(bound)
    wrong = []
    for ret, name, params in protos:
        restype, argtypes = bound[name]
        if restype is not RETURNS[ret]:
            wrong.append(f"{name}: returns {ret}, bound as {restype}")
        params = [" ".join(p.split()) for p in params.split(",")]
        params = [] if params == ["void"] else params
        if len(params) != len(argtypes):
            wrong.append(f"{name}: {len(params)} parameters, bound with {len(argtypes)}")
            continue
        for i, (p, t) in enumerate(zip(params, argtypes)):
            struct = re.search(r"\b(sdfr_\w+)\s*\*", p)
            if struct:
                cls = named.get(struct.group(1)) or named[alias[struct.group(1)]]
                ok = t is ctypes.c_void_p or t is ctypes.POINTER(cls)
            elif "*" in p:
                ok = t is ctypes.c_void_p or issubclass(t, ctypes._Pointer)
            else:
                ok = t is SCALARS[re.fullmatch(r"(?:const )?(\w+) \w+", p).group(1)]
            if not ok:
                wrong.append(f"{name}: parameter {i} `{p}` bound as {t}")
    assert not wrong, "\n".join(wrong)
