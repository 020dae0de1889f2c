"""The C-prototype parser and the type rule of the binding tests (tests/test_abi_symbols.py runs them over every header of
_abi.HEADERS; the host tests of a header read single prototypes through header_prototypes)."""
import ctypes
import re

from epilogos_amd import _abi

CTYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "uint64_t": ctypes.c_uint64}


def header_prototypes(which):
    """name -> (return type, [parameter declarations]) of every prototype in the header `which` of _abi.HEADERS."""
    txt = re.sub(r"/\*.*?\*/", "", _abi.HEADERS[which].path.read_text(), flags=re.S)
    txt = re.sub(r'^\s*(#.*|extern "C" \{|\})\s*$', "", txt, flags=re.M)
    protos = {}
    for stmt in txt.split(";"):
        m = re.match(r"\s*(.*?)\b(epg[tf]?_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, flags=re.S)
        if m:
            args = " ".join(m.group(3).split())
            protos[m.group(2)] = (" ".join(m.group(1).split()), [] if args in ("", "void") else [a.strip() for a in args.split(",")])
    return protos


def ctypes_of(decl, returned=False):
    """THE ctypes type that binds a header type (a return type, or a parameter declaration with or without its name): a pointer
    parameter is c_void_p, a returned `const char*` c_char_p, an integer exactly its own type."""
    if "*" in decl:
        if returned:
            assert decl.replace(" ", "") == "constchar*", decl
            return ctypes.c_char_p
        return ctypes.c_void_p
    return CTYPES[decl.replace("const ", "").split()[0]]
