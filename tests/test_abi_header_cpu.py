"""include/danhip.h against dan_amd/_lib.py: every function's return type and parameters against PROTOTYPES, every struct's fields
against its ctypes mirror.  The header is read as text (comments stripped); only the last test loads the library.

What is compared is a CLASS per type: "pointer" (any pointer or array parameter, whichever ctypes pointer type the table uses), or for
a scalar (kind, bytes) with kind i / u / f.  int and int32_t are one class.  ctypes itself makes c_size_t and c_uint64 ONE object where
the platform's size_t is 64 bits wide (as it makes c_int32 and c_int one), so a table entry cannot say which of the two it means; the
class is what the call passes, and on a platform where size_t and uint64_t differ in width the two classes differ too.  int64_t,
uint32_t, float and double each stand alone."""
import ctypes
import os
import re

import pytest

from dan_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_SCALARS = {"int": ("i", ctypes.sizeof(ctypes.c_int)), "int32_t": ("i", 4), "int64_t": ("i", 8), "size_t": ("u", ctypes.sizeof(ctypes.c_size_t)),
             "uint8_t": ("u", 1), "uint16_t": ("u", 2), "uint32_t": ("u", 4), "uint64_t": ("u", 8), "float": ("f", 4), "double": ("f", 8)}
STRUCT = re.compile(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", re.S)
FUNCTION = re.compile(r"([\w\s*]+?)\b(danhip_\w+)\s*\((.*)\)", re.S)
# danhip_augment_item has no Python mirror: its users take danhip_augment_item_bytes() and hand danhip_augment_item_init a raw buffer
UNMIRRORED = ("danhip_augment_item",)


def c_class(decl, what):
    """Class of a C declaration without its name: 'const float*' -> pointer, 'int32_t' -> ('i', 4)."""
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    assert len(words) == 1 and words[0] in C_SCALARS, "%s: the parser does not know the type %r" % (what, decl)
    return C_SCALARS[words[0]]


def py_class(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, (ctypes._Pointer, ctypes.Array)):
        return "pointer"
    return ("f" if t in (ctypes.c_float, ctypes.c_double) else "u" if t(-1).value > 0 else "i", ctypes.sizeof(t))


def parse_header(text):
    """-> ({function: (return class, [parameter classes])}, {struct: [(field, class, array lengths)]}); anything else is an error."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M).replace('extern "C" {', "")
    structs = {}
    for body, name in STRUCT.findall(text):
        fields = structs[name] = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(r"(.*?[\w*])\s+(\w[\w\s,\[\]]*)", decl, re.S)
            assert m, "struct %s: the parser cannot read the field %r" % (name, decl)
            names = [n.strip() for n in m.group(2).split(",")]
            assert "*" not in m.group(1) or len(names) == 1, "struct %s: several declarators behind a pointer type: %r" % (name, decl)
            for n in names:
                dims = tuple(int(d) for d in re.findall(r"\[(\d+)\]", n))
                fields.append((n.split("[")[0], c_class(m.group(1), "struct " + name), dims))
    functions = {}
    for stmt in filter(None, (s.strip() for s in STRUCT.sub("", text).split(";"))):
        m = FUNCTION.fullmatch(stmt)
        assert m or stmt == "}", "the parser cannot read the statement %r" % stmt          # "}" closes extern "C"
        if m:
            params = [] if m.group(3).strip() == "void" else [p.strip() for p in m.group(3).split(",")]
            classes = []
            for p in params:
                pm = re.fullmatch(r"(.*?[\w*])\s*\b(\w+)((?:\[\d+\])*)", p, re.S)
                assert pm, "%s: the parser cannot read the parameter %r" % (m.group(2), p)
                classes.append("pointer" if pm.group(3) else c_class(pm.group(1), m.group(2)))
            assert m.group(2) not in functions, "declared twice: " + m.group(2)
            functions[m.group(2)] = (c_class(m.group(1), m.group(2)), classes)
    return functions, structs


def function_mismatches(declared, table):
    out = ["PROTOTYPES lacks " + n for n in declared if n not in table] + ["the header lacks " + n for n in table if n not in declared]
    for name in declared:
        if name in table:
            res, args = table[name]
            if not isinstance(args, list):
                out.append("%s: no explicit argtypes list" % name)
                continue
            got = (py_class(res), [py_class(a) for a in args])
            if got != declared[name]:
                out.append("%s: the header says %r, PROTOTYPES %r" % (name, declared[name], got))
    return out


def mirror_fields(cls):
    out = []
    for name, t in cls._fields_:
        dims = ()
        while issubclass(t, ctypes.Array):
            dims, t = dims + (t._length_,), t._type_
        out.append((name, py_class(t), dims))
    return out


def mirror_of(struct):
    """danhip_jpeg_enc_desc -> _lib.JpegEncDesc"""
    return getattr(_lib, "".join(w.capitalize() for w in struct[len("danhip_"):].split("_")), None)


def struct_mismatches(structs, mirrors):
    out = []
    for name, fields in structs.items():
        if name in UNMIRRORED:
            continue
        if mirrors.get(name) is None:
            out.append("%s has no mirror in dan_amd/_lib.py" % name)
        elif mirrors[name] != fields:
            out.append("%s: the header says %r, the mirror %r" % (name, fields, mirrors[name]))
    return out


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "danhip.h")) as f:
        return parse_header(f.read())


def test_the_parser_reads_the_whole_header(header):
    functions, structs = header
    assert len(functions) >= 195 and len(structs) >= 11
    assert functions["danhip_last_error"] == ("pointer", []) and functions["danhip_draw_glyph"] == (("i", 4), [("i", 4), "pointer"])
    assert functions["danhip_crc32c_combine"] == (("u", 4), [("u", 4), ("u", 4), ("u", 8)])
    assert functions["danhip_resize_u8_linear"][1][6:9] == [("i", 4), ("f", 8), ("f", 8)]
    assert structs["danhip_jpeg_desc"][-1] == ("quant", ("u", 2), (4, 64)) and structs["danhip_conv_pitch"][1] == ("y_pitch", ("i", 4), ())
    assert set(UNMIRRORED) <= set(structs)


def test_every_prototype_agrees_with_the_header(header):
    assert function_mismatches(header[0], _lib.PROTOTYPES) == []
    assert all(_lib.PROTOTYPES[n] == (ctypes.c_int, a) for n, a in _lib.SIGNATURES.items())


def test_every_struct_mirror_agrees_with_the_header(header):
    mirrors = {name: mirror_fields(mirror_of(name)) if mirror_of(name) else None for name in header[1]}
    assert struct_mismatches(header[1], mirrors) == []


def test_wrong_prototypes_and_mirrors_are_reported(header):
    """The comparison applied to deliberately wrong copies of one entry: each is reported, and nothing else is."""
    functions, structs = header
    P, I32, I64 = _lib.P, _lib.I32, _lib.I64
    assert _lib.PROTOTYPES["danhip_relu_bits"] == (ctypes.c_int, [P, P, I64, I32, P])
    assert _lib.PROTOTYPES["danhip_reduce_workspace_bytes"] == (ctypes.c_size_t, [I64, I32])
    for name, wrong in (("danhip_relu_bits", (ctypes.c_int, [P, P, I32, I32, P])),                 # int64_t bound as I32
                        ("danhip_relu_bits", (ctypes.c_int, [P, P, I64, I32])),                    # one argument dropped
                        ("danhip_reduce_workspace_bytes", (ctypes.c_int, [I64, I32])),             # a size_t return left at int
                        ("danhip_version", (ctypes.c_int, None))):                                 # no argtypes at all
        found = function_mismatches(functions, dict(_lib.PROTOTYPES, **{name: wrong}))
        assert len(found) == 1 and found[0].startswith(name + ":"), (name, wrong, found)
    found = function_mismatches(functions, {n: p for n, p in _lib.PROTOTYPES.items() if n != "danhip_add16"})
    assert found == ["PROTOTYPES lacks danhip_add16"]
    found = function_mismatches(functions, dict(_lib.PROTOTYPES, danhip_no_such_call=(ctypes.c_int, [])))
    assert found == ["the header lacks danhip_no_such_call"]
    mirrors = {name: mirror_fields(mirror_of(name)) for name in structs if name not in UNMIRRORED}
    info = mirrors["danhip_jpeg_info"]
    assert [f[0] for f in info[4:6]] == ["reason", "reserved"] and info[4][1:] == info[5][1:]
    swapped = dict(mirrors, danhip_jpeg_info=info[:4] + [info[5], info[4]] + info[6:])              # two fields of one type swapped
    found = struct_mismatches(structs, swapped)
    assert len(found) == 1 and found[0].startswith("danhip_jpeg_info:"), found
    assert struct_mismatches(structs, dict(mirrors, danhip_draw_item=None)) == ["danhip_draw_item has no mirror in dan_amd/_lib.py"]


def test_mirror_sizes_equal_the_library_sizeof_exports(header):
    """sizeof of every mirror whose struct has a <struct>_bytes() export, asked of both builds."""
    from dan_amd import build
    build.build()
    asked = []
    for so in (build.OUT, build.OUT_F16):
        L = ctypes.CDLL(so)
        for name in header[1]:
            if name + "_bytes" in _lib.PROTOTYPES and name not in UNMIRRORED:
                _lib.bind(L, [name + "_bytes"])
                assert getattr(L, name + "_bytes")() == ctypes.sizeof(mirror_of(name)), name
                asked.append(name)
    assert sorted(set(asked)) == ["danhip_crc_segment", "danhip_draw_item", "danhip_jpeg_enc_desc", "danhip_resize_item"]
