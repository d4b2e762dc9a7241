"""The C ABI as include/locator_hip.h declares it, read once at import: the LOC_* constants as module attributes, the
structs as ctypes Structures (STRUCTS) and the prototypes as (restype, argtypes) pairs (PROTOTYPES).  Nothing else in the
package restates the header.  The headers of the later entry points (_EXTENSION_TABLE: one line a header) are read likewise:
EXTENSIONS[tag] holds a header's path, constants and prototypes, the constants are module attributes too, and ALL_PROTOTYPES
is what the library binds.  _LATER_TABLE -> LATER[tag] is the same for the headers added since EXTENSIONS' tags were pinned, and _OPEN_TABLE -> OPEN[tag]
for those added since LATER's were.  No torch here: locator_amd.genotypes and the command line import this module before torch.

The reader knows the header's spelling, not C: one declaration per `;`, scalar types from _SCALARS, comments only as
/* */.  Anything else raises with the offending text, so that a header edit cannot silently drop or mis-type an entry."""
import ctypes as C
import os
import re
from typing import NamedTuple

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "locator_hip.h")
# The headers of the entry points added after version 1 of the ABI (the prototype list of locator_hip.h, which tests/test_abi.py
# pins), in the same spelling: (tag, file, the prefix its integer constants carry; None: it declares functions only).  A header
# declares no struct, and no function or constant that another header declares.  A new header goes at the end.
_EXTENSION_TABLE = (
    ("ext", "locator_hip_query.h", None),
    ("region", "locator_hip_regions.h", "LOC_REGION_"),
    ("neighbor", "locator_hip_neighbors.h", "LOC_IBS_"),
    ("pca", "locator_hip_pca.h", "LOC_PCA_"),
    ("ld", "locator_hip_ld.h", "LOC_LD_"),
    ("spa", "locator_hip_spa.h", "LOC_SPA_"),
    ("admix", "locator_hip_admix.h", "LOC_ADMIX_"),
    ("localpca", "locator_hip_localpca.h", "LOC_LOCALPCA_"),
    ("paint", "locator_hip_paint.h", "LOC_PAINT_"),
    ("ibd", "locator_hip_ibd.h", "LOC_IBD_"),
    ("impute", "locator_hip_impute.h", "LOC_IMPUTE_"),
)
# The headers added after that table's tags were pinned (tests/abi_util.py states them and is a yardstick that later changes leave
# alone), in the same form, read by the same loop with the same refusals: LATER[tag].  Its tags are pinned too (tests/test_phase.py).
_LATER_TABLE = (
    ("phase", "locator_hip_phase.h", "LOC_PHASE_"),
)
# The open table, in the same form, read by the same loop with the same refusals: OPEN[tag].  New headers go here, at the end.  A
# test asserts only the line of its own tag (OPEN["local"]), never the list of this table's keys, so that the next header needs no
# fourth table.
_OPEN_TABLE = (
    ("local", "locator_hip_local.h", "LOC_LOCAL_"),
)

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
_POINTEES = ("void", "char", "int8_t", "uint8_t")        # types that occur only behind a pointer
_BY_REFERENCE = ("loc_dims", "loc_layout", "loc_net", "loc_tuning")   # structs Python fills and passes with byref()

_FIRST = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*)*)(\w+)$")     # `const float* w1s`, `int K`, `void** h_ev`
_NEXT = re.compile(r"((?:\*\s*)*)(\w+)$")                            # `*beta`, `Kp` after a comma
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(LOC_\w+)[ \t]+(\S.*?)[ \t]*$", re.M)   # object-like only
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", re.S)
_PROTO = re.compile(r"(.*?)\b(loc_\w+)\s*\((.*)\)$", re.S)


def _ctype(base, stars, name, structs, arg):
    """The ctypes type of one declarator: a struct member (arg False) or a parameter (arg True)."""
    if base not in _SCALARS and base not in _POINTEES and base not in structs:
        raise ValueError(f"locator_hip.h: unknown type `{base}` in `{base} {stars}{name}`")
    if not stars:
        if base in _SCALARS:
            return _SCALARS[base]
        if base in structs and not arg:
            return structs[base]
        raise ValueError(f"locator_hip.h: `{base} {name}` is neither a scalar nor a pointer")
    if arg and stars == "**":
        return C.POINTER(C.c_void_p)
    if arg and base in _BY_REFERENCE:
        return C.POINTER(structs[base])
    if arg and name.startswith("h_") and base in _SCALARS:           # the header's rule: host pointers are named h_*
        return C.POINTER(_SCALARS[base])
    return C.c_void_p


def _declarators(decl, structs, arg):
    """`float *gamma, *beta` -> [("gamma", c_void_p), ("beta", c_void_p)]."""
    first, *rest = [p.strip() for p in decl.split(",")]
    m = _FIRST.match(first)
    if not m:
        raise ValueError(f"locator_hip.h: cannot split `{decl.strip()}` into type and name")
    out = [(m.group(3), _ctype(m.group(1), m.group(2).replace(" ", ""), m.group(3), structs, arg))]
    for p in rest:
        n = _NEXT.match(p)
        if not n:
            raise ValueError(f"locator_hip.h: cannot read declarator `{p}` of `{decl.strip()}`")
        out.append((n.group(2), _ctype(m.group(1), n.group(1).replace(" ", ""), n.group(2), structs, arg)))
    return out


def parse(text):
    """Header text -> (constants, structs, prototypes), each a dict in header order."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts, structs, protos = {}, {}, {}
    for name, value in _DEFINE.findall(text):
        if not re.fullmatch(r"-?\d+|-?\d+\.\d*f?", value):
            raise ValueError(f"locator_hip.h: `#define {name} {value}` is not an integer or float literal")
        consts[name] = int(value) if value.lstrip("-").isdigit() else float(value.rstrip("f"))
    text = re.sub(r"#ifdef __cplusplus.*?#endif", "", text, flags=re.S)          # extern "C" { ... }
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)

    def struct(m):
        fields = [f for decl in m.group(2).split(";") if decl.strip() for f in _declarators(decl, structs, False)]
        pyname = "".join(w.title() for w in m.group(1).split("_")[1:])           # loc_cb_state -> CbState
        structs[m.group(1)] = type(pyname, (C.Structure,), {"_fields_": fields})
        return ""

    for decl in _STRUCT.sub(struct, text).split(";"):
        if not decl.strip():
            continue
        m = _PROTO.fullmatch(decl.strip())
        if not m:
            raise ValueError(f"locator_hip.h: `{decl.strip()}` is not a prototype `T loc_name(args)`")
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        res = C.c_char_p if ret == "const char*" else _declarators(ret + " _", structs, False)[0][1]
        protos[name] = (res, [] if args == "void" else [_declarators(a, structs, True)[0][1] for a in args.split(",")])
    return consts, structs, protos


if not os.path.exists(HEADER):
    raise FileNotFoundError(f"{HEADER} not found: locator_amd runs in-tree and derives its ctypes binding from "
                            "include/locator_hip.h (the same relative path locator_amd/csrc compiles against).")
with open(HEADER) as _f:
    CONSTANTS, STRUCTS, PROTOTYPES = parse(_f.read())
globals().update(CONSTANTS)


class Extension(NamedTuple):
    header: str
    constants: dict
    prototypes: dict


EXTENSIONS, LATER, OPEN = {}, {}, {}
ALL_PROTOTYPES = dict(PROTOTYPES)
_declared = set(CONSTANTS) | set(PROTOTYPES)         # by the main header and the tables' lines so far
for _into, _table in ((EXTENSIONS, _EXTENSION_TABLE), (LATER, _LATER_TABLE), (OPEN, _OPEN_TABLE)):
    for _tag, _name, _prefix in _table:
        _path = os.path.join(os.path.dirname(HEADER), _name)
        if not os.path.exists(_path):
            raise FileNotFoundError(f"{_path} not found: it declares entry points added after include/locator_hip.h")
        with open(_path) as _f:
            _consts, _structs, _protos = parse(_f.read())
        _again = sorted(_declared & (set(_consts) | set(_protos)))
        _foreign = sorted(k for k, v in _consts.items() if _prefix is None or not k.startswith(_prefix) or not isinstance(v, int))
        if _structs or _again or _foreign or _tag in EXTENSIONS or _tag in LATER or _tag in OPEN:
            raise ValueError(f"{_path} may declare new functions " + ("only" if _prefix is None else f"and {_prefix}* integer constants only")
                             + "".join(f"; {what}: {', '.join(names)}" for what, names in (("declared before", _again), ("not such a constant", _foreign))
                                       if names))
        _declared |= set(_consts) | set(_protos)
        _into[_tag] = Extension(_path, _consts, _protos)
        ALL_PROTOTYPES.update(_protos)
        globals().update(_consts)
