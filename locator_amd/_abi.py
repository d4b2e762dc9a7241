"""The C ABI as include/locator_hip.h declares it, read once at import: the LOC_* constants as module attributes, the
structs as ctypes Structures (STRUCTS) and the prototypes as (restype, argtypes) pairs (PROTOTYPES).  Nothing else in the
package restates the header.  include/locator_hip_query.h (later entry points) is read likewise: EXT_PROTOTYPES, and so is
include/locator_hip_regions.h (the regions command): REGION_PROTOTYPES and its LOC_REGION_* constants, and
include/locator_hip_neighbors.h (the neighbors command): NEIGHBOR_PROTOTYPES and its LOC_IBS_* constants, and
include/locator_hip_pca.h (the pca command): PCA_PROTOTYPES and its LOC_PCA_* constants, and
include/locator_hip_ld.h (the ld command): LD_PROTOTYPES and its LOC_LD_* constants, and
include/locator_hip_spa.h (the spa command): SPA_PROTOTYPES and its LOC_SPA_* constants, and
include/locator_hip_admix.h (the admix command): ADMIX_PROTOTYPES and its LOC_ADMIX_* constants, and
include/locator_hip_localpca.h (the localpca command): LOCALPCA_PROTOTYPES and its LOC_LOCALPCA_* constants, and
include/locator_hip_paint.h (the paint command): PAINT_PROTOTYPES and its LOC_PAINT_* constants, and
include/locator_hip_ibd.h (the ibd command): IBD_PROTOTYPES and its LOC_IBD_* constants.  No torch here: locator_amd.genotypes and the command line import this module before torch.

The reader knows the header's spelling, not C: one declaration per `;`, scalar types from _SCALARS, comments only as
/* */.  Anything else raises with the offending text, so that a header edit cannot silently drop or mis-type an entry."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "locator_hip.h")
# entry points added after version 1 of the ABI (the prototype list of locator_hip.h, which tests/test_abi.py pins): the same
# spelling, read by the same parser into EXT_PROTOTYPES; it declares functions only
EXT_HEADER = os.path.join(os.path.dirname(HEADER), "locator_hip_query.h")
# the regions command's entry points (locator_amd/regions.py): functions and LOC_REGION_* integer constants only
REGION_HEADER = os.path.join(os.path.dirname(HEADER), "locator_hip_regions.h")
# the neighbors command's entry points (locator_amd/neighbors.py): functions and LOC_IBS_* integer constants only
NEIGHBOR_HEADER = os.path.join(os.path.dirname(HEADER), "locator_hip_neighbors.h")
# the pca command's entry points (locator_amd/pca.py): functions and LOC_PCA_* integer constants only
PCA_HEADER = os.path.join(os.path.dirname(HEADER), "locator_hip_pca.h")
# the ld command's entry point (locator_amd/ld.py): functions and LOC_LD_* integer constants only
LD_HEADER = os.path.join(os.path.dirname(HEADER), "locator_hip_ld.h")
# the spa command's entry points (locator_amd/spa.py): functions and LOC_SPA_* integer constants only
SPA_HEADER = os.path.join(os.path.dirname(HEADER), "locator_hip_spa.h")
# the admix command's entry points (locator_amd/admix.py): functions and LOC_ADMIX_* integer constants only
ADMIX_HEADER = os.path.join(os.path.dirname(HEADER), "locator_hip_admix.h")
# the localpca command's entry point (locator_amd/localpca.py): functions and LOC_LOCALPCA_* integer constants only
LOCALPCA_HEADER = os.path.join(os.path.dirname(HEADER), "locator_hip_localpca.h")
# the paint command's entry points (locator_amd/paint.py): functions and LOC_PAINT_* integer constants only
PAINT_HEADER = os.path.join(os.path.dirname(HEADER), "locator_hip_paint.h")
# the ibd command's entry points (locator_amd/ibd.py): functions and LOC_IBD_* integer constants only
IBD_HEADER = os.path.join(os.path.dirname(HEADER), "locator_hip_ibd.h")

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
if not os.path.exists(EXT_HEADER):
    raise FileNotFoundError(f"{EXT_HEADER} not found: it declares the entry points added after include/locator_hip.h")
with open(EXT_HEADER) as _f:
    _consts, _structs, EXT_PROTOTYPES = parse(_f.read())
if _consts or _structs or set(EXT_PROTOTYPES) & set(PROTOTYPES):
    raise ValueError(f"{EXT_HEADER} may declare new functions only")
if not os.path.exists(REGION_HEADER):
    raise FileNotFoundError(f"{REGION_HEADER} not found: it declares the entry points of the regions command")
with open(REGION_HEADER) as _f:
    REGION_CONSTANTS, _structs, REGION_PROTOTYPES = parse(_f.read())
if (_structs or set(REGION_PROTOTYPES) & (set(PROTOTYPES) | set(EXT_PROTOTYPES)) or set(REGION_CONSTANTS) & set(CONSTANTS)
        or not all(k.startswith("LOC_REGION_") and isinstance(v, int) for k, v in REGION_CONSTANTS.items())):
    raise ValueError(f"{REGION_HEADER} may declare new functions and LOC_REGION_* integer constants only")
globals().update(REGION_CONSTANTS)
if not os.path.exists(NEIGHBOR_HEADER):
    raise FileNotFoundError(f"{NEIGHBOR_HEADER} not found: it declares the entry points of the neighbors command")
with open(NEIGHBOR_HEADER) as _f:
    NEIGHBOR_CONSTANTS, _structs, NEIGHBOR_PROTOTYPES = parse(_f.read())
if (_structs or set(NEIGHBOR_PROTOTYPES) & (set(PROTOTYPES) | set(EXT_PROTOTYPES) | set(REGION_PROTOTYPES))
        or not all(k.startswith("LOC_IBS_") and isinstance(v, int) for k, v in NEIGHBOR_CONSTANTS.items())):
    raise ValueError(f"{NEIGHBOR_HEADER} may declare new functions and LOC_IBS_* integer constants only")
globals().update(NEIGHBOR_CONSTANTS)
if not os.path.exists(PCA_HEADER):
    raise FileNotFoundError(f"{PCA_HEADER} not found: it declares the entry points of the pca command")
with open(PCA_HEADER) as _f:
    PCA_CONSTANTS, _structs, PCA_PROTOTYPES = parse(_f.read())
if (_structs or set(PCA_PROTOTYPES) & (set(PROTOTYPES) | set(EXT_PROTOTYPES) | set(REGION_PROTOTYPES) | set(NEIGHBOR_PROTOTYPES))
        or not all(k.startswith("LOC_PCA_") and isinstance(v, int) for k, v in PCA_CONSTANTS.items())):
    raise ValueError(f"{PCA_HEADER} may declare new functions and LOC_PCA_* integer constants only")
globals().update(PCA_CONSTANTS)
if not os.path.exists(LD_HEADER):
    raise FileNotFoundError(f"{LD_HEADER} not found: it declares the entry point of the ld command")
with open(LD_HEADER) as _f:
    LD_CONSTANTS, _structs, LD_PROTOTYPES = parse(_f.read())
if (_structs or set(LD_PROTOTYPES) & (set(PROTOTYPES) | set(EXT_PROTOTYPES) | set(REGION_PROTOTYPES) | set(NEIGHBOR_PROTOTYPES)
                                      | set(PCA_PROTOTYPES))
        or not all(k.startswith("LOC_LD_") and isinstance(v, int) for k, v in LD_CONSTANTS.items())):
    raise ValueError(f"{LD_HEADER} may declare new functions and LOC_LD_* integer constants only")
globals().update(LD_CONSTANTS)
if not os.path.exists(SPA_HEADER):
    raise FileNotFoundError(f"{SPA_HEADER} not found: it declares the entry points of the spa command")
with open(SPA_HEADER) as _f:
    SPA_CONSTANTS, _structs, SPA_PROTOTYPES = parse(_f.read())
if (_structs or set(SPA_PROTOTYPES) & (set(PROTOTYPES) | set(EXT_PROTOTYPES) | set(REGION_PROTOTYPES) | set(NEIGHBOR_PROTOTYPES)
                                       | set(PCA_PROTOTYPES) | set(LD_PROTOTYPES))
        or not all(k.startswith("LOC_SPA_") and isinstance(v, int) for k, v in SPA_CONSTANTS.items())):
    raise ValueError(f"{SPA_HEADER} may declare new functions and LOC_SPA_* integer constants only")
globals().update(SPA_CONSTANTS)
if not os.path.exists(ADMIX_HEADER):
    raise FileNotFoundError(f"{ADMIX_HEADER} not found: it declares the entry points of the admix command")
with open(ADMIX_HEADER) as _f:
    ADMIX_CONSTANTS, _structs, ADMIX_PROTOTYPES = parse(_f.read())
if (_structs or set(ADMIX_PROTOTYPES) & (set(PROTOTYPES) | set(EXT_PROTOTYPES) | set(REGION_PROTOTYPES) | set(NEIGHBOR_PROTOTYPES)
                                         | set(PCA_PROTOTYPES) | set(LD_PROTOTYPES) | set(SPA_PROTOTYPES))
        or not all(k.startswith("LOC_ADMIX_") and isinstance(v, int) for k, v in ADMIX_CONSTANTS.items())):
    raise ValueError(f"{ADMIX_HEADER} may declare new functions and LOC_ADMIX_* integer constants only")
globals().update(ADMIX_CONSTANTS)
if not os.path.exists(LOCALPCA_HEADER):
    raise FileNotFoundError(f"{LOCALPCA_HEADER} not found: it declares the entry point of the localpca command")
with open(LOCALPCA_HEADER) as _f:
    LOCALPCA_CONSTANTS, _structs, LOCALPCA_PROTOTYPES = parse(_f.read())
if (_structs or set(LOCALPCA_PROTOTYPES) & (set(PROTOTYPES) | set(EXT_PROTOTYPES) | set(REGION_PROTOTYPES) | set(NEIGHBOR_PROTOTYPES)
                                            | set(PCA_PROTOTYPES) | set(LD_PROTOTYPES) | set(SPA_PROTOTYPES) | set(ADMIX_PROTOTYPES))
        or not all(k.startswith("LOC_LOCALPCA_") and isinstance(v, int) for k, v in LOCALPCA_CONSTANTS.items())):
    raise ValueError(f"{LOCALPCA_HEADER} may declare new functions and LOC_LOCALPCA_* integer constants only")
globals().update(LOCALPCA_CONSTANTS)
if not os.path.exists(PAINT_HEADER):
    raise FileNotFoundError(f"{PAINT_HEADER} not found: it declares the entry points of the paint command")
with open(PAINT_HEADER) as _f:
    PAINT_CONSTANTS, _structs, PAINT_PROTOTYPES = parse(_f.read())
if (_structs or set(PAINT_PROTOTYPES) & (set(PROTOTYPES) | set(EXT_PROTOTYPES) | set(REGION_PROTOTYPES) | set(NEIGHBOR_PROTOTYPES)
                                         | set(PCA_PROTOTYPES) | set(LD_PROTOTYPES) | set(SPA_PROTOTYPES) | set(ADMIX_PROTOTYPES)
                                         | set(LOCALPCA_PROTOTYPES))
        or not all(k.startswith("LOC_PAINT_") and isinstance(v, int) for k, v in PAINT_CONSTANTS.items())):
    raise ValueError(f"{PAINT_HEADER} may declare new functions and LOC_PAINT_* integer constants only")
globals().update(PAINT_CONSTANTS)
if not os.path.exists(IBD_HEADER):
    raise FileNotFoundError(f"{IBD_HEADER} not found: it declares the entry points of the ibd command")
with open(IBD_HEADER) as _f:
    IBD_CONSTANTS, _structs, IBD_PROTOTYPES = parse(_f.read())
if (_structs or set(IBD_PROTOTYPES) & (set(PROTOTYPES) | set(EXT_PROTOTYPES) | set(REGION_PROTOTYPES) | set(NEIGHBOR_PROTOTYPES)
                                       | set(PCA_PROTOTYPES) | set(LD_PROTOTYPES) | set(SPA_PROTOTYPES) | set(ADMIX_PROTOTYPES)
                                       | set(LOCALPCA_PROTOTYPES) | set(PAINT_PROTOTYPES))
        or not all(k.startswith("LOC_IBD_") and isinstance(v, int) for k, v in IBD_CONSTANTS.items())):
    raise ValueError(f"{IBD_HEADER} may declare new functions and LOC_IBD_* integer constants only")
globals().update(IBD_CONSTANTS)
