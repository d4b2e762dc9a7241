"""What every command's header test asserts about its line of locator_amd._abi's table: the test states the prototypes and the
constants, check_extension compares them with the header's text, the table's entry and the loaded library."""
import os
import re

from locator_amd import _abi, _lib

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADERS = {"ext": "locator_hip_query.h", "region": "locator_hip_regions.h", "neighbor": "locator_hip_neighbors.h",
           "pca": "locator_hip_pca.h", "ld": "locator_hip_ld.h", "spa": "locator_hip_spa.h", "admix": "locator_hip_admix.h",
           "localpca": "locator_hip_localpca.h", "paint": "locator_hip_paint.h", "ibd": "locator_hip_ibd.h",
           "impute": "locator_hip_impute.h"}


def check_extension(tag, prototypes, constants):
    """prototypes: {name: (restype, [argtypes])}, every function of the header spelled out.  constants: the exact {name: value},
    or the set of names where the test pins no values."""
    assert list(_abi.EXTENSIONS) == list(HEADERS)
    ext = _abi.EXTENSIONS[tag]
    assert ext.header == os.path.join(INCLUDE, HEADERS[tag])
    src = re.sub(r"/\*.*?\*/", "", open(ext.header).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(loc_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(prototypes) == sorted(ext.prototypes)
    assert ext.prototypes == prototypes
    assert ext.constants == constants if isinstance(constants, dict) else set(ext.constants) == constants
    assert all(type(v) is int and v > 0 and getattr(_abi, k) == v for k, v in ext.constants.items())
    others = [(_abi.CONSTANTS, _abi.PROTOTYPES)] + [(o.constants, o.prototypes) for t, o in _abi.EXTENSIONS.items() if t != tag]
    for consts, protos in others:
        assert not set(names) & set(protos) and not set(ext.constants) & set(consts)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert _abi.ALL_PROTOTYPES[name] == prototypes[name]
        assert fn.restype is prototypes[name][0] and list(fn.argtypes) == prototypes[name][1]
