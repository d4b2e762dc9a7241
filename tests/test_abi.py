"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/locator_hip.h declares, ctypes signatures cover them all, and the host-only layout helpers
agree with the documented swizzle.  No kernel is launched here."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from locator_amd import _abi, _lib, genotypes


def _header_symbols(repo_root):
    src = open(os.path.join(repo_root, "include", "locator_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(loc_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(repo_root):
    lib = _lib.load()
    names = _header_symbols(repo_root)
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/locator_hip.h but not exported"
    assert set(names) == set(_lib.SIGNATURES), set(names) ^ set(_lib.SIGNATURES)
    assert lib.loc_version() == 1


def test_struct_sizes_match_header():
    assert C.sizeof(_lib.Dims) == 24
    assert C.sizeof(_lib.Layout) == 14 * 8


def _struct_fields(src, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"([A-Za-z_0-9]+)\s*$", decl.strip()).group(1) for decl in body.split(";") if decl.strip()]


def test_ctypes_structs_follow_the_header_field_for_field(repo_root):
    """loc_net / loc_dims / loc_layout in include/locator_hip.h, the ctypes Structures in locator_amd/_lib.py
    and the stub shown in INTEGRATION.md must list the same fields in the same order."""
    src = open(os.path.join(repo_root, "include", "locator_hip.h")).read()
    for cname, ctype in (("loc_dims", _lib.Dims), ("loc_layout", _lib.Layout), ("loc_net", _lib.Net), ("loc_tuning", _lib.Tuning)):
        assert _struct_fields(src, cname) == [f[0] for f in ctype._fields_], cname
    doc = open(os.path.join(repo_root, "INTEGRATION.md")).read()
    stub = re.search(r"class Net\(C\.Structure\):\s*_fields_ = \[(.*?)\]\n", doc, flags=re.S).group(1)
    assert re.findall(r'\("([a-z_0-9A-Z]+)"', stub) == [f[0] for f in _lib.Net._fields_]
    tstub = re.search(r"class Tuning\(C\.Structure\): _fields_ = \[\(n, C\.c_int\) for n in \((.*?)\)\]", doc).group(1)
    assert re.findall(r'"([a-z_0-9A-Z]+)"', tstub) == [f[0] for f in _lib.Tuning._fields_]
    # pointer / int64 / int / float members only: the natural-alignment size is what both compilers produce
    assert C.sizeof(_lib.Net) % 8 == 0


def test_c_compiler_agrees_with_the_derived_structs(repo_root, tmp_path):
    """An independent witness of locator_amd/_abi.py: a C program that includes the header prints sizeof and every offsetof /
    member size of every struct in it (gcc, the host compiler build() needs for libloc_codecs.so); the ctypes classes must
    agree field by field.  The struct and member names come from this test's own reading of the header, not from _abi."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(repo_root, "include", "locator_hip.h")).read(), flags=re.S)
    structs = {}
    for name, body in re.findall(r"typedef struct (\w+) \{(.*?)\} \1;", src, flags=re.S):
        structs[name] = [re.search(r"(\w+)\s*$", piece).group(1)
                         for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
    assert list(structs) == ["loc_dims", "loc_layout", "loc_tuning", "loc_net", "loc_gb_tail", "loc_cb_state"]
    lines = ['#include <stdio.h>', '#include "locator_hip.h"', "int main(void) {"]
    for name, fields in structs.items():
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f in fields]
    lines += ["    return 0;", "}"]
    (tmp_path / "witness.c").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "witness")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I", os.path.join(repo_root, "include"), "-o", exe,
                           str(tmp_path / "witness.c")])
    seen = dict(line.split(" ", 1) for line in subprocess.check_output([exe], text=True).splitlines())
    assert set(_abi.STRUCTS) == set(structs)
    for name, fields in structs.items():
        ctype = _abi.STRUCTS[name]
        assert [f[0] for f in ctype._fields_] == fields, name
        assert int(seen[name]) == C.sizeof(ctype), name
        for f in fields:
            assert seen[f"{name}.{f}"] == f"{getattr(ctype, f).offset} {getattr(ctype, f).size}", (name, f)
    sizes = {n: int(seen[n]) for n in ("loc_dims", "loc_layout", "loc_tuning", "loc_net", "loc_cb_state")}
    assert sizes == {"loc_dims": 24, "loc_layout": 112, "loc_tuning": 40, "loc_net": 248, "loc_cb_state": 72}
    assert seen["loc_net.tune"] == "204 40"
    assert (_lib.Dims, _lib.Layout, _lib.Tuning, _lib.Net, _lib.CbState) == tuple(
        _abi.STRUCTS[n] for n in ("loc_dims", "loc_layout", "loc_tuning", "loc_net", "loc_cb_state"))


def test_prototypes_follow_the_header_rules():
    """Spot checks of each mapping rule of locator_amd/_abi.py on real entry points."""
    vp, S = C.c_void_p, _lib.SIGNATURES
    assert S is _abi.PROTOTYPES and len(S) == 89
    assert S["loc_last_error"] == (C.c_char_p, []) and S["loc_version"] == (C.c_int, [])
    assert S["loc_make_dims"] == (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(_lib.Dims)])
    assert S["loc_workspace_bn4"] == (vp, [C.POINTER(_lib.Net)])                      # float* return: a device pointer
    assert S["loc_bn_var_add"] == (C.c_float, [C.c_int])
    assert S["loc_init_uniform"] == (C.c_int, [vp, C.c_int64, C.c_float, C.c_uint64, C.c_uint64, vp])
    assert S["loc_kde_peak_batch"] == (C.c_int, [vp, vp, C.c_int, C.c_double, vp, vp, vp])
    assert S["loc_event_create"] == (C.c_int, [C.POINTER(vp)])                        # T**
    assert S["loc_event_elapsed_ms"] == (C.c_int, [vp, vp, C.POINTER(C.c_float)])     # h_ms
    assert S["loc_l1_forward_gemm_i8_partial"][1][-4:] == [C.POINTER(_lib.Tuning), C.POINTER(C.c_int), C.POINTER(vp), vp]
    assert S["loc_snapshot_if"] == (C.c_int, [vp, vp, vp, C.c_int64, vp])             # loc_cb_state*: a device pointer
    assert S["loc_stack_dw_adam_tail"][1][-2:] == [vp, vp] and len(S["loc_stack_dw_adam_tail"][1]) == 28
    assert [len(S[n][1]) for n in ("loc_l1_backward_adam", "loc_l1_backward_adam_chain")] == [31, 32]


@pytest.mark.parametrize("text", [
    "int loc_f(size_t n);",                                    # a scalar type outside the table
    "typedef struct loc_s { long n; } loc_s;",                 # ... in a struct
    "int loc_f(int n, const float*);",                         # a parameter without a name
    "int loc_f(int);",
    "int loc_f(loc_dims d);",                                  # a struct by value
    "int loc_f(int n) int loc_g(int n);",                      # two declarations before one `;`
    "static const int x = 3;",                                 # not a prototype
    "#define LOC_N (1 << 4)\n",                                # an object-like constant that is not a literal
])
def test_parser_refuses_what_it_cannot_type(text):
    head = "typedef struct loc_dims { int K, Kp; } loc_dims;\n"
    assert list(_abi.parse(head + "int loc_f(const loc_dims* d, float* h_out);")[2]) == ["loc_f"]
    with pytest.raises(ValueError):
        _abi.parse(head + text)


def test_constants_come_from_the_header():
    assert len(_abi.CONSTANTS) == 14 and all(getattr(_abi, k) == v for k, v in _abi.CONSTANTS.items())
    assert _abi.LOC_PREDICT_CHUNK == 16384 and type(_abi.LOC_PREDICT_CHUNK) is int
    assert _abi.LOC_DOSAGE_UNIT == 63 == genotypes.DOSAGE_UNIT
    assert (_abi.LOC_ROWS, _abi.LOC_MAX_WIDTH, _abi.LOC_MAX_BATCH, _abi.LOC_BIG_BATCH_MAX, _abi.LOC_BATCH_SLOT) == (32, 1024, 128, 4096, 128)
    assert (_abi.LOC_ROWS_TILE, _abi.LOC_ROWS_BLOCKS, _abi.LOC_MAX_FWD_GRID, _abi.LOC_GEMM_I8_PACKED_MIN_ROWS) == (128, 256, 512, 3072)
    assert (_abi.LOC_GUARD_FAST_MEDIAN, _abi.LOC_GUARD_FAST_MAX, _abi.LOC_GUARD_EXACT_MAX) == (64.0, 512.0, 512.0)
    lib = _lib.load()
    assert [lib.loc_gemm_min_rows(p) for p in (1, 2, 3)] == [640, 768, 1152]
    assert [lib.loc_gemm_i8_min_rows(g) for g in (2, 3)] == [512, 512]
    for width in (32, 256, 1024):
        d = _lib.make_dims(1000, width, 4)
        assert lib.loc_l1_partial_floats(C.byref(d)) == 256 * 128 * d.Hp == max(512 * 32, 256 * 128) * width


def test_header_modules_do_not_import_torch(repo_root):
    """The command line and the fork server start without torch: _abi, genotypes and locator must not pull it in."""
    code = ("import sys; import locator_amd._abi, locator_amd.genotypes, locator_amd.locator; "
            "assert 'torch' not in sys.modules, 'torch was imported'")
    subprocess.check_call([sys.executable, "-c", code], cwd=repo_root)


def test_missing_header_is_an_error_that_names_the_path(repo_root, tmp_path):
    pkg = tmp_path / "locator_amd"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "_abi.py").write_text(open(os.path.join(repo_root, "locator_amd", "_abi.py")).read())
    r = subprocess.run([sys.executable, "-c", "import locator_amd._abi"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode != 0 and os.path.join(str(tmp_path), "include", "locator_hip.h") in r.stderr


def test_an_extension_header_that_declares_what_it_may_not_is_refused_by_name(repo_root, tmp_path):
    import shutil
    pkg = tmp_path / "locator_amd"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    shutil.copy(os.path.join(repo_root, "locator_amd", "_abi.py"), pkg / "_abi.py")
    shutil.copytree(os.path.join(repo_root, "include"), tmp_path / "include")
    run = lambda: subprocess.run([sys.executable, "-c", "import locator_amd._abi"], cwd=tmp_path, capture_output=True, text=True)
    assert run().returncode == 0
    for header, addition in (("locator_hip_ibd.h", "int loc_ibs_knn(int N);"),          # a function of locator_hip_neighbors.h
                             ("locator_hip_pca.h", "int loc_version(void);"),           # a function of the main header
                             ("locator_hip_paint.h", "#define LOC_PAINT_TILE 2.5"),     # no integer
                             ("locator_hip_paint.h", "#define LOC_IBD_TILE 2"),         # a constant outside its prefix
                             ("locator_hip_query.h", "#define LOC_QUERY_TILE 64")):     # this header may declare functions only
        path = tmp_path / "include" / header
        text = path.read_text()
        path.write_text(text + "\n" + addition + "\n")
        r = run()
        assert r.returncode != 0 and "ValueError" in r.stderr and str(path) + " may declare" in r.stderr, (header, addition, r.stderr)
        path.write_text(text)


def test_dims_and_layout():
    d = _lib.make_dims(5830, 256, 10)
    assert (d.K, d.Kp, d.H, d.Hp, d.L, d.n_pre) == (5830, 5856, 256, 256, 10, 5)
    lay = _lib.param_layout(d)
    assert lay.w1 == 0 and lay.gamma == 5856 * 256 and lay.beta == lay.gamma + 5856
    assert lay.wh == lay.b1 + 256 and lay.bh == lay.wh + 9 * 256 * 256
    assert lay.n_trainable % 4 == 0 and lay.mov_var == lay.mov_mean + 5856
    assert lay.n_total == lay.mov_var + 5856
    d1 = _lib.make_dims(10, 256, 1)         # --nlayers 1: no Dense layer before the Dropout layer
    assert (d1.L, d1.n_pre) == (1, 0) and _lib.param_layout(d1).wh == _lib.param_layout(d1).bh
    d2 = _lib.make_dims(33, 100, 3)
    assert (d2.Kp, d2.Hp, d2.n_pre) == (64, 128, 1)
    with pytest.raises(_lib.LocatorHipError):
        _lib.make_dims(10, 256, 0)          # nlayers < 1
    with pytest.raises(_lib.LocatorHipError):
        _lib.make_dims(10, 1025, 4)            # LOC_MAX_WIDTH is 1024


def test_w1s_index_is_a_bijection_and_matches_mfma_layout():
    lib = _lib.load()
    Hp, Kp = 64, 96
    idx = np.array([[lib.loc_w1s_index(h, k, Hp) for k in range(Kp)] for h in range(Hp)])
    assert sorted(idx.ravel().tolist()) == list(range(Hp * Kp))
    # lane l = hi*32 + (k&31), float4 q, component c  <->  unit 8q + 4hi + c of the tile (accumulator rows)
    for (h, k) in [(0, 0), (5, 3), (37, 40), (63, 95)]:
        kt, kl, ht, hl = k >> 5, k & 31, h >> 5, h & 31
        q, hi, c = hl >> 3, (hl >> 2) & 1, hl & 3
        assert idx[h, k] == ((kt * (Hp // 32) + ht) * 4 + q) * 256 + (hi * 32 + kl) * 4 + c
    # a (k-tile, unit-tile) block is one contiguous 1024-float run
    blk = idx[32:64, 32:64]
    assert blk.min() == (1 * 2 + 1) * 1024 and blk.max() == blk.min() + 1023


def test_codecs_library_loads_and_exports_its_entry_points(repo_root):
    """libloc_codecs.so (csrc/codecs.c, host-side Blosc-1 / LZ4 chunk decoder of the zarr reader)."""
    lib = C.CDLL(os.path.join(repo_root, "locator_amd", "libloc_codecs.so"))
    for name in ("loc_lz4_decompress", "loc_blosc1_decompress", "loc_blosc1_info"):
        assert hasattr(lib, name), name


def test_train_chain_supported_is_decided_by_shape_alone():
    """loc_train_chain_supported is host logic over the loc_net fields (no kernel, no device memory): width padding to
    64, 128, 256 or 512, at least one hidden layer, batch <= 32, Dropout not on the BatchNorm output, 16-byte row pitch, and the chained
    kernel's 32-bit byte offsets (Kp * max(Hp, 256) * 4 < 2^32: just under 4.2 million SNPs, 2.1 million at width 512)."""
    lib = _lib.load()

    def net(K=100000, width=256, nlayers=10, drop=0.25, slot_rows=32, pitch=None, wht=1, grid=512):
        n = _lib.Net()
        n.d = _lib.make_dims(K, width, nlayers)
        n.drop_p = drop
        n.wht = wht                                # only tested for NULL here
        n.slot_rows, n.l1_bwd_grid = slot_rows, grid
        n.x_pitch = n.d.Kp if pitch is None else pitch
        return n

    ok = lambda **kw: bool(lib.loc_train_chain_supported(C.byref(net(**kw))))
    assert ok() and ok(width=225) and ok(nlayers=2) and ok(drop=0.0) and ok(K=31)
    assert ok(width=64) and ok(width=33) and ok(width=128) and ok(width=97)        # round 4: 2 and 4 unit tiles
    assert ok(width=512) and ok(width=481)                                         # ... and 16 (two per wave)
    assert not ok(width=224) and not ok(width=257) and not ok(width=32) and not ok(width=513) and not ok(width=1024)
    assert not ok(nlayers=1) and ok(nlayers=1, drop=0.0) is False
    assert not ok(slot_rows=128)                                     # --batch_size > 64
    assert ok(slot_rows=64) and not ok(slot_rows=64, width=128) and not ok(slot_rows=64, width=512)   # 33..64: two row blocks, width 256 only
    assert not ok(wht=None)                                          # no fused hidden stack
    assert not ok(pitch=100008)                                      # rows not 16-byte aligned
    assert ok(K=4194240) and not ok(K=4194304)                       # Kp * 1024 < 2^32
    assert ok(width=512, K=2097120) and not ok(width=512, K=2097152)  # width 512: Kp * 2048 < 2^32
    assert ok(width=128, K=4194240) and ok(width=64, K=4194240) and not ok(width=64, K=4194304)   # narrower: the width-256 limit
    assert ok(nlayers=3) and ok(nlayers=2, drop=0.25)                # Dropout after layer 1 is fine (n_pre = 1), only n_pre = 0 is not
