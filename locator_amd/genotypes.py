"""Genotype ingest and SNP filtering for the locator path, without scikit-allel / zarr / h5py.

Mirrors /root/reference/locator/locator.py:187-281 (load_genotypes, replace_md, filter_snps).
The reference delegates to scikit-allel (`read_vcf`, `GenotypeArray.count_alleles / is_biallelic /
to_allele_counts / is_missing`) and zarr; neither is available on the target, so the small subset
of their behaviour that the path relies on is implemented here on plain NumPy:

  genotypes : int8 array (variants, samples, ploidy=2), -1 = missing allele  (allel.GenotypeArray)
  count_alleles()[:, a]      number of called alleles equal to a, per variant
  is_biallelic()             exactly two distinct alleles observed at the variant
  to_allele_counts()[:,:,1]  per-sample count of allele 1 (missing alleles count as 0)
  is_missing()               any allele of the call is < 0
"""
from __future__ import annotations

import gzip
import json
import os
import struct
import zlib

import numpy as np

from . import _abi


# ------------------------------------------------------------------ VCF
def _parse_gt_fast(fields, n, seps=None):
    """All calls are single-digit diploid 'a|b' / 'a/b' with GT the only (or first) FORMAT key.  seps: a list that gets
    the separator bytes of the line (124 '|', 47 '/') appended."""
    s = "\t".join(fields)
    if len(s) != 4 * n - 1:
        return None
    arr = np.frombuffer((s + "\t").encode("ascii"), dtype=np.uint8).reshape(n, 4)
    sep = arr[:, 1]
    if not np.all((sep == 124) | (sep == 47)) or not np.all(arr[:, 3] == 9):
        return None
    out = np.empty((n, 2), np.int8)
    for j, col in enumerate((0, 2)):
        c = arr[:, col]
        digit = (c >= 48) & (c <= 57)
        if not np.all(digit | (c == 46)):
            return None
        out[:, j] = np.where(digit, c.astype(np.int16) - 48, -1).astype(np.int8)
    if seps is not None:
        seps.append(sep)
    return out


def _parse_gt_slow(fields, n, seps=None):
    out = np.full((n, 2), -1, np.int8)
    sep = np.full(n, 124, np.uint8)
    for i, f in enumerate(fields):
        raw = f.split(":", 1)[0]
        if "/" in raw:
            sep[i] = 47
        gt = raw.replace("|", "/").split("/")
        for j, a in enumerate(gt[:2]):
            if a != "." and a != "":
                out[i, j] = int(a)
        if len(gt) == 1:            # haploid call: second allele stays missing (-1), as allel pads
            out[i, 1] = -1
    if seps is not None:
        seps.append(sep)
    return out


def unphased_hets(gt, sep):
    """Heterozygous calls written unphased: both alleles called, different, separator '/' (47).  gt (..., 2) int8,
    sep (...) uint8 -> count."""
    a, b = gt[..., 0], gt[..., 1]
    return int(np.count_nonzero((sep == 47) & (a >= 0) & (b >= 0) & (a != b)))


def read_vcf(path, phase=False, sites=False):
    """Subset of allel.read_vcf used by locator.py:195-199: returns dict with 'calldata/GT'
    (variants, samples, 2) int8, 'samples' (object array of str) and 'variants/POS' (int32).  phase=True (--phased) adds
    'unphased_hets': the number of heterozygous calls written with '/' (their two alleles have no order).  sites=True
    (--keep_model, locator_amd.predict) adds 'variants/CHROM' and 'variants/REF' (object arrays of str) and 'variants/ALT'
    (variants, max ALT count) object array of str padded with '' as allel lays it out."""
    opener = gzip.open if str(path).endswith(".gz") else open
    samples, gts, pos = None, [], []
    chrom, ref, alt = [], [], []
    unphased = 0
    seps = [] if phase else None
    with opener(path, "rt") as fh:
        for line in fh:
            if line.startswith("##"):
                continue
            line = line.rstrip("\n")
            if line.startswith("#CHROM"):
                samples = np.array(line.split("\t")[9:], dtype=object)
                continue
            if not line:
                continue
            f = line.split("\t")
            n = len(f) - 9
            fmt = f[8]
            g = None
            if fmt == "GT":
                g = _parse_gt_fast(f[9:], n, seps)
            if g is None:
                if fmt.split(":")[0] != "GT":
                    raise ValueError("VCF FORMAT must start with GT")
                g = _parse_gt_slow(f[9:], n, seps)
            if phase:
                unphased += unphased_hets(g, seps.pop())
            gts.append(g)
            pos.append(int(f[1]))
            if sites:
                chrom.append(f[0])
                ref.append(f[3])
                alt.append([] if f[4] == "." else f[4].split(","))
    if samples is None:
        raise ValueError(f"{path}: no #CHROM header line")
    gt = np.stack(gts, axis=0) if gts else np.zeros((0, len(samples), 2), np.int8)
    out = {"calldata/GT": gt, "samples": samples, "variants/POS": np.asarray(pos, dtype=np.int32)}
    if phase:
        out["unphased_hets"] = unphased
    if sites:
        out["variants/CHROM"] = np.array(chrom, dtype=object)
        out["variants/REF"] = np.array(ref, dtype=object)
        table = np.full((len(alt), max([1] + [len(a) for a in alt])), "", dtype=object)
        for i, a in enumerate(alt):
            table[i, :len(a)] = a
        out["variants/ALT"] = table
    return out


def zarr_unphased_hets(callset):
    """--phased on a zarr store: heterozygous calls flagged unphased by a `calldata/GT_phased` array (variants, samples)
    of bools, as `allel.vcf_to_zarr` writes it when asked for that field.  None when the store has no such array or this
    reader cannot read it (the store is then taken as phased).  Reads the flags a chunk of variants at a time and the
    calls only where a flag is False."""
    try:
        ph = callset["calldata/GT_phased"]
        if len(ph.shape) != 2 or np.dtype(ph.dtype) != np.bool_:
            return None
        gt = callset["calldata/GT"]
        step = max(1, int(ph.chunks[0]))
        n = 0
        for a in range(0, ph.shape[0], step):
            flags = np.asarray(ph[a:a + step])
            if flags.all():
                continue
            g = np.asarray(gt[a:a + step])
            het = (g[:, :, 0] >= 0) & (g[:, :, 1] >= 0) & (g[:, :, 0] != g[:, :, 1])
            n += int(np.count_nonzero(het & ~flags))
        return n
    except (KeyError, ValueError, OSError, IndexError):
        return None


# ------------------------------------------------------------------ zarr v2 directory store
_CODECS = None


def _codecs():
    """libloc_codecs.so (locator_amd/csrc/codecs.c): the Blosc-1 / LZ4 chunk decoder, built with the HIP library."""
    global _CODECS
    if _CODECS is None:
        import ctypes as C
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libloc_codecs.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found: build it with `make -C locator_amd/csrc` (blosc-compressed zarr "
                               "chunks cannot be read without it)")
        lib = C.CDLL(path)
        lib.loc_blosc1_decompress.restype = C.c_int64
        lib.loc_blosc1_decompress.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int]
        lib.loc_blosc1_info.restype = C.c_int
        lib.loc_blosc1_info.argtypes = [C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]
        lib.loc_lz4_decompress.restype = C.c_int64
        lib.loc_lz4_decompress.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_int64]
        lib.loc_zstd_available.restype = C.c_int
        lib.loc_zstd_decompress.restype = C.c_int64
        lib.loc_zstd_decompress.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_int64]
        lib.loc_zstd_compress.restype = C.c_int64
        lib.loc_zstd_compress.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int]
        lib.loc_snp_flags.restype = C.c_int64
        lib.loc_snp_flags.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
        lib.loc_snp_allele_counts.restype = None
        lib.loc_snp_allele_counts.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p]
        lib.loc_rows_transposed.restype = None
        lib.loc_rows_transposed.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                            C.c_int64]
        _CODECS = lib
    return _CODECS


NO_ZSTD = ("this store's chunks are zstd-compressed and libzstd.so.1 was not found on this machine; install the zstd "
           "runtime library (libzstd1) or re-encode the store with Blosc(cname='lz4') / zlib")


def zstd_available():
    return bool(_codecs().loc_zstd_available())


def zstd_decompress(raw, nbytes):
    """One zstd frame of known decoded size (the numcodecs `zstd` compressor; also the payload of Blosc codec 4)."""
    out = np.empty(max(int(nbytes), 1), np.uint8)
    r = _codecs().loc_zstd_decompress(bytes(raw), len(raw), out.ctypes.data, int(nbytes))
    if r == -5:
        raise RuntimeError(NO_ZSTD)
    if r != nbytes:
        raise ValueError("malformed zstd chunk")
    return out[:nbytes].tobytes()


def zstd_compress(raw, level=3):
    """Writer side, for test / synthetic stores only."""
    raw = bytes(raw)
    out = np.empty(len(raw) + len(raw) // 128 + 256, np.uint8)
    r = _codecs().loc_zstd_compress(raw, len(raw), out.ctypes.data, out.size, int(level))
    if r == -5:
        raise RuntimeError(NO_ZSTD)
    if r < 0:
        raise ValueError("zstd compression failed")
    return out[:r].tobytes()


def blosc_decompress(raw):
    """One Blosc-1 chunk (what numcodecs.Blosc / `allel.vcf_to_zarr` write by default: LZ4, byte-shuffle) -> bytes.
    Codecs: lz4 / lz4hc, zlib, zstd (through the system's libzstd), stored; filters: byte-shuffle.  blosclz /
    bit-shuffle raise."""
    import ctypes as C
    lib = _codecs()
    info = (C.c_int64 * 5)()
    if lib.loc_blosc1_info(raw, len(raw), info) != 0:
        raise ValueError("blosc chunk shorter than its header")
    nbytes, blocksize = int(info[0]), int(info[1])
    out = np.empty(nbytes, np.uint8)
    tmp = np.empty(max(blocksize, 1), np.uint8)
    for mode in (0, 1, 2):            # as the header says; then the two split conventions of writers that do not say
        r = lib.loc_blosc1_decompress(raw, len(raw), out.ctypes.data, nbytes, tmp.ctypes.data, mode)
        if r == nbytes:
            return out.tobytes()
        if r == -5:
            raise RuntimeError(NO_ZSTD)
        if r in (-2, -3):
            what = "codec (supported: lz4, zlib, zstd, stored)" if r == -2 else "filter bit-shuffle"
            raise ValueError(f"blosc chunk uses an unsupported {what}; re-encode the store with "
                             "Blosc(cname='lz4') or zlib")
    raise ValueError("malformed blosc chunk")


def _lz4_compress_block(data):
    """Greedy LZ4 block encoder (hash of 4-byte windows, one candidate per hash).  Only used to WRITE small
    synthetic / test stores in the format real tools produce; the reader side is csrc/codecs.c."""
    n = len(data)
    out = bytearray()
    table = {}
    i = anchor = 0
    limit = n - 12                              # format rule: the last match starts >= 12 bytes before the end
    while i < limit:
        key = data[i:i + 4]
        cand = table.get(key)
        table[key] = i
        if cand is not None and i - cand <= 65535:
            m = 4
            end = n - 5                         # and the last 5 bytes are literals
            while i + m < end and data[cand + m] == data[i + m]:
                m += 1
            lit = i - anchor
            token = (min(lit, 15) << 4) | min(m - 4, 15)
            out.append(token)
            if lit >= 15:
                r = lit - 15
                while r >= 255:
                    out.append(255)
                    r -= 255
                out.append(r)
            out += data[anchor:i]
            out += (i - cand).to_bytes(2, "little")
            if m - 4 >= 15:
                r = m - 4 - 15
                while r >= 255:
                    out.append(255)
                    r -= 255
                out.append(r)
            i += m
            anchor = i
        else:
            i += 1
    lit = n - anchor
    out.append(min(lit, 15) << 4)
    if lit >= 15:
        r = lit - 15
        while r >= 255:
            out.append(255)
            r -= 255
        out.append(r)
    out += data[anchor:]
    return bytes(out)


def blosc_compress(raw, typesize=1, shuffle=True, blocksize=1 << 16, cname="lz4"):
    """Blosc-1 chunk with LZ4 (or zstd) streams and byte-shuffle, laid out as c-blosc writes it (16-byte header, block
    offsets, per-stream {int32 size, data}, split into `typesize` streams when the block is large enough)."""
    raw = bytes(raw)
    nbytes = len(raw)
    typesize = max(1, int(typesize))
    blocksize = max(typesize, min(blocksize, nbytes) // typesize * typesize) if nbytes else typesize
    do_shuffle = shuffle and typesize > 1
    flags = ({"lz4": 1, "zstd": 4}[cname] << 5) | (1 if do_shuffle else 0)
    nblocks = (nbytes + blocksize - 1) // blocksize if nbytes else 0
    body, starts = bytearray(), []
    pos = 16 + 4 * nblocks
    for b in range(nblocks):
        blk = raw[b * blocksize:(b + 1) * blocksize]
        leftover = len(blk) != blocksize
        if do_shuffle:
            ne = len(blk) // typesize
            arr = np.frombuffer(blk[:ne * typesize], np.uint8).reshape(ne, typesize).T.tobytes() + blk[ne * typesize:]
        else:
            arr = blk
        split = typesize > 1 and typesize <= 16 and blocksize // typesize >= 128 and not leftover
        ns = typesize if split else 1
        ss = len(arr) // ns
        starts.append(pos)
        for k in range(ns):
            stream = arr[k * ss:(k + 1) * ss]
            comp = _lz4_compress_block(stream) if cname == "lz4" else zstd_compress(stream)
            if len(comp) >= len(stream):
                comp = stream                                    # stored
            body += len(comp).to_bytes(4, "little") + comp
            pos += 4 + len(comp)
    head = bytes([2, 1, flags, typesize]) + nbytes.to_bytes(4, "little") + blocksize.to_bytes(4, "little") + \
        (16 + 4 * nblocks + len(body)).to_bytes(4, "little")
    return head + b"".join(x.to_bytes(4, "little") for x in starts) + bytes(body)


class ZarrArray:
    """Read-only zarr-v2 array in a directory store.  Compressors: none, zlib, gzip and blosc (the default of
    `allel.vcf_to_zarr`, scripts/vcf_to_zarr.py:12: Blosc-1 container with LZ4 / zlib payloads and byte-shuffle,
    decoded by csrc/codecs.c).  Filters: vlen-utf8 (object string arrays)."""

    def __init__(self, path):
        self.path = path
        with open(os.path.join(path, ".zarray")) as fh:
            meta = json.load(fh)
        if meta.get("zarr_format") != 2:
            raise ValueError(f"{path}: only zarr_format 2 is supported")
        self.shape = tuple(meta["shape"])
        self.chunks = tuple(meta["chunks"])
        self.dtype = np.dtype(meta["dtype"])
        self.order = meta.get("order", "C")
        self.fill_value = meta.get("fill_value")
        self.compressor = meta.get("compressor")
        self.filters = meta.get("filters") or []
        self.sep = meta.get("dimension_separator", ".")
        self.ndim = len(self.shape)
        self.vlen_utf8 = any(f.get("id") == "vlen-utf8" for f in self.filters)
        if self.compressor is not None and self.compressor.get("id") not in ("zlib", "gzip", "blosc", "zstd"):
            raise ValueError(f"{path}: compressor {self.compressor.get('id')!r} is not supported here "
                             "(supported: null, zlib, gzip, blosc, zstd)")

    def __len__(self):
        return self.shape[0]

    def _decode(self, raw, cshape):
        if self.compressor is not None and self.compressor.get("id") == "blosc":
            raw = blosc_decompress(raw)
        elif self.compressor is not None and self.compressor.get("id") == "zstd":
            if self.vlen_utf8:
                raise ValueError(f"{self.path}: zstd-compressed string arrays are not supported")
            raw = zstd_decompress(raw, int(np.prod(cshape)) * self.dtype.itemsize)
        elif self.compressor is not None:
            raw = zlib.decompress(raw, 15 + 32)        # auto-detect zlib / gzip framing
        if self.vlen_utf8:
            n = struct.unpack_from("<I", raw, 0)[0]
            out = np.empty(n, dtype=object)
            off = 4
            for i in range(n):
                ln = struct.unpack_from("<I", raw, off)[0]
                off += 4
                out[i] = raw[off:off + ln].decode("utf-8")
                off += ln
            return out.reshape(cshape, order=self.order)
        return np.frombuffer(raw, dtype=self.dtype).reshape(cshape, order=self.order)

    def _chunk(self, idx):
        fn = os.path.join(self.path, self.sep.join(str(i) for i in idx))
        if not os.path.exists(fn):
            fill = 0 if self.fill_value is None else self.fill_value
            return np.full(self.chunks, fill, dtype=object if self.vlen_utf8 else self.dtype)
        with open(fn, "rb") as fh:
            return self._decode(fh.read(), self.chunks)

    def __getitem__(self, key):
        """Supports a[:], a[a:b] and a[a:b, :, :] (slicing on the first axis only)."""
        if isinstance(key, tuple):
            if any(k != slice(None) for k in key[1:]):
                raise IndexError("ZarrArray: only the first axis can be sliced")
            key = key[0]
        if not isinstance(key, slice):
            raise IndexError("ZarrArray: use a slice")
        start, stop, step = key.indices(self.shape[0])
        if step != 1:
            raise IndexError("ZarrArray: step must be 1")
        n0 = max(stop - start, 0)
        out = np.empty((n0,) + self.shape[1:], dtype=object if self.vlen_utf8 else self.dtype)
        if n0 == 0:
            return out
        c0 = self.chunks[0]
        grid = [range((s + c - 1) // c) for s, c in zip(self.shape[1:], self.chunks[1:])]
        for ci in range(start // c0, (stop - 1) // c0 + 1):
            lo, hi = max(start, ci * c0), min(stop, (ci + 1) * c0)

            def rec(prefix, dims):
                if not dims:
                    ch = self._chunk((ci,) + tuple(prefix))
                    sl = [slice(lo - ci * c0, hi - ci * c0)]
                    dst = [slice(lo - start, hi - start)]
                    for ax, j in enumerate(prefix):
                        c = self.chunks[ax + 1]
                        a, b = j * c, min((j + 1) * c, self.shape[ax + 1])
                        sl.append(slice(0, b - a))
                        dst.append(slice(a, b))
                    out[tuple(dst)] = ch[tuple(sl)]
                    return
                for j in dims[0]:
                    rec(prefix + [j], dims[1:])

            rec([], grid)
        return out

    def read_into(self, out, start, stop, threads=4):
        """out[...] = self[start:stop] for a caller-owned array (e.g. a view of pinned memory that is uploaded as it is:
        the --windows loop, locator.py:539).  Uncompressed chunks that span the trailing axes are read straight from the
        file into `out` (one copy, page cache -> destination); compressed chunks are decoded on `threads` threads (the
        C codecs release the GIL) and copied in."""
        start, stop, _ = slice(start, stop).indices(self.shape[0])
        n0 = max(stop - start, 0)
        if tuple(out.shape) != (n0,) + tuple(self.shape[1:]) or out.dtype != self.dtype or not out.flags.c_contiguous:
            raise ValueError("read_into: `out` must be a C-contiguous array of the slice's shape and dtype")
        if n0 == 0:
            return out
        c0 = self.chunks[0]
        whole = tuple(self.chunks[1:]) == tuple(self.shape[1:]) and self.order == "C" and not self.vlen_utf8
        if not whole:
            out[...] = self[start:stop]
            return out
        row = int(np.prod(self.shape[1:], dtype=np.int64)) * self.dtype.itemsize
        flat = out.reshape(n0, -1).view(np.uint8).reshape(-1)
        tail = (0,) * (self.ndim - 1)

        def one(ci):
            lo, hi = max(start, ci * c0), min(stop, (ci + 1) * c0)
            dst = memoryview(flat)[(lo - start) * row:(hi - start) * row]
            fn = os.path.join(self.path, self.sep.join(str(i) for i in (ci,) + tail))
            if not os.path.exists(fn):
                np.frombuffer(dst, dtype=np.uint8)[...] = 0 if self.fill_value is None else self.fill_value
            elif self.compressor is None:
                with open(fn, "rb", buffering=0) as fh:
                    fh.seek((lo - ci * c0) * row)
                    got, want = 0, len(dst)
                    while got < want:
                        k = fh.readinto(dst[got:])
                        if not k:
                            raise IOError(f"{fn}: chunk shorter than its shape")
                        got += k
            else:
                with open(fn, "rb") as fh:
                    ch = self._decode(fh.read(), self.chunks)
                np.frombuffer(dst, dtype=self.dtype).reshape((hi - lo,) + tuple(self.shape[1:]))[...] = ch[lo - ci * c0:hi - ci * c0]

        cis = list(range(start // c0, (stop - 1) // c0 + 1))
        if len(cis) > 1 and threads > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(min(threads, len(cis))) as ex:
                list(ex.map(one, cis))
        else:
            for ci in cis:
                one(ci)
        return out

    def __array__(self, dtype=None, copy=None):
        a = self[:]
        return a.astype(dtype) if dtype is not None else a


class ZarrGroup:
    """`zarr.open_group(path, mode='r')` stand-in: group['calldata/GT'] -> ZarrArray."""

    def __init__(self, path):
        if not os.path.isdir(path):
            raise FileNotFoundError(path)
        self.path = path

    def __getitem__(self, key):
        p = os.path.join(self.path, *key.split("/"))
        if os.path.exists(os.path.join(p, ".zarray")):
            return ZarrArray(p)
        if os.path.isdir(p):
            return ZarrGroup(p)
        raise KeyError(key)

    def __iter__(self):
        """Member names (arrays and sub-groups: the sub-directories, as __getitem__ opens them) in sorted order, as
        `zarr` lists a group's keys."""
        for name in sorted(os.listdir(self.path)):
            if not name.startswith(".") and os.path.isdir(os.path.join(self.path, name)):
                yield name


def open_group(path, mode="r"):
    return ZarrGroup(path)


def walk_outlines(path):
    """Every [2][n] lon / lat outline of a zarr-v2 map store, as (region, part, lon, lat) float64 in the store's iteration
    order.  A nested store `Country/Part` gives one region per top-level group and one part per array of it; in a flat
    store each top-level array is a region of one part, named as the region.  The one walk that plot.read_basemap (to
    draw) and regions.read_map (to assign) share."""
    store = ZarrGroup(path)
    for region in store:
        node = store[region]
        members = [(region, node)] if isinstance(node, ZarrArray) else [(m, node[m]) for m in node]
        for part, arr in members:
            if isinstance(arr, ZarrArray):
                xy = np.asarray(arr[:], dtype=np.float64)
                yield region, part, xy[0], xy[1]


def write_zarr_array(path, arr, chunks, compressor=None):
    """Minimal zarr-v2 writer (uncompressed, zlib, "blosc" = Blosc-1 / LZ4 / byte-shuffle as `allel.vcf_to_zarr` writes
    by default, "blosc-zstd" = the same container with zstd streams, "zstd" = numcodecs' plain zstd frames) used to
    build synthetic stores (config 4) and test fixtures."""
    arr = np.asarray(arr)
    os.makedirs(path, exist_ok=True)
    chunks = tuple(int(min(c, s)) if s else 1 for c, s in zip(chunks, arr.shape))
    meta = {"zarr_format": 2, "shape": list(arr.shape), "chunks": list(chunks), "dtype": arr.dtype.str,
            "compressor": {None: None, "zlib": {"id": "zlib", "level": 1},
                           "blosc": {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0},
                           "blosc-zstd": {"id": "blosc", "cname": "zstd", "clevel": 5, "shuffle": 1, "blocksize": 0},
                           "zstd": {"id": "zstd", "level": 3}}[compressor], "fill_value": 0,
            "order": "C", "filters": None}
    with open(os.path.join(path, ".zarray"), "w") as fh:
        json.dump(meta, fh)
    ranges = [range((s + c - 1) // c) for s, c in zip(arr.shape, chunks)]
    import itertools
    for idx in itertools.product(*ranges):
        sl = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, chunks, arr.shape))
        block = np.zeros(chunks, arr.dtype)
        block[tuple(slice(0, s.stop - s.start) for s in sl)] = arr[sl]
        raw = block.tobytes()
        if compressor == "zlib":
            raw = zlib.compress(raw, 1)
        elif compressor == "blosc":
            raw = blosc_compress(raw, arr.dtype.itemsize)
        elif compressor == "blosc-zstd":
            raw = blosc_compress(raw, arr.dtype.itemsize, cname="zstd")
        elif compressor == "zstd":
            raw = zstd_compress(raw)
        with open(os.path.join(path, ".".join(map(str, idx))), "wb") as fh:
            fh.write(raw)


def write_callset_zarr(path, gt, pos, samples, chunk_variants=65536, compressor=None, chrom=None, ref=None, alt=None):
    """Synthetic `allel.vcf_to_zarr`-shaped store: calldata/GT, variants/POS, samples, and variants/CHROM / REF / ALT
    (fixed-width unicode; ALT may be 2-D, one column per alternate allele) when given."""
    os.makedirs(path, exist_ok=True)
    for g in ("", "calldata", "variants"):
        os.makedirs(os.path.join(path, g), exist_ok=True)
        with open(os.path.join(path, g, ".zgroup"), "w") as fh:
            json.dump({"zarr_format": 2}, fh)
    gt = np.asarray(gt, dtype=np.int8)
    write_zarr_array(os.path.join(path, "calldata", "GT"), gt, (chunk_variants, gt.shape[1], 2), compressor)
    write_zarr_array(os.path.join(path, "variants", "POS"), np.asarray(pos, np.int32), (chunk_variants,), compressor)
    s = np.asarray(samples)
    write_zarr_array(os.path.join(path, "samples"), s.astype("U"), (len(s),), None)
    for name, col in (("CHROM", chrom), ("REF", ref), ("ALT", alt)):
        if col is not None:
            col = np.asarray(col).astype("U")
            write_zarr_array(os.path.join(path, "variants", name), col, (chunk_variants,) + col.shape[1:], compressor)


def zarr_sites(callset):
    """variants/CHROM, POS, REF, ALT of a zarr store (allel.vcf_to_zarr layout; ALT (variants, numalt) or 1-D) as the dict
    read_vcf(sites=True) returns.  Raises KeyError naming the first array the store lacks."""
    out = {}
    for name in ("CHROM", "POS", "REF", "ALT"):
        try:
            a = np.asarray(callset["variants/" + name][:])
        except KeyError:
            raise KeyError(f"variants/{name}") from None
        if name == "POS":
            out["variants/POS"] = a.astype(np.int64)
            continue
        a = a.astype(str).astype(object)
        if name == "ALT" and a.ndim == 1:
            a = a[:, None]
        out["variants/" + name] = a
    return out


def site_columns(d):
    """read_vcf(sites=True) / zarr_sites dict -> {chrom, pos, ref, alt}: ALT[0] of each variant."""
    alt = np.asarray(d["variants/ALT"], dtype=object)
    return {"chrom": np.asarray(d["variants/CHROM"], dtype=object).astype(str),
            "pos": np.asarray(d["variants/POS"], dtype=np.int64),
            "ref": np.asarray(d["variants/REF"], dtype=object).astype(str),
            "alt": (alt[:, 0] if alt.ndim == 2 else alt).astype(str)}


def matrix_sites(path):
    """The column names of a --matrix file after 'sampleID': the identities of its sites."""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rt") as fh:
        header = fh.readline().rstrip("\n").split("\t")
    return np.array([h.strip('"') for h in header if h.strip('"') != "sampleID"], dtype=object)


def site_af(gt, idx, chunk=65536):
    """Allele-1 frequency over the called alleles of every row, of the variants gt[idx] (the kept sites of a fit)."""
    idx = np.asarray(idx, dtype=np.int64)
    out = np.zeros(len(idx), np.float64)
    for a in range(0, len(idx), chunk):
        g = np.asarray(gt[idx[a:a + chunk]]).reshape(min(chunk, len(idx) - a), -1)
        called = np.count_nonzero(g >= 0, axis=1)
        out[a:a + chunk] = np.count_nonzero(g == 1, axis=1) / np.maximum(called, 1)
    return out


# ------------------------------------------------------------------ tab-delimited count matrix
def read_matrix(path):
    """locator.py:200-227: first column 'sampleID', then one column per site holding 0/1/2 counts.
    The reference turns count c into haplotypes (1 if c>=1, 1 if c==2) and re-counts; other values
    contribute nothing.  Returns the equivalent (variants, samples, 2) int8 genotype array."""
    import pandas as pd
    gmat = pd.read_csv(path, sep="\t")
    samples = np.array(gmat["sampleID"])
    g = np.array(gmat.drop(labels="sampleID", axis=1), dtype="int8")      # samples x sites
    h1 = ((g == 1) | (g == 2)).astype(np.int8)
    h2 = (g == 2).astype(np.int8)
    gt = np.stack([h1.T, h2.T], axis=2)
    return gt, samples


# ------------------------------------------------------------------ --dosage
DOSAGE_UNIT = _abi.LOC_DOSAGE_UNIT          # 63: q = rint(fp32(d) * 63), 0..126
Q_MISSING = 255           # host form of a missing value in a q matrix (variants, samples)
DOSAGE_LO, DOSAGE_HI = -0.001, 2.001      # accepted range of an input dosage; clamped to [0, 2] after the check


def _dosage_value(tok, field):
    """One sample's DS or GP subfield -> dosage as a Python float (NaN = missing)."""
    if tok == "" or tok == ".":
        return float("nan")
    if field == "DS":
        return float(tok)
    gp = tok.split(",")
    if len(gp) != 3:
        if all(g == "." for g in gp):
            return float("nan")
        raise ValueError(f"GP holds {len(gp)} values (3 expected for a diploid biallelic call)")
    if any(g == "." for g in gp):
        return float("nan")
    return float(gp[1]) + 2.0 * float(gp[2])


def read_vcf_dosage(path, field="DS", sites=False):
    """--dosage: the expected alt-allele dosage of every call from FORMAT/DS, or from FORMAT/GP as GP1 + 2 GP2, at the field's
    position in each record's FORMAT (which may differ from record to record).  '.' = missing (NaN).  Records with more than
    one ALT allele are dropped (their number is returned as 'multiallelic_dropped').  A record without the field, or a value
    outside [-0.001, 2.001], raises ValueError naming the record and the sample; values are clamped to [0, 2] after that check.
    Returns {'calldata/DS': float32 (variants, samples), 'samples', 'variants/POS', 'multiallelic_dropped'}.  sites=True
    (locator_amd.predict --dosage) adds 'variants/CHROM', 'variants/REF' and 'variants/ALT' (object arrays of str, one entry
    per kept record; ALT '' where the record has none)."""
    if field not in ("DS", "GP"):
        raise ValueError(f"--dosage takes DS or GP (got {field!r})")
    opener = gzip.open if str(path).endswith(".gz") else open
    samples, rows, pos = None, [], []
    chrom, ref, alt = [], [], []
    dropped = 0
    with opener(path, "rt") as fh:
        for line in fh:
            if line.startswith("##"):
                continue
            line = line.rstrip("\n")
            if line.startswith("#CHROM"):
                samples = np.array(line.split("\t")[9:], dtype=object)
                continue
            if not line:
                continue
            f = line.split("\t")
            where = f"{path}: record {f[0]}:{f[1]}"
            if "," in f[4]:
                dropped += 1
                continue
            keys = f[8].split(":") if len(f) > 8 else []
            if field not in keys:
                raise ValueError(f"{where} has no FORMAT/{field} (FORMAT is {f[8] if len(f) > 8 else 'absent'})")
            at = keys.index(field)
            vals = np.empty(len(f) - 9, np.float64)
            for i, cell in enumerate(f[9:]):
                sub = cell.split(":")
                try:
                    vals[i] = _dosage_value(sub[at] if at < len(sub) else ".", field)
                except ValueError as e:
                    raise ValueError(f"{where}, sample {samples[i] if samples is not None else i}: {field} {cell!r}: {e}") \
                        from None
            bad = ~np.isnan(vals) & ((vals < DOSAGE_LO) | (vals > DOSAGE_HI))
            if bad.any():
                i = int(np.flatnonzero(bad)[0])
                raise ValueError(f"{where}, sample {samples[i] if samples is not None else i}: dosage {vals[i]:g} from "
                                 f"{field} is outside [{DOSAGE_LO}, {DOSAGE_HI}]")
            rows.append(np.clip(vals, 0.0, 2.0).astype(np.float32))
            pos.append(int(f[1]))
            if sites:
                chrom.append(f[0])
                ref.append(f[3])
                alt.append("" if f[4] == "." else f[4])
    if samples is None:
        raise ValueError(f"{path}: no #CHROM header line")
    ds = np.stack(rows, axis=0) if rows else np.zeros((0, len(samples)), np.float32)
    out = {"calldata/DS": ds, "samples": samples, "variants/POS": np.asarray(pos, dtype=np.int32),
           "multiallelic_dropped": dropped}
    if sites:
        out["variants/CHROM"] = np.array(chrom, dtype=object)
        out["variants/REF"] = np.array(ref, dtype=object)
        out["variants/ALT"] = np.array(alt, dtype=object)
    return out


def read_matrix_dosage(path):
    """--matrix with --dosage: the same table, values read as float dosages (NA = missing).  Returns (float32 (sites,
    samples), samples); values outside [-0.001, 2.001] raise ValueError, the rest are clamped to [0, 2]."""
    import pandas as pd
    gmat = pd.read_csv(path, sep="\t")
    samples = np.array(gmat["sampleID"])
    d = np.array(gmat.drop(labels="sampleID", axis=1), dtype=np.float64).T
    return check_dosage(d, path), samples


def check_dosage(d, where):
    """Range check of float dosages (NaN = missing) and the clamp to [0, 2]: float32 of the same shape."""
    d = np.asarray(d, dtype=np.float64)
    bad = ~np.isnan(d) & ((d < DOSAGE_LO) | (d > DOSAGE_HI))
    if bad.any():
        v, s = (int(i) for i in np.argwhere(bad)[0])
        raise ValueError(f"{where}: dosage {d[v, s]:g} of variant {v}, sample {s} is outside [{DOSAGE_LO}, {DOSAGE_HI}]")
    return np.clip(d, 0.0, 2.0).astype(np.float32)


def dosage_q(d):
    """Fixed-point dosages: q = rint(fp32(d) * 63) clamped to 0..126, Q_MISSING where d is NaN; uint8 of d's shape.  The
    device's form (csrc/common.h, dosage_q_dev) makes the same single fp32 product and rounding."""
    d = np.asarray(d, dtype=np.float32)
    q = np.clip(np.rint(d * np.float32(DOSAGE_UNIT)), 0, 2 * DOSAGE_UNIT)
    out = np.where(np.isnan(d), Q_MISSING, q).astype(np.uint8)
    return out


def dosage_site_sums(q):
    """(sum of q over the called samples int64, number of called samples) per variant of a q matrix."""
    called = q != Q_MISSING
    return np.where(called, q, 0).sum(axis=1, dtype=np.int64), called.sum(axis=1)


def filter_dosage(q, min_mac=2, max_snps=None, impute_missing=False, rng=np.random, verbose=True):
    """filter_snps for a q matrix (variants, samples) uint8 (dosage_q): keep a site iff, over its called samples,
    S = sum(q) >= 63 * min_mac, S > 0 and S < 126 * n_called (not monomorphic).  Missing values become 0, or with
    impute_missing 63 * Binomial(2, af), af = S / (126 n_called), drawn from `rng` once per missing value in variant-major
    order as replace_md draws.  Then the optional random subset of max_snps sites, as filter_snps.  Returns uint8 (sites,
    samples) in q units."""
    if verbose:
        print("filtering SNPs")
    q = np.asarray(q, dtype=np.uint8)
    S, n_called = dosage_site_sums(q)
    keep = (S >= DOSAGE_UNIT * int(min_mac)) & (S > 0) & (S < 2 * DOSAGE_UNIT * n_called)
    ac = q[keep]
    missing = ac == Q_MISSING
    ac = np.where(missing, 0, ac).astype(np.uint8)
    if impute_missing and missing.any():
        af = S[keep] / (2.0 * DOSAGE_UNIT * n_called[keep])
        for i, j in np.argwhere(missing):
            ac[i, j] = DOSAGE_UNIT * rng.binomial(2, af[i])
    if max_snps is not None:
        pick = rng.choice(range(ac.shape[0]), max_snps, replace=False)
        ac = ac[pick, :]
    if verbose:
        print("running on " + str(len(ac)) + " genotypes after filtering\n\n\n")
    return np.ascontiguousarray(ac)


def write_dosage_zarr(path, ds, chunk_variants=65536, compressor=None):
    """calldata/DS float32 (variants, samples) into an existing callset store (write_callset_zarr), as `allel.vcf_to_zarr`
    lays it out when asked for the field (NaN = missing)."""
    ds = np.asarray(ds, dtype=np.float32)
    write_zarr_array(os.path.join(path, "calldata", "DS"), ds, (chunk_variants, ds.shape[1]), compressor)


def zarr_dosage(callset, where):
    """The calldata/DS array of a store, or SystemExit naming it.  Only float32 (variants, samples) is accepted."""
    try:
        ds = callset["calldata/DS"]
    except KeyError:
        raise SystemExit(f"--dosage: {where} has no calldata/DS array (expected dosages, float32 (variants, samples))") \
            from None
    if len(ds.shape) != 2 or np.dtype(ds.dtype) != np.float32:
        raise SystemExit(f"--dosage: {where}: calldata/DS is {np.dtype(ds.dtype)} {tuple(ds.shape)}, expected float32 "
                         "(variants, samples)")
    return ds


# ------------------------------------------------------------------ allel.GenotypeArray subset
def count_alleles(gt, max_allele=None):
    """(variants, max_allele+1) int32 counts of called alleles; max_allele defaults to the data's max."""
    if max_allele is None:
        max_allele = int(gt.max()) if gt.size else 0
    max_allele = max(max_allele, 0)
    out = np.zeros((gt.shape[0], max_allele + 1), np.int32)
    flat = gt.reshape(gt.shape[0], int(np.prod(gt.shape[1:])))       # not -1: no variant at all is a valid input
    for a in range(max_allele + 1):
        out[:, a] = np.count_nonzero(flat == a, axis=1)
    return out


def is_biallelic(ac):
    return (ac > 0).sum(axis=1) == 2


def to_allele_counts_1(gt):
    """to_allele_counts()[:, :, 1]: per-sample number of allele-1 copies; int8 (variants, samples).
    Written as byte adds over the ploidy axis: `(gt == 1).sum(axis=2)` goes through int64 and is ~100x slower
    on a (150k, 765, 2) window, which makes the serial window prologue the Amdahl term of --windows."""
    b = (gt == 1).view(np.uint8)
    out = b[:, :, 0].copy()
    for p in range(1, gt.shape[2]):
        out += b[:, :, p]
    return out.view(np.int8)


def is_missing(gt):
    return (gt < 0).any(axis=2)


def replace_md(gt, rng=np.random):
    """locator.py:251-262: impute missing calls with Binomial(P, allele-1 frequency of the site), drawing
    from the global legacy NumPy stream once per missing call in variant-major order.  P = gt.shape[2], the ploidy of
    the calls: 2 for diploid genotypes (the reference's Binomial(2, dc / (2 n_called))), 1 for the haplotype view
    (V, 2N, 1) of --phased, whose missing alleles get Binomial(1, dc / n_called) - 0 or 1."""
    P = gt.shape[2]
    dc = count_alleles(gt, max(int(gt.max()), 1))[:, 1]
    ac = to_allele_counts_1(gt)
    missingness = is_missing(gt)
    ninds = (~missingness).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        af = dc / (P * ninds)
    for i, j in np.argwhere(missingness):
        ac[i, j] = rng.binomial(P, af[i])
    return ac


def haplotypes(gt):
    """--phased: the calls (V, N, 2) viewed as (V, 2N, 1) - row 2s + h holds allele h of sample s (no copy).  Every filter
    and count of this module then works on haplotype rows: to_allele_counts_1 gives 1 where the allele is 1, else 0."""
    V, N, P = gt.shape
    return gt.reshape(V, N * P, 1)


HOST_THREADS = 8      # threads of the C passes below (they release the GIL)


def _chunks(n, parts):
    step = max(1, -(-n // max(1, parts)))
    return [(a, min(a + step, n)) for a in range(0, n, step)]


def _filter_snps_native(gt, min_mac):
    """The biallelic + allele-1-count filters and to_allele_counts()[:, :, 1] of filter_snps as two C passes over the calls
    (csrc/codecs.c: loc_snp_flags, loc_snp_allele_counts), a few threads each: (ac int8 [K][N], keep flags)."""
    from concurrent.futures import ThreadPoolExecutor
    lib = _codecs()
    gt = np.ascontiguousarray(gt, dtype=np.int8)
    V, N, P = gt.shape
    keep = np.zeros(V, np.uint8)
    parts = _chunks(V, HOST_THREADS * 4)
    with ThreadPoolExecutor(HOST_THREADS) as ex:
        list(ex.map(lambda ab: lib.loc_snp_flags(gt.ctypes.data, ab[0], ab[1], N * P, int(min_mac), keep.ctypes.data), parts))
        pos = np.zeros(V, np.int64)
        np.cumsum(keep[:-1], out=pos[1:]) if V > 1 else None
        K = int(keep.sum())
        ac = np.empty((K, N), np.int8)
        list(ex.map(lambda ab: lib.loc_snp_allele_counts(gt.ctypes.data, ab[0], ab[1], N, P, keep.ctypes.data,
                                                         pos.ctypes.data, ac.ctypes.data), parts))
    return ac, keep


def rows_transposed(ac, rows):
    """`ac[:, rows].T` (split_train_test, locator.py:303-306) as a C blocked transpose on a few threads: the sample-major
    int8 matrix [len(rows)][K] the training path uploads."""
    from concurrent.futures import ThreadPoolExecutor
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    K, N = ac.shape
    out = np.empty((len(rows), K), ac.dtype)
    if len(rows) == 0 or K == 0:
        return out
    if ac.dtype.itemsize != 1 or not ac.flags.c_contiguous:
        return np.ascontiguousarray(ac[:, rows].T)
    lib = _codecs()
    step = (max(64, -(-K // (HOST_THREADS * 4))) + 63) // 64 * 64          # 64-SNP blocks: a write run is one cache line
    parts = [(a, min(a + step, K)) for a in range(0, K, step)]
    with ThreadPoolExecutor(HOST_THREADS) as ex:
        list(ex.map(lambda ab: lib.loc_rows_transposed(ac.ctypes.data, ab[0], ab[1], N, rows.ctypes.data, len(rows),
                                                       out.ctypes.data, K), parts))
    return out


def filter_snps(gt, min_mac=2, max_snps=None, impute_missing=False, rng=np.random, verbose=True, native=True, sites=False):
    """locator.py:265-281: biallelic sites -> allele-1 count >= min_mac (skipped when min_mac == 1) ->
    allele-1 count matrix (sites x samples) -> optional random subset of max_SNPs sites.
    Quirks kept: the count filtered on is allele 1's, not the minor allele's; monomorphic
    sites never pass (Q8).  native: the two filters and the allele counts as C passes (same integers; the NumPy spelling
    below stays as their restatement and as the --impute_missing path, whose draws follow the filtered array).  sites=True:
    (matrix, index of the input variant of every row) - the same draws, nothing more (--keep_model)."""
    if verbose:
        print("filtering SNPs")
    if native and not impute_missing and np.ndim(gt) == 3 and gt.shape[0] > 0 and int(np.min(gt.shape)) > 0:
        ac, keep = _filter_snps_native(gt, min_mac)
        idx = np.flatnonzero(keep)
        if max_snps is not None:
            pick = rng.choice(range(ac.shape[0]), max_snps, replace=False)
            ac, idx = ac[pick, :], idx[pick]
        if verbose:
            print("running on " + str(len(ac)) + " genotypes after filtering\n\n\n")
        return (ac, idx) if sites else ac
    tmp = count_alleles(gt)
    idx = np.flatnonzero(is_biallelic(tmp))
    gt = gt[idx]
    if not min_mac == 1:
        derived = count_alleles(gt, max(int(gt.max()) if gt.size else 1, 1))[:, 1]
        gt, idx = gt[derived >= min_mac], idx[derived >= min_mac]
    ac = replace_md(gt, rng) if impute_missing else to_allele_counts_1(gt)
    if max_snps is not None:
        pick = rng.choice(range(ac.shape[0]), max_snps, replace=False)
        ac, idx = ac[pick, :], idx[pick]
    if verbose:
        print("running on " + str(len(ac)) + " genotypes after filtering\n\n\n")
    return (ac, idx) if sites else ac
