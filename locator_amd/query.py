"""A kept model on new genotypes: read a `.model.npz` (`--keep_model`), match its sites to a query file, refuse what
cannot be predicted, and build the model-ordered genotype rows on the device (`loc_query_rows`).

Matching: model column k looks for a query variant with the same CHROM and POS whose allele list (REF,
then every ALT) holds both the model's REF and its ALT; the column then counts copies of allele `a` = the index of the
model's ALT in that list (1 normally, 0 when the query swaps REF and ALT, 2.. in a multi-allelic record).  Several
matching records: the first in file order wins.  A `--matrix` query matches by column name, a = 1.  A column without a
match is absent: its batch-normalisation gamma is set to 0, so the network sees it at the training moving mean whatever
the rows hold.  Nothing here draws from the NumPy stream except `impute_missing`.

`--dosage` queries (imputed or low-coverage samples: FORMAT/DS or GP, `calldata/DS`, a float matrix) go the same way with
float dosages in place of calls: `read_query_dosage`, `check_query_dosage`, `compact_dosages`, `impute_dosages`, and
`loc_query_rows_dosage` builds the rows in the fixed-point unit q = rint(63 d) that `LocatorNet(unit=63)` runs any model on.
"""
from __future__ import annotations

import json
import os

import numpy as np

from . import genotypes as G


class QueryRefused(SystemExit):
    """A query that cannot be predicted with a model (raised before any device work)."""


# ------------------------------------------------------------------ model files
def model_paths(specs):
    """--model arguments (files or directories of `*.model.npz`) -> file list; a directory contributes its model files in
    name order."""
    out = []
    for spec in specs:
        if os.path.isdir(spec):
            found = sorted(f for f in os.listdir(spec) if f.endswith(".model.npz"))
            if not found:
                raise QueryRefused(f"--model {spec}: no *.model.npz in this directory")
            out += [os.path.join(spec, f) for f in found]
        else:
            out.append(spec)
    return out


def model_stem(path):
    name = os.path.basename(path)
    for suffix in (".model.npz", ".npz"):
        if name.endswith(suffix):
            return name[:-len(suffix)]
    return name


def load_model(path):
    """A `.model.npz` -> dict: weights (the oracle-format dict LocatorNet.import_params takes), site table, normalisation,
    ploidy, phased, params.  Read without pickle.  A `.weights.npz` (no site table) is refused."""
    from .locator import read_weights
    with np.load(path, allow_pickle=False) as z:
        if "site_chrom" not in z.files:
            raise QueryRefused(f"{path}: no site table - a --keep_weights file cannot be matched to another genotype file; "
                               "train with --keep_model")
        version = int(z["format_version"])
        if version != 1:
            raise QueryRefused(f"{path}: model format_version {version}; this reader knows 1")
        m = {"path": path, "stem": model_stem(path),
             "chrom": z["site_chrom"].astype(str), "pos": z["site_pos"].astype(np.int64), "ref": z["site_ref"].astype(str),
             "alt": z["site_alt"].astype(str), "af": z["site_af"].astype(np.float64),
             "locs_norm": [float(v) for v in z["locs_norm"]], "ploidy": int(z["ploidy"]), "phased": bool(z["phased"]),
             "params": json.loads(str(z["params_json"])), "width": int(z["width"]), "nlayers": int(z["nlayers"])}
    m["weights"] = read_weights(path)
    m["K"] = int(m["weights"]["W"][0].shape[0])
    return m


# ------------------------------------------------------------------ query files
def read_query(vcf=None, zarr=None, matrix=None):
    """The query's calls and site identities: {"gt" (V, N, P) int8, "samples", "kind" ("vcf" / "zarr" / "matrix"),
    "chrom", "pos", "alleles" (list per variant: REF then every ALT) - or "names" for a matrix -, "unphased_hets"
    (None when unknown)}."""
    if sum(x is not None for x in (vcf, zarr, matrix)) != 1:
        raise QueryRefused("give exactly one of --vcf, --zarr or --matrix as the query")
    if vcf is not None:
        d = G.read_vcf(vcf, phase=True, sites=True)
        q = {"gt": d["calldata/GT"], "samples": np.asarray(d["samples"]).astype(str), "kind": "vcf",
             "unphased_hets": d["unphased_hets"]}
    elif zarr is not None:
        callset = G.open_group(zarr, mode="r")
        try:
            d = G.zarr_sites(callset)
        except KeyError as e:
            raise QueryRefused(f"--zarr {zarr}: no {e.args[0]} - the sites of the query cannot be identified") from None
        za = callset["calldata/GT"]
        gt = np.empty(za.shape, np.int8) if (za.dtype == np.int8 and za.ndim == 3) else None
        if gt is not None:
            za.read_into(gt, 0, za.shape[0], threads=G.HOST_THREADS)
        else:
            gt = np.asarray(za[:], dtype=np.int8)
        q = {"gt": gt, "samples": np.asarray(callset["samples"][:]).astype(str), "kind": "zarr",
             "unphased_hets": G.zarr_unphased_hets(callset)}
    else:
        gt, samples = G.read_matrix(matrix)
        return {"gt": gt, "samples": np.asarray(samples).astype(str), "kind": "matrix",
                "names": G.matrix_sites(matrix).astype(str), "unphased_hets": None}
    q["chrom"] = np.asarray(d["variants/CHROM"]).astype(str)
    q["pos"] = np.asarray(d["variants/POS"], dtype=np.int64)
    ref = np.asarray(d["variants/REF"]).astype(str)
    alt = np.asarray(d["variants/ALT"], dtype=object)
    if alt.ndim == 1:
        alt = alt[:, None]
    q["alleles"] = [[r] + [str(a) for a in row if str(a) not in ("", ".")] for r, row in zip(ref, alt)]
    return q


def read_query_dosage(vcf=None, zarr=None, matrix=None, field="DS"):
    """--dosage form of read_query: {"ds" (V, N) float32 expected alt-allele dosages (NaN = missing), range-checked and
    clamped by genotypes.check_dosage, "samples", "kind", "chrom", "pos", "alleles" (always [REF, ALT]: records with several
    ALT alleles are dropped by the reader and counted in "multiallelic_dropped") - or "names" for a matrix}.  GP is read from a
    VCF only.  A file without the field or with a value outside [-0.001, 2.001] is refused here."""
    if sum(x is not None for x in (vcf, zarr, matrix)) != 1:
        raise QueryRefused("give exactly one of --vcf, --zarr or --matrix as the query")
    if field not in ("DS", "GP"):
        raise QueryRefused(f"--dosage takes DS or GP (got {field!r})")
    if vcf is not None:
        try:
            d = G.read_vcf_dosage(vcf, field, sites=True)
        except ValueError as e:
            raise QueryRefused(f"--dosage {field}: {e}") from None
        q = {"ds": d["calldata/DS"], "samples": np.asarray(d["samples"]).astype(str), "kind": "vcf",
             "multiallelic_dropped": int(d["multiallelic_dropped"])}
    elif zarr is not None:
        if field == "GP":
            raise QueryRefused("--dosage GP: a zarr store is read from calldata/DS only; use --dosage DS")
        callset = G.open_group(zarr, mode="r")
        try:
            d = G.zarr_sites(callset)
        except KeyError as e:
            raise QueryRefused(f"--zarr {zarr}: no {e.args[0]} - the sites of the query cannot be identified") from None
        try:
            za = G.zarr_dosage(callset, zarr)
            ds = G.check_dosage(np.asarray(za[:]), f"{zarr}: calldata/DS")
        except (SystemExit, ValueError) as e:
            raise QueryRefused(str(e)) from None
        q = {"ds": ds, "samples": np.asarray(callset["samples"][:]).astype(str), "kind": "zarr", "multiallelic_dropped": 0}
    else:
        if field == "GP":
            raise QueryRefused("--dosage GP: a --matrix holds one value per site and sample; use --dosage DS")
        try:
            ds, samples = G.read_matrix_dosage(matrix)
        except ValueError as e:
            raise QueryRefused(f"--dosage: {e}") from None
        return {"ds": ds, "samples": np.asarray(samples).astype(str), "kind": "matrix",
                "names": G.matrix_sites(matrix).astype(str)}
    q["chrom"] = np.asarray(d["variants/CHROM"]).astype(str)
    q["pos"] = np.asarray(d["variants/POS"], dtype=np.int64)
    ref = np.asarray(d["variants/REF"]).astype(str)
    alt = np.asarray(d["variants/ALT"], dtype=object)
    if alt.ndim == 2:                       # a store lists every ALT: the first is the record's, more than one is not biallelic
        extra = np.array([sum(str(a) not in ("", ".") for a in row[1:]) for row in alt], dtype=np.int64)
        alt = np.where(extra > 0, "", alt[:, 0].astype(str))        # no ALT to match: such a record stays absent
        q["multiallelic_dropped"] += int((extra > 0).sum())
    q["alleles"] = [[r, "" if str(a) == "." else str(a)] for r, a in zip(ref, alt)]
    return q


# ------------------------------------------------------------------ matching
def match_sites(model, query):
    """-> (col_variant int32 [K]: query variant of every model column or -1, col_allele int8 [K], report dict)."""
    K = len(model["chrom"])
    col_variant = np.full(K, -1, np.int32)
    col_allele = np.zeros(K, np.int8)
    if query["kind"] == "matrix":
        first = {}
        for i, name in enumerate(query["names"]):
            first.setdefault(name, i)
        for k, name in enumerate(model["chrom"]):
            v = first.get(name)
            if v is not None:
                col_variant[k], col_allele[k] = v, 1
    else:
        where = {}
        for i, key in enumerate(zip(query["chrom"], query["pos"].tolist())):
            where.setdefault(key, []).append(i)                 # file order
        alleles = query["alleles"]
        for k, key in enumerate(zip(model["chrom"], model["pos"].tolist())):
            ref, alt = model["ref"][k], model["alt"][k]
            for v in where.get(key, ()):
                al = alleles[v]
                if ref in al and alt in al and al.index(alt) <= 127:
                    col_variant[k], col_allele[k] = v, al.index(alt)
                    break
    present = col_variant >= 0
    report = {"model": model["stem"], "K": K, "matched": int(present.sum()),
              "allele_not_1": int((present & (col_allele != 1)).sum()), "absent": int((~present).sum())}
    return col_variant, col_allele, report


def check_query(model, query, report, min_site_overlap=0.5):
    """The refusals, before any device work: too few matched sites, another ploidy, unphased heterozygotes for a phased
    model (or a count matrix, which carries no phase)."""
    name = model["path"]
    if report["matched"] < min_site_overlap * report["K"]:
        raise QueryRefused(f"{name}: {report['matched']} of the model's {report['K']} sites are in the query, fewer than "
                           f"--min_site_overlap {min_site_overlap} of them")
    P = int(query["gt"].shape[2])
    if P != model["ploidy"]:
        raise QueryRefused(f"{name}: the model was trained on ploidy {model['ploidy']}, the query has ploidy {P}")
    if model["phased"]:
        if query["kind"] == "matrix":
            raise QueryRefused(f"{name} is a --phased model: an allele-count --matrix query carries no phase")
        n = query["unphased_hets"]
        if n:
            raise QueryRefused(f"{name} is a --phased model and the query has {n} heterozygous call(s) without phase "
                               "(written 'a/b'); phase them first")


def check_query_dosage(model, query, report, min_site_overlap=0.5):
    """check_query for a --dosage query: the same overlap rule; a --phased model (a dosage has no haplotypes), a model of
    another ploidy than 2 (a dosage counts the copies of a diploid call), a query without dosages and a dosage outside
    [-0.001, 2.001] are refused.  All before any device work."""
    name = model["path"]
    if model["phased"]:
        raise QueryRefused(f"{name} is a --phased model: a --dosage query has no haplotypes")
    if model["ploidy"] != 2:
        raise QueryRefused(f"{name}: the model was trained on ploidy {model['ploidy']}; a dosage is the expected allele count "
                           "of a diploid call (ploidy 2)")
    ds = query.get("ds")
    if ds is None:
        raise QueryRefused(f"{name}: the query holds no dosages (FORMAT/DS or GP, calldata/DS, or a float --matrix)")
    ds = np.asarray(ds)
    bad = ~np.isnan(ds) & ((ds < G.DOSAGE_LO) | (ds > G.DOSAGE_HI))
    if bad.any():
        v, s = (int(i) for i in np.argwhere(bad)[0])
        raise QueryRefused(f"{name}: dosage {ds[v, s]:g} of query variant {v}, sample {s} is outside "
                           f"[{G.DOSAGE_LO}, {G.DOSAGE_HI}]")
    if report["matched"] < min_site_overlap * report["K"]:
        raise QueryRefused(f"{name}: {report['matched']} of the model's {report['K']} sites are in the query, fewer than "
                           f"--min_site_overlap {min_site_overlap} of them")


def select_samples(query, ids=None):
    """--samples: the query sample indices to predict, in the file's order (default: every sample)."""
    samples = list(query["samples"])
    if ids is None:
        return np.arange(len(samples), dtype=np.int64)
    index = {s: i for i, s in enumerate(samples)}
    missing = [s for s in ids if s not in index]
    if missing:
        raise QueryRefused(f"--samples: {len(missing)} ID(s) not in the query, first {missing[0]!r}")
    if len(set(ids)) != len(ids):
        raise QueryRefused("--samples lists an ID twice")
    return np.array([index[s] for s in ids], dtype=np.int64)


def compact_calls(query, columns):
    """The calls of the matched variants only, as contiguous rows in query order: (calls (U, N, P) int8, remapped
    col_variant per model).  columns: [(col_variant, col_allele), ...] of every model of the set."""
    used = np.unique(np.concatenate([cv[cv >= 0] for cv, _ in columns] + [np.zeros(0, np.int32)]))
    calls = np.ascontiguousarray(query["gt"][used])
    remapped = [np.where(cv >= 0, np.searchsorted(used, cv), -1).astype(np.int32) for cv, _ in columns]
    return calls, remapped, used


def compact_dosages(query, columns):
    """compact_calls for a --dosage query: (ds (U, N) float32 of the matched variants, contiguous and in query order,
    remapped col_variant per model, the query variants used)."""
    used = np.unique(np.concatenate([cv[cv >= 0] for cv, _ in columns] + [np.zeros(0, np.int32)]))
    ds = np.ascontiguousarray(query["ds"][used], dtype=np.float32)
    remapped = [np.where(cv >= 0, np.searchsorted(used, cv), -1).astype(np.int32) for cv, _ in columns]
    return ds, remapped, used


def impute_calls(calls, rows, col_variant, col_allele, af, phased, rng=np.random):
    """--impute_missing: every call of a predicted row with a missing allele at a present site becomes Binomial(P, af)
    copies of the column's allele (P = the calls' ploidy; 1 for the haplotype rows of a phased model), af = the model's
    allele-1 frequency of that site.  Draws from the global NumPy stream in variant-then-row order.  A variant that
    several columns use takes the allele and frequency of the first.  calls (U, N, P) is modified in place."""
    view = G.haplotypes(calls) if phased else calls
    P = view.shape[2]
    first = {}
    for k, v in enumerate(col_variant.tolist()):
        if v >= 0 and v not in first:
            first[v] = k
    if not first:
        return calls
    vs = np.array(sorted(first), dtype=np.int64)
    ks = np.array([first[v] for v in vs], dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    miss = (view[vs][:, rows, :] < 0).any(axis=2)               # (variants, rows)
    vi, ri = np.nonzero(miss)                                   # row-major: variant, then row
    if not len(vi):
        return calls
    draws = rng.binomial(P, af[ks[vi]])
    a = col_allele[ks[vi]].astype(np.int8)
    other = np.where(a == 0, 1, 0).astype(np.int8)
    for p in range(P):
        view[vs[vi], rows[ri], p] = np.where(p < draws, a, other)
    return calls


def impute_dosages(ds, rows, col_variant, col_allele, af, rng=np.random):
    """--impute_missing for a --dosage query: every NaN of a predicted row at a present site becomes a whole dosage from
    draws = Binomial(2, af) copies of the column's allele, af = the model's allele-1 frequency of that site: the stored
    (alt-allele) dosage is `draws` for a column of allele 1 and 2 - draws for allele 0, so that the column holds 63 draws
    either way.  The draws are those impute_calls makes for the same missing pattern: global NumPy stream, variant-then-row
    order, a variant that several columns use takes the allele and frequency of the first.  ds (U, N) is modified in place."""
    first = {}
    for k, v in enumerate(col_variant.tolist()):
        if v >= 0 and v not in first:
            first[v] = k
    if not first:
        return ds
    vs = np.array(sorted(first), dtype=np.int64)
    ks = np.array([first[v] for v in vs], dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    vi, ri = np.nonzero(np.isnan(ds[vs][:, rows]))              # row-major: variant, then row
    if not len(vi):
        return ds
    draws = rng.binomial(2, af[ks[vi]])
    ds[vs[vi], rows[ri]] = np.where(col_allele[ks[vi]] == 0, 2 - draws, draws).astype(ds.dtype)
    return ds


def absent_gamma(weights, col_variant):
    """The weights with gamma = 0 on every absent column: inference batch-norm then gives beta_k - the feature at its
    training moving mean - whatever the column holds."""
    w = dict(weights)
    w["gamma"] = np.where(col_variant >= 0, weights["gamma"], 0).astype(weights["gamma"].dtype)
    return w


# ------------------------------------------------------------------ device
def query_rows(calls_dev, col_variant, col_allele, sample_order, K):
    """loc_query_rows: (U, N, P) int8 device calls -> uint8 [len(sample_order)][Kp] rows in model column order (padding
    columns zero)."""
    import torch

    from . import _lib
    from .net import _ptr, _stream
    lib = _lib.load()
    assert calls_dev.dtype == torch.int8 and calls_dev.is_contiguous() and calls_dev.dim() == 3
    dev = calls_dev.device
    U, N, P = (int(v) for v in calls_dev.shape)
    Kp = (max(int(K), 1) + 31) // 32 * 32
    so = torch.as_tensor(np.asarray(sample_order, dtype=np.int32)).to(dev)
    cv = torch.as_tensor(np.ascontiguousarray(col_variant, dtype=np.int32)).to(dev)
    ca = torch.as_tensor(np.ascontiguousarray(col_allele, dtype=np.int8)).to(dev)
    X = torch.zeros((len(so), Kp), dtype=torch.uint8, device=dev)
    _lib.check(lib.loc_query_rows(_ptr(calls_dev) if U else None, U, N, P, _ptr(cv), _ptr(ca), int(K), _ptr(so), len(so),
                                  _ptr(X), X.stride(0), _stream()), "loc_query_rows")
    return X


def query_rows_dosage(ds_dev, col_variant, col_allele, sample_order, K):
    """loc_query_rows_dosage: (U, N) float32 device dosages -> uint8 [len(sample_order)][Kp] rows in model column order, in
    q units (0..126; padding columns zero)."""
    import torch

    from . import _lib
    from .net import _ptr, _stream
    lib = _lib.load()
    assert ds_dev.dtype == torch.float32 and ds_dev.is_contiguous() and ds_dev.dim() == 2
    dev = ds_dev.device
    U, N = (int(v) for v in ds_dev.shape)
    Kp = (max(int(K), 1) + 31) // 32 * 32
    so = torch.as_tensor(np.asarray(sample_order, dtype=np.int32)).to(dev)
    cv = torch.as_tensor(np.ascontiguousarray(col_variant, dtype=np.int32)).to(dev)
    ca = torch.as_tensor(np.ascontiguousarray(col_allele, dtype=np.int8)).to(dev)
    X = torch.zeros((len(so), Kp), dtype=torch.uint8, device=dev)
    _lib.check(lib.loc_query_rows_dosage(_ptr(ds_dev) if U else None, U, N, _ptr(cv), _ptr(ca), int(K), _ptr(so), len(so),
                                         _ptr(X), X.stride(0), _stream()), "loc_query_rows_dosage")
    return X


def predict_rows(model, X, settings, device="cuda:0", unit=1):
    """The model's z-scored predictions for every row of X (uint8 [n][Kp] on the device) -> float32 (n, 2).  unit: the
    fixed-point unit of X - 1 for allele counts, genotypes.DOSAGE_UNIT for the rows of a --dosage query (the weights go
    through import_params as they are: it converts the moving statistics to q units)."""
    import torch

    from .net import LocatorNet
    n = int(X.shape[0])
    if n == 0:
        return np.zeros((0, 2), np.float32)
    Y = torch.zeros((n, 2), dtype=torch.float32, device=device)
    net = LocatorNet(X, Y, model["K"], model["width"], model["nlayers"], float(model["params"].get("dropout_prop", 0.25)),
                     seed=0, device=device, **settings, **({"unit": int(unit)} if unit != 1 else {}))
    net.import_params(model["weights_used"])
    rows = torch.arange(n, dtype=torch.int32, device=device)
    yhat = torch.zeros((n, 2), dtype=torch.float32, device=device)
    net.predict_rows(rows, n, yhat)
    torch.cuda.current_stream().synchronize()
    return yhat.cpu().numpy()
