"""What the baseline commands (neighbors.py: IBS distances and a kNN placement; pca.py: principal components and a PC-regression
placement; paint.py and ibd.py: a top-k placement from a sample-by-sample weight) share: the count matrix, the inputs, the
common command line (with the --k / --kmax of neighbors, paint and ibd and the haplotype prelude of the latter two), the errors
of a placement, the choice of the smallest leave-one-out median, the top-k weighted placement with its summary entries and the
common part of the summaries.  Messages name the command that runs (`prog`: "locator_amd.pca")."""
import argparse
import io
import os
import zipfile

import numpy as np


# ---------------------------------------------------------------- counts

def _counts_by_site(gt, idx):
    from . import genotypes as G
    g = np.asarray(gt)[np.asarray(idx, dtype=np.int64)]
    P = int(g.shape[2])
    if P not in (1, 2):
        raise ValueError(f"calls of ploidy {P}: the IBS distance is built for ploidy 1 and 2")
    c = G.to_allele_counts_1(g).copy()
    c[G.is_missing(g)] = -1
    return c, P


def count_matrix(gt, idx):
    """(c, P): c int8 [samples][sites] = allele-1 counts of the variants gt[idx] (variants, samples, P), -1 where the call is
    missing in any allele; P = the ploidy of the calls."""
    c, P = _counts_by_site(gt, idx)
    return np.ascontiguousarray(c.T), P


def count_matrix_sites(gt, idx):
    """(ct, P): count_matrix's values site-major, int8 [sites][samples], not transposed: what the ld command compares."""
    c, P = _counts_by_site(gt, idx)
    return np.ascontiguousarray(c, dtype=np.int8), P


def check_counts(c, P):
    """c as an int8 [N][K] array, after the refusals that precede any device work."""
    c = np.asarray(c)
    if c.ndim != 2:
        raise ValueError(f"count matrix of shape {c.shape}: needs [samples][sites]")
    if P not in (1, 2):
        raise ValueError(f"P = {P}: must be 1 or 2")
    if c.size and int(c.max()) > P:
        raise ValueError(f"a count of {int(c.max())} exceeds the ploidy {P}: allele-1 counts are 0 .. {P}, missing is -1")
    if c.shape[1] * P >= 2 ** 31:
        raise ValueError(f"{c.shape[1]} sites x ploidy {P}: a distance sum could leave int32")
    c = np.ascontiguousarray(c, dtype=np.int8)
    return np.where(c < 0, np.int8(-1), c) if c.size and int(c.min()) < -1 else c


def padded(c, pitch=None, fill=-1):
    """c copied into rows of `pitch` bytes (default: the next multiple of 16), the pad filled with `fill`: a value, or a
    np.random.Generator for arbitrary bytes (the kernel must not interpret them)."""
    N, K = c.shape
    pitch = (K + 15) // 16 * 16 if pitch is None else int(pitch)
    if isinstance(fill, np.random.Generator):
        buf = fill.integers(-128, 128, (N, max(pitch, 16)), dtype=np.int8)
    else:
        buf = np.full((N, max(pitch, 16)), fill, dtype=np.int8)
    buf[:, :K] = c
    return buf


# ---------------------------------------------------------------- placements

def errors(xy, truth, longlat=False):
    """Distance of every placement from the true location: Euclidean in map units, or with longlat great-circle km."""
    if longlat:
        from .plot import distance_km
        return distance_km(xy[..., 0], xy[..., 1], truth[..., 0], truth[..., 1])
    return np.sqrt(((xy - truth) ** 2).sum(axis=-1))


def choose_smallest_median(placed, locs, located, longlat, nothing):
    """(q, per-q median error) of placements [Q][N][2], q = 1 .. Q (--k auto, --p auto): the leave-one-out median error over the
    located samples for every q and the smallest q that attains the smallest of them; `nothing` refuses when no q has an error."""
    err = errors(placed[:, located], np.asarray(locs, dtype=np.float64)[located][None], longlat)
    med = np.array([np.nan if np.isnan(e).all() else np.nanmedian(e) for e in err])
    if np.isnan(med).all():
        raise ValueError(nothing)
    return int(np.nanargmin(med)) + 1, med


def top_donors(W, candidate, kmax):
    """(nbr int32 [N][kmax], weight float64 [N][kmax]): for sample s the candidate samples t with W[s][t] > 0 by W descending,
    ties to the lower index; -1 and 0 past their number."""
    N = W.shape[0]
    nbr, weight = np.full((N, kmax), -1, dtype=np.int32), np.zeros((N, kmax))
    cand = np.flatnonzero(candidate)
    for s in range(N):
        ts = cand[W[s, cand] > 0]
        ts = ts[np.argsort(-W[s, ts], kind="stable")][:kmax]
        nbr[s, :len(ts)], weight[s, :len(ts)] = ts, W[s, ts]
    return nbr, weight


def placements(nbr, weight, locs):
    """[kmax][N][2]: for k = 1 .. kmax the weighted mean location of each sample's first k donors, summed in rank order; a
    sample with fewer than k donors keeps the mean over those it has, one with none is NaN."""
    xy = np.where((nbr >= 0)[:, :, None], np.asarray(locs, dtype=np.float64)[np.maximum(nbr, 0)], 0.0) * weight[:, :, None]
    sums, tot = np.cumsum(xy, axis=1), np.cumsum(weight, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.transpose(sums / tot[:, :, None], (1, 0, 2))


def r2(a, b):
    """The squared Pearson correlation, NaN for fewer than two values or a constant."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.corrcoef(a, b)[0][1] ** 2) if len(a) > 1 else np.nan


def num(v):
    return None if v is None or not np.isfinite(v) else float(v)


def placement_summary(c, P, located, xy, locs, longlat, method, how="leave-one-out"):
    """(entries, lines) every baseline reports about its chosen placement xy [N][2]: the summary entries N, n_located, K, P,
    error_unit, r2_x, r2_y, mean_error, median_error (the command fixes the key order) and the terminal lines of R2 and error.
    how: what the located samples' placements are (spa: "held-out", its folds are no leave-one-out)."""
    err = errors(xy[located], locs[located], longlat)
    ok = ~np.isnan(err)
    fitted, truth = xy[located][ok], locs[located][ok]
    r = [r2(fitted[:, a], truth[:, a]) for a in (0, 1)]
    unit = "km" if longlat else "map units"
    entries = {"N": int(c.shape[0]), "n_located": int(located.sum()), "K": int(c.shape[1]), "P": int(P), "error_unit": unit,
               "r2_x": num(r[0]), "r2_y": num(r[1]), "mean_error": num(np.mean(err[ok])) if ok.any() else None,
               "median_error": num(np.median(err[ok])) if ok.any() else None}
    lines = [f"R2(x)={r[0]}", f"R2(y)={r[1]}", f"mean {method} {how} error {entries['mean_error']}",
             f"median {method} {how} error {entries['median_error']} ({unit})"]
    return entries, lines


def located_mask(locs, N, prog):
    """(locs float64 [N][2], located bool [N]) after the refusal of locations none of which is known."""
    locs = np.asarray(locs, dtype=np.float64).reshape(N, 2)
    located = ~np.isnan(locs).any(axis=1)
    if not located.any():
        raise SystemExit(f"{prog}: no sample of --sample_data has a location: nothing to place from")
    return locs, located


def place_by_weight(prog, W, candidate, kmax, k, c, P, locs, located, longlat, method, nothing):
    """The placement of the paint and ibd commands from a sample-by-sample weight W [N][N]: (xy [N][2], head entries,
    placed_own entries, terminal lines, nbr, weight).  nbr, weight: top_donors among the candidates, min(kmax, their number) a
    sample.  located None (no locations): xy None, no entries and no lines.  Else xy is the W-weighted mean location of the first
    k donors, k the smallest leave-one-out median error's with "auto" (`nothing` refuses when no k has one); head and lines are
    placement_summary's for the method word."""
    kmax = int(min(kmax, np.count_nonzero(candidate)))
    nbr, weight = top_donors(W, candidate, kmax)
    if located is None:
        return None, {}, {}, [], nbr, weight
    placed = placements(nbr, weight, locs)
    try:
        k_auto, med = choose_smallest_median(placed, locs, located, longlat, nothing)
    except ValueError as e:
        raise SystemExit(f"{prog}: {e}") from None
    k_used = min(k_auto if k == "auto" else int(k), kmax)
    xy = placed[k_used - 1]
    head, lines = placement_summary(c, P, located, xy, locs, longlat, method)
    own = {"kmax": kmax, "k": int(k_used), "k_auto": int(k_auto), "k_chosen_by": "auto" if k == "auto" else "--k",
           "median_error_by_k": [num(v) for v in med]}
    lines = [f"k = {k_used} ({own['k_chosen_by']}; leave-one-out median error by k, k = 1 .. {kmax}, smallest at k = {k_auto})", *lines]
    return xy, head, own, lines, nbr, weight


def assemble_summary(head, own, placed_own, head_keys, own_keys, placed_keys, host):
    """The summary of the paint and ibd commands in its key order: the shared head (N, K, P alone without a placement), the
    command's own entries, those of the placement, and the path."""
    summary = {**{key: head[key] for key in (head_keys if "n_located" in head else ("N", "K", "P"))},
               **{key: own[key] for key in own_keys}, **{key: placed_own[key] for key in placed_keys if key in placed_own}}
    summary["path"] = "host" if host else "device"
    return summary


def write_locs(path, xy, samples):
    """The x,y,sampleID file of a placement, written as a predlocs file is."""
    import pandas as pd
    from ._files import write_atomic
    frame = pd.DataFrame({"x": xy[:, 0], "y": xy[:, 1], "sampleID": np.asarray(samples).astype(object)})
    write_atomic(path, lambda fh: frame.to_csv(fh, index=False))


def save_npz(fh, **arrays):
    """np.savez_compressed with a fixed member date: two runs that hold the same arrays write the same bytes."""
    with zipfile.ZipFile(fh, "w", zipfile.ZIP_DEFLATED) as z:
        for name, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


# ---------------------------------------------------------------- command

def read_inputs(a, prog):
    """(gt, samples) by the readers of the fit (genotypes.py), and the refusal of a --matrix with counts above 2 (read_matrix
    itself lets them contribute nothing)."""
    from . import genotypes as G
    if a.zarr is not None:
        callset = G.open_group(a.zarr, mode="r")
        return np.asarray(callset["calldata/GT"][:], dtype=np.int8), np.asarray(callset["samples"][:])
    if a.vcf is not None:
        vcf = G.read_vcf(a.vcf)
        return vcf["calldata/GT"], vcf["samples"]
    import pandas as pd
    raw = pd.read_csv(a.matrix, sep="\t").drop(labels="sampleID", axis=1).to_numpy()
    if raw.size and raw.max() > 2:
        raise SystemExit(f"{prog}: {a.matrix} holds a count of {raw.max()}: allele counts above 2 (ploidy above 2) are not supported")
    return G.read_matrix(a.matrix)


def read_inputs_sites(a, prog, phase=False):
    """(gt, samples, chrom, pos) for the LD window: read_inputs' answers and the variants' CHROM / POS tables.  A --matrix has
    one chromosome and no positions (pos None).  phase (the paint command): the calls must be phased, so a --matrix and an
    input with a heterozygous call written without phase are refused as locator.py --phased refuses them."""
    from . import genotypes as G
    if phase and a.zarr is None and a.vcf is None:
        raise SystemExit(f"{prog} needs --vcf or --zarr: an allele-count --matrix carries no phase")
    if a.zarr is not None:
        callset = G.open_group(a.zarr, mode="r")
        if phase:
            refuse_unphased(G.zarr_unphased_hets(callset), f"{a.zarr}: calldata/GT_phased", prog)
        try:
            sites = G.zarr_sites(callset)
        except KeyError as e:
            raise SystemExit(f"{prog}: {a.zarr} lacks {e.args[0]}: the LD window needs the variants' CHROM and POS") from None
        return (np.asarray(callset["calldata/GT"][:], dtype=np.int8), np.asarray(callset["samples"][:]), sites["variants/CHROM"],
                sites["variants/POS"])
    if a.vcf is not None:
        vcf = G.read_vcf(a.vcf, phase=phase, sites=True)
        if phase:
            refuse_unphased(vcf["unphased_hets"], a.vcf, prog)
        return vcf["calldata/GT"], vcf["samples"], vcf["variants/CHROM"], vcf["variants/POS"]
    gt, samples = read_inputs(a, prog)
    return gt, samples, None, None


def refuse_unphased(n, where, prog):
    """The refusal of n heterozygous calls without phase (n None or 0: none is known of)."""
    if n:
        raise SystemExit(f"{prog}: {where} has {n} heterozygous call(s) without phase (written 'a/b'); phase them first (python -m "
                         "locator_amd.phase)")


def read_locations(sample_data, samples, prog):
    """[N][2] x / y of the genotype samples in their order (NaN = not located); every sample must be in the table."""
    import pandas as pd
    table = pd.read_csv(sample_data, sep="\t").drop_duplicates("sampleID").set_index("sampleID")
    ids = np.asarray(samples).astype(str)
    table.index = table.index.astype(str)
    missing = [s for s in ids if s not in table.index]
    if missing:
        raise SystemExit(f"{prog}: {len(missing)} genotype samples are not in {sample_data} (first: {missing[0]})")
    return table.reindex(ids)[["x", "y"]].to_numpy(dtype=np.float64)


def require_gpu(prog, launch):
    """The refusal of a device run without a device; `launch` says what the device would have done."""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{prog}: no GPU visible ({launch}); pass --host for the NumPy form")


def add_window_arguments(p):
    """--ld_window / --ld_window_bp: the window of the ld command and of --ld_prune."""
    p.add_argument("--ld_window", default=100, type=int, metavar="W",
                   help="sites after a site that it is compared with (default 100)")
    p.add_argument("--ld_window_bp", default=None, type=int, metavar="B",
                   help="also compare only sites at most B base pairs apart (needs positions: not with --matrix)")


def check_window(parser, a):
    """The refusals of a window: a size outside 1 .. LOC_LD_MAX_WINDOW, a negative or positionless base-pair limit."""
    from ._abi import LOC_LD_MAX_WINDOW
    if not 1 <= a.ld_window <= LOC_LD_MAX_WINDOW:
        parser.error(f"--ld_window must be 1 .. {LOC_LD_MAX_WINDOW}")
    if a.ld_window_bp is not None and a.ld_window_bp < 0:
        parser.error("--ld_window_bp must be >= 0")
    if a.ld_window_bp is not None and a.matrix is not None:
        parser.error("--ld_window_bp needs positions: a --matrix has none")


KMAX_LIMIT = 64                      # the largest --kmax of the neighbors, paint and ibd commands


def add_k_arguments(p, kmax, averaged, listed=None):
    """--k / --kmax.  kmax: the default; averaged: what k counts ("neighbours"); listed: what the command lists kmax a sample
    of ("neighbours"), None where it lists none."""
    p.add_argument("--k", default="auto", help=f"{averaged} averaged: a number, or `auto` (default): the k in 1 .. --kmax with "
                                               "the smallest leave-one-out median error")
    p.add_argument("--kmax", default=kmax, type=int, help=("" if listed is None else f"{listed} listed per sample and ") +
                   f"largest k tried (default {kmax}, at most {KMAX_LIMIT})")


def check_k(parser, a):
    """The parse-time refusals of --k / --kmax; a.k becomes an int unless it is `auto`."""
    if a.k != "auto":
        try:
            a.k = int(a.k)
        except ValueError:
            parser.error("--k must be `auto` or a whole number")
    if not 1 <= a.kmax <= KMAX_LIMIT:
        parser.error(f"--kmax must be 1 .. {KMAX_LIMIT}")
    if a.k != "auto" and not 1 <= a.k <= a.kmax:
        parser.error(f"--k must be `auto` or 1 .. --kmax ({a.kmax})")


def check_budget(parser, a):
    if not a.budget_gb > 0:
        parser.error("--budget_gb must be positive")


def build_parser(prog, description, own, sample_data=True, prune=True, sample_data_help=None):
    """The command line of a baseline: inputs, site filter and output stem, then what own(parser) adds, then the device.
    sample_data False: the command needs no locations, --sample_data is optional (sample_data_help: what it does with them when
    they are given; prelude then returns locs None without them); prune: the --ld_prune options."""
    p = argparse.ArgumentParser(prog=prog, description=description)
    p.add_argument("--vcf", default=None, help="VCF (optionally gzipped) with the genotypes")
    p.add_argument("--zarr", default=None, help="zarr-v2 callset with calldata/GT and samples")
    p.add_argument("--matrix", default=None, help="tab-separated count matrix: sampleID, then 0 / 1 / 2 per site")
    if sample_data:
        p.add_argument("--sample_data", required=True, help="tab-separated sampleID, x, y; NaN / NA = to be placed")
    else:
        p.add_argument("--sample_data", default=None, help=sample_data_help or "not needed by this command; accepted and not read")
    p.add_argument("--out", required=True, help="output stem")
    p.add_argument("--min_mac", default=2, type=int, help="minimum allele-1 count of a site, as in a fit (default 2)")
    p.add_argument("--max_SNPs", default=None, type=int, help="random subset of sites, drawn as a fit with the same --seed draws it")
    p.add_argument("--seed", default=None, type=int, help="NumPy seed of the --max_SNPs draw")
    own(p)
    if prune:
        p.add_argument("--ld_prune", default=None, type=float, metavar="R2",
                       help="prune the sites first: walking them in input order, a kept site removes every site of its window "
                            "with r2 above R2 (locator_amd.ld); no default threshold")
        add_window_arguments(p)
    p.add_argument("--gpu_number", default=None, type=str, help="the GPU to use (sets HIP_VISIBLE_DEVICES)")
    p.add_argument("--silence", default=False, action="store_true", help="no terminal output")
    return p


def parse_args(parser, argv):
    """parser.parse_args, and the refusal of a command line without exactly one genotype input."""
    a = parser.parse_args(argv)
    if sum(v is not None for v in (a.vcf, a.zarr, a.matrix)) != 1:
        parser.error("exactly one of --vcf / --zarr / --matrix must be given")
    if getattr(a, "ld_prune", None) is not None:
        if not np.isfinite(a.ld_prune):
            parser.error("--ld_prune must be a finite r2 threshold")
        check_window(parser, a)
    return a


def prelude(parser, a, launch, sites=False, phase=False):
    """Parsed arguments -> (c, P, samples, locs, idx): the count matrix of the sites a fit would train on, its ploidy, the sample
    IDs, their locations (None when the command's --sample_data is optional and was not given), the site indices.  Without --host and without a GPU it refuses (require_gpu) before anything is read.
    With --ld_prune the sites are pruned first (ld.prune_sites: in ascending variant index, on the device unless --host); idx
    keeps its survivors in its own order and a.ld_summary holds the entries the summaries gain.  The site tables are read
    only then, or with sites=True (localpca), which appends the CHROM and POS of idx to the answer (None, None for a --matrix).
    phase=True (paint, with sites=True): phased calls are required (read_inputs_sites) and the calls themselves, (variants,
    samples, 2), are appended after them: the haplotype view needs what the counts have summed."""
    if a.gpu_number is not None:
        for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
            os.environ[var] = a.gpu_number
    if not a.host:
        require_gpu(parser.prog, launch)
    from . import genotypes as G
    if a.seed is not None:
        np.random.seed(a.seed)
    prune = getattr(a, "ld_prune", None) is not None
    chrom = pos = None
    if prune or sites:
        gt, samples, chrom, pos = read_inputs_sites(a, parser.prog, phase)
    else:
        gt, samples = read_inputs(a, parser.prog)
    locs = None if a.sample_data is None else read_locations(a.sample_data, samples, parser.prog)
    _, idx = G.filter_snps(gt, min_mac=a.min_mac, max_snps=a.max_SNPs, verbose=False, sites=True)
    try:
        if prune:
            from . import ld
            idx = np.asarray(idx)
            kept = ld.prune_sites(gt, idx, chrom, pos, a.ld_prune, a.ld_window, a.ld_window_bp, a.host)
            a.ld_summary = {"ld_prune": float(a.ld_prune), "ld_window": int(a.ld_window),
                            "ld_window_bp": None if a.ld_window_bp is None else int(a.ld_window_bp), "K_before_prune": int(len(idx))}
            idx = idx[np.isin(idx, kept)]
        c, P = count_matrix(gt, idx)
    except ValueError as e:
        raise SystemExit(f"{parser.prog}: {e}") from None
    if sites:
        at = np.asarray(idx, dtype=np.int64)
        answer = (c, P, samples, locs, idx, None if chrom is None else np.asarray(chrom)[at], None if pos is None else np.asarray(pos)[at])
        return answer + (gt,) if phase else answer
    return c, P, samples, locs, idx


def haplotype_prelude(parser, a, launch, built_for):
    """Parsed arguments of the paint and ibd commands -> (hap, c, P, samples, locs, chrom, pos): prelude's answers for phased
    calls with the sites in ascending variant order (a --max_SNPs draw comes in drawn order), hap int8 [sites][2 samples] the
    site-major haplotype matrix, c the count matrix of the same sites.  built_for: the command's words after "calls of ploidy
    P: " in the refusal of a ploidy other than 2."""
    c, P, samples, locs, idx, chrom, pos, gt = prelude(parser, a, launch, sites=True, phase=True)
    from . import genotypes as G
    try:
        if P != 2:
            raise ValueError(f"calls of ploidy {P}: {built_for}")
        order = np.argsort(idx, kind="stable")
        chrom, pos = (None if t is None else np.asarray(t)[order] for t in (chrom, pos))
        hap, _ = count_matrix_sites(G.haplotypes(np.asarray(gt)), np.asarray(idx)[order])
    except ValueError as e:
        raise SystemExit(f"{parser.prog}: {e}") from None
    return hap, np.ascontiguousarray(c[:, order]), P, samples, locs, chrom, pos
