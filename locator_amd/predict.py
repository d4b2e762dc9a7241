#!/usr/bin/env python3
"""`python -m locator_amd.predict`: place new samples with kept models (`--keep_model` files), without training.

  python -m locator_amd.predict --model out/run.model.npz --vcf new.vcf.gz --out out/new
  python -m locator_amd.predict --model out/boot_dir --zarr new.zarr --samples ids.txt --out out/new
  python -m locator_amd.predict --model out/run.model.npz --vcf imputed.vcf.gz --dosage --out out/new     (FORMAT/DS; GP: --dosage GP)

Every model's sites are matched to the query on the host (locator_amd/query.py); everything that can be
refused is refused before any device work.  The calls of the matched variants go to the device once; every model of the
set builds its own rows from that copy (loc_query_rows) and predicts them.  With --dosage the query is read as expected
alt-allele dosages (imputed or low-coverage samples); the rows are built in the fixed-point unit q = rint(63 d)
(loc_query_rows_dosage) and the model runs on d = q / 63.  Outputs, each written atomically:
  one model:     {out}_predlocs.txt
  several:       {out}_{model stem}_predlocs.txt each, and {out}_centroids.txt (what `python -m locator_amd.summarize`
                 computes over those files)
  always:        {out}_sites.txt - per model: SNPs, matched, matched with an allele other than 1, absent
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(prog="locator_amd.predict",
                                description="Predict the locations of new samples with models kept by --keep_model.")
    p.add_argument("--model", nargs="+", required=True,
                   help="one or more .model.npz files, or directories holding them")
    p.add_argument("--vcf", help="query genotypes: VCF (optionally gzipped)")
    p.add_argument("--zarr", help="query genotypes: zarr-v2 store with calldata/GT, samples and variants/CHROM, POS, REF, ALT")
    p.add_argument("--matrix", help="query genotypes: tab-delimited sampleID + one 0/1/2 column per site (matched by name)")
    p.add_argument("--samples", default=None,
                   help="file of query sample IDs to predict, one per line (default: every query sample)")
    p.add_argument("--out", required=True, help="stem of every output file")
    p.add_argument("--min_site_overlap", default=0.5, type=float,
                   help="refuse a model of which fewer than this fraction of sites are in the query (default 0.5)")
    p.add_argument("--impute_missing", default=False, action="store_true",
                   help="missing calls at matched sites: Binomial(ploidy, training allele frequency) instead of 0")
    p.add_argument("--seed", default=None, type=int, help="NumPy seed of the --impute_missing draws")
    p.add_argument("--gpu_number", default=None, type=str, help="run on this GPU index")
    p.add_argument("--dosage", default=None, nargs="?", const="DS", choices=("DS", "GP"),
                   help="read the query as expected alt-allele dosages instead of GT calls: FORMAT/DS (bare --dosage; "
                        "calldata/DS of a zarr store, float values of a --matrix) or FORMAT/GP as GP1 + 2 GP2 (VCF only)")
    p.add_argument("--predict_mode", default="auto", choices=("auto", "exact", "fast"),
                   help="first-layer arithmetic of many-row predictions (as the training command's flag)")
    p.add_argument("--predict_pieces", default=None, type=int, help="as the training command's flag")
    return p


def _read_ids(path):
    with open(path) as fh:
        return [line.strip() for line in fh if line.strip()]


def _centroids(paths, out, write):
    """{out}_centroids.txt over the predlocs files, exactly as summarize.summarize reads and groups them (name order)."""
    import pandas as pd

    from . import summarize as S
    files = sorted(paths, key=os.path.basename)
    aeg = pd.concat([pd.read_csv(f) for f in files], ignore_index=True).rename(columns={"x": "xpred", "y": "ypred"})
    groups = [(sid, g["xpred"].to_numpy(), g["ypred"].to_numpy()) for sid, g in aeg.groupby("sampleID", sort=False)]
    dev = S.device_summaries([(x, y) for _, x, y in groups])[1]
    rows = [{"sampleID": sid, "x": np.nan, "y": np.nan, "kd_x": float(d[0]), "kd_y": float(d[1]), "gc_x": float(d[2]),
             "gc_y": float(d[3])} for (sid, _, _), d in zip(groups, dev)]
    frame = pd.DataFrame(rows, columns=["sampleID", "x", "y", "kd_x", "kd_y", "gc_x", "gc_y"])
    write(out + "_centroids.txt", lambda fh: frame.to_csv(fh, index=False, sep="\t"))


def main(argv=None):
    t0 = time.time()
    a = build_parser().parse_args(argv)
    if a.gpu_number is not None:
        for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
            os.environ[var] = a.gpu_number
    if a.seed is not None:
        np.random.seed(a.seed)
    from . import genotypes as G
    from . import query as Q
    from ._files import write_atomic
    from .locator import _to_map_units, predict_settings, write_predlocs

    # ---- host: read, match, refuse (nothing on the device yet)
    models = [Q.load_model(p) for p in Q.model_paths(a.model)]
    if len({(m["phased"], m["ploidy"]) for m in models}) > 1:
        raise Q.QueryRefused("--model: phased and unphased models (or models of different ploidy) cannot share one query")
    stems = [m["stem"] for m in models]
    if len(set(stems)) != len(stems):
        raise Q.QueryRefused("--model: two model files share the name stem " + repr(sorted(s for s in stems if stems.count(s) > 1)[0]))
    dosage = a.dosage is not None
    query = Q.read_query_dosage(a.vcf, a.zarr, a.matrix, a.dosage) if dosage else Q.read_query(a.vcf, a.zarr, a.matrix)
    columns, reports = [], []
    for m in models:
        cv, ca, rep = Q.match_sites(m, query)
        (Q.check_query_dosage if dosage else Q.check_query)(m, query, rep, a.min_site_overlap)
        columns.append((cv, ca))
        reports.append(rep)
    phased = models[0]["phased"]
    idx = Q.select_samples(query, _read_ids(a.samples) if a.samples else None)
    rows = ((2 * idx[:, None] + np.arange(2)).reshape(-1) if phased else idx).astype(np.int32)
    ids = query["samples"][idx]
    if phased:
        ids = np.array([f"{s}_h{h}" for s in ids for h in (0, 1)], dtype=object)
    calls, remapped, _ = (Q.compact_dosages if dosage else Q.compact_calls)(query, columns)
    if a.impute_missing:
        # every matched variant once, with the allele and frequency of the first model column that uses it
        every = (np.concatenate(remapped), np.concatenate([ca for _, ca in columns]), np.concatenate([m["af"] for m in models]))
        if dosage:
            Q.impute_dosages(calls, rows, *every)
        else:
            Q.impute_calls(calls, rows, *every, phased)
    for m, (cv, _) in zip(models, columns):
        m["weights_used"] = Q.absent_gamma(m["weights"], cv)

    def sites_report(fh):
        fh.write("model\tsnps\tmatched\tallele_not_1\tabsent\n")
        for r in reports:
            fh.write(f"{r['model']}\t{r['K']}\t{r['matched']}\t{r['allele_not_1']}\t{r['absent']}\n")
    write_atomic(a.out + "_sites.txt", sites_report)
    for r in reports:
        print(f"{r['model']}: {r['matched']} of {r['K']} sites matched ({r['allele_not_1']} with allele != 1), "
              f"{r['absent']} absent")

    # ---- device: one upload of the matched calls, then rows + predict per model
    import torch

    from .net import require_gpu
    require_gpu()
    dev = "cuda:0"
    calls_dev = torch.from_numpy(calls).to(dev)
    if phased:
        U, N, P = calls.shape
        calls_dev = calls_dev.view(U, N * P, 1)
    settings = predict_settings(a)
    written = []
    for m, cv, (_, ca) in zip(models, remapped, columns):
        if dosage:
            X = Q.query_rows_dosage(calls_dev, cv, ca, rows, m["K"])
            z = Q.predict_rows(m, X, settings, dev, unit=G.DOSAGE_UNIT)
        else:
            X = Q.query_rows(calls_dev, cv, ca, rows, m["K"])
            z = Q.predict_rows(m, X, settings, dev)
        del X
        meanlong, sdlong, meanlat, sdlat = m["locs_norm"]
        xy = _to_map_units(z, sdlong, meanlong, sdlat, meanlat)
        path = a.out + "_predlocs.txt" if len(models) == 1 else f"{a.out}_{m['stem']}_predlocs.txt"
        write_predlocs(path, xy, ids)
        written.append(path)
    if len(models) > 1:
        _centroids(written, a.out, write_atomic)
    print(f"predicted {len(ids)} rows with {len(models)} model(s) in {time.time() - t0:.2f} s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
