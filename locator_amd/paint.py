#!/usr/bin/env python3
"""`python -m locator_amd.paint`: the haplotype copying model (Li & Stephens 2003; ChromoPainter, Lawson et al. 2012) and a
placement baseline from it.  Every haplotype is read as a mosaic of the donor haplotypes; the share of its sites copied from
each donor and the expected number of copied chunks come from one normalised forward-backward recursion a recipient.  With
--sample_data a sample is placed at the share-weighted mean location of the donor samples it copies most from.

  python -m locator_amd.paint --vcf phased.vcf.gz --out out/test [--sample_data samples.txt]

  haplotypes  h [K][pitch] int8, site-major: h[j][d] = allele of haplotype column d at site j, 0 or 1, negative = missing;
              column 2 s + a is allele a of sample s.  donor [H] flags, owner [H] the individual of a column, rec [R] the
              recipient columns, rho [K] in [0, 1] the switch probability on entering site j (rho[0] counts as 1), theta in
              [1e-7, 0.5] the mismatch probability.
  model       `copy_host(h, donor, owner, rec, rho, theta, dtype)` -> (share [R][H], chunks [R][H], ll [R], n_donors [R]),
              every operation in `dtype`.  For recipient r: its donors are the columns d with donor[d] set and owner[d] !=
              owner[r], D of them, u = 1 / D.
                e_j(d) = 0 where d is no donor of r, else 1 where either allele is missing, 1 - theta where they are equal,
                  theta where they differ;
                forward, from a-hat_(-1) = 0: p = (1 - rho_j) a-hat_(j-1) + rho_j u, a = e_j p, c_j = sum_d a,
                  a-hat_j = a (1 / c_j); ll = sum_j log c_j in float64;
                backward, from b_(K-1) = u: t = e_j b_j, T = sum_d t, g = a-hat_j b_j, G = sum_d g, gamma = g (1 / G) with
                  1 / G read as 0 where G is below the smallest normal number; b_(j-1) = ((1 - rho_j) (1 / T)) t + rho_j u;
                share = (sum_j gamma) / K: the expected share of the sites copied from d, rows sum to 1;
                chunks = gamma_0 + sum_(j >= 1) xi_j, xi_j(d) = t ((rho_j u (1 / G)) (1 / c_j)): the posterior probability that
                  a chunk copied from d starts at j.  This is gamma_j rho_j u / p_j written without p_j (gamma = p t / (c G)):
                  p_j(d) underflows to 0 over a long stretch without switching and the quotient would be 0 / 0; as written no
                  quotient by a value of a column is formed, rho_j = 0 gives an exact 0, and rho u / G <= c / T keeps every
                  factor in range.
              A recipient with D = 0 gets rows of zeros, ll = 0, n_donors = 0.  K = 0: zeros everywhere.
  switching   rho_j = 1 - exp(-lambda g_j), g_j the base-pair gap to the previous site over the mean within-chromosome gap
              (--uniform: g_j = 1), rho_j = 1 at the first site of a chromosome.  --switch is the first lambda; each of the
              --em_rounds rounds runs at most --em_sample evenly spaced individuals as recipients and sets lambda <- lambda
              (posterior expected switches) / (prior expected switches), both over the sites with rho_j < 1: the posterior
              count is the sum of `chunks` less one for every rho_j = 1 site of a recipient, the prior sum_r sum_j rho_j.  The
              lambda with the largest sum of ll among the rounds (the first on a tie) is used for the final pass.
  theta       default Li & Stephens' 0.5 w / (D + w), w = 1 / sum_(m=1)^(D-1) 1 / m, D the number of donor haplotypes.
  donors      the haplotypes of the located samples (of every sample without --sample_data), with --max_donors M those of every
              ceil(n / M)-th located sample.  Recipients are all haplotypes; nobody copies from their own individual, so a
              located sample's placement is leave-one-out by construction.  The donor columns and as many other samples as
              fit --max_haps columns form one launch group.
  placement   W[s][t] = the sum of the four haplotype shares of sample s in donor sample t.  For k = 1 .. --kmax the placement
              is the W-weighted mean location of the k donor samples with the largest W[s][t] (ties to the lower index); --k
              auto takes the k with the smallest leave-one-out median error, as the neighbors command does.

Outputs: {out}_paint_summary.json, {out}_paint_history.txt (round lambda ll), {out}_paint_donors.txt (sampleID rank donorID
share, share = W / 2), with --sample_data {out}_paint_locs.txt (x,y,sampleID), with --keep_matrix {out}_paint.npz (lengths =
K W / 2 in sites and counts, the sample-level chunk lengths and chunk counts, and samples).  Without a GPU the run stops and
says so; --host asks for the NumPy form in float64.  The device computes in fp32 (loc_paint_copy,
include/locator_hip_paint.h): the files of the two paths agree within round-off and are not byte-identical; each path is
deterministic.  --host_dtype float32 runs the NumPy form in float32, the yardstick the device's round-off is measured against;
--budget_gb bounds the scratch of one launch (the recipients go in batches, which changes no bit).

Not built: recombination maps, per-population donor pools (the posterior per window and label: `python -m
locator_amd.ancestry`), ploidy other than 2, estimating theta.  Unphased calls are phased by
`python -m locator_amd.phase` first.
"""
from __future__ import annotations

import json
import sys

import numpy as np

from . import _abi
from . import baselines as B
from ._files import write_atomic

MAX_HAPS = _abi.LOC_PAINT_MAX_HAPS
THETA_MIN, THETA_MAX = 1e-7, 0.5
PROG = "locator_amd.paint"
LAUNCH = "the recursions are loc_paint_copy launches"
NOTHING_TO_CHOOSE_BY = "no located sample copies from a located donor: nothing to choose k by"
HEAD = ("N", "n_located", "K", "P", "error_unit", "r2_x", "r2_y", "mean_error", "median_error")
OWN = ("H", "n_donor_haps", "groups", "theta", "switch", "uniform", "em_rounds", "em_recipients", "ll", "mean_chunks")
PLACED = ("kmax", "k", "k_auto", "k_chosen_by", "median_error_by_k")
HOST_BATCH_BYTES = 1 << 28          # a-hat of all sites that copy_host keeps for one batch of recipients


# ---------------------------------------------------------------- the definition

def _check(h, donor, owner, rec, rho, theta):
    h = np.asarray(h)
    if h.ndim != 2 or h.dtype != np.int8:
        raise ValueError(f"haplotypes of shape {h.shape} and type {h.dtype}: need int8 [sites][columns]")
    donor, owner, rec = np.asarray(donor), np.asarray(owner, dtype=np.int64), np.asarray(rec, dtype=np.int64)
    H = len(donor)
    if not 1 <= H <= MAX_HAPS:
        raise ValueError(f"{H} haplotype columns: must be 1 .. {MAX_HAPS}")
    if h.shape[1] < H or len(owner) != H:
        raise ValueError(f"{H} donor flags with {len(owner)} owners and rows of {h.shape[1]} columns")
    if len(rec) and (rec.min() < 0 or rec.max() >= H):
        raise ValueError(f"a recipient outside the columns 0 .. {H - 1}")
    rho = np.asarray(rho, dtype=np.float64)
    if rho.shape != (h.shape[0],):
        raise ValueError(f"{rho.shape} switch probabilities for {h.shape[0]} sites")
    if len(rho) > 1 and not (np.isfinite(rho[1:]).all() and rho[1:].min() >= 0 and rho[1:].max() <= 1):
        raise ValueError("a switch probability outside [0, 1]")
    if not THETA_MIN <= float(np.float32(theta)) <= THETA_MAX:
        raise ValueError(f"theta = {theta}: must be {THETA_MIN} .. {THETA_MAX}")
    return h, donor != 0, owner, rec, rho


def emissions(h, j, rcols, dn, theta, dtype):
    """e_j [R][H] of the module text for the recipient columns rcols and their donor flags dn [R][H]."""
    f = np.dtype(dtype).type
    H = dn.shape[1]
    a, x = h[j, rcols][:, None], h[j, :H][None, :]
    e = np.where((a < 0) | (x < 0), f(1), np.where(a == x, f(1) - f(theta), f(theta)))
    return np.where(dn, e, f(0)).astype(dtype)


def forward_batch(h, dn, rcols, rho, theta, dtype):
    """The forward pass of the module text for the recipient columns rcols with the donor flags dn [R][H]: (u [R][1], rho with
    rho[0] = 1 in dtype, a-hat [K][R][H], c [K][R], ll [R] float64).  copy_host and impute.dose_host walk back from it."""
    f = np.dtype(dtype).type
    K, (R, H) = h.shape[0], dn.shape
    u = (f(1) / dn.sum(axis=1).astype(dtype))[:, None]
    rj = np.concatenate([[1.0], rho[1:]]).astype(dtype)
    ah_all, c_all = np.empty((K, R, H), dtype=dtype), np.empty((K, R), dtype=dtype)
    ah, ll = np.zeros((R, H), dtype=dtype), np.zeros(R)
    for j in range(K):
        a = emissions(h, j, rcols, dn, theta, dtype) * ((f(1) - rj[j]) * ah + rj[j] * u)
        c = a.sum(axis=1, dtype=dtype)
        ah = a * (f(1) / c)[:, None]
        ah_all[j], c_all[j] = ah, c
        ll += np.log(c.astype(np.float64))
    return u, rj, ah_all, c_all, ll


def _copy_batch(h, dn, rcols, rho, theta, dtype):
    f = np.dtype(dtype).type
    K, (R, H) = h.shape[0], dn.shape
    u, rj, ah_all, c_all, ll = forward_batch(h, dn, rcols, rho, theta, dtype)
    b = np.broadcast_to(u, (R, H)).astype(dtype)
    sa, ca = np.zeros((R, H), dtype=dtype), np.zeros((R, H), dtype=dtype)
    tiny = np.finfo(dtype).tiny
    for j in range(K - 1, -1, -1):
        t = emissions(h, j, rcols, dn, theta, dtype) * b
        g = ah_all[j] * b
        T, G = t.sum(axis=1, dtype=dtype), g.sum(axis=1, dtype=dtype)
        with np.errstate(divide="ignore"):
            invG = np.where(G >= tiny, f(1) / G, f(0)).astype(dtype)
        gam = g * invG[:, None]
        sa += gam
        ru = rj[j] * u
        ca += gam if j == 0 else t * ((ru[:, 0] * invG) * (f(1) / c_all[j]))[:, None]
        b = ((f(1) - rj[j]) * (f(1) / T))[:, None] * t + ru
    return sa / f(K), ca, ll


def hap_cols(samples):
    """The haplotype columns 2 s, 2 s + 1 of the samples s, in their order."""
    samples = np.asarray(samples)
    return np.stack([2 * samples, 2 * samples + 1], axis=1).reshape(-1)


def _outputs(specs, R, H, K):
    """The outputs of a model function before a recipient ran.  specs: (columns "H", "K" or their number, dtype, the value an
    unrun row holds) an output."""
    return [np.full((R, {"H": H, "K": K}.get(cols, cols)), value, dtype=dtype) for cols, dtype, value in specs]


def _host_model(batch, specs, h, donor, owner, rec, rho, theta, dtype, extra=()):
    """copy_host, impute.dose_host and ancestry.local_host: (the outputs of `specs`, ll [R] float64, n_donors [R] int32) from
    `batch` (_copy_batch, impute._dose_batch, ancestry._local_batch) over the recipients that have a donor, HOST_BATCH_BYTES of
    a-hat at a time.  extra: further inputs that `batch` takes behind dtype."""
    h, donor, owner, rec, rho = _check(h, donor, owner, rec, rho, theta)
    K, H, R = h.shape[0], len(donor), len(rec)
    outs = _outputs(specs, R, H, K)
    ll, n_donors = np.zeros(R), np.zeros(R, dtype=np.int32)
    if K == 0 or R == 0:
        return (*outs, ll, n_donors)
    dn = donor[None, :] & (owner[None, :] != owner[rec][:, None])
    n_donors[:] = dn.sum(axis=1)
    live = np.flatnonzero(n_donors > 0)
    step = max(1, HOST_BATCH_BYTES // (K * H * np.dtype(dtype).itemsize))
    for a in range(0, len(live), step):
        rows = live[a:a + step]
        *got, ll[rows] = batch(h, dn[rows], rec[rows], rho, theta, dtype, *extra)
        for out, part in zip(outs, got):
            out[rows] = part
    return (*outs, ll, n_donors)


def copy_host(h, donor, owner, rec, rho, theta, dtype=np.float64):
    """(share [R][H] dtype, chunks [R][H] dtype, ll [R] float64, n_donors [R] int32): the definition in the module text."""
    return _host_model(_copy_batch, (("H", dtype, 0), ("H", dtype, 0)), h, donor, owner, rec, rho, theta, dtype)


# ---------------------------------------------------------------- the device form

def _device_model(entry, specs, site_bytes, h, donor, owner, rec, rho, theta, block, pitch, pad_fill, fill, budget, device, extra=()):
    """copy_device, impute.dose_device and ancestry.local_device: _host_model's answer from launches of the entry point `entry`,
    which takes the outputs of `specs` before ll.  The recipients go in batches whose scratch, and site_bytes a site of a
    recipient and the outputs of a fixed number of columns beside it, stay within `budget` bytes; an output without columns
    (K = 0) is not copied back.  extra: further inputs that `entry` takes between block and the outputs, a NumPy array (uploaded
    as it is) or a number each."""
    import torch as t
    from . import _device as D, _lib
    lib = _lib.load()
    h, dflag, owner, rec, rho = _check(h, donor, owner, rec, rho, theta)
    K, H, R = h.shape[0], len(dflag), len(rec)
    buf = B.padded(np.ascontiguousarray(h[:, :H]), pitch, pad_fill)
    with t.cuda.device(device):
        d_h, d_donor, d_owner = D.put(buf, np.int8, device), D.put(dflag, np.uint8, device), D.put(owner, np.int32, device)
        d_rho = D.put(rho if K else np.zeros(1), np.float32, device)
        one = int(lib.loc_paint_work_bytes(H, K, 1, int(block)))
        if one < 0:
            _lib.check(-1, "loc_paint_work_bytes")
        outs = _outputs(specs, R, H, K)
        fixed = sum(out.shape[1] * out.itemsize for out, spec in zip(outs, specs) if spec[0] not in ("H", "K"))
        step = max(1, int(budget) // max(one + site_bytes * K + fixed, 1))
        d_extra = [D.put(x, None, device) if isinstance(x, np.ndarray) else x for x in extra]
        ll, n_donors = np.zeros(R), np.zeros(R, dtype=np.int32)
        for a in range(0, R, step):
            n = min(step, R - a)
            d_rec = D.put(rec[a:a + n], np.int32, device)
            d_outs = [t.empty((n, max(out.shape[1], 1)), dtype=getattr(t, out.dtype.name), device=device) for out in outs]
            d_ll = t.empty(n, dtype=t.float64, device=device)
            d_nd = t.empty(n, dtype=t.int32, device=device)
            d_work, work_bytes = D.work_buffer(lib, "loc_paint_work_bytes", H, K, n, int(block), device=device, fill=fill)
            D.prefill((*d_outs, d_ll, d_nd), fill)
            _lib.check(getattr(lib, entry)(d_h.data_ptr(), H, K, int(buf.shape[1]), d_donor.data_ptr(), d_owner.data_ptr(),
                                           d_rec.data_ptr(), n, d_rho.data_ptr(), float(theta), int(block),
                                           *(x.data_ptr() if isinstance(x, t.Tensor) else x for x in d_extra),
                                           *(d.data_ptr() for d in d_outs), d_ll.data_ptr(), d_nd.data_ptr(), d_work.data_ptr(),
                                           work_bytes, D.stream()), entry)
            for out, d in zip(outs, d_outs):
                if out.shape[1]:
                    out[a:a + n] = d.cpu().numpy()
            ll[a:a + n], n_donors[a:a + n] = d_ll.cpu().numpy(), d_nd.cpu().numpy()
            del d_work
    return (*outs, ll, n_donors)


def copy_device(h, donor, owner, rec, rho, theta, block=0, pitch=None, pad_fill=-1, fill=None, budget=4 << 30, device="cuda:0"):
    """copy_host's answer from loc_paint_copy launches (share and chunks float32), the recipients in batches whose scratch
    stays within `budget` bytes.  fill: a 32-bit pattern that scratch and the outputs hold before a launch (tests)."""
    return _device_model("loc_paint_copy", (("H", np.float32, 0), ("H", np.float32, 0)), 0, h, donor, owner, rec, rho, theta, block,
                         pitch, pad_fill, fill, budget, device)


# ---------------------------------------------------------------- the driver's pieces

def site_gaps(chrom, pos, K, uniform=False):
    """(g float64 [K], first bool [K]): the gap of every site to the one before it over the mean within-chromosome gap, and
    the first sites of the chromosomes.  Without positions, with --uniform or when no gap is positive every g is 1."""
    first = np.zeros(K, dtype=bool)
    if K:
        first[0] = True
    if chrom is not None and K:
        chrom = np.asarray(chrom).astype(str)
        first[1:] = chrom[1:] != chrom[:-1]
    g = np.ones(K)
    if pos is not None and not uniform and K > 1:
        d = np.diff(np.asarray(pos, dtype=np.float64), prepend=0.0)
        inside = ~first
        if (d[inside] < 0).any():
            raise ValueError("the positions of a chromosome are not in ascending order")
        mean = d[inside].mean() if inside.any() else 0.0
        if mean > 0:
            g = np.where(inside, d / mean, 1.0)
    return g, first


def switch_rates(lam, g, first):
    """rho float32 [K]: 1 - exp(-lambda g), 1 at the first site of a chromosome."""
    return np.where(first, 1.0, -np.expm1(-float(lam) * g)).astype(np.float32)


def default_theta(D):
    """Li & Stephens' mismatch probability for D donor haplotypes, kept inside the model's range."""
    if D < 2:
        return THETA_MAX
    w = 1.0 / sum(1.0 / m for m in range(1, D))
    return float(min(max(0.5 * w / (D + w), THETA_MIN), THETA_MAX))


def em_update(lam, rho, chunks, n_donors):
    """lambda (posterior expected switches) / (prior expected switches) over the sites with rho < 1 and the recipients that
    have a donor; lambda itself where either count is not positive."""
    rho = np.asarray(rho, dtype=np.float64)
    live = int((np.asarray(n_donors) > 0).sum())
    post = float(np.asarray(chunks, dtype=np.float64).sum()) - live * int((rho >= 1).sum())
    prior = live * float(rho[rho < 1].sum())
    return float(lam) * post / prior if post > 0 and prior > 0 else float(lam)


def launch_groups(N, donor_samples, max_haps):
    """[(columns' samples, recipient samples)]: every group holds the donor samples first, then as many other samples as fit
    max_haps columns; the donors are recipients of the first group."""
    donor_samples = np.asarray(donor_samples, dtype=np.int64)
    others = np.setdiff1d(np.arange(N, dtype=np.int64), donor_samples)
    room = max_haps // 2 - len(donor_samples)
    if len(others) and room < 1:
        raise ValueError("no column is left for a recipient beside the donors")
    groups = [(np.concatenate([donor_samples, others[:max(room, 0)]]), np.concatenate([donor_samples, others[:max(room, 0)]]))]
    for a in range(max(room, 0), len(others), max(room, 1)):
        part = others[a:a + room]
        groups.append((np.concatenate([donor_samples, part]), part))
    return groups


def group_columns(N, donor_samples, max_haps):
    """launch_groups as a launch takes them, a group a tuple: cols (its samples), at (where its recipient samples are in cols),
    hcols (its haplotype columns of the whole matrix), donor and owner of its columns, rec (the recipients' columns in it)."""
    for cols, recs in launch_groups(N, donor_samples, max_haps):
        at = np.flatnonzero(np.isin(cols, recs))
        yield (cols, at, hap_cols(cols), np.repeat(np.isin(cols, donor_samples), 2).astype(np.uint8),
               np.repeat(np.arange(len(cols), dtype=np.int32), 2), hap_cols(at))


def sample_weights(copy, hap, donor_samples, rho, theta, max_haps=MAX_HAPS, recipients=None):
    """The model over launch groups, folded to samples: (W [N][N] = the four haplotype shares of sample s in sample t summed,
    C [N][N] likewise of chunks, ll [2N], n_donors [2N], number of groups).  hap int8 [K][2N]; copy: copy_host or copy_device
    with the leading six arguments; recipients: the samples to run (default all), the others keep rows of zeros."""
    K, H2 = hap.shape
    N = H2 // 2
    W, C = np.zeros((N, N)), np.zeros((N, N))
    ll, nd = np.zeros(2 * N), np.zeros(2 * N, dtype=np.int32)
    wanted = np.ones(N, dtype=bool) if recipients is None else np.isin(np.arange(N), recipients)
    n_groups = 0
    for n_groups, (cols, at, hcols, donor, owner, rec) in enumerate(group_columns(N, donor_samples, max_haps), 1):
        run = wanted[cols[at]]
        at, rec = at[run], rec[np.repeat(run, 2)]
        if not len(at):
            continue
        share, chunks, l, n = copy(np.ascontiguousarray(hap[:, hcols]), donor, owner, rec, rho, theta)
        fold = lambda m: np.asarray(m, dtype=np.float64).reshape(len(at), 2, len(cols), 2).sum(axis=(1, 3))
        W[np.ix_(cols[at], cols)] = fold(share)
        C[np.ix_(cols[at], cols)] = fold(chunks)
        ll[hap_cols(cols[at])], nd[hap_cols(cols[at])] = l, n
    return W, C, ll, nd, n_groups


def estimate_switch(copy, hap, donors, g, first, switch, em_rounds, em_sample, theta, max_haps=MAX_HAPS, pool=None):
    """(lambda, history [(round, lambda, sum of ll)], the recipient samples of the rounds): the module text's estimate of the
    switch rate from the first value `switch`.  pool: the samples the recipients are spread over evenly (default all)."""
    pool = np.arange(hap.shape[1] // 2) if pool is None else np.asarray(pool, dtype=np.int64)
    m = min(em_sample, len(pool))
    em_recipients = pool[np.unique((np.arange(m) * len(pool)) // max(m, 1))]
    history, lam = [], float(switch)
    for t in range(em_rounds):
        rho = switch_rates(lam, g, first)
        _, C, ll, nd, _ = sample_weights(copy, hap, donors, rho, theta, max_haps, em_recipients)
        history.append((t, lam, float(ll.sum())))
        # C holds the chunks of the recipients that ran, folded over haplotypes: its sum is theirs
        lam = em_update(lam, rho, C, nd)
    if history:
        lam = max(history, key=lambda r: (r[2], -r[0]))[1]
    return lam, history, em_recipients


def checked_options(prog, switch, em_rounds, em_sample, theta, n_donor_haps):
    """The refusals of the model's options that the paint and impute commands share; returns theta, the default for
    n_donor_haps donor haplotypes where none is given."""
    if not (np.isfinite(switch) and switch > 0):
        raise SystemExit(f"{prog}: --switch must be a positive number")
    if em_rounds < 0 or em_sample < 1:
        raise SystemExit(f"{prog}: --em_rounds must be >= 0 and --em_sample >= 1")
    if theta is None:
        theta = default_theta(n_donor_haps)
    if not THETA_MIN <= theta <= THETA_MAX:
        raise SystemExit(f"{prog}: --theta must be {THETA_MIN} .. {THETA_MAX}")
    return theta


def check_room(prog, room, n_donors, max_haps, of):
    """The refusal of donors that leave no column of a launch to a recipient.  of: whom --max_donors thins, in the command's words."""
    if room > max_haps:
        raise SystemExit(f"{prog}: {2 * n_donors} donor haplotypes and a recipient do not fit {max_haps} columns (--max_haps, at "
                         f"most {MAX_HAPS}: a wave holds a value a column in registers); pass --max_donors M to take every "
                         f"ceil(n / M)-th {of} as a donor, M <= {max_haps // 2 - 1}")


def model_form(on_host, on_device, host, dtype, budget, device):
    """on_host in `dtype` or on_device within `budget` on `device`, as a function of the model's six leading arguments."""
    if host:
        return lambda *six: on_host(*six, dtype=dtype)
    return lambda *six: on_device(*six, budget=budget, device=device)


def write_history(path, history):
    write_atomic(path, "round\tswitch\tll\n" + "".join(f"{t}\t{l!r}\t{v!r}\n" for t, l, v in history))


# the placement from a sample-by-sample weight is shared with the ibd command: baselines.py holds it, these are its names here
top_donors, placements = B.top_donors, B.placements


# ---------------------------------------------------------------- the command's work

def paint(hap, c, P, samples, locs, chrom=None, pos=None, out=None, switch=0.01, em_rounds=3, em_sample=256, theta=None,
          uniform=False, max_donors=None, max_haps=MAX_HAPS, k="auto", kmax=16, longlat=False, keep_matrix=False, host=False,
          silence=False, device="cuda:0", budget=4 << 30, dtype=np.float64):
    """The command's work for a site-major haplotype matrix hap [K][2N] (c: the count matrix of the same sites, for the shared
    summary entries): returns the summary dict and writes the output files when `out` is given.  locs None: no locations.
    dtype: the arithmetic of --host."""
    hap = np.ascontiguousarray(hap, dtype=np.int8)
    K, H = hap.shape
    N = H // 2
    samples = np.asarray(samples).astype(str)
    if H != 2 * N or len(samples) != N or N < 2:
        raise SystemExit(f"{PROG}: {H} haplotype columns for {len(samples)} samples: needs two a sample and two samples at least")
    if K == 0:
        raise SystemExit(f"{PROG}: no site is left after the filters: nothing to paint")
    if not 2 <= max_haps <= MAX_HAPS:
        raise SystemExit(f"{PROG}: --max_haps must be 2 .. {MAX_HAPS}")
    if max_donors is not None and max_donors < 1:
        raise SystemExit(f"{PROG}: --max_donors must be >= 1")
    located = None
    if locs is not None:
        locs, located = B.located_mask(locs, N, PROG)
    pool = np.arange(N) if located is None else np.flatnonzero(located)
    donors = pool if max_donors is None else pool[::-(-len(pool) // max_donors)]
    check_room(PROG, 2 * len(donors) + (2 if len(donors) < N else 0), len(donors), max_haps, f"of the {len(pool)} candidate samples")
    theta = checked_options(PROG, switch, em_rounds, em_sample, theta, 2 * len(donors))
    if k != "auto" and not 1 <= int(k) <= kmax or not 1 <= kmax <= B.KMAX_LIMIT:
        raise SystemExit(f"{PROG}: --kmax must be 1 .. {B.KMAX_LIMIT} and --k `auto` or 1 .. --kmax")
    if not host:
        B.require_gpu(PROG, LAUNCH)
    copy = model_form(copy_host, copy_device, host, dtype, budget, device)
    g, first = site_gaps(chrom, pos, K, uniform)

    lam, history, em_recipients = estimate_switch(copy, hap, donors, g, first, switch, em_rounds, em_sample, theta, max_haps)
    rho = switch_rates(lam, g, first)
    W, C, ll, nd, n_groups = sample_weights(copy, hap, donors, rho, theta, max_haps)

    own = {"H": int(H), "n_donor_haps": int(2 * len(donors)), "groups": int(n_groups), "theta": float(theta), "switch": float(lam),
           "uniform": bool(uniform or pos is None), "em_rounds": int(em_rounds), "em_recipients": int(2 * len(em_recipients)),
           "ll": B.num(ll.sum()), "mean_chunks": B.num(C.sum() / max(int((nd > 0).sum()), 1))}
    xy, head, placed_own, lines, nbr, weight = B.place_by_weight(PROG, W, np.isin(np.arange(N), donors), kmax, k, c, P, locs, located,
                                                                 longlat, "copying", NOTHING_TO_CHOOSE_BY)
    summary = B.assemble_summary(head or {"N": int(N), "K": int(K), "P": int(P)}, own, placed_own, HEAD, OWN, PLACED, host)
    lines = [f"{N} samples, {K} sites: {H} haplotypes copy from {2 * len(donors)} donor haplotypes in {n_groups} launch group(s)",
             f"theta {theta!r}, switch rate {lam!r} after {em_rounds} rounds, ll {own['ll']!r}, {own['mean_chunks']!r} chunks a "
             f"haplotype", *lines]
    if out is not None:
        write_history(out + "_paint_history.txt", history)
        rows = ["sampleID\trank\tdonorID\tshare\n"]
        for s in range(N):
            for r in range(nbr.shape[1]):
                if nbr[s, r] < 0:
                    break
                rows.append(f"{samples[s]}\t{r + 1}\t{samples[nbr[s, r]]}\t{float(weight[s, r] / 2)!r}\n")
        write_atomic(out + "_paint_donors.txt", "".join(rows))
        write_atomic(out + "_paint_summary.json", json.dumps(summary, indent=1) + "\n")
        if xy is not None:
            B.write_locs(out + "_paint_locs.txt", xy, samples)
        if keep_matrix:
            write_atomic(out + "_paint.npz", lambda fh: B.save_npz(fh, lengths=K * W / 2, counts=C, samples=samples), mode="wb")
    if not silence:
        for line in lines:
            print(line)
    summary["_W"], summary["_C"], summary["_xy"], summary["_history"], summary["_ll"] = W, C, xy, history, ll
    return summary


# ---------------------------------------------------------------- command

def add_model_arguments(p):
    """The model's options of the paint and impute commands."""
    p.add_argument("--switch", default=0.01, type=float, help="first switch rate lambda a mean gap (default 0.01)")
    p.add_argument("--em_rounds", default=3, type=int, help="rounds that re-estimate the switch rate (default 3)")
    p.add_argument("--em_sample", default=256, type=int, help="individuals used as recipients of those rounds at most (default 256)")
    p.add_argument("--theta", default=None, type=float, help=f"mismatch probability, {THETA_MIN} .. {THETA_MAX} (default: Li & "
                                                             "Stephens' from the number of donor haplotypes)")
    p.add_argument("--uniform", default=False, action="store_true", help="every site one mean gap from the one before it")
    p.add_argument("--max_donors", default=None, type=int, metavar="M", help="take every ceil(n / M)-th candidate sample as a donor")
    p.add_argument("--max_haps", default=MAX_HAPS, type=int, help=f"haplotype columns of a launch at most (default and limit {MAX_HAPS})")


def add_path_arguments(p, budget_help, host_help):
    """--budget_gb, --host and --host_dtype of the two commands; what a launch's budget holds and what --host changes differ."""
    p.add_argument("--budget_gb", default=4.0, type=float, help=budget_help)
    p.add_argument("--host", default=False, action="store_true", help=host_help)
    p.add_argument("--host_dtype", default="float64", choices=("float64", "float32"),
                   help="the arithmetic of --host (float32: what the device's round-off is measured against)")


def _own_arguments(p):
    add_model_arguments(p)
    B.add_k_arguments(p, 16, "donor samples", "donors")
    p.add_argument("--longlat", default=False, action="store_true",
                   help="x / y are longitude / latitude degrees: errors are great-circle km (the mean stays planar)")
    p.add_argument("--keep_matrix", default=False, action="store_true",
                   help="keep the sample-level chunk lengths, chunk counts and the sample IDs in {out}_paint.npz")
    add_path_arguments(p, "device scratch of a launch at most, GiB (default 4)",
                       "the NumPy form in float64 instead of the GPU (the files differ as the module text says)")


def build_parser():
    return B.build_parser(PROG, "The haplotype copying model: copying shares, chunk counts and a placement baseline.", _own_arguments,
                          sample_data=False, prune=False, sample_data_help="tab-separated sampleID, x, y; NaN / NA = to be placed.  "
                          "Optional: the located samples are the donors; without it every sample is one and no placement is made")


def main(argv=None):
    parser = build_parser()
    a = B.parse_args(parser, argv)
    B.check_k(parser, a)
    B.check_budget(parser, a)
    hap, c, P, samples, locs, chrom, pos = B.haplotype_prelude(parser, a, LAUNCH, "the copying model is built for two haplotypes a sample")
    try:
        paint(hap, c, P, samples, locs, chrom, pos, a.out, a.switch, a.em_rounds, a.em_sample, a.theta,
              a.uniform, a.max_donors, a.max_haps, a.k, a.kmax, a.longlat, a.keep_matrix, a.host, a.silence,
              budget=int(a.budget_gb * (1 << 30)), dtype=np.dtype(a.host_dtype).type)
    except ValueError as e:
        raise SystemExit(f"{PROG}: {e}") from None
    return 0


if __name__ == "__main__":
    sys.exit(main())
