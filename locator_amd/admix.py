#!/usr/bin/env python3
"""`python -m locator_amd.admix`: model-based ancestry proportions (the model of STRUCTURE, FRAPPE and ADMIXTURE) and the
Q-regression placement baseline.  Every sample gets its shares q_i of C ancestral clusters, every cluster its allele-1
frequencies, by accelerated EM on the binomial likelihood; with --sample_data the located samples' x and y are regressed on the
shares, the counterpart of the PC regression of the pca command.

  python -m locator_amd.admix --vcf genotypes.vcf.gz --pops 4 --out out/test [--sample_data samples.txt]

  counts      c [N][K] int8 exactly as the other baselines take them (baselines.prelude): -1 = missing, 0 .. P.
  model       Q [N][C], rows on the simplex; F [K][C], the allele-1 frequency of cluster c at site k; 2 <= C <= 16; EPS = 1e-5.
              c_ik ~ Binomial(P, h_ik), h_ik = sum_c Q_ic F_kc.
  step        `step_host(c, P, Q, F, dtype)` -> (Q', F', ll), FRAPPE's EM map, every operation in `dtype`.  With m = [c >= 0],
              g = m c, r = m (P - c), Fb = 1 - F:
                h = sum_c Q_ic F_kc and hb = sum_c Q_ic Fb_kc, clusters added in ascending order.  hb is a sum of its own, never
                  1 - h: every sum of the step then has non-negative terms only, which keeps float32 within round-off of
                  float64 also where frequencies sit at the bounds;
                a = g / h, b = r / hb, both 0 where the call is missing;
                ll = sum g log h + r log hb, the log-likelihood of the INPUT (Q, F); its terms are in `dtype`, their sum float64;
                A_kc = sum_i Q_ic a_ik, B_kc = sum_i Q_ic b_ik; F' = F A / (F A + Fb B), F where that denominator is 0 (no called
                  sample); then clipped to [EPS, 1 - EPS];
                S_ic = sum_k (F_kc a_ik + Fb_kc b_ik), n_i = sum_k m; Q' = Q S / (P n_i), Q where n_i = 0; then max(., EPS) and
                  divided by the sum of the row (clusters added in ascending order).
              With no sample or no site nothing moves: (Q, F, 0).
  fit         `fit_host`: the start is np.random.default_rng(init_seed): Q = dirichlet(ones(C), N), F = uniform(0.1, 0.9, (K, C)),
              both rounded to float32 (host and device start from the same bits; np.random's global state, which --seed sets for
              --max_SNPs, is not touched).  Round t = 0, 1, ... with accel = "squarem" (Varadhan & Roland's S3):
                x1 = M(x0) gives ll0_t; x2 = M(x1) gives ll1; r = x1 - x0, v = (x2 - x1) - r over Q and F together;
                alpha = -max(1, |r| / |v|), norms in float64, alpha = -1 when |v| = 0; xa = (x0 - 2 alpha r) + alpha^2 v, projected
                as the step projects (clip F, floor and renormalise Q); x3 = M(xa) gives lla; the next x0 is x3 if lla >= ll1
                (accepted), else x2.  In exact arithmetic ll0_t cannot decrease.
              With accel = "none" a round is one step.  Round t >= 1 stops after its first step when
              ll0_t - ll0_(t-1) < tol P sum_i n_i: the result is that round's x0 with ll = ll0_t.  After max_rounds whole rounds
              one more step gives the ll of the result and converged = False.
  labels      after the fit the clusters are renumbered by descending sum_i Q_ic, ties to the lower index.
  placement   `placements`: over the located samples x and y are regressed by least squares on [1, q_1 .. q_(C-1)]; a located
              sample gets its leave-one-out prediction by the hat matrix, (yhat_i - h_ii y_i) / (1 - h_ii), NaN where
              1 - h_ii < 1e-9; an unlocated one the full fit's prediction.  Fewer than C + 1 located samples: no placement.

Outputs: {out}_admix_Q.txt (sampleID q1 .. qC), {out}_admix_history.txt (round ll accepted: accepted is 1 / 0 for a squarem
round, 1 for a plain one, NA for the closing line, which holds the ll of the result), {out}_admix_summary.json, with
--sample_data {out}_admix_locs.txt (x,y,sampleID as {out}_knn_locs.txt), with --keep_frequencies {out}_admix_frequencies.npz
(idx, F, samples).  --ld_prune as in the other baselines.  Without a GPU the run stops and says so; --host asks for the NumPy
form.

The device steps in fp32 (loc_admix_step, include/locator_hip_admix.h), --host in float64: the files of the two paths are not
byte-identical.  One step agrees within (max(N, K) + 32) 2^-23 relative; with SQUAREM's accept / reject branch two arithmetic
forms may part on a round and reach slightly different points of the same flat top of the likelihood.
Each path is deterministic: two runs of it write the same bytes.

Not built: choosing C by cross-validation, several starts, supervised ancestry, --dosage and --phased inputs, ploidy above 2.
"""
from __future__ import annotations

import json
import sys

import numpy as np

from . import _abi
from . import baselines as B
from ._files import write_atomic

MAX_POPS = _abi.LOC_ADMIX_MAX_POPS
LL_RUN = _abi.LOC_ADMIX_LL_RUN
TILE = _abi.LOC_ADMIX_TILE
BLOCK = _abi.LOC_ADMIX_BLOCK
EPS = 1e-5
ACCELS = ("squarem", "none")
PROG = "locator_amd.admix"
LAUNCH = "the EM steps are loc_admix_step launches"
# the key order of {out}_admix_summary.json: HEAD with a placement, ("N", "K", "P") without; then OWN, --ld_prune's, "path"
HEAD = ("N", "n_located", "K", "P", "error_unit", "r2_x", "r2_y", "mean_error", "median_error")
OWN = ("C", "rounds", "steps", "converged", "ll", "ll_per_allele", "tol", "accel", "init_seed", "cluster_sizes")


# ---------------------------------------------------------------- the definitions

def _check_model(c, Q, F):
    N, K = c.shape
    if Q.ndim != 2 or F.ndim != 2 or Q.shape[0] != N or F.shape[0] != K or Q.shape[1] != F.shape[1]:
        raise ValueError(f"Q of shape {Q.shape} and F of shape {F.shape} with counts of shape {c.shape}: need [N][C] and [K][C]")
    if not 2 <= Q.shape[1] <= MAX_POPS:
        raise ValueError(f"C = {Q.shape[1]}: must be 2 .. {MAX_POPS}")


def project(Q, F):
    """The projection a step ends with: F clipped to [EPS, 1 - EPS]; Q floored at EPS and divided by the sum of its row, the
    clusters added in ascending order.  Works in the dtype of its arguments."""
    f = Q.dtype.type
    F = np.minimum(np.maximum(F, F.dtype.type(EPS)), F.dtype.type(1) - F.dtype.type(EPS))
    Q = np.maximum(Q, f(EPS))
    s = Q[:, 0].copy()
    for x in range(1, Q.shape[1]):
        s = s + Q[:, x]
    return Q / s[:, None], F


def step_host(c, P, Q, F, dtype=np.float64):
    """(Q', F', ll): one EM step, the definition in the module text."""
    c = B.check_counts(c, P)
    N, K = c.shape
    f = np.dtype(dtype).type
    Q, F = np.asarray(Q).astype(dtype), np.asarray(F).astype(dtype)
    _check_model(c, Q, F)
    C = Q.shape[1]
    if N == 0 or K == 0:
        return Q, F, 0.0
    m = c >= 0
    g = np.where(m, c, 0).astype(dtype)
    r = np.where(m, P - c, 0).astype(dtype)
    Fb = f(1) - F
    h, hb = np.zeros((N, K), dtype=dtype), np.zeros((N, K), dtype=dtype)
    for x in range(C):
        h += Q[:, x, None] * F[None, :, x]
        hb += Q[:, x, None] * Fb[None, :, x]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(m, g / h, f(0))
        b = np.where(m, r / hb, f(0))
        terms = np.where(m, g * np.log(h), f(0)), np.where(m, r * np.log(hb), f(0))
    ll = float(terms[0].sum(dtype=np.float64) + terms[1].sum(dtype=np.float64))
    A, Bm, S = np.zeros((K, C), dtype=dtype), np.zeros((K, C), dtype=dtype), np.zeros((N, C), dtype=dtype)
    for x in range(C):
        A[:, x] = (Q[:, x, None] * a).sum(axis=0, dtype=dtype)
        Bm[:, x] = (Q[:, x, None] * b).sum(axis=0, dtype=dtype)
        S[:, x] = (F[None, :, x] * a + Fb[None, :, x] * b).sum(axis=1, dtype=dtype)
    FA = F * A
    den = FA + Fb * Bm
    with np.errstate(divide="ignore", invalid="ignore"):
        Fn = np.where(den > 0, FA / den, F)
        n = m.sum(axis=1, dtype=np.int64)
        Qn = np.where(n[:, None] > 0, Q * S / (P * n).astype(dtype)[:, None], Q)
    Qn, Fn = project(Qn, Fn)
    return Qn, Fn, ll


def start(N, K, C, init_seed=1):
    """(Q, F) float32: the start of a fit (module text)."""
    rng = np.random.default_rng(init_seed)
    Q = rng.dirichlet(np.ones(C), N).astype(np.float32)
    F = rng.uniform(0.1, 0.9, (K, C)).astype(np.float32)
    return Q, F


class _HostOps:
    """What the driver asks of an arithmetic: the step, the float64 norm of a (Q, F) pair and the projection."""

    def __init__(self, c, P, dtype):
        self.c, self.P, self.dtype = c, P, dtype

    def take(self, Q, F):
        return Q.astype(self.dtype), F.astype(self.dtype)

    def step(self, Q, F):
        return step_host(self.c, self.P, Q, F, self.dtype)

    def norm(self, dQ, dF):
        return float(np.sqrt((dQ.astype(np.float64) ** 2).sum() + (dF.astype(np.float64) ** 2).sum()))

    def project(self, Q, F):
        return project(Q, F)

    def give(self, Q, F):
        return np.asarray(Q), np.asarray(F)


def extrapolate(ops, x0, x1, x2, alpha=None):
    """(xa, alpha): SQUAREM's point from three iterates, each a (Q, F) pair; alpha None = -max(1, |r| / |v|), -1 when |v| = 0."""
    r = (x1[0] - x0[0], x1[1] - x0[1])
    v = ((x2[0] - x1[0]) - r[0], (x2[1] - x1[1]) - r[1])
    if alpha is None:
        nr, nv = ops.norm(*r), ops.norm(*v)
        alpha = -1.0 if nv == 0 else -max(1.0, nr / nv)
    two, sq = 2.0 * alpha, alpha * alpha
    return ops.project((x0[0] - two * r[0]) + sq * v[0], (x0[1] - two * r[1]) + sq * v[1]), alpha


def _fit(ops, x0, n_alleles, accel, tol, max_rounds):
    """The driver of the module text over an arithmetic `ops`; x0 the start.  Returns the result dict before the relabelling."""
    if accel not in ACCELS:
        raise ValueError(f"accel = {accel!r}: must be one of {ACCELS}")
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError(f"tol = {tol}: must be finite and >= 0")
    if max_rounds < 1:
        raise ValueError(f"max_rounds = {max_rounds}: must be >= 1")
    threshold = tol * n_alleles
    history, steps, converged, before = [], 0, False, None
    t = 0
    while True:
        Q1, F1, ll0 = ops.step(*x0)
        steps += 1
        if t >= 1 and ll0 - before < threshold:
            converged = True
            break
        if t == max_rounds:
            break
        before = ll0
        if accel == "none":
            history.append((t, ll0, 1))
            x0 = (Q1, F1)
        else:
            Q2, F2, ll1 = ops.step(Q1, F1)
            xa, _ = extrapolate(ops, x0, (Q1, F1), (Q2, F2))
            Q3, F3, lla = ops.step(*xa)
            steps += 2
            accepted = bool(lla >= ll1)
            history.append((t, ll0, int(accepted)))
            x0 = (Q3, F3) if accepted else (Q2, F2)
        t += 1
    history.append((t, ll0, None))
    return {"x": x0, "ll": float(ll0), "rounds": t, "steps": steps, "converged": converged, "history": history}


def relabel(Q, F):
    """(Q, F, order): the clusters renumbered by descending sum_i Q_ic (float64), ties to the lower index."""
    order = np.argsort(-np.asarray(Q, dtype=np.float64).sum(axis=0), kind="stable")
    return np.ascontiguousarray(Q[:, order]), np.ascontiguousarray(F[:, order]), order


def n_alleles(c, P):
    """P sum_i n_i: the allele copies with a call."""
    return int(P) * int((np.asarray(c) >= 0).sum())


def _finish(res, ops):
    Q, F = ops.give(*res.pop("x"))
    res["Q"], res["F"], res["order"] = relabel(Q, F)
    return res


def fit_host(c, P, C, init_seed=1, accel="squarem", tol=1e-7, max_rounds=200, dtype=np.float64):
    """The fit by step_host in `dtype`: a dict of Q [N][C], F [K][C] (relabelled, in `dtype`), ll, rounds, steps, converged,
    history = [(round, ll0, accepted)] with accepted None on the closing line, order (the relabelling)."""
    c = B.check_counts(c, P)
    ops = _HostOps(c, P, dtype)
    return _finish(_fit(ops, ops.take(*start(c.shape[0], c.shape[1], C, init_seed)), n_alleles(c, P), accel, tol, max_rounds), ops)


# ---------------------------------------------------------------- the device forms

class _DeviceOps:
    """The arithmetic of the device: loc_admix_step on tensors that stay there; the extrapolation and projection are torch
    elementwise operations, the norms float64 torch sums.  A step reads one double back."""

    def __init__(self, c, P, C, k_groups=0, pitch=None, pad_fill=-1, device="cuda:0", fill=None):
        import torch
        from . import _device as D, _lib
        self.torch, self.D, self.lib, self.check = torch, D, _lib.load(), _lib.check
        c = np.ascontiguousarray(c, dtype=np.int8)
        self.N, self.K = c.shape
        self.P, self.C, self.k_groups, self.device, self.fill = int(P), int(C), int(k_groups), device, fill
        buf = B.padded(c, pitch, pad_fill)
        self.pitch = int(buf.shape[1])
        with torch.cuda.device(device):
            self.d_c = D.put(buf, np.int8, device)
            self.work, self.work_bytes = D.work_buffer(self.lib, "loc_admix_work_bytes", self.N, self.K, self.C, self.k_groups,
                                                       device=device)
            self.d_ll = torch.empty(1, dtype=torch.float64, device=device)

    def take(self, Q, F):
        return (self.D.put(np.reshape(Q, (self.N, self.C)), np.float32, self.device),
                self.D.put(np.reshape(F, (self.K, self.C)), np.float32, self.device))

    def step(self, Q, F):
        t = self.torch
        with t.cuda.device(self.device):
            Qn = t.empty((max(self.N, 1), self.C), dtype=t.float32, device=self.device)[:self.N]
            Fn = t.empty((max(self.K, 1), self.C), dtype=t.float32, device=self.device)[:self.K]
            self.D.prefill((self.work, Qn, Fn, self.d_ll), self.fill)    # tests: what scratch and the outputs hold before
            Q, F = Q.contiguous(), F.contiguous()
            self.check(self.lib.loc_admix_step(self.d_c.data_ptr(), self.N, self.K, self.pitch, self.P, self.C, Q.data_ptr(),
                                               F.data_ptr(), Qn.data_ptr(), Fn.data_ptr(), self.d_ll.data_ptr(), self.k_groups,
                                               self.work.data_ptr(), self.work_bytes, self.D.stream()), "loc_admix_step")
            return Qn, Fn, float(self.d_ll.item())

    def norm(self, dQ, dF):
        return float(((dQ.double() ** 2).sum() + (dF.double() ** 2).sum()).sqrt().item())

    def project(self, Q, F):
        t = self.torch
        hi = float(np.float32(1) - np.float32(EPS))
        F = t.clamp(F, float(np.float32(EPS)), hi)
        Q = t.clamp_min(Q, float(np.float32(EPS)))
        s = Q[:, 0].clone()
        for x in range(1, self.C):
            s = s + Q[:, x]
        return Q / s[:, None], F

    def give(self, Q, F):
        return Q.cpu().numpy(), F.cpu().numpy()


def step_device(c, P, Q, F, k_groups=0, pitch=None, pad_fill=-1, device="cuda:0", fill=None):
    """step_host's answer from one loc_admix_step launch: (Q' float32, F' float32, ll).  fill: a 32-bit pattern that scratch,
    Q_out, F_out and ll hold before the launch (tests)."""
    c = np.ascontiguousarray(c, dtype=np.int8)
    Q = np.asarray(Q, dtype=np.float32)
    ops = _DeviceOps(c, P, Q.shape[1], k_groups, pitch, pad_fill, device, fill)
    Qn, Fn, ll = ops.step(*ops.take(Q, F))
    return Qn.cpu().numpy(), Fn.cpu().numpy(), ll


def fit_device(c, P, C, init_seed=1, accel="squarem", tol=1e-7, max_rounds=200, k_groups=0, device="cuda:0"):
    """fit_host's dict from loc_admix_step launches; Q, F and the three iterates of a round stay on the device, the host reads
    the three ll of a round and the two norms."""
    c = B.check_counts(c, P)
    ops = _DeviceOps(c, P, C, k_groups, device=device)
    return _finish(_fit(ops, ops.take(*start(c.shape[0], c.shape[1], C, init_seed)), n_alleles(c, P), accel, tol, max_rounds), ops)


# ---------------------------------------------------------------- placement

def _design(Q, rows):
    return np.concatenate([np.ones((len(rows), 1)), Q[rows][:, :-1]], axis=1)


def placements(Q, locs, located):
    """xy [N][2] of the module text, or None with fewer than C + 1 located samples.  The hat matrix comes from the singular
    vectors of the design, directions below the rank tolerance dropped (two clusters no located sample tells apart)."""
    Q = np.asarray(Q, dtype=np.float64)
    locs = np.asarray(locs, dtype=np.float64)
    located = np.asarray(located, dtype=bool)
    li, ui = np.flatnonzero(located), np.flatnonzero(~located)
    if len(li) < Q.shape[1] + 1:
        return None
    y = locs[li]
    X = _design(Q, li)
    U, s, Vt = np.linalg.svd(X, full_matrices=False)
    keep = s > s[0] * max(X.shape) * np.finfo(np.float64).eps
    U = U[:, keep]
    coef = U.T @ y
    fitted = U @ coef
    hii = (U * U).sum(axis=1)
    out = np.full((len(Q), 2), np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        loo = (fitted - hii[:, None] * y) / (1.0 - hii)[:, None]
    loo[1.0 - hii < 1e-9] = np.nan
    out[li] = loo
    if len(ui):
        out[ui] = _design(Q, ui) @ ((Vt[keep].T / s[keep][None]) @ coef)
    return out


# ---------------------------------------------------------------- the command's work

def admix(c, P, samples, locs, out=None, pops=3, accel="squarem", tol=1e-7, max_rounds=200, init_seed=1, longlat=False,
          keep_frequencies=False, host=False, silence=False, device="cuda:0", sites=None, extra=None):
    """The command's work for a count matrix: returns the summary dict and writes the output files when `out` is given.
    locs None: no locations were given.  extra: entries of the summary (--ld_prune: what baselines.prelude recorded)."""
    import pandas as pd
    c = B.check_counts(c, P)
    N, K = c.shape
    samples = np.asarray(samples).astype(str)
    if not 2 <= pops <= MAX_POPS:
        raise SystemExit(f"{PROG}: --pops must be 2 .. {MAX_POPS}")
    if pops > N:
        raise SystemExit(f"{PROG}: --pops {pops} with {N} samples: at most one cluster a sample")
    if K == 0:
        raise SystemExit(f"{PROG}: no site is left after the filters: nothing to fit")
    if not (np.isfinite(tol) and tol >= 0):
        raise SystemExit(f"{PROG}: --tol must be finite and >= 0")
    if max_rounds < 1:
        raise SystemExit(f"{PROG}: --max_rounds must be >= 1")
    if accel not in ACCELS:
        raise SystemExit(f"{PROG}: --accel must be one of {', '.join(ACCELS)}")
    if host:
        res = fit_host(c, P, pops, init_seed, accel, tol, max_rounds)
    else:
        B.require_gpu(PROG, LAUNCH)
        res = fit_device(c, P, pops, init_seed, accel, tol, max_rounds, device=device)
    Q, F = res["Q"].astype(np.float64), res["F"]
    alleles = n_alleles(c, P)

    xy, shared, lines = None, {"N": int(N), "K": int(K), "P": int(P)}, []
    if locs is not None:
        locs = np.asarray(locs, dtype=np.float64).reshape(N, 2)
        located = ~np.isnan(locs).any(axis=1)
        xy = placements(Q, locs, located)
        if xy is None:
            lines.append(f"{int(located.sum())} located samples for {pops} clusters: fewer than C + 1, no placement is made")
        else:
            shared, lines = B.placement_summary(c, P, located, xy, locs, longlat, "Q-regression")
    own = {"C": int(pops), "rounds": int(res["rounds"]), "steps": int(res["steps"]), "converged": bool(res["converged"]),
           "ll": B.num(res["ll"]), "ll_per_allele": B.num(res["ll"] / alleles) if alleles else None, "tol": float(tol),
           "accel": accel, "init_seed": int(init_seed), "cluster_sizes": [float(v) for v in Q.sum(axis=0)]}
    summary = {**{k: shared[k] for k in (HEAD if "n_located" in shared else ("N", "K", "P"))}, **{k: own[k] for k in OWN}}
    summary.update(extra or {})
    summary["path"] = "host" if host else "device"
    lines = [f"{N} samples, {K} sites, ploidy {P}: {pops} clusters after {res['rounds']} rounds ({res['steps']} steps, "
             f"{'converged' if res['converged'] else 'not converged'}), ll {res['ll']!r} ({own['ll_per_allele']!r} per allele)",
             "cluster sizes: " + ", ".join(f"{v:.2f}" for v in own["cluster_sizes"]), *lines]

    if out is not None:
        write_atomic(out + "_admix_Q.txt", "sampleID\t" + "\t".join(f"q{x + 1}" for x in range(pops)) + "\n" + "".join(
            f"{samples[i]}\t" + "\t".join(repr(float(v)) for v in Q[i]) + "\n" for i in range(N)))
        write_atomic(out + "_admix_history.txt", "round\tll\taccepted\n" + "".join(
            f"{t}\t{float(ll)!r}\t{'NA' if acc is None else acc}\n" for t, ll, acc in res["history"]))
        write_atomic(out + "_admix_summary.json", json.dumps(summary, indent=1) + "\n")
        if xy is not None:
            frame = pd.DataFrame({"x": xy[:, 0], "y": xy[:, 1], "sampleID": samples.astype(object)})
            write_atomic(out + "_admix_locs.txt", lambda fh: frame.to_csv(fh, index=False))
        if keep_frequencies:
            idx = np.arange(K, dtype=np.int64) if sites is None else np.asarray(sites, dtype=np.int64)
            write_atomic(out + "_admix_frequencies.npz", lambda fh: B.save_npz(fh, idx=idx, F=F, samples=samples), mode="wb")
    if not silence:
        for line in lines:
            print(line)
    summary["_Q"], summary["_F"], summary["_xy"], summary["_history"] = Q, F, xy, res["history"]
    return summary


# ---------------------------------------------------------------- command

def _own_arguments(p):
    p.add_argument("--pops", default=3, type=int, help=f"ancestral clusters C (default 3, 2 .. {MAX_POPS})")
    p.add_argument("--accel", default="squarem", choices=ACCELS, help="squarem (default): three EM steps and an extrapolation a "
                                                                      "round; none: one EM step a round")
    p.add_argument("--tol", default=1e-7, type=float, help="stop when a round gains less than TOL per called allele copy in "
                                                           "log-likelihood (default 1e-7)")
    p.add_argument("--max_rounds", default=200, type=int, help="rounds at most (default 200)")
    p.add_argument("--init_seed", default=1, type=int, help="seed of the random start (default 1; --seed drives --max_SNPs)")
    p.add_argument("--longlat", default=False, action="store_true",
                   help="x / y are longitude / latitude degrees: errors are great-circle km (the regression stays planar)")
    p.add_argument("--keep_frequencies", default=False, action="store_true",
                   help="keep the clusters' allele-1 frequencies, the site indices and the sample IDs in {out}_admix_frequencies.npz")
    p.add_argument("--host", default=False, action="store_true",
                   help="the NumPy form in float64 instead of the GPU (the files differ as the module text says)")


def build_parser():
    return B.build_parser(PROG, "Model-based ancestry proportions and a Q-regression placement baseline.", _own_arguments,
                          sample_data=False, sample_data_help="tab-separated sampleID, x, y; NaN / NA = to be placed.  Optional: "
                                                              "without it no placement is made")


def main(argv=None):
    parser = build_parser()
    a = B.parse_args(parser, argv)
    if not 2 <= a.pops <= MAX_POPS:
        parser.error(f"--pops must be 2 .. {MAX_POPS}")
    if not (np.isfinite(a.tol) and a.tol >= 0):
        parser.error("--tol must be finite and >= 0")
    if a.max_rounds < 1:
        parser.error("--max_rounds must be >= 1")
    c, P, samples, locs, idx = B.prelude(parser, a, LAUNCH)
    try:
        admix(c, P, samples, locs, a.out, a.pops, a.accel, a.tol, a.max_rounds, a.init_seed, a.longlat, a.keep_frequencies, a.host,
              a.silence, sites=idx, extra=getattr(a, "ld_summary", None))
    except ValueError as e:
        raise SystemExit(f"{PROG}: {e}") from None
    return 0


if __name__ == "__main__":
    sys.exit(main())
