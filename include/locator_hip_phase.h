/* Entry points of liblocator_hip.so behind `python -m locator_amd.phase` (locator_amd/csrc/phase_kernels.hip): the diploid form of
 * the haplotype copying model of Li & Stephens, one most-likely pair of copying paths a recipient sample.  The spelling rules of
 * locator_hip.h hold (one declaration per `;`, comments only as this one), and locator_amd/_abi.py derives the ctypes binding
 * from this file with the same reader (LATER["phase"], and the LOC_PHASE_* constants).  As in locator_hip.h: device pointers
 * unless named h_*, `stream` a hipStream_t, 0 = success, -1 = bad arguments with loc_last_error set and nothing launched.  The
 * NumPy definition is locator_amd/phase.py: viterbi_host, which the device equals bit for bit in float32. */
#ifndef LOCATOR_HIP_PHASE_H
#define LOCATOR_HIP_PHASE_H
#include "locator_hip.h"

#define LOC_PHASE_MAX_STATES 64   /* most donor slots S of a recipient: lane = first slot, a value a second slot in registers */
#define LOC_PHASE_MIN_STATES 2

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the first haplotype of R recipient samples ----
 * h [K][pitch] int8, site-major: h[j][c] = allele of haplotype column c at site j, 0 or 1, or negative = missing (no value above
 * 1); column 2 s + a is allele a of sample s; columns H .. pitch - 1 are never interpreted.  H even, 2 <= H < 2^30, pitch >= H,
 * pitch a multiple of 16, h 16-byte aligned, K < 2^31.  rec [R] int32: the samples to phase, each 0 .. H / 2 - 1, in any order,
 * repeats allowed.  don [R][S] int32: the donor columns of recipient i, each -1 (none) or 0 .. H - 1 and none of the recipient's
 * own two columns; repeats allowed; LOC_PHASE_MIN_STATES <= S <= LOC_PHASE_MAX_STATES.  rho [K] float in [0, 1] (rho[0] is not
 * read: it counts as 1), 1e-7 <= theta <= 0.5.  The launcher reads rec and don back to check them: one synchronisation of
 * `stream` before the launch.
 * For recipient s = rec[i]: a slot d is valid where don[i][d] >= 0, D of them, u = 1 / D.  A state is an ordered pair (d1, d2) of
 * slots.  All in fp32, every operation rounded on its own (no fused multiply-add), denormals kept, the quotients correctly rounded:
 *   omt = 1 - theta; q(x, a) = omt where the donor allele x == a, theta where not, 0.5 where x < 0;
 *   g = the recipient's genotype at site j: missing where h[j][2s] < 0 or h[j][2s+1] < 0, else their sum; x, y the alleles of
 *   the donors of d1, d2:  e = q(x,0) q(y,0) for g = 0, q(x,1) q(y,1) for g = 2, q(x,1) q(y,0) + q(x,0) q(y,1) for g = 1,
 *   1 for g missing, and 0 where d1 or d2 is no valid slot.  e is symmetric in (d1, d2) bit for bit, and so is v.
 *   v_(-1) = 1 at pairs of valid slots, else 0.  R(d) = max_d' v(d, d') with arg(d) the lowest such d'; G = max_d R(d) at the
 *   lowest flat index d * S + arg(d).  Step j with r = rho_j (1 at j = 0), om = 1 - r, ru = r u, t = om + ru, tt = t t,
 *   tr = t ru, rr = ru ru:
 *     a = tt v(d1,d2) [stay], b = tr max(R(d1), R(d2)) [row where R(d1) >= R(d2): predecessor (d1, arg(d1)); else column:
 *     (arg(d2), d2)], c = rr G [both: the predecessor is G's pair];  best = a, then b if b > best, then c if c > best;
 *     v'(d1,d2) = e best;  m = max v';  v = v' (1 / m);  ll += log((double)m).
 *   The end state is the lowest flat index of max v_(K-1).  The traceback follows the predecessors; n_switch adds 1 for a row or
 *   column step and 2 for both, at the sites j >= 1.  At a site of the path (d1, d2) where g = 1, with x, y as above:
 *   p10 = q(x,1) q(y,0), p01 = q(x,0) q(y,1); first[i][j] = 1 if p10 > p01, 0 if p10 < p01, else h[j][2s] (and n_tied adds 1).
 *   Where g is not 1, first[i][j] = h[j][2s].
 * first [R][first_pitch] int8 (first_pitch >= K; bytes K .. first_pitch - 1 of a row are not written), ll [R] double, n_switch,
 * n_tied, n_donors [R] int32; row i belongs to rec[i].  No output may overlap an input.  A recipient with D = 0 gets its own first
 * alleles, ll = 0 and zeros and runs no recursion.
 * v is checkpointed every `block` sites by a forward pass (which also gives ll); then the blocks from the last to the first, each
 * recomputed from its checkpoint by the same step while its back-pointers (2 bits a state, arg(d) a slot, G's pair) are written,
 * then traced back: no result depends on `block`, bit for bit.  block 0 = the block with the least scratch (nb - 1) c + block p,
 * c and p the bytes of a checkpoint and of a site's back-pointers and nb = ceil(K / block) (near sqrt(K c / p); found by trying
 * every block count); a block above K counts as K.  One wave a recipient; no atomics; a lane reads back only scratch that it wrote itself in this launch; the
 * same arguments give the same bits, however the recipients are batched.
 * work: loc_phase_work_bytes(S, K, R, block) bytes (-1 on bad sizes), 16-byte aligned.
 * R = 0 or K = 0 launches nothing; K = 0 sets ll, n_switch, n_tied and n_donors to zeros (no recursion ran). */
int64_t loc_phase_work_bytes(int S, int64_t K, int R, int block);
int loc_phase_viterbi(const int8_t* h, int H, int64_t K, int64_t pitch, const int32_t* rec, int R, const int32_t* don, int S,
                      const float* rho, float theta, int block, int8_t* first, int64_t first_pitch, double* ll,
                      int32_t* n_switch, int32_t* n_tied, int32_t* n_donors, void* work, int64_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
