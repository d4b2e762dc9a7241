// Shared device helpers for the gfx950 kernels (wave = 64 lanes, MFMA f32 32x32x2).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/locator_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t fbits(float f) { return __builtin_bit_cast(uint32_t, f); }
__device__ __forceinline__ float bitsf(uint32_t u) { return __builtin_bit_cast(float, u); }
// dword = { top16(lo) in bits 0..15, top16(hi) in bits 16..31 }: two bf16 values from two fp32 by truncation
__device__ __forceinline__ uint32_t pack_top16(uint32_t lo, uint32_t hi) {
    return __builtin_amdgcn_perm(hi, lo, 0x07060302u);
}

#define BN_EPS 1e-3f
#define BN_MOMENTUM 0.99f
#define ADAM_C1 0.1f     /* (float)(1 - 0.9)   */
#define ADAM_C2 0.001f   /* (float)(1 - 0.999) */
#define ADAM_EPS 1e-7f
#define KT 32  // SNPs per k-tile of layer 1

// the top 16 bits of u + this = u rounded to bf16, nearest even
__device__ __forceinline__ uint32_t rne16(uint32_t u) { return u + 0x7FFFu + ((u >> 16) & 1u); }
// the 32-bit LDS address of a pointer into shared memory (operand of ds_read / M0 of an LDS-DMA)
__device__ __forceinline__ uint32_t lds_addr32(const void* p) {
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}

// Row of accumulator register r in lane-half hi for v_mfma_f32_32x32x2_f32:
// D[i][j]: j = lane & 31, i = rowmap(r, lane >> 5).
__device__ __forceinline__ int rowmap(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float elu_f(float z) { return z > 0.f ? z : expm1f(z); }
// ELU'(z) from the activation value a = ELU(z):  1 if z > 0 else e^z = a + 1
__device__ __forceinline__ float elu_grad_from_act(float a) { return a > 0.f ? 1.f : a + 1.f; }

// --dosage: the fixed-point form of a float dosage, q = rint(fp32(d) * 63) clamped to 0..126, -1 for NaN
// (missing).  A single fp32 product and a rounding - nothing for contraction to fuse - so it agrees bit for bit with
// genotypes.dosage_q.  ONE home: filter_kernels.hip (training windows) and query_kernels.hip (a kept model's query).
__device__ __forceinline__ int dosage_q_dev(float d) {
    if (d != d) return -1;                           // NaN: missing
    const float f = fminf(fmaxf(rintf(d * (float)LOC_DOSAGE_UNIT), 0.f), (float)(2 * LOC_DOSAGE_UNIT));
    return (int)f;
}

// Keras Adam: eps outside the root, bias correction folded into alpha.
__device__ __forceinline__ void adam_update(float& w, float& m, float& v, float g, float alpha) {
    m = m + (g - m) * ADAM_C1;
    v = v + (g * g - v) * ADAM_C2;
    w = w - (m * alpha) / (sqrtf(v) + ADAM_EPS);
}

// the same with v_sqrt_f32 / v_rcp_f32: 1 ulp each, i.e. < 4e-7 relative on an update that is <= lr
__device__ __forceinline__ void adam_update_fast(float& w, float& m, float& v, float g, float alpha) {
    m = m + (g - m) * ADAM_C1;
    v = v + (g * g - v) * ADAM_C2;
    w = w - (m * alpha) * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v) + ADAM_EPS);
}

__device__ __forceinline__ float adam_alpha(const float* alpha_tab, int alpha_tab_len, const float* lr,
                                            const int* t_base, int t_off) {
    int t = t_base[0] + t_off;
    if (t >= alpha_tab_len) t = alpha_tab_len - 1;
    return lr[0] * alpha_tab[t];
}

// gamma/beta Adam for SNP k from the per-wave partial sums left by l1_bwd_adam_kernel (fixed order: slot 0 +
// slot 1), and -- if next_stats is given -- the NEXT minibatch's [scale|shift|mean|rstd] from its precomputed
// batch statistics and the just-updated gamma/beta.  Shared by l1_gamma_beta_adam_kernel and the tail blocks of
// stack_dw_all_kernel.
__device__ __forceinline__ void gamma_beta_adam_body(int k, int Kp, const float* __restrict__ gbs,
                                                     float* __restrict__ gamma, float* __restrict__ beta,
                                                     float* __restrict__ m_gamma, float* __restrict__ v_gamma,
                                                     float* __restrict__ m_beta, float* __restrict__ v_beta,
                                                     float alpha, const float* __restrict__ next_stats,
                                                     float* __restrict__ bn4) {
    const float* g0 = gbs + (int64_t)(k >> 5) * 128 + (k & 31);
    const float dg = g0[0] + g0[64], db = g0[32] + g0[96];
    float wv = gamma[k], mv = m_gamma[k], vv = v_gamma[k];
    adam_update(wv, mv, vv, dg, alpha);
    const float g = wv;
    gamma[k] = wv; m_gamma[k] = mv; v_gamma[k] = vv;
    wv = beta[k]; mv = m_beta[k]; vv = v_beta[k];
    adam_update(wv, mv, vv, db, alpha);
    beta[k] = wv; m_beta[k] = mv; v_beta[k] = vv;
    if (next_stats) {
        const float mu = next_stats[k], rstd = 1.0f / sqrtf(next_stats[Kp + k] + BN_EPS);
        const float sc = g * rstd;
        bn4[k] = sc;
        bn4[Kp + k] = wv - mu * sc;
        bn4[2 * (int64_t)Kp + k] = mu;
        bn4[3 * (int64_t)Kp + k] = rstd;
    }
}

// =========================================================================================================
// Untracked vector-memory operations and hand-counted waits.  ONE home: l1_gemm.hip, l1_gemm_i8.hip, l1_chain.hip and
// stack_fused.hip use these and keep only their own count tables, next to the loops they count.
//
// Why: left to itself the compiler merges its per-register wait counts conservatively around a loop and then waits for
// the prefetch it has just issued before the first use of the CURRENT registers, so nothing overlaps (l1_gemm.hip saw
// vmcnt(2) where 9 loads may stay in flight, stack_fused.hip a full drain in front of every backward pass).  A load
// written as asm is neither counted nor waited for by the compiler; the waits below do that.  The "memory" clobbers keep
// these loads, the compiler's own stores and the waits in program order, which is what the counts rely on.
//
// COUNTING RULE (gfx9 has one counter for loads and stores): loads retire in order among loads and stores among stores,
// but a store may retire before an older load.  So "at most N outstanding" proves that a load has landed only if N is the
// number of LOADS that EVERY wave issues after it: stores never count, and neither do loads behind a condition.
//
// The compiler believes an asm output is valid at once.  Where forms below differ, that is why.
// ---------------------------------------------------------------------------------------------------------
// Workgroup barrier that orders LDS traffic only.  __syncthreads() would also drain vmcnt, i.e. wait for the prefetch
// that is deliberately kept in flight across it.  Legal where no thread reads another thread's GLOBAL writes, so that LDS
// ordering is all the barrier has to provide ("memory" keeps the compiler from moving accesses across it).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// ... FENCED: and nothing (MFMAs included) scheduled across it.  The two large-M GEMMs hand the matrix pipe from one
// group of waves to the other at this barrier.
__device__ __forceinline__ void lds_barrier_fenced() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
// this wave's LDS traffic done, without the barrier; bare (l1_gemm.hip's epilogue) and fenced (l1_gemm_i8.hip's loop)
__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void wait_lgkm0_fenced() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// ---- loads.  UNIFORM: 16 bytes at (wave-uniform base, in scalar registers) + (32-bit byte offset of the lane) + OFF: one
// offset register serves several arrays (W1, m and v in l1_chain.hip; every row of a ring slot in stack_fused.hip).
// NT = non-temporal.  The destination is a fresh definition ("=v"), so every such load is issued UNCONDITIONALLY (a dummy
// address where there is nothing to fetch): a load under a branch would meet "not loaded" in a phi, and a copy inserted
// for that phi would read the register before the data lands.  tests/test_chain_asm.py checks the generated code for
// exactly that.  In stack_fused.hip, that a ring register is never copied while its load is in flight follows from how
// the requests are placed, not from the constraint: every request is unconditional (one chain of definitions per
// register, nothing for the compiler to merge), and the readers of the old rows are ordered in front of the request
// (trip(): the sums pass through an asm statement), so the old value is dead where the new one is defined and both get
// the same register.  The ISA of every instantiation shows no move of a ring register; look again after any change here.
template <int OFF, bool NT = false>
__device__ __forceinline__ void gload16_uniform(f32x4& v, const void* base, uint32_t voff) {
    if (NT) asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3 nt" : "=v"(v) : "v"(voff), "s"(base), "n"(OFF) : "memory");
    else asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(v) : "v"(voff), "s"(base), "n"(OFF) : "memory");
}
// the base of such a request must be in scalar registers: a pointer that is the same in every lane, said so to the compiler
__device__ __forceinline__ const float* uniform_ptr(const float* p) {
    const uint64_t u = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
    return reinterpret_cast<const float*>(((uint64_t)hi << 32) | lo);
}
// LANE: 16 bytes at a per-lane 64-bit address (the large-M GEMM's genotype lines and weight fragments)
template <typename T>
__device__ __forceinline__ void gload16_lane(T& r, const void* p) {
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r) : "v"(p) : "memory");
}
// 4 bytes at a per-lane 64-bit address, FRESH definition ("=v"): unconditional loads only, as above (l1_chain.hip)
__device__ __forceinline__ void gload4_fresh(uint32_t& v, const void* p) {
    asm volatile("global_load_dword %0, %1, off" : "=v"(v) : "v"(p) : "memory");
}
// 4 bytes / 1 byte (zero-extended) at a per-lane address, IN-OUT.  Several of these sit behind a condition
// (stack_fused.hip), so the destination is an in-out operand ("+v") of an initialised variable: the load overwrites the
// register that holds the initial value, and there is no second value that a merge behind the condition could make the
// compiler copy while the load is in flight.  (By the counting rule such a load is never counted.)
template <class T>
__device__ __forceinline__ void gload4_inout(T& v, const void* p) {
    static_assert(sizeof(T) == 4, "one register");
    asm volatile("global_load_dword %0, %1, off" : "+v"(v) : "v"(p) : "memory");
}
__device__ __forceinline__ void gload1_inout(uint32_t& v, const void* p) {
    asm volatile("global_load_ubyte %0, %1, off" : "+v"(v) : "v"(p) : "memory");
}
// ---- the store that goes with gload16_uniform.
// The two wait states behind the store are part of it: on gfx940+ a vector-memory store of more than 8 bytes still reads its
// data registers for two wait states after it issues, and a vector-ALU write to them in that window corrupts what is
// stored.  The compiler's hazard recognizer pads its OWN stores; it cannot see into an asm statement, and once the data
// registers are dead after the asm it is free to reuse them at once - round 4's register allocation of the second step did
// (`v_pk_add_f32 v[24:25]` right behind `global_store_dwordx4 v142, v[22:25]`: wrong Adam moments in memory, right weights).
template <int OFF, bool NT>
__device__ __forceinline__ void gstore16_uniform(const f32x4& v, float* base, uint32_t voff) {
    if (NT) asm volatile("global_store_dwordx4 %0, %1, %2 offset:%3 nt\n\ts_nop 1" : : "v"(voff), "v"(v), "s"(base), "n"(OFF) : "memory");
    else asm volatile("global_store_dwordx4 %0, %1, %2 offset:%3\n\ts_nop 1" : : "v"(voff), "v"(v), "s"(base), "n"(OFF) : "memory");
}

// ---- waits: until at most N vector-memory operations of the wave are outstanding (N by the counting rule above).
// The drained twin: a -DLOC_DEBUG_DRAIN build (`make debug_drain`, liblocator_hip_drain.so) turns every hand count of
// every kernel into vmcnt(0); tests/test_gpu_chain.py, test_gpu_gemm_i8.py and test_gpu_stack_stream.py compare the two
// builds bit for bit.  This is the one place that reads the switch.
#ifdef LOC_DEBUG_DRAIN
#define LOC_VMCNT(N) 0
#else
#define LOC_VMCNT(N) (N)
#endif
#define LOC_VMCNT_FITS(N) static_assert((N) >= 0 && (N) <= 63, "vmcnt has six bits")
// BARE: asm volatile statements keep their order, so vm_landed(x) right behind it ties a register that the wait protects:
// every use of x depends on the tie, and none can be scheduled above the wait.
template <int N>
__device__ __forceinline__ void vm_wait() {
    LOC_VMCNT_FITS(N);
    asm volatile("s_waitcnt vmcnt(%0)" : : "n"(LOC_VMCNT(N)) : "memory");
}
template <class T>
__device__ __forceinline__ void vm_landed(T& x) { asm volatile("" : "+v"(x)); }
// FENCED: nothing at all scheduled across it (the large-M GEMMs, whose loaded registers feed MFMAs in fixed phases)
template <int N>
__device__ __forceinline__ void vm_wait_fenced() {
    LOC_VMCNT_FITS(N);
    asm volatile("s_waitcnt vmcnt(%0)" : : "n"(LOC_VMCNT(N)) : "memory");
    __builtin_amdgcn_sched_barrier(0);
}
// TYING: the operands are the registers the wait protects, so no use of them can be scheduled above it.
// SLOT: the one or four registers of a ring slot (stack_fused.hip)
template <int N>
__device__ __forceinline__ void vm_wait_slot(f32x4& a) {
    LOC_VMCNT_FITS(N);
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(a) : "n"(LOC_VMCNT(N)) : "memory");
}
template <int N>
__device__ __forceinline__ void vm_wait_slot(f32x4& a, f32x4& b, f32x4& c, f32x4& d) {
    LOC_VMCNT_FITS(N);
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(LOC_VMCNT(N)) : "memory");
}
// UNIT: every register an untracked load of a wave of l1_chain.hip may still be writing: the current unit's three register
// sets and the small-operand words of its 1, 2 or 4 loader roles.  One operand list per role count: an asm statement's
// operands cannot be a pack.
template <int N>
__device__ __forceinline__ void vm_wait_unit(f32x4 (&a)[4], f32x4 (&b)[4], f32x4 (&c)[4], uint32_t (&ld)[1][3]) {
    LOC_VMCNT_FITS(N);
    asm volatile("s_waitcnt vmcnt(%15)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]),
                   "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(ld[0][0]), "+v"(ld[0][1]), "+v"(ld[0][2])
                 : "n"(LOC_VMCNT(N))
                 : "memory");
}
template <int N>
__device__ __forceinline__ void vm_wait_unit(f32x4 (&a)[4], f32x4 (&b)[4], f32x4 (&c)[4], uint32_t (&ld)[2][3]) {
    LOC_VMCNT_FITS(N);
    asm volatile("s_waitcnt vmcnt(%18)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]),
                   "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(ld[0][0]), "+v"(ld[0][1]), "+v"(ld[0][2]),
                   "+v"(ld[1][0]), "+v"(ld[1][1]), "+v"(ld[1][2])
                 : "n"(LOC_VMCNT(N))
                 : "memory");
}
template <int N>
__device__ __forceinline__ void vm_wait_unit(f32x4 (&a)[4], f32x4 (&b)[4], f32x4 (&c)[4], uint32_t (&ld)[4][3]) {
    LOC_VMCNT_FITS(N);
    asm volatile("s_waitcnt vmcnt(%24)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]),
                   "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(ld[0][0]), "+v"(ld[0][1]), "+v"(ld[0][2]),
                   "+v"(ld[1][0]), "+v"(ld[1][1]), "+v"(ld[1][2]), "+v"(ld[2][0]), "+v"(ld[2][1]), "+v"(ld[2][2]),
                   "+v"(ld[3][0]), "+v"(ld[3][1]), "+v"(ld[3][2])
                 : "n"(LOC_VMCNT(N))
                 : "memory");
}
// =========================================================================================================

// ---- Philox4x32-10 counter RNG -------------------------------------------------
struct philox4 {
    uint32_t v[4];
};
__host__ __device__ inline philox4 philox4x32_10(uint64_t ctr_lo, uint64_t ctr_hi, uint64_t key) {
    uint32_t c0 = (uint32_t)ctr_lo, c1 = (uint32_t)(ctr_lo >> 32), c2 = (uint32_t)ctr_hi, c3 = (uint32_t)(ctr_hi >> 32);
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    for (int i = 0; i < 10; ++i) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    philox4 r;
    r.v[0] = c0; r.v[1] = c1; r.v[2] = c2; r.v[3] = c3;
    return r;
}

// W1S index of element (h, k): see include/locator_hip.h
__host__ __device__ inline int64_t w1s_index(int h, int k, int nht) {
    int kt = k >> 5, kl = k & 31, ht = h >> 5, hl = h & 31;
    int q = hl >> 3, hi = (hl >> 2) & 1, c = hl & 3;
    return ((int64_t)(kt * nht + ht) * 4 + q) * 256 + (hi * 32 + kl) * 4 + c;
}

// host-side error plumbing (api.hip)
void loc_set_error(const char* fmt, ...);
// l1_gemm.hip: the shift-term and SNP-group reductions shared by the bf16 and int8 large-M GEMMs
int gm_launch_cvec(const float* cpart, int nkt64, float* cvec8, void* stream);
int gm_launch_reduce(const float* partial, int G, int64_t MH, const float* cvec8, const float* b1, float* a1,
                     void* stream);

// stack_rows.hip: the hidden stack + heads for many rows on the fp32 matrix pipe (32 or 16 rows per workgroup: tile_rows, 0 = by row count)
int sr_eval_launch(const float* a1, const float* rd_partial, int rd_G, int64_t rd_MH, const float* rd_cvec8, const float* rd_b1,
                   const float* Wh, const float* bh, const float* wa, const float* ba, const float* wb, const float* bb, int L,
                   int n_b, const int32_t* rows, const float* Y, float* yhat, float* dist, int tile_rows, void* stream);
extern "C" int loc_stack_rows_min_rows(void);
int sr_compute_units();   // compute units of the current device (cached per device; 256 when there is none)
extern "C" int loc_stack_rows_supported(int Hp, int L);

// l1_kernels.hip: the layer-1 reduction alone (partial sums of G groups -> a1, optional Dropout on a1)
int loc_l1_reduce_launch_drop(const float* partial, int G, int rows_p, int Hp, const float* b1, float* a1, float* a1_drop,
                              const uint8_t* mask, float keep_scale, void* stream);

// Raises a kernel's dynamic-LDS limit.  The limit is an attribute of the function PER DEVICE, so the "largest value
// set so far" is remembered per (call site = kernel instantiation, device); the call is idempotent, which makes the
// unsynchronised cache benign.  FUNC may hold template commas: wrap it in parentheses.
#define LOC_MAX_DEVICES 64
#define LOC_ENSURE_LDS(FUNC, BYTES)                                                                          \
    do {                                                                                                     \
        static size_t set__[LOC_MAX_DEVICES] = {};                                                           \
        int dev__ = 0;                                                                                       \
        (void)hipGetDevice(&dev__);                                                                          \
        dev__ = dev__ < 0 ? 0 : dev__ % LOC_MAX_DEVICES;                                                     \
        if ((size_t)(BYTES) > set__[dev__]) {                                                                \
            hipError_t e__ = hipFuncSetAttribute(reinterpret_cast<const void*>(FUNC),                        \
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)(BYTES));  \
            if (e__ != hipSuccess) {                                                                         \
                loc_set_error("hipFuncSetAttribute(%zu): %s", (size_t)(BYTES), hipGetErrorString(e__));     \
                return (int)e__;                                                                             \
            }                                                                                                \
            set__[dev__] = (size_t)(BYTES);                                                                  \
        }                                                                                                    \
    } while (0)
// one launch per padded width: MACRO(NHT) for NHT = Hp / 32 = 1..32
#define NHT_SWITCH(NHT_VALUE, MACRO)                                                        \
    switch (NHT_VALUE) {                                                                    \
        case 1: MACRO(1); break;   case 2: MACRO(2); break;   case 3: MACRO(3); break;      \
        case 4: MACRO(4); break;   case 5: MACRO(5); break;   case 6: MACRO(6); break;      \
        case 7: MACRO(7); break;   case 8: MACRO(8); break;   case 9: MACRO(9); break;      \
        case 10: MACRO(10); break; case 11: MACRO(11); break; case 12: MACRO(12); break;    \
        case 13: MACRO(13); break; case 14: MACRO(14); break; case 15: MACRO(15); break;    \
        case 16: MACRO(16); break; case 17: MACRO(17); break; case 18: MACRO(18); break;    \
        case 19: MACRO(19); break; case 20: MACRO(20); break; case 21: MACRO(21); break;    \
        case 22: MACRO(22); break; case 23: MACRO(23); break; case 24: MACRO(24); break;    \
        case 25: MACRO(25); break; case 26: MACRO(26); break; case 27: MACRO(27); break;    \
        case 28: MACRO(28); break; case 29: MACRO(29); break; case 30: MACRO(30); break;    \
        case 31: MACRO(31); break; case 32: MACRO(32); break;                               \
        default: loc_set_error("%s: width %d unsupported (Hp must be 32..1024)", __func__, 32 * (NHT_VALUE)); return -1; \
    }
#define LOC_GRID_Y_MAX 32768 /* HIP limits grid.y to 65535: kernels launched with one y-block per row stride over it */
#define LOC_CHECK_LAUNCH()                                              \
    do {                                                                \
        hipError_t e__ = hipGetLastError();                             \
        if (e__ != hipSuccess) {                                        \
            loc_set_error("%s: %s", __func__, hipGetErrorString(e__));  \
            return (int)e__;                                            \
        }                                                               \
    } while (0)
