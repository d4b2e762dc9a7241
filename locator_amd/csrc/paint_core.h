// What the kernels of the haplotype copying model share: paint_kernel (paint_kernels.hip, loc_paint_copy), impute_kernel
// (impute_kernels.hip, loc_impute_dose) and local_kernel (local_kernels.hip, loc_paint_local).  The pk_* device functions are one forward step, the forward pass with its checkpoints
// and the recomputation of a block, with their loads and stores: the kernels run the same forward pass by the same
// operations, so ll and n_donors of the entry points are the same bits.  Behind them the launchers' common part: the sweeps
// of a column count, the scratch layout and the refusals.  include/locator_hip_paint.h states the arithmetic.
// Every operation fp32 and uncontracted except the fused multiply-adds that are written out: the pragma below holds for the
// including file too.
#pragma once
#include "common.h"
#include "pair_tiles.h"

#include "../../include/locator_hip_paint.h"

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#pragma clang fp contract(off)

// Timing ablations (tools/paint_bench.py, tools/impute_bench.py, tools/local_bench.py; `make variant F=paint_kernels XDEF=-DPK_ABLATE=<bits>
// TAG=pk<bits>`): the results are WRONG by construction, only the time counts.  1: no cross-lane sums; 2: no alleles read,
// constant emissions; 4: no scratch rows and checkpoints written or read; impute_kernels.hip only: 8: no dose stored (it is still
// formed), 16: every column counted as allele 0 and as allele 1 (no compare and select a value); local_kernels.hip only
// (tools/local_bench.py): 32: no contraction at a window's end (zeros are stored).
#ifndef PK_ABLATE
#define PK_ABLATE 0
#endif

constexpr int PK_X = LOC_PAINT_LANE_COLS;
constexpr int PK_SWEEP = 64 * PK_X;               // columns one dword of every lane covers
constexpr int PK_RUN = LOC_PAINT_LL_RUN;
constexpr int PK_CS = LOC_PAINT_C_SLOTS;
static_assert(PK_X == 4 && PK_CS == 64 && LOC_PAINT_MAX_HAPS == 16 * PK_SWEEP, "a dword of alleles a lane, at most 16 of them");

__device__ __forceinline__ float pk_lane4(const float (&s)[PK_X]) { return (s[0] + s[1]) + (s[2] + s[3]); }
__device__ __forceinline__ float pk_wave_sum(float v) {
    if (PK_ABLATE & 1) return v * 64.0f;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}

// the donors of a recipient of the individual `own` among the lane's columns, one bit a value of the lane; D: their number.
// paint_kernel spells the same loop out: behind this function the compiler schedules that kernel differently, and its code is
// held identical to what was measured (tools/isa_diff.py).
template <int NR>
__device__ __forceinline__ uint64_t pk_donor_mask(const uint8_t* __restrict__ donor, const int32_t* __restrict__ owner, int H, int own,
                                                  int lane, int& D) {
    uint64_t mask = 0;
    D = 0;
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int x = 0; x < PK_X; ++x) {
            const int d = PK_X * lane + PK_SWEEP * i + x;
            if (d < H && donor[d] != 0 && owner[d] != own) {
                mask |= (uint64_t)1 << (PK_X * i + x);
                ++D;
            }
        }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) D += __shfl_xor(D, d, 64);
    return mask;
}

// e_j of the four columns of the dword w against the recipient's allele ar; bits: which of the four are donors
__device__ __forceinline__ void pk_emit(uint32_t w, int ar, uint32_t bits, float th, float omt, float (&e)[PK_X]) {
#pragma unroll
    for (int x = 0; x < PK_X; ++x) {
        if (PK_ABLATE & 2) {
            e[x] = ((bits >> x) & 1u) ? omt : 0.0f;
            continue;
        }
        const int a = (int)(w << (24 - 8 * x)) >> 24;
        const float v = (a < 0 || ar < 0) ? 1.0f : (a == ar ? omt : th);
        e[x] = ((bits >> x) & 1u) ? v : 0.0f;
    }
}

template <int NR>
__device__ __forceinline__ void pk_load_alleles(const int8_t* __restrict__ h, int64_t j, int64_t pitch, int rc, int lane,
                                                uint32_t (&w)[NR], int& ar) {
    const int8_t* row = h + j * pitch;
    if (PK_ABLATE & 2) {
#pragma unroll
        for (int i = 0; i < NR; ++i) w[i] = 0u;
        ar = 0;
        return;
    }
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int64_t col = PK_X * lane + PK_SWEEP * i;       // pitch is a multiple of 16: a dword that starts inside ends inside
        w[i] = col < pitch ? *reinterpret_cast<const uint32_t*>(row + col) : 0xffffffffu;
    }
    ar = row[rc];
}

template <int NR>
__device__ __forceinline__ void pk_load_row(const float* __restrict__ row, int lane, float (&v)[NR][PK_X]) {
    if (PK_ABLATE & 4) {
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
            for (int x = 0; x < PK_X; ++x) v[i][x] = 0.001f;
        return;
    }
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const float4 q = *reinterpret_cast<const float4*>(row + PK_X * lane + PK_SWEEP * i);
        v[i][0] = q.x; v[i][1] = q.y; v[i][2] = q.z; v[i][3] = q.w;
    }
}

template <int NR>
__device__ __forceinline__ void pk_store_row(float* __restrict__ row, int lane, const float (&v)[NR][PK_X]) {
    if (PK_ABLATE & 4) return;
#pragma unroll
    for (int i = 0; i < NR; ++i)
        *reinterpret_cast<float4*>(row + PK_X * lane + PK_SWEEP * i) = make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
}

// one forward step in place: ah = a-hat_(j-1) -> a-hat_j; returns c_j.  The forward pass and the recomputation both run this.
template <int NR>
__device__ __forceinline__ float pk_forward(float (&ah)[NR][PK_X], const uint32_t (&w)[NR], int ar, uint64_t mask, float om, float ru,
                                            float th, float omt) {
    float s[PK_X] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        float e[PK_X];
        pk_emit(w[i], ar, (uint32_t)(mask >> (PK_X * i)) & 15u, th, omt, e);
#pragma unroll
        for (int x = 0; x < PK_X; ++x) {
            const float a = e[x] * __builtin_fmaf(om, ah[i][x], ru);
            ah[i][x] = a;
            s[x] = s[x] + a;
        }
    }
    const float c = pk_wave_sum(pk_lane4(s));
    const float inv = 1.0f / c;
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int x = 0; x < PK_X; ++x) ah[i][x] = ah[i][x] * inv;
    return c;
}

// the sites lo .. hi - 1 forward from ah.  CKPT: the forward pass (ll, a checkpoint after every B-th site, into `out`);
// else the recomputation (row j - lo of `out` = a-hat_j, c_j behind it)
template <int NR, bool CKPT>
__device__ __forceinline__ double pk_run(const int8_t* __restrict__ h, int64_t pitch, int rc, int lane, const float* __restrict__ rho,
                                         int64_t lo, int64_t hi, int64_t K, int64_t B, float (&ah)[NR][PK_X], uint64_t mask, float u,
                                         float th, float omt, float* __restrict__ out, int64_t stride) {
    uint32_t w[NR], wn[NR];
    int ar, arn;
    double ll = 0.0, run = 1.0;
    int64_t since = 0, slot = 0;                             // sites since the last checkpoint, checkpoints written
    pk_load_alleles<NR>(h, lo, pitch, rc, lane, w, ar);
    for (int64_t j = lo; j < hi; ++j) {
        pk_load_alleles<NR>(h, j + 1 < hi ? j + 1 : j, pitch, rc, lane, wn, arn);
        const float rj = j == 0 ? 1.0f : rho[j];
        const float c = pk_forward<NR>(ah, w, ar, mask, 1.0f - rj, rj * u, th, omt);
        if (CKPT) {
            run = run * (double)c;
            if (j % PK_RUN == PK_RUN - 1 || j == K - 1) {
                ll = ll + log(run);
                run = 1.0;
            }
            if (++since == B && j + 1 < K) {                 // a-hat_j with j + 1 = (slot + 1) B: what block slot + 1 starts from
                pk_store_row<NR>(out + slot * stride, lane, ah);
                ++slot;
                since = 0;
            }
        } else {
            float* row = out + (j - lo) * stride;
            pk_store_row<NR>(row, lane, ah);
            row[PK_SWEEP * NR + lane] = c;
        }
#pragma unroll
        for (int i = 0; i < NR; ++i) w[i] = wn[i];
        ar = arn;
    }
    return ll;
}

// ---------------------------------------------------------------------------------------------------- the launchers' common part
static int pk_sweeps(int H) {
    const int n = (H + PK_SWEEP - 1) / PK_SWEEP;
    return n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : 16;
}

static bool pk_sizes_ok(const char* who, int H, int64_t K, int R, int block) {
    if (H < 1 || H > LOC_PAINT_MAX_HAPS || K < 0 || K >= ((int64_t)1 << 31) || R < 0 || block < 0) {
        loc_set_error("%s: H=%d K=%lld R=%d block=%d (H 1 .. %d: more haplotypes do not fit a wave's registers; K below 2^31; R and "
                      "block not negative)", who, H, (long long)K, R, block, LOC_PAINT_MAX_HAPS);
        return false;
    }
    return true;
}

static int64_t pk_block(int64_t K, int block) {
    int64_t B = block;
    if (B == 0) {
        B = (int64_t)std::sqrt((double)K);
        while (B * B < K) ++B;
    }
    return B < 1 ? 1 : B > K ? K : B;
}

struct pk_layout { int64_t B, per_rec, bytes; };
static pk_layout pk_work(int H, int64_t K, int R, int block) {
    pk_layout L = {0, 0, 0};
    if (R == 0 || K == 0) return L;
    const int64_t HP = (int64_t)PK_SWEEP * pk_sweeps(H);
    L.B = pk_block(K, block);
    const int64_t nb = (K + L.B - 1) / L.B;
    L.per_rec = (nb - 1) * HP + L.B * (HP + PK_CS);
    L.bytes = L.per_rec * R * (int64_t)sizeof(float);
    return L;
}

// the refusals of sizes, pitch and theta, which come before R = 0 returns
static bool pk_args_ok(const char* who, int H, int64_t K, int R, int block, int64_t pitch, int64_t work_bytes, float theta) {
    if (!pk_sizes_ok(who, H, K, R, block)) return false;
    if (pitch < H || pitch % 16 != 0 || work_bytes < 0) {
        loc_set_error("%s: pitch=%lld work_bytes=%lld (pitch >= H = %d and a multiple of 16; work_bytes not negative)", who,
                      (long long)pitch, (long long)work_bytes, H);
        return false;
    }
    if (!(theta >= 1e-7f && theta <= 0.5f)) {
        loc_set_error("%s: theta=%g (must be 1e-7 .. 0.5)", who, (double)theta);
        return false;
    }
    return true;
}

// a device array that an entry point reads back beside rec, in rec's synchronisation (loc_paint_local: its windows)
struct pk_also { const void* src; void* dst; size_t bytes; };

// rec read back and checked (one synchronisation of the stream): 0, -1 for a recipient that is no column, or the HIP error
static int pk_rec_ok(const char* who, const int32_t* rec, int R, int H, hipStream_t s, const pk_also* also) {
    std::vector<int32_t> h_rec((size_t)R);
    hipError_t e = hipMemcpyAsync(h_rec.data(), rec, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && also) e = hipMemcpyAsync(also->dst, also->src, also->bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        loc_set_error("%s: reading rec: %s", who, hipGetErrorString(e));
        return (int)e;
    }
    for (int i = 0; i < R; ++i)
        if (h_rec[(size_t)i] < 0 || h_rec[(size_t)i] >= H) {
            loc_set_error("%s: rec[%d] = %d is no column (0 .. %d)", who, i, (int)h_rec[(size_t)i], H - 1);
            return -1;
        }
    return 0;
}

// What the two entry points take alike, and an output of a call's own: its name in the messages, where it is, and the bytes
// that K = 0 zeroes (0: none).
struct pk_call {
    const int8_t* h; int H; int64_t K, pitch; const uint8_t* donor; const int32_t* owner; const int32_t* rec; int R;
    const float* rho; float theta; int block; double* ll; int32_t* n_donors; void* work; int64_t work_bytes; hipStream_t stream;
};
struct pk_out { const char* name; void* p; size_t zero_bytes; };

// Every step of an entry point before its launch, in the order the header states: the refusals, R = 0, the scratch layout into
// L, rec read back, the zeros of K = 0.  true: launch.  false: the entry point returns rc (0: nothing left to do; -1 or the HIP
// error: refused, loc_set_error called).
static bool pk_enter(const char* who, const pk_call& c, const pk_out* outs, int n_outs, pk_layout& L, int& rc,
                     const pk_also* also = nullptr) {
    rc = -1;
    if (!pk_args_ok(who, c.H, c.K, c.R, c.block, c.pitch, c.work_bytes, c.theta)) return false;
    if (c.R == 0) {
        rc = 0;
        return false;
    }
    bool null = !c.ll || !c.n_donors || !c.rec || !c.donor || !c.owner || (c.K > 0 && (!c.h || !c.rho));
    bool odd = (uintptr_t)c.ll % 8 != 0 || (uintptr_t)c.n_donors % 4 != 0 || (uintptr_t)c.rho % 4 != 0 || (uintptr_t)c.owner % 4 != 0 ||
               (uintptr_t)c.rec % 4 != 0;
    std::string names;
    for (int i = 0; i < n_outs; ++i) {
        null = null || !outs[i].p;
        odd = odd || (uintptr_t)outs[i].p % 4 != 0;
        names += outs[i].name;
        names += ", ";
    }
    if (null) {
        loc_set_error("%s: null buffer", who);
        return false;
    }
    if (odd) {
        loc_set_error("%s: %sn_donors, rho, owner and rec must be multiples of 4 bytes, ll of 8", who, names.c_str());
        return false;
    }
    if (c.K > 0 && !pt_rows_aligned(who, c.h, c.pitch)) return false;
    L = pk_work(c.H, c.K, c.R, c.block);
    if (!pt_work_ok(who, "loc_paint_work_bytes", c.work, c.work_bytes, L.bytes)) return false;
    if ((rc = pk_rec_ok(who, c.rec, c.R, c.H, c.stream, also)) != 0) return false;
    if (c.K > 0) return true;
    hipError_t e = hipSuccess;
    for (int i = 0; i < n_outs && e == hipSuccess; ++i)
        if (outs[i].zero_bytes) e = hipMemsetAsync(outs[i].p, 0, outs[i].zero_bytes, c.stream);
    if (e == hipSuccess) e = hipMemsetAsync(c.ll, 0, (size_t)c.R * sizeof(double), c.stream);
    if (e == hipSuccess) e = hipMemsetAsync(c.n_donors, 0, (size_t)c.R * sizeof(int32_t), c.stream);
    if (e != hipSuccess) {
        loc_set_error("%s: %s", who, hipGetErrorString(e));
        rc = (int)e;
    }
    return false;
}

// f(std::integral_constant<int, NR>()) for the NR of H columns: the one switch over pk_sweeps
template <class F>
static void pk_dispatch(int H, F&& f) {
    switch (pk_sweeps(H)) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 4: return f(std::integral_constant<int, 4>());
        case 8: return f(std::integral_constant<int, 8>());
        default: return f(std::integral_constant<int, 16>());
    }
}

// after pk_dispatch: 0, or the HIP error of the launch under the name `who`
static int pk_launched(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    loc_set_error("%s: %s", who, hipGetErrorString(e));
    return (int)e;
}
