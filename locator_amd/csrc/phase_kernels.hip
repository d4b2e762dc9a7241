// The diploid copying model of the phase command (locator_amd/phase.py): loc_phase_viterbi, defined in
// include/locator_hip_phase.h; the NumPy form phase.viterbi_host(float32) is what tests/test_gpu_phase.py holds it to, bit for
// bit.  Plain vector code: every operation fp32, rounded on its own (no contraction), denormals kept, quotients correctly rounded.
//
// One wave (a workgroup of its own) runs one recipient sample: K dependent site steps over the SP x SP states (d1, d2).  Lane =
// d1; the lane's SP values v(d1, .) live in registers.  SP = 16, 32 or 64 by S; the slots past S are invalid and hold exact zeros.
// v is symmetric bit for bit, so R(d) = max_d' v(d, d') is a lane-local maximum and also the column maximum; the 64 values go
// through one 256-byte row of LDS, which every lane reads back whole (broadcast reads).  G and its flat index come from one
// butterfly over (value, index) that prefers the lower index.
// phase_kernel, in order:
//   the donor columns and D;
//   the forward pass over all sites: ll, and v after every `block`-th site into the recipient's checkpoints;
//   for the blocks from the last to the first: the block's sites recomputed from its checkpoint by the same ph_step, which now
//   writes the back-pointers of a site (a lane: the 2-bit codes of its SP states, arg(d1) and G's pair of the site before), then
//   the traceback over the block.  All lanes follow the path; a lane reads back only the words it wrote itself, and the lane that
//   owns d1 supplies the code by a shuffle.  What the traceback reads at a site does not depend on the path, so the site before is
//   requested ahead.
#include "common.h"
#include "pair_tiles.h"

#include "../../include/locator_hip_phase.h"

#include <cmath>
#include <cstdint>
#include <type_traits>
#include <vector>

#pragma clang fp contract(off)

// Timing ablations (tools/phase_bench.py; `make variant F=phase_kernels XDEF=-DPH_ABLATE=<bits> TAG=ph<bits>`): the results are
// WRONG by construction, only the time counts.  1: no traceback; 2: no recomputation and no traceback (the forward pass alone);
// 4: no log (ll is wrong).
#ifndef PH_ABLATE
#define PH_ABLATE 0
#endif

constexpr int PH_LL_RUN = 8;            // sites whose m_j are multiplied in double before one log is taken: m_j >= 2.4e-18

template <int SP>
struct ph_geo {
    static constexpr int NW = SP / 16;                          // dwords of 2-bit codes a lane and site
    static constexpr int64_t CK = (int64_t)SP * 64;             // floats of a checkpoint
    static constexpr int64_t BP = 64 * (NW + 1);                // dwords of a site's back-pointers: the codes, then a word a lane
};

struct ph_state {                       // beside v: what a step needs of the site before
    float Rme, G;                       // R(lane), max R
    int arg, gflat;                     // arg(lane); G's pair as d1 * 64 + d2
};

// R, arg of the lane's row, the row of all R in LDS, G and its lowest flat index
template <int SP>
__device__ __forceinline__ void ph_summary(const float (&v)[SP], float* sR, int lane, ph_state& st) {
    float Rn = v[0];
    int an = 0;
#pragma unroll
    for (int d = 1; d < SP; ++d)
        if (v[d] > Rn) {
            Rn = v[d];
            an = d;
        }
    __syncthreads();                                            // every lane has read the row of the site before
    sR[lane] = Rn;
    __syncthreads();
    float g = Rn;
    int gi = lane * 64 + an;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float og = __shfl_xor(g, d, 64);
        const int oi = __shfl_xor(gi, d, 64);
        if (og > g || (og == g && oi < gi)) {
            g = og;
            gi = oi;
        }
    }
    st.Rme = Rn;
    st.arg = an;
    st.G = g;
    st.gflat = gi;
}

// One site in place: v_(j-1) -> v_j; returns m_j.  BP: the site's back-pointers go to `bp`.  x: the allele of the lane's donor
// (any value where the lane's slot is invalid), a0, a1: the recipient's; valid: the valid slots, a bit a slot.
template <int SP, bool BP>
__device__ __forceinline__ float ph_step(float (&v)[SP], ph_state& st, float* sR, int lane, int x, int a0, int a1, uint64_t valid,
                                         float r, float u, float th, float omt, uint32_t* __restrict__ bp) {
    constexpr int NW = ph_geo<SP>::NW;
    const float om = 1.0f - r, ru = r * u, t = om + ru;
    const float tt = t * t, tr = t * ru, rr = ru * ru;
    const float cG = rr * st.G;
    const bool me = (valid >> lane) & 1u;
    const uint64_t m1 = __ballot(me && x == 1) & valid, m0 = __ballot(me && x == 0) & valid, mm = __ballot(me && x < 0) & valid;
    // the lane's row of the emission table: against a donor allele 0, 1, missing
    const float qx0 = x < 0 ? 0.5f : (x == 0 ? omt : th), qx1 = x < 0 ? 0.5f : (x == 1 ? omt : th);
    float e0, e1, em;
    if (a0 < 0 || a1 < 0) {
        e0 = e1 = em = 1.0f;
    } else if (a0 + a1 == 0) {
        e0 = qx0 * omt; e1 = qx0 * th; em = qx0 * 0.5f;
    } else if (a0 + a1 == 2) {
        e0 = qx1 * th; e1 = qx1 * omt; em = qx1 * 0.5f;
    } else {
        e0 = qx1 * omt + qx0 * th; e1 = qx1 * th + qx0 * omt; em = qx1 * 0.5f + qx0 * 0.5f;
    }
    if (!me) e0 = e1 = em = 0.0f;

    uint32_t codes[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) codes[w] = 0u;
    float Mx = 0.0f;
    const float4* rows = reinterpret_cast<const float4*>(sR);
#pragma unroll
    for (int q = 0; q < SP / 4; ++q) {
        const float4 R4 = rows[q];
        const float Rq[4] = {R4.x, R4.y, R4.z, R4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int d2 = 4 * q + i;
            const float R2 = Rq[i];
            const float e = ((m1 >> d2) & 1u) ? e1 : ((m0 >> d2) & 1u) ? e0 : ((mm >> d2) & 1u) ? em : 0.0f;
            float best = tt * v[d2];
            uint32_t code = 0u;
            const float b = tr * (st.Rme >= R2 ? st.Rme : R2);
            if (b > best) {
                best = b;
                code = st.Rme >= R2 ? 1u : 2u;
            }
            if (cG > best) {
                best = cG;
                code = 3u;
            }
            const float nv = e * best;
            v[d2] = nv;
            Mx = nv > Mx ? nv : Mx;
            if (BP) codes[d2 / 16] |= code << (2 * (d2 % 16));
        }
    }
    if (BP) {                                                   // before the summary below replaces arg and G's pair
        uint32_t* mine = bp + (int64_t)lane * NW;
        if constexpr (NW == 4) *reinterpret_cast<uint4*>(mine) = make_uint4(codes[0], codes[1], codes[2], codes[3]);
        else if constexpr (NW == 2) *reinterpret_cast<uint2*>(mine) = make_uint2(codes[0], codes[1]);
        else mine[0] = codes[0];
        bp[64 * NW + lane] = (uint32_t)st.arg | ((uint32_t)st.gflat << 8);
    }
    float m = Mx;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float o = __shfl_xor(m, d, 64);
        m = o > m ? o : m;
    }
    const float inv = 1.0f / m;
#pragma unroll
    for (int d = 0; d < SP; ++d) v[d] = v[d] * inv;
    ph_summary<SP>(v, sR, lane, st);
    return m;
}

template <int SP>
__device__ __forceinline__ void ph_store_v(float* __restrict__ ck, int lane, const float (&v)[SP]) {
#pragma unroll
    for (int q = 0; q < SP / 4; ++q)
        *reinterpret_cast<float4*>(ck + ((int64_t)q * 64 + lane) * 4) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

template <int SP>
__device__ __forceinline__ void ph_load_v(const float* __restrict__ ck, int lane, float (&v)[SP]) {
#pragma unroll
    for (int q = 0; q < SP / 4; ++q) {
        const float4 f = *reinterpret_cast<const float4*>(ck + ((int64_t)q * 64 + lane) * 4);
        v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
    }
}

// the alleles a step reads at site j: the lane's donor's, the recipient's two
__device__ __forceinline__ void ph_alleles(const int8_t* __restrict__ h, int64_t j, int64_t pitch, int dcol, int c0, int& x, int& a0,
                                           int& a1) {
    const int8_t* row = h + j * pitch;
    x = dcol >= 0 ? (int)row[dcol] : -1;
    a0 = row[c0];
    a1 = row[c0 + 1];
}

// the sites lo .. hi - 1 forward.  CKPT: the forward pass (returns ll; v after every B-th site into `out`); else the
// recomputation (the back-pointers of site j into row j - lo of `out`)
template <int SP, bool CKPT>
__device__ __forceinline__ double ph_run(const int8_t* __restrict__ h, int64_t pitch, int dcol, int c0, int lane,
                                         const float* __restrict__ rho, int64_t lo, int64_t hi, int64_t K, int64_t B, float (&v)[SP],
                                         ph_state& st, float* sR, uint64_t valid, float u, float th, float omt, void* out) {
    double ll = 0.0, run = 1.0;
    int64_t since = 0, slot = 0;
    int x, a0, a1, xn, a0n, a1n;
    ph_alleles(h, lo, pitch, dcol, c0, x, a0, a1);
    for (int64_t j = lo; j < hi; ++j) {
        ph_alleles(h, j + 1 < hi ? j + 1 : j, pitch, dcol, c0, xn, a0n, a1n);
        const float rj = j == 0 ? 1.0f : rho[j];
        if (CKPT) {
            const float m = ph_step<SP, false>(v, st, sR, lane, x, a0, a1, valid, rj, u, th, omt, nullptr);
            run = run * (double)m;
            if (j % PH_LL_RUN == PH_LL_RUN - 1 || j == K - 1) {
                ll = ll + ((PH_ABLATE & 4) ? run : log(run));
                run = 1.0;
            }
            if (++since == B && j + 1 < K) {                    // v_j with j + 1 = (slot + 1) B: what block slot + 1 starts from
                ph_store_v<SP>((float*)out + slot * ph_geo<SP>::CK, lane, v);
                ++slot;
                since = 0;
            }
        } else {
            ph_step<SP, true>(v, st, sR, lane, x, a0, a1, valid, rj, u, th, omt, (uint32_t*)out + (j - lo) * ph_geo<SP>::BP);
        }
        x = xn; a0 = a0n; a1 = a1n;
    }
    return ll;
}

// what the traceback reads at site j: the lane's own back-pointer words, its donor's allele, the recipient's two
template <int SP>
struct ph_back {
    uint32_t codes[ph_geo<SP>::NW], aux;
    int x, a0, a1;
};

template <int SP>
__device__ __forceinline__ void ph_load_back(const uint32_t* __restrict__ bp, const int8_t* __restrict__ h, int64_t j, int64_t pitch,
                                             int dcol, int c0, int lane, ph_back<SP>& k) {
    constexpr int NW = ph_geo<SP>::NW;
    const uint32_t* mine = bp + (int64_t)lane * NW;
    if constexpr (NW == 4) {
        const uint4 q = *reinterpret_cast<const uint4*>(mine);
        k.codes[0] = q.x; k.codes[1] = q.y; k.codes[2] = q.z; k.codes[3] = q.w;
    } else if constexpr (NW == 2) {
        const uint2 q = *reinterpret_cast<const uint2*>(mine);
        k.codes[0] = q.x; k.codes[1] = q.y;
    } else {
        k.codes[0] = mine[0];
    }
    k.aux = bp[64 * NW + lane];
    ph_alleles(h, j, pitch, dcol, c0, k.x, k.a0, k.a1);
}

template <int SP>
__global__ __launch_bounds__(64) void phase_kernel(const int8_t* __restrict__ h, int64_t K, int64_t pitch, const int32_t* __restrict__ rec,
                                                   const int32_t* __restrict__ don, int S, const float* __restrict__ rho, float theta,
                                                   int64_t B, int8_t* __restrict__ first, int64_t first_pitch, double* __restrict__ ll,
                                                   int32_t* __restrict__ n_switch, int32_t* __restrict__ n_tied,
                                                   int32_t* __restrict__ n_donors, float* __restrict__ work, int64_t per_rec) {
    using geo = ph_geo<SP>;
    __shared__ __attribute__((aligned(16))) float sR[64];
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x;
    const int c0 = 2 * rec[i];
    const int dcol = lane < S ? don[i * S + lane] : -1;
    const uint64_t valid = __ballot(dcol >= 0);
    const int D = __popcll(valid);
    int8_t* const out = first + i * first_pitch;
    if (lane == 0) n_donors[i] = D;
    if (D == 0) {
        for (int64_t j = lane; j < K; j += 64) out[j] = h[j * pitch + c0];
        if (lane == 0) {
            ll[i] = 0.0;
            n_switch[i] = 0;
            n_tied[i] = 0;
        }
        return;
    }
    const float u = 1.0f / (float)D, th = theta, omt = 1.0f - theta;
    const bool me = (valid >> lane) & 1u;
    const int64_t nb = (K + B - 1) / B;
    float* const ck = work + i * per_rec;                        // nb - 1 checkpoints of CK floats
    uint32_t* const bps = reinterpret_cast<uint32_t*>(ck + (nb - 1) * geo::CK);     // B sites of BP dwords

    float v[SP];
    ph_state st;
    auto start = [&]() {                                        // v_(-1): 1 at the pairs of valid slots
#pragma unroll
        for (int d = 0; d < SP; ++d) v[d] = (me && ((valid >> d) & 1u)) ? 1.0f : 0.0f;
        ph_summary<SP>(v, sR, lane, st);
    };
    start();
    const double L = ph_run<SP, true>(h, pitch, dcol, c0, lane, rho, 0, K, K, B, v, st, sR, valid, u, th, omt, ck);
    if (lane == 0) ll[i] = L;
    if (PH_ABLATE & 2) return;

    int c1 = 0, c2 = 0, switches = 0, tied = 0;                  // the path's state at the site in hand, the same in every lane
    for (int64_t k = nb - 1; k >= 0; --k) {
        const int64_t lo = k * B, hi = lo + B < K ? lo + B : K;
        if (k == 0) {
            start();
        } else {
            ph_load_v<SP>(ck + (k - 1) * geo::CK, lane, v);
            ph_summary<SP>(v, sR, lane, st);
        }
        ph_run<SP, false>(h, pitch, dcol, c0, lane, rho, lo, hi, K, B, v, st, sR, valid, u, th, omt, bps);
        if (PH_ABLATE & 1) continue;
        if (k == nb - 1) {                                      // the end state: the lowest flat index of max v_(K-1)
            c1 = st.gflat >> 6;
            c2 = st.gflat & 63;
        }
        ph_back<SP> now, next;
        ph_load_back<SP>(bps + (hi - 1 - lo) * geo::BP, h, hi - 1, pitch, dcol, c0, lane, next);
        for (int64_t j = hi - 1; j >= lo; --j) {
            now = next;
            const int64_t jp = j > lo ? j - 1 : j;
            ph_load_back<SP>(bps + (jp - lo) * geo::BP, h, jp, pitch, dcol, c0, lane, next);
            int f = now.a0;
            if (now.a0 >= 0 && now.a1 >= 0 && now.a0 + now.a1 == 1) {
                const int x = __shfl(now.x, c1, 64), y = __shfl(now.x, c2, 64);
                const float qx0 = x < 0 ? 0.5f : (x == 0 ? omt : th), qx1 = x < 0 ? 0.5f : (x == 1 ? omt : th);
                const float qy0 = y < 0 ? 0.5f : (y == 0 ? omt : th), qy1 = y < 0 ? 0.5f : (y == 1 ? omt : th);
                const float p10 = qx1 * qy0, p01 = qx0 * qy1;
                if (p10 > p01) f = 1;
                else if (p10 < p01) f = 0;
                else ++tied;
            }
            if (lane == 0) out[j] = (int8_t)f;
            if (j > 0) {
                uint32_t word = now.codes[0];
#pragma unroll
                for (int w = 1; w < geo::NW; ++w) word = (c2 >> 4) == w ? now.codes[w] : word;
                const int code = __shfl((int)((word >> (2 * (c2 & 15))) & 3u), c1, 64);
                const int arg = (int)(now.aux & 255u);
                const int p1 = __shfl(arg, c1, 64), p2 = __shfl(arg, c2, 64);
                const int gf = (int)(now.aux >> 8);
                if (code == 1) {
                    c2 = p1;
                    switches += 1;
                } else if (code == 2) {
                    c1 = p2;
                    switches += 1;
                } else if (code == 3) {
                    c1 = gf >> 6;
                    c2 = gf & 63;
                    switches += 2;
                }
            }
        }
    }
    if (lane == 0) {
        n_switch[i] = switches;
        n_tied[i] = tied;
    }
}

// ---------------------------------------------------------------------------------------------------------------- launcher
static int ph_slots(int S) { return S <= 16 ? 16 : S <= 32 ? 32 : 64; }

static bool ph_sizes_ok(const char* who, int S, int64_t K, int R, int block) {
    if (S < LOC_PHASE_MIN_STATES || S > LOC_PHASE_MAX_STATES || K < 0 || K >= ((int64_t)1 << 31) || R < 0 || block < 0) {
        loc_set_error("%s: S=%d K=%lld R=%d block=%d (S %d .. %d: a lane a donor slot; K below 2^31; R and block not negative)", who, S,
                      (long long)K, R, block, LOC_PHASE_MIN_STATES, LOC_PHASE_MAX_STATES);
        return false;
    }
    return true;
}

struct ph_layout { int64_t B, per_rec, bytes; };
static ph_layout ph_work(int S, int64_t K, int R, int block) {
    ph_layout L = {0, 0, 0};
    if (R == 0 || K == 0) return L;
    const int SP = ph_slots(S);
    const int64_t ck = (int64_t)SP * 64, bp = 64 * (SP / 16 + 1);          // dwords of a checkpoint, of a site's back-pointers
    int64_t B = block;
    if (B == 0) {                                               // the least scratch: the best block of every block count tried
        int64_t least = K * bp;
        B = K;
        for (int64_t nb = 2; nb <= K && (nb - 1) * ck < least; ++nb) {
            const int64_t b = (K + nb - 1) / nb, cost = ((K + b - 1) / b - 1) * ck + b * bp;
            if (cost < least) {
                least = cost;
                B = b;
            }
        }
    }
    L.B = B < 1 ? 1 : B > K ? K : B;
    const int64_t nb = (K + L.B - 1) / L.B;
    L.per_rec = (nb - 1) * ck + L.B * bp;
    L.bytes = L.per_rec * R * 4;
    return L;
}

extern "C" int64_t loc_phase_work_bytes(int S, int64_t K, int R, int block) {
    if (!ph_sizes_ok("loc_phase_work_bytes", S, K, R, block)) return -1;
    return ph_work(S, K, R, block).bytes;
}

extern "C" int loc_phase_viterbi(const int8_t* h, int H, int64_t K, int64_t pitch, const int32_t* rec, int R, const int32_t* don, int S,
                                 const float* rho, float theta, int block, int8_t* first, int64_t first_pitch, double* ll,
                                 int32_t* n_switch, int32_t* n_tied, int32_t* n_donors, void* work, int64_t work_bytes, void* stream) {
    const char* who = "loc_phase_viterbi";
    hipStream_t s = (hipStream_t)stream;
    if (!ph_sizes_ok(who, S, K, R, block)) return -1;
    if (H < 2 || H % 2 != 0 || H >= (1 << 30) || pitch < H || pitch % 16 != 0 || first_pitch < K || work_bytes < 0) {
        loc_set_error("%s: H=%d pitch=%lld first_pitch=%lld work_bytes=%lld (H even, 2 .. 2^30 - 2; pitch >= H and a multiple of 16; "
                      "first_pitch >= K = %lld; work_bytes not negative)", who, H, (long long)pitch, (long long)first_pitch,
                      (long long)work_bytes, (long long)K);
        return -1;
    }
    if (!(theta >= 1e-7f && theta <= 0.5f)) {
        loc_set_error("%s: theta=%g (must be 1e-7 .. 0.5)", who, (double)theta);
        return -1;
    }
    if (R == 0) return 0;
    if (!rec || !don || !ll || !n_switch || !n_tied || !n_donors || (K > 0 && (!h || !rho || !first))) {
        loc_set_error("%s: null buffer", who);
        return -1;
    }
    if ((uintptr_t)ll % 8 != 0 || (uintptr_t)rec % 4 != 0 || (uintptr_t)don % 4 != 0 || (uintptr_t)rho % 4 != 0 ||
        (uintptr_t)n_switch % 4 != 0 || (uintptr_t)n_tied % 4 != 0 || (uintptr_t)n_donors % 4 != 0) {
        loc_set_error("%s: rec, don, rho, n_switch, n_tied and n_donors must be multiples of 4 bytes, ll of 8", who);
        return -1;
    }
    if (K > 0 && !pt_rows_aligned(who, h, pitch)) return -1;
    const ph_layout L = ph_work(S, K, R, block);
    if (!pt_work_ok(who, "loc_phase_work_bytes", work, work_bytes, L.bytes)) return -1;

    // rec and don read back and checked: one synchronisation of the stream
    std::vector<int32_t> h_rec((size_t)R), h_don((size_t)R * (size_t)S);
    hipError_t e = hipMemcpyAsync(h_rec.data(), rec, h_rec.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(h_don.data(), don, h_don.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        loc_set_error("%s: reading rec and don: %s", who, hipGetErrorString(e));
        return (int)e;
    }
    for (int i = 0; i < R; ++i) {
        const int32_t smp = h_rec[(size_t)i];
        if (smp < 0 || smp >= H / 2) {
            loc_set_error("%s: rec[%d] = %d is no sample (0 .. %d)", who, i, (int)smp, H / 2 - 1);
            return -1;
        }
        for (int d = 0; d < S; ++d) {
            const int32_t c = h_don[(size_t)i * (size_t)S + (size_t)d];
            if (c < -1 || c >= H) {
                loc_set_error("%s: don[%d][%d] = %d is no column (-1 = none, 0 .. %d)", who, i, d, (int)c, H - 1);
                return -1;
            }
            if (c == 2 * smp || c == 2 * smp + 1) {
                loc_set_error("%s: don[%d][%d] = %d is a column of the recipient sample %d itself", who, i, d, (int)c, (int)smp);
                return -1;
            }
        }
    }
    if (K == 0) {
        e = hipMemsetAsync(ll, 0, (size_t)R * sizeof(double), s);
        if (e == hipSuccess) e = hipMemsetAsync(n_switch, 0, (size_t)R * sizeof(int32_t), s);
        if (e == hipSuccess) e = hipMemsetAsync(n_tied, 0, (size_t)R * sizeof(int32_t), s);
        if (e == hipSuccess) e = hipMemsetAsync(n_donors, 0, (size_t)R * sizeof(int32_t), s);
        if (e != hipSuccess) {
            loc_set_error("%s: %s", who, hipGetErrorString(e));
            return (int)e;
        }
        return 0;
    }
    auto launch = [&](auto sp) {
        hipLaunchKernelGGL(phase_kernel<decltype(sp)::value>, dim3((unsigned)R), dim3(64), 0, s, h, K, pitch, rec, don, S, rho, theta, L.B,
                           first, first_pitch, ll, n_switch, n_tied, n_donors, (float*)work, L.per_rec);
    };
    switch (ph_slots(S)) {
        case 16: launch(std::integral_constant<int, 16>()); break;
        case 32: launch(std::integral_constant<int, 32>()); break;
        default: launch(std::integral_constant<int, 64>()); break;
    }
    e = hipGetLastError();
    if (e != hipSuccess) {
        loc_set_error("%s: %s", who, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}
